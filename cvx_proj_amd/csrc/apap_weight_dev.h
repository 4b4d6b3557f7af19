// The moving-DLT weight of one keypoint for one cell, shared by apap_kernels.hip (K2's careful path, the weight tensor) and
// apap_local_model.hip (the robust moving DLT): one definition, hence the same bits wherever a weight is computed.
// Needs -ffp-contract=off like every kernel source: each fused multiply-add is written fma().
#pragma once
#include <hip/hip_runtime.h>

namespace {

// weight of one keypoint for one cell: max(exp(-|v - s| / sigma^2), gamma), float64 like
// apap.py:150-152 (np.sqrt and np.exp on float64).
//
// sqrt and exp are the device library's algorithms (v_rsq_f64 + Goldschmidt with two
// residual corrections; Cody-Waite reduction + degree-11 polynomial + v_ldexp_f64, same
// constants and operation order, hence the same bits) with their range guards replaced
// by what this call site needs: 10 + 18 instructions instead of 17 + 22.
//   * d2 is clamped below at 1e-300 instead of special-casing 0: sqrt gives 1e-150 and
//     exp(-1e-150/sigma^2) == 1.0 exactly, the value for distance 0.
//   * the exponent argument is clamped at -1100 (exp underflows to 0 there).
//   * inf/NaN coordinates are not propagated as NaN (the reference would produce NaN
//     matrices for them).
__device__ __forceinline__ double sqrt_pos(double x) {
    const double y = __builtin_amdgcn_rsq(x);
    double g = x * y;
    double h = y * 0.5;
    const double r = fma(-h, g, 0.5);
    g = fma(g, r, g);
    h = fma(h, r, h);
    double d = fma(-g, g, x);
    g = fma(d, h, g);
    d = fma(-g, g, x);
    return fma(d, h, g);
}

__device__ __forceinline__ double exp_nonpos(double x) {
    x = fmax(x, -1100.0);
    const double n = __builtin_rint(x * 0x1.71547652b82fep+0);       // log2(e)
    double r = fma(n, -0x1.62e42fefa39efp-1, x);                        // -ln2 high
    r = fma(n, -0x1.abc9e3b39803fp-56, r);                              // -ln2 low
    double p = fma(r, 0x1.ade156a5dcb37p-26, 0x1.28af3fca7ab0cp-22);
    p = fma(r, p, 0x1.71dee623fde64p-19);
    p = fma(r, p, 0x1.a01997c89e6b0p-16);
    p = fma(r, p, 0x1.a01a014761f6ep-13);
    p = fma(r, p, 0x1.6c16c1852b7b0p-10);
    p = fma(r, p, 0x1.1111111122322p-7);
    p = fma(r, p, 0x1.55555555502a1p-5);
    p = fma(r, p, 0x1.5555555555511p-3);
    p = fma(r, p, 0x1.000000000000bp-1);
    p = fma(r, p, 1.0);
    p = fma(r, p, 1.0);
    return __builtin_ldexp(p, (int)n);
}

__device__ __forceinline__ double cell_weight(double vx, double vy, double sx, double sy,
                                              double inv_sigma, double gamma) {
    const double dx = vx - sx;
    const double dy = vy - sy;
    const double d2 = fmax(dx * dx + dy * dy, 1e-300);
    const double dist = sqrt_pos(d2);
    const double w = exp_nonpos(-(dist * inv_sigma));
    return fmax(w, gamma);
}

}  // namespace
