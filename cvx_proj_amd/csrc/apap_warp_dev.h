// The device functions with which K3 turns a canvas pixel into a source pixel, shared by apap_kernels.hip (k_warp,
// k_warp_rows, k_warp_fast) and apap_panorama.hip (k_panorama): one definition, hence the same bits wherever a pixel of
// local_warp is computed.  Needs -ffp-contract=off like every kernel source: each fused multiply-add is written fma().
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "apap_internal.h"

namespace {

// 12 bytes to ANY byte address with the non-temporal hint (global_store_dwordx3 ... nt)
__device__ __forceinline__ void store12_stream(uint8_t *p, unsigned a, unsigned b, unsigned c) {
    typedef unsigned Dwords3 __attribute__((ext_vector_type(3)));
    typedef Dwords3 Dwords3AnyByte __attribute__((aligned(1)));
    const Dwords3 v = {a, b, c};
    __builtin_nontemporal_store(v, reinterpret_cast<Dwords3AnyByte *>(p));
}

// target coordinate of canvas pixel (i, j) through the (already inverted) cell matrix:
// float64 FMA chain in the order h0*x + h1*y + h2, then the two divisions by the third
// component (apap.py:172-184,211-213: float32 H^-1 promoted to float64 by the int64
// point).  The two quotients share one reciprocal (v_rcp_f64 + two Newton steps) and get
// one residual correction each - the Markstein sequence, which returns the correctly
// rounded quotient the reference's true division produces (checked against the oracle's
// coordinates in tests: equal).
struct Hinv9 {
    double2 a, b, c, d, e;  // h0 h1 | h2 h3 | h4 h5 | h6 h7 | h8 -
};

__device__ __forceinline__ Hinv9 load_hinv(const double *__restrict__ hinv_pad, unsigned cell) {
    // unsigned 32-bit byte offset: lets the load use the scalar-base + 32-bit-offset form
    const double2 *p = reinterpret_cast<const double2 *>(reinterpret_cast<const char *>(hinv_pad) +
                                                         (size_t)(cell * (unsigned)(APAP_HINV_STRIDE * sizeof(double))));
    Hinv9 h;
    h.a = p[0]; h.b = p[1]; h.c = p[2]; h.d = p[3]; h.e = p[4];
    return h;
}

__device__ __forceinline__ Hinv9 select_hinv(bool first, const Hinv9 &x, const Hinv9 &y) {
    Hinv9 h;
    h.a = first ? x.a : y.a; h.b = first ? x.b : y.b; h.c = first ? x.c : y.c;
    h.d = first ? x.d : y.d; h.e.x = first ? x.e.x : y.e.x; h.e.y = 0.0;
    return h;
}

__device__ __forceinline__ void target_from(const Hinv9 &h, double x, double y, double &tx, double &ty) {
    const double t0 = fma(h.b.x, 1.0, fma(h.a.y, y, h.a.x * x));
    const double t1 = fma(h.c.y, 1.0, fma(h.c.x, y, h.b.y * x));
    const double t2 = fma(h.e.x, 1.0, fma(h.d.y, y, h.d.x * x));
    double r = __builtin_amdgcn_rcp(t2);
    r = fma(fma(-t2, r, 1.0), r, r);
    r = fma(fma(-t2, r, 1.0), r, r);
    const double q0 = t0 * r, q1 = t1 * r;
    tx = fma(fma(-t2, q0, t0), r, q0);
    ty = fma(fma(-t2, q1, t1), r, q1);
}

__device__ __forceinline__ void target_of(const double *__restrict__ hinv_pad, int cell, double x,
                                          double y, double &tx, double &ty) {
    target_from(load_hinv(hinv_pad, (unsigned)cell), x, y, tx, ty);
}

// What a lane keeps per pixel while its strip stays in one cell row: the three products with
// the pixel's x (the first terms of the reference's sums, apap.py:172-184) and the other six
// coefficients.
struct PixelH {
    double p0, p1, p2;  // h0 x, h3 x, h6 x
    double h1, h2, h4, h5, h7, h8;
};

__device__ __forceinline__ PixelH pixel_h(const Hinv9 &h, double x) {
    PixelH q;
    q.p0 = h.a.x * x; q.p1 = h.b.y * x; q.p2 = h.d.x * x;
    q.h1 = h.a.y; q.h2 = h.b.x; q.h4 = h.c.x; q.h5 = h.c.y; q.h7 = h.d.y; q.h8 = h.e.x;
    return q;
}

// the 3 bytes at byte offset `o` of the source as a 24-bit value; 0 for the "outside" marker 0xffffffff.
// Reads the dword at the pixel's first byte; for the image's very last pixel the dword one byte earlier,
// shifted (v_alignbyte_b32), so that no byte beyond the image is touched.
__device__ __forceinline__ unsigned gather_px(const uint8_t *__restrict__ img, unsigned o, unsigned last) {
    unsigned int v;
    const unsigned oc = o < last ? o : last;
    __builtin_memcpy(&v, img + oc, 4);
    v = __builtin_amdgcn_alignbyte(0u, v, o - oc);
    // v & 0xffffff & ~sign(o): v_bfe_i32 + v_bitop3_b32 (truth table a & b & ~c = 0x40)
    return (unsigned)__builtin_amdgcn_bitop3_b32((int)v, 0x00ffffff, __builtin_amdgcn_sbfe((int)o, 31u, 1u), 0x40);
}

}  // namespace
