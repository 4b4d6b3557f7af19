// K1's long exp table and short weight chain (k_assemble_mfma, float64 weights): the table's layout in LDS, the limit below
// which a chunk of keypoints may take the short chain, and both chains as plain host and device functions, so that
// tools/exp_long_check.cpp can compare them on the CPU bit for bit (fract, fma, ldexp, the conversion and max are IEEE
// operations: the host's results are the device's).
//
// The full chain (exp_neg_scaled, then the clamp), with T[i] the correctly rounded 2^(i / 512), i = 0 .. 511 (kExp2Tab):
//     n = (int)(-yu);  f = fract(yu);  w2 = max(ldexp(T[n & 511] * poly(f), n >> 9), gamma2)
// For 0 <= yu < kExpLong, j = floor(yu) = -n, the scaling is by 2^0, 2^-1 or 2^-2: exact, so it can be applied to the table
// entry instead of the product, tab3[j] = ldexp(T[(-j) & 511], (-j) >> 9) = 2^(-j / 512), and where tab3[j] * poly(f) >
// gamma2 the max returns its first operand.  The short chain is then
//     n = (int)(-yu);  f = fract(yu);  w2 = E[n] * (poly(f) / 2),   E[-j] = 2 tab3[j]
// with poly / 2 evaluated by halved coefficients (every Horner step is the full chain's, scaled by a power of two: the same
// mantissas).  Why twice tab3 and why indexed downwards: E[-j] = T[512 - j] for j = 1 .. 512 - the table the FULL chain
// reads, in its place - so one LDS array serves both bodies of the kernel,
//     s[kExpLong]:  s[kExpLongZero + i] = T[i], i = 0 .. 511;  s[kExpLongZero + 512] = 2 (j = 0);
//                   s[kExpLongZero - k] = T[512 - k] / 2, k = 1 .. kExpLongZero (j = 512 + k)
// and the entry of j is s[kExpLong - 1 - j]: one shift-and-add from n.
#pragma once

#include <cmath>

#if defined(__HIP__)
#define APAP_EXP_HD __host__ __device__
#else
#define APAP_EXP_HD
#endif

namespace apap {

constexpr int kExpTabN = 512;                           // entries of T (kExpN)
constexpr int kExpLong = 768;                           // entries of s: j = floor(yu) in [0, kExpLong)
constexpr int kExpLongZero = kExpLong - kExpTabN - 1;   // where T[0] sits in s
static_assert(kExpLong % 64 == 0 && kExpLong > kExpTabN && kExpLong <= kExpTabN + kExpTabN / 2,
              "the entries beyond T come from T's upper half (one per thread of a block of 256)");

// Entry `a` of s, from T.
APAP_EXP_HD inline double exp_long_entry(const double *T, int a) {
    const int i = a - kExpLongZero;
    return i < 0 ? 0.5 * T[kExpTabN + i] : i < kExpTabN ? T[i] : 2.0;
}

constexpr double kExpLn2N = 0x1.62e42fefa39efp-1 / kExpTabN;   // ln2 / 512
// poly(f) scaled by `h` (1 or 1/2): exp(-f ln2 / 512), degree 4
APAP_EXP_HD inline double exp_long_poly(double f, double h) {
    constexpr double L = kExpLn2N;
    double p = fma(f, h * (L * L * L * L / 24), h * -(L * L * L / 6));
    p = fma(f, p, h * (L * L / 2));
    p = fma(f, p, h * -L);
    return fma(f, p, h);
}
// The two chains from yu on, on the host: `s` is the long table.  (The device's forms are exp_neg_scaled / exp_neg_short in
// apap_kernels.hip; these are the same operations in the same order.)
inline double exp_chain_full(double yu, const double *s, double gamma2) {
    const double m = -yu;       // (int)(-yu) as v_cvt_i32_f64 does it: truncating, saturating, NaN -> 0
    const int n = m != m ? 0 : m <= -2147483648.0 ? (int)(-2147483647 - 1) : m >= 2147483647.0 ? 2147483647 : (int)m;
    const double f = yu - std::floor(yu);
    const double t = s[kExpLongZero + (n & (kExpTabN - 1))];
    return std::fmax(std::ldexp(t * exp_long_poly(f, 1.0), n >> 9), gamma2);
}
inline double exp_chain_short(double yu, const double *s) {     // for 0 <= yu < kExpLong only
    const int n = (int)(-yu);
    const double f = yu - std::floor(yu);
    return s[kExpLong - 1 + n] * exp_long_poly(f, 0.5);
}

// The limit: a keypoint whose scaled distance yu to every cell of a block is below it takes the short chain.
//   ylim = (1 - 2^-20) min(kExpLong, Y),  Y = -512 log2(gamma2), the yu at which 2^(-yu / 512) meets the clamp;
//   0 (never) for gamma2 >= 1 or not finite, and for Y < 2^-10, where the margin would be thinner than the chain's roundings.
// The margin covers the roundings between the bound that is checked and the chain's own yu (differences, two fused steps, a
// square root within one ulp, one product: a few 2^-53) with thirty bits to spare, and it makes the clamp idle strictly:
// yu <= (1 - 2^-20) Y gives 2^(-yu / 512) >= gamma2 (1 + Y ln2 2^-29) >= gamma2 (1 + 2^-40), against a chain within 2^-50.
inline double exp_long_limit(double gamma2) {
    const double margin = 1.0 - 0x1p-20;
    if (!(gamma2 >= 0.0) || !(gamma2 < 1.0)) return 0.0;
    if (gamma2 == 0.0) return margin * kExpLong;
    const double Y = -512.0 * std::log2(gamma2);
    if (!(Y >= 0x1p-10)) return 0.0;
    return margin * (Y < (double)kExpLong ? Y : (double)kExpLong);
}

}  // namespace apap
