// The per-pixel steps of the warp kernels, each defined ONCE: the same bits wherever a pixel of local_warp is computed, and one
// place to change them.  Needs -ffp-contract=off like every kernel source: each fused multiply-add is written fma().
//   matrices      load_hinv, select_hinv; target_from / target_of: the exact coordinate with TWO Newton steps, used per pixel by
//                 k_warp, k_warp_coords and k_warp_fast's exact_offset (apap_kernels.hip)
//   strips        pixel_h, strip_cell_row, strip_source, strip_offset: a cell row's matrices for a lane's four pixels and the
//                 exact coordinate with ONE Newton step, used by k_warp_rows and k_panorama (strip_offset also by k_warp_fast)
//   gather        gather_px: one source pixel from a byte offset or the outside marker (k_warp_rows, k_warp_fast, k_panorama)
//   bilinear      strip_source_xy (strip_source with the coordinate handed back), fixed_coord, bilinear_taps, gather_tap(s),
//                 bilinear_blend: APAP_SAMPLING_BILINEAR's per-pixel steps (k_warp_bilinear, apap_warp_bilinear.hip, and
//                 k_panorama's bilinear forms)
//   stitch        blend_center: centre paste + uniform_blend of one pixel (k_warp, k_warp_rows, k_warp_fast)
//   tables        warp_stamp, warp_tables_ready: the stamp of a workspace's lookup tables (every gather kernel)
//   store         store12_stream, APAP_STORE_PX4: four pixels as one 12-byte non-temporal store, or a partial group byte by byte
//                 (every kernel above and k_image_warp, apap_image_warp.hip)
// The two exact sequences stay apart; each is pinned by its own tests.  Their three sums are the same bits: fma(h, 1.0, s) is
// the correctly rounded h + s, which is what `s + h` is.  Their quotients are NOT shown equal from the arithmetic: with one
// Newton step the quotient's error before its final rounding is ~2^-92, with two it is smaller still, and the quotient of two
// doubles can lie closer than that to the midpoint of two neighbouring doubles, where the two forms may round apart.  Either
// form gives the oracle's coordinate wherever the tests compare them.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "apap_internal.h"

namespace {

// 12 bytes to ANY byte address with the non-temporal hint (global_store_dwordx3 ... nt): a canvas is written once and never
// read back by the kernel that writes it - the bytes stream past the L2 instead of waiting in it, dirty, for the write-back at
// the end of the kernel (tools/k3_policy.hip: of the eight sc0 / sc1 / nt combinations on the stores and the eight on the
// gathers, nt stores + plain loads is the fastest; K3 at C3 16.0 -> 15.1 us warm, 19.3 -> 17.5 us cold)
__device__ __forceinline__ void store12_stream(uint8_t *p, unsigned a, unsigned b, unsigned c) {
    typedef unsigned Dwords3 __attribute__((ext_vector_type(3)));
    typedef Dwords3 Dwords3AnyByte __attribute__((aligned(1)));
    const Dwords3 v = {a, b, c};
    __builtin_nontemporal_store(v, reinterpret_cast<Dwords3AnyByte *>(p));
}

// The first `npx` (1 .. 4) of a lane's four 24-bit pixels p[0 .. 3] to `o`.  A whole group: 4 x 24 bits -> 3 dwords with one
// shift-or and two byte permutes (v_perm_b32 picks bytes 0-3 from its second operand, 4-7 from its first); groups start at
// any byte: an unaligned, non-temporal 12-byte store.  A partial group (the end of a row or of the canvas) byte by byte, never
// past it.  A macro, not a function: as a function, even a forced-inline one, hipcc optimises the byte loop on its own before it
// meets the strip's pixel array, and the strip kernels come out with another tail (80-130 instructions more per strip row, or
// with a loop pragma against that, the 8-row k_warp_fast with its gathers in another order: 2 % slower at 32 C5 pairs per
// launch, profiles/warp_shared_steps.txt).  Expanded in the kernel the strip kernels compile to the instructions they had
// with the text written out in each.
#define APAP_STORE_PX4(o_, p_, npx_)                                                                                     \
    do {                                                                                                                 \
        uint8_t *const apap_o = (o_);                                                                                    \
        const int apap_n = (npx_);                                                                                       \
        if (apap_n == 4) {                                                                                               \
            store12_stream(apap_o, (p_)[0] | ((p_)[1] << 24), __builtin_amdgcn_perm((p_)[2], (p_)[1], 0x05040201u),      \
                           __builtin_amdgcn_perm((p_)[3], (p_)[2], 0x06050402u));                                        \
        } else {                                                                                                         \
            for (int apap_k = 0; apap_k < apap_n; ++apap_k) {                                                            \
                apap_o[3 * apap_k] = (uint8_t)((p_)[apap_k] & 0xff);                                                     \
                apap_o[3 * apap_k + 1] = (uint8_t)(((p_)[apap_k] >> 8) & 0xff);                                          \
                apap_o[3 * apap_k + 2] = (uint8_t)(((p_)[apap_k] >> 16) & 0xff);                                         \
            }                                                                                                            \
        }                                                                                                                \
    } while (0)

// The stamp of the sizes a warp workspace's lookup tables were built for (the word behind the lut; apap_kernels.hip describes
// it at warp_stamp16), and the test every gather kernel makes before it uses a table value as an index.
__host__ __device__ __forceinline__ int warp_stamp(int mesh_rows, int mesh_cols, int final_w, int final_h) {
    return (int)(((unsigned)mesh_rows * 0x9E3779B1u) ^ ((unsigned)mesh_cols * 0x85EBCA77u) ^ ((unsigned)final_w * 0xC2B2AE3Du) ^
                 ((unsigned)final_h * 0x27D4EB2Fu)) | 1;
}
__device__ __forceinline__ bool warp_tables_ready(int have, int mesh_rows, int mesh_cols, int final_w, int final_h, int *status) {
    if (__builtin_expect(have == warp_stamp(mesh_rows, mesh_cols, final_w, final_h), 1)) return true;
    if ((threadIdx.x & 63) == 0) atomicOr(status, APAP_STATUS_UNPREPARED);
    return false;
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

// The matrices of one cell row (its first cell is `base`) for a lane's four pixels, whose cell columns are col[] and whose
// x are xs[]: the cells of the first and the last pixel; the two in between almost always sit in one of those (cell columns
// are monotone along a row and cells are wider than 2 px), otherwise a third load.
__device__ __forceinline__ void strip_cell_row(const double *__restrict__ hinv_pad, int base, const int (&col)[4],
                                               const double (&xs)[4], PixelH (&q)[4]) {
    const Hinv9 ha = load_hinv(hinv_pad, (unsigned)(base + col[0]));
    const Hinv9 hb = load_hinv(hinv_pad, (unsigned)(base + col[3]));
    q[0] = pixel_h(ha, xs[0]);
    q[3] = pixel_h(hb, xs[3]);
#pragma unroll
    for (int k = 1; k < 3; ++k) {
        const bool is_a = col[k] == col[0];
        Hinv9 hk = select_hinv(is_a, ha, hb);
        if (!is_a && col[k] != col[3]) hk = load_hinv(hinv_pad, (unsigned)(base + col[k]));  // a third cell
        q[k] = pixel_h(hk, xs[k]);
    }
}

// The exact source pixel (ix, iy) of a canvas pixel whose y relative to the centre is yd; false: outside the source (ix, iy
// are then whatever the conversions gave).
__device__ __forceinline__ bool strip_source(const PixelH &q, double yd, int img_w, int img_h, int &ix, int &iy) {
    // (h0 x + h1 y) + h2 and so on: the order of the reference's matrix-vector product
    const double t0 = fma(q.h1, yd, q.p0) + q.h2;
    const double t1 = fma(q.h4, yd, q.p1) + q.h5;
    const double t2 = fma(q.h7, yd, q.p2) + q.h8;
    // shared reciprocal (one Newton step: ~2^-46) and a residual correction per
    // quotient: the quotient's error before its final rounding is ~2^-92
    double rc = __builtin_amdgcn_rcp(t2);
    rc = fma(fma(-t2, rc, 1.0), rc, rc);
    const double q0 = t0 * rc, q1 = t1 * rc;
    const double tx = fma(fma(-t2, q0, t0), rc, q0);
    const double ty = fma(fma(-t2, q1, t1), rc, q1);
    // strict 0 < t < size, then truncation (apap.py:214-215).  For t > 0 the upper
    // test is the same on the truncated integer (the conversion saturates, NaN
    // fails t > 0).
    ix = (int)tx;
    iy = (int)ty;
    return (tx > 0.0) & (ty > 0.0) & (ix < img_w) & (iy < img_h);  // no short-circuit branches
}

// The byte offset of source pixel (ix, iy), or the outside marker: a pixel outside the source is marked by the sign bit (the
// launcher sends sources of 2 GiB or more to the flat-order kernel)
__device__ __forceinline__ unsigned strip_offset(bool ok, int ix, int iy, int img_w) {
    return ok ? (__umul24((unsigned)iy, (unsigned)img_w) + (unsigned)ix) * 3u : 0xffffffffu;
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

// ---- bilinear sampling (APAP_OPT_WARP_SAMPLING = APAP_SAMPLING_BILINEAR; the numpy definition is tests/warp_bilinear_spec.py),
// used by k_warp_bilinear (apap_warp_bilinear.hip) and k_panorama's bilinear forms --------------------------------------------

// strip_source's sibling: the same sequence, the same bits, and the coordinate itself.
__device__ __forceinline__ bool strip_source_xy(const PixelH &q, double yd, int img_w, int img_h, int &ix, int &iy, double &tx,
                                                double &ty) {
    const double t0 = fma(q.h1, yd, q.p0) + q.h2;
    const double t1 = fma(q.h4, yd, q.p1) + q.h5;
    const double t2 = fma(q.h7, yd, q.p2) + q.h8;
    double rc = __builtin_amdgcn_rcp(t2);
    rc = fma(fma(-t2, rc, 1.0), rc, rc);
    const double q0 = t0 * rc, q1 = t1 * rc;
    tx = fma(fma(-t2, q0, t0), rc, q0);
    ty = fma(fma(-t2, q1, t1), rc, q1);
    ix = (int)tx;
    iy = (int)ty;
    return (tx > 0.0) & (ty > 0.0) & (ix < img_w) & (iy < img_h);
}

// X = rint(32 t) for 0 <= t < 2^31, split into the tap index X >> 5 and the weight X & 31.  One FMA: 32 t is exact, and the sum
// with 1.5 x 2^52 lies in [2^52, 2^53), where doubles are the integers - the FMA's single rounding (to nearest, ties to even;
// the constant is even) IS rint, and the sum's low mantissa bits are X: its low word holds X mod 2^32, bits 0 .. 18 of its high
// word X >> 32 (X < 2^36 for any side a source of under 4 GiB can have).  Any other t (an absent pixel) gives some pair of
// numbers.
__device__ __forceinline__ void fixed_coord(double t, unsigned &s, unsigned &a) {
    const double d = fma(32.0, t, 6755399441055744.0);
    const unsigned lo = (unsigned)__double2loint(d), hi = (unsigned)__double2hiint(d);
    s = __builtin_amdgcn_alignbit(hi, lo, 5u);
    a = lo & 31u;
}

// A sample's four taps in one register pair.  off: the byte offset of tap (y0, x0) = (min(sy, h - 1), min(sx, w - 1)) - all 32
// bits are offset, a source may have up to 4 GiB - 1 bytes, so presence is held apart, in `fr`.  fr: ax | ay << 5 | (x1 > x0) << 10
// | (y1 > y0) << 11 | present << 12 (bits 16 and up are the caller's); tap (y0, x1) is 3 bytes on when x1 > x0, and row y1 is
// 3 w bytes on when y1 > y0: the border is replicated.  An absent pixel gets the taps of pixel (0, 0) - addresses that are
// valid and shared, as the outside marker's are in gather_px - and its value is never used.
__device__ __forceinline__ void bilinear_taps(bool ok, double tx, double ty, int img_w, int img_h, unsigned &off, unsigned &fr) {
    unsigned sx, ax, sy, ay;
    fixed_coord(tx, sx, ax);
    fixed_coord(ty, sy, ay);
    sx = ok ? sx : 0u;
    sy = ok ? sy : 0u;
    const unsigned x0 = min(sx, (unsigned)img_w - 1u), y0 = min(sy, (unsigned)img_h - 1u);
    const unsigned stepx = (unsigned)(x0 + 1u < (unsigned)img_w), stepy = (unsigned)(y0 + 1u < (unsigned)img_h);
    off = (y0 * (unsigned)img_w + x0) * 3u;
    fr = ax | (ay << 5) | (stepx << 10) | (stepy << 11) | ((unsigned)ok << 12);
}

// the dword that holds the 3 bytes at byte offset `o` of the source in its low 24 bits (the top byte is whatever follows).
// For the image's very last pixel the dword one byte earlier, shifted, as in gather_px: no byte beyond the image is touched.
__device__ __forceinline__ unsigned gather_tap(const uint8_t *__restrict__ img, unsigned o, unsigned last) {
    unsigned int v;
    const unsigned oc = o < last ? o : last;
    __builtin_memcpy(&v, img + oc, 4);
    return __builtin_amdgcn_alignbyte(0u, v, o - oc);
}

// the four taps of (off, fr) in the order p00, p01, p10, p11; row_bytes = 3 w
__device__ __forceinline__ void gather_taps(const uint8_t *__restrict__ img, unsigned off, unsigned fr, unsigned row_bytes,
                                            unsigned last, unsigned (&p)[4]) {
    const unsigned dx = (fr & (1u << 10)) ? 3u : 0u, dy = (fr & (1u << 11)) ? row_bytes : 0u;
    p[0] = gather_tap(img, off, last);
    p[1] = gather_tap(img, off + dx, last);
    p[2] = gather_tap(img, off + dy, last);
    p[3] = gather_tap(img, off + dy + dx, last);
}

// ((32 - ax)(32 - ay) p00 + ax (32 - ay) p01 + (32 - ax) ay p10 + ax ay p11 + 512) >> 10 per channel as a 24-bit pixel; 0 for an
// absent sample.  Rows first, channels 0 and 2 side by side in one register (a row's sum is at most 32 x 255 < 2^13), then the
// columns channel by channel (at most 1024 x 255 + 512 < 2^18): integer sums, so the order does not matter.
__device__ __forceinline__ unsigned bilinear_blend(const unsigned (&p)[4], unsigned fr) {
    const unsigned ax = fr & 31u, ay = (fr >> 5) & 31u, bx = 32u - ax, by = 32u - ay;
    const unsigned t02 = __umul24(bx, p[0] & 0x00ff00ffu) + __umul24(ax, p[1] & 0x00ff00ffu);
    const unsigned t1 = __umul24(bx, (p[0] >> 8) & 0xffu) + __umul24(ax, (p[1] >> 8) & 0xffu);
    const unsigned b02 = __umul24(bx, p[2] & 0x00ff00ffu) + __umul24(ax, p[3] & 0x00ff00ffu);
    const unsigned b1 = __umul24(bx, (p[2] >> 8) & 0xffu) + __umul24(ax, (p[3] >> 8) & 0xffu);
    const unsigned c0 = (__umul24(by, t02 & 0xffffu) + __umul24(ay, b02 & 0xffffu) + 512u) >> 10;
    const unsigned c1 = (__umul24(by, t1) + __umul24(ay, b1) + 512u) >> 10;
    const unsigned c2 = (__umul24(by, t02 >> 16) + __umul24(ay, b02 >> 16) + 512u) >> 10;
    const unsigned v = c0 | (c1 << 8) | (c2 << 16);
    return (fr & (1u << 12)) ? v : 0u;
}

// The stitch of one canvas pixel: paste the centre picture's pixel (ci, cj) - nothing outside the picture - and uniform_blend
// (apap_utils.py:75-88) it with the warped pixel `w`.  clast: bytes of the centre - 4; the centre's very last pixel is read
// one byte earlier and shifted, as in gather_px.
__device__ __forceinline__ unsigned blend_center(unsigned w, const uint8_t *__restrict__ center, int ci, int cj, int center_h,
                                                 int center_w, unsigned clast) {
    const bool in = ci >= 0 && ci < center_h && cj >= 0 && cj < center_w;
    const unsigned co = in ? ((unsigned)ci * (unsigned)center_w + (unsigned)cj) * 3u : 0u;
    const unsigned cc = co < clast ? co : clast;
    unsigned int c;
    __builtin_memcpy(&c, center + cc, 4);
    c = in ? ((c >> (8 * (co - cc))) & 0x00ffffffu) : 0u;
    // uniform_blend: a pixel is "present" when its channel mean is > 0, i.e. any
    // channel is non-zero; both present -> floor((a + b) / 2) per channel (float64
    // sum * 0.5, astype(uint8)), otherwise a + b with one of them 0
    const unsigned avg = (w & c) + (((w ^ c) & 0x00fefefeu) >> 1);
    return (w != 0u && c != 0u) ? avg : (w | c);
}

}  // namespace
