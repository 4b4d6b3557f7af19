// image_warping of the reference's utils.py:93-127: a global-homography warp of one picture onto a canvas that bounds it and
// a base picture, and the paste or mean blend of the base picture - the output stage of spectral_method.py -s (:226-232).
// The definition - OpenCV 4.x's fixed-point INTER_LINEAR / BORDER_CONSTANT(0) warpPerspective in its exact-integer form,
// restated without OpenCV - is in DESIGN.md "Global warp and blend" and, operation by operation, in tests/image_warp_spec.py.
//
// k_image_warp: one fused pass over the canvas.  A lane owns 4 consecutive pixels of a canvas row (12 contiguous output
// bytes, one non-temporal global_store_dwordx3 to any byte address; a row's tail is stored byte by byte, never past the row),
// a wave 256 pixels of a row, a block of 256 threads 4 consecutive rows.  Per pixel:
//   1. X0, Y0, W0 = Minv (x, y, 1) in fp64, left to right, no fused multiply-add (the sources are built with
//      -ffp-contract=off); W = W0 ? 32 / W0 : 0 (the IEEE division); X = rint(clamp(X0 W)), Y likewise (round half to even);
//   2. sx = clamp(X >> 5) to int16, ax = X & 31; the four taps, each one unaligned dword load at the pixel's first byte
//      (3 bytes used; the picture's last pixel is read one byte earlier and shifted, so no byte beyond it is touched),
//      0 outside the source;
//   3. per channel (w00 p00 + w01 p01 + w10 p10 + w11 p11 + 512) >> 10 with the integer weights (32 - ax)(32 - ay) ...;
//   4. inside the base rectangle: the base pixel (direct blend; the taps are then not read at all), or the truncating
//      mean of the two where any warped channel is non-zero, else the base pixel.
// No intermediate canvas, no second pass, no atomics; the taps of neighbouring lanes are neighbouring source pixels because
// a stitching homography is close to a similarity.
//
// A batch is the same launch: a table of problem descriptors in device memory (pointers, shapes, Minv, canvas geometry, blend
// mode, first block), uploaded once; a block finds its problem by bisection of the first-block prefix.  The single call is
// the batch of one.  Minv is formed on the host (cv::invert's closed form for 3 x 3, fp64).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "apap_internal.h"
#include "apap_warp_dev.h"      // APAP_STORE_PX4: the canvas store the local warp's kernels use

namespace {

constexpr int kMaxSide = APAP_IMAGE_WARP_MAX_SIDE;
constexpr int kMaxProblems = APAP_IMAGE_WARP_MAX_PROBLEMS;
constexpr int kThreads = 256;
constexpr int kRowsPerBlock = kThreads / 64;   // a wave per canvas row
constexpr int kPxPerLane = 4;
constexpr int kColsPerBlock = 64 * kPxPerLane;

struct alignas(16) WarpProblem {   // one problem, in device memory
    const uint8_t *src, *base;
    uint8_t *out;
    double minv[9];
    int src_h, src_w, base_h, base_w, canvas_w, canvas_h, off_x, off_y, direct, col_blocks;
    unsigned block0;               // its first block of the launch (the next problem's block0 ends it)
    int pad;
};
static_assert(sizeof(WarpProblem) == 144, "the descriptor table's stride");

size_t table_bytes(int n) { return apap::up256((size_t)n * sizeof(WarpProblem)); }

// the 3 bytes at byte offset `off` of a picture of `total` bytes (off + 3 <= total), in the low 24 bits.  One unaligned dword
// load; at the picture's last pixel the dword one byte earlier, shifted, so that no byte beyond the picture is touched.
// kTiny: three byte loads - a picture of fewer than 4 bytes (1 x 1) has no such dword
template <bool kTiny>
__device__ __forceinline__ unsigned load_px(const uint8_t *__restrict__ img, unsigned off, unsigned total) {
    if (kTiny) return (unsigned)img[off] | ((unsigned)img[off + 1] << 8) | ((unsigned)img[off + 2] << 16);
    const unsigned last = total - 4u, oc = off < last ? off : last;
    unsigned v;
    __builtin_memcpy(&v, img + oc, 4);
    return (v >> (8u * (off - oc))) & 0x00ffffffu;
}

// a tap of the source: 0 outside it (and where the pixel is not wanted at all: the load then reads the picture's first bytes)
template <bool kTiny>
__device__ __forceinline__ unsigned tap(const uint8_t *__restrict__ src, bool want, int sx, int sy, int w, int h, unsigned total) {
    const bool ok = want && (unsigned)sx < (unsigned)w && (unsigned)sy < (unsigned)h;
    const unsigned off = ok ? ((unsigned)sy * (unsigned)w + (unsigned)sx) * 3u : 0u;
    const unsigned v = load_px<kTiny>(src, off, total);
    return ok ? v : 0u;
}

__device__ __forceinline__ int fixed_coord(double v) {
    return (int)rint(fmin(fmax(v, -2147483648.0), 2147483647.0));   // a NaN takes the lower bound
}

// The four pixels (x0 .. x0 + 3, y) of one lane, staged so that the loads of all four are in flight together: the base
// pixels, then the coordinates, then the 16 taps, then the integer blends.  A pixel past the row's end is computed like any
// other (its loads are bounds-checked like every tap) and not stored.
template <bool kTiny>
__device__ __forceinline__ void warp_lane(const WarpProblem &P, int x0, int y) {
    const uint8_t *__restrict__ src = P.src;
    const uint8_t *__restrict__ base = P.base;
    const int cw = P.canvas_w, w2 = P.src_w, h2 = P.src_h, w1 = P.base_w, h1 = P.base_h;
    const unsigned src_total = (unsigned)h2 * (unsigned)w2 * 3u, base_total = (unsigned)h1 * (unsigned)w1 * 3u;
    const bool direct = P.direct != 0;
    const int cy = y - P.off_y;
    const bool row_in = (unsigned)cy < (unsigned)h1;

    bool in[kPxPerLane];
    unsigned bpx[kPxPerLane], warped[kPxPerLane];
#pragma unroll
    for (int k = 0; k < kPxPerLane; ++k) {
        const int cx = x0 + k - P.off_x;
        in[k] = row_in && (unsigned)cx < (unsigned)w1;
        const unsigned v = load_px<kTiny>(base, in[k] ? ((unsigned)cy * (unsigned)w1 + (unsigned)cx) * 3u : 0u, base_total);
        bpx[k] = in[k] ? v : 0u;
        warped[k] = 0u;
    }
    // with the base picture pasted over them the warped pixels inside its rectangle are never seen: not computed, not read
    if (!(direct && in[0] && in[1] && in[2] && in[3])) {
        const double m0 = P.minv[0], m1 = P.minv[1], m2 = P.minv[2], m3 = P.minv[3], m4 = P.minv[4], m5 = P.minv[5], m6 = P.minv[6],
                     m7 = P.minv[7], m8 = P.minv[8];
        const double yd = (double)y;
        int X[kPxPerLane], Y[kPxPerLane];
#pragma unroll
        for (int k = 0; k < kPxPerLane; ++k) {
            const double xd = (double)(x0 + k);
            const double X0 = m0 * xd + m1 * yd + m2;
            const double Y0 = m3 * xd + m4 * yd + m5;
            const double W0 = m6 * xd + m7 * yd + m8;
            const double W = W0 != 0.0 ? 32.0 / W0 : 0.0;
            X[k] = fixed_coord(X0 * W);
            Y[k] = fixed_coord(Y0 * W);
        }
        unsigned p[kPxPerLane][4];
#pragma unroll
        for (int k = 0; k < kPxPerLane; ++k) {
            const bool want = !(direct && in[k]);
            const int sx = min(max(X[k] >> 5, -32768), 32767), sy = min(max(Y[k] >> 5, -32768), 32767);
            p[k][0] = tap<kTiny>(src, want, sx, sy, w2, h2, src_total);
            p[k][1] = tap<kTiny>(src, want, sx + 1, sy, w2, h2, src_total);
            p[k][2] = tap<kTiny>(src, want, sx, sy + 1, w2, h2, src_total);
            p[k][3] = tap<kTiny>(src, want, sx + 1, sy + 1, w2, h2, src_total);
        }
#pragma unroll
        for (int k = 0; k < kPxPerLane; ++k) {
            const unsigned ax = (unsigned)(X[k] & 31), ay = (unsigned)(Y[k] & 31);
            const unsigned w00 = (32u - ax) * (32u - ay), w01 = ax * (32u - ay), w10 = (32u - ax) * ay, w11 = ax * ay;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const unsigned s = 8u * (unsigned)c;
                const unsigned v = (w00 * ((p[k][0] >> s) & 255u) + w01 * ((p[k][1] >> s) & 255u) + w10 * ((p[k][2] >> s) & 255u) +
                                    w11 * ((p[k][3] >> s) & 255u) + 512u) >> 10;
                warped[k] |= v << s;
            }
        }
    }
    unsigned px[kPxPerLane];
#pragma unroll
    for (int k = 0; k < kPxPerLane; ++k) {
        // the truncating mean per channel: floor((a + b) / 2) = (a & b) + ((a ^ b) >> 1), three bytes at once
        const unsigned mean = (warped[k] & bpx[k]) + (((warped[k] ^ bpx[k]) & 0x00fefefeu) >> 1);
        px[k] = in[k] ? ((direct || warped[k] == 0u) ? bpx[k] : mean) : warped[k];
    }
    static_assert(kPxPerLane == 4, "APAP_STORE_PX4 stores a group of four");
    APAP_STORE_PX4(P.out + ((size_t)y * (size_t)cw + (size_t)x0) * 3u, px, min(kPxPerLane, cw - x0));
}

__global__ __launch_bounds__(kThreads) void k_image_warp(const WarpProblem *__restrict__ tab, int n_problems) {
    // the problem of this block: the last one whose first block is not beyond it
    int lo = 0, hi = n_problems - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (tab[mid].block0 <= blockIdx.x) lo = mid; else hi = mid - 1;
    }
    const WarpProblem &P = tab[lo];
    const int col_blocks = P.col_blocks;
    const unsigned b = blockIdx.x - P.block0;
    const int row_tile = (int)(b / (unsigned)col_blocks), col_block = (int)(b - (unsigned)row_tile * (unsigned)col_blocks);
    const int y = row_tile * kRowsPerBlock + (int)(threadIdx.x >> 6);
    const int x0 = col_block * kColsPerBlock + (int)(threadIdx.x & 63u) * kPxPerLane;
    if (y >= P.canvas_h || x0 >= P.canvas_w) return;
    if (P.src_h * P.src_w < 2 || P.base_h * P.base_w < 2) warp_lane<true>(P, x0, y);   // a 1 x 1 picture (block-uniform)
    else warp_lane<false>(P, x0, y);
}

// cv::invert's closed form for 3 x 3 (DECOMP_LU, double): the cofactors times 1 / det, det expanded along row 0
bool invert3(const double *m, double *out) {
    const double det = m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6]) + m[2] * (m[3] * m[7] - m[4] * m[6]);
    if (!(det != 0.0) || !std::isfinite(det)) return false;
    const double d = 1.0 / det;
    out[0] = (m[4] * m[8] - m[5] * m[7]) * d;
    out[1] = (m[2] * m[7] - m[1] * m[8]) * d;
    out[2] = (m[1] * m[5] - m[2] * m[4]) * d;
    out[3] = (m[5] * m[6] - m[3] * m[8]) * d;
    out[4] = (m[0] * m[8] - m[2] * m[6]) * d;
    out[5] = (m[2] * m[3] - m[0] * m[5]) * d;
    out[6] = (m[3] * m[7] - m[4] * m[6]) * d;
    out[7] = (m[1] * m[6] - m[0] * m[7]) * d;
    out[8] = (m[0] * m[4] - m[1] * m[3]) * d;
    for (int k = 0; k < 9; ++k)
        if (!std::isfinite(out[k])) return false;
    return true;
}

unsigned blocks_of(int canvas_w, int canvas_h) {
    return (unsigned)((canvas_w + kColsPerBlock - 1) / kColsPerBlock) * (unsigned)((canvas_h + kRowsPerBlock - 1) / kRowsPerBlock);
}

}  // namespace

namespace apap {

// The argument checks of the global warp's entry points that need no device pointer.
int image_warp_check(const int *base_h, const int *base_w, const int *src_h, const int *src_w, const double *M, const int *canvas_w,
                     const int *canvas_h, const int *off_x, const int *off_y, const int *direct_blend, int n_problems,
                     const long long *out_offset, const char *who) {
    if (!base_h || !base_w || !src_h || !src_w || !M || !canvas_w || !canvas_h || !off_x || !off_y || !direct_blend || !out_offset)
        return fail(APAP_ERR_INVALID_ARG, "%s: null shapes / M / canvas geometry / blend modes / out_offset", who);
    if (n_problems < 1 || n_problems > kMaxProblems)
        return fail(APAP_ERR_INVALID_ARG, "%s: n_problems = %d (1 .. %d)", who, n_problems, kMaxProblems);
    unsigned long long blocks = 0;
    for (int p = 0; p < n_problems; ++p) {
        const auto side = [](int v) { return v >= 1 && v <= kMaxSide; };
        if (!side(base_h[p]) || !side(base_w[p]) || !side(src_h[p]) || !side(src_w[p]))
            return fail(APAP_ERR_INVALID_ARG, "%s: problem %d: base %d x %d, source %d x %d (sides 1 .. %d)", who, p, base_h[p], base_w[p],
                        src_h[p], src_w[p], kMaxSide);
        if (!side(canvas_h[p]) || !side(canvas_w[p]))
            return fail(APAP_ERR_INVALID_ARG, "%s: problem %d: canvas %d x %d (sides 1 .. %d)", who, p, canvas_h[p], canvas_w[p], kMaxSide);
        if (off_x[p] < 0 || off_y[p] < 0 || (long long)off_x[p] + base_w[p] > canvas_w[p] || (long long)off_y[p] + base_h[p] > canvas_h[p])
            return fail(APAP_ERR_INVALID_ARG, "%s: problem %d: the %d x %d base picture does not fit the %d x %d canvas at (%d, %d)", who, p,
                        base_h[p], base_w[p], canvas_h[p], canvas_w[p], off_x[p], off_y[p]);
        if (direct_blend[p] != 0 && direct_blend[p] != 1)
            return fail(APAP_ERR_INVALID_ARG, "%s: problem %d: direct_blend = %d (0 or 1)", who, p, direct_blend[p]);
        if (out_offset[p] < 0) return fail(APAP_ERR_INVALID_ARG, "%s: problem %d: out_offset = %lld: negative", who, p, out_offset[p]);
        double minv[9];
        for (int k = 0; k < 9; ++k)
            if (!std::isfinite(M[9 * p + k])) return fail(APAP_ERR_INVALID_ARG, "%s: problem %d: M is not finite", who, p);
        if (!invert3(M + 9 * p, minv))
            return fail(APAP_ERR_INVALID_ARG, "%s: problem %d: M is singular (det = 0, or its inverse is not finite)", who, p);
        blocks += blocks_of(canvas_w[p], canvas_h[p]);
    }
    if (blocks > 0x7fffffffull) return fail(APAP_ERR_INVALID_ARG, "%s: the canvases take %llu blocks (at most 2^31 - 1 per call)", who, blocks);
    // the canvases must not overlap in the output buffer
    std::vector<std::pair<long long, long long>> span((size_t)n_problems);
    for (int p = 0; p < n_problems; ++p) span[p] = {out_offset[p], out_offset[p] + (long long)canvas_h[p] * canvas_w[p] * 3};
    std::sort(span.begin(), span.end());
    for (int p = 1; p < n_problems; ++p)
        if (span[p].first < span[p - 1].second)
            return fail(APAP_ERR_INVALID_ARG, "%s: two canvases overlap in the output buffer (offsets %lld and %lld)", who, span[p - 1].first,
                        span[p].first);
    return APAP_OK;
}

}  // namespace apap

extern "C" {

int apap_image_warp_bounds(int h1, int w1, int h2, int w2, const double *H, int *out) {
    const char *who = "apap_image_warp_bounds";
    if (!H || !out) return apap::fail(APAP_ERR_INVALID_ARG, "%s: null argument", who);
    if (h1 < 1 || h1 > kMaxSide || w1 < 1 || w1 > kMaxSide || h2 < 1 || h2 > kMaxSide || w2 < 1 || w2 > kMaxSide)
        return apap::fail(APAP_ERR_INVALID_ARG, "%s: base %d x %d, source %d x %d (sides 1 .. %d)", who, h1, w1, h2, w2, kMaxSide);
    // utils.py:101-104: the base picture's corners and the source's through H (cv.perspectiveTransform: fp64, rounded to float32)
    const float cx[4] = {0.f, 0.f, (float)w2, (float)w2}, cy[4] = {0.f, (float)h2, (float)h2, 0.f};
    float xs[8] = {0.f, 0.f, (float)w1, (float)w1}, ys[8] = {0.f, (float)h1, (float)h1, 0.f};
    for (int k = 0; k < 4; ++k) {
        const double x = (double)cx[k], y = (double)cy[k];
        double w = H[6] * x + H[7] * y + H[8];
        w = w != 0.0 ? 1.0 / w : 0.0;
        xs[4 + k] = (float)((H[0] * x + H[1] * y + H[2]) * w);
        ys[4 + k] = (float)((H[3] * x + H[4] * y + H[5]) * w);
    }
    float lo[2] = {xs[0], ys[0]}, hi[2] = {xs[0], ys[0]};
    for (int k = 0; k < 8; ++k) {
        if (!std::isfinite(xs[k]) || !std::isfinite(ys[k]))
            return apap::fail(APAP_ERR_INVALID_ARG, "%s: H sends a corner of the source to a non-finite point", who);
        lo[0] = std::min(lo[0], xs[k]); lo[1] = std::min(lo[1], ys[k]);
        hi[0] = std::max(hi[0], xs[k]); hi[1] = std::max(hi[1], ys[k]);
    }
    // utils.py:105-106: np.int32(min - 0.5), np.int32(max + 0.5): float32 arithmetic, truncation toward zero
    float v[4] = {lo[0] - 0.5f, lo[1] - 0.5f, hi[0] + 0.5f, hi[1] + 0.5f};
    for (int k = 0; k < 4; ++k) {
        if (!(std::fabs(v[k]) < 2147483648.f)) return apap::fail(APAP_ERR_INVALID_ARG, "%s: H sends a corner of the source beyond the int32 range", who);
        out[k] = (int)v[k];
    }
    const long long cw = (long long)out[2] - out[0], ch = (long long)out[3] - out[1];
    if (cw < 1 || cw > kMaxSide || ch < 1 || ch > kMaxSide)
        return apap::fail(APAP_ERR_INVALID_ARG, "%s: the canvas would be %lld x %lld (sides 1 .. %d)", who, ch, cw, kMaxSide);
    return APAP_OK;
}

size_t apap_image_warp_workspace_bytes(int n_problems) { return n_problems < 1 || n_problems > kMaxProblems ? 0 : table_bytes(n_problems); }

int apap_image_warp_batch_device(apap_ctx *ctx, const uint8_t *const *d_bases, const int *base_h, const int *base_w,
                                 const uint8_t *const *d_srcs, const int *src_h, const int *src_w, const double *M, const int *canvas_w,
                                 const int *canvas_h, const int *off_x, const int *off_y, const int *direct_blend, int n_problems,
                                 uint8_t *d_out, const long long *out_offset, void *d_work, size_t work_bytes, int *d_status, void *stream) {
    const char *who = "apap_image_warp_batch_device";
    (void)ctx;
    (void)d_status;   // no condition of this kernel is reported through it
    int rc = apap::image_warp_check(base_h, base_w, src_h, src_w, M, canvas_w, canvas_h, off_x, off_y, direct_blend, n_problems, out_offset, who);
    if (rc) return rc;
    if (!d_bases || !d_srcs || !d_out || !d_work) return apap::fail(APAP_ERR_INVALID_ARG, "%s: null device pointer", who);
    for (int p = 0; p < n_problems; ++p)
        if (!d_bases[p] || !d_srcs[p]) return apap::fail(APAP_ERR_INVALID_ARG, "%s: problem %d: null device pointer", who, p);
    const size_t need = table_bytes(n_problems);
    if (work_bytes < need) return apap::fail(APAP_ERR_WORKSPACE, "%s: workspace %zu < %zu bytes", who, work_bytes, need);
    if (((uintptr_t)d_work & 255) != 0) return apap::fail(APAP_ERR_INVALID_ARG, "%s: workspace must be 256-byte aligned", who);

    std::vector<WarpProblem> tab((size_t)n_problems);
    unsigned blocks = 0;
    for (int p = 0; p < n_problems; ++p) {
        WarpProblem &P = tab[p];
        std::memset(&P, 0, sizeof(P));
        P.src = d_srcs[p];
        P.base = d_bases[p];
        P.out = d_out + out_offset[p];
        invert3(M + 9 * p, P.minv);
        P.src_h = src_h[p]; P.src_w = src_w[p]; P.base_h = base_h[p]; P.base_w = base_w[p];
        P.canvas_w = canvas_w[p]; P.canvas_h = canvas_h[p]; P.off_x = off_x[p]; P.off_y = off_y[p];
        P.direct = direct_blend[p];
        P.col_blocks = (canvas_w[p] + kColsPerBlock - 1) / kColsPerBlock;
        P.block0 = blocks;
        blocks += blocks_of(canvas_w[p], canvas_h[p]);
    }
    hipStream_t s = (hipStream_t)stream;
    // from pageable memory in stream order: the copy returns once its source has been consumed
    hipError_t e = hipMemcpyAsync(d_work, tab.data(), (size_t)n_problems * sizeof(WarpProblem), hipMemcpyHostToDevice, s);
    if (e != hipSuccess) return apap::hip_fail(e, "apap_image_warp_batch_device: descriptor upload");
    hipLaunchKernelGGL(k_image_warp, dim3(blocks), dim3(kThreads), 0, s, (const WarpProblem *)d_work, n_problems);
    e = hipGetLastError();
    if (e != hipSuccess) return apap::hip_fail(e, "apap_image_warp_batch_device launch");
    return APAP_OK;
}

int apap_image_warp_device(apap_ctx *ctx, const uint8_t *d_base, int h1, int w1, const uint8_t *d_src, int h2, int w2, const double *M,
                           int canvas_w, int canvas_h, int off_x, int off_y, int direct_blend, uint8_t *d_out, void *d_work,
                           size_t work_bytes, int *d_status, void *stream) {
    const long long at = 0;
    return apap_image_warp_batch_device(ctx, &d_base, &h1, &w1, &d_src, &h2, &w2, M, &canvas_w, &canvas_h, &off_x, &off_y, &direct_blend, 1,
                                        d_out, &at, d_work, work_bytes, d_status, stream);
}

}  // extern "C"
