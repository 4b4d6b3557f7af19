// Panorama: the centre picture and up to APAP_PANORAMA_MAX_LAYERS neighbours, each warped through its own local-homography
// grid, on ONE canvas in one fused pass (DESIGN.md "Panorama"; the numpy definition is tests/panorama_spec.py).
//
// Geometry.  Layer k has what local_warp takes for one pair: a source picture, a forward grid, mesh edges, the pair canvas
// (fw_k, fh_k) and the offsets (ox_k, oy_k) at which the centre sits on it.  The union canvas puts the centre at
// (OX, OY) = (max ox_k, max oy_k) and is W = OX + max(fw_k - ox_k) wide, H = OY + max(fh_k - oy_k) high; pair canvas k
// covers its columns [OX - ox_k, OX - ox_k + fw_k) and rows [OY - oy_k, OY - oy_k + fh_k).  The value of layer k at
// canvas pixel (X, Y) is local_warp_k[Y - OY + oy_k, X - OX + ox_k] inside that rectangle and black outside it.  The
// point the cell's inverse is applied to is (X - OX, Y - OY) for EVERY layer: a pixel's coordinates relative to the centre
// do not depend on the pair canvas it is seen through.
//
// Set-up: per layer the warp's own set-up launch (apap::warp_phase with kWarpSetup) into that layer's slice of the
// workspace; it leaves the cell inverses and the row / column -> cell tables (apap::warp_tables).
//
// k_panorama<mode>: K3's row-strip shape.  A lane owns 4 consecutive pixels of a canvas row, a wave a strip of kRows rows
// of 256 pixels, a block kWaves strips below each other.  The layer descriptors travel BY VALUE in the kernel argument
// (1 KB; no upload); the loop over layers is wave-uniform, a strip tests a layer's rectangle with scalar compares and
// skips the layers it does not touch.  Per layer the lane looks up its four cell columns, the wave its rows' cell rows, and
// the coordinates come from k_warp_rows' arithmetic (strip_cell_row, strip_source: the float64 chain, the strict bounds test, the
// truncation): the same device functions (apap_warp_dev.h), the same bits.  A layer's state (cell matrices, offsets, gathered pixels)
// is dead before the next layer starts: the registers do not grow with the layer count.
//   mean : per pixel the channel sums and the number of present values (any byte non-zero) in two registers
//          (ch0 | ch2 << 16, ch1 | count << 16; at most 17 x 255 per sum); the quotient is one multiply and shift with
//          ceil(2^18 / count) from a 18-entry LDS table (mean_recip / mean_div: exact for these ranges, checked exhaustively
//          on the host through apap_panorama_mean_of).
//   paste: inside the centre's rectangle the centre, unconditionally; outside it the first present layer.  A pixel that is
//          decided is not computed again, and once a ballot shows a whole strip decided the wave leaves the layer loop - a
//          strip wholly inside the centre's rectangle computes no coordinate at all.
//   ramp : the mean with a weight per sample, min(distance of the SOURCE pixel from its picture's border, ramp), 1 .. ramp
//          (ramp_weight; the centre's source pixel is (X - OX, Y - OY)).  Per pixel three registers of weight x value sums
//          (below 2^21) and the weight sums of two neighbouring pixels in one (below 2^13 each, 16 bits apart); a layer's
//          sixteen weights wait for its gathered pixels in registers.  The quotient is ramp_quotient, one IEEE float32
//          division per channel - exact for these ranges, checked on the host through apap_panorama_ramp_quotients.
//   band : the two-band blend (DESIGN.md "Panorama, two-band blend"; in numpy: tests/panorama_band_spec.py).  Every view has a
//          low-pass picture B_v, its box blur of radius `band` in SOURCE space (k_box_blur below, once per picture, border
//          replicated; band = 0: B_v = I_v) - not a blur of the warped canvas, for the reason the ramp weighs source pixels:
//          the blend stays in this one pass and needs no canvas-sized intermediate.  A view's sample c_v and the sample b_v of
//          B_v at the same place (the same pixel, or the same four taps and weights) are gathered together; presence is
//          decided on c_v.  The low band is the ramp blend of the b_v: L = floor(sum w_v b'_v / sum w_v), w_v = min(D_v, ramp)
//          with D_v the uncapped border distance of the source pixel.  The detail c'_s - b'_s comes from ONE view, the present
//          one with the largest D_v (the lowest index on ties), so fine detail is never averaged: out = clip(L + c'_s - b'_s,
//          0, 255).  Per pixel the ramp's three sums, one register with the weight sum (low 16 bits) and the best D so far
//          (14 bits, from bit 16), and one with the best view's detail, 9 bits a channel, biased by 255.  A strip of this
//          mode has kBandRows rows: the second gather's pixels live next to the first's.
// The canvas is written once with 12-byte non-temporal stores (a row's tail byte by byte, never past the row).
//
// k_box_blur: B = (T + (n^2 >> 1)) / n^2, n = 2 r + 1, T the sum of the picture over the n x n window with the border
// replicated; every view of a call in one launch (descriptors by value).  See the kernel.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstring>

#include "apap_internal.h"
#include "apap_warp_dev.h"

namespace {

constexpr int kMaxLayers = APAP_PANORAMA_MAX_LAYERS;
constexpr int kRows = 4;            // canvas rows of a strip (one wave)
constexpr int kBandRows = 2;        // ... of the two-band blend, which holds two gathers' pixels at a time
constexpr int strip_rows(int mode) { return mode == APAP_PANORAMA_BAND ? kBandRows : kRows; }
constexpr int kWaves = 4;           // strips of a block
constexpr int kStripCols = 256;     // 64 lanes x 4 pixels
constexpr unsigned kMeanShift = 18;

// floor(sum / count) for count = 1 .. 17 and sum <= 255 count as (sum * mean_recip(count)) >> 18: with m = ceil(2^18 / count)
// the error m count - 2^18 is below count, and sum * 17 < 2^18, so the product's floor is the quotient's; count = 0 gives 0.
__host__ __device__ inline unsigned mean_recip(unsigned count) { return count ? ((1u << kMeanShift) - 1u) / count + 1u : 0u; }
__host__ __device__ inline unsigned mean_div(unsigned sum, unsigned recip) { return (sum * recip) >> kMeanShift; }

// The weight of pixel (x, y) of a w x h picture: its distance from the border, counted from 1, at most ramp.
__host__ __device__ inline int min_of(int a, int b) { return a < b ? a : b; }
__host__ __device__ inline int ramp_weight(int x, int y, int w, int h, int ramp) {
    return min_of(min_of(min_of(x + 1, w - x), min_of(y + 1, h - y)), ramp);
}

// floor(sum / wsum) for wsum = 1 .. 17 x 256 and sum <= 255 wsum (below 2^21): both convert to float32 exactly, and the
// correctly rounded quotient truncates to the true one.  Where sum = k wsum the quotient is k, exactly.  Elsewhere the true
// quotient lies at least 1 / wsum > 2^-13 below k + 1 and rounding moves it by less than 255 x 2^-24 < 2^-16; it does not
// fall below k, which is a float32.  wsum = 0 gives 0.  Plain IEEE `/` on both sides (no reciprocal, no fast-math): the
// same bits on the host and in the kernel.
__host__ __device__ inline unsigned ramp_quotient(unsigned sum, unsigned wsum) {
    return wsum ? (unsigned)((float)sum / (float)wsum) : 0u;
}

struct PanoLayer {      // 64 bytes
    const uint8_t *img;
    const double *hinv_pad;     // [cells][APAP_HINV_STRIDE]
    const int *lut;             // [fh] cell row of a pair-canvas row, then [fw] cell column of a pair-canvas column
    int img_h, img_w, mesh_cols, fw, fh;
    int dx, dy;                 // the union-canvas column / row of the pair canvas' first: OX - ox, OY - oy
    unsigned last;              // bytes of the source - 4 (gather_px)
    const uint8_t *blur;        // band: the picture's low-pass picture, the same layout (img itself at band = 0)
};
static_assert(sizeof(PanoLayer) == 64, "the descriptor's size in the kernel argument");

struct PanoArgs {
    PanoLayer layer[kMaxLayers];
    const uint8_t *center;
    uint8_t *out;
    int center_h, center_w, OX, OY, W, H, n_layers, col_blocks;
    unsigned clast;             // bytes of the centre - 4
    int ramp;                   // ramp, band: the largest weight
    const uint8_t *center_blur; // band: the centre's low-pass picture
};
static_assert(sizeof(PanoArgs) <= 4096, "kernel arguments");

// ---- the two-band blend's per-pixel steps ----
// The uncapped distance of pixel (x, y) of a w x h picture from its border, counted from 1: below 2^14 for a picture of
// less than 2 GiB.
__host__ __device__ inline int border_distance(int x, int y, int w, int h) { return min_of(min_of(x + 1, w - x), min_of(y + 1, h - y)); }
constexpr unsigned kNoDetail = 255u | (255u << 9) | (255u << 18);      // c' = b' in every channel
// c' - b' + 255 per channel, 9 bits each
__device__ __forceinline__ unsigned band_detail(unsigned cg, unsigned bg) {
    return ((cg & 0xffu) + 255u - (bg & 0xffu)) | ((((cg >> 8) & 0xffu) + 255u - ((bg >> 8) & 0xffu)) << 9) |
           (((cg >> 16) + 255u - (bg >> 16)) << 18);
}
// One present view's sample into a pixel's state: D is its source pixel's border distance, 0 for an absent view, which then
// weighs nothing and never beats the best so far.  wd: weight sum (at most 17 x 256) | best D << 16.
__device__ __forceinline__ void band_take(unsigned cg, unsigned bg, unsigned D, unsigned ramp, unsigned &s0, unsigned &s1, unsigned &s2,
                                          unsigned &wd, unsigned &det) {
    const unsigned wt = min(D, ramp);
    s0 += __umul24(wt, bg & 0xffu);
    s1 += __umul24(wt, (bg >> 8) & 0xffu);
    s2 += __umul24(wt, bg >> 16);
    const bool better = (D << 16) > (wd & 0xffff0000u);     // strictly: the lowest index wins a tie
    det = better ? band_detail(cg, bg) : det;
    wd = (better ? (wd & 0xffffu) | (D << 16) : wd) + wt;
}
// clip(L + c' - b', 0, 255) of one channel
__device__ __forceinline__ unsigned band_channel(unsigned low, unsigned biased) {
    const int v = (int)low + (int)biased - 255;
    return (unsigned)min(max(v, 0), 255);
}

// ---- gain compensation (DESIGN.md "Panorama, gain compensation"; the numpy definition is tests/panorama_gain_spec.py) ----
constexpr int kViews = kMaxLayers + 1;      // view 0 is the centre, view k layer k - 1

// One channel of a sample under the 4.12 fixed-point gain q = 1024 .. 16383: round to nearest, clamp at 255.  q = 4096 is
// the identity, and 0 stays 0 at every q (2048 >> 12): a sample outside its picture stays black.
__host__ __device__ inline unsigned gain_channel(unsigned c, unsigned q) {
    const unsigned v = (c * q + 2048u) >> 12;
    return v < 255u ? v : 255u;
}
__host__ __device__ inline unsigned gain_px(unsigned v, unsigned q) {
    return gain_channel(v & 0xffu, q) | (gain_channel((v >> 8) & 0xffu, q) << 8) | (gain_channel(v >> 16, q) << 16);
}

// The arguments of the gained forms: the panorama's, and the gains by value or, where d_gain is set (the resident chain,
// whose solve runs on the device), in device memory.
struct PanoGainArgs {
    PanoArgs A;
    const int *d_gain;
    int gain_q[kViews];
};
static_assert(sizeof(PanoGainArgs) <= 4096, "kernel arguments");
template <bool kGain> struct ArgsOf { typedef PanoArgs type; };
template <> struct ArgsOf<true> { typedef PanoGainArgs type; };
__device__ __forceinline__ const PanoArgs &pano_args(const PanoArgs &a) { return a; }
__device__ __forceinline__ const PanoArgs &pano_args(const PanoGainArgs &g) { return g.A; }
__device__ __forceinline__ unsigned gain_of(const PanoArgs &, int) { return 4096u; }
__device__ __forceinline__ unsigned gain_of(const PanoGainArgs &g, int view) {
    return (unsigned)(g.d_gain ? g.d_gain[view] : g.gain_q[view]);
}

// kGain: every sample is scaled by its view's gain (gain_px) AFTER its presence, its ramp weight and paste's choice have
// been decided on the ungained bytes.  Without it the code is the ungained kernel's, instruction for instruction.
template <int kMode, int kSampling, bool kGain>
__global__ __launch_bounds__(kWaves * 64) void k_panorama(const typename ArgsOf<kGain>::type P) {
    const PanoArgs &A = pano_args(P);
    constexpr int kRows = strip_rows(kMode);
    __shared__ unsigned recip[32];
    if (kMode == APAP_PANORAMA_MEAN) {
        if (threadIdx.x < 32) recip[threadIdx.x] = threadIdx.x <= (unsigned)kMaxLayers + 1u ? mean_recip(threadIdx.x) : 0u;
        __syncthreads();
    }
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const unsigned row_block = blockIdx.x / (unsigned)A.col_blocks;
    const int x_wave = (int)(blockIdx.x - row_block * (unsigned)A.col_blocks) * kStripCols;
    const int j0 = x_wave + lane * 4;
    const int y_first = ((int)row_block * kWaves + wave) * kRows;
    const int y_end = min(y_first + kRows, A.H);
    if (j0 >= A.W || y_first >= y_end) return;
    const int npx = min(4, A.W - j0);
    double xs[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) xs[k] = (double)(j0 + k - A.OX);

    // the centre's pixels of the strip; bit 4 t + k of `live`: pixel k of row t is on the canvas
    unsigned live = 0u;
    unsigned und = 0u;                  // paste: live pixels no picture has decided yet
    unsigned a0[kRows][4], a1[kRows][4];    // mean: ch0 | ch2 << 16 and ch1 | count << 16; paste: a0 = the pixel
    unsigned a2[kRows][4], aw[kRows][2];    // ramp: a0, a1, a2 = sums of weight x channel; aw = weight sums of pixels 2 k | 2 k + 1 << 16
    unsigned ad[kRows][4], det[kRows][4];   // band: a0, a1, a2 = sums of weight x low band; ad = weight sum | best D << 16; det = the best view's detail
    const int ramp = A.ramp;
    {
        const uint8_t *__restrict__ center = A.center;
        const unsigned gain_c = gain_of(P, 0);
        unsigned co[kRows][4];
#pragma unroll
        for (int t = 0; t < kRows; ++t) {
            const int ci = y_first + t - A.OY;
            const bool row_on = y_first + t < y_end;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int cj = j0 + k - A.OX;
                const bool on = row_on && k < npx;
                const bool in = on && (unsigned)ci < (unsigned)A.center_h && (unsigned)cj < (unsigned)A.center_w;
                live |= (unsigned)on << (4 * t + k);
                und |= (unsigned)(on && !in) << (4 * t + k);
                co[t][k] = in ? ((unsigned)ci * (unsigned)A.center_w + (unsigned)cj) * 3u : 0xffffffffu;
            }
        }
#pragma unroll
        for (int t = 0; t < kRows; ++t) {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const unsigned c = gather_px(center, co[t][k], A.clast);
                const unsigned cg = kGain ? gain_px(c, gain_c) : c;
                if (kMode == APAP_PANORAMA_MEAN) {
                    a0[t][k] = cg & 0x00ff00ffu;
                    a1[t][k] = ((cg >> 8) & 0xffu) | ((unsigned)(c != 0u) << 16);
                } else if (kMode == APAP_PANORAMA_RAMP) {
                    // c != 0 only inside the centre's rectangle, where the weight is defined
                    const unsigned wt = c != 0u ? (unsigned)ramp_weight(j0 + k - A.OX, y_first + t - A.OY, A.center_w, A.center_h, ramp) : 0u;
                    a0[t][k] = __umul24(wt, cg & 0xffu);
                    a1[t][k] = __umul24(wt, (cg >> 8) & 0xffu);
                    a2[t][k] = __umul24(wt, cg >> 16);
                    aw[t][k >> 1] = (k & 1) ? aw[t][k >> 1] | (wt << 16) : wt;
                } else if (kMode == APAP_PANORAMA_BAND) {
                    const unsigned b = gather_px(A.center_blur, co[t][k], A.clast);
                    const unsigned D = c != 0u ? (unsigned)border_distance(j0 + k - A.OX, y_first + t - A.OY, A.center_w, A.center_h) : 0u;
                    a0[t][k] = a1[t][k] = a2[t][k] = ad[t][k] = 0u;
                    det[t][k] = kNoDetail;
                    band_take(cg, kGain ? gain_px(b, gain_c) : b, D, (unsigned)ramp, a0[t][k], a1[t][k], a2[t][k], ad[t][k], det[t][k]);
                } else {
                    a0[t][k] = cg;
                    a1[t][k] = 0u;
                }
            }
        }
    }

    for (int l = 0; l < A.n_layers; ++l) {      // wave-uniform
        if (kMode == APAP_PANORAMA_PASTE && __all(und == 0u)) break;
        const PanoLayer &L = A.layer[l];
        const int dx = L.dx, dy = L.dy, fw = L.fw, fh = L.fh;
        // the strip against the pair canvas' rectangle: scalar compares
        if (y_first >= dy + fh || y_end <= dy || x_wave >= dx + fw || x_wave + kStripCols <= dx) continue;
        const int *__restrict__ lut = L.lut;
        const double *__restrict__ hinv_pad = L.hinv_pad;
        const uint8_t *__restrict__ img = L.img;
        const uint8_t *__restrict__ blur = L.blur;      // band only
        const int img_w = L.img_w, img_h = L.img_h, mesh_cols = L.mesh_cols;
        const unsigned gain_l = gain_of(P, l + 1);
        int col[4];
        unsigned want = 0u;             // bit 4 t + k: the pixel lies on the pair canvas (and, paste, is still undecided)
        unsigned colin = 0u;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int j = j0 + k - dx;
            colin |= (unsigned)((unsigned)j < (unsigned)fw) << k;
            col[k] = lut[(unsigned)(fh + min(max(j, 0), fw - 1))];     // a pixel beside the pair canvas: any valid column
        }
        int rr[kRows];
        unsigned todo = 0u;             // the strip's rows on the pair canvas
#pragma unroll
        for (int t = 0; t < kRows; ++t) {
            const int i = y_first + t - dy;
            const bool rowin = (unsigned)i < (unsigned)fh && y_first + t < y_end;
            todo |= (unsigned)rowin << t;
            want |= rowin ? colin << (4 * t) : 0u;
            rr[t] = lut[(unsigned)min(max(i, 0), fh - 1)];
        }
#pragma unroll
        for (int t = 0; t < kRows; ++t) rr[t] = __builtin_amdgcn_readfirstlane(rr[t]);
        want &= kMode == APAP_PANORAMA_PASTE ? und : live;
        if (kSampling == APAP_SAMPLING_BILINEAR) {
            // The same passes over the cell rows; a sample keeps its first tap's offset and, in one register, its weights, its
            // presence and (ramp) its weight in the blend, which is still that of source pixel (int(tx), int(ty)).  A sample
            // that is absent, undecided or off the pair canvas keeps the taps of pixel (0, 0) and counts as black.  Then row by
            // row: sixteen taps in flight, four blends, four pixels into the accumulators.
            unsigned boff[kRows][4], bfr[kRows][4];
#pragma unroll
            for (int t = 0; t < kRows; ++t)
#pragma unroll
                for (int k = 0; k < 4; ++k) boff[t][k] = bfr[t][k] = 0u;
            while (todo != 0u) {
                const int first = __builtin_ctz(todo);
                int r = rr[0];
#pragma unroll
                for (int t = 1; t < kRows; ++t) r = (t == first) ? rr[t] : r;
                PixelH q[4];
                strip_cell_row(hinv_pad, r * mesh_cols, col, xs, q);
#pragma unroll
                for (int t = 0; t < kRows; ++t) {
                    if (!((todo >> t) & 1u) || rr[t] != r) continue;
                    todo &= ~(1u << t);
                    const double yd = (double)(y_first + t - A.OY);
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        int ix, iy;
                        double tx, ty;
                        const bool ok = strip_source_xy(q[k], yd, img_w, img_h, ix, iy, tx, ty) & (((want >> (4 * t + k)) & 1u) != 0u);
                        bilinear_taps(ok, tx, ty, img_w, img_h, boff[t][k], bfr[t][k]);
                        if (kMode == APAP_PANORAMA_RAMP) bfr[t][k] |= (ok ? (unsigned)ramp_weight(ix, iy, img_w, img_h, ramp) : 0u) << 16;
                        if (kMode == APAP_PANORAMA_BAND) bfr[t][k] |= (ok ? (unsigned)border_distance(ix, iy, img_w, img_h) : 0u) << 16;
                    }
                }
            }
            const unsigned last = L.last, row_bytes = (unsigned)img_w * 3u;
#pragma unroll
            for (int t = 0; t < kRows; ++t) {
                unsigned tap[4][4];
#pragma unroll
                for (int k = 0; k < 4; ++k) gather_taps(img, boff[t][k], bfr[t][k], row_bytes, last, tap[k]);
                unsigned low[4];        // band: the low-pass picture through the same taps and weights
                if (kMode == APAP_PANORAMA_BAND) {
                    unsigned btap[4][4];
#pragma unroll
                    for (int k = 0; k < 4; ++k) gather_taps(blur, boff[t][k], bfr[t][k], row_bytes, last, btap[k]);
#pragma unroll
                    for (int k = 0; k < 4; ++k) low[k] = bilinear_blend(btap[k], bfr[t][k]);
                }
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const unsigned v = bilinear_blend(tap[k], bfr[t][k]);
                    const unsigned vg = kGain ? gain_px(v, gain_l) : v;
                    if (kMode == APAP_PANORAMA_BAND) {
                        const unsigned D = v != 0u ? bfr[t][k] >> 16 : 0u;
                        band_take(vg, kGain ? gain_px(low[k], gain_l) : low[k], D, (unsigned)ramp, a0[t][k], a1[t][k], a2[t][k], ad[t][k], det[t][k]);
                    } else if (kMode == APAP_PANORAMA_MEAN) {
                        a0[t][k] += vg & 0x00ff00ffu;
                        a1[t][k] += ((vg >> 8) & 0xffu) | ((unsigned)(v != 0u) << 16);
                    } else if (kMode == APAP_PANORAMA_RAMP) {
                        const unsigned wt = v != 0u ? bfr[t][k] >> 16 : 0u;
                        a0[t][k] += __umul24(wt, vg & 0xffu);
                        a1[t][k] += __umul24(wt, (vg >> 8) & 0xffu);
                        a2[t][k] += __umul24(wt, vg >> 16);
                        aw[t][k >> 1] += wt << (16 * (k & 1));
                    } else {
                        a0[t][k] = v != 0u ? vg : a0[t][k];
                        und &= ~((unsigned)(v != 0u) << (4 * t + k));
                    }
                }
            }
            continue;
        }
        unsigned off[kRows][4];
#pragma unroll
        for (int t = 0; t < kRows; ++t)
#pragma unroll
            for (int k = 0; k < 4; ++k) off[t][k] = 0xffffffffu;
        unsigned wgt[kRows][4];         // ramp: the weights of the layer's samples
#pragma unroll
        for (int t = 0; t < kRows; ++t)
#pragma unroll
            for (int k = 0; k < 4; ++k) wgt[t][k] = 0u;
        // One pass per cell row the strip touches, as in k_warp_rows: fetch that row's matrices, then do every strip row that
        // lies in it.  All branches are wave-uniform.
        while (todo != 0u) {
            const int first = __builtin_ctz(todo);
            int r = rr[0];
#pragma unroll
            for (int t = 1; t < kRows; ++t) r = (t == first) ? rr[t] : r;
            PixelH q[4];
            strip_cell_row(hinv_pad, r * mesh_cols, col, xs, q);
#pragma unroll
            for (int t = 0; t < kRows; ++t) {
                if (!((todo >> t) & 1u) || rr[t] != r) continue;
                todo &= ~(1u << t);
                const double yd = (double)(y_first + t - A.OY);
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    int ix, iy;
                    const bool ok = strip_source(q[k], yd, img_w, img_h, ix, iy) & (((want >> (4 * t + k)) & 1u) != 0u);
                    off[t][k] = strip_offset(ok, ix, iy, img_w);
                    if (kMode == APAP_PANORAMA_RAMP) wgt[t][k] = (unsigned)ramp_weight(ix, iy, img_w, img_h, ramp);  // used where ok
                    if (kMode == APAP_PANORAMA_BAND) wgt[t][k] = (unsigned)border_distance(ix, iy, img_w, img_h);    // D, used where ok
                }
            }
        }
        const unsigned last = L.last;
        unsigned px[kRows][4];
#pragma unroll
        for (int t = 0; t < kRows; ++t)
#pragma unroll
            for (int k = 0; k < 4; ++k) px[t][k] = gather_px(img, off[t][k], last);
        unsigned bpx[kRows][4];         // band: the low-pass picture at the same offsets
        if (kMode == APAP_PANORAMA_BAND) {
#pragma unroll
            for (int t = 0; t < kRows; ++t)
#pragma unroll
                for (int k = 0; k < 4; ++k) bpx[t][k] = gather_px(blur, off[t][k], last);
        }
#pragma unroll
        for (int t = 0; t < kRows; ++t) {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const unsigned v = px[t][k];
                const unsigned vg = kGain ? gain_px(v, gain_l) : v;
                if (kMode == APAP_PANORAMA_BAND) {
                    // v != 0 only where the sample lies inside its picture, where wgt is its distance
                    const unsigned D = v != 0u ? wgt[t][k] : 0u;
                    band_take(vg, kGain ? gain_px(bpx[t][k], gain_l) : bpx[t][k], D, (unsigned)ramp, a0[t][k], a1[t][k], a2[t][k], ad[t][k], det[t][k]);
                } else if (kMode == APAP_PANORAMA_MEAN) {
                    a0[t][k] += vg & 0x00ff00ffu;
                    a1[t][k] += ((vg >> 8) & 0xffu) | ((unsigned)(v != 0u) << 16);
                } else if (kMode == APAP_PANORAMA_RAMP) {
                    // v != 0 only where the sample lies inside its picture: a black or outside sample weighs nothing
                    const unsigned wt = v != 0u ? wgt[t][k] : 0u;
                    a0[t][k] += __umul24(wt, vg & 0xffu);
                    a1[t][k] += __umul24(wt, (vg >> 8) & 0xffu);
                    a2[t][k] += __umul24(wt, vg >> 16);
                    aw[t][k >> 1] += wt << (16 * (k & 1));
                } else {
                    // off is the outside marker for every pixel that is decided: v != 0 only where the pixel is still open
                    a0[t][k] = v != 0u ? vg : a0[t][k];
                    und &= ~((unsigned)(v != 0u) << (4 * t + k));
                }
            }
        }
    }

#pragma unroll
    for (int t = 0; t < kRows; ++t) {
        const int y = y_first + t;
        if (y >= y_end) break;  // wave-uniform
        unsigned p[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (kMode == APAP_PANORAMA_MEAN) {
                const unsigned m = recip[a1[t][k] >> 16] & 0x7ffffu;
                p[k] = mean_div(a0[t][k] & 0xffffu, m) | (mean_div(a1[t][k] & 0xffffu, m) << 8) | (mean_div(a0[t][k] >> 16, m) << 16);
            } else if (kMode == APAP_PANORAMA_RAMP) {
                const unsigned ws = (aw[t][k >> 1] >> (16 * (k & 1))) & 0xffffu;
                p[k] = ramp_quotient(a0[t][k], ws) | (ramp_quotient(a1[t][k], ws) << 8) | (ramp_quotient(a2[t][k], ws) << 16);
            } else if (kMode == APAP_PANORAMA_BAND) {
                const unsigned ws = ad[t][k] & 0xffffu, d = det[t][k];
                p[k] = band_channel(ramp_quotient(a0[t][k], ws), d & 0x1ffu) | (band_channel(ramp_quotient(a1[t][k], ws), (d >> 9) & 0x1ffu) << 8) |
                       (band_channel(ramp_quotient(a2[t][k], ws), d >> 18) << 16);
            } else {
                p[k] = a0[t][k];
            }
        }
        APAP_STORE_PX4(A.out + ((size_t)y * (size_t)A.W + (size_t)j0) * 3u, p, npx);
    }
}

// ---- the low-pass pictures of the two-band blend ----------------------------------------------------------------------------
// k_box_blur: B = (T + (n^2 >> 1)) / n^2 with n = 2 r + 1 and T[y][x][c] the sum of I[clamp(y + dy)][clamp(x + dx)][c] over
// |dx|, |dy| <= r, for every picture of a call in ONE launch: the descriptors travel by value, a block finds its picture by
// comparing its index with the pictures' first blocks (scalar compares).  A block owns a tile of kBlurCols x th pixels
// (th = 32 rows up to r = 16, 16 rows above: the tile with its halo and the row sums fill at most 60 KB of LDS) and goes
// through four phases, a barrier after each:
//   load   the tile's rows with their halo, (th + 2 r) rows of (kBlurCols + 2 r) pixels, into LDS as bytes.  A row of the
//          picture is 3 w bytes and starts at any alignment: the row's span is read as the ALIGNED dwords that cover it; a
//          dword that is not wholly inside the picture (only the picture's first and last can be) byte by byte, the bytes
//          inside it only.  A row above or below the picture is the clamped row, read again; the columns beside the picture
//          are then filled from the row's first / last pixel in LDS.  Every byte of the LDS tile is written.
//   rows   16-bit sums over n pixels along x (at most 255 x 65), as running sums over runs of kBlurRun outputs.
//   cols   32-bit sums of n row sums along y, as running sums over runs of kBlurRun rows, then the division: T + (n^2 >> 1)
//          is below 2^21 and n^2 <= 4225, ramp_quotient's ranges (checked exhaustively on the host through
//          apap_panorama_ramp_quotients).  The bytes go to LDS, over the dead input tile.
//   store  the tile's rows as aligned dwords; a dword that is not wholly inside the tile's span of the row byte by byte, the
//          bytes inside it only - a neighbouring tile owns the others.  Plain stores: the canvas pass reads them next.
// Integers throughout: the result depends neither on the tile nor on any order.
constexpr int kBlurCols = 64, kBlurThreads = 256, kBlurRun = 8;
constexpr int kBlurOutBytes = kBlurCols * 3;

struct BlurView {       // 32 bytes
    const uint8_t *img;
    uint8_t *out;
    int h, w;
    unsigned first, tiles_x;    // the picture's first block; tiles in a row of tiles
};
struct BlurArgs {
    BlurView view[kViews];
    int n_views, r, th;
};
static_assert(sizeof(BlurArgs) <= 4096, "kernel arguments");

__host__ __device__ inline int blur_tile_rows(int r) { return r <= 16 ? 32 : 16; }
__host__ __device__ inline int blur_in_stride(int r) { return ((kBlurCols + 2 * r) * 3 + 3) & ~3; }
__host__ __device__ inline size_t blur_lds_bytes(int r) {
    const int rows_in = blur_tile_rows(r) + 2 * r;
    return (size_t)rows_in * blur_in_stride(r) + (size_t)rows_in * kBlurOutBytes * sizeof(uint16_t);
}

__global__ __launch_bounds__(kBlurThreads) void k_box_blur(const BlurArgs P) {
    extern __shared__ __align__(16) uint8_t blur_lds[];
    int vi = 0;
    for (int i = 1; i < P.n_views; ++i) vi = blockIdx.x >= P.view[i].first ? i : vi;    // first blocks ascend
    const BlurView &V = P.view[vi];
    const uint8_t *__restrict__ img = V.img;
    uint8_t *__restrict__ out = V.out;
    const int w = V.w, h = V.h, r = P.r, n = 2 * r + 1, th = P.th;
    const unsigned tile = blockIdx.x - V.first;
    const int tile_y = (int)(tile / V.tiles_x), tile_x = (int)(tile - (unsigned)tile_y * V.tiles_x);
    const int x0 = tile_x * kBlurCols, y0 = tile_y * th;
    const int rows_in = th + 2 * r, cols_in = kBlurCols + 2 * r, in_stride = blur_in_stride(r);
    uint8_t *tin = blur_lds;
    uint16_t *hs = (uint16_t *)(blur_lds + (size_t)rows_in * in_stride);
    const int tid = threadIdx.x;
    const long long total = (long long)h * w * 3;

    // load: pixels [xa, xb) of every row, to LDS columns [ca, cb)
    const int xa = max(x0 - r, 0), xb = min(x0 + kBlurCols + r, w);
    const int ca = xa - (x0 - r), cb = xb - (x0 - r);
    {
        const int nb = (xb - xa) * 3, ndm = (nb + 6) >> 2;      // dwords that cover nb bytes at any alignment
        for (int it = tid; it < rows_in * ndm; it += kBlurThreads) {
            const int ry = it / ndm, d = it - ry * ndm;
            const int sy = min(max(y0 - r + ry, 0), h - 1);
            const long long g = ((long long)sy * w + xa) * 3;
            const long long p = g - (long long)((uintptr_t)(img + g) & 3u) + 4 * d;
            const long long lo = p > g ? p : g, hi = p + 4 < g + nb ? p + 4 : g + nb;
            if (lo >= hi) continue;
            unsigned v = 0u;
            if (p >= 0 && p + 4 <= total) {
                v = *(const unsigned *)(img + p);
            } else {
                for (long long q = lo; q < hi; ++q) v |= (unsigned)img[q] << (8 * (int)(q - p));
            }
            uint8_t *dst = tin + ry * in_stride + ca * 3 + (int)(p - g);
            for (long long q = lo; q < hi; ++q) dst[(int)(q - p)] = (uint8_t)(v >> (8 * (int)(q - p)));
        }
    }
    __syncthreads();
    {   // the columns beside the picture: the row's first / last pixel
        const int pad = ca + (cols_in - cb);
        for (int it = tid; it < rows_in * pad * 3; it += kBlurThreads) {
            const int ry = it / (pad * 3), e = it - ry * (pad * 3), pc = e / 3, c = e - pc * 3;
            const int col = pc < ca ? pc : cb + (pc - ca);
            tin[ry * in_stride + col * 3 + c] = tin[ry * in_stride + (pc < ca ? ca : cb - 1) * 3 + c];
        }
    }
    __syncthreads();
    // rows: hs[ry][ob] = the sum of tin[ry][ob + 3 j], j = 0 .. 2 r
    for (int it = tid; it < rows_in * (kBlurOutBytes / kBlurRun); it += kBlurThreads) {
        const int ry = it / (kBlurOutBytes / kBlurRun), e = it - ry * (kBlurOutBytes / kBlurRun), run = e / 3, c = e - run * 3;
        const uint8_t *src = tin + ry * in_stride + run * kBlurRun * 3 + c;
        uint16_t *dst = hs + ry * kBlurOutBytes + run * kBlurRun * 3 + c;
        unsigned s = 0u;
        for (int j = 0; j < n; ++j) s += src[3 * j];
        dst[0] = (uint16_t)s;
#pragma unroll
        for (int i = 1; i < kBlurRun; ++i) {
            s += (unsigned)src[3 * (i - 1 + n)] - (unsigned)src[3 * (i - 1)];
            dst[3 * i] = (uint16_t)s;
        }
    }
    __syncthreads();
    // cols: the sums of n row sums, the quotient, the byte over the dead input tile
    uint8_t *tout = tin;
    const unsigned n2 = (unsigned)(n * n), half = n2 >> 1;
    for (int it = tid; it < (th / kBlurRun) * kBlurOutBytes; it += kBlurThreads) {
        const int run = it / kBlurOutBytes, ob = it - run * kBlurOutBytes;
        const uint16_t *src = hs + run * kBlurRun * kBlurOutBytes + ob;
        uint8_t *dst = tout + run * kBlurRun * kBlurOutBytes + ob;
        unsigned s = 0u;
        for (int j = 0; j < n; ++j) s += src[j * kBlurOutBytes];
        dst[0] = (uint8_t)ramp_quotient(s + half, n2);
#pragma unroll
        for (int i = 1; i < kBlurRun; ++i) {
            s += (unsigned)src[(i - 1 + n) * kBlurOutBytes] - (unsigned)src[(i - 1) * kBlurOutBytes];
            dst[i * kBlurOutBytes] = (uint8_t)ramp_quotient(s + half, n2);
        }
    }
    __syncthreads();
    // store: pixels [x0, xe) of rows [y0, y0 + rows_out)
    const int rows_out = min(th, h - y0), nb = (min(x0 + kBlurCols, w) - x0) * 3;
    constexpr int ndm = (kBlurOutBytes + 6) >> 2;
    for (int it = tid; it < rows_out * ndm; it += kBlurThreads) {
        const int oy = it / ndm, d = it - oy * ndm;
        const long long g = ((long long)(y0 + oy) * w + x0) * 3;
        const long long p = g - (long long)((uintptr_t)(out + g) & 3u) + 4 * d;
        const long long lo = p > g ? p : g, hi = p + 4 < g + nb ? p + 4 : g + nb;
        if (lo >= hi) continue;
        const uint8_t *src = tout + oy * kBlurOutBytes + (int)(p - g);
        if (lo == p && hi == p + 4) {
            *(unsigned *)(out + p) = (unsigned)src[0] | ((unsigned)src[1] << 8) | ((unsigned)src[2] << 16) | ((unsigned)src[3] << 24);
        } else {
            for (long long q = lo; q < hi; ++q) out[q] = src[(int)(q - p)];
        }
    }
}

// ---- overlap statistics -------------------------------------------------------------------------------------------------
// k_panorama_stats: N[a][b], the number of lattice pixels (X % step == 0 and Y % step == 0) at which views a and b are both
// present, and S[a][b], the sum of I_a = r + g + b of view a's sample over them.  One pass over the lattice.  A lane owns 4
// consecutive lattice columns of one lattice row, a wave 256 of them, a block kStatWaves lattice rows; a block takes strips
// blockIdx.x, blockIdx.x + gridDim.x, ...  Per pixel the panorama's own layer loop - the rectangle test with scalar compares,
// strip_cell_row / strip_source[_xy] / gather_px or the bilinear taps with the same arguments, hence the same bits - leaves a
// presence mask in a register and the intensities of the lane's four pixels, 16 bits each, in the lane's own 8 bytes of LDS
// per view (a register array indexed by the layer would go to scratch).  Then, for every pair of views some lane of the wave
// saw (a wave-uniform loop over the OR of the masks), the lanes' counts and sums are added across the wave, and lane 0 adds
// them to the block's table in LDS with integer atomics.  At its end the block adds every touched entry to the table in
// memory with one 64-bit integer atomic each.  Integers throughout: the result does not depend on the grid or on any order.
// The block's table holds 32-bit words: the launcher gives a block at most 2048 strips, 2^21 pixels, and 765 x 2^21 < 2^31.
constexpr int kStatWaves = 4;

struct StatsArgs {
    PanoArgs A;
    unsigned long long *N, *S;      // [V][V] each, V = n_layers + 1
    int step, LW, LH;               // the lattice: LW x LH pixels
    unsigned col_strips, n_strips;  // strips of 256 lattice columns in a row; blocks' strips in all
};
static_assert(sizeof(StatsArgs) <= 4096, "kernel arguments");

__device__ __forceinline__ unsigned wave_sum(unsigned v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += (unsigned)__shfl_xor((int)v, d, 64);
    return v;
}

__device__ __forceinline__ unsigned intensity(unsigned v) { return (v & 0xffu) + ((v >> 8) & 0xffu) + (v >> 16); }

template <int kSampling>
__global__ __launch_bounds__(kStatWaves * 64) void k_panorama_stats(const StatsArgs P) {
    const PanoArgs &A = P.A;
    __shared__ uint2 inten[kViews][kStatWaves * 64];    // [view][thread]: I of the thread's four pixels, 16 bits each
    __shared__ unsigned tn[kViews * kViews], ts[kViews * kViews];
    for (int i = threadIdx.x; i < kViews * kViews; i += kStatWaves * 64) tn[i] = ts[i] = 0u;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int V = A.n_layers + 1;
    const int step = P.step;
    for (unsigned strip = blockIdx.x; strip < P.n_strips; strip += gridDim.x) {    // block-uniform
        const unsigned row_block = strip / P.col_strips;
        const int lx_wave = (int)(strip - row_block * P.col_strips) * 256;
        const int ly = (int)row_block * kStatWaves + wave;
        if (ly >= P.LH) continue;       // wave-uniform; nothing below waits for another wave
        const int Y = ly * step;
        // the wave's canvas columns [x_first, x_last]: lattice columns lx_wave .. lx_wave + 255, as far as the lattice goes
        const int x_first = lx_wave * step, x_last = (min(lx_wave + 255, P.LW - 1)) * step;
        int X[4];
        double xs[4];
        unsigned live = 0u;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int lx = lx_wave + lane * 4 + k;
            const bool on = lx < P.LW;
            live |= (unsigned)on << k;
            X[k] = on ? lx * step : 0;      // a lane past the lattice: a valid column whose sample is not wanted
            xs[k] = (double)(X[k] - A.OX);
        }
        unsigned m[4];                      // bit v: view v is present at pixel k
        {
            const int ci = Y - A.OY;
            unsigned iv[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int cj = X[k] - A.OX;
                const bool in = ((live >> k) & 1u) && (unsigned)ci < (unsigned)A.center_h && (unsigned)cj < (unsigned)A.center_w;
                const unsigned co = in ? ((unsigned)ci * (unsigned)A.center_w + (unsigned)cj) * 3u : 0xffffffffu;
                const unsigned c = gather_px(A.center, co, A.clast);
                m[k] = (unsigned)(c != 0u);
                iv[k] = intensity(c);
            }
            inten[0][threadIdx.x] = make_uint2(iv[0] | (iv[1] << 16), iv[2] | (iv[3] << 16));
        }
        const double yd = (double)(Y - A.OY);
        for (int l = 0; l < A.n_layers; ++l) {      // wave-uniform
            const PanoLayer &L = A.layer[l];
            const int dx = L.dx, dy = L.dy, fw = L.fw, fh = L.fh;
            if (Y < dy || Y >= dy + fh || x_first >= dx + fw || x_last < dx) continue;
            const int *__restrict__ lut = L.lut;
            const double *__restrict__ hinv_pad = L.hinv_pad;
            const uint8_t *__restrict__ img = L.img;
            const int img_w = L.img_w, img_h = L.img_h;
            int col[4];
            unsigned want = 0u;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int j = X[k] - dx;
                want |= (unsigned)((unsigned)j < (unsigned)fw) << k;
                col[k] = lut[(unsigned)(fh + min(max(j, 0), fw - 1))];
            }
            want &= live;
            const int r = __builtin_amdgcn_readfirstlane(lut[(unsigned)(Y - dy)]);
            PixelH q[4];
            strip_cell_row(hinv_pad, r * L.mesh_cols, col, xs, q);
            const unsigned last = L.last;
            unsigned v[4];
            if (kSampling == APAP_SAMPLING_BILINEAR) {
                unsigned boff[4], bfr[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    int ix, iy;
                    double tx, ty;
                    const bool ok = strip_source_xy(q[k], yd, img_w, img_h, ix, iy, tx, ty) & (((want >> k) & 1u) != 0u);
                    bilinear_taps(ok, tx, ty, img_w, img_h, boff[k], bfr[k]);
                }
                unsigned tap[4][4];
#pragma unroll
                for (int k = 0; k < 4; ++k) gather_taps(img, boff[k], bfr[k], (unsigned)img_w * 3u, last, tap[k]);
#pragma unroll
                for (int k = 0; k < 4; ++k) v[k] = bilinear_blend(tap[k], bfr[k]);
            } else {
                unsigned off[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    int ix, iy;
                    const bool ok = strip_source(q[k], yd, img_w, img_h, ix, iy) & (((want >> k) & 1u) != 0u);
                    off[k] = strip_offset(ok, ix, iy, img_w);
                }
#pragma unroll
                for (int k = 0; k < 4; ++k) v[k] = gather_px(img, off[k], last);
            }
            unsigned iv[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                m[k] |= (unsigned)(v[k] != 0u) << (l + 1);
                iv[k] = intensity(v[k]);
            }
            inten[l + 1][threadIdx.x] = make_uint2(iv[0] | (iv[1] << 16), iv[2] | (iv[3] << 16));
        }

        // the pairs: a view the wave skipped left no bit in any mask, and what its LDS words hold is never selected
        const unsigned mine = m[0] | m[1] | m[2] | m[3];
        unsigned seen = 0u;
        for (int v = 0; v < V; ++v) seen |= __any((int)((mine >> v) & 1u)) ? 1u << v : 0u;
        seen = __builtin_amdgcn_readfirstlane(seen);
        for (unsigned ua = seen; ua != 0u; ua &= ua - 1u) {
            const int a = __builtin_ctz(ua);
            const uint2 pa = inten[a][threadIdx.x];
            const unsigned ia[4] = {pa.x & 0xffffu, pa.x >> 16, pa.y & 0xffffu, pa.y >> 16};
            for (unsigned ub = ua; ub != 0u; ub &= ub - 1u) {      // b = a, then every later view
                const int b = __builtin_ctz(ub);
                unsigned both = 0u;
#pragma unroll
                for (int k = 0; k < 4; ++k) both |= ((m[k] >> a) & (m[k] >> b) & 1u) << k;
                if (!__any((int)both)) continue;
                const uint2 pb = inten[b][threadIdx.x];
                const unsigned ib[4] = {pb.x & 0xffffu, pb.x >> 16, pb.y & 0xffffu, pb.y >> 16};
                unsigned x = 0u, y = 0u;    // x: count << 20 | sum of I_a (a wave: at most 256 and 256 x 765 < 2^18); y: sum of I_b
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const bool on = ((both >> k) & 1u) != 0u;
                    x += on ? (1u << 20) + ia[k] : 0u;
                    y += on ? ib[k] : 0u;
                }
                x = wave_sum(x);
                y = wave_sum(y);
                if (lane == 0) {
                    atomicAdd(&tn[a * kViews + b], x >> 20);
                    atomicAdd(&ts[a * kViews + b], x & 0xfffffu);
                    if (b != a) {
                        atomicAdd(&tn[b * kViews + a], x >> 20);
                        atomicAdd(&ts[b * kViews + a], y);
                    }
                }
            }
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < V * V; i += kStatWaves * 64) {
        const int a = i / V, b = i - a * V;
        const unsigned n = tn[a * kViews + b], s = ts[a * kViews + b];
        if (n != 0u) atomicAdd(&P.N[i], (unsigned long long)n);
        if (s != 0u) atomicAdd(&P.S[i], (unsigned long long)s);
    }
}

// ---- the gains ----------------------------------------------------------------------------------------------------------
// The normal equations of Brown & Lowe's gain compensation over n views and their solution by Cholesky, float64, in ONE
// written-out order of + - * / sqrt (the build has -ffp-contract=off: nothing is fused), so that host and device give the
// same bits; tests/panorama_gain_spec.py spells the same order in Python floats.  N, S: [n][n]; L: n x kViews doubles of
// scratch (row stride kViews); g: n doubles, q: n ints.  Returns 1, with every gain 1, when a pivot is not positive and
// finite or a gain is not finite - which valid statistics cannot cause -, else 0.
__host__ __device__ inline int gain_solve(const unsigned long long *N, const unsigned long long *S, int n, double sigma_n,
                                          double sigma_g, double *L, double *g, int *q) {
    const double big = 1.7976931348623157e308;
    const double inv_n2 = 1.0 / (sigma_n * sigma_n), inv_g2 = 1.0 / (sigma_g * sigma_g);
    for (int c = 0; c < n; ++c) {
        double acc = 0.0, rhs = 0.0;
        for (int b = 0; b < n; ++b) {
            L[c * kViews + b] = 0.0;
            if (b == c || N[c * n + b] == 0ull) continue;
            const double nf = (double)N[c * n + b];
            const double d3 = 3.0 * nf;
            const double mcb = (double)S[c * n + b] / d3, mbc = (double)S[b * n + c] / d3;
            acc = acc + nf * ((2.0 * (mcb * mcb)) * inv_n2 + inv_g2);
            rhs = rhs + nf * inv_g2;
            L[c * kViews + b] = -((((2.0 * nf) * mcb) * mbc) * inv_n2);
        }
        const bool overlaps = acc > 0.0;
        L[c * kViews + c] = overlaps ? acc : 1.0;       // a view that overlaps nothing: gain 1
        g[c] = overlaps ? rhs : 1.0;
    }
    int bad = 0;
    for (int j = 0; j < n && !bad; ++j) {       // the lower triangle, row by row, in place
        for (int k = 0; k < j; ++k) {
            double s = L[j * kViews + k];
            for (int p = 0; p < k; ++p) s = s - L[j * kViews + p] * L[k * kViews + p];
            L[j * kViews + k] = s / L[k * kViews + k];
        }
        double d = L[j * kViews + j];
        for (int p = 0; p < j; ++p) d = d - L[j * kViews + p] * L[j * kViews + p];
        if (!(d > 0.0) || d > big) bad = 1;
        else L[j * kViews + j] = sqrt(d);
    }
    if (!bad) {
        for (int j = 0; j < n; ++j) {
            double s = g[j];
            for (int p = 0; p < j; ++p) s = s - L[j * kViews + p] * g[p];
            g[j] = s / L[j * kViews + j];
        }
        for (int j = n - 1; j >= 0; --j) {
            double s = g[j];
            for (int p = j + 1; p < n; ++p) s = s - L[p * kViews + j] * g[p];
            g[j] = s / L[j * kViews + j];
        }
        for (int j = 0; j < n; ++j)
            if (!(g[j] >= -big && g[j] <= big)) bad = 1;
    }
    for (int j = 0; j < n; ++j) {
        if (bad) g[j] = 1.0;
        double t = rint(4096.0 * g[j]);     // half to even
        t = t >= 1024.0 ? t : 1024.0;
        t = t <= 16383.0 ? t : 16383.0;
        q[j] = (int)t;
    }
    return bad;
}

// One lane runs gain_solve on the table in device memory: the resident chain does not wait for the host.
__global__ __launch_bounds__(64) void k_panorama_gain_solve(const unsigned long long *N, const unsigned long long *S, int n,
                                                            double sigma_n, double sigma_g, double *g, int *q, int *flag) {
    __shared__ double L[kViews * kViews];
    if (threadIdx.x == 0) *flag = gain_solve(N, S, n, sigma_n, sigma_g, L, g, q);
}

size_t slice_bytes(int mesh_rows, int mesh_cols, int final_w, int final_h) {
    return apap::up256(apap_warp_workspace_bytes(mesh_rows, mesh_cols, final_w, final_h));
}

// W, H, OX, OY of the union canvas from the pair canvases; refuses a centre that does not fit one of them (the check of
// apap_stitch_device) and a canvas of 2^31 pixels or more
int bounds_of(int center_h, int center_w, const int *final_w, const int *final_h, const int *off_x, const int *off_y, int n_layers,
              int *out, const char *who) {
    if (!final_w || !final_h || !off_x || !off_y || !out) return apap::fail(APAP_ERR_INVALID_ARG, "%s: null argument", who);
    if (n_layers < 1 || n_layers > kMaxLayers) return apap::fail(APAP_ERR_INVALID_ARG, "%s: n_layers = %d (1 .. %d)", who, n_layers, kMaxLayers);
    if (center_h < 1 || center_w < 1) return apap::fail(APAP_ERR_INVALID_ARG, "%s: centre picture %d x %d", who, center_h, center_w);
    long long OX = 0, OY = 0, right = 0, below = 0;
    for (int k = 0; k < n_layers; ++k) {
        if (final_w[k] < 1 || final_h[k] < 1)
            return apap::fail(APAP_ERR_INVALID_ARG, "%s: layer %d: canvas %d x %d", who, k, final_w[k], final_h[k]);
        if (off_x[k] < 0 || off_y[k] < 0 || (long long)off_y[k] + center_h > final_h[k] || (long long)off_x[k] + center_w > final_w[k])
            return apap::fail(APAP_ERR_INVALID_ARG, "%s: layer %d: centre image %dx%d at (%d,%d) does not fit canvas %dx%d", who, k, center_w,
                              center_h, off_x[k], off_y[k], final_w[k], final_h[k]);
        OX = std::max(OX, (long long)off_x[k]);
        OY = std::max(OY, (long long)off_y[k]);
        right = std::max(right, (long long)final_w[k] - off_x[k]);
        below = std::max(below, (long long)final_h[k] - off_y[k]);
    }
    const long long W = OX + right, H = OY + below;
    if ((unsigned long long)W * (unsigned long long)H >= (1ull << 31))
        return apap::fail(APAP_ERR_INVALID_ARG, "%s: canvas %lld x %lld: 2^31 pixels or more", who, W, H);
    out[0] = (int)W; out[1] = (int)H; out[2] = (int)OX; out[3] = (int)OY;
    return APAP_OK;
}

}  // namespace

namespace apap {

int panorama_check(int center_h, int center_w, const int *img_h, const int *img_w, const int *mesh_rows, const int *mesh_cols,
                   const int *n_w, const int *n_h, const int *final_w, const int *final_h, const int *off_x, const int *off_y,
                   int n_layers, int mode, const int *ramp, int *bounds, const char *who) {
    if (!img_h || !img_w || !mesh_rows || !mesh_cols || !n_w || !n_h) return fail(APAP_ERR_INVALID_ARG, "%s: null argument", who);
    if (ramp) {
        if (*ramp < 1 || *ramp > APAP_PANORAMA_MAX_RAMP)
            return fail(APAP_ERR_INVALID_ARG, "%s: ramp = %d (1 .. %d)", who, *ramp, APAP_PANORAMA_MAX_RAMP);
    } else if (mode != APAP_PANORAMA_MEAN && mode != APAP_PANORAMA_PASTE) {
        return fail(APAP_ERR_INVALID_ARG, "%s: mode = %d (APAP_PANORAMA_MEAN or APAP_PANORAMA_PASTE)", who, mode);
    }
    const int rc = bounds_of(center_h, center_w, final_w, final_h, off_x, off_y, n_layers, bounds, who);
    if (rc) return rc;
    // a picture: at least 2 pixels (the gather reads a dword), sides below 2^24 (24-bit multiplies), below 2 GiB (the sign
    // bit of a byte offset marks a pixel outside it)
    const auto picture = [](int h, int w) {
        return h >= 1 && w >= 1 && (unsigned long long)h * w >= 2 && h < (1 << 24) && w < (1 << 24) &&
               (unsigned long long)h * (unsigned long long)w * 3ull < (1ull << 31);
    };
    if (!picture(center_h, center_w))
        return fail(APAP_ERR_INVALID_ARG, "%s: centre picture %d x %d (at least 2 pixels, sides below 2^24, below 2 GiB)", who, center_h, center_w);
    for (int k = 0; k < n_layers; ++k) {
        if (!picture(img_h[k], img_w[k]))
            return fail(APAP_ERR_INVALID_ARG, "%s: layer %d: picture %d x %d (at least 2 pixels, sides below 2^24, below 2 GiB)", who, k,
                        img_h[k], img_w[k]);
        if (mesh_rows[k] < 1 || mesh_cols[k] < 1 || n_w[k] < 1 || n_h[k] < 1)
            return fail(APAP_ERR_INVALID_ARG, "%s: layer %d: mesh %d x %d with %d / %d edges", who, k, mesh_rows[k], mesh_cols[k], n_w[k], n_h[k]);
        if ((unsigned long long)mesh_rows[k] * (unsigned long long)mesh_cols[k] * APAP_HINV_STRIDE * sizeof(double) >= (1ull << 32))
            return fail(APAP_ERR_INVALID_ARG, "%s: layer %d: mesh of 53 million cells or more", who, k);
    }
    return APAP_OK;
}

int panorama_band_check(int band, const char *who) {
    if (band < 0 || band > APAP_PANORAMA_MAX_BAND) return fail(APAP_ERR_INVALID_ARG, "%s: band = %d (0 .. %d)", who, band, APAP_PANORAMA_MAX_BAND);
    return APAP_OK;
}

// k_box_blur of radius r = 1 .. APAP_PANORAMA_MAX_BAND over n = 1 .. kViews pictures (img, out, h, w set; checked by the caller).
static int blur_launch(apap_ctx *ctx, const BlurView *views, int n, int r, void *stream) {
    BlurArgs B;
    std::memset(&B, 0, sizeof(B));
    B.r = r;
    B.th = blur_tile_rows(r);
    B.n_views = n;
    unsigned long long blocks = 0;
    for (int i = 0; i < n; ++i) {
        B.view[i] = views[i];
        B.view[i].tiles_x = (unsigned)((views[i].w + kBlurCols - 1) / kBlurCols);
        B.view[i].first = (unsigned)blocks;
        blocks += (unsigned long long)B.view[i].tiles_x * (unsigned)((views[i].h + B.th - 1) / B.th);
    }
    if (blocks >= (1ull << 31)) return apap::fail(APAP_ERR_INVALID_ARG, "k_box_blur: 2^31 tiles or more");
    hipStream_t s = (hipStream_t)stream;
    {
        apap::ProfScope prof(ctx, APAP_PROF_WARP, s);
        hipLaunchKernelGGL(k_box_blur, dim3((unsigned)blocks), dim3(kBlurThreads), blur_lds_bytes(r), s, B);
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return apap::hip_fail(e, "k_box_blur launch");
    return APAP_OK;
}

static bool blur_picture(int h, int w) { return h >= 1 && w >= 1 && (unsigned long long)h * (unsigned long long)w * 3ull < (1ull << 31); }

int box_blur_check(int h, int w, int radius, const char *who) {
    if (radius < 0 || radius > APAP_PANORAMA_MAX_BAND)
        return fail(APAP_ERR_INVALID_ARG, "%s: radius = %d (0 .. %d)", who, radius, APAP_PANORAMA_MAX_BAND);
    if (!blur_picture(h, w)) return fail(APAP_ERR_INVALID_ARG, "%s: picture %d x %d (at least 1 pixel, below 2 GiB)", who, h, w);
    return APAP_OK;
}

// The checks of the device forms that follow panorama_check, the warp's own set-up of every layer into its slice of the
// workspace, and the kernel arguments all three kernels share (`out` is left NULL).  band (NULL for every other blend): the
// low-pass pictures of the views into their slots behind the layers' slices, one k_box_blur launch, and their pointers.
static int panorama_prepare(apap_ctx *ctx, const PanoGeometry &G, const int *b, void *d_work, size_t work_bytes, int *d_status,
                            void *stream, const char *who, PanoArgs &A, const int *band = nullptr) {
    const int n_layers = G.n_layers;
    if (!G.d_center || !G.d_imgs || !G.d_Hfwd || !G.d_mesh_w || !G.d_mesh_h || !d_work || !d_status)
        return apap::fail(APAP_ERR_INVALID_ARG, "%s: null device pointer", who);
    for (int k = 0; k < n_layers; ++k)
        if (!G.d_imgs[k] || !G.d_Hfwd[k] || !G.d_mesh_w[k] || !G.d_mesh_h[k])
            return apap::fail(APAP_ERR_INVALID_ARG, "%s: layer %d: null device pointer", who, k);
    const size_t need = band ? apap_panorama_band_workspace_bytes(G.center_h, G.center_w, G.img_h, G.img_w, G.mesh_rows, G.mesh_cols, G.final_w,
                                                                  G.final_h, n_layers, *band)
                             : apap_panorama_workspace_bytes(G.mesh_rows, G.mesh_cols, G.final_w, G.final_h, n_layers);
    if (work_bytes < need) return apap::fail(APAP_ERR_WORKSPACE, "%s: workspace %zu < %zu bytes", who, work_bytes, need);
    if (((uintptr_t)d_work & 255) != 0) return apap::fail(APAP_ERR_INVALID_ARG, "%s: workspace must be 256-byte aligned", who);

    std::memset(&A, 0, sizeof(A));
    char *w = (char *)d_work;
    for (int k = 0; k < n_layers; ++k) {
        const size_t slice = slice_bytes(G.mesh_rows[k], G.mesh_cols[k], G.final_w[k], G.final_h[k]);
        // the warp's own set-up, unchanged: cell inverses and lookup tables of this pair into its slice
        const int rc = apap::warp_phase(ctx, nullptr, 0, 0, nullptr, 0, 0, G.d_Hfwd[k], G.mesh_rows[k], G.mesh_cols[k], G.d_mesh_w[k],
                                        G.n_w[k], G.d_mesh_h[k], G.n_h[k], G.final_w[k], G.final_h[k], G.off_x[k], G.off_y[k], nullptr,
                                        nullptr, w, slice, d_status + k, stream, 0, 0, apap::kWarpSetup, nullptr);
        if (rc) return rc;
        const apap::WarpTables t = apap::warp_tables(w, G.mesh_rows[k], G.mesh_cols[k], G.final_w[k], G.final_h[k]);
        PanoLayer &L = A.layer[k];
        L.img = G.d_imgs[k];
        L.hinv_pad = t.hinv_pad;
        L.lut = t.lut;
        L.img_h = G.img_h[k]; L.img_w = G.img_w[k]; L.mesh_cols = G.mesh_cols[k];
        L.fw = G.final_w[k]; L.fh = G.final_h[k];
        L.dx = b[2] - G.off_x[k]; L.dy = b[3] - G.off_y[k];
        L.last = (unsigned)G.img_h[k] * (unsigned)G.img_w[k] * 3u - 4u;
        w += slice;
    }
    A.center = G.d_center;
    A.center_h = G.center_h; A.center_w = G.center_w;
    A.W = b[0]; A.H = b[1]; A.OX = b[2]; A.OY = b[3];
    A.n_layers = n_layers;
    A.col_blocks = (A.W + kStripCols - 1) / kStripCols;
    A.clast = (unsigned)G.center_h * (unsigned)G.center_w * 3u - 4u;
    if (!band) return APAP_OK;
    // band = 0: B = I.  Else view v's low-pass picture in slot v; a view whose picture (pointer and size) an earlier view has
    // reads that view's and is not blurred again.
    BlurView todo[kViews];
    int n_todo = 0;
    const uint8_t *blurred[kViews];
    for (int v = 0; v <= n_layers; ++v) {
        const uint8_t *img = v ? G.d_imgs[v - 1] : G.d_center;
        const int h = v ? G.img_h[v - 1] : G.center_h, wd = v ? G.img_w[v - 1] : G.center_w;
        blurred[v] = img;
        if (*band > 0) {
            int same = -1;
            for (int u = 0; u < v && same < 0; ++u)
                if ((u ? G.d_imgs[u - 1] : G.d_center) == img && (u ? G.img_h[u - 1] : G.center_h) == h && (u ? G.img_w[u - 1] : G.center_w) == wd)
                    same = u;
            if (same >= 0) {
                blurred[v] = blurred[same];
            } else {
                blurred[v] = (const uint8_t *)w;
                todo[n_todo++] = BlurView{img, (uint8_t *)w, h, wd, 0u, 0u};
            }
            w += up256((size_t)h * wd * 3);
        }
        if (v) A.layer[v - 1].blur = blurred[v];
        else A.center_blur = blurred[v];
    }
    return n_todo ? blur_launch(ctx, todo, n_todo, *band, stream) : APAP_OK;
}

// k_panorama over the canvas.  gain_q (host, n_layers + 1 values) or d_gain (device) selects the gained forms.
static int panorama_launch(apap_ctx *ctx, PanoArgs &A, int mode, const int *ramp, const int *gain_q, const int *d_gain, uint8_t *d_out,
                           void *stream, bool band = false) {
    A.out = d_out;
    A.ramp = ramp ? *ramp : 0;
    const int rows = kWaves * strip_rows(band ? APAP_PANORAMA_BAND : APAP_PANORAMA_RAMP);
    const unsigned row_blocks = (unsigned)((A.H + rows - 1) / rows);
    const dim3 grid((unsigned)A.col_blocks * row_blocks);       // W H < 2^31: below 2^31 blocks
    hipStream_t s = (hipStream_t)stream;
    const bool bilinear = apap::opt(ctx, APAP_OPT_WARP_SAMPLING) == APAP_SAMPLING_BILINEAR;
    {
        apap::ProfScope prof(ctx, APAP_PROF_WARP, s);
        // APAP_OPT_WARP_SAMPLING: the option the pair warps read (the set-up phases above do not depend on it)
#define APAP_LAUNCH_PANORAMA(S, GAIN, ARGS)                                                                                       \
    do {                                                                                                                          \
        if (band) hipLaunchKernelGGL((k_panorama<APAP_PANORAMA_BAND, S, GAIN>), grid, dim3(kWaves * 64), 0, s, ARGS);             \
        else if (ramp) hipLaunchKernelGGL((k_panorama<APAP_PANORAMA_RAMP, S, GAIN>), grid, dim3(kWaves * 64), 0, s, ARGS);        \
        else if (mode == APAP_PANORAMA_MEAN) hipLaunchKernelGGL((k_panorama<APAP_PANORAMA_MEAN, S, GAIN>), grid, dim3(kWaves * 64), 0, s, ARGS); \
        else hipLaunchKernelGGL((k_panorama<APAP_PANORAMA_PASTE, S, GAIN>), grid, dim3(kWaves * 64), 0, s, ARGS);                 \
    } while (0)
        if (gain_q || d_gain) {
            PanoGainArgs GA;
            std::memset(&GA, 0, sizeof(GA));
            GA.A = A;
            GA.d_gain = d_gain;
            for (int v = 0; v < kViews; ++v) GA.gain_q[v] = gain_q && v <= A.n_layers ? gain_q[v] : 4096;
            if (bilinear) APAP_LAUNCH_PANORAMA(APAP_SAMPLING_BILINEAR, true, GA);
            else APAP_LAUNCH_PANORAMA(APAP_SAMPLING_NEAREST, true, GA);
        } else if (bilinear) {
            APAP_LAUNCH_PANORAMA(APAP_SAMPLING_BILINEAR, false, A);
        } else {
            APAP_LAUNCH_PANORAMA(APAP_SAMPLING_NEAREST, false, A);
        }
#undef APAP_LAUNCH_PANORAMA
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return apap::hip_fail(e, "k_panorama launch");
    return APAP_OK;
}

// The tables zeroed on the stream, then k_panorama_stats over the lattice.
static int stats_launch(apap_ctx *ctx, const PanoArgs &A, int step, unsigned long long *d_N, unsigned long long *d_S, void *stream) {
    hipStream_t s = (hipStream_t)stream;
    const size_t bytes = (size_t)(A.n_layers + 1) * (A.n_layers + 1) * sizeof(unsigned long long);
    hipError_t e = hipMemsetAsync(d_N, 0, bytes, s);
    if (e == hipSuccess) e = hipMemsetAsync(d_S, 0, bytes, s);
    if (e != hipSuccess) return apap::hip_fail(e, "panorama statistics: zero fill");
    StatsArgs P;
    std::memset(&P, 0, sizeof(P));
    P.A = A;
    P.N = d_N; P.S = d_S;
    P.step = step;
    P.LW = (A.W - 1) / step + 1;
    P.LH = (A.H - 1) / step + 1;
    P.col_strips = (unsigned)((P.LW + 255) / 256);
    P.n_strips = P.col_strips * (unsigned)((P.LH + kStatWaves - 1) / kStatWaves);      // LW LH < 2^31: fits
    // 4096 blocks, block x with the strips x, x + 4096, ... - or more blocks, so that none takes more than 2048 strips: 2^21
    // pixels at most, and a sum of the block's 32-bit table at most 765 times that, below 2^31.
    const dim3 grid(std::max(std::min(P.n_strips, 4096u), (P.n_strips + 2047u) / 2048u));
    {
        apap::ProfScope prof(ctx, APAP_PROF_WARP, s);
        if (apap::opt(ctx, APAP_OPT_WARP_SAMPLING) == APAP_SAMPLING_BILINEAR)
            hipLaunchKernelGGL((k_panorama_stats<APAP_SAMPLING_BILINEAR>), grid, dim3(kStatWaves * 64), 0, s, P);
        else
            hipLaunchKernelGGL((k_panorama_stats<APAP_SAMPLING_NEAREST>), grid, dim3(kStatWaves * 64), 0, s, P);
    }
    e = hipGetLastError();
    if (e != hipSuccess) return apap::hip_fail(e, "k_panorama_stats launch");
    return APAP_OK;
}

int panorama_gain_check(int n_views, const int *step, const int *gain_q, const double *sigma_n, const double *sigma_g, const char *who) {
    if (n_views < 2 || n_views > kViews) return fail(APAP_ERR_INVALID_ARG, "%s: n_views = %d (2 .. %d)", who, n_views, kViews);
    if (step && (*step < 1 || *step > APAP_PANORAMA_GAIN_MAX_STEP))
        return fail(APAP_ERR_INVALID_ARG, "%s: step = %d (1 .. %d)", who, *step, APAP_PANORAMA_GAIN_MAX_STEP);
    if (gain_q)
        for (int v = 0; v < n_views; ++v)
            if (gain_q[v] < APAP_PANORAMA_GAIN_MIN_Q || gain_q[v] > APAP_PANORAMA_GAIN_MAX_Q)
                return fail(APAP_ERR_INVALID_ARG, "%s: gain_q[%d] = %d (%d .. %d)", who, v, gain_q[v], APAP_PANORAMA_GAIN_MIN_Q,
                            APAP_PANORAMA_GAIN_MAX_Q);
    const double big = 1.7976931348623157e308;
    if (sigma_n && !(*sigma_n > 0.0 && *sigma_n <= big)) return fail(APAP_ERR_INVALID_ARG, "%s: sigma_n must be finite and positive", who);
    if (sigma_g && !(*sigma_g > 0.0 && *sigma_g <= big)) return fail(APAP_ERR_INVALID_ARG, "%s: sigma_g must be finite and positive", who);
    return APAP_OK;
}

int panorama_run(apap_ctx *ctx, const PanoGeometry &G, const PanoJob &J, void *d_work, size_t work_bytes, int *d_status, void *stream,
                 const char *who) {
    int b[4];
    int rc = J.band ? panorama_band_check(*J.band, who) : APAP_OK;
    if (rc) return rc;
    rc = panorama_check(G.center_h, G.center_w, G.img_h, G.img_w, G.mesh_rows, G.mesh_cols, G.n_w, G.n_h, G.final_w, G.final_h, G.off_x,
                        G.off_y, G.n_layers, J.mode, J.ramp, b, who);
    if (rc) return rc;
    const bool stats = J.what == kPanoStats || J.what == kPanoAuto;
    if (J.what != kPanoPlain &&
        (rc = panorama_gain_check(G.n_layers + 1, stats ? &J.step : nullptr, J.what == kPanoGain ? J.gain_q : nullptr,
                                  J.what == kPanoAuto ? &J.sigma_n : nullptr, J.what == kPanoAuto ? &J.sigma_g : nullptr, who)))
        return rc;
    if (J.what == kPanoGain && !J.gain_q) return fail(APAP_ERR_INVALID_ARG, "%s: null gain_q", who);
    if (stats && (!J.d_N || !J.d_S)) return fail(APAP_ERR_INVALID_ARG, "%s: null statistics table", who);
    if (J.what == kPanoAuto && (!J.d_g || !J.d_q || !J.d_flag)) return fail(APAP_ERR_INVALID_ARG, "%s: null gain output", who);
    if (J.what != kPanoStats && !J.d_out) return fail(APAP_ERR_INVALID_ARG, "%s: null device pointer", who);
    PanoArgs A;
    if ((rc = panorama_prepare(ctx, G, b, d_work, work_bytes, d_status, stream, who, A, J.band))) return rc;
    if (stats && (rc = stats_launch(ctx, A, J.step, J.d_N, J.d_S, stream))) return rc;
    if (J.what == kPanoStats) return APAP_OK;
    if (J.what == kPanoAuto) {
        hipLaunchKernelGGL(k_panorama_gain_solve, dim3(1), dim3(64), 0, (hipStream_t)stream, J.d_N, J.d_S, G.n_layers + 1, J.sigma_n,
                           J.sigma_g, J.d_g, J.d_q, J.d_flag);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return apap::hip_fail(e, "k_panorama_gain_solve launch");
    }
    return panorama_launch(ctx, A, J.mode, J.ramp, J.what == kPanoGain ? J.gain_q : nullptr, J.what == kPanoAuto ? J.d_q : nullptr, J.d_out,
                           stream, J.band != nullptr);
}

int panorama_device(apap_ctx *ctx, const uint8_t *d_center, int center_h, int center_w, const uint8_t *const *d_imgs, const int *img_h,
                    const int *img_w, const float *const *d_Hfwd, const int *mesh_rows, const int *mesh_cols,
                    const double *const *d_mesh_w, const int *n_w, const double *const *d_mesh_h, const int *n_h, const int *final_w,
                    const int *final_h, const int *off_x, const int *off_y, int n_layers, int mode, const int *ramp, uint8_t *d_out,
                    void *d_work, size_t work_bytes, int *d_status, void *stream, const char *who) {
    const PanoGeometry G{d_center, center_h, center_w, d_imgs, img_h, img_w, d_Hfwd, mesh_rows, mesh_cols, d_mesh_w, n_w, d_mesh_h, n_h,
                         final_w, final_h, off_x, off_y, n_layers};
    PanoJob J;
    J.mode = mode; J.ramp = ramp; J.d_out = d_out;
    return panorama_run(ctx, G, J, d_work, work_bytes, d_status, stream, who);
}

int panorama_gain_solve_host(const unsigned long long *N, const unsigned long long *S, int n_views, double sigma_n, double sigma_g,
                             double *g, int *q) {
    double L[kViews * kViews];
    return gain_solve(N, S, n_views, sigma_n, sigma_g, L, g, q);
}

}  // namespace apap

extern "C" {

unsigned apap_panorama_mean_of(unsigned sum, unsigned count) { return mean_div(sum, mean_recip(count)); }

int apap_panorama_ramp_weight(int x, int y, int w, int h, int ramp) { return ramp_weight(x, y, w, h, ramp); }

void apap_panorama_ramp_quotients(const unsigned *sum, const unsigned *wsum, int n, unsigned *out) {
    if (!sum || !wsum || !out) return;
    for (int k = 0; k < n; ++k) out[k] = ramp_quotient(sum[k], wsum[k]);
}

int apap_panorama_gain_solve(const unsigned long long *N, const unsigned long long *S, int n_views, double sigma_n, double sigma_g,
                             double *g_out, int *q_out, int *flag_out) {
    const char *who = "apap_panorama_gain_solve";
    if (!N || !S || !g_out || !q_out || !flag_out) return apap::fail(APAP_ERR_INVALID_ARG, "%s: null argument", who);
    const int rc = apap::panorama_gain_check(n_views, nullptr, nullptr, &sigma_n, &sigma_g, who);
    if (rc) return rc;
    *flag_out = apap::panorama_gain_solve_host(N, S, n_views, sigma_n, sigma_g, g_out, q_out);
    return APAP_OK;
}

int apap_panorama_gain_apply(const uint8_t *values, int n, int q, uint8_t *out) {
    const char *who = "apap_panorama_gain_apply";
    if (!values || !out || n < 0) return apap::fail(APAP_ERR_INVALID_ARG, "%s: null argument or negative n", who);
    if (q < APAP_PANORAMA_GAIN_MIN_Q || q > APAP_PANORAMA_GAIN_MAX_Q)
        return apap::fail(APAP_ERR_INVALID_ARG, "%s: q = %d (%d .. %d)", who, q, APAP_PANORAMA_GAIN_MIN_Q, APAP_PANORAMA_GAIN_MAX_Q);
    for (int k = 0; k < n; ++k) out[k] = (uint8_t)gain_channel(values[k], (unsigned)q);
    return APAP_OK;
}

int apap_panorama_gain_stats_device(apap_ctx *ctx, const uint8_t *d_center, int center_h, int center_w, const uint8_t *const *d_imgs,
                                    const int *img_h, const int *img_w, const float *const *d_Hfwd, const int *mesh_rows,
                                    const int *mesh_cols, const double *const *d_mesh_w, const int *n_w,
                                    const double *const *d_mesh_h, const int *n_h, const int *final_w, const int *final_h,
                                    const int *off_x, const int *off_y, int n_layers, int step, unsigned long long *d_N,
                                    unsigned long long *d_S, void *d_work, size_t work_bytes, int *d_status, void *stream) {
    const apap::PanoGeometry G{d_center, center_h, center_w, d_imgs, img_h, img_w, d_Hfwd, mesh_rows, mesh_cols, d_mesh_w, n_w, d_mesh_h,
                               n_h, final_w, final_h, off_x, off_y, n_layers};
    apap::PanoJob J;
    J.what = apap::kPanoStats; J.step = step; J.d_N = d_N; J.d_S = d_S;
    return apap::panorama_run(ctx, G, J, d_work, work_bytes, d_status, stream, "apap_panorama_gain_stats_device");
}

int apap_panorama_gain_device(apap_ctx *ctx, const uint8_t *d_center, int center_h, int center_w, const uint8_t *const *d_imgs,
                              const int *img_h, const int *img_w, const float *const *d_Hfwd, const int *mesh_rows,
                              const int *mesh_cols, const double *const *d_mesh_w, const int *n_w, const double *const *d_mesh_h,
                              const int *n_h, const int *final_w, const int *final_h, const int *off_x, const int *off_y, int n_layers,
                              int mode, int ramp, const int *gain_q, uint8_t *d_out, void *d_work, size_t work_bytes, int *d_status,
                              void *stream) {
    const apap::PanoGeometry G{d_center, center_h, center_w, d_imgs, img_h, img_w, d_Hfwd, mesh_rows, mesh_cols, d_mesh_w, n_w, d_mesh_h,
                               n_h, final_w, final_h, off_x, off_y, n_layers};
    apap::PanoJob J;
    J.what = apap::kPanoGain; J.mode = mode; J.ramp = mode == APAP_PANORAMA_RAMP ? &ramp : nullptr;
    J.gain_q = gain_q; J.d_out = d_out;
    return apap::panorama_run(ctx, G, J, d_work, work_bytes, d_status, stream, "apap_panorama_gain_device");
}

int apap_panorama_auto_gain_device(apap_ctx *ctx, const uint8_t *d_center, int center_h, int center_w, const uint8_t *const *d_imgs,
                                   const int *img_h, const int *img_w, const float *const *d_Hfwd, const int *mesh_rows,
                                   const int *mesh_cols, const double *const *d_mesh_w, const int *n_w, const double *const *d_mesh_h,
                                   const int *n_h, const int *final_w, const int *final_h, const int *off_x, const int *off_y,
                                   int n_layers, int mode, int ramp, int step, double sigma_n, double sigma_g, uint8_t *d_out,
                                   unsigned long long *d_N, unsigned long long *d_S, double *d_g, int *d_q, int *d_flag, void *d_work,
                                   size_t work_bytes, int *d_status, void *stream) {
    const apap::PanoGeometry G{d_center, center_h, center_w, d_imgs, img_h, img_w, d_Hfwd, mesh_rows, mesh_cols, d_mesh_w, n_w, d_mesh_h,
                               n_h, final_w, final_h, off_x, off_y, n_layers};
    apap::PanoJob J;
    J.what = apap::kPanoAuto; J.mode = mode; J.ramp = mode == APAP_PANORAMA_RAMP ? &ramp : nullptr;
    J.step = step; J.sigma_n = sigma_n; J.sigma_g = sigma_g;
    J.d_out = d_out; J.d_N = d_N; J.d_S = d_S; J.d_g = d_g; J.d_q = d_q; J.d_flag = d_flag;
    return apap::panorama_run(ctx, G, J, d_work, work_bytes, d_status, stream, "apap_panorama_auto_gain_device");
}

int apap_panorama_bounds(int center_h, int center_w, const int *final_w, const int *final_h, const int *off_x, const int *off_y,
                         int n_layers, int *out) {
    return bounds_of(center_h, center_w, final_w, final_h, off_x, off_y, n_layers, out, "apap_panorama_bounds");
}

size_t apap_panorama_workspace_bytes(const int *mesh_rows, const int *mesh_cols, const int *final_w, const int *final_h, int n_layers) {
    if (!mesh_rows || !mesh_cols || !final_w || !final_h || n_layers < 1 || n_layers > kMaxLayers) return 0;
    size_t total = 0;
    for (int k = 0; k < n_layers; ++k) {
        const size_t b = slice_bytes(mesh_rows[k], mesh_cols[k], final_w[k], final_h[k]);
        if (b == 0) return 0;
        total += b;
    }
    return total;
}

int apap_panorama_device(apap_ctx *ctx, const uint8_t *d_center, int center_h, int center_w, const uint8_t *const *d_imgs,
                         const int *img_h, const int *img_w, const float *const *d_Hfwd, const int *mesh_rows, const int *mesh_cols,
                         const double *const *d_mesh_w, const int *n_w, const double *const *d_mesh_h, const int *n_h,
                         const int *final_w, const int *final_h, const int *off_x, const int *off_y, int n_layers, int mode,
                         uint8_t *d_out, void *d_work, size_t work_bytes, int *d_status, void *stream) {
    return apap::panorama_device(ctx, d_center, center_h, center_w, d_imgs, img_h, img_w, d_Hfwd, mesh_rows, mesh_cols, d_mesh_w, n_w,
                                 d_mesh_h, n_h, final_w, final_h, off_x, off_y, n_layers, mode, nullptr, d_out, d_work, work_bytes,
                                 d_status, stream, "apap_panorama_device");
}

int apap_panorama_ramp_device(apap_ctx *ctx, const uint8_t *d_center, int center_h, int center_w, const uint8_t *const *d_imgs,
                              const int *img_h, const int *img_w, const float *const *d_Hfwd, const int *mesh_rows,
                              const int *mesh_cols, const double *const *d_mesh_w, const int *n_w, const double *const *d_mesh_h,
                              const int *n_h, const int *final_w, const int *final_h, const int *off_x, const int *off_y, int n_layers,
                              int ramp, uint8_t *d_out, void *d_work, size_t work_bytes, int *d_status, void *stream) {
    return apap::panorama_device(ctx, d_center, center_h, center_w, d_imgs, img_h, img_w, d_Hfwd, mesh_rows, mesh_cols, d_mesh_w, n_w,
                                 d_mesh_h, n_h, final_w, final_h, off_x, off_y, n_layers, APAP_PANORAMA_RAMP, &ramp, d_out, d_work,
                                 work_bytes, d_status, stream, "apap_panorama_ramp_device");
}

size_t apap_panorama_band_workspace_bytes(int center_h, int center_w, const int *img_h, const int *img_w, const int *mesh_rows,
                                          const int *mesh_cols, const int *final_w, const int *final_h, int n_layers, int band) {
    const size_t base = apap_panorama_workspace_bytes(mesh_rows, mesh_cols, final_w, final_h, n_layers);
    if (base == 0 || !img_h || !img_w || band < 0 || band > APAP_PANORAMA_MAX_BAND || !apap::blur_picture(center_h, center_w)) return 0;
    size_t total = base + (band ? apap::up256((size_t)center_h * center_w * 3) : 0);
    for (int k = 0; k < n_layers; ++k) {
        if (!apap::blur_picture(img_h[k], img_w[k])) return 0;
        if (band) total += apap::up256((size_t)img_h[k] * img_w[k] * 3);
    }
    return total;
}

int apap_box_blur_device(apap_ctx *ctx, const uint8_t *d_img, int h, int w, int radius, uint8_t *d_out, void *stream) {
    const char *who = "apap_box_blur_device";
    const int rc = apap::box_blur_check(h, w, radius, who);
    if (rc) return rc;
    if (!d_img || !d_out) return apap::fail(APAP_ERR_INVALID_ARG, "%s: null device pointer", who);
    const size_t bytes = (size_t)h * w * 3;
    if (d_img < d_out + bytes && d_out < d_img + bytes) return apap::fail(APAP_ERR_INVALID_ARG, "%s: the output overlaps the picture", who);
    if (radius == 0) {
        const hipError_t e = hipMemcpyAsync(d_out, d_img, bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream);
        return e == hipSuccess ? APAP_OK : apap::hip_fail(e, "apap_box_blur_device: copy");
    }
    const BlurView v{d_img, d_out, h, w, 0u, 0u};
    return apap::blur_launch(ctx, &v, 1, radius, stream);
}

int apap_panorama_band_device(apap_ctx *ctx, const uint8_t *d_center, int center_h, int center_w, const uint8_t *const *d_imgs,
                              const int *img_h, const int *img_w, const float *const *d_Hfwd, const int *mesh_rows,
                              const int *mesh_cols, const double *const *d_mesh_w, const int *n_w, const double *const *d_mesh_h,
                              const int *n_h, const int *final_w, const int *final_h, const int *off_x, const int *off_y, int n_layers,
                              int ramp, int band, const int *gain_q, uint8_t *d_out, void *d_work, size_t work_bytes, int *d_status,
                              void *stream) {
    const apap::PanoGeometry G{d_center, center_h, center_w, d_imgs, img_h, img_w, d_Hfwd, mesh_rows, mesh_cols, d_mesh_w, n_w, d_mesh_h,
                               n_h, final_w, final_h, off_x, off_y, n_layers};
    apap::PanoJob J;
    J.what = gain_q ? apap::kPanoGain : apap::kPanoPlain;
    J.mode = APAP_PANORAMA_BAND; J.ramp = &ramp; J.band = &band;
    J.gain_q = gain_q; J.d_out = d_out;
    return apap::panorama_run(ctx, G, J, d_work, work_bytes, d_status, stream, "apap_panorama_band_device");
}

}  // extern "C"
