// The local warp under APAP_OPT_WARP_SAMPLING = APAP_SAMPLING_BILINEAR (DESIGN.md "Bilinear sampling"; the numpy definition is
// tests/warp_bilinear_spec.py): the coordinate, the presence test and the footprint of the truncating warp, and a pixel
// reconstructed at that coordinate from its four neighbours with 5 fractional bits instead of taken at (int(tx), int(ty)).
//
// k_warp_bilinear<kBlend, kRows> has k_warp_rows' shape (apap_kernels.hip): a lane owns 4 consecutive pixels of a canvas row
// and walks kRows rows with them, a wave shares its rows, so cell rows are wave-uniform and the matrices are fetched once per
// cell row the strip touches.  Per pixel and row: strip_source_xy (the strip's exact float64 sequence, one Newton step),
// bilinear_taps (X = rint(32 tx) in one FMA, the clamped taps), four gathers, bilinear_blend, blend_center when stitching;
// four pixels leave as one 12-byte non-temporal store.  All of it from apap_warp_dev.h: the panorama uses the same bits.
//
// Sources of every size warp_impl admits (under 4 GiB, sides of any length) are served by this one kernel: a sample's byte
// offset uses all 32 bits and its presence is a bit of the register that holds its weights, not the offset's sign; offsets are
// formed with full 32-bit multiplies.  There is no flat-order fallback.
//
// kRows = 2, from the register budget (DESIGN.md has the table): with 2 rows the kernel has 32 taps in flight per lane in 124 /
// 128 registers, k_warp_rows' 4 waves per SIMD, no scratch; with 4 rows (64 taps) the compiler takes 178 / 219 registers, 2
// waves per SIMD, and held to 128 registers it spills.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "apap_internal.h"
#include "apap_warp_dev.h"

namespace {

constexpr int kStripRows = 2;       // canvas rows of a strip (one wave)
constexpr int kWaves = 4;           // strips of a block

template <bool kBlend, int kRows>
__global__ __launch_bounds__(kWaves * 64) void k_warp_bilinear(const apap::WarpGather G) {
    const int final_w = G.final_w, final_h = G.final_h;
    const int *__restrict__ lut = G.lut;
    if (!warp_tables_ready(lut[final_w + final_h], G.mesh_rows, G.mesh_cols, final_w, final_h, G.status)) return;
    const long long pair = blockIdx.z;      // pair of a batch
    const uint8_t *__restrict__ img = G.img + pair * G.img_stride;
    uint8_t *__restrict__ out = G.out + pair * G.out_stride;
    const uint8_t *__restrict__ center = kBlend ? G.center + pair * G.center_stride : nullptr;
    const double *__restrict__ hinv_pad = G.hinv_pad + pair * G.hinv_stride;
    const int img_w = G.img_w, img_h = G.img_h, off_x = G.off_x, off_y = G.off_y, mesh_cols = G.mesh_cols;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int j0 = ((int)blockIdx.x * 64 + lane) * 4;
    const int y_first = G.row_begin + ((int)blockIdx.y * kWaves + wave) * kRows;
    const int y_end = min(y_first + kRows, G.row_begin + G.row_count);
    if (j0 >= final_w || y_first >= y_end) return;
    const unsigned last = (unsigned)img_h * (unsigned)img_w * 3u - 4u;
    const unsigned row_bytes = (unsigned)img_w * 3u;
    const unsigned clast = kBlend ? (unsigned)G.center_h * (unsigned)G.center_w * 3u - 4u : 0u;
    const int npx = min(4, final_w - j0);
    int col[4];
    double xs[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int j = min(j0 + k, final_w - 1);  // pixels past the row end repeat the last one and are not stored
        col[k] = lut[(unsigned)(final_h + j)];
        xs[k] = (double)(j - off_x);
    }
    int rr[kRows];
#pragma unroll
    for (int t = 0; t < kRows; ++t) rr[t] = lut[(unsigned)min(y_first + t, y_end - 1)];
#pragma unroll
    for (int t = 0; t < kRows; ++t) rr[t] = __builtin_amdgcn_readfirstlane(rr[t]);
    unsigned off[kRows][4], fr[kRows][4];
    // One pass per cell row the strip touches, as in k_warp_rows.  All branches are wave-uniform.
    unsigned todo = (1u << kRows) - 1u;
    while (todo != 0u) {
        const int first = __builtin_ctz(todo);
        int r = rr[0];
#pragma unroll
        for (int t = 1; t < kRows; ++t) r = (t == first) ? rr[t] : r;
        PixelH q[4];
        strip_cell_row(hinv_pad, r * mesh_cols, col, xs, q);
#pragma unroll
        for (int t = 0; t < kRows; ++t) {
            if (rr[t] != r) continue;
            todo &= ~(1u << t);
            const double yd = (double)(y_first + t - off_y);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                int ix, iy;
                double tx, ty;
                const bool ok = strip_source_xy(q[k], yd, img_w, img_h, ix, iy, tx, ty);
                bilinear_taps(ok, tx, ty, img_w, img_h, off[t][k], fr[t][k]);
            }
        }
    }
    unsigned tap[kRows][4][4];
#pragma unroll
    for (int t = 0; t < kRows; ++t)
#pragma unroll
        for (int k = 0; k < 4; ++k) gather_taps(img, off[t][k], fr[t][k], row_bytes, last, tap[t][k]);
#pragma unroll
    for (int t = 0; t < kRows; ++t) {
        const int y = y_first + t;
        if (y >= y_end) break;  // wave-uniform
        unsigned px[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            px[k] = bilinear_blend(tap[t][k], fr[t][k]);
            if (kBlend) px[k] = blend_center(px[k], center, y - off_y, j0 + k - off_x, G.center_h, G.center_w, clast);
        }
        APAP_STORE_PX4(out + ((size_t)(y - G.row_begin) * (size_t)final_w) * 3 + (unsigned)j0 * 3u, px, npx);
    }
}

}  // namespace

namespace apap {

int warp_bilinear_launch(apap_ctx *ctx, const WarpGather &g, int batch, void *stream) {
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)((g.final_w + 255) / 256), (unsigned)((g.row_count + kWaves * kStripRows - 1) / (kWaves * kStripRows)),
                    (unsigned)batch);
    {
        ProfScope prof(ctx, APAP_PROF_WARP, s);
        if (g.center) hipLaunchKernelGGL((k_warp_bilinear<true, kStripRows>), grid, dim3(kWaves * 64), 0, s, g);
        else hipLaunchKernelGGL((k_warp_bilinear<false, kStripRows>), grid, dim3(kWaves * 64), 0, s, g);
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail((int)e, "k_warp_bilinear launch");
    return APAP_OK;
}

}  // namespace apap
