// Internal declarations shared by the host set-up, the kernel launchers and the C ABI.
#pragma once
#include <cstddef>
#include <cstdint>

#include <mutex>
#include <vector>

#include "../../include/apap_hip.h"

namespace apap {

struct ProfSpan {   // one bracketed kernel: two HIP events on the launch stream
    int slot;
    void *a, *b;
};

struct DevSlot {    // one pooled device buffer of the host-buffer entry points
    void *ptr = nullptr;
    size_t cap = 0;
    int dev = -1;
};
enum { S_TABLE, S_VERT, S_DENORM, S_H, S_WORK, S_W, S_IMG, S_OUT, S_MESHW, S_MESHH, S_HINV, S_STATUS, S_AUX, S_COUNT };

}  // namespace apap

// The context of include/apap_hip.h: options, profiling events, device-buffer pool.  Nothing else
// in the library is mutable after load.
struct apap_ctx {
    int opt[APAP_OPT_COUNT] = {APAP_VARIANT_AUTO, APAP_EIGEN_AUTO, 1, 0, 4096, 1, 1 << 20, 4096, 1, 0, 0, 30, 0, 0, APAP_SAMPLING_NEAREST};
    int short_chain = 1;    // apap_ctx_set_short_chain: K1's short weight chain where a chunk proves it (apap_exp_long.h)
    std::vector<apap::ProfSpan> spans;
    apap::DevSlot slots[apap::S_COUNT];
    std::mutex mu;   // serialises the host-buffer entry points that share this context's pool
    // overlap of PCIe and kernels in apap_local_warp / apap_local_stitch: three streams (upload, kernels,
    // download), their events, a small pinned buffer for what the host reads back mid-call; made on first use
    void *streams[3] = {nullptr, nullptr, nullptr};
    std::vector<void *> events;
    void *pinned = nullptr;
    size_t pinned_cap = 0;
    int pipe_dev = -1;
    // resident blocks of k_assemble_mfma's three forms on device k1_slots_dev (0: not asked yet), for the paired launch
    int k1_slots[3] = {0, 0, 0};
    int k1_slots_dev = -1;
    // two device words k_assemble_mfma counts its chunks in under APAP_OPT_PROFILE (apap_ctx_profile_k1_chunks); made on first use
    void *k1_chunk_counts = nullptr;
};

namespace apap {

// Option `which` of `ctx`, or its built-in default when ctx is NULL.
int opt(const apap_ctx *ctx, int which);

// Records a thread-local message for apap_last_error() and returns `code`.
int fail(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));

// Records "<what>: <hipGetErrorString>" and returns APAP_ERR_HIP.
int hip_fail(int hip_error, const char *what);

// Optional per-kernel timing (APAP_OPT_PROFILE / apap_ctx_profile_read): brackets the kernels
// launched in its scope with HIP events on `stream`, kept in the context.
struct ProfScope {
    ProfScope(apap_ctx *ctx, int slot, void *stream);
    ~ProfScope();
    ProfScope(const ProfScope &) = delete;
    ProfScope &operator=(const ProfScope &) = delete;

  private:
    apap_ctx *ctx_;
    void *stream_, *a_, *b_;
    int slot_;
    bool on_;
};

bool inv3_f64(const double in[9], double out[9]);
bool inv3_f32(const float in[9], float out[9]);

// ---- geometry of the solve launch (shared by launcher and workspace sizing) ----
struct SolvePlan {
    int variant;       // APAP_VARIANT_VALU or APAP_VARIANT_MFMA
    int cells_pad;     // cells rounded up to the cell tile of the variant
    int cell_tiles;    // grid.x
    int splits;        // grid.y: independent slices of the keypoint list
    int pts_per_split; // keypoints per slice (a multiple of 4)
    size_t moment_bytes;
};
SolvePlan plan_solve(int n, int cells, int variant, int batch, int want_waves, int plan_cells = 0, int moments = 30);
// Blocks of k_assemble_mfma that take two tiles of one split when `slots` blocks are resident at once (0: the plain 3-D grid).
int plan_pairs(int cell_tiles, int splits, int batch, int slots);

// ---- the warp in two phases on one workspace (the host-buffer entry points overlap PCIe with it) ----
constexpr int kWarpSetup = APAP_WARP_GEOMETRY | APAP_WARP_CELLS;   // lookup tables + cell inverses and fast records (and, if asked, source-row intervals)
constexpr int kWarpRows = APAP_WARP_GATHER;   // the gather kernel over canvas rows [row_begin, row_begin + row_count)
// apap_warp_rows_device / apap_stitch_device with a choice of phases.  With `d_src_rows` non-null the set-up also
// fills, per cell row, the interval of source rows its pixels can read (device ints [rows][2], then one flag word:
// bit 0 = irregular mesh, intervals void); the caller pre-sets the lower bounds to a large and the upper bounds to a
// small value.  *d_src_rows is set to the device address, or to NULL when this mesh has no such table; phase 0 only
// reports that address and launches nothing.
int warp_phase(apap_ctx *ctx, const uint8_t *d_img, int img_h, int img_w, const uint8_t *d_center, int center_h, int center_w,
               const float *d_Hfwd, int mesh_rows, int mesh_cols, const double *d_mesh_w, int n_w, const double *d_mesh_h,
               int n_h, int final_w, int final_h, int off_x, int off_y, uint8_t *d_out_band, float *d_Hinv_out, void *d_work,
               size_t work_bytes, int *d_status, void *stream, int row_begin, int row_count, int phase, int **d_src_rows);

// Where the set-up phases (kWarpSetup) leave the exact path's tables in a single-pair warp workspace, on the fast-table
// path and on the linear-scan path alike: hinv_pad [cells][APAP_HINV_STRIDE] f64, the cells' inverses widened, and lut
// [final_h + final_w] i32, canvas row -> cell row, then canvas column -> cell column (every entry a valid index, also where
// the set-up reported APAP_STATUS_INDEX).  Launches nothing.
struct WarpTables {
    const double *hinv_pad;
    const int *lut;
};
WarpTables warp_tables(void *d_work, int mesh_rows, int mesh_cols, int final_w, int final_h);

// The gather of a warp under APAP_SAMPLING_BILINEAR (apap_warp_bilinear.hip): what warp_impl hands its kernel once the set-up
// has run - the sizes it has checked, the exact path's tables, the pairs' strides (bytes; hinv in doubles).  Travels by value
// in the kernel argument.  center = NULL: no stitch.
struct WarpGather {
    const uint8_t *img;
    const uint8_t *center;
    uint8_t *out;               // row `row_begin` of pair 0's canvas
    const double *hinv_pad;
    const int *lut;
    int *status;
    long long img_stride, center_stride, out_stride, hinv_stride;
    int img_h, img_w, center_h, center_w, mesh_rows, mesh_cols, final_w, final_h, off_x, off_y, row_begin, row_count;
};
// k_warp_bilinear over rows [row_begin, row_begin + row_count) of `batch` canvases on `stream` (under the APAP_PROF_WARP slot).
int warp_bilinear_launch(apap_ctx *ctx, const WarpGather &g, int batch, void *stream);

// The panorama's third blend, the edge ramp, has entry points of its own (apap_panorama_ramp*): apap_panorama[_device] refuse
// APAP_PANORAMA_RAMP like any other unknown mode; only the gain entry points take it as a mode.
// The argument checks of the panorama's entry points (apap_panorama.hip) that need no device pointer; fills bounds[4] =
// W, H, OX, OY.  `ramp` is NULL for the entry points that take a mode (APAP_PANORAMA_MEAN or APAP_PANORAMA_PASTE) and
// points to the ramp width, 1 .. APAP_PANORAMA_MAX_RAMP, for those that take one (`mode` is APAP_PANORAMA_RAMP then).
int panorama_check(int center_h, int center_w, const int *img_h, const int *img_w, const int *mesh_rows, const int *mesh_cols,
                   const int *n_w, const int *n_h, const int *final_w, const int *final_h, const int *off_x, const int *off_y,
                   int n_layers, int mode, const int *ramp, int *bounds, const char *who);
// apap_panorama_device and apap_panorama_ramp_device: the set-up launches and k_panorama<mode>, with `who` in the messages.
int panorama_device(apap_ctx *ctx, const uint8_t *d_center, int center_h, int center_w, const uint8_t *const *d_imgs, const int *img_h,
                    const int *img_w, const float *const *d_Hfwd, const int *mesh_rows, const int *mesh_cols,
                    const double *const *d_mesh_w, const int *n_w, const double *const *d_mesh_h, const int *n_h, const int *final_w,
                    const int *final_h, const int *off_x, const int *off_y, int n_layers, int mode, const int *ramp, uint8_t *d_out,
                    void *d_work, size_t work_bytes, int *d_status, void *stream, const char *who);

// Gain compensation (apap_panorama.hip, DESIGN.md "Panorama, gain compensation").  The per-layer arguments of the device
// entry points as one value, and what a call is to do with them.
struct PanoGeometry {
    const uint8_t *d_center;
    int center_h, center_w;
    const uint8_t *const *d_imgs;
    const int *img_h, *img_w;
    const float *const *d_Hfwd;
    const int *mesh_rows, *mesh_cols;
    const double *const *d_mesh_w;
    const int *n_w;
    const double *const *d_mesh_h;
    const int *n_h, *final_w, *final_h, *off_x, *off_y;
    int n_layers;
};
enum { kPanoPlain = 0, kPanoGain, kPanoStats, kPanoAuto };   // the blend; the blend under gain_q; the statistics; statistics, device solve, blend
struct PanoJob {
    int what = kPanoPlain;
    int mode = APAP_PANORAMA_MEAN;
    const int *ramp = nullptr;      // as in panorama_check
    const int *band = nullptr;      // the two-band blend (mode APAP_PANORAMA_BAND, `ramp` set; kPanoPlain or kPanoGain): the blur's radius
    uint8_t *d_out = nullptr;
    const int *gain_q = nullptr;    // kPanoGain: n_layers + 1 HOST ints
    int step = 1;                   // kPanoStats, kPanoAuto
    unsigned long long *d_N = nullptr, *d_S = nullptr;
    double sigma_n = 10.0, sigma_g = 0.1;   // kPanoAuto
    double *d_g = nullptr;
    int *d_q = nullptr, *d_flag = nullptr;
};
// Every check (panorama_check, then panorama_gain_check, then the device pointers and the workspace), the set-up launches and
// the job's kernels on `stream`; does not wait.
int panorama_run(apap_ctx *ctx, const PanoGeometry &G, const PanoJob &J, void *d_work, size_t work_bytes, int *d_status, void *stream,
                 const char *who);
// The two-band blend's radius, 0 .. APAP_PANORAMA_MAX_BAND: the first check of its entry points, before panorama_check.
int panorama_band_check(int band, const char *who);
// apap_box_blur[_device]'s arguments that need no device: the radius, then a picture of at least 1 pixel and below 2 GiB.
int box_blur_check(int h, int w, int radius, const char *who);
// The gain arguments that need no device: n_views 2 .. 17 and, where the pointer is set, step 1 .. 64, every q 1024 .. 16383,
// sigmas finite and positive.
int panorama_gain_check(int n_views, const int *step, const int *gain_q, const double *sigma_n, const double *sigma_g, const char *who);
// The shared solve on the host: g and q of n_views views; returns the flag.
int panorama_gain_solve_host(const unsigned long long *N, const unsigned long long *S, int n_views, double sigma_n, double sigma_g,
                             double *g, int *q);

constexpr int kMoments = 30;       // distinct sums of A^T W^2 A

// The spectral weights (apap_spectral.hip).  spectral_run is apap_spectral_device; with sync_each = 1 (the host-buffer
// entry point) it waits for every restart cycle and enqueues no more once the device reports convergence.
int spectral_run(apap_ctx *ctx, const float *d_src, const float *d_dst, const float *d_c, const float *d_o, int n,
                 const double *d_F, const double *params, const float *d_Hg, const float *d_mask, double *d_segment,
                 float *d_ransac, float *d_original, double *d_info, int *d_status, void *d_work, size_t work_bytes,
                 void *stream, int sync_each);
// apap_spectral_em_device, with `sync_each` = 1 for the host-buffer entry point (each round's spectral cycles stop at
// convergence, as in spectral_run).
int spectral_em_run(apap_ctx *ctx, const float *d_src, const float *d_dst, const float *d_c_feats, const float *d_o_feats, int n,
                    const double *d_F, const double *spec_params, const double *model_params, int em_steps, const float *d_mask_in,
                    float *d_H, double *d_info, double *d_segment, float *d_ransac_mask, float *d_original_mask,
                    double *d_spec_info, int *d_status, void *d_work, size_t work_bytes, void *stream, int sync_each);
// apap_spectral_em_batch_device (apap_em_batch.hip), with `sync_each` = 1 for the host-buffer entry point: it waits for every
// restart cycle and stops a round's cycles once every problem of the batch reports convergence.
int spectral_em_batch_run(apap_ctx *ctx, const float *d_src, const float *d_dst, const float *d_c_feats, const float *d_o_feats,
                          const double *d_F, const float *d_mask_in, const int *pair_offset, int n_pairs, const int *pair_of,
                          const double *spec_params, const double *model_params, int n_problems, int em_steps, float *d_H,
                          double *d_info, double *d_segment, float *d_ransac_mask, float *d_original_mask, double *d_spec_info,
                          int *d_status, void *d_work, size_t work_bytes, void *stream, int sync_each);
// The argument checks of the batch entry points that need no device pointer.
int spectral_em_batch_check(const int *pair_offset, int n_pairs, const int *pair_of, const double *spec_params,
                            const double *model_params, int n_problems, int em_steps, const char *who);
// The argument checks of the robust moving DLT's entry points (apap_local_model.hip) that need no device pointer.
int local_model_check(int n, int cells, double gamma, double sigma, const double *params, const char *who);
// The argument checks of the descriptor matcher's entry points (apap_match.hip) that need no device pointer.
int match_check(const int *q_offset, const int *t_offset, int n_pairs, const char *who);
// The argument checks of the guided matcher's entry points (apap_match_guided.hip) that need no device pointer: match_check,
// then the kind and every pair's r2; and those of its records.
int guided_check(const int *q_offset, const int *t_offset, int n_pairs, int kind, const double *r2, const char *who);
int guided_records_check(int n, const void *model, int what, const char *who);
// The argument checks of the fundamental-matrix entry points (apap_fundamental.hip) that need no device pointer.
int fundamental_check(const int *pair_offset, int n_pairs, double thresh, int iterations, const char *who);
// The argument checks of the notch denoising's entry points (apap_denoise.hip) that need no device pointer: the planes of a
// call (the grid's second dimension) and the transform's lengths; the notch's parameters; all of a denoising call's.
constexpr int kDenoiseMaxPlanes = 65535;
int fft_check(int planes, int h, int w, const char *who);
int notch_check(int spacing, int r, int sn, const char *who);
int denoise_check(int n_images, int h, int w, int channels, int spacing, int r, int sn, int out_type, const char *who);
// The argument checks of the co-visibility and triangulation entry points (apap_sfm.hip) that need no device pointer.
int covis_check(const int *view_offset, int n_views, float eps, const char *who);
int triangulate_tracks_check(int max_tracks, int n_views, const int *dst_offset, int n_cams, int center_cam, const int *view_cam,
                             int min_views, const char *who);
// The dehazing (apap_dehaze.hip).  dehaze_check: the arguments that need no device pointer.  dehaze_run: every check, then the
// stages that the outputs asked for (any of d_dark, d_A, d_t, d_J may be null) on `stream`; does not wait.
int dehaze_check(int n_images, int h, int w, int channels, int radius, int omega_q, int t0_q, int refine, int eps, const char *who);
int dehaze_run(const uint8_t *d_imgs, int n_images, int h, int w, int channels, int radius, int omega_q, int t0_q, int refine, int eps,
               uint8_t *d_dark, uint8_t *d_A, uint16_t *d_t, uint8_t *d_J, void *d_work, size_t work_bytes, void *stream, const char *who);
// `bytes` rounded up to the 256-byte boundary on which every part of a workspace or pooled buffer starts.
inline size_t up256(size_t bytes) { return (bytes + 255) / 256 * 256; }

// The images of the feature front end (corner detection, descriptor extraction): their sides and their number in one call.
// 7: every reflect-101 index that a valid descriptor sample reads reflects once (apap_image_dev.h).  (kImage...: named apart
// from the global warp's own kMaxSide, 32767, which apap_image_warp.hip uses inside this namespace.)
constexpr int kImageMinSide = 7, kImageMaxSide = 32768, kMaxImages = 65535;
// Their per-image checks, one image a call so that each caller keeps its own order: corner_check looks at every image's
// sides and then at every image's channels, sift_check at image after image.
inline int image_sides_check(int m, int h, int w, const char *who) {
    if (h < kImageMinSide || h > kImageMaxSide || w < kImageMinSide || w > kImageMaxSide)
        return fail(APAP_ERR_INVALID_ARG, "%s: image %d is %d x %d (sides %d .. %d)", who, m, h, w, kImageMinSide, kImageMaxSide);
    return APAP_OK;
}
inline int image_channels_check(int m, int c, const char *who) {
    if (c != 1 && c != 3) return fail(APAP_ERR_INVALID_ARG, "%s: image %d has %d channels (1 = grey or 3 = BGR)", who, m, c);
    return APAP_OK;
}
// The argument checks of the descriptor extraction's entry points (apap_sift.hip) that need no device pointer.
int sift_check(const int *heights, const int *widths, const int *channels, int n_images, const int *pt_offset, const char *who);
// The 13 taps of the base image's Gaussian in float64 (apap_sift.hip): both descriptor kernels round them to float32.
void sift_taps_f64(double *g);
// sift_check, then the oriented entry points' own smallest side (apap_sift_orient.hip): 13, one reflection of the 25 x 25 patch.
constexpr int kOrientMinSide = 13;
int sift_orient_check(const int *heights, const int *widths, const int *channels, int n_images, const int *pt_offset, const char *who);
// The argument checks of the corner detector's entry points (apap_corner.hip) that need no device pointer.
int corner_check(const int *heights, const int *widths, const int *channels, int n_images, int max_corners, int radius,
                 int quality_permille, const char *who);
// The argument checks of the image pyramid's entry points (apap_pyramid.hip) that need no device pointer, and of its pack's.
int pyramid_check(const int *heights, const int *widths, const int *channels, int n_images, int n_levels, const char *who);
int pyramid_keypoints_check(int slab_rows, const int *counts, const int *scale_num, const int *scale_shift, const int *level_index,
                            int n_level_images, const char *who);
// The argument checks of the global warp's entry points (apap_image_warp.hip) that need no device pointer.
int image_warp_check(const int *base_h, const int *base_w, const int *src_h, const int *src_w, const double *M, const int *canvas_w,
                     const int *canvas_h, const int *off_x, const int *off_y, const int *direct_blend, int n_problems,
                     const long long *out_offset, const char *who);
// Set-up and the dense M (n x n doubles) on `stream`.
int spectral_affinity_run(const float *d_src, const float *d_dst, const float *d_c, const float *d_o, int n, const double *d_F,
                          const double *params, double *d_M, void *d_work, size_t work_bytes, void *stream);

}  // namespace apap

#if defined(__HIP__)
// ---- device helpers shared by the kernel sources ----
#include <hip/hip_runtime.h>

namespace apap {

// 1 / x to <= 1 ulp (v_rcp_f64 + two Newton steps: 5 instructions where the IEEE division sequence is 12).
// inf / NaN / 0 in -> NaN or inf out; the callers test their operands.
__device__ __forceinline__ double rcp_full(double x) {
    double r = __builtin_amdgcn_rcp(x);
    r = fma(fma(-x, r, 1.0), r, r);
    return fma(fma(-x, r, 1.0), r, r);
}

// --------------------------------------------------------------------------------
// 3x3 inverse in float64 by LU with partial pivoting (what numpy.linalg.inv does for a
// float32 input: dgesv on the widened matrix, result cast back - apap.py:203,252).
// Branch-free row swaps so that everything stays in registers.  Returns false on an
// exactly-zero pivot.
// --------------------------------------------------------------------------------
__device__ __forceinline__ void cswap(bool c, double &x, double &y) {
    const double tx = c ? y : x, ty = c ? x : y;
    x = tx;
    y = ty;
}

// a / b with 1 / b in hand (rb = rcp_full(b)): the product and one residual correction - the Markstein sequence, which
// returns the correctly rounded quotient except in a vanishing share of cases (then 1 ulp off); `plain` false (a pivot that
// is zero, denormal, huge or NaN): the IEEE division.  Twelve of these replace twelve ~30-instruction division sequences in
// inv3, which runs once per cell in the solve's tail and in the warp's set-up.
template <bool kFast>
__device__ __forceinline__ double quot(double a, double b, double rb) {
    if (!kFast) return a / b;
    const double q0 = a * rb;
    return fma(fma(-b, q0, a), rb, q0);
}

// `plain` (kFast only): every pivot was an ordinary number - the reciprocal-based quotients are valid
template <bool kFast>
__device__ __forceinline__ bool inv3_impl(const double *m, double *out, bool &plain) {
    double a00 = m[0], a01 = m[1], a02 = m[2], a10 = m[3], a11 = m[4], a12 = m[5], a20 = m[6], a21 = m[7], a22 = m[8];
    double b00 = 1, b01 = 0, b02 = 0, b10 = 0, b11 = 1, b12 = 0, b20 = 0, b21 = 0, b22 = 1;
    bool ok = true, p0, p1;
    double r0, r1;
    // column 0 pivot: first maximal |a_i0|
    {
        const bool s1 = fabs(a10) > fabs(a00);
        cswap(s1, a00, a10); cswap(s1, a01, a11); cswap(s1, a02, a12);
        cswap(s1, b00, b10); cswap(s1, b01, b11); cswap(s1, b02, b12);
        const bool s2 = fabs(a20) > fabs(a00);
        cswap(s2, a00, a20); cswap(s2, a01, a21); cswap(s2, a02, a22);
        cswap(s2, b00, b20); cswap(s2, b01, b21); cswap(s2, b02, b22);
        // the two conditional swaps above pick the max but may permute the two
        // non-pivot rows differently from LAPACK; the inverse does not depend on it
        // beyond rounding at the 1e-16 level.
        ok = ok && (a00 != 0.0);
        p0 = fabs(a00) >= 1e-290 && fabs(a00) <= 1e290;
        r0 = kFast ? rcp_full(a00) : 0.0;
        const double l1 = quot<kFast>(a10, a00, r0), l2 = quot<kFast>(a20, a00, r0);
        a11 = fma(-l1, a01, a11); a12 = fma(-l1, a02, a12);
        b10 = fma(-l1, b00, b10); b11 = fma(-l1, b01, b11); b12 = fma(-l1, b02, b12);
        a21 = fma(-l2, a01, a21); a22 = fma(-l2, a02, a22);
        b20 = fma(-l2, b00, b20); b21 = fma(-l2, b01, b21); b22 = fma(-l2, b02, b22);
    }
    {
        const bool s = fabs(a21) > fabs(a11);
        cswap(s, a11, a21); cswap(s, a12, a22);
        cswap(s, b10, b20); cswap(s, b11, b21); cswap(s, b12, b22);
        ok = ok && (a11 != 0.0);
        p1 = fabs(a11) >= 1e-290 && fabs(a11) <= 1e290;
        r1 = kFast ? rcp_full(a11) : 0.0;
        const double l = quot<kFast>(a21, a11, r1);
        a22 = fma(-l, a12, a22);
        b20 = fma(-l, b10, b20); b21 = fma(-l, b11, b21); b22 = fma(-l, b12, b22);
    }
    ok = ok && (a22 != 0.0);
    const bool p2 = fabs(a22) >= 1e-290 && fabs(a22) <= 1e290;
    const double r2 = kFast ? rcp_full(a22) : 0.0;
    plain = p0 && p1 && p2;
    // back substitution, column by column
    const double x20 = quot<kFast>(b20, a22, r2), x21 = quot<kFast>(b21, a22, r2), x22 = quot<kFast>(b22, a22, r2);
    const double x10 = quot<kFast>(fma(-a12, x20, b10), a11, r1), x11 = quot<kFast>(fma(-a12, x21, b11), a11, r1),
                 x12 = quot<kFast>(fma(-a12, x22, b12), a11, r1);
    const double x00 = quot<kFast>(fma(-a02, x20, fma(-a01, x10, b00)), a00, r0);
    const double x01 = quot<kFast>(fma(-a02, x21, fma(-a01, x11, b01)), a00, r0);
    const double x02 = quot<kFast>(fma(-a02, x22, fma(-a01, x12, b02)), a00, r0);
    out[0] = x00; out[1] = x01; out[2] = x02;
    out[3] = x10; out[4] = x11; out[5] = x12;
    out[6] = x20; out[7] = x21; out[8] = x22;
    return ok;
}

// 3 x 3 inverse by LU with partial pivoting (what numpy.linalg.inv does in float64, apap.py:203).  The common path takes its
// twelve quotients from three reciprocals; a wave that holds a cell with a zero, denormal, huge or NaN pivot redoes its cells
// with IEEE divisions (wave-uniform branch).
__device__ __forceinline__ bool inv3(const double *m, double *out) {
    bool plain;
    bool ok = inv3_impl<true>(m, out, plain);
    if (!__all(plain)) {
        double o2[9];
        bool dummy;
        const bool ok2 = inv3_impl<false>(m, o2, dummy);
#pragma unroll
        for (int k = 0; k < 9; ++k) out[k] = plain ? out[k] : o2[k];
        ok = plain ? ok : ok2;
    }
    return ok;
}

}  // namespace apap
#endif  // __HIP__
