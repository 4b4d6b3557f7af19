// SIFT descriptors at given keypoints: what cv.SIFT.create().compute(img, [cv.KeyPoint(x, y, 1) ...]) defines (OpenCV 4.x,
// calcSIFTDescriptor for size 1, angle -1, octave 0), restated in DESIGN.md "Descriptor extraction" and, operation by
// operation, in tests/sift_spec.py.
//
// The descriptor of one keypoint depends on 49 samples of the Gaussian base image (offsets |i|, |j| <= 3 around the rounded
// keypoint), each a central difference: a 9 x 9 patch of the base image, which is a 13-tap separable blur of the grey image:
// a 21 x 21 patch of the grey image.  The base image is never built.
//
// k_sift_describe: one wave per keypoint, four keypoints per block of 256 threads, a private LDS region per wave.
//   1. the 21 x 21 grey patch, reflect-101 on the indices, BGR -> grey in integers on the fly;
//   2. the horizontal blur to 21 x 9, the vertical blur to 9 x 9: the taps ascending from 0, a multiply and an add per tap -
//      the very sums of a full-image blur, so the patch equals the full image's base image bit for bit;
//   3. lane k < 49 makes sample k: gradient, magnitude x window weight, orientation bin and its fraction, and the four
//      spatial shares (OpenCV's v1 = v * f, v0 = v - v1);
//   4. every lane gathers two of the 128 bins (lane and lane + 64: the same column and orientation, two rows apart) in one
//      pass over the samples in ascending order, each adding its share (or 0) - a fixed order, no atomics;
//   (steps 1, 2 and 5, the image table and atan2 are apap_sift_dev.h's, shared with apap_sift_orient.hip)
//   5. sum of squares by a fixed binary tree (bins b and b + 64, then lanes l and l ^ 32, ^ 16 .. ^ 1), clamp at 0.2 of the
//      norm, the same tree again, scale to 512, round, saturate; two coalesced 256-byte stores.
// Every operation is one IEEE float32 operation (the sources are built with -ffp-contract=off; sqrt and the division are the
// correctly rounded ones), atan2 is the polynomial below: the bytes are a function of the image and the coordinates alone.
//
// A batch is the same launch: a table of image descriptors in device memory, the keypoints concatenated; a wave finds its
// image by bisection of the table's keypoint offsets.  The single call is the batch of one.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <cstdint>
#include <vector>

#include "apap_internal.h"
#include "apap_sift_dev.h"

namespace {

using apap::SiftImage;

constexpr int kDim = apap::kSiftDim;
constexpr int kSamples = APAP_SIFT_SAMPLES;
constexpr int kTaps = apap::kSiftTaps;
constexpr int kPatch = APAP_SIFT_PATCH;
constexpr int kBase = kPatch - (kTaps - 1);        // 9: the base-image patch
constexpr int kPerBlock = apap::kSiftPerBlock;
constexpr int kThreads = apap::kSiftThreads;
constexpr int kWinCols = APAP_SIFT_WINDOW_COLS;
constexpr int kMaxRows = 1 << 24;
static_assert(kDim == 128 && kSamples == 49 && kTaps == 13 && kPatch == 21 && kBase == 9 && kPerBlock == 4, "the lane mapping below is for these");

struct SiftConst {   // the constants of the kernel, a kernel argument: made on the host in float64, rounded to float32
    float taps[kTaps];
    float w[kSamples], fr[kSamples], fc[kSamples];   // window weight, fractions of rbin and cbin
    int r0[kSamples], c0[kSamples];                  // floor(rbin), floor(cbin): -1 .. 3
};

// The 49 x 8 window table (include/apap_hip.h): rbin, cbin, weight, frac(rbin), frac(cbin), floor(rbin), floor(cbin), 0.
void window_f64(double *t) {
    const double ang = 361.0 * (M_PI / 180.0), hist_width = 1.5;
    const double cs = std::cos(ang) / hist_width, sn = std::sin(ang) / hist_width;
    int k = 0;
    for (int i = -3; i <= 3; ++i)
        for (int j = -3; j <= 3; ++j, ++k) {
            const double c_rot = j * cs - i * sn, r_rot = j * sn + i * cs;
            const double rbin = r_rot + 1.5, cbin = c_rot + 1.5;
            double *row = t + k * kWinCols;
            row[0] = rbin;
            row[1] = cbin;
            row[2] = std::exp(-(c_rot * c_rot + r_rot * r_rot) / 8.0);
            row[3] = rbin - std::floor(rbin);
            row[4] = cbin - std::floor(cbin);
            row[5] = std::floor(rbin);
            row[6] = std::floor(cbin);
            row[7] = 0.0;
        }
}

SiftConst make_const() {
    SiftConst K;
    double g[kTaps], t[kSamples * kWinCols];
    apap::sift_taps_f64(g);
    window_f64(t);
    for (int i = 0; i < kTaps; ++i) K.taps[i] = (float)g[i];
    for (int k = 0; k < kSamples; ++k) {
        K.w[k] = (float)t[k * kWinCols + 2];
        K.fr[k] = (float)t[k * kWinCols + 3];
        K.fc[k] = (float)t[k * kWinCols + 4];
        K.r0[k] = (int)t[k * kWinCols + 5];
        K.c0[k] = (int)t[k * kWinCols + 6];
    }
    return K;
}

__global__ __launch_bounds__(kThreads) void k_sift_describe(const SiftImage *__restrict__ tab, int n_images,
                                                            const float *__restrict__ pts, float *__restrict__ out, int k_begin,
                                                            int k_end, const SiftConst K) {
    __shared__ float s_patch[kPerBlock][kPatch * kPatch];
    __shared__ float s_hb[kPerBlock][kPatch * kBase];
    __shared__ float s_base[kPerBlock][kBase * kBase];
    __shared__ float s_v[kPerBlock][kSamples * 4];
    __shared__ float s_fo[kPerBlock][kSamples];
    __shared__ int s_o0[kPerBlock][kSamples];

    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const long long row = (long long)k_begin + (long long)blockIdx.x * kPerBlock + wv;
    const bool live = row < k_end;

    const SiftImage I = apap::sift_image_of(tab, n_images, row, live);   // the image of this keypoint

    // pt = (rint(x), rint(y)), round half to even; a keypoint that has no valid sample (or a non-finite coordinate) is all zeros
    int px = 0, py = 0;
    bool work = false;
    if (live) {
        const float fx = rintf(pts[2 * row]), fy = rintf(pts[2 * row + 1]);
        work = fx > -3.f && fx < (float)(I.w + 2) && fy > -3.f && fy < (float)(I.h + 2);   // false for NaN
        if (work) {
            px = (int)fx;
            py = (int)fy;
        }
    }
    float *patch = s_patch[wv], *hb = s_hb[wv], *base = s_base[wv];

    apap::sift_base_patch<kPatch>(I, py, px, work, lane, K.taps, patch, hb, base);
    if (work && lane < kSamples) {
        const int k = lane, i = k / 7 - 3, j = k - (k / 7) * 7 - 3;
        const int r = 4 + i, c = 4 + j;
        const bool valid = py + i > 0 && py + i < I.h - 1 && px + j > 0 && px + j < I.w - 1;
        const float dx = base[r * kBase + c + 1] - base[r * kBase + c - 1];
        const float dy = base[(r - 1) * kBase + c] - base[(r + 1) * kBase + c];
        float mag = sqrtf(dx * dx + dy * dy) * K.w[k];
        if (!valid) mag = 0.f;
        const float obin = (apap::sift_atan2_deg(dy, dx) - 361.f) * 2.222222276e-02f;   // 8 / 360
        const float o0f = floorf(obin), fo = obin - o0f;                     // o0f in -9 .. -1
        const float fr = K.fr[k], fc = K.fc[k];
        const float v_r1 = mag * fr, v_r0 = mag - v_r1;
        const float v11 = v_r1 * fc, v10 = v_r1 - v11, v01 = v_r0 * fc, v00 = v_r0 - v01;
        s_v[wv][4 * k + 0] = v00;
        s_v[wv][4 * k + 1] = v01;
        s_v[wv][4 * k + 2] = v10;
        s_v[wv][4 * k + 3] = v11;
        s_fo[wv][k] = fo;
        s_o0[wv][k] = ((int)o0f + 16) & 7;
    }
    __syncthreads();
    if (!live) return;

    // bins b = lane and lane + 64: (r * 4 + c) * 8 + o with the same column c and orientation o, rows r and r + 2
    float h[2] = {0.f, 0.f};
    if (work) {
        const int r = lane >> 5, c = (lane >> 3) & 3, o = lane & 7;
        for (int k = 0; k < kSamples; ++k) {
            const int dr = r - K.r0[k], dc = c - K.c0[k];
            const int d = (o - s_o0[wv][k]) & 7;
            const float fo = s_fo[wv][k];
            const bool col = (unsigned)dc < 2u;
#pragma unroll
            for (int half = 0; half < 2; ++half) {
                const int drh = dr + 2 * half;
                const float v = col && (unsigned)drh < 2u ? s_v[wv][4 * k + 2 * drh + dc] : 0.f;
                const float v1 = v * fo;
                h[half] = h[half] + (d == 0 ? v - v1 : d == 1 ? v1 : 0.f);
            }
        }
    }
    apap::sift_finish(h[0], h[1], out, row, lane);
}

}  // namespace

namespace apap {

void sift_taps_f64(double *g) {
    const double sigma2 = 1.6 * 1.6 - 0.5 * 0.5;   // sigma = sqrt(1.6^2 - 0.5^2)
    double sum = 0.0;
    for (int t = 0; t < kTaps; ++t) {
        g[t] = std::exp(-(double)((t - 6) * (t - 6)) / (2.0 * sigma2));
        sum += g[t];
    }
    for (int t = 0; t < kTaps; ++t) g[t] /= sum;
}

// The argument checks of the descriptor extraction's entry points that need no device pointer.
int sift_check(const int *heights, const int *widths, const int *channels, int n_images, const int *pt_offset, const char *who) {
    if (!heights || !widths || !channels || !pt_offset) return apap::fail(APAP_ERR_INVALID_ARG, "%s: null heights / widths / channels / pt_offset", who);
    if (n_images < 1 || n_images > apap::kMaxImages)
        return apap::fail(APAP_ERR_INVALID_ARG, "%s: n_images = %d (1 .. %d)", who, n_images, apap::kMaxImages);
    if (pt_offset[0] < 0) return apap::fail(APAP_ERR_INVALID_ARG, "%s: pt_offset[0] = %d: negative", who, pt_offset[0]);
    for (int m = 0; m < n_images; ++m) {
        if (int rc = apap::image_sides_check(m, heights[m], widths[m], who)) return rc;
        if (int rc = apap::image_channels_check(m, channels[m], who)) return rc;
        const long long n = (long long)pt_offset[m + 1] - pt_offset[m];
        if (n < 1 || n > kMaxRows)
            return apap::fail(APAP_ERR_INVALID_ARG, "%s: image %d: %lld keypoints (offsets must increase strictly, an image holds "
                                                    "1 .. 2^24 keypoints)", who, m, n);
    }
    return APAP_OK;
}

}  // namespace apap

extern "C" {

int apap_sift_window(float *out) {
    if (!out) return apap::fail(APAP_ERR_INVALID_ARG, "apap_sift_window: null argument");
    double t[kSamples * kWinCols];
    window_f64(t);
    for (int k = 0; k < kSamples * kWinCols; ++k) out[k] = (float)t[k];
    return APAP_OK;
}

int apap_sift_taps(float *out) {
    if (!out) return apap::fail(APAP_ERR_INVALID_ARG, "apap_sift_taps: null argument");
    double g[kTaps];
    apap::sift_taps_f64(g);
    for (int t = 0; t < kTaps; ++t) out[t] = (float)g[t];
    return APAP_OK;
}

size_t apap_sift_workspace_bytes(int n_images) { return n_images < 1 || n_images > apap::kMaxImages ? 0 : apap::sift_table_bytes(n_images); }

int apap_sift_describe_batch_device(apap_ctx *ctx, const uint8_t *const *d_imgs, const int *heights, const int *widths,
                                    const int *channels, int n_images, const float *d_pts, const int *pt_offset, float *d_out,
                                    void *d_work, size_t work_bytes, void *stream) {
    const char *who = "apap_sift_describe_batch_device";
    (void)ctx;
    int rc = apap::sift_check(heights, widths, channels, n_images, pt_offset, who);
    if (rc) return rc;
    if (!d_pts || !d_out) return apap::fail(APAP_ERR_INVALID_ARG, "%s: null device pointer", who);
    if (((uintptr_t)d_pts & 7) != 0 || ((uintptr_t)d_out & 3) != 0)
        return apap::fail(APAP_ERR_INVALID_ARG, "%s: keypoints must be 8-byte and descriptors 4-byte aligned", who);
    hipStream_t s = (hipStream_t)stream;
    if ((rc = apap::sift_table_upload(d_imgs, heights, widths, channels, n_images, pt_offset, d_work, work_bytes, s, who))) return rc;
    const int k_begin = pt_offset[0], k_end = pt_offset[n_images];
    const unsigned blocks = (unsigned)(((long long)k_end - k_begin + kPerBlock - 1) / kPerBlock);
    const SiftConst K = make_const();
    hipLaunchKernelGGL(k_sift_describe, dim3(blocks), dim3(kThreads), 0, s, (const SiftImage *)d_work, n_images, d_pts, d_out, k_begin,
                       k_end, K);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return apap::hip_fail(e, "apap_sift_describe_batch_device launch");
    return APAP_OK;
}

int apap_sift_describe_device(apap_ctx *ctx, const uint8_t *d_img, int h, int w, int channels, const float *d_pts, int n, float *d_out,
                              void *d_work, size_t work_bytes, void *stream) {
    const int off[2] = {0, n};
    return apap_sift_describe_batch_device(ctx, &d_img, &h, &w, &channels, 1, d_pts, off, d_out, d_work, work_bytes, stream);
}

}  // extern "C"
