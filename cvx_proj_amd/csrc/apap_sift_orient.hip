// Keypoint orientation and the SIFT descriptor at an orientation: OpenCV 4.x's calcOrientationHist and calcSIFTDescriptor for a
// size-1, octave-0 keypoint, restated in DESIGN.md "Keypoint orientation" and, operation by operation, in
// tests/sift_orient_spec.py.  apap_sift.hip keeps the unoriented descriptor (angle -1) with its constant sample tables.
//
// A descriptor at an angle reads the 121 samples |i|, |j| <= 5 of the Gaussian base image around the rounded keypoint, each
// a central difference: a 13 x 13 patch of the base image, a 25 x 25 patch of the grey image.  The orientation reads the 25
// samples |i|, |j| <= 2 of the same patch.
//
// k_sift_orient<orient, describe>: one wave per keypoint, four keypoints per block of 256 threads, a private LDS region per
// wave (apap_sift_dev.h has the steps shared with k_sift_describe).
//   1. the 25 x 25 grey patch; 2. the blur to 25 x 13 and to 13 x 13: the full image's base image bit for bit;
//   3. (orient) lanes < 25 make the orientation samples (weight x magnitude, bin = rint(angle / 10) wrapped); lanes < 36 each
//      walk the 25 samples in order and add those of their bin; OpenCV's circular smoothing through LDS; the first largest bin
//      by a wave reduction on (value, lowest index); the parabola through its neighbours; angle = 360 - 10 bin;
//   4. (describe) cos and sin of ori = 360 - angle from one polynomial each after an exact reduction by quadrant; each lane
//      makes samples lane and lane + 64 of the 121: rotated bin coordinates, their floors and fractions, magnitude x window
//      weight, orientation bin, the four spatial shares; the records go to LDS as arrays over the samples (a lane writes
//      consecutive words; a gathering wave reads one word of each array, in different banks: no conflict either way);
//   5. every lane owns bins lane and lane + 64 and walks the 121 records in ascending order - a fixed order, no atomics;
//   6. the shared tree sums, clamp, scale and stores.
// The records reuse the LDS of the grey patch and the horizontal blur, which are dead by then.  Every operation is one IEEE
// float32 operation (-ffp-contract=off; sqrt and the division are the correctly rounded ones); atan2, sin and cos are
// polynomials of this library: the bytes are a function of the image, the coordinates and the angles alone.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <cstdint>

#include "apap_internal.h"
#include "apap_sift_dev.h"

namespace {

using apap::SiftImage;

constexpr int kPerBlock = apap::kSiftPerBlock;
constexpr int kThreads = apap::kSiftThreads;
constexpr int kTaps = apap::kSiftTaps;
constexpr int kPatch = APAP_SIFT_ORIENT_PATCH;
constexpr int kBase = kPatch - (kTaps - 1);   // 13: the base-image patch, the keypoint at (6, 6)
constexpr int kOriSamples = APAP_SIFT_ORIENT_SAMPLES, kOriBins = 36;
constexpr int kSamples = APAP_SIFT_DESCR_SAMPLES;
static_assert(kPatch == 25 && kBase == 13 && kOriSamples == 25 && kSamples == 121 && kPerBlock == 4, "the lane mappings below are for these");

// one wave's LDS, in floats: the grey patch, the horizontal blur, the base patch; later, over the first two, the orientation's
// scratch and then the sample records
constexpr int kAtHb = kPatch * kPatch, kAtBase = kAtHb + kPatch * kBase, kWaveLds = kAtBase + kBase * kBase;
constexpr int kAtTerm = 0, kAtBin = 32, kAtHist = 64, kAtSmooth = 128;           // orientation: 25, 25, 36, 36 words
constexpr int kAtV = 0, kAtFo = 4 * kSamples, kAtKey = 5 * kSamples;             // records: v00 v01 v10 v11 | fo | key
static_assert(6 * kSamples <= kAtBase && kAtSmooth + kOriBins <= kAtBase, "the records and the orientation's scratch must not reach the base patch");
static_assert((kSamples % 32) != 0 && (2 * kSamples % 32) != 0 && (3 * kSamples % 32) != 0 && (kSamples % 32) != (3 * kSamples % 32),
              "the four share arrays of one sample must lie in four banks");

struct OrientConst {   // the constants of the kernel, a kernel argument: made on the host in float64, rounded to float32
    float taps[kTaps];
    float wo[kOriSamples];   // the orientation window
    float wd[kSamples];      // the descriptor window
};

void orient_window_f64(double *w) {
    int k = 0;
    for (int i = -2; i <= 2; ++i)
        for (int j = -2; j <= 2; ++j, ++k) w[k] = std::exp(-(double)(i * i + j * j) / (2.0 * 0.75 * 0.75));
}

void descr_window_f64(double *w) {   // exp(-(c_rot^2 + r_rot^2) / 8), c_rot^2 + r_rot^2 = (i^2 + j^2) / 1.5^2 at every angle
    int k = 0;
    for (int i = -5; i <= 5; ++i)
        for (int j = -5; j <= 5; ++j, ++k) w[k] = std::exp(-(double)(i * i + j * j) / (2.25 * 8.0));
}

OrientConst make_const() {
    OrientConst K;
    double g[kTaps], wo[kOriSamples], wd[kSamples];
    apap::sift_taps_f64(g);
    orient_window_f64(wo);
    descr_window_f64(wd);
    for (int i = 0; i < kTaps; ++i) K.taps[i] = (float)g[i];
    for (int k = 0; k < kOriSamples; ++k) K.wo[k] = (float)wo[k];
    for (int k = 0; k < kSamples; ++k) K.wd[k] = (float)wd[k];
    return K;
}

// cos and sin of an angle in degrees in [0, 360).  q = its quadrant, r = ori - 90 q in [0, 90) exactly; x = r pi / 180;
// sin x = x S(x^2), cos x = C(x^2), the Taylor polynomials of degree 11 and 12 by Horner (|error| <= 2.1e-7 on the whole
// circle, tests/test_sift_orient_spec.py); then the quadrant.  0, 90, 180 and 270 give exactly 0 and +-1.
__device__ __forceinline__ void sincos_deg(float ori, float *cs_out, float *sn_out) {
    const int q = (ori >= 90.f) + (ori >= 180.f) + (ori >= 270.f);
    const float r = ori - 90.f * (float)q;
    const float x = r * 1.745329238e-02f, s = x * x;
    float p = -2.505210794e-08f;
    p = p * s + 2.755731884e-06f;
    p = p * s + -1.984127011e-04f;
    p = p * s + 8.333333768e-03f;
    p = p * s + -1.666666716e-01f;
    p = p * s + 1.f;
    const float sn = x * p;
    float c = 2.087675588e-09f;
    c = c * s + -2.755731998e-07f;
    c = c * s + 2.480158764e-05f;
    c = c * s + -1.388888923e-03f;
    c = c * s + 4.166666791e-02f;
    c = c * s + -0.5f;
    c = c * s + 1.f;
    *cs_out = q == 0 ? c : q == 1 ? -sn : q == 2 ? -c : sn;
    *sn_out = q == 0 ? sn : q == 1 ? c : q == 2 ? -sn : -c;
}

template <bool kOrient, bool kDescribe>
__global__ __launch_bounds__(kThreads) void k_sift_orient(const SiftImage *__restrict__ tab, int n_images, const float *__restrict__ pts,
                                                          const float *__restrict__ angles_in, float *__restrict__ angles_out,
                                                          float *__restrict__ out, int k_begin, int k_end, const OrientConst K) {
    __shared__ float s_lds[kPerBlock][kWaveLds];

    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const long long row = (long long)k_begin + (long long)blockIdx.x * kPerBlock + wv;
    const bool live = row < k_end;

    const SiftImage I = apap::sift_image_of(tab, n_images, row, live);

    // pt = (rint(x), rint(y)), round half to even.  No work: a keypoint that cannot have a valid sample, a non-finite
    // coordinate, a given angle that is not in [0, 360] - angle 0 and a zero row.
    int px = 0, py = 0;
    bool work = false;
    float angle = 0.f;
    if (live) {
        const float fx = rintf(pts[2 * row]), fy = rintf(pts[2 * row + 1]);
        work = fx > -5.f && fx < (float)(I.w + 4) && fy > -5.f && fy < (float)(I.h + 4);   // false for NaN
        if (!kOrient) {
            const float a = angles_in[row];
            work = work && a >= 0.f && a <= 360.f;                                          // false for NaN
            if (work) angle = a;
        }
        if (work) {
            px = (int)fx;
            py = (int)fy;
        }
    }
    float *S = s_lds[wv], *base = S + kAtBase;
    apap::sift_base_patch<kPatch>(I, py, px, work, lane, K.taps, S, S + kAtHb, base);

    if (kOrient) {
        float *o_term = S + kAtTerm, *o_hist = S + kAtHist, *o_smooth = S + kAtSmooth;
        int *o_bin = (int *)(S + kAtBin);
        if (work && lane < kOriSamples) {
            const int i = lane / 5 - 2, j = lane - (lane / 5) * 5 - 2;
            const int r = 6 + i, c = 6 + j;
            const bool valid = py + i > 0 && py + i < I.h - 1 && px + j > 0 && px + j < I.w - 1;
            const float dx = base[r * kBase + c + 1] - base[r * kBase + c - 1];
            const float dy = base[(r - 1) * kBase + c] - base[(r + 1) * kBase + c];
            int b = (int)rintf(apap::sift_atan2_deg(dy, dx) * 0.1f);   // 36 / 360
            if (b >= kOriBins) b -= kOriBins;
            o_term[lane] = K.wo[lane] * sqrtf(dx * dx + dy * dy);
            o_bin[lane] = valid ? b : -1;
        }
        __syncthreads();
        float t = 0.f;
        if (work && lane < kOriBins) {
            for (int k = 0; k < kOriSamples; ++k)
                if (o_bin[k] == lane) t = t + o_term[k];
            o_hist[lane] = t;
        }
        __syncthreads();
        float sm = -1.f;   // below every smoothed bin: lanes 36 .. 63 never win
        if (work && lane < kOriBins) {
            const float tm2 = o_hist[(lane + 34) % kOriBins], tp2 = o_hist[(lane + 2) % kOriBins];
            const float tm1 = o_hist[(lane + 35) % kOriBins], tp1 = o_hist[(lane + 1) % kOriBins];
            sm = (tm2 + tp2) * 0.0625f + (tm1 + tp1) * 0.25f + t * 0.375f;
            o_smooth[lane] = sm;
        }
        __syncthreads();
        float best = sm;
        int at = lane;
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {   // the largest value, the lowest index among equals: the same pair in every lane
            const float ov = __shfl_xor(best, m);
            const int oa = __shfl_xor(at, m);
            if (ov > best || (ov == best && oa < at)) {
                best = ov;
                at = oa;
            }
        }
        if (work) {
            const float l = o_smooth[(at + 35) % kOriBins], r = o_smooth[(at + 1) % kOriBins];
            const float num = 0.5f * (l - r), den = (l - 2.f * best) + r;
            const float off = den == 0.f ? 0.f : num / den;
            float bin = (float)at + off;
            bin = bin < 0.f ? 36.f + bin : bin >= 36.f ? bin - 36.f : bin;
            angle = 360.f - 10.f * bin;
            if (fabsf(angle - 360.f) < FLT_EPSILON) angle = 0.f;
        }
        if (live && lane == 0) angles_out[row] = angle;
        __syncthreads();   // the records overwrite the orientation's scratch
    }
    if (!kDescribe) return;

    float *r_v = S + kAtV, *r_fo = S + kAtFo;
    int *r_key = (int *)(S + kAtKey);
    if (work) {
        float ori = 360.f - angle;
        if (fabsf(ori - 360.f) < FLT_EPSILON) ori = 0.f;
        float cs, sn;
        sincos_deg(ori, &cs, &sn);
        for (int k = lane; k < kSamples; k += 64) {
            const int i = k / 11 - 5, j = k - (k / 11) * 11 - 5;
            const int r = 6 + i, c = 6 + j;
            const bool valid = py + i > 0 && py + i < I.h - 1 && px + j > 0 && px + j < I.w - 1;
            const float fi = (float)i, fj = (float)j;
            const float c_rot = (fj * cs - fi * sn) / 1.5f, r_rot = (fj * sn + fi * cs) / 1.5f;
            const float rbin = r_rot + 1.5f, cbin = c_rot + 1.5f;
            const bool counted = valid && rbin > -1.f && rbin < 4.f && cbin > -1.f && cbin < 4.f;
            int key = -1;   // a sample that does not count: the gather skips it
            if (counted) {
                const float dx = base[r * kBase + c + 1] - base[r * kBase + c - 1];
                const float dy = base[(r - 1) * kBase + c] - base[(r + 1) * kBase + c];
                const float mag = sqrtf(dx * dx + dy * dy) * K.wd[k];
                const float obin = (apap::sift_atan2_deg(dy, dx) - ori) * 2.222222276e-02f;   // 8 / 360
                const float r0f = floorf(rbin), c0f = floorf(cbin), o0f = floorf(obin);       // -1 .. 3, -1 .. 3, -8 .. 8
                const float fr = rbin - r0f, fc = cbin - c0f;
                const float v_r1 = mag * fr, v_r0 = mag - v_r1;
                const float v11 = v_r1 * fc, v10 = v_r1 - v11, v01 = v_r0 * fc, v00 = v_r0 - v01;
                r_v[0 * kSamples + k] = v00;
                r_v[1 * kSamples + k] = v01;
                r_v[2 * kSamples + k] = v10;
                r_v[3 * kSamples + k] = v11;
                r_fo[k] = obin - o0f;
                key = (((int)o0f + 16) & 7) | (((int)r0f + 1) << 3) | (((int)c0f + 1) << 6);
            }
            r_key[k] = key;
        }
    }
    __syncthreads();
    if (!live) return;

    // bins b = lane and lane + 64: (r * 4 + c) * 8 + o with the same column c and orientation o, rows r and r + 2
    float h[2] = {0.f, 0.f};
    if (work) {
        const int r = lane >> 5, c = (lane >> 3) & 3, o = lane & 7;
        for (int k = 0; k < kSamples; ++k) {
            const int key = r_key[k];   // the same word in every lane: the branch is uniform
            if (key < 0) continue;
            const int dr = r - (((key >> 3) & 7) - 1), dc = c - ((key >> 6) - 1);
            const int d = (o - (key & 7)) & 7;
            const float fo = r_fo[k];
            const bool col = (unsigned)dc < 2u;
#pragma unroll
            for (int half = 0; half < 2; ++half) {
                const int drh = dr + 2 * half;
                const float v = col && (unsigned)drh < 2u ? r_v[(2 * drh + dc) * kSamples + k] : 0.f;
                const float v1 = v * fo;
                h[half] = h[half] + (d == 0 ? v - v1 : d == 1 ? v1 : 0.f);
            }
        }
    }
    apap::sift_finish(h[0], h[1], out, row, lane);
}

// mode: angles out only; descriptors at given angles; both
int run(const uint8_t *const *d_imgs, const int *heights, const int *widths, const int *channels, int n_images, const float *d_pts,
        const int *pt_offset, const float *d_angles_in, float *d_angles_out, float *d_out, void *d_work, size_t work_bytes, void *stream,
        const char *who) {
    int rc = apap::sift_orient_check(heights, widths, channels, n_images, pt_offset, who);
    if (rc) return rc;
    const bool orient = d_angles_in == nullptr, describe = d_out != nullptr;
    if (!d_pts || (orient && !d_angles_out)) return apap::fail(APAP_ERR_INVALID_ARG, "%s: null device pointer", who);
    if (((uintptr_t)d_pts & 7) != 0 || ((uintptr_t)d_out & 3) != 0 || ((uintptr_t)d_angles_in & 3) != 0 || ((uintptr_t)d_angles_out & 3) != 0)
        return apap::fail(APAP_ERR_INVALID_ARG, "%s: keypoints must be 8-byte, angles and descriptors 4-byte aligned", who);
    hipStream_t s = (hipStream_t)stream;
    if ((rc = apap::sift_table_upload(d_imgs, heights, widths, channels, n_images, pt_offset, d_work, work_bytes, s, who))) return rc;
    const int k_begin = pt_offset[0], k_end = pt_offset[n_images];
    const dim3 blocks((unsigned)(((long long)k_end - k_begin + kPerBlock - 1) / kPerBlock)), threads(kThreads);
    const OrientConst K = make_const();
    const SiftImage *tab = (const SiftImage *)d_work;
    if (orient && describe)
        hipLaunchKernelGGL((k_sift_orient<true, true>), blocks, threads, 0, s, tab, n_images, d_pts, d_angles_in, d_angles_out, d_out, k_begin, k_end, K);
    else if (orient)
        hipLaunchKernelGGL((k_sift_orient<true, false>), blocks, threads, 0, s, tab, n_images, d_pts, d_angles_in, d_angles_out, d_out, k_begin, k_end, K);
    else
        hipLaunchKernelGGL((k_sift_orient<false, true>), blocks, threads, 0, s, tab, n_images, d_pts, d_angles_in, d_angles_out, d_out, k_begin, k_end, K);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return apap::hip_fail(e, "k_sift_orient launch");
    return APAP_OK;
}

}  // namespace

namespace apap {

int sift_orient_check(const int *heights, const int *widths, const int *channels, int n_images, const int *pt_offset, const char *who) {
    if (int rc = sift_check(heights, widths, channels, n_images, pt_offset, who)) return rc;
    for (int m = 0; m < n_images; ++m)
        if (heights[m] < kOrientMinSide || widths[m] < kOrientMinSide)
            return fail(APAP_ERR_INVALID_ARG, "%s: image %d is %d x %d (sides %d .. %d)", who, m, heights[m], widths[m], kOrientMinSide, kImageMaxSide);
    return APAP_OK;
}

}  // namespace apap

extern "C" {

int apap_sift_orient_window(float *out) {
    if (!out) return apap::fail(APAP_ERR_INVALID_ARG, "apap_sift_orient_window: null argument");
    double w[kOriSamples];
    orient_window_f64(w);
    for (int k = 0; k < kOriSamples; ++k) out[k] = (float)w[k];
    return APAP_OK;
}

int apap_sift_descr_window(float *out) {
    if (!out) return apap::fail(APAP_ERR_INVALID_ARG, "apap_sift_descr_window: null argument");
    double w[kSamples];
    descr_window_f64(w);
    for (int k = 0; k < kSamples; ++k) out[k] = (float)w[k];
    return APAP_OK;
}

size_t apap_sift_orient_workspace_bytes(int n_images) { return n_images < 1 || n_images > apap::kMaxImages ? 0 : apap::sift_table_bytes(n_images); }

int apap_sift_orient_batch_device(apap_ctx *ctx, const uint8_t *const *d_imgs, const int *heights, const int *widths, const int *channels,
                                  int n_images, const float *d_pts, const int *pt_offset, float *d_angles, void *d_work, size_t work_bytes,
                                  void *stream) {
    (void)ctx;
    const char *who = "apap_sift_orient_batch_device";
    if (!d_angles) return apap::fail(APAP_ERR_INVALID_ARG, "%s: null device pointer", who);
    return run(d_imgs, heights, widths, channels, n_images, d_pts, pt_offset, nullptr, d_angles, nullptr, d_work, work_bytes, stream, who);
}

int apap_sift_orient_device(apap_ctx *ctx, const uint8_t *d_img, int h, int w, int channels, const float *d_pts, int n, float *d_angles,
                            void *d_work, size_t work_bytes, void *stream) {
    const int off[2] = {0, n};
    return apap_sift_orient_batch_device(ctx, &d_img, &h, &w, &channels, 1, d_pts, off, d_angles, d_work, work_bytes, stream);
}

int apap_sift_describe_oriented_batch_device(apap_ctx *ctx, const uint8_t *const *d_imgs, const int *heights, const int *widths,
                                             const int *channels, int n_images, const float *d_pts, const int *pt_offset,
                                             const float *d_angles, float *d_angles_out, float *d_out, void *d_work, size_t work_bytes,
                                             void *stream) {
    (void)ctx;
    const char *who = "apap_sift_describe_oriented_batch_device";
    if (!d_out) return apap::fail(APAP_ERR_INVALID_ARG, "%s: null device pointer", who);
    if (d_angles && d_angles_out) return apap::fail(APAP_ERR_INVALID_ARG, "%s: angles are given: angles_out must be null", who);
    return run(d_imgs, heights, widths, channels, n_images, d_pts, pt_offset, d_angles, d_angles_out, d_out, d_work, work_bytes, stream, who);
}

int apap_sift_describe_oriented_device(apap_ctx *ctx, const uint8_t *d_img, int h, int w, int channels, const float *d_pts, int n,
                                       const float *d_angles, float *d_angles_out, float *d_out, void *d_work, size_t work_bytes,
                                       void *stream) {
    const int off[2] = {0, n};
    return apap_sift_describe_oriented_batch_device(ctx, &d_img, &h, &w, &channels, 1, d_pts, off, d_angles, d_angles_out, d_out, d_work,
                                                    work_bytes, stream);
}

}  // extern "C"
