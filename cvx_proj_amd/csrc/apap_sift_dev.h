// The steps that the two descriptor kernels share, defined once: k_sift_describe (apap_sift.hip: KeyPoint(x, y, 1) at its
// default angle, constant sample tables) and k_sift_orient (apap_sift_orient.hip: the keypoint's orientation and the
// descriptor at an angle).  Both run one wave per keypoint and four keypoints per block, find their image by bisection of the
// image table, build the base-image patch around the keypoint from a grey patch alone, take atan2 from one polynomial and end
// the descriptor with the same tree sums, clamp, scale and stores.  tests/sift_spec.py and tests/sift_orient_spec.py restate
// every step in numpy; tests/test_gpu_sift.py and tests/test_gpu_feature_edges.py pin the first kernel's bytes.
#pragma once
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cstdint>
#include <vector>

#include "apap_image_dev.h"
#include "apap_internal.h"

namespace apap {

constexpr int kSiftDim = APAP_SIFT_DIM;
constexpr int kSiftTaps = APAP_SIFT_TAPS;
constexpr int kSiftPerBlock = APAP_SIFT_BLOCK_KEYPOINTS;
constexpr int kSiftThreads = 64 * kSiftPerBlock;
static_assert(kSiftDim == 128 && kSiftTaps == 13 && kSiftPerBlock == 4, "the lane mappings of both kernels are for these");

struct alignas(16) SiftImage {   // one image, in device memory
    const uint8_t *img;
    int h, w, c;
    int k0;                      // its first keypoint: a row of the concatenated arrays (the next image's k0 ends it)
    int pad[2];
};
static_assert(sizeof(SiftImage) == 32, "SiftImage");

inline size_t sift_table_bytes(int n_images) { return up256((size_t)n_images * sizeof(SiftImage)); }

// The checks of the _device entry points' image pointers and workspace, then the image table into the workspace, in stream
// order from pageable memory: the copy returns once its source has been consumed.
inline int sift_table_upload(const uint8_t *const *d_imgs, const int *heights, const int *widths, const int *channels, int n_images,
                             const int *pt_offset, void *d_work, size_t work_bytes, hipStream_t s, const char *who) {
    if (!d_imgs || !d_work) return fail(APAP_ERR_INVALID_ARG, "%s: null device pointer", who);
    for (int m = 0; m < n_images; ++m)
        if (!d_imgs[m]) return fail(APAP_ERR_INVALID_ARG, "%s: image %d: null device pointer", who, m);
    const size_t need = sift_table_bytes(n_images);
    if (work_bytes < need) return fail(APAP_ERR_WORKSPACE, "%s: workspace %zu < %zu bytes", who, work_bytes, need);
    if (((uintptr_t)d_work & 255) != 0) return fail(APAP_ERR_INVALID_ARG, "%s: workspace must be 256-byte aligned", who);
    std::vector<SiftImage> tab((size_t)n_images);
    for (int m = 0; m < n_images; ++m) tab[m] = SiftImage{d_imgs[m], heights[m], widths[m], channels[m], pt_offset[m], {0, 0}};
    hipError_t e = hipMemcpyAsync(d_work, tab.data(), (size_t)n_images * sizeof(SiftImage), hipMemcpyHostToDevice, s);
    if (e != hipSuccess) return hip_fail(e, "descriptor extraction: image table upload");
    return APAP_OK;
}

#if defined(__HIP__)

// The image of keypoint `row`: the last entry whose first keypoint is not after it (entry 0 for a wave without a keypoint).
__device__ __forceinline__ SiftImage sift_image_of(const SiftImage *__restrict__ tab, int n_images, long long row, bool live) {
    int lo = 0, hi = n_images - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (live && tab[mid].k0 <= row)
            lo = mid;
        else
            hi = mid - 1;
    }
    return tab[lo];
}

// The kB x kB base-image patch around (py, px), kB = kP - 12, from the kP x kP grey patch: reflect-101 on the indices, BGR ->
// grey in integers on the fly; the horizontal blur to kP x kB, the vertical blur to kB x kB, the taps ascending from 0, a
// multiply and an add per tap - the very sums of a full-image blur, so the patch equals the full image's base image bit for
// bit.  One wave's work on its own LDS; every wave of the block calls it (three block barriers), whether it has work or not.
template <int kP>
__device__ __forceinline__ void sift_base_patch(const SiftImage &I, int py, int px, bool work, int lane, const float (&taps)[kSiftTaps],
                                                float *patch, float *hb, float *base) {
    constexpr int kB = kP - (kSiftTaps - 1), kHalf = kP / 2;
    if (work) {
        for (int at = lane; at < kP * kP; at += 64) {
            const int pr = at / kP, pc = at - pr * kP;
            const int y = reflect(py - kHalf + pr, I.h), x = reflect(px - kHalf + pc, I.w);
            patch[at] = (float)grey_at(I.img, y, x, I.w, I.c);
        }
    }
    __syncthreads();
    if (work) {
        for (int at = lane; at < kP * kB; at += 64) {
            const int r = at / kB, c = at - r * kB;
            float acc = 0.f;
#pragma unroll
            for (int t = 0; t < kSiftTaps; ++t) acc = acc + taps[t] * patch[r * kP + c + t];
            hb[at] = acc;
        }
    }
    __syncthreads();
    if (work) {
        for (int at = lane; at < kB * kB; at += 64) {
            const int r = at / kB, c = at - r * kB;
            float acc = 0.f;
#pragma unroll
            for (int t = 0; t < kSiftTaps; ++t) acc = acc + taps[t] * hb[(r + t) * kB + c];
            base[at] = acc;
        }
    }
    __syncthreads();
}

// atan2(y, x) in degrees, in [0, 360]: |error| <= 2e-6 rad against the exact value (tests/sift_spec.py measures it).
// a = min(|x|, |y|) / max(|x|, |y|) in [0, 1]; atan(a) = a p(a^2), p of degree 7 (a near-minimax fit, 3.8e-8 in exact
// arithmetic), Horner with a multiply and an add per step; then the octant: pi/2 - r, pi - r, -r.  atan2(0, 0) = 0.
__device__ __forceinline__ float sift_atan2_deg(float y, float x) {
    const float ax = fabsf(x), ay = fabsf(y);
    const float mx = fmaxf(ax, ay), mn = fminf(ax, ay);
    if (mx == 0.f) return 0.f;
    const float a = mn / mx, s = a * a;
    float p = -4.054558929e-03f;
    p = p * s + 2.186292969e-02f;
    p = p * s + -5.591228977e-02f;
    p = p * s + 9.642194957e-02f;
    p = p * s + -1.390862912e-01f;
    p = p * s + 1.994656622e-01f;
    p = p * s + -3.332985938e-01f;
    p = p * s + 9.999993443e-01f;
    float r = a * p;
    if (ay > ax) r = 1.570796371e+00f - r;
    if (x < 0.f) r = 3.141592741e+00f - r;
    if (y < 0.f) r = -r;
    float deg = r * 5.729578018e+01f;
    if (deg < 0.f) deg = deg + 360.f;
    return deg;
}

__device__ __forceinline__ float sift_tree_sum(float a, float b) {   // bins (l, l + 64), then lanes l ^ 32, ^ 16 .. ^ 1
    float s = a + b;
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) s = s + __shfl_xor(s, m);
    return s;
}

// The descriptor's end, the whole wave: h0 and h1 are bins lane and lane + 64.  Sum of squares by the fixed tree, clamp at
// 0.2 of the norm, the same tree again, scale to 512, round, saturate; two coalesced 256-byte stores into row `row`.
__device__ __forceinline__ void sift_finish(float h0, float h1, float *__restrict__ out, long long row, int lane) {
    const float n1 = sift_tree_sum(h0 * h0, h1 * h1);
    const float thr = 0.2f * sqrtf(n1);
    h0 = fminf(h0, thr);
    h1 = fminf(h1, thr);
    const float n2 = sift_tree_sum(h0 * h0, h1 * h1);
    const float scale = 512.f / fmaxf(sqrtf(n2), FLT_EPSILON);
    float *o = out + (size_t)row * kSiftDim;
    o[lane] = fminf(fmaxf(rintf(h0 * scale), 0.f), 255.f);
    o[lane + 64] = fminf(fmaxf(rintf(h1 * scale), 0.f), 255.f);
}

#endif  // __HIP__

}  // namespace apap
