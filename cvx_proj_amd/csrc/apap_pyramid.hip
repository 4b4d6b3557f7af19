// The image pyramid of the feature front end: grey levels at scales 2^-k and (3/4) 2^-k, in exact integer arithmetic, and the
// pack that brings the corners found on the levels back into the base picture's frame.  The contract is in
// include/apap_hip.h "image pyramid" and DESIGN.md "Image pyramid and scale", and, in numpy int64, in tests/pyramid_spec.py:
//   grey    level 0: the uint8 picture as it is, or BGR through apap::grey_at's formula
//   H(g)    ((h + 1) >> 1, (w + 1) >> 1): (sum_{i,j = -2..2} b_i b_j g[r(2y + i), r(2x + j)] + 128) >> 8, b = 1 4 6 4 1,
//           r = reflect-101; one rounding, so the order of the two passes does not matter
//   Q(g)    ((3h) >> 2, (3w) >> 2): output 3k + r reads sources 4k + r and 4k + r + 1 with weights (5, 1), (3, 3), (1, 5);
//           (sum of wy wx g + 18) / 36
//   levels  even 2k = H^k(level 0), odd 2k + 1 = H^k(Q(level 0)); without half steps the even ones alone
//
// k_pyramid_reduce: one launch builds, for every picture of the call, every level that depends only on levels already built.
// A job is one source level; a block of 256 threads takes a 64 x 32 tile of it, found by bisection of the jobs' first
// blocks.  The tile is staged once in LDS as grey with the halo H needs ((2 * 32 + 3) x (2 * 16 + 3) pixels are read from it;
// Q's 4 -> 3 pattern never leaves the tile), four pixels a thread, by dword loads where the address allows.  From it the
// block writes up to three outputs: the grey plane itself (step 1 of a picture: level 0, so a BGR picture is read once), the
// 48 x 24 tile of Q and the 32 x 16 tile of H, four adjacent bytes a thread, one dword store where the address allows.
// Integers only, no atomics.  The whole pyramid of any number of pictures takes 1 + ceil((levels - 1) / 2) launches at most.
//
// k_pyramid_keypoints: one thread per row of the concatenated keypoint list; its level image by bisection of the levels'
// first rows; the base-frame coordinate 2^k x, or (2^(k + 3) x + 1) / 6 as one float64 division, rounded to float32.
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>
#include <vector>

#include "apap_image_dev.h"
#include "apap_internal.h"

namespace {

using apap::reflect, apap::up256;

constexpr int kMaxLevels = APAP_PYRAMID_MAX_LEVELS, kMinSide = APAP_PYRAMID_MIN_SIDE;
constexpr int kSW = APAP_PYRAMID_TILE_W, kSH = APAP_PYRAMID_TILE_H;   // the source tile of a block
constexpr int kThreads = 256;
constexpr int kLW = kSW + 8, kLH = kSH + 3;   // in LDS: columns x0 - 4 .. x0 + 67 (groups of four stay aligned), rows y0 - 2 .. y0 + 32
constexpr int kHGroups = (kSW / 2) * (kSH / 2) / 4, kQGroups = (kSW / 4 * 3) * (kSH / 4 * 3) / 4;   // 128, 288
static_assert(kSW == 64 && kSH == 32 && kMaxLevels == 16 && kMinSide == 32, "the tile mapping below is for these");

struct alignas(16) PyrJob {   // one source level, in device memory
    const uint8_t *src;
    uint8_t *grey, *q, *h;    // the outputs; any may be null
    int sh, sw, sc;           // the source: sc = 3 only for a picture itself
    int tile0, tiles_x;       // its first block, its tiles per row
    int pad[3];
};
static_assert(sizeof(PyrJob) == 64, "PyrJob");

struct alignas(16) KpLevel {  // one level image of the pack
    int k0;                   // its first row of the concatenated list (the next entry's k0 ends it)
    int num, shift, level;
};

__device__ __forceinline__ int grey_of(int b, int g, int r) { return (3735 * b + 19235 * g + 9798 * r + 16384) >> 15; }

// Four bytes to p: one dword where all four are wanted and p is aligned, else the first n of them one by one.
__device__ __forceinline__ void store4(uint8_t *p, unsigned packed, int n) {
    if (n >= 4 && ((uintptr_t)p & 3) == 0) {
        *reinterpret_cast<unsigned *>(p) = packed;
    } else {
        for (int i = 0; i < 4 && i < n; ++i) p[i] = (uint8_t)(packed >> (8 * i));
    }
}

__global__ __launch_bounds__(kThreads) void k_pyramid_reduce(const PyrJob *__restrict__ jobs, int n_jobs) {
    __shared__ alignas(16) uint8_t s_g[kLH * kLW];

    int lo = 0, hi = n_jobs - 1;   // the last job whose first block is not after this one
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (jobs[mid].tile0 <= (int)blockIdx.x)
            lo = mid;
        else
            hi = mid - 1;
    }
    const PyrJob J = jobs[lo];
    const int t = (int)blockIdx.x - J.tile0;
    const int tile_y = t / J.tiles_x, tile_x = t - tile_y * J.tiles_x;
    const int x0 = tile_x * kSW, y0 = tile_y * kSH;
    const int tid = threadIdx.x;

    // the grey tile with its halo, reflected; level 0's grey plane on the way
    for (int at = tid; at < kLH * (kLW / 4); at += kThreads) {
        const int ly = at / (kLW / 4), lx = 4 * (at - ly * (kLW / 4));
        const int gy = y0 - 2 + ly, gx = x0 - 4 + lx;
        const int y = reflect(gy, J.sh);
        unsigned packed = 0;
        if (gx >= 0 && gx + 3 < J.sw) {
            const uint8_t *p = J.src + ((size_t)y * J.sw + gx) * J.sc;
            if (J.sc == 1) {
                if (((uintptr_t)p & 3) == 0)
                    packed = *reinterpret_cast<const unsigned *>(p);
                else
                    packed = (unsigned)p[0] | ((unsigned)p[1] << 8) | ((unsigned)p[2] << 16) | ((unsigned)p[3] << 24);
            } else {
                unsigned a, b, c;   // the twelve bytes B G R B | G R B G | R B G R
                if (((uintptr_t)p & 3) == 0) {
                    const unsigned *q = reinterpret_cast<const unsigned *>(p);
                    a = q[0];
                    b = q[1];
                    c = q[2];
                } else {
                    a = (unsigned)p[0] | ((unsigned)p[1] << 8) | ((unsigned)p[2] << 16) | ((unsigned)p[3] << 24);
                    b = (unsigned)p[4] | ((unsigned)p[5] << 8) | ((unsigned)p[6] << 16) | ((unsigned)p[7] << 24);
                    c = (unsigned)p[8] | ((unsigned)p[9] << 8) | ((unsigned)p[10] << 16) | ((unsigned)p[11] << 24);
                }
                const int g0 = grey_of(a & 255, (a >> 8) & 255, (a >> 16) & 255);
                const int g1 = grey_of(a >> 24, b & 255, (b >> 8) & 255);
                const int g2 = grey_of((b >> 16) & 255, b >> 24, c & 255);
                const int g3 = grey_of((c >> 8) & 255, (c >> 16) & 255, c >> 24);
                packed = (unsigned)g0 | ((unsigned)g1 << 8) | ((unsigned)g2 << 16) | ((unsigned)g3 << 24);
            }
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) packed |= (unsigned)apap::grey_at(J.src, y, reflect(gx + i, J.sw), J.sw, J.sc) << (8 * i);
        }
        *reinterpret_cast<unsigned *>(s_g + ly * kLW + lx) = packed;
        // the tile's own pixels (not the halo): rows y0 .. y0 + 31, columns x0 .. x0 + 63, inside the picture
        if (J.grey && ly >= 2 && ly < 2 + kSH && gy < J.sh && lx >= 4 && lx < 4 + kSW && gx < J.sw)
            store4(J.grey + (size_t)gy * J.sw + gx, packed, J.sw - gx);
    }
    __syncthreads();

    for (int g = tid; g < kHGroups + kQGroups; g += kThreads) {
        if (g < kHGroups) {   // four adjacent pixels of H: waves 0 and 1
            if (!J.h) continue;
            const int hh = (J.sh + 1) >> 1, hw = (J.sw + 1) >> 1;
            const int oy = g / (kSW / 8), ox = 4 * (g - oy * (kSW / 8));
            const int Y = (y0 >> 1) + oy, X = (x0 >> 1) + ox;
            if (Y >= hh || X >= hw) continue;
            const uint8_t *s = s_g + (2 * oy) * kLW + 2 + 2 * ox;   // row 2 Y - 2, column 2 X - 2 of the picture
            int v[11];
#pragma unroll
            for (int c = 0; c < 11; ++c)
                v[c] = (int)s[c] + 4 * (int)s[kLW + c] + 6 * (int)s[2 * kLW + c] + 4 * (int)s[3 * kLW + c] + (int)s[4 * kLW + c];
            unsigned packed = 0;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int sum = v[2 * i] + 4 * v[2 * i + 1] + 6 * v[2 * i + 2] + 4 * v[2 * i + 3] + v[2 * i + 4];
                packed |= (unsigned)((sum + 128) >> 8) << (8 * i);
            }
            store4(J.h + (size_t)Y * hw + X, packed, hw - X);
        } else {              // four adjacent pixels of Q
            if (!J.q) continue;
            const int qh = (3 * J.sh) >> 2, qw = (3 * J.sw) >> 2;
            const int k = g - kHGroups;
            const int oy = k / (kSW / 4 * 3 / 4), ox = 4 * (k - oy * (kSW / 4 * 3 / 4));
            const int Y = (y0 >> 2) * 3 + oy, X = (x0 >> 2) * 3 + ox;
            if (Y >= qh || X >= qw) continue;
            const int ky = oy / 3, ry = oy - 3 * ky;
            const uint8_t *row0 = s_g + (2 + 4 * ky + ry) * kLW + 4, *row1 = row0 + kLW;
            const int wy0 = 5 - 2 * ry, wy1 = 1 + 2 * ry;
            unsigned packed = 0;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int kx = (ox + i) / 3, rx = (ox + i) - 3 * kx;
                const int c = 4 * kx + rx, wx0 = 5 - 2 * rx, wx1 = 1 + 2 * rx;
                const int sum = wy0 * (wx0 * (int)row0[c] + wx1 * (int)row0[c + 1]) + wy1 * (wx0 * (int)row1[c] + wx1 * (int)row1[c + 1]);
                packed |= (unsigned)((sum + 18) / 36) << (8 * i);
            }
            store4(J.q + (size_t)Y * qw + X, packed, qw - X);
        }
    }
}

__global__ __launch_bounds__(kThreads) void k_pyramid_keypoints(const KpLevel *__restrict__ tab, int n_level_images, int slab_rows,
                                                                const float *__restrict__ slab_pts,
                                                                const long long *__restrict__ slab_response, int total,
                                                                float *__restrict__ pts, float *__restrict__ level_pts,
                                                                int *__restrict__ level, long long *__restrict__ response) {
    const int row = (int)blockIdx.x * kThreads + (int)threadIdx.x;
    if (row >= total) return;
    int lo = 0, hi = n_level_images - 1;   // the last level image whose first row is not after this one: never an empty one
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (tab[mid].k0 <= row)
            lo = mid;
        else
            hi = mid - 1;
    }
    const KpLevel L = tab[lo];
    const size_t from = (size_t)lo * slab_rows + (size_t)(row - L.k0);
    const float x = slab_pts[2 * from], y = slab_pts[2 * from + 1];
    float bx, by;
    if (L.num == 1) {
        bx = (float)(double)((long long)x << L.shift);
        by = (float)(double)((long long)y << L.shift);
    } else {   // scale 3 / 2^shift: (2^(shift + 1) x + 1) / 6
        bx = (float)((double)(((long long)x << (L.shift + 1)) + 1) / 6.0);
        by = (float)((double)(((long long)y << (L.shift + 1)) + 1) / 6.0);
    }
    pts[2 * (size_t)row] = bx;
    pts[2 * (size_t)row + 1] = by;
    level_pts[2 * (size_t)row] = x;
    level_pts[2 * (size_t)row + 1] = y;
    level[row] = L.level;
    response[row] = slab_response[from];
}

struct Level {
    int h, w, num, shift;
    long long off;
};

// The levels of one picture (sides already checked); returns their number and the bytes they take, a 256-byte multiple.
int levels_of(int h, int w, int n_levels, int half_steps, Level *L, long long *total) {
    int count = 0;
    long long at = 0;
    for (int l = 0; l < n_levels; ++l) {
        const bool odd = half_steps && (l & 1);
        const int k = half_steps ? l >> 1 : l;
        int lh = odd ? (3 * h) >> 2 : h, lw = odd ? (3 * w) >> 2 : w;
        for (int i = 0; i < k; ++i) {
            lh = (lh + 1) >> 1;
            lw = (lw + 1) >> 1;
        }
        if (lh < kMinSide || lw < kMinSide) break;
        L[count++] = Level{lh, lw, odd ? 3 : 1, odd ? k + 2 : k, at};
        at += (long long)up256((size_t)lh * lw);
    }
    *total = at;
    return count;
}

int sides_check(int m, int h, int w, const char *who) {
    if (h < kMinSide || h > apap::kImageMaxSide || w < kMinSide || w > apap::kImageMaxSide)
        return apap::fail(APAP_ERR_INVALID_ARG, "%s: image %d is %d x %d (sides %d .. %d)", who, m, h, w, kMinSide, apap::kImageMaxSide);
    return APAP_OK;
}

int levels_check(int n_levels, const char *who) {
    if (n_levels < 1 || n_levels > kMaxLevels) return apap::fail(APAP_ERR_INVALID_ARG, "%s: n_levels = %d (1 .. %d)", who, n_levels, kMaxLevels);
    return APAP_OK;
}

}  // namespace

namespace apap {

// The argument checks of the pyramid's entry points that need no device pointer.
int pyramid_check(const int *heights, const int *widths, const int *channels, int n_images, int n_levels, const char *who) {
    if (!heights || !widths || !channels) return fail(APAP_ERR_INVALID_ARG, "%s: null heights / widths / channels", who);
    if (n_images < 1 || n_images > kMaxImages) return fail(APAP_ERR_INVALID_ARG, "%s: n_images = %d (1 .. %d)", who, n_images, kMaxImages);
    if (int rc = levels_check(n_levels, who)) return rc;
    for (int m = 0; m < n_images; ++m) {
        if (int rc = sides_check(m, heights[m], widths[m], who)) return rc;
        if (int rc = image_channels_check(m, channels[m], who)) return rc;
    }
    return APAP_OK;
}

// The argument checks of the pack's entry points that need no device pointer.
int pyramid_keypoints_check(int slab_rows, const int *counts, const int *scale_num, const int *scale_shift, const int *level_index,
                            int n_level_images, const char *who) {
    if (!counts || !scale_num || !scale_shift || !level_index)
        return fail(APAP_ERR_INVALID_ARG, "%s: null counts / scale_num / scale_shift / level_index", who);
    if (n_level_images < 1 || n_level_images > kMaxImages)
        return fail(APAP_ERR_INVALID_ARG, "%s: n_level_images = %d (1 .. %d)", who, n_level_images, kMaxImages);
    if (slab_rows < 1) return fail(APAP_ERR_INVALID_ARG, "%s: slab_rows = %d (>= 1)", who, slab_rows);
    long long total = 0;
    for (int m = 0; m < n_level_images; ++m) {
        if (counts[m] < 0 || counts[m] > slab_rows)
            return fail(APAP_ERR_INVALID_ARG, "%s: level image %d: count %d (0 .. slab_rows = %d)", who, m, counts[m], slab_rows);
        if ((scale_num[m] != 1 && scale_num[m] != 3) || scale_shift[m] < 0 || scale_shift[m] > kMaxLevels + 2)
            return fail(APAP_ERR_INVALID_ARG, "%s: level image %d: scale %d / 2^%d (1 or 3 over 2^0 .. 2^%d)", who, m, scale_num[m],
                        scale_shift[m], kMaxLevels + 2);
        total += counts[m];
    }
    if (total > INT_MAX) return fail(APAP_ERR_INVALID_ARG, "%s: %lld keypoints in all exceed the int32 offsets", who, total);
    return APAP_OK;
}

}  // namespace apap

extern "C" {

int apap_pyramid_layout(int h, int w, int n_levels, int half_steps, int *heights, int *widths, long long *offsets, int *scale_num,
                        int *scale_shift) {
    const char *who = "apap_pyramid_layout";
    if (sides_check(0, h, w, who) || levels_check(n_levels, who)) return 0;
    Level L[kMaxLevels];
    long long total;
    const int n = levels_of(h, w, n_levels, half_steps, L, &total);
    for (int l = 0; l < n; ++l) {
        if (heights) heights[l] = L[l].h;
        if (widths) widths[l] = L[l].w;
        if (offsets) offsets[l] = L[l].off;
        if (scale_num) scale_num[l] = L[l].num;
        if (scale_shift) scale_shift[l] = L[l].shift;
    }
    if (offsets) offsets[n] = total;
    return n;
}

int apap_pyramid_level_caps(int max_corners, int n_levels, int half_steps, int *caps) {
    const char *who = "apap_pyramid_level_caps";
    if (!caps) return apap::fail(APAP_ERR_INVALID_ARG, "%s: null argument", who);
    if (max_corners < 1) return apap::fail(APAP_ERR_INVALID_ARG, "%s: max_corners = %d (>= 1)", who, max_corners);
    if (int rc = levels_check(n_levels, who)) return rc;
    for (int l = 0; l < n_levels; ++l) {
        const bool odd = half_steps && (l & 1);
        const int k = half_steps ? l >> 1 : l;
        const long long share = odd ? (9ll * max_corners) >> (2 * k + 4) : (long long)max_corners >> (2 * k);
        const long long cap = share < 16 ? 16 : share;
        caps[l] = (int)(cap < max_corners ? cap : max_corners);
    }
    return APAP_OK;
}

size_t apap_pyramid_workspace_bytes(int n_images, int n_levels) {
    if (n_images < 1 || n_images > apap::kMaxImages || n_levels < 1 || n_levels > kMaxLevels) return 0;
    return up256((size_t)n_images * n_levels * sizeof(PyrJob));
}

int apap_pyramid_build_batch_device(apap_ctx *ctx, const uint8_t *const *d_imgs, const int *heights, const int *widths,
                                    const int *channels, int n_images, int n_levels, int half_steps, uint8_t *d_levels,
                                    size_t levels_bytes, void *d_work, size_t work_bytes, void *stream) {
    const char *who = "apap_pyramid_build_batch_device";
    (void)ctx;
    int rc = apap::pyramid_check(heights, widths, channels, n_images, n_levels, who);
    if (rc) return rc;
    if (!d_imgs || !d_levels || !d_work) return apap::fail(APAP_ERR_INVALID_ARG, "%s: null device pointer", who);
    for (int m = 0; m < n_images; ++m)
        if (!d_imgs[m]) return apap::fail(APAP_ERR_INVALID_ARG, "%s: image %d: null device pointer", who, m);
    const size_t need = apap_pyramid_workspace_bytes(n_images, n_levels);
    if (work_bytes < need) return apap::fail(APAP_ERR_WORKSPACE, "%s: workspace %zu < %zu bytes", who, work_bytes, need);
    if (((uintptr_t)d_work & 255) != 0 || ((uintptr_t)d_levels & 255) != 0)
        return apap::fail(APAP_ERR_INVALID_ARG, "%s: workspace and level buffer must be 256-byte aligned", who);

    // every picture's levels, back to back
    std::vector<Level> lev((size_t)n_images * kMaxLevels);
    std::vector<int> count((size_t)n_images);
    std::vector<long long> base((size_t)n_images);
    long long at = 0;
    int deepest = 0;
    for (int m = 0; m < n_images; ++m) {
        long long total;
        count[m] = levels_of(heights[m], widths[m], n_levels, half_steps, &lev[(size_t)m * kMaxLevels], &total);
        base[m] = at;
        at += total;
        deepest = count[m] > deepest ? count[m] : deepest;
    }
    if (levels_bytes < (size_t)at) return apap::fail(APAP_ERR_WORKSPACE, "%s: level buffer %zu < %lld bytes", who, levels_bytes, at);

    // the jobs of every step: step 1 reads the pictures, step s > 1 halves the chains' last levels
    auto level_ptr = [&](int m, int l) -> uint8_t * { return l < count[m] ? d_levels + base[m] + lev[(size_t)m * kMaxLevels + l].off : nullptr; };
    std::vector<PyrJob> jobs;
    std::vector<int> step_first, step_tiles;
    const int stride = half_steps ? 2 : 1;
    for (int s = 1; s <= deepest; ++s) {   // ends at the first step without a job
        const size_t first = jobs.size();
        long long tiles = 0;
        auto add = [&](const uint8_t *src, int sh, int sw, int sc, uint8_t *grey, uint8_t *q, uint8_t *h) {
            const int tx = (sw + kSW - 1) / kSW, ty = (sh + kSH - 1) / kSH;
            jobs.push_back(PyrJob{src, grey, q, h, sh, sw, sc, (int)(tiles < INT_MAX ? tiles : INT_MAX), tx, {0, 0, 0}});
            tiles += (long long)tx * ty;
        };
        for (int m = 0; m < n_images; ++m) {
            const Level *L = &lev[(size_t)m * kMaxLevels];
            if (s == 1) {
                add(d_imgs[m], heights[m], widths[m], channels[m], level_ptr(m, 0), half_steps ? level_ptr(m, 1) : nullptr, level_ptr(m, stride));
            } else if (half_steps) {
                const int even = 2 * (s - 1), odd = 2 * s - 3;   // the sources; their halves are levels even + 2 and odd + 2
                if (even + 2 < count[m]) add(level_ptr(m, even), L[even].h, L[even].w, 1, nullptr, nullptr, level_ptr(m, even + 2));
                if (odd + 2 < count[m]) add(level_ptr(m, odd), L[odd].h, L[odd].w, 1, nullptr, nullptr, level_ptr(m, odd + 2));
            } else if (s < count[m]) {
                add(level_ptr(m, s - 1), L[s - 1].h, L[s - 1].w, 1, nullptr, nullptr, level_ptr(m, s));
            }
        }
        if (tiles > INT_MAX) return apap::fail(APAP_ERR_INVALID_ARG, "%s: %lld tiles in one launch exceed 2^31 - 1", who, tiles);
        if (jobs.size() == first) break;
        step_first.push_back((int)first);
        step_tiles.push_back((int)tiles);
    }
    if (jobs.size() * sizeof(PyrJob) > need) return apap::fail(APAP_ERR_WORKSPACE, "%s: job table exceeds the workspace", who);

    hipStream_t st = (hipStream_t)stream;
    // from pageable memory in stream order: the copy returns once its source has been consumed
    hipError_t e = hipMemcpyAsync(d_work, jobs.data(), jobs.size() * sizeof(PyrJob), hipMemcpyHostToDevice, st);
    if (e != hipSuccess) return apap::hip_fail(e, "apap_pyramid_build_batch_device: job table upload");
    for (size_t s = 0; s < step_first.size(); ++s) {
        const int n_jobs = (int)((s + 1 < step_first.size() ? (size_t)step_first[s + 1] : jobs.size()) - (size_t)step_first[s]);
        hipLaunchKernelGGL(k_pyramid_reduce, dim3((unsigned)step_tiles[s]), dim3(kThreads), 0, st, (const PyrJob *)d_work + step_first[s],
                           n_jobs);
        e = hipGetLastError();
        if (e != hipSuccess) return apap::hip_fail(e, "apap_pyramid_build_batch_device launch");
    }
    return APAP_OK;
}

int apap_pyramid_build_device(apap_ctx *ctx, const uint8_t *d_img, int h, int w, int channels, int n_levels, int half_steps,
                              uint8_t *d_levels, size_t levels_bytes, void *d_work, size_t work_bytes, void *stream) {
    return apap_pyramid_build_batch_device(ctx, &d_img, &h, &w, &channels, 1, n_levels, half_steps, d_levels, levels_bytes, d_work,
                                           work_bytes, stream);
}

size_t apap_pyramid_keypoints_workspace_bytes(int n_level_images) {
    return n_level_images < 1 || n_level_images > apap::kMaxImages ? 0 : up256((size_t)n_level_images * sizeof(KpLevel));
}

int apap_pyramid_keypoints_device(apap_ctx *ctx, const float *d_slab_pts, const long long *d_slab_response, int slab_rows,
                                  const int *counts, const int *scale_num, const int *scale_shift, const int *level_index,
                                  int n_level_images, float *d_pts, float *d_level_pts, int *d_level, long long *d_response,
                                  int *level_offset, void *d_work, size_t work_bytes, void *stream) {
    const char *who = "apap_pyramid_keypoints_device";
    (void)ctx;
    int rc = apap::pyramid_keypoints_check(slab_rows, counts, scale_num, scale_shift, level_index, n_level_images, who);
    if (rc) return rc;
    if (!level_offset) return apap::fail(APAP_ERR_INVALID_ARG, "%s: null level_offset", who);
    if (!d_slab_pts || !d_slab_response || !d_pts || !d_level_pts || !d_level || !d_response || !d_work)
        return apap::fail(APAP_ERR_INVALID_ARG, "%s: null device pointer", who);
    const size_t need = apap_pyramid_keypoints_workspace_bytes(n_level_images);
    if (work_bytes < need) return apap::fail(APAP_ERR_WORKSPACE, "%s: workspace %zu < %zu bytes", who, work_bytes, need);
    if (((uintptr_t)d_work & 255) != 0 || ((uintptr_t)d_slab_pts & 7) != 0 || ((uintptr_t)d_slab_response & 7) != 0 ||
        ((uintptr_t)d_pts & 7) != 0 || ((uintptr_t)d_level_pts & 7) != 0 || ((uintptr_t)d_level & 3) != 0 || ((uintptr_t)d_response & 7) != 0)
        return apap::fail(APAP_ERR_INVALID_ARG, "%s: workspace must be 256-byte, points and responses 8-byte and levels 4-byte aligned", who);
    std::vector<KpLevel> tab((size_t)n_level_images);
    int total = 0;
    for (int m = 0; m < n_level_images; ++m) {
        level_offset[m] = total;
        tab[m] = KpLevel{total, scale_num[m], scale_shift[m], level_index[m]};
        total += counts[m];
    }
    level_offset[n_level_images] = total;
    if (total == 0) return APAP_OK;
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = hipMemcpyAsync(d_work, tab.data(), tab.size() * sizeof(KpLevel), hipMemcpyHostToDevice, st);
    if (e != hipSuccess) return apap::hip_fail(e, "apap_pyramid_keypoints_device: level table upload");
    hipLaunchKernelGGL(k_pyramid_keypoints, dim3((unsigned)((total + kThreads - 1) / kThreads)), dim3(kThreads), 0, st,
                       (const KpLevel *)d_work, n_level_images, slab_rows, d_slab_pts, d_slab_response, total, d_pts, d_level_pts, d_level,
                       d_response);
    e = hipGetLastError();
    if (e != hipSuccess) return apap::hip_fail(e, "apap_pyramid_keypoints_device launch");
    return APAP_OK;
}

}  // extern "C"
