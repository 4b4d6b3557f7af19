// Harris corners in exact integer arithmetic: the keypoints that apap_sift_describe takes, from the image alone.  The contract
// is in include/apap_hip.h and DESIGN.md "Corner detection", and, in numpy int64, in tests/corner_spec.py:
//   grey   uint8 as it is, or BGR -> (3735 B + 19235 G + 9798 R + 16384) >> 15: apap::grey_at, which the descriptor reads too
//   Ix, Iy 3 x 3 Sobel, reflect-101 on the grey image's indices: -1020 .. 1020
//   a b c  unnormalised 3 x 3 box sums of Ix^2, Ix Iy, Iy^2, reflect-101 on the product images' indices: < 2^24
//   R      25 (a c - b^2) - (a + c)^2 in int64: 25 times Harris's det - 0.04 tr^2
//   corner R > 0 and (R, -index) greater than that of every other pixel of the (2 radius + 1)^2 window inside the image
//   out    corners with 1000 R >= quality_permille Rmax, by R descending then index ascending, the first max_corners
//
// k_corner_tile: a block of 256 threads takes a 64 x 32 tile of one image (blockIdx.y: the image of a batch), all in LDS:
//   1. the grey tile with a halo of radius + 2, indices reflected, BGR converted on the fly;
//   2. (Ix, Iy) packed in a dword on the tile with a halo of radius + 1; a position one pixel outside the image holds the
//      gradient of its reflection, which is what the box sum's reflect-101 reads there;
//   3. a, b, c and R on the tile with a halo of radius (INT64_MIN outside the image: nothing competes there); a c, b^2 and
//      (a + c)^2 are one 32 x 32 -> 64 multiply each;
//   4. the window test on integers alone.  q beats p iff R(q) > R(p), or R(q) = R(p) and q has the smaller index; the window
//      splits into the pixels before p (the rows above, and the same row to the left) and those after it, so p is a corner iff
//      R > 0, max R before p < R, and max R after p <= R.  Row pass: the maximum over columns x - radius .. x + radius of every
//      row of the tile and its halo; column pass: the maxima of the rows above and below, and of the two halves of p's own row;
//   5. the block's corners go to an LDS list, one atomic add reserves their rows of the image's candidate list, and one 64-bit
//      integer atomic max folds the block's largest response into the image's Rmax.
// k_corner_select: a block of 1024 threads per image.  Survivors of the quality test are counted; if more than max_corners, a
// radix select (7 digits of 8 bits, R < 2^56) finds the max_corners-th largest R; the candidates at or above it are compacted
// (in LDS up to 2048, else in the workspace), padded to a power of two and sorted by a bitonic network on the total order
// (R descending, index ascending).  Indices are distinct, so the sorted sequence - and every output byte - does not depend on
// the order in which the atomics appended the candidates.
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>
#include <vector>

#include "apap_image_dev.h"
#include "apap_internal.h"

namespace {

using apap::grey_at, apap::reflect, apap::up256;

constexpr int kTW = APAP_CORNER_TILE_W, kTH = APAP_CORNER_TILE_H;
constexpr int kThreads = 256;
constexpr int kMaxRadius = APAP_CORNER_MAX_RADIUS;
constexpr int kSmallRadius = 5;          // the kernel instance with the smaller LDS footprint serves radius <= 5
constexpr int kSelThreads = 1024;
constexpr int kLdsSort = 2048;           // candidates sorted in LDS (32 KB)
static_assert(kTW == 64 && kTH == 32 && kMaxRadius == 16, "the tile kernel's LDS budget is for these");

struct alignas(16) Cand {   // one corner: 16 bytes
    long long R;
    int idx;                // y * w + x
    int pad;
};

struct alignas(16) CornerImage {   // one image, in device memory
    const uint8_t *img;
    Cand *cand;                    // its candidate list: cap entries
    Cand *sorted;                  // selection's buffer: pow2ceil(cap) entries
    int h, w, c, cap;
    long long pad;
};
static_assert(sizeof(CornerImage) == 48, "CornerImage");

struct alignas(16) CornerCount {   // per image, zeroed before the tile kernel
    unsigned long long rmax;
    unsigned n;
    unsigned pad;
};

// ceil(h / (radius + 1)) ceil(w / (radius + 1)): no two corners lie within radius of each other in both axes
inline size_t corner_cap(int h, int w, int radius) {
    const int s = radius + 1;
    return (size_t)((h + s - 1) / s) * (size_t)((w + s - 1) / s);
}
inline size_t pow2ceil(size_t n) {
    size_t p = 1;
    while (p < n) p <<= 1;
    return p;
}

template <int RMAX>
__global__ __launch_bounds__(kThreads) void k_corner_tile(const CornerImage *__restrict__ tab, CornerCount *__restrict__ cnt, int r) {
    constexpr int GMAX = (kTH + 2 * RMAX + 4) * (kTW + 2 * RMAX + 4);
    constexpr int DMAX = (kTH + 2 * RMAX + 2) * (kTW + 2 * RMAX + 2);
    constexpr int RRMAX = (kTH + 2 * RMAX) * (kTW + 2 * RMAX);
    constexpr int MMAX = (kTH + 2 * RMAX) * kTW;
    // the block's corner list reuses the gradients' space: at most ceil(32 / 2) ceil(64 / 2) = 512 corners (radius 1)
    constexpr unsigned kListMax = 512;
    static_assert(DMAX * sizeof(int) >= kListMax * sizeof(Cand), "the corner list must fit over the gradients");
    __shared__ long long s_R[RRMAX];
    __shared__ long long s_M[MMAX];
    __shared__ alignas(16) int s_d[DMAX];
    __shared__ uint8_t s_g[(GMAX + 15) / 16 * 16];
    __shared__ unsigned long long s_max;
    __shared__ unsigned s_n, s_base;

    const CornerImage I = tab[blockIdx.y];
    const int tiles_x = (I.w + kTW - 1) / kTW, tiles_y = (I.h + kTH - 1) / kTH;
    if ((int)blockIdx.x >= tiles_x * tiles_y) return;   // a smaller image of a ragged batch
    const int tile_y = blockIdx.x / tiles_x, tile_x = blockIdx.x - tile_y * tiles_x;
    const int x0 = tile_x * kTW, y0 = tile_y * kTH;
    const int tid = threadIdx.x;
    const int GW = kTW + 2 * r + 4, GH = kTH + 2 * r + 4;
    const int DW = kTW + 2 * r + 2, DH = kTH + 2 * r + 2;
    const int RW = kTW + 2 * r, RH = kTH + 2 * r;
    if (tid == 0) {
        s_max = 0;
        s_n = 0;
    }

    for (int at = tid; at < GW * GH; at += kThreads) {
        const int ly = at / GW, lx = at - ly * GW;
        const int y = reflect(y0 - r - 2 + ly, I.h), x = reflect(x0 - r - 2 + lx, I.w);
        s_g[at] = (uint8_t)grey_at(I.img, y, x, I.w, I.c);
    }
    __syncthreads();

    for (int at = tid; at < DW * DH; at += kThreads) {
        const int ly = at / DW, lx = at - ly * DW;
        const int gy = y0 - r - 1 + ly, gx = x0 - r - 1 + lx;
        int packed = 0;
        if (gy >= -1 && gy <= I.h && gx >= -1 && gx <= I.w) {
            // the pixel itself, or its reflection: at least one pixel inside the staged grey region on every side
            const int cy = reflect(gy, I.h) - (y0 - r - 2), cx = reflect(gx, I.w) - (x0 - r - 2);
            const uint8_t *g = s_g + cy * GW + cx;
            const int ix = ((int)g[-GW + 1] + 2 * (int)g[1] + (int)g[GW + 1]) - ((int)g[-GW - 1] + 2 * (int)g[-1] + (int)g[GW - 1]);
            const int iy = ((int)g[GW - 1] + 2 * (int)g[GW] + (int)g[GW + 1]) - ((int)g[-GW - 1] + 2 * (int)g[-GW] + (int)g[-GW + 1]);
            packed = (int)((unsigned)(ix & 0xffff) | ((unsigned)iy << 16));
        }
        s_d[at] = packed;
    }
    __syncthreads();

    for (int at = tid; at < RW * RH; at += kThreads) {
        const int ly = at / RW, lx = at - ly * RW;
        const int gy = y0 - r + ly, gx = x0 - r + lx;
        long long R = LLONG_MIN;
        if (gy >= 0 && gy < I.h && gx >= 0 && gx < I.w) {
            int a = 0, b = 0, c = 0;
#pragma unroll
            for (int dy = 0; dy < 3; ++dy)
#pragma unroll
                for (int dx = 0; dx < 3; ++dx) {
                    const int d = s_d[(ly + dy) * DW + lx + dx];
                    const int ix = (int)(short)(d & 0xffff), iy = d >> 16;
                    a += ix * ix;
                    b += ix * iy;
                    c += iy * iy;
                }
            const int t = a + c;
            R = 25 * ((long long)a * c - (long long)b * b) - (long long)t * t;
        }
        s_R[at] = R;
    }
    __syncthreads();

    // row pass: the maximum over the window's columns, for every row of the tile and its halo
    for (int at = tid; at < RH * kTW; at += kThreads) {
        const int ly = at / kTW, tx = at - ly * kTW;
        const long long *row = s_R + ly * RW + tx;
        long long m = row[0];
        for (int k = 1; k <= 2 * r; ++k) m = max(m, row[k]);
        s_M[at] = m;
    }
    __syncthreads();

    Cand *s_list = reinterpret_cast<Cand *>(s_d);   // the gradients are dead
    for (int at = tid; at < kTH * kTW; at += kThreads) {
        const int ty = at / kTW, tx = at - ty * kTW;
        const long long *row = s_R + (ty + r) * RW + tx;
        const long long R = row[r];
        if (R <= 0) continue;   // also every pixel outside the image
        long long before = LLONG_MIN, after = LLONG_MIN;
        for (int k = 0; k < r; ++k) {
            before = max(before, max(row[k], s_M[(ty + k) * kTW + tx]));
            after = max(after, max(row[r + 1 + k], s_M[(ty + r + 1 + k) * kTW + tx]));
        }
        if (before < R && after <= R) {
            const unsigned slot = atomicAdd(&s_n, 1u);
            if (slot < kListMax) s_list[slot] = Cand{R, (y0 + ty) * I.w + x0 + tx, 0};   // always: the bound holds for a tile too
            atomicMax(&s_max, (unsigned long long)R);
        }
    }
    __syncthreads();
    const unsigned n = min(s_n, kListMax);
    if (n == 0) return;
    if (tid == 0) {
        s_base = atomicAdd(&cnt[blockIdx.y].n, n);
        atomicMax(&cnt[blockIdx.y].rmax, s_max);
    }
    __syncthreads();
    const unsigned base = s_base;
    for (unsigned k = tid; k < n; k += kThreads)
        if (base + k < (unsigned)I.cap) I.cand[base + k] = s_list[k];   // the bound on the corner count makes this always true
}

__device__ __forceinline__ bool before(const Cand &p, const Cand &q) { return p.R > q.R || (p.R == q.R && p.idx < q.idx); }

// bitonic network on P = 2^k entries, into the order `before`; every thread of the block calls it
__device__ __forceinline__ void bitonic_sort(Cand *a, int P) {
    for (int k = 2; k <= P; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = threadIdx.x; t < P / 2; t += kSelThreads) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
                const Cand p = a[i], q = a[l];
                if ((i & k) == 0 ? before(q, p) : before(p, q)) {
                    a[i] = q;
                    a[l] = p;
                }
            }
            __syncthreads();
        }
}

__global__ __launch_bounds__(kSelThreads) void k_corner_select(const CornerImage *__restrict__ tab, const CornerCount *__restrict__ cnt,
                                                               int max_corners, int quality_permille, float *__restrict__ pts,
                                                               long long *__restrict__ response, int *__restrict__ count) {
    __shared__ Cand s_sort[kLdsSort];
    __shared__ unsigned s_hist[256];
    __shared__ unsigned s_count[2];
    __shared__ int s_digit, s_remaining;

    const int m = blockIdx.x, tid = threadIdx.x;
    const CornerImage I = tab[m];
    const int n = (int)min(cnt[m].n, (unsigned)I.cap);
    const long long floor_q = (long long)quality_permille * (long long)cnt[m].rmax;   // keep 1000 R >= this
    const Cand *cand = I.cand;

    if (tid < 2) s_count[tid] = 0;
    __syncthreads();
    {
        unsigned mine = 0;
#pragma unroll 4
        for (int i = tid; i < n; i += kSelThreads) mine += 1000 * cand[i].R >= floor_q;
        if (mine) atomicAdd(&s_count[0], mine);
    }
    __syncthreads();
    const int survivors = (int)s_count[0];
    const int K = min(max_corners, survivors);

    // the K-th largest response among the survivors, when not all of them are kept: a radix select, most significant digit first
    unsigned long long T = 0, mask = 0;
    if (survivors > max_corners) {
        int remaining = K;
        for (int shift = 48; shift >= 0; shift -= 8) {
            if (tid < 256) s_hist[tid] = 0;
            __syncthreads();
#pragma unroll 4
            for (int i = tid; i < n; i += kSelThreads) {
                const long long R = cand[i].R;
                if (1000 * R >= floor_q && ((unsigned long long)R & mask) == T) atomicAdd(&s_hist[((unsigned long long)R >> shift) & 255], 1u);
            }
            __syncthreads();
            if (tid == 0) {
                int above = 0, d = 255;
                for (; d > 0; --d) {
                    if (above + (int)s_hist[d] >= remaining) break;
                    above += (int)s_hist[d];
                }
                s_digit = d;
                s_remaining = remaining - above;
            }
            __syncthreads();
            T |= (unsigned long long)s_digit << shift;
            mask |= 255ull << shift;
            remaining = s_remaining;
        }
    }
    // every candidate at or above T (all responses equal to T included: the index decides among them)
    {
        unsigned mine = 0;
#pragma unroll 4
        for (int i = tid; i < n; i += kSelThreads) {
            const long long R = cand[i].R;
            mine += 1000 * R >= floor_q && (unsigned long long)R >= T;
        }
        if (mine) atomicAdd(&s_count[1], mine);
    }
    __syncthreads();
    const int chosen = (int)s_count[1];
    int P = 1;
    while (P < chosen) P <<= 1;
    Cand *a = P <= kLdsSort ? s_sort : I.sorted;
    __syncthreads();
    if (tid == 0) s_count[0] = 0;
    __syncthreads();
    for (int i = tid; i < n; i += kSelThreads) {
        const Cand c = cand[i];
        if (1000 * c.R >= floor_q && (unsigned long long)c.R >= T) a[atomicAdd(&s_count[0], 1u)] = c;
    }
    for (int i = chosen + tid; i < P; i += kSelThreads) a[i] = Cand{0, INT_MAX, 0};   // after every corner: R > 0
    __syncthreads();
    if (P <= kLdsSort)
        bitonic_sort(s_sort, P);
    else
        bitonic_sort(I.sorted, P);

    float *o_pts = pts + (size_t)m * max_corners * 2;
    long long *o_resp = response + (size_t)m * max_corners;
    for (int i = tid; i < max_corners; i += kSelThreads) {
        float x = 0.f, y = 0.f;
        long long R = 0;
        if (i < K) {
            const Cand c = a[i];
            const int cy = c.idx / I.w;
            x = (float)(c.idx - cy * I.w);
            y = (float)cy;
            R = c.R;
        }
        o_pts[2 * (size_t)i] = x;
        o_pts[2 * (size_t)i + 1] = y;
        o_resp[i] = R;
    }
    if (tid == 0) count[m] = K;
}

struct Layout {   // the workspace: image table, counters, then every image's candidate list and selection buffer
    size_t counters, lists, total;
};
Layout layout(const int *heights, const int *widths, int n_images, int radius) {
    Layout L;
    L.counters = up256((size_t)n_images * sizeof(CornerImage));
    L.lists = L.counters + up256((size_t)n_images * sizeof(CornerCount));
    L.total = L.lists;
    for (int m = 0; m < n_images; ++m) {
        const size_t cap = corner_cap(heights[m], widths[m], radius);
        L.total += up256(cap * sizeof(Cand)) + up256(pow2ceil(cap) * sizeof(Cand));
    }
    return L;
}

int shapes_check(const int *heights, const int *widths, int n_images, int radius, const char *who) {
    if (!heights || !widths) return apap::fail(APAP_ERR_INVALID_ARG, "%s: null heights / widths", who);
    if (n_images < 1 || n_images > apap::kMaxImages)
        return apap::fail(APAP_ERR_INVALID_ARG, "%s: n_images = %d (1 .. %d)", who, n_images, apap::kMaxImages);
    if (radius < 1 || radius > kMaxRadius) return apap::fail(APAP_ERR_INVALID_ARG, "%s: radius = %d (1 .. %d)", who, radius, kMaxRadius);
    for (int m = 0; m < n_images; ++m)
        if (int rc = apap::image_sides_check(m, heights[m], widths[m], who)) return rc;
    return APAP_OK;
}

}  // namespace

namespace apap {

// The argument checks of the corner detector's entry points that need no device pointer.
int corner_check(const int *heights, const int *widths, const int *channels, int n_images, int max_corners, int radius,
                 int quality_permille, const char *who) {
    if (!channels) return apap::fail(APAP_ERR_INVALID_ARG, "%s: null channels", who);
    int rc = shapes_check(heights, widths, n_images, radius, who);
    if (rc) return rc;
    for (int m = 0; m < n_images; ++m)
        if ((rc = apap::image_channels_check(m, channels[m], who))) return rc;
    if (max_corners < 1) return apap::fail(APAP_ERR_INVALID_ARG, "%s: max_corners = %d (>= 1)", who, max_corners);
    if (quality_permille < 0 || quality_permille > 1000)
        return apap::fail(APAP_ERR_INVALID_ARG, "%s: quality_permille = %d (0 .. 1000)", who, quality_permille);
    return APAP_OK;
}

}  // namespace apap

extern "C" {

size_t apap_corner_workspace_bytes(const int *heights, const int *widths, int n_images, int radius) {
    if (shapes_check(heights, widths, n_images, radius, "apap_corner_workspace_bytes")) return 0;
    return layout(heights, widths, n_images, radius).total;
}

int apap_corner_detect_batch_device(apap_ctx *ctx, const uint8_t *const *d_imgs, const int *heights, const int *widths,
                                    const int *channels, int n_images, int max_corners, int radius, int quality_permille,
                                    float *d_pts, long long *d_response, int *d_count, void *d_work, size_t work_bytes, void *stream) {
    const char *who = "apap_corner_detect_batch_device";
    (void)ctx;
    int rc = apap::corner_check(heights, widths, channels, n_images, max_corners, radius, quality_permille, who);
    if (rc) return rc;
    if (!d_imgs || !d_pts || !d_response || !d_count || !d_work) return apap::fail(APAP_ERR_INVALID_ARG, "%s: null device pointer", who);
    for (int m = 0; m < n_images; ++m)
        if (!d_imgs[m]) return apap::fail(APAP_ERR_INVALID_ARG, "%s: image %d: null device pointer", who, m);
    const Layout L = layout(heights, widths, n_images, radius);
    if (work_bytes < L.total) return apap::fail(APAP_ERR_WORKSPACE, "%s: workspace %zu < %zu bytes", who, work_bytes, L.total);
    if (((uintptr_t)d_work & 255) != 0 || ((uintptr_t)d_pts & 7) != 0 || ((uintptr_t)d_response & 7) != 0 || ((uintptr_t)d_count & 3) != 0)
        return apap::fail(APAP_ERR_INVALID_ARG, "%s: workspace must be 256-byte, corners and responses 8-byte and counts 4-byte aligned", who);

    char *w = (char *)d_work;
    std::vector<CornerImage> tab((size_t)n_images);
    size_t at = L.lists;
    unsigned tiles = 0;
    for (int m = 0; m < n_images; ++m) {
        const size_t cap = corner_cap(heights[m], widths[m], radius);
        Cand *cand = (Cand *)(w + at);
        at += up256(cap * sizeof(Cand));
        Cand *sorted = (Cand *)(w + at);
        at += up256(pow2ceil(cap) * sizeof(Cand));
        tab[m] = CornerImage{d_imgs[m], cand, sorted, heights[m], widths[m], channels[m], (int)cap, 0};
        const unsigned t = (unsigned)((widths[m] + kTW - 1) / kTW) * (unsigned)((heights[m] + kTH - 1) / kTH);
        tiles = t > tiles ? t : tiles;
    }
    hipStream_t s = (hipStream_t)stream;
    // from pageable memory in stream order: the copy returns once its source has been consumed
    hipError_t e = hipMemcpyAsync(d_work, tab.data(), (size_t)n_images * sizeof(CornerImage), hipMemcpyHostToDevice, s);
    if (e != hipSuccess) return apap::hip_fail(e, "apap_corner_detect_batch_device: descriptor upload");
    e = hipMemsetAsync(w + L.counters, 0, (size_t)n_images * sizeof(CornerCount), s);
    if (e != hipSuccess) return apap::hip_fail(e, "apap_corner_detect_batch_device: counters");
    const CornerImage *d_tab = (const CornerImage *)d_work;
    CornerCount *d_cnt = (CornerCount *)(w + L.counters);
    if (radius <= kSmallRadius)
        hipLaunchKernelGGL(k_corner_tile<kSmallRadius>, dim3(tiles, (unsigned)n_images), dim3(kThreads), 0, s, d_tab, d_cnt, radius);
    else
        hipLaunchKernelGGL(k_corner_tile<kMaxRadius>, dim3(tiles, (unsigned)n_images), dim3(kThreads), 0, s, d_tab, d_cnt, radius);
    e = hipGetLastError();
    if (e != hipSuccess) return apap::hip_fail(e, "apap_corner_detect_batch_device: tile launch");
    hipLaunchKernelGGL(k_corner_select, dim3((unsigned)n_images), dim3(kSelThreads), 0, s, d_tab, (const CornerCount *)d_cnt, max_corners,
                       quality_permille, d_pts, d_response, d_count);
    e = hipGetLastError();
    if (e != hipSuccess) return apap::hip_fail(e, "apap_corner_detect_batch_device: select launch");
    return APAP_OK;
}

int apap_corner_detect_device(apap_ctx *ctx, const uint8_t *d_img, int h, int w, int channels, int max_corners, int radius,
                              int quality_permille, float *d_pts, long long *d_response, int *d_count, void *d_work, size_t work_bytes,
                              void *stream) {
    return apap_corner_detect_batch_device(ctx, &d_img, &h, &w, &channels, 1, max_corners, radius, quality_permille, d_pts, d_response,
                                           d_count, d_work, work_bytes, stream);
}

}  // extern "C"
