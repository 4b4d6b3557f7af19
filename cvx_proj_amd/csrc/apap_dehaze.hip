// Single-picture dehazing by the dark channel prior (He, Sun, Tang, CVPR 2009) with the guided filter (ECCV 2010) as the
// refinement of the transmission, in exact integers: tests/dehaze_spec.py is the definition, and every kernel here equals it
// byte for byte.  include/apap_hip.h states the definition next to the entry points.
//
// Five launches for any number of pictures of one shape (grid.y is the picture), no host wait between them:
//   D1 k_dehaze_dark          tile + halo of the channel minimum in LDS, row then column minimum -> D (uint8); a 256-bin
//                             histogram of the tile's D in LDS, one integer atomic per non-empty bin
//   D2 k_dehaze_airlight      every block derives the threshold T from the 256 counts itself, scans its pixels and sends at
//                             most one 64-bit atomicMax of (sum << 32) | (0xFFFFFFFF - index): the winner is the largest sum,
//                             the lowest index among equals, whatever the launch.  A stays in that device word: the later
//                             kernels read the winner's pixel.
//   D3 k_dehaze_transmission  the three 256-entry tables of min(4096, 4096 v / A_c) in LDS, tile + halo of n, row then column
//                             minimum, p = 4096 - ((omega_q Dn + 128) >> 8) -> uint16
//   D4 k_dehaze_ab            tile + halo of the guide G (grey_at, recomputed from the picture) and p in LDS, the four box sums
//                             as running column sums then row sums, one 64-bit floor division -> a_q (int32), b_q (int64)
//   D5 k_dehaze_recover       box sums of a_q and b_q (column sums from whole row segments of the L2, row sums from LDS), t, the clip, J
// Without refinement D4 is left out and D5 reads p as t.  Integers throughout: no result depends on a tile, a launch or an order.
// A tile's rows are stored by consecutive lanes: 128 bytes of D, 256 of p, 256 of a_q, 512 of b_q, 128 of t, 192 of J a row.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "apap_image_dev.h"
#include "apap_internal.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxR = APAP_DEHAZE_MAX_RADIUS;                 // of the minimum's window and of the guided filter's
constexpr int kMinRows = APAP_DEHAZE_MIN_TILE_ROWS, kMinCols = APAP_DEHAZE_MIN_TILE_COLS;   // D1, D3
constexpr int kAbRows = APAP_DEHAZE_AB_TILE_ROWS, kAbCols = APAP_DEHAZE_AB_TILE_COLS;       // D4
constexpr int kRecRows = APAP_DEHAZE_REC_TILE_ROWS, kRecCols = APAP_DEHAZE_REC_TILE_COLS;   // D5
constexpr int kRun = 4;                                       // outputs of one running sum
constexpr int kAirChunk = APAP_DEHAZE_AIR_CHUNK;              // consecutive pixels a block of D2 scans at a time
constexpr int kAirMaxBlocks = APAP_DEHAZE_AIR_MAX_BLOCKS;    // of D2's grid: a larger picture is scanned in passes
constexpr int kOne = 4096;                                    // 12 fractional bits
static_assert(kMinRows * kMinCols % kThreads == 0 && kAbRows * kAbCols == kRun * kThreads && kRecRows * kRecCols == kRun * kThreads, "tiles");
static_assert(kAbCols % kRun == 0 && kRecCols % kRun == 0 && kRecRows % kRun == 0, "runs");

struct Pictures {       // n pictures of one shape, one behind the other
    const uint8_t *img;
    int h, w, c;
    unsigned tiles_x;
};

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

// floor(a / b) for b > 0
__device__ __forceinline__ long long floor_div(long long a, long long b) {
    long long q = a / b;
    if (a - q * b < 0) --q;
    return q;
}
__device__ __forceinline__ int floor_div(int a, int b) {
    int q = a / b;
    if (a - q * b < 0) --q;
    return q;
}

template <class T>
__device__ __forceinline__ T lesser(T a, T b) { return b < a ? b : a; }

// The row then column minimum of a staged tile: tin holds rows_in x cols_in values, tmp rows_in x kMinCols row minima.
template <class T>
__device__ __forceinline__ void tile_row_min(const T *tin, T *tmp, int rows_in, int cols_in, int n) {
    for (int it = threadIdx.x; it < rows_in * kMinCols; it += kThreads) {
        const int ry = it / kMinCols, ox = it - ry * kMinCols;
        const T *src = tin + ry * cols_in + ox;
        T v = src[0];
        for (int j = 1; j < n; ++j) v = lesser(v, src[j]);
        tmp[it] = v;
    }
}
template <class T>
__device__ __forceinline__ T tile_col_min(const T *tmp, int oy, int ox, int n) {
    const T *src = tmp + oy * kMinCols + ox;
    T v = src[0];
    for (int j = 1; j < n; ++j) v = lesser(v, src[j * kMinCols]);
    return v;
}

// ---- D1.  Dynamic LDS: the 256 bins, then the tile plus halo [rows_in][cols_in], then the row minima [rows_in][kMinCols].
__host__ __device__ inline size_t dark_lds_bytes(int r) {
    return 256 * sizeof(unsigned) + (size_t)(kMinRows + 2 * r) * (2 * kMinCols + 2 * r);
}
__global__ __launch_bounds__(kThreads) void k_dehaze_dark(const Pictures P, int r, uint8_t *__restrict__ dark, unsigned *__restrict__ hist) {
    extern __shared__ __align__(16) uint8_t dark_lds[];
    const int h = P.h, w = P.w, c = P.c, n = 2 * r + 1, tid = threadIdx.x;
    const size_t N = (size_t)h * w;
    const uint8_t *__restrict__ img = P.img + (size_t)blockIdx.y * N * c;
    const int ty = (int)(blockIdx.x / P.tiles_x), tx = (int)(blockIdx.x - (unsigned)ty * P.tiles_x);
    const int y0 = ty * kMinRows, x0 = tx * kMinCols, rows_in = kMinRows + 2 * r, cols_in = kMinCols + 2 * r;
    unsigned *bins = (unsigned *)dark_lds;
    uint8_t *tin = dark_lds + 256 * sizeof(unsigned), *tmp = tin + rows_in * cols_in;
    bins[tid] = 0u;
    for (int it = tid; it < rows_in * cols_in; it += kThreads) {
        const int ry = it / cols_in, cx = it - ry * cols_in;
        const int y = clampi(y0 - r + ry, 0, h - 1), x = clampi(x0 - r + cx, 0, w - 1);
        const uint8_t *p = img + ((size_t)y * w + x) * c;
        int m = p[0];
        if (c == 3) m = min(m, min((int)p[1], (int)p[2]));
        tin[it] = (uint8_t)m;
    }
    __syncthreads();
    tile_row_min(tin, tmp, rows_in, cols_in, n);
    __syncthreads();
    for (int it = tid; it < kMinRows * kMinCols; it += kThreads) {
        const int oy = it / kMinCols, ox = it - oy * kMinCols;
        if (y0 + oy < h && x0 + ox < w) {
            const uint8_t v = tile_col_min(tmp, oy, ox, n);
            dark[blockIdx.y * N + (size_t)(y0 + oy) * w + x0 + ox] = v;
            atomicAdd(&bins[v], 1u);
        }
    }
    __syncthreads();
    if (bins[tid]) atomicAdd(&hist[(size_t)blockIdx.y * 256 + tid], bins[tid]);
}

// ---- D2
__global__ __launch_bounds__(kThreads) void k_dehaze_airlight(const Pictures P, const uint8_t *__restrict__ dark, const unsigned *__restrict__ hist,
                                                              unsigned long long *__restrict__ key) {
    __shared__ unsigned cnt[256];
    __shared__ int T_s;
    __shared__ unsigned long long best_s;
    const int c = P.c, tid = threadIdx.x;
    const long long N = (long long)P.h * P.w;
    const uint8_t *__restrict__ img = P.img + (size_t)blockIdx.y * N * c;
    const uint8_t *__restrict__ D = dark + (size_t)blockIdx.y * N;
    cnt[tid] = hist[(size_t)blockIdx.y * 256 + tid];
    if (tid == 0) {
        T_s = 0;
        best_s = 0ull;
    }
    __syncthreads();
    {   // the largest level with at least k pixels at or above it (level 0 has all N >= k)
        const unsigned k = (unsigned)max(1ll, N / 1000);
        unsigned at_least = 0u;
        for (int u = tid; u < 256; ++u) at_least += cnt[u];
        if (at_least >= k) atomicMax(&T_s, tid);
    }
    __syncthreads();
    const int T = T_s;
    unsigned long long best = 0ull;
    for (long long base = (long long)blockIdx.x * kAirChunk; base < N; base += (long long)gridDim.x * kAirChunk) {
        const long long end = min(base + kAirChunk, N);
        for (long long i = base + tid; i < end; i += kThreads) {
            if (D[i] < T) continue;
            const uint8_t *p = img + (size_t)i * c;
            unsigned s = p[0];
            if (c == 3) s += (unsigned)p[1] + (unsigned)p[2];
            const unsigned long long cand = ((unsigned long long)s << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)i);
            best = cand > best ? cand : best;
        }
    }
    if (best) atomicMax(&best_s, best);
    __syncthreads();
    if (tid == 0 && best_s) atomicMax(&key[blockIdx.y], best_s);
}

// A of a picture from its winner's word: the pixel's channels, each at least 1.
__device__ __forceinline__ void airlight_of(const uint8_t *img, unsigned long long key, int c, int *A) {
    const size_t at = (size_t)(0xFFFFFFFFu - (unsigned)key) * c;
    for (int ch = 0; ch < 3; ++ch) A[ch] = ch < c ? max(1, (int)img[at + ch]) : 1;
}

// A alone (apap_atmospheric_light): one lane per picture
__global__ __launch_bounds__(kThreads) void k_dehaze_write_A(const Pictures P, int n_images, const unsigned long long *__restrict__ key,
                                                              uint8_t *__restrict__ A_out) {
    const int m = blockIdx.x * kThreads + threadIdx.x;
    if (m >= n_images) return;
    int A[3];
    airlight_of(P.img + (size_t)m * P.h * P.w * P.c, key[m], P.c, A);
    for (int ch = 0; ch < P.c; ++ch) A_out[m * P.c + ch] = (uint8_t)A[ch];
}

// ---- D3.  Dynamic LDS, uint16: the three tables, then the tile plus halo [rows_in][cols_in], then the row minima [rows_in][kMinCols].
__host__ __device__ inline size_t trans_lds_bytes(int r) {
    return (3 * 256 + (size_t)(kMinRows + 2 * r) * (2 * kMinCols + 2 * r)) * sizeof(uint16_t);
}
__global__ __launch_bounds__(kThreads) void k_dehaze_transmission(const Pictures P, int r, int omega_q, int lo, const unsigned long long *__restrict__ key,
                                                                  uint16_t *__restrict__ trans, uint8_t *__restrict__ A_out) {
    extern __shared__ __align__(16) uint8_t trans_lds[];
    const int h = P.h, w = P.w, c = P.c, n = 2 * r + 1, tid = threadIdx.x;
    const size_t N = (size_t)h * w;
    const uint8_t *__restrict__ img = P.img + (size_t)blockIdx.y * N * c;
    const int ty = (int)(blockIdx.x / P.tiles_x), tx = (int)(blockIdx.x - (unsigned)ty * P.tiles_x);
    const int y0 = ty * kMinRows, x0 = tx * kMinCols, rows_in = kMinRows + 2 * r, cols_in = kMinCols + 2 * r;
    uint16_t(*tab)[256] = (uint16_t(*)[256])trans_lds;
    uint16_t *tin = (uint16_t *)trans_lds + 3 * 256, *tmp = tin + rows_in * cols_in;
    int A[3];
    airlight_of(img, key[blockIdx.y], c, A);
    for (int ch = 0; ch < c; ++ch) tab[ch][tid] = (uint16_t)min(kOne, kOne * tid / A[ch]);
    if (A_out && blockIdx.x == 0 && tid < c) A_out[blockIdx.y * c + tid] = (uint8_t)A[tid];
    __syncthreads();
    for (int it = tid; it < rows_in * cols_in; it += kThreads) {
        const int ry = it / cols_in, cx = it - ry * cols_in;
        const int y = clampi(y0 - r + ry, 0, h - 1), x = clampi(x0 - r + cx, 0, w - 1);
        const uint8_t *p = img + ((size_t)y * w + x) * c;
        uint16_t m = tab[0][p[0]];
        if (c == 3) m = lesser(m, lesser(tab[1][p[1]], tab[2][p[2]]));
        tin[it] = m;
    }
    __syncthreads();
    tile_row_min(tin, tmp, rows_in, cols_in, n);
    __syncthreads();
    for (int it = tid; it < kMinRows * kMinCols; it += kThreads) {
        const int oy = it / kMinCols, ox = it - oy * kMinCols;
        if (y0 + oy < h && x0 + ox < w) {
            const int dn = tile_col_min(tmp, oy, ox, n);
            const int p = kOne - ((omega_q * dn + 128) >> 8);
            trans[blockIdx.y * N + (size_t)(y0 + oy) * w + x0 + ox] = (uint16_t)max(p, lo);
        }
    }
}

// ---- D4.  Dynamic LDS: uint4 column sums [kAbRows][cols_in], then p [rows_in][cols_in] uint16, then G [rows_in][cols_in] uint8.
// Columns first: the column sums of kAbRows output rows take less room than the row sums of rows_in rows would.
constexpr int kAbColRun = 4;
static_assert(kAbRows % kAbColRun == 0, "column runs");
__host__ __device__ inline size_t ab_lds_bytes(int rho) {
    const size_t rows_in = kAbRows + 2 * rho, cols_in = kAbCols + 2 * rho;
    return kAbRows * cols_in * 16 + rows_in * cols_in * 3;
}
__global__ __launch_bounds__(kThreads) void k_dehaze_ab(const Pictures P, int rho, long long eps_w2, const uint16_t *__restrict__ trans,
                                                        int *__restrict__ a_out, long long *__restrict__ b_out) {
    extern __shared__ __align__(16) uint8_t ab_lds[];
    const int h = P.h, w = P.w, c = P.c, n = 2 * rho + 1, tid = threadIdx.x;
    const size_t N = (size_t)h * w;
    const uint8_t *__restrict__ img = P.img + (size_t)blockIdx.y * N * c;
    const uint16_t *__restrict__ tp_g = trans + blockIdx.y * N;
    const int ty = (int)(blockIdx.x / P.tiles_x), tx = (int)(blockIdx.x - (unsigned)ty * P.tiles_x);
    const int y0 = ty * kAbRows, x0 = tx * kAbCols, rows_in = kAbRows + 2 * rho, cols_in = kAbCols + 2 * rho;
    uint4 *cs = (uint4 *)ab_lds;
    uint16_t *tp = (uint16_t *)(ab_lds + (size_t)kAbRows * cols_in * 16);
    uint8_t *tg = (uint8_t *)(tp + rows_in * cols_in);
    for (int it = tid; it < rows_in * cols_in; it += kThreads) {
        const int ry = it / cols_in, cx = it - ry * cols_in;
        const int y = clampi(y0 - rho + ry, 0, h - 1), x = clampi(x0 - rho + cx, 0, w - 1);
        tg[it] = (uint8_t)apap::grey_at(img, y, x, w, c);
        tp[it] = tp_g[(size_t)y * w + x];
    }
    __syncthreads();
    // columns: sums of G, G G, p and G p over n taps (at most 65 x 255 x 4096 < 2^27), running over kAbColRun output rows
    for (int it = tid; it < cols_in * (kAbRows / kAbColRun); it += kThreads) {
        const int part = it / cols_in, cx = it - part * cols_in, oy0 = part * kAbColRun;
        const uint8_t *g = tg + oy0 * cols_in + cx;
        const uint16_t *p = tp + oy0 * cols_in + cx;
        unsigned sg = 0u, sgg = 0u, sp = 0u, sgp = 0u;
        for (int j = 0; j < n; ++j) {
            const unsigned gv = g[j * cols_in], pv = p[j * cols_in];
            sg += gv;
            sgg += gv * gv;
            sp += pv;
            sgp += gv * pv;
        }
        cs[oy0 * cols_in + cx] = make_uint4(sg, sgg, sp, sgp);
#pragma unroll
        for (int i = 1; i < kAbColRun; ++i) {
            const unsigned ga = g[(i - 1 + n) * cols_in], pa = p[(i - 1 + n) * cols_in], gs = g[(i - 1) * cols_in], ps = p[(i - 1) * cols_in];
            sg += ga - gs;
            sgg += ga * ga - gs * gs;
            sp += pa - ps;
            sgp += ga * pa - gs * ps;
            cs[(oy0 + i) * cols_in + cx] = make_uint4(sg, sgg, sp, sgp);
        }
    }
    __syncthreads();
    // rows: one lane owns kRun neighbouring outputs of a row; S(G p) reaches 2^32.04 and is summed in 64 bits
    const int oy = tid / (kAbCols / kRun), ox0 = (tid - oy * (kAbCols / kRun)) * kRun, y = y0 + oy;
    const uint4 *row = cs + oy * cols_in + ox0;
    unsigned SG = 0u, SGG = 0u, SP = 0u;
    unsigned long long SGP = 0ull;
    for (int j = 0; j < n; ++j) {
        const uint4 v = row[j];
        SG += v.x;
        SGG += v.y;
        SP += v.z;
        SGP += v.w;
    }
    const long long W = (long long)n * n;
    for (int i = 0; i < kRun; ++i) {
        if (i) {
            const uint4 add = row[i - 1 + n], sub = row[i - 1];
            SG += add.x - sub.x;
            SGG += add.y - sub.y;
            SP += add.z - sub.z;
            SGP += (unsigned long long)add.w - (unsigned long long)sub.w;
        }
        const int x = x0 + ox0 + i;
        if (y < h && x < w) {
            const long long covN = W * (long long)SGP - (long long)SG * (long long)SP;
            const long long varN = W * (long long)SGG - (long long)SG * (long long)SG;
            const long long a_q = floor_div(kOne * covN, varN + eps_w2);
            const size_t at = blockIdx.y * N + (size_t)y * w + x;
            a_out[at] = (int)a_q;
            b_out[at] = kOne * (long long)SP - a_q * (long long)SG;
        }
    }
}

// ---- D5.  Columns first, so that every global read is a whole row segment: a lane owns one column of the tile plus halo and
// kColRun output rows, and runs the sums of a_q and b_q down the column (consecutive lanes, consecutive addresses); the column sums
// go to LDS - int64 of b_q [kRecRows][cols_in], then int32 of a_q [kRecRows][cols_in] (|a_q| < 2^23, 65 taps) - and a lane then
// runs the row sums of kRun neighbouring outputs from there.  The tile's J bytes are staged over the dead column sums.
// rho = 0: no LDS phase, t = p (clipped by D3 already).
constexpr int kColRun = 8;
static_assert(kRecRows % kColRun == 0 && (kRecCols + 2 * kMaxR) * (kRecRows / kColRun) <= kThreads, "one column item a lane");
__host__ __device__ inline size_t rec_lds_bytes(int rho) {
    return rho ? (size_t)kRecRows * (kRecCols + 2 * rho) * 12 : (size_t)kRecRows * kRecCols * 3;
}
__global__ __launch_bounds__(kThreads) void k_dehaze_recover(const Pictures P, int rho, int t0_q, const unsigned long long *__restrict__ key,
                                                             const uint16_t *__restrict__ trans, const int *__restrict__ a_in,
                                                             const long long *__restrict__ b_in, uint16_t *__restrict__ t_out,
                                                             uint8_t *__restrict__ J_out) {
    extern __shared__ __align__(16) uint8_t rec_lds[];
    const int h = P.h, w = P.w, c = P.c, n = 2 * rho + 1, tid = threadIdx.x;
    const size_t N = (size_t)h * w;
    const uint8_t *__restrict__ img = P.img + (size_t)blockIdx.y * N * c;
    const int ty = (int)(blockIdx.x / P.tiles_x), tx = (int)(blockIdx.x - (unsigned)ty * P.tiles_x);
    const int y0 = ty * kRecRows, x0 = tx * kRecCols, cols_in = kRecCols + 2 * rho;
    long long *cb = (long long *)rec_lds;
    int *ca = (int *)(rec_lds + (size_t)kRecRows * cols_in * 8);
    if (rho) {
        const int *__restrict__ a_g = a_in + blockIdx.y * N;
        const long long *__restrict__ b_g = b_in + blockIdx.y * N;
        if (tid < cols_in * (kRecRows / kColRun)) {
            const int part = tid / cols_in, cx = tid - part * cols_in, oy0 = part * kColRun;
            const int x = clampi(x0 - rho + cx, 0, w - 1), ys = y0 + oy0 - rho;
            int sa = 0;
            long long sb = 0;
            for (int j = 0; j < n; ++j) {
                const size_t at = (size_t)clampi(ys + j, 0, h - 1) * w + x;
                sa += a_g[at];
                sb += b_g[at];
            }
            ca[oy0 * cols_in + cx] = sa;
            cb[oy0 * cols_in + cx] = sb;
            for (int i = 1; i < kColRun; ++i) {
                const size_t add = (size_t)clampi(ys + i - 1 + n, 0, h - 1) * w + x, sub = (size_t)clampi(ys + i - 1, 0, h - 1) * w + x;
                sa += a_g[add] - a_g[sub];
                sb += b_g[add] - b_g[sub];
                ca[(oy0 + i) * cols_in + cx] = sa;
                cb[(oy0 + i) * cols_in + cx] = sb;
            }
        }
        __syncthreads();
    }
    // rows: one lane owns kRun neighbouring outputs of a row
    const int oy = tid / (kRecCols / kRun), ox0 = (tid - oy * (kRecCols / kRun)) * kRun, y = y0 + oy;
    int tq[kRun];
    if (rho) {
        const int *ra = ca + oy * cols_in + ox0;
        const long long *rb = cb + oy * cols_in + ox0;
        long long SA = 0, SB = 0;
        for (int j = 0; j < n; ++j) {
            SA += ra[j];
            SB += rb[j];
        }
        const long long W = (long long)n * n, den = kOne * W * W;
        for (int i = 0; i < kRun; ++i) {
            if (i) {
                SA += ra[i - 1 + n] - ra[i - 1];
                SB += rb[i - 1 + n] - rb[i - 1];
            }
            const int x = x0 + ox0 + i;
            long long t = t0_q;
            if (y < h && x < w) t = floor_div(SA * (long long)apap::grey_at(img, y, x, w, c) * W + SB, den);
            tq[i] = (int)min(max(t, (long long)t0_q), (long long)kOne);
        }
        __syncthreads();    // the column sums are dead: J is staged over them
    } else {
        for (int i = 0; i < kRun; ++i) {
            const int x = x0 + ox0 + i;
            tq[i] = y < h && x < w ? (int)trans[blockIdx.y * N + (size_t)y * w + x] : t0_q;
        }
    }
    uint8_t *tj = rec_lds;
    int A[3];
    airlight_of(img, key[blockIdx.y], c, A);
    for (int i = 0; i < kRun; ++i) {
        const int x = x0 + ox0 + i;
        if (y >= h || x >= w) continue;
        const int t = tq[i];
        if (t_out) t_out[blockIdx.y * N + (size_t)y * w + x] = (uint16_t)t;
        if (J_out) {
            const uint8_t *p = img + ((size_t)y * w + x) * c;
            for (int ch = 0; ch < c; ++ch)
                tj[(oy * kRecCols + ox0 + i) * c + ch] = (uint8_t)clampi(A[ch] + floor_div(2 * kOne * ((int)p[ch] - A[ch]) + t, 2 * t), 0, 255);
        }
    }
    if (!J_out) return;
    __syncthreads();
    const int row_bytes = min(kRecCols, w - x0) * c;      // of the tile's part of a picture's row
    for (int it = tid; it < kRecRows * kRecCols * c; it += kThreads) {
        const int ry = it / (kRecCols * c), e = it - ry * (kRecCols * c);
        if (y0 + ry < h && e < row_bytes) J_out[(blockIdx.y * N + (size_t)(y0 + ry) * w + x0) * c + e] = tj[it];
    }
}

// ---------------------------------------------------------------- host side
unsigned tiles(int n, int side) { return (unsigned)((n + side - 1) / side); }

struct Workspace {
    unsigned long long *key;
    unsigned *hist;
    uint8_t *dark;
    uint16_t *p;
    int *a;
    long long *b;
};
size_t head_bytes(int n) { return apap::up256((size_t)n * (8 + 256 * 4)); }
Workspace carve(void *d_work, int n, size_t N, int refine) {
    char *at = (char *)d_work;
    Workspace ws{};
    ws.key = (unsigned long long *)at;
    ws.hist = (unsigned *)(at + (size_t)n * 8);
    at += head_bytes(n);
    ws.dark = (uint8_t *)at;
    at += apap::up256(n * N);
    ws.p = (uint16_t *)at;
    at += apap::up256(n * N * 2);
    if (refine) {
        ws.a = (int *)at;
        at += apap::up256(n * N * 4);
        ws.b = (long long *)at;
    }
    return ws;
}

int launched(const char *who) {
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? APAP_OK : apap::hip_fail((int)e, who);
}

}  // namespace

namespace apap {

int dehaze_check(int n_images, int h, int w, int channels, int radius, int omega_q, int t0_q, int refine, int eps, const char *who) {
    if (n_images < 1 || n_images > kMaxImages) return fail(APAP_ERR_INVALID_ARG, "%s: %d pictures (1 .. %d)", who, n_images, kMaxImages);
    if (h < 1 || w < 1 || (long long)h * w >= (1ll << 31))
        return fail(APAP_ERR_INVALID_ARG, "%s: a picture of %d x %d (sides at least 1, fewer than 2^31 pixels)", who, h, w);
    if (channels != 1 && channels != 3) return fail(APAP_ERR_INVALID_ARG, "%s: %d channels (1 = grey or 3 = BGR)", who, channels);
    if (radius < 0 || radius > APAP_DEHAZE_MAX_RADIUS) return fail(APAP_ERR_INVALID_ARG, "%s: radius=%d (0 .. %d)", who, radius, APAP_DEHAZE_MAX_RADIUS);
    if (omega_q < 0 || omega_q > 256) return fail(APAP_ERR_INVALID_ARG, "%s: omega_q=%d (0 .. 256)", who, omega_q);
    if (t0_q < 1 || t0_q > kOne) return fail(APAP_ERR_INVALID_ARG, "%s: t0_q=%d (1 .. %d)", who, t0_q, kOne);
    if (refine < 0 || refine > APAP_DEHAZE_MAX_RADIUS) return fail(APAP_ERR_INVALID_ARG, "%s: refine=%d (0 .. %d)", who, refine, APAP_DEHAZE_MAX_RADIUS);
    if (eps < 1 || eps > 65535) return fail(APAP_ERR_INVALID_ARG, "%s: eps=%d (1 .. 65535)", who, eps);
    return APAP_OK;
}

// The stages that the outputs asked for need, on `stream`; does not wait.  Any of d_dark, d_A, d_t, d_J may be null.
int dehaze_run(const uint8_t *d_imgs, int n_images, int h, int w, int channels, int radius, int omega_q, int t0_q, int refine, int eps,
               uint8_t *d_dark, uint8_t *d_A, uint16_t *d_t, uint8_t *d_J, void *d_work, size_t work_bytes, void *stream, const char *who) {
    int rc = dehaze_check(n_images, h, w, channels, radius, omega_q, t0_q, refine, eps, who);
    if (rc) return rc;
    if (!d_imgs || !d_work || !(d_dark || d_A || d_t || d_J)) return fail(APAP_ERR_INVALID_ARG, "%s: null device pointer", who);
    const bool guided = refine > 0 && (d_t || d_J);
    const size_t need = apap_dehaze_workspace_bytes(n_images, h, w, channels, guided ? refine : 0);
    if (work_bytes < need) return fail(APAP_ERR_WORKSPACE, "%s: workspace %zu < %zu bytes", who, work_bytes, need);
    if (((uintptr_t)d_work & 255) != 0) return fail(APAP_ERR_INVALID_ARG, "%s: workspace not 256-byte aligned", who);
    hipStream_t s = (hipStream_t)stream;
    const size_t N = (size_t)h * w;
    const Workspace ws = carve(d_work, n_images, N, guided ? refine : 0);
    Pictures P{d_imgs, h, w, channels, tiles(w, kMinCols)};
    const dim3 block(kThreads), min_grid(P.tiles_x * tiles(h, kMinRows), (unsigned)n_images);
    // the counts and the winners' words start at zero; this workspace promises nothing between calls
    const hipError_t e = hipMemsetAsync(d_work, 0, head_bytes(n_images), s);
    if (e != hipSuccess) return hip_fail((int)e, who);
    uint8_t *dark = d_dark ? d_dark : ws.dark;
    hipLaunchKernelGGL(k_dehaze_dark, min_grid, block, dark_lds_bytes(radius), s, P, radius, dark, ws.hist);
    if ((rc = launched(who))) return rc;
    if (!(d_A || d_t || d_J)) return APAP_OK;
    const unsigned air_blocks = (unsigned)std::min<size_t>((N + kAirChunk - 1) / kAirChunk, kAirMaxBlocks);
    hipLaunchKernelGGL(k_dehaze_airlight, dim3(air_blocks, (unsigned)n_images), block, 0, s, P, (const uint8_t *)dark, (const unsigned *)ws.hist, ws.key);
    if ((rc = launched(who))) return rc;
    if (!(d_t || d_J)) {
        hipLaunchKernelGGL(k_dehaze_write_A, dim3(tiles(n_images, kThreads)), block, 0, s, P, n_images, (const unsigned long long *)ws.key, d_A);
        return launched(who);
    }
    const bool direct = !guided && !d_J;      // the raw transmission, clipped, is the result
    hipLaunchKernelGGL(k_dehaze_transmission, min_grid, block, trans_lds_bytes(radius), s, P, radius, omega_q, guided ? 0 : t0_q, (const unsigned long long *)ws.key,
                       direct ? d_t : ws.p, d_A);
    if ((rc = launched(who)) || direct) return rc;
    if (guided) {
        const long long W = (long long)(2 * refine + 1) * (2 * refine + 1);
        P.tiles_x = tiles(w, kAbCols);
        hipLaunchKernelGGL(k_dehaze_ab, dim3(P.tiles_x * tiles(h, kAbRows), (unsigned)n_images), block, ab_lds_bytes(refine), s, P, refine,
                           (long long)eps * W * W, (const uint16_t *)ws.p, ws.a, ws.b);
        if ((rc = launched(who))) return rc;
    }
    P.tiles_x = tiles(w, kRecCols);
    hipLaunchKernelGGL(k_dehaze_recover, dim3(P.tiles_x * tiles(h, kRecRows), (unsigned)n_images), block, rec_lds_bytes(guided ? refine : 0), s, P,
                       guided ? refine : 0, t0_q, (const unsigned long long *)ws.key, (const uint16_t *)ws.p, (const int *)ws.a,
                       (const long long *)ws.b, d_t, d_J);
    return launched(who);
}

}  // namespace apap

extern "C" {

size_t apap_dehaze_workspace_bytes(int n_images, int h, int w, int channels, int refine) {
    if (apap::dehaze_check(n_images, h, w, channels, 0, 0, 1, refine, 1, "apap_dehaze_workspace_bytes")) return 0;
    const size_t N = (size_t)h * w * n_images;
    return head_bytes(n_images) + apap::up256(N) + apap::up256(N * 2) + (refine ? apap::up256(N * 4) + apap::up256(N * 8) : 0);
}

int apap_dark_channel_device(apap_ctx *ctx, const uint8_t *d_imgs, int n_images, int h, int w, int channels, int radius, uint8_t *d_dark,
                             void *d_work, size_t work_bytes, void *stream) {
    (void)ctx;
    return apap::dehaze_run(d_imgs, n_images, h, w, channels, radius, 0, 1, 0, 1, d_dark, nullptr, nullptr, nullptr, d_work, work_bytes, stream,
                            "apap_dark_channel_device");
}

int apap_atmospheric_light_device(apap_ctx *ctx, const uint8_t *d_imgs, int n_images, int h, int w, int channels, int radius, uint8_t *d_A,
                                  void *d_work, size_t work_bytes, void *stream) {
    (void)ctx;
    return apap::dehaze_run(d_imgs, n_images, h, w, channels, radius, 0, 1, 0, 1, nullptr, d_A, nullptr, nullptr, d_work, work_bytes, stream,
                            "apap_atmospheric_light_device");
}

int apap_transmission_device(apap_ctx *ctx, const uint8_t *d_imgs, int n_images, int h, int w, int channels, int radius, int omega_q, int t0_q,
                             int refine, int eps, uint16_t *d_t, void *d_work, size_t work_bytes, void *stream) {
    (void)ctx;
    return apap::dehaze_run(d_imgs, n_images, h, w, channels, radius, omega_q, t0_q, refine, eps, nullptr, nullptr, d_t, nullptr, d_work,
                            work_bytes, stream, "apap_transmission_device");
}

int apap_dehaze_device(apap_ctx *ctx, const uint8_t *d_imgs, int n_images, int h, int w, int channels, int radius, int omega_q, int t0_q,
                       int refine, int eps, uint8_t *d_out, uint16_t *d_t, uint8_t *d_A, void *d_work, size_t work_bytes, void *stream) {
    (void)ctx;
    if (!d_out) return apap::fail(APAP_ERR_INVALID_ARG, "apap_dehaze_device: null device pointer");
    return apap::dehaze_run(d_imgs, n_images, h, w, channels, radius, omega_q, t0_q, refine, eps, nullptr, d_A, d_t, d_out, d_work, work_bytes,
                            stream, "apap_dehaze_device");
}

}  // extern "C"
