// Notch denoising of periodic noise (pyviz/median_filter.py apply_median_filter), device half: equalise, 2-D FFT, replace
// small discs around the noise lattice's harmonics by the median of a larger disc, inverse FFT, magnitude.
// Specification: tests/denoise_spec.py, byte for byte.  complex128 throughout, every complex product spelt out as
// (ac - bd, ad + bc) (the library is built with -ffp-contract=off), twiddles from one host table (apap_fft_twiddles).
//   F1 k_fft_pass<.., false>: rows.  A block holds one row (several short ones) in LDS and runs the mixed-radix (4, 2, 3, 5)
//      Stockham stages between two LDS buffers.  The loader reads complex128 or the uint8 picture itself (no float copy of
//      the picture exists); the writer stores complex128 or only the magnitude (float64 / uint8) of the scaled value.
//   F2 k_fft_pass<.., true>: columns, the same stages over a strip of adjacent columns held interleaved in LDS, so that a
//      global access covers the strip's width of consecutive complex128 values.
//      Columns of more than 1024 points (a strip of four would not fit) go through T1 k_transpose: the plane is turned
//      through 32 x 32 LDS tiles, its columns are transformed by F1 as rows, and it is turned back.
//   N1 k_notch: one block per distinct centre of the schedule and plane.  The clipped read disc is gathered into LDS in
//      row-major order (its rows' extents are known in closed form, so no atomics), the lexicographic median is the middle of
//      a bitonic sort in LDS, the inner disc is written in place.  Where two of a call's four centres coincide (the axis terms) the
//      block applies both assignments in order on its LDS copy.
// Every distinct centre reads the ORIGINAL spectrum: for spacing > max(6r, 5r + 3) no write disc meets another centre's read
// disc (DESIGN.md "Notch denoising"), which the argument check enforces.
#include <hip/hip_runtime.h>

#include <atomic>
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <map>
#include <mutex>
#include <vector>

#include "apap_internal.h"

namespace {

constexpr int kFftThreads = 256;       // a block of short transforms
constexpr int kFftThreadsLong = 1024;  // ... of 2048 points or more: a butterfly or two a thread, since only one or two such blocks fit a CU
constexpr int kFftLdsPoints = 4096;     // complex128 points in each of a block's two LDS buffers: 2 x 64 KiB of the CU's 160 KiB
constexpr int kFftMaxRows = 8;          // short rows per block
constexpr int kFftMaxStrip = 16;        // columns per strip

// the radix-3 and radix-5 constants (tests/denoise_spec.py writes the same literals)
constexpr double kSin3 = 0.8660254037844386;      // sin(2 pi / 3)
constexpr double kCos5a = 0.30901699437494745;    // cos(2 pi / 5)
constexpr double kCos5b = -0.8090169943749475;    // cos(4 pi / 5)
constexpr double kSin5a = 0.9510565162951535;     // sin(2 pi / 5)
constexpr double kSin5b = 0.5877852522924731;     // sin(4 pi / 5)

enum { kInU8 = 0, kInC128 = 1 };
enum { kOutC128 = 0, kOutMagF64 = 1, kOutMagU8 = 2 };

// One pass over `planes` planes (grid.y): `count` transforms of length n each, `per_block` of them per block.
// complex128 planes are [rows][row_len]; a row pass has n = row_len, count = rows, a column pass n = rows, count = row_len.
// The uint8 input and the magnitude output are pictures of `channels` interleaved channels: plane p is channel p % channels of
// picture p / channels.
struct FftPass {
    const void *in;
    void *out;
    const double2 *tw;      // n entries: (cos, sin) of -2 pi k / n
    int n, count, per_block, channels;
    double sign;            // +1 forward, -1 inverse (the conjugate table)
    int scaled;             // the writer multiplies real and imaginary part by `scale`
    double scale;
};

__device__ __forceinline__ double2 cadd(double2 a, double2 b) { return double2{a.x + b.x, a.y + b.y}; }
__device__ __forceinline__ double2 csub(double2 a, double2 b) { return double2{a.x - b.x, a.y - b.y}; }
__device__ __forceinline__ double2 cmul(double2 a, double2 w) { return double2{a.x * w.x - a.y * w.y, a.x * w.y + a.y * w.x}; }
__device__ __forceinline__ double2 cscale(double c, double2 a) { return double2{c * a.x, c * a.y}; }
// -i sg u: the quarter turn of the forward transform (sg = 1), its opposite for the inverse
__device__ __forceinline__ double2 cturn(double2 u, double sg) { return double2{sg * u.y, -(sg * u.x)}; }

template <int P>
__device__ __forceinline__ void butterfly(double2 (&a)[P], double sg);

template <>
__device__ __forceinline__ void butterfly<2>(double2 (&a)[2], double) {
    const double2 y0 = cadd(a[0], a[1]), y1 = csub(a[0], a[1]);
    a[0] = y0; a[1] = y1;
}
template <>
__device__ __forceinline__ void butterfly<4>(double2 (&a)[4], double sg) {
    const double2 t0 = cadd(a[0], a[2]), t1 = csub(a[0], a[2]), t2 = cadd(a[1], a[3]), t3 = cturn(csub(a[1], a[3]), sg);
    a[0] = cadd(t0, t2); a[1] = cadd(t1, t3); a[2] = csub(t0, t2); a[3] = csub(t1, t3);
}
template <>
__device__ __forceinline__ void butterfly<3>(double2 (&a)[3], double sg) {
    const double2 t1 = cadd(a[1], a[2]), t2 = csub(a[1], a[2]);
    const double2 m = csub(a[0], cscale(0.5, t1)), u = cturn(cscale(kSin3, t2), sg);
    a[0] = cadd(a[0], t1); a[1] = cadd(m, u); a[2] = csub(m, u);
}
template <>
__device__ __forceinline__ void butterfly<5>(double2 (&a)[5], double sg) {
    const double2 t1 = cadd(a[1], a[4]), t2 = cadd(a[2], a[3]), t3 = csub(a[1], a[4]), t4 = csub(a[2], a[3]);
    const double2 m1 = cadd(cadd(a[0], cscale(kCos5a, t1)), cscale(kCos5b, t2));
    const double2 m2 = cadd(cadd(a[0], cscale(kCos5b, t1)), cscale(kCos5a, t2));
    const double2 u1 = cturn(cadd(cscale(kSin5a, t3), cscale(kSin5b, t4)), sg);
    const double2 u2 = cturn(csub(cscale(kSin5b, t3), cscale(kSin5a, t4)), sg);
    a[0] = cadd(cadd(a[0], t1), t2);
    a[1] = cadd(m1, u1); a[4] = csub(m1, u1);
    a[2] = cadd(m2, u2); a[3] = csub(m2, u2);
}

// One Stockham stage of radix P over `nb` transforms: element e of transform b is at b * bstride + e * estride.  s is the
// product of the earlier radices, m = n / (s P).  Butterfly (q, j) reads e = j + s (q + m k), writes e = j + s (P q + k)
// after the twiddle w^(q k s), k = 0 .. P - 1.
template <int P>
__device__ __forceinline__ void fft_stage(const double2 *src, double2 *dst, const double2 *__restrict__ tw, int n, int s, int m,
                                          int nb, int estride, int bstride, double sg) {
    const int per = n / P;
    for (int id = threadIdx.x; id < nb * per; id += blockDim.x) {
        const int b = id / per, r = id - b * per, q = r / s, j = r - q * s;
        const int base = b * bstride;
        double2 a[P];
#pragma unroll
        for (int k = 0; k < P; ++k) a[k] = src[base + (j + s * (q + m * k)) * estride];
        butterfly<P>(a, sg);
#pragma unroll
        for (int k = 0; k < P; ++k) {
            double2 y = a[k];
            if (k > 0) {
                double2 w = tw[q * k * s];
                w.y = sg * w.y;
                y = cmul(y, w);
            }
            dst[base + (j + s * (P * q + k)) * estride] = y;
        }
    }
}

// the radix of the next stage of a length whose remaining factor is rem: 4 while it divides, then 2, 3, 5
__host__ __device__ __forceinline__ int fft_radix(int rem) { return rem % 4 == 0 ? 4 : rem % 2 == 0 ? 2 : rem % 3 == 0 ? 3 : 5; }

template <int IN, int OUT, bool COLS>
__global__ __launch_bounds__(kFftThreadsLong) void k_fft_pass(const FftPass p) {
    extern __shared__ double2 s_fft[];
    const int n = p.n, nb = p.per_block, first = blockIdx.x * nb;
    const int estride = COLS ? nb : 1, bstride = COLS ? 1 : n;
    const size_t plane = blockIdx.y, plane_pts = (size_t)n * p.count;
    const size_t pic = plane / p.channels * plane_pts * p.channels + plane % p.channels;   // of the uint8 / magnitude picture
    double2 *src = s_fft, *dst = s_fft + nb * n;
    for (int e = threadIdx.x; e < nb * n; e += blockDim.x) {
        // rows: consecutive threads along the row; columns: along the strip
        const int b = COLS ? e % nb : e / n, k = COLS ? e / nb : e % n, t = first + b;
        double2 v = double2{0.0, 0.0};
        if (t < p.count) {
            const size_t at = COLS ? (size_t)k * p.count + t : (size_t)t * n + k;
            if (IN == kInU8) v.x = (double)((const uint8_t *)p.in)[pic + at * p.channels];
            else v = ((const double2 *)p.in)[plane * plane_pts + at];
        }
        src[b * bstride + k * estride] = v;
    }
    __syncthreads();
    for (int rem = n, s = 1; rem > 1;) {
        const int radix = fft_radix(rem), m = rem / radix;
        if (radix == 4) fft_stage<4>(src, dst, p.tw, n, s, m, nb, estride, bstride, p.sign);
        else if (radix == 2) fft_stage<2>(src, dst, p.tw, n, s, m, nb, estride, bstride, p.sign);
        else if (radix == 3) fft_stage<3>(src, dst, p.tw, n, s, m, nb, estride, bstride, p.sign);
        else fft_stage<5>(src, dst, p.tw, n, s, m, nb, estride, bstride, p.sign);
        __syncthreads();
        double2 *const swap = src;
        src = dst;
        dst = swap;
        s *= radix;
        rem = m;
    }
    for (int e = threadIdx.x; e < nb * n; e += blockDim.x) {
        const int b = COLS ? e % nb : e / n, k = COLS ? e / nb : e % n, t = first + b;
        if (t >= p.count) continue;
        double2 v = src[b * bstride + k * estride];
        if (p.scaled) v = cscale(p.scale, v);
        const size_t at = COLS ? (size_t)k * p.count + t : (size_t)t * n + k;
        if (OUT == kOutC128) {
            ((double2 *)p.out)[plane * plane_pts + at] = v;
        } else {
            const double mag = sqrt(v.x * v.x + v.y * v.y);
            if (OUT == kOutMagF64) {
                ((double *)p.out)[pic + at * p.channels] = mag;
            } else {
                const double q = floor(mag + 0.5);      // min(255, floor(x + 0.5))
                ((uint8_t *)p.out)[pic + at * p.channels] = (uint8_t)(q < 255.0 ? q : 255.0);
            }
        }
    }
}

// --------------------------------------------------------------------------------
// The notch step.  Block x of the grid is one distinct centre: the terms i = 2 .. sn - 1 of the schedule take 8 i blocks
// each - the diagonal call's four centres, the 2 (i - 1) mixed calls' four each, the two axis calls' two each (an axis
// call names each of its two centres twice).
// --------------------------------------------------------------------------------
constexpr int kNotchThreads = 512;
constexpr int kNotchMaxR = 6;
constexpr int kNotchSpan = 10 * kNotchMaxR + 1;     // rows (and columns) of the largest read disc
constexpr int kNotchMaxPts = 2821;                  // lattice points within 30 of a lattice point
constexpr int kNotchSortPts = 4096;                 // ... rounded up to a power of two: the sort's array, 64 KiB of LDS

// real part, then imaginary part: np.median's (np.sort's) order of complex values
__device__ __forceinline__ bool lex_less(double2 a, double2 b) { return a.x < b.x || (a.x == b.x && a.y < b.y); }

__global__ __launch_bounds__(kNotchThreads) void k_notch(double2 *f, int H, int W, int spacing, int r, int shifted, int transposed) {
    __shared__ double2 s_sort[kNotchSortPts];
    __shared__ int s_at[kNotchMaxPts];
    __shared__ unsigned char s_inner[kNotchMaxPts];
    __shared__ int s_xl[kNotchSpan], s_cnt[kNotchSpan], s_off[kNotchSpan + 1];
    int t = blockIdx.x, i = 2;
    while (t >= 8 * i) {
        t -= 8 * i;
        ++i;
    }
    int a, b, sign, r1 = r, r2 = 5 * r, reps = 1;
    if (t < 4) {
        a = b = i;
        sign = t;
    } else if (t < 4 + 8 * (i - 1)) {
        const int u = t - 4, c = u >> 2, j = (c >> 1) + 1;
        sign = u & 3;
        a = (c & 1) ? i : j;
        b = (c & 1) ? j : i;
    } else {
        const int u = t - 4 - 8 * (i - 1);
        r1 = 3;
        r2 = 3 * r;
        reps = 2;
        a = u < 2 ? 0 : i;
        b = u < 2 ? i : 0;
        sign = u < 2 ? (u & 1) : ((u & 1) << 1);
    }
    // the four centres of a call in the order of their assignments: (+a, +b), (+a, -b), (-a, +b), (-a, -b)
    const int cx = W / 2 + ((sign & 2) ? -a : a) * spacing, cy = H / 2 + ((sign & 1) ? -b : b) * spacing;
    const int span = 2 * r2 + 1;
    if ((int)threadIdx.x < span) {
        const int y = cy - r2 + (int)threadIdx.x, dy = (int)threadIdx.x - r2;
        int xl = 0, cnt = 0;
        if (y >= 0 && y < H) {
            int hw = 0;
            while ((hw + 1) * (hw + 1) + dy * dy <= r2 * r2) ++hw;
            xl = max(0, cx - hw);
            cnt = max(0, min(W - 1, cx + hw) - xl + 1);
        }
        s_xl[threadIdx.x] = xl;
        s_cnt[threadIdx.x] = cnt;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int sum = 0;
        for (int k = 0; k < span; ++k) {
            s_off[k] = sum;
            sum += s_cnt[k];
        }
        s_off[span] = sum;
    }
    __syncthreads();
    const int n = s_off[span];
    if (n == 0) return;     // an empty disc assigns nothing
    double2 *plane = f + (size_t)blockIdx.y * H * W;
    for (int e = threadIdx.x; e < span * span; e += kNotchThreads) {
        const int ry = e / span, x = cx - r2 + e % span;
        if (x < s_xl[ry] || x >= s_xl[ry] + s_cnt[ry]) continue;
        const int y = cy - r2 + ry, slot = s_off[ry] + (x - s_xl[ry]);
        const int gy = shifted ? y : (y + H - H / 2) % H, gx = shifted ? x : (x + W - W / 2) % W;
        s_at[slot] = transposed ? gx * H + gy : gy * W + gx;     // transposed: the plane is stored [W][H]
        s_inner[slot] = (x - cx) * (x - cx) + (y - cy) * (y - cy) <= r1 * r1;
    }
    __syncthreads();
    int padded = 1;
    while (padded < n) padded <<= 1;
    const int lo = (n - 1) / 2, hi = n / 2;
    double2 med = double2{0.0, 0.0};
    for (int rep = 0; rep < reps; ++rep) {
        // the disc as the assignment finds it (the coincident centre's second one reads what the first wrote), padded with
        // +inf, then a bitonic sort: the median is the middle of the sorted values, whichever way equal ones fall
        for (int e = threadIdx.x; e < padded; e += kNotchThreads) {
            double vx = INFINITY, vy = INFINITY;
            if (e < n) {
                const bool again = rep > 0 && s_inner[e];
                const double2 g = plane[s_at[e]];
                vx = again ? med.x : g.x;
                vy = again ? med.y : g.y;
            }
            s_sort[e] = double2{vx, vy};
        }
        __syncthreads();
        for (int k = 2; k <= padded; k <<= 1) {
            for (int j = k >> 1; j > 0; j >>= 1) {
                for (int e = threadIdx.x; e < padded; e += kNotchThreads) {
                    const int o = e ^ j;
                    if (o > e) {
                        const double2 u = s_sort[e], v = s_sort[o];
                        if (lex_less(v, u) == ((e & k) == 0)) {
                            s_sort[e] = v;
                            s_sort[o] = u;
                        }
                    }
                }
                __syncthreads();
            }
        }
        const double2 m0 = s_sort[lo], m1 = s_sort[hi];
        med = lo == hi ? m0 : double2{(m0.x + m1.x) * 0.5, (m0.y + m1.y) * 0.5};
        __syncthreads();    // everyone has read the middle before the next fill
    }
    for (int e = threadIdx.x; e < n; e += kNotchThreads)
        if (s_inner[e]) plane[s_at[e]] = med;
}

// --------------------------------------------------------------------------------
// T1 k_transpose: planes [rows][cols] -> [cols][rows] through 32 x 32 tiles in LDS, so that both the reads and the writes
// cover 512 consecutive bytes.  Columns longer than 1024 points do not fit a strip of four in LDS; their planes are turned,
// transformed as rows (the same arithmetic on the same values) and turned back.
// --------------------------------------------------------------------------------
constexpr int kTile = 32;
__global__ __launch_bounds__(256) void k_transpose(const double2 *__restrict__ in, double2 *__restrict__ out, int rows, int cols) {
    __shared__ double2 tile[kTile][kTile + 1];
    const size_t plane = (size_t)blockIdx.z * rows * cols;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5, r0 = blockIdx.y * kTile, c0 = blockIdx.x * kTile;
    for (int k = ty; k < kTile; k += 8)
        if (r0 + k < rows && c0 + tx < cols) tile[k][tx] = in[plane + (size_t)(r0 + k) * cols + c0 + tx];
    __syncthreads();
    for (int k = ty; k < kTile; k += 8)
        if (c0 + k < cols && r0 + tx < rows) out[plane + (size_t)(c0 + k) * rows + r0 + tx] = tile[tx][k];
}

// ---------------------------------------------------------------- host side
bool five_smooth(int n) {
    for (int p : {2, 3, 5})
        while (n % p == 0) n /= p;
    return n == 1;
}

// The table of a length, computed once and kept: the address stays valid, so an asynchronous upload may read it after the
// call has returned.  A cache; no result depends on it.
const double *twiddle_table(int n) {
    static std::mutex mu;
    static std::map<int, std::vector<double>> tables;
    std::lock_guard<std::mutex> lock(mu);
    std::vector<double> &t = tables[n];
    if (t.empty()) {
        t.resize((size_t)2 * n);
        apap_fft_twiddles(n, t.data());
    }
    return t.data();
}

int rows_per_block(int n) { return std::max(1, std::min(kFftMaxRows, 512 / n)); }
int strip_width(int n, int count) { return std::max(1, std::min(std::min(kFftMaxStrip, count), kFftLdsPoints / n)); }

template <int IN, int OUT, bool COLS>
int launch_pass(const FftPass &p, int planes, hipStream_t s, const char *who) {
    const size_t lds = (size_t)2 * p.per_block * p.n * sizeof(double2);
    void (*kern)(const FftPass) = k_fft_pass<IN, OUT, COLS>;
    if (lds > 65536) {   // the attribute, once per instantiation and device: the largest a block asks for
        static std::atomic<unsigned long long> raised{0};
        int dev = 0;
        hipError_t e = hipGetDevice(&dev);
        if (e != hipSuccess) return apap::hip_fail((int)e, who);
        const unsigned long long bit = 1ull << (dev & 63);
        if (dev >= 64 || !(raised.load() & bit)) {
            e = hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, 2 * kFftLdsPoints * (int)sizeof(double2));
            if (e != hipSuccess) return apap::hip_fail((int)e, who);
            raised.fetch_or(bit);
        }
    }
    hipLaunchKernelGGL(kern, dim3((unsigned)((p.count + p.per_block - 1) / p.per_block), (unsigned)planes), dim3(p.per_block * p.n >= 2048 ? kFftThreadsLong : kFftThreads), lds, s, p);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return apap::hip_fail((int)e, who);
    return APAP_OK;
}

FftPass row_pass(const void *in, void *out, const double *tw_w, int h, int w, int channels, bool inverse) {
    FftPass p{in, out, (const double2 *)tw_w, w, h, rows_per_block(w), channels, inverse ? -1.0 : 1.0, 0, 1.0};
    if (inverse) {
        p.scaled = 1;
        p.scale = 1.0 / ((double)h * (double)w);
    }
    return p;
}
FftPass col_pass(const void *in, void *out, const double *tw_h, int h, int w, bool inverse) {
    return FftPass{in, out, (const double2 *)tw_h, h, w, strip_width(h, w), 1, inverse ? -1.0 : 1.0, 0, 1.0};
}

// Columns of more than 1024 points: a strip of four (64 bytes an access) does not fit the LDS buffers.  Such planes are
// transposed (k_transpose), their columns transformed as rows, and transposed back.
bool tall(int h) { return h > kFftLdsPoints / 4; }
FftPass tall_pass(void *buf, const double *tw_h, int h, int w, bool inverse) {
    return FftPass{buf, buf, (const double2 *)tw_h, h, w, rows_per_block(h), 1, inverse ? -1.0 : 1.0, 0, 1.0};
}
int launch_transpose(const void *in, void *out, int planes, int rows, int cols, hipStream_t s, const char *who) {
    hipLaunchKernelGGL(k_transpose, dim3((unsigned)((cols + kTile - 1) / kTile), (unsigned)((rows + kTile - 1) / kTile), (unsigned)planes), dim3(256), 0,
                       s, (const double2 *)in, (double2 *)out, rows, cols);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return apap::hip_fail((int)e, who);
    return APAP_OK;
}
// The column pass of `planes` planes from d_in to d_out (which may be one), by strips or, for tall planes, through d_turn.
int column_pass(const void *d_in, void *d_out, void *d_turn, const double *tw_h, int planes, int h, int w, bool inverse, hipStream_t s,
                const char *who) {
    if (!tall(h)) return launch_pass<kInC128, kOutC128, true>(col_pass(d_in, d_out, tw_h, h, w, inverse), planes, s, who);
    int rc = launch_transpose(d_in, d_turn, planes, h, w, s, who);
    if (rc) return rc;
    if ((rc = launch_pass<kInC128, kOutC128, false>(tall_pass(d_turn, tw_h, h, w, inverse), planes, s, who))) return rc;
    return launch_transpose(d_turn, d_out, planes, w, h, s, who);
}

struct Twiddles {
    const double *h, *w;
};
size_t twiddle_bytes(int h, int w) { return apap::up256((size_t)h * 16) + apap::up256((size_t)w * 16); }
// Both tables at the head of a workspace.
int upload_twiddles(void *d_work, int h, int w, hipStream_t s, Twiddles *tw, const char *who) {
    double *d_h = (double *)d_work, *d_w = (double *)((char *)d_work + apap::up256((size_t)h * 16));
    hipError_t e = hipMemcpyAsync(d_h, twiddle_table(h), (size_t)h * 16, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(d_w, twiddle_table(w), (size_t)w * 16, hipMemcpyHostToDevice, s);
    if (e != hipSuccess) return apap::hip_fail((int)e, who);
    tw->h = d_h;
    tw->w = d_w;
    return APAP_OK;
}

int launch_notch(double *d_f, int planes, int h, int w, int spacing, int r, int sn, int shifted, int transposed, hipStream_t s,
                 const char *who) {
    // terms whose every centre lies a read disc beyond both sides assign nothing
    const long long reach = ((long long)std::max(h, w) + 5 * r) / spacing + 2;
    const long long terms = std::min<long long>(sn, reach);
    const long long blocks = 4 * terms * (terms - 1) - 8;    // sum of 8 i over i = 2 .. terms - 1
    if (blocks <= 0) return APAP_OK;
    hipLaunchKernelGGL(k_notch, dim3((unsigned)blocks, (unsigned)planes), dim3(kNotchThreads), 0, s, (double2 *)d_f, h, w, spacing, r,
                       shifted, transposed);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return apap::hip_fail((int)e, who);
    return APAP_OK;
}

size_t spectrum_bytes(int planes, int h, int w) { return apap::up256((size_t)planes * h * w * 16); }
// the second copy that tall planes are turned into
size_t turn_bytes(int planes, int h, int w) { return tall(h) ? spectrum_bytes(planes, h, w) : 0; }

}  // namespace

namespace apap {

int fft_check(int planes, int h, int w, const char *who) {
    if (planes < 1 || planes > kDenoiseMaxPlanes) return fail(APAP_ERR_INVALID_ARG, "%s: %d planes (1 .. %d)", who, planes, kDenoiseMaxPlanes);
    for (int n : {h, w}) {
        if (n < APAP_FFT_MIN_LENGTH || n > APAP_FFT_MAX_LENGTH)
            return fail(APAP_ERR_INVALID_ARG, "%s: length %d of a %d x %d plane (lengths %d .. %d)", who, n, h, w, APAP_FFT_MIN_LENGTH,
                        APAP_FFT_MAX_LENGTH);
        if (!five_smooth(n))
            return fail(APAP_ERR_INVALID_ARG, "%s: length %d of a %d x %d plane is not 5-smooth (only the factors 2, 3 and 5)", who, n, h, w);
    }
    return APAP_OK;
}

int notch_check(int spacing, int r, int sn, const char *who) {
    if (r < 1 || r > APAP_NOTCH_MAX_R) return fail(APAP_ERR_INVALID_ARG, "%s: r=%d (1 .. %d)", who, r, APAP_NOTCH_MAX_R);
    if (sn < 2) return fail(APAP_ERR_INVALID_ARG, "%s: sn=%d (at least 2)", who, sn);
    const int bound = std::max(6 * r, 5 * r + 3);
    if (spacing <= bound)
        return fail(APAP_ERR_INVALID_ARG, "%s: spacing=%d must exceed max(6 r, 5 r + 3) = %d, or a write disc meets another centre's read disc",
                    who, spacing, bound);
    return APAP_OK;
}

int denoise_check(int n_images, int h, int w, int channels, int spacing, int r, int sn, int out_type, const char *who) {
    if (n_images < 1 || channels < 1 || channels > 4)
        return fail(APAP_ERR_INVALID_ARG, "%s: %d pictures of %d channels (at least 1 picture, 1 .. 4 channels)", who, n_images, channels);
    if (n_images > kDenoiseMaxPlanes / channels)
        return fail(APAP_ERR_INVALID_ARG, "%s: %d pictures of %d channels (%d planes at most)", who, n_images, channels, kDenoiseMaxPlanes);
    int rc = fft_check(n_images * channels, h, w, who);
    if (rc) return rc;
    if ((rc = notch_check(spacing, r, sn, who))) return rc;
    if (out_type != APAP_DENOISE_OUT_F64 && out_type != APAP_DENOISE_OUT_U8)
        return fail(APAP_ERR_INVALID_ARG, "%s: output type %d (APAP_DENOISE_OUT_F64 or APAP_DENOISE_OUT_U8)", who, out_type);
    return APAP_OK;
}

}  // namespace apap

extern "C" {

int apap_fft_twiddles(int n, double *out) {
    if (n < 1 || !out) return apap::fail(APAP_ERR_INVALID_ARG, "apap_fft_twiddles: n=%d or a null table", n);
    const long double step = -2.0L * 3.141592653589793238462643383279502884L / (long double)n;
    for (int k = 0; k < n; ++k) {
        out[2 * k] = (double)cosl(step * (long double)k);
        out[2 * k + 1] = (double)sinl(step * (long double)k);
    }
    out[0] = 1.0;
    out[1] = 0.0;
    return APAP_OK;
}

size_t apap_fft2_workspace_bytes(int planes, int h, int w) {
    if (apap::fft_check(planes, h, w, "apap_fft2_workspace_bytes")) return 0;
    return twiddle_bytes(h, w) + turn_bytes(planes, h, w);
}

int apap_fft2_device(apap_ctx *ctx, const double *d_in, double *d_out, int planes, int h, int w, int inverse, void *d_work,
                     size_t work_bytes, void *stream) {
    const char *who = "apap_fft2_device";
    (void)ctx;
    int rc = apap::fft_check(planes, h, w, who);
    if (rc) return rc;
    if (!d_in || !d_out || !d_work) return apap::fail(APAP_ERR_INVALID_ARG, "%s: null device pointer", who);
    const size_t need = apap_fft2_workspace_bytes(planes, h, w);
    if (work_bytes < need) return apap::fail(APAP_ERR_WORKSPACE, "%s: workspace %zu < %zu bytes", who, work_bytes, need);
    if (((uintptr_t)d_work & 255) != 0) return apap::fail(APAP_ERR_INVALID_ARG, "%s: workspace not 256-byte aligned", who);
    void *d_turn = (char *)d_work + twiddle_bytes(h, w);
    hipStream_t s = (hipStream_t)stream;
    Twiddles tw;
    if ((rc = upload_twiddles(d_work, h, w, s, &tw, who))) return rc;
    if (!inverse) {
        if ((rc = launch_pass<kInC128, kOutC128, false>(row_pass(d_in, d_out, tw.w, h, w, 1, false), planes, s, who))) return rc;
        return column_pass(d_out, d_out, d_turn, tw.h, planes, h, w, false, s, who);
    }
    if ((rc = column_pass(d_in, d_out, d_turn, tw.h, planes, h, w, true, s, who))) return rc;
    return launch_pass<kInC128, kOutC128, false>(row_pass(d_out, d_out, tw.w, h, w, 1, true), planes, s, who);
}

int apap_notch_spectrum_device(apap_ctx *ctx, double *d_f, int planes, int h, int w, int spacing, int r, int sn, void *stream) {
    const char *who = "apap_notch_spectrum_device";
    (void)ctx;
    // the notch itself takes any plane of at least 1 x 1; the transform's lengths are not its concern
    if (planes < 1 || planes > apap::kDenoiseMaxPlanes || h < 1 || w < 1 || h > APAP_FFT_MAX_LENGTH || w > APAP_FFT_MAX_LENGTH)
        return apap::fail(APAP_ERR_INVALID_ARG, "%s: %d planes of %d x %d (1 .. %d planes, sides 1 .. %d)", who, planes, h, w,
                          apap::kDenoiseMaxPlanes, APAP_FFT_MAX_LENGTH);
    const int rc = apap::notch_check(spacing, r, sn, who);
    if (rc) return rc;
    if (!d_f) return apap::fail(APAP_ERR_INVALID_ARG, "%s: null device pointer", who);
    return launch_notch(d_f, planes, h, w, spacing, r, sn, 1, 0, (hipStream_t)stream, who);
}

size_t apap_notch_denoise_workspace_bytes(int n_images, int h, int w, int channels) {
    if (n_images < 1 || channels < 1 || channels > 4 || n_images > apap::kDenoiseMaxPlanes / channels) return 0;
    if (apap::fft_check(n_images * channels, h, w, "apap_notch_denoise_workspace_bytes")) return 0;
    return twiddle_bytes(h, w) + spectrum_bytes(n_images * channels, h, w) + turn_bytes(n_images * channels, h, w) + apap::up256((size_t)n_images * h * w * channels) +
           apap::up256(apap_equalize_workspace_bytes(channels));
}

int apap_notch_denoise_device(apap_ctx *ctx, const uint8_t *d_imgs, int n_images, int h, int w, int channels, int equalize, int spacing,
                              int r, int sn, int out_type, void *d_out, void *d_work, size_t work_bytes, void *stream) {
    const char *who = "apap_notch_denoise_device";
    int rc = apap::denoise_check(n_images, h, w, channels, spacing, r, sn, out_type, who);
    if (rc) return rc;
    if (!d_imgs || !d_out || !d_work) return apap::fail(APAP_ERR_INVALID_ARG, "%s: null device pointer", who);
    const size_t need = apap_notch_denoise_workspace_bytes(n_images, h, w, channels);
    if (work_bytes < need) return apap::fail(APAP_ERR_WORKSPACE, "%s: workspace %zu < %zu bytes", who, work_bytes, need);
    if (((uintptr_t)d_work & 255) != 0) return apap::fail(APAP_ERR_INVALID_ARG, "%s: workspace not 256-byte aligned", who);
    hipStream_t s = (hipStream_t)stream;
    const int planes = n_images * channels;
    const size_t pic_bytes = (size_t)h * w * channels;
    char *at = (char *)d_work + twiddle_bytes(h, w);
    double *d_spec = (double *)at;
    at += spectrum_bytes(planes, h, w);
    double *d_turn = (double *)at;
    at += turn_bytes(planes, h, w);
    uint8_t *d_eq = (uint8_t *)at;
    at += apap::up256(pic_bytes * n_images);
    void *d_eq_work = at;
    Twiddles tw;
    if ((rc = upload_twiddles(d_work, h, w, s, &tw, who))) return rc;
    const uint8_t *d_planes = d_imgs;
    if (equalize) {
        // the equalisation wants its counters zero on entry and leaves them so; this workspace promises nothing between calls
        const size_t eq_bytes = apap_equalize_workspace_bytes(channels);
        const hipError_t e = hipMemsetAsync(d_eq_work, 0, eq_bytes, s);
        if (e != hipSuccess) return apap::hip_fail((int)e, who);
        for (int m = 0; m < n_images; ++m)   // its tables are one picture's: a picture a time
            if ((rc = apap_equalize_hist_device(ctx, d_imgs + m * pic_bytes, h, w, channels, d_eq + m * pic_bytes, d_eq_work, eq_bytes, stream)))
                return rc;
        d_planes = d_eq;
    }
    if ((rc = launch_pass<kInU8, kOutC128, false>(row_pass(d_planes, d_spec, tw.w, h, w, channels, false), planes, s, who))) return rc;
    if (!tall(h)) {
        if ((rc = launch_pass<kInC128, kOutC128, true>(col_pass(d_spec, d_spec, tw.h, h, w, false), planes, s, who))) return rc;
        if ((rc = launch_notch(d_spec, planes, h, w, spacing, r, sn, 0, 0, s, who))) return rc;
        if ((rc = launch_pass<kInC128, kOutC128, true>(col_pass(d_spec, d_spec, tw.h, h, w, true), planes, s, who))) return rc;
    } else {   // turned once: both column transforms and the notch between them work on the [w][h] copy
        if ((rc = launch_transpose(d_spec, d_turn, planes, h, w, s, who))) return rc;
        if ((rc = launch_pass<kInC128, kOutC128, false>(tall_pass(d_turn, tw.h, h, w, false), planes, s, who))) return rc;
        if ((rc = launch_notch(d_turn, planes, h, w, spacing, r, sn, 0, 1, s, who))) return rc;
        if ((rc = launch_pass<kInC128, kOutC128, false>(tall_pass(d_turn, tw.h, h, w, true), planes, s, who))) return rc;
        if ((rc = launch_transpose(d_turn, d_spec, planes, w, h, s, who))) return rc;
    }
    const FftPass last = row_pass(d_spec, d_out, tw.w, h, w, channels, true);
    if (out_type == APAP_DENOISE_OUT_U8) return launch_pass<kInC128, kOutMagU8, false>(last, planes, s, who);
    return launch_pass<kInC128, kOutMagF64, false>(last, planes, s, who);
}

}  // extern "C"
