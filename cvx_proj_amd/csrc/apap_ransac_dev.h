// The steps that the two RANSAC front ends share on the device: the seed homography (apap_frontend.hip, R1-R3; specification
// oracle/frontend_oracle.py) and the fundamental matrix (apap_fundamental.hip, F2-F4; specification
// tests/fundamental_spec.py).  The one definition of the counter-based sampler, of the consensus count and of the selection
// of the winner; what differs between the two - the minimal solver, the inlier predicate, where a pair's matches start -
// stays with each source.  Both specifications restate these steps in numpy, independently of each other.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace apap {

__device__ __forceinline__ unsigned long long splitmix64(unsigned long long x) {
    unsigned long long z = x + 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// K distinct indices below n (n >= K) for hypothesis h, in the order drawn: draw j is the high 32 bits of
// splitmix64(seed + K h + j) (the counter wraps at 2^64) modulo n - j, then stepped over the earlier picks in ascending order.
// `sorted` holds the earlier picks in ascending order (compare-exchange insertion: every index is a constant, so both arrays
// stay in registers).
template <int K>
__device__ __forceinline__ void draw_distinct(unsigned long long seed, int h, int n, int (&picks)[K]) {
    int sorted[K];
#pragma unroll
    for (int j = 0; j < K; ++j) {
        const unsigned int r =
            (unsigned int)(splitmix64(seed + (unsigned long long)K * (unsigned long long)h + (unsigned long long)j) >> 32);
        int p = (int)(r % (unsigned int)(n - j));
#pragma unroll
        for (int k = 0; k < j; ++k) p += (p >= sorted[k]) ? 1 : 0;
        picks[j] = p;
        int v = p;
#pragma unroll
        for (int k = 0; k < j; ++k) {
            const int lo = min(sorted[k], v), hi = max(sorted[k], v);
            sorted[k] = lo;
            v = hi;
        }
        sorted[j] = v;
    }
}

// The block of the consensus kernels (score and select): four waves.
constexpr int kConsensusThreads = 256;
constexpr int kConsensusWaves = kConsensusThreads / 64;

// The matches a block works on: rows first .. first + count - 1 of the point arrays and of the mask.
struct MatchRange {
    int first, count;
};

// The score kernel's body: how many of the matches satisfy `inlier` under the model m[0..8], stored by thread 0.  `inlier`
// is a callable (const double (&m)[9], x, y, u, v, thr2) -> bool.  Each lane counts its matches in ascending order, then
// c[l] += c[l + d] for d = 32 .. 1 in each wave, then the four waves in ascending order.
template <class Inlier>
__device__ __forceinline__ void consensus_score(const float *__restrict__ src, const float *__restrict__ dst, MatchRange r,
                                                const double *__restrict__ model, double thr2, Inlier inlier,
                                                int *__restrict__ count) {
    __shared__ int s_part[kConsensusWaves];
    double m[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) m[i] = model[i];
    const float2 *s2 = reinterpret_cast<const float2 *>(src) + r.first, *d2 = reinterpret_cast<const float2 *>(dst) + r.first;
    int c = 0;
    for (int k = threadIdx.x; k < r.count; k += kConsensusThreads) {
        const float2 s = s2[k], d = d2[k];
        c += inlier(m, (double)s.x, (double)s.y, (double)d.x, (double)d.y, thr2) ? 1 : 0;
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) c += __shfl_down(c, d);
    if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        int total = s_part[0];
#pragma unroll
        for (int w = 1; w < kConsensusWaves; ++w) total += s_part[w];
        *count = total;
    }
}

// The select kernel's body, one block: the first of the `iterations` hypotheses with the most inliers (the strictly greater
// scan keeps a thread's first, the reduction breaks ties to the lower index), its nine doubles to `winner`, {index, count} to
// `result`, and the mask of the range's matches by the same predicate.  `hyps`, `counts`, `winner` and `result` are the
// caller's pair's; `mask` is indexed like the point arrays.
template <class Inlier>
__device__ __forceinline__ void consensus_select(const float *__restrict__ src, const float *__restrict__ dst, MatchRange r,
                                                 const double *__restrict__ hyps, const int *__restrict__ counts,
                                                 int iterations, double thr2, Inlier inlier, double *__restrict__ winner,
                                                 uint8_t *__restrict__ mask, int *__restrict__ result) {
    __shared__ int s_cnt[kConsensusThreads], s_idx[kConsensusThreads];
    int bc = -1, bi = 0x7fffffff;
    for (int i = threadIdx.x; i < iterations; i += kConsensusThreads) {      // ascending: strictly greater keeps the first
        const int c = counts[i];
        if (c > bc) { bc = c; bi = i; }
    }
    s_cnt[threadIdx.x] = bc;
    s_idx[threadIdx.x] = bi;
    __syncthreads();
    for (int d = kConsensusThreads / 2; d > 0; d >>= 1) {
        if (threadIdx.x < d) {
            const int oc = s_cnt[threadIdx.x + d], oi = s_idx[threadIdx.x + d];
            if (oc > s_cnt[threadIdx.x] || (oc == s_cnt[threadIdx.x] && oi < s_idx[threadIdx.x])) {
                s_cnt[threadIdx.x] = oc;
                s_idx[threadIdx.x] = oi;
            }
        }
        __syncthreads();
    }
    const int best = s_idx[0];
    double m[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) m[i] = hyps[(size_t)best * 9 + i];
    if (threadIdx.x < 9) winner[threadIdx.x] = m[threadIdx.x];
    if (threadIdx.x == 0) {
        result[0] = best;
        result[1] = s_cnt[0];
    }
    const float2 *s2 = reinterpret_cast<const float2 *>(src) + r.first, *d2 = reinterpret_cast<const float2 *>(dst) + r.first;
    for (int k = threadIdx.x; k < r.count; k += kConsensusThreads) {
        const float2 s = s2[k], d = d2[k];
        mask[(size_t)r.first + k] = inlier(m, (double)s.x, (double)s.y, (double)d.x, (double)d.y, thr2) ? 1 : 0;
    }
}

}  // namespace apap
