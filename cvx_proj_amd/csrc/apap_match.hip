// Exact descriptor matching: for every query row of q (nq x 128 float32) the nearest and the second-nearest row of
// t (nt x 128 float32) under the L2 distance - what cv.DescriptorMatcher.match / knnMatch(k = 2) approximate.
//
//     d2(i, j) = sum_k (q[i, k] - t[j, k])^2          float32, difference form: one subtraction, one fmaf per (i, j, k),
//                                                     k ascending.  Never |q|^2 + |t|^2 - 2 q.t, which cancels.
//
// For integer-valued descriptors in 0 .. 255 (OpenCV's SIFT) every term is <= 65 025 and every sum <= 8 323 200 < 2^24:
// d2 is exact.
//
// Candidates are ordered by (d2, train index), lexicographically; a NaN or infinite d2 is never a candidate.  That order
// is total, so the minimum and the runner-up do not depend on how the train rows are cut into chunks, splits or blocks, and
// d2(i, j) is always computed by the same instruction sequence: the outputs depend on (q, t) alone, not on the launch
// geometry or on what else is in a batch.  No floating-point atomics.
//
// k_match_sweep: one block of 256 threads takes kMatchQ = 64 queries (all 128 dimensions in LDS, dimension-major, staged
// once) and a run of train chunks of kMatchT = 128 rows, each staged in 4 slices of kMatchK = 32 dimensions (dimension-major;
// the next slice's global loads are in flight while this one is consumed).  A thread owns a 4 x 8 register tile of d2: per
// dimension 3 ds_read_b128 feed 64 VALU operations.  After a chunk every thread folds its 32 sums into its running
// (best, second) of its 4 queries; after the last chunk the 16 threads of a query merge through LDS, and the block writes one
// partial per query.  The train axis is split over blockIdx so that a small nq still fills the chip.
// k_match_merge: one thread per query merges the partials of its splits in ascending order and writes idx, dist (the
// correctly rounded square root of d2), idx2, dist2.
//
// A batch is the same two launches with the pair in blockIdx.y: the table of pair descriptors is in device memory, and
// blocks beyond a pair's own count return at once.  The single call is the batch of one.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#include "apap_internal.h"

namespace {

constexpr int kDim = APAP_MATCH_DIM;
constexpr int kMatchQ = APAP_MATCH_QUERY_TILE;    // queries per block
constexpr int kMatchT = APAP_MATCH_TRAIN_CHUNK;   // train rows per chunk
constexpr int kMatchK = 32;                       // dimensions per staged slice
constexpr int kThreads = 256;
constexpr int kQS = kMatchQ + 4, kTS = kMatchT + 4;   // LDS row strides in floats: 16-byte multiples, off the bank period
constexpr int kMaxPairs = 65535;                  // grid.y
constexpr int kMaxRows = 1 << 24;
static_assert(kDim == 128 && kMatchQ == 64 && kMatchT == 128 && kDim % kMatchK == 0, "the thread mapping below is for these");

struct MatchPart {   // a query's running result over some train rows: (d2, index) of the best and of the runner-up
    float d1;
    int i1;
    float d2;
    int i2;
};

struct alignas(16) MatchPair {   // one pair, in device memory
    int q0, t0, nq, nt;          // first query / train row in the concatenated arrays, counts
    int q_tiles, splits, cps;    // blocks along the queries, splits of the train axis, chunks per split
    int pad;
    long long part0;             // first partial of the pair: partial of (split s, query i) at part0 + s nq + i
    long long pad2;
};
static_assert(sizeof(MatchPair) == 48, "MatchPair");

// (da, ia) before (db, ib) in the order of the candidates.  An empty slot is (+inf, -1): no candidate is infinite, so every
// candidate comes before it.
__device__ __forceinline__ bool before(float da, int ia, float db, int ib) { return da < db || (da == db && ia < ib); }

__device__ __forceinline__ MatchPart merge(MatchPart a, MatchPart b) {
    if (before(b.d1, b.i1, a.d1, a.i1)) {
        const MatchPart s = a;
        a = b;
        b = s;
    }
    if (before(b.d1, b.i1, a.d2, a.i2)) {
        a.d2 = b.d1;
        a.i2 = b.i1;
    }
    return a;
}

__global__ __launch_bounds__(kThreads) void k_match_sweep(const float *__restrict__ q, const float *__restrict__ t,
                                                          const MatchPair *__restrict__ tab, MatchPart *__restrict__ parts) {
    const MatchPair P = tab[blockIdx.y];
    if (blockIdx.x >= (unsigned)(P.q_tiles * P.splits)) return;
    const int qt = blockIdx.x % P.q_tiles, sp = blockIdx.x / P.q_tiles;
    const int n_chunks = (P.nt + kMatchT - 1) / kMatchT;
    const int c_begin = sp * P.cps, c_end = min(n_chunks, c_begin + P.cps);

    __shared__ __attribute__((aligned(16))) float qs[kDim * kQS];      // qs[k][query]
    __shared__ __attribute__((aligned(16))) float ts[kMatchK * kTS];   // ts[k - slice][train row of the chunk]
    static_assert(sizeof(MatchPart) * kMatchQ * 16 <= sizeof(float) * kMatchK * kTS, "the final merge reuses ts");

    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const float *qp = q + (size_t)P.q0 * kDim, *tp = t + (size_t)P.t0 * kDim;

    // the block's queries, all dimensions: 64 rows x 32 float4
#pragma unroll
    for (int it = 0; it < kMatchQ * (kDim / 4) / kThreads; ++it) {
        const int at = tid + kThreads * it, row = at >> 5, c = at & 31, i = qt * kMatchQ + row;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (i < P.nq) v = *(const float4 *)(qp + (size_t)i * kDim + 4 * c);
        qs[(4 * c + 0) * kQS + row] = v.x;
        qs[(4 * c + 1) * kQS + row] = v.y;
        qs[(4 * c + 2) * kQS + row] = v.z;
        qs[(4 * c + 3) * kQS + row] = v.w;
    }

    // a slice of a chunk: 128 rows x 8 float4, 4 per thread (8 consecutive lanes read one row's 128 bytes)
    float4 pre[4];
    const int lr = tid >> 3, lc = tid & 7;
    auto load_slice = [&](int chunk, int s) {
#pragma unroll
        for (int it = 0; it < 4; ++it) {
            const int j = chunk * kMatchT + lr + 32 * it;
            pre[it] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (j < P.nt) pre[it] = *(const float4 *)(tp + (size_t)j * kDim + s * kMatchK + 4 * lc);
        }
    };
    auto store_slice = [&]() {
#pragma unroll
        for (int it = 0; it < 4; ++it) {
            const int r = lr + 32 * it;
            ts[(4 * lc + 0) * kTS + r] = pre[it].x;
            ts[(4 * lc + 1) * kTS + r] = pre[it].y;
            ts[(4 * lc + 2) * kTS + r] = pre[it].z;
            ts[(4 * lc + 3) * kTS + r] = pre[it].w;
        }
    };

    MatchPart best[4];
#pragma unroll
    for (int a = 0; a < 4; ++a) best[a] = MatchPart{INFINITY, -1, INFINITY, -1};

    load_slice(c_begin, 0);
    for (int chunk = c_begin; chunk < c_end; ++chunk) {
        float acc[4][8];
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 8; ++b) acc[a][b] = 0.f;
        for (int s = 0; s < kDim / kMatchK; ++s) {
            __syncthreads();   // the previous slice has been consumed
            store_slice();
            __syncthreads();   // (the first of these also publishes qs)
            if (s + 1 < kDim / kMatchK)
                load_slice(chunk, s + 1);
            else if (chunk + 1 < c_end)
                load_slice(chunk + 1, 0);
            const float *qk = qs + s * kMatchK * kQS + 4 * ty, *tk = ts + 4 * tx;
#pragma unroll 8
            for (int k = 0; k < kMatchK; ++k) {
                const float4 qv = *(const float4 *)(qk + k * kQS);
                const float4 ta = *(const float4 *)(tk + k * kTS), tb = *(const float4 *)(tk + k * kTS + kMatchT / 2);
                const float qa[4] = {qv.x, qv.y, qv.z, qv.w};
                const float tv[8] = {ta.x, ta.y, ta.z, ta.w, tb.x, tb.y, tb.z, tb.w};
#pragma unroll
                for (int a = 0; a < 4; ++a)
#pragma unroll
                    for (int b = 0; b < 8; ++b) {
                        const float d = qa[a] - tv[b];
                        acc[a][b] = fmaf(d, d, acc[a][b]);
                    }
            }
        }
        // fold the chunk in: this thread's train rows come in ascending order, here and from chunk to chunk, so the strict
        // comparisons keep the lowest index among equal distances
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const int j = chunk * kMatchT + (b < 4 ? 4 * tx + b : kMatchT / 2 + 4 * tx + b - 4);
#pragma unroll
            for (int a = 0; a < 4; ++a) {
                const float d = j < P.nt ? acc[a][b] : INFINITY;
                if (d < best[a].d1) {
                    best[a].d2 = best[a].d1;
                    best[a].i2 = best[a].i1;
                    best[a].d1 = d;
                    best[a].i1 = j;
                } else if (d < best[a].d2) {
                    best[a].d2 = d;
                    best[a].i2 = j;
                }
            }
        }
    }

    // the 16 threads of a query, merged in the order of tx
    __syncthreads();
    MatchPart *red = (MatchPart *)ts;
#pragma unroll
    for (int a = 0; a < 4; ++a) red[(4 * ty + a) * 16 + tx] = best[a];
    __syncthreads();
    if (tid < kMatchQ) {
        const int i = qt * kMatchQ + tid;
        MatchPart m = red[tid * 16];
        for (int x = 1; x < 16; ++x) m = merge(m, red[tid * 16 + x]);
        if (i < P.nq) parts[P.part0 + (long long)sp * P.nq + i] = m;
    }
}

__global__ __launch_bounds__(kThreads) void k_match_merge(const MatchPair *__restrict__ tab, const MatchPart *__restrict__ parts,
                                                          int *__restrict__ idx, float *__restrict__ dist, int *__restrict__ idx2,
                                                          float *__restrict__ dist2) {
    const MatchPair P = tab[blockIdx.y];
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= P.nq) return;
    MatchPart m = parts[P.part0 + i];
    for (int s = 1; s < P.splits; ++s) m = merge(m, parts[P.part0 + (long long)s * P.nq + i]);
    // float32(sqrt in float64) is the correctly rounded float32 square root: 53 >= 2 * 24 + 2 bits
    const size_t o = (size_t)P.q0 + i;
    idx[o] = m.i1;
    dist[o] = m.i1 >= 0 ? (float)sqrt((double)m.d1) : INFINITY;
    if (idx2) idx2[o] = m.i2;
    if (dist2) dist2[o] = m.i2 >= 0 ? (float)sqrt((double)m.d2) : INFINITY;
}

// How a pair of (nq, nt) rows is cut: a function of the pair alone.
struct MatchPlan {
    int q_tiles, splits, cps;
    size_t part_bytes;   // a 256-byte multiple
};

MatchPlan plan_match(int nq, int nt) {
    MatchPlan p;
    p.q_tiles = (nq + kMatchQ - 1) / kMatchQ;
    const int n_chunks = (nt + kMatchT - 1) / kMatchT;
    // enough blocks for several rounds over the chip's 256 CUs x 3 resident blocks, so that the last round's idle share is small
    const int want = std::min(n_chunks, (APAP_MATCH_WANT_BLOCKS + p.q_tiles - 1) / p.q_tiles);
    p.cps = (n_chunks + want - 1) / want;
    p.splits = (n_chunks + p.cps - 1) / p.cps;
    p.part_bytes = apap::up256((size_t)p.splits * nq * sizeof(MatchPart));
    return p;
}

size_t table_bytes(int n_pairs) { return apap::up256((size_t)n_pairs * sizeof(MatchPair)); }

}  // namespace

namespace apap {

// The argument checks of the matching entry points that need no device pointer.
int match_check(const int *q_offset, const int *t_offset, int n_pairs, const char *who) {
    if (!q_offset || !t_offset) return apap::fail(APAP_ERR_INVALID_ARG, "%s: null q_offset / t_offset", who);
    if (n_pairs < 1 || n_pairs > kMaxPairs)
        return apap::fail(APAP_ERR_INVALID_ARG, "%s: n_pairs = %d (1 .. %d)", who, n_pairs, kMaxPairs);
    if (q_offset[0] < 0 || t_offset[0] < 0)
        return apap::fail(APAP_ERR_INVALID_ARG, "%s: q_offset[0] = %d, t_offset[0] = %d: negative", who, q_offset[0], t_offset[0]);
    for (int p = 0; p < n_pairs; ++p) {
        const long long nq = (long long)q_offset[p + 1] - q_offset[p], nt = (long long)t_offset[p + 1] - t_offset[p];
        if (nq < 1 || nq > kMaxRows || nt < 1 || nt > kMaxRows)
            return apap::fail(APAP_ERR_INVALID_ARG, "%s: pair %d: %lld queries, %lld train rows (offsets must increase strictly, a "
                                                    "pair holds 1 .. 2^24 rows of each)", who, p, nq, nt);
    }
    return APAP_OK;
}

}  // namespace apap

extern "C" {

size_t apap_match_batch_workspace_bytes(const int *q_offset, const int *t_offset, int n_pairs) {
    if (apap::match_check(q_offset, t_offset, n_pairs, "apap_match_batch_workspace_bytes")) return 0;
    size_t total = table_bytes(n_pairs);
    for (int p = 0; p < n_pairs; ++p) total += plan_match(q_offset[p + 1] - q_offset[p], t_offset[p + 1] - t_offset[p]).part_bytes;
    return total;
}

size_t apap_match_workspace_bytes(int nq, int nt) {
    const int qo[2] = {0, nq}, to[2] = {0, nt};
    return apap_match_batch_workspace_bytes(qo, to, 1);
}

int apap_match_descriptors_batch_device(apap_ctx *ctx, const float *d_q, const float *d_t, const int *q_offset, const int *t_offset,
                                        int n_pairs, int *d_idx, float *d_dist, int *d_idx2, float *d_dist2, void *d_work,
                                        size_t work_bytes, void *stream) {
    const char *who = "apap_match_descriptors_batch_device";
    (void)ctx;
    int rc = apap::match_check(q_offset, t_offset, n_pairs, who);
    if (rc) return rc;
    if (!d_q || !d_t || !d_idx || !d_dist || !d_work) return apap::fail(APAP_ERR_INVALID_ARG, "%s: null device pointer", who);
    const size_t need = apap_match_batch_workspace_bytes(q_offset, t_offset, n_pairs);
    if (work_bytes < need) return apap::fail(APAP_ERR_WORKSPACE, "%s: workspace %zu < %zu bytes", who, work_bytes, need);
    if (((uintptr_t)d_work & 255) != 0 || ((uintptr_t)d_q & 15) != 0 || ((uintptr_t)d_t & 15) != 0)
        return apap::fail(APAP_ERR_INVALID_ARG, "%s: workspace must be 256-byte and descriptors 16-byte aligned", who);

    std::vector<MatchPair> tab((size_t)n_pairs);
    size_t off = table_bytes(n_pairs);
    int max_blocks = 0, max_nq = 0;
    for (int p = 0; p < n_pairs; ++p) {
        MatchPair &d = tab[p];
        d.q0 = q_offset[p];
        d.t0 = t_offset[p];
        d.nq = q_offset[p + 1] - q_offset[p];
        d.nt = t_offset[p + 1] - t_offset[p];
        const MatchPlan plan = plan_match(d.nq, d.nt);
        d.q_tiles = plan.q_tiles;
        d.splits = plan.splits;
        d.cps = plan.cps;
        d.pad = 0;
        d.part0 = (long long)((off - table_bytes(n_pairs)) / sizeof(MatchPart));
        d.pad2 = 0;
        off += plan.part_bytes;
        max_blocks = std::max(max_blocks, plan.q_tiles * plan.splits);
        max_nq = std::max(max_nq, d.nq);
    }
    hipStream_t s = (hipStream_t)stream;
    MatchPair *d_tab = (MatchPair *)d_work;
    MatchPart *d_parts = (MatchPart *)((char *)d_work + table_bytes(n_pairs));
    // from pageable memory in stream order: the copy returns once its source has been consumed
    hipError_t e = hipMemcpyAsync(d_tab, tab.data(), (size_t)n_pairs * sizeof(MatchPair), hipMemcpyHostToDevice, s);
    if (e != hipSuccess) return apap::hip_fail(e, "apap_match_descriptors_batch_device: descriptor upload");
    hipLaunchKernelGGL(k_match_sweep, dim3(max_blocks, n_pairs), dim3(kThreads), 0, s, d_q, d_t, d_tab, d_parts);
    hipLaunchKernelGGL(k_match_merge, dim3((max_nq + kThreads - 1) / kThreads, n_pairs), dim3(kThreads), 0, s, d_tab, d_parts, d_idx,
                       d_dist, d_idx2, d_dist2);
    e = hipGetLastError();
    if (e != hipSuccess) return apap::hip_fail(e, "apap_match_descriptors_batch_device launch");
    return APAP_OK;
}

int apap_match_descriptors_device(apap_ctx *ctx, const float *d_q, int nq, const float *d_t, int nt, int *d_idx, float *d_dist,
                                  int *d_idx2, float *d_dist2, void *d_work, size_t work_bytes, void *stream) {
    const int qo[2] = {0, nq}, to[2] = {0, nt};
    return apap_match_descriptors_batch_device(ctx, d_q, d_t, qo, to, 1, d_idx, d_dist, d_idx2, d_dist2, d_work, work_bytes, stream);
}

}  // extern "C"
