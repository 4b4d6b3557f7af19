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
#include "apap_match_dev.h"

namespace {

using namespace apap;

constexpr int kDim = APAP_MATCH_DIM;
constexpr int kMatchQ = APAP_MATCH_QUERY_TILE;    // queries per block
constexpr int kMatchT = APAP_MATCH_TRAIN_CHUNK;   // train rows per chunk
constexpr int kMatchK = 32;                       // dimensions per staged slice
constexpr int kThreads = 256;
constexpr int kQS = kMatchQ + 4, kTS = kMatchT + 4;   // LDS row strides in floats: 16-byte multiples, off the bank period
static_assert(kDim == 128 && kMatchQ == 64 && kMatchT == 128 && kDim % kMatchK == 0, "the thread mapping below is for these");
// every pair's partials start on a 256-byte boundary: 16 partials
constexpr MatchTiling kTiling{kMatchQ, kMatchT, APAP_MATCH_WANT_BLOCKS, 256 / sizeof(Top2)};

__global__ __launch_bounds__(kThreads) void k_match_sweep(const float *__restrict__ q, const float *__restrict__ t,
                                                          const MatchPair *__restrict__ tab, Top2 *__restrict__ parts) {
    const MatchPair P = tab[blockIdx.y];
    if (blockIdx.x >= (unsigned)(P.q_tiles * P.splits)) return;
    const PairRun<kMatchT> run(P, blockIdx.x);
    const int qt = run.qt, c_begin = run.c_begin, c_end = run.c_end;

    __shared__ __attribute__((aligned(16))) float qs[kDim * kQS];      // qs[k][query]
    __shared__ __attribute__((aligned(16))) float ts[kMatchK * kTS];   // ts[k - slice][train row of the chunk]
    static_assert(sizeof(Top2) * kMatchQ * 16 <= sizeof(float) * kMatchK * kTS, "the final merge reuses ts");

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

    Top2 best[4];
#pragma unroll
    for (int a = 0; a < 4; ++a) best[a] = empty_top2();

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
                    for (int b = 0; b < 8; ++b) acc[a][b] = d2_step(acc[a][b], qa[a], tv[b]);
            }
        }
        // fold the chunk in: this thread's train rows come in ascending order, here and from chunk to chunk
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const int j = chunk * kMatchT + (b < 4 ? 4 * tx + b : kMatchT / 2 + 4 * tx + b - 4);
#pragma unroll
            for (int a = 0; a < 4; ++a) take_ascending(best[a], j < P.nt ? acc[a][b] : INFINITY, j);
        }
    }

    // the 16 threads of a query, merged in the order of tx
    __syncthreads();
    Top2 *red = (Top2 *)ts;
#pragma unroll
    for (int a = 0; a < 4; ++a) red[(4 * ty + a) * 16 + tx] = best[a];
    __syncthreads();
    if (tid < kMatchQ) {
        const int i = qt * kMatchQ + tid;
        Top2 m = red[tid * 16];
        for (int x = 1; x < 16; ++x) m = merge(m, red[tid * 16 + x]);
        if (i < P.nq) parts[P.part0 + (long long)run.sp * P.nq + i] = m;
    }
}

__global__ __launch_bounds__(kThreads) void k_match_merge(const MatchPair *__restrict__ tab, const Top2 *__restrict__ parts,
                                                          int *__restrict__ idx, float *__restrict__ dist, int *__restrict__ idx2,
                                                          float *__restrict__ dist2) {
    const MatchPair P = tab[blockIdx.y];
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= P.nq) return;
    Top2 m = parts[P.part0 + i];
    for (int s = 1; s < P.splits; ++s) m = merge(m, parts[P.part0 + (long long)s * P.nq + i]);
    write_top2(m, (size_t)P.q0 + i, idx, dist, idx2, dist2);
}

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
    return pair_table_bytes(n_pairs) + kTiling.parts(q_offset, t_offset, n_pairs) * sizeof(Top2);
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
    const size_t need = apap_match_batch_workspace_bytes(q_offset, t_offset, n_pairs);
    if ((rc = match_device_check(d_q && d_t && d_idx && d_dist && d_work, true, d_q, d_t, d_work, work_bytes, need, who))) return rc;

    hipStream_t s = (hipStream_t)stream;
    MatchPair *d_tab = (MatchPair *)d_work;
    Top2 *d_parts = (Top2 *)((char *)d_work + pair_table_bytes(n_pairs));
    PairExtent ext;
    hipError_t e = upload_pair_table(kTiling, q_offset, t_offset, n_pairs, nullptr, d_tab, s, &ext);
    if (e != hipSuccess) return apap::hip_fail(e, "apap_match_descriptors_batch_device: descriptor upload");
    hipLaunchKernelGGL(k_match_sweep, dim3(ext.max_blocks, n_pairs), dim3(kThreads), 0, s, d_q, d_t, d_tab, d_parts);
    hipLaunchKernelGGL(k_match_merge, dim3((ext.max_nq + kThreads - 1) / kThreads, n_pairs), dim3(kThreads), 0, s, d_tab, d_parts, d_idx,
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
