// Guided descriptor matching: apap_match_descriptors' nearest and second-nearest train row, searched only among the train rows
// that a geometric gate admits (include/apap_hip.h, DESIGN.md "Guided matching").
//
// Every keypoint of either side carries a record of three float64 (k_guided_records: the point itself, the point under a
// 3 x 3 model, or the line that the model makes of it).  The gate of a (query, train) pair is 6 float64 operations on the two
// records, each a single IEEE operation in the written order; the comparison is strict and a NaN fails it.
//
//     d2(i, j) = sum_k (q[i, k] - t[j, k])^2          float32, from acc = 0 by the matcher's d2_step, k ascending
//
// The step, the order of the candidates, the pair's record, the split of the train axis and the finish are the matcher's own
// (apap_match_dev.h).
//
// Candidates are ordered by (d2, train index), the reverse side by (d2, query index); a NaN or infinite d2 is counted by the
// gate and never selected.  Both orders are total, so no output depends on how the rows are cut into tiles, chunks and splits
// or on the order in which survivors are summed.  No nq x nt buffer and no floating-point atomics: the reverse side is an
// integer minimum over (bits of d2, query) - d2 is a sum of squares from +0, so its bits order as it does.
//
// k_guided_sweep<kind>: a block of 256 threads takes kGuidedQ = 256 queries, one per lane, and a run of train chunks of
// kGuidedT = 128 records staged in LDS (the two coordinates the gates read, 2 KiB).  A wave walks the chunk four rows at a time: the
// broadcast LDS reads, the gates, the ballots.  Where a row has survivors - about one row in nt / 70 - the wave appends
// (lane, row) to its own list in LDS; once the list holds kGuidedDrain = 64 entries (and at the end of the run) the wave
// drains it: lane e sums the 128 terms of entry e, so the serial sums run 64 abreast whichever lanes the survivors came
// from, and a query that admits every train row costs what 1 / 64 of a dense sweep costs.  A row appends at most 64 entries
// to fewer than 64: the list of 128 never overflows, nothing is truncated.  The wave then hands each result to its owner
// lane, which keeps (best, second) under the total order.  The train axis is split over blockIdx as in the matcher.
// k_guided_finish: one thread per query merges its splits' partials in ascending order, sums their counts and writes idx,
// dist, idx2, dist2, count; the same thread turns train row i's packed minimum into ridx, rdist.
//
// A batch is the same launches with the pair in blockIdx.y; the single call is the batch of one.
#include "apap_match_dev.h"

namespace {

using namespace apap;

constexpr int kDim = APAP_MATCH_DIM;
constexpr int kGuidedQ = APAP_GUIDED_QUERY_TILE;     // queries per block, one per lane
constexpr int kGuidedT = APAP_GUIDED_TRAIN_CHUNK;    // train records per staged chunk
constexpr int kGuidedDrain = APAP_GUIDED_DRAIN;      // survivors a wave sums at once
constexpr int kThreads = 256, kWave = 64;
constexpr int kGroup = 4;                            // train records gated between two looks at the ballots
constexpr unsigned long long kNone = ~0ull;          // a train row that no query has reached
static_assert(kDim == 128 && kGuidedQ == kThreads && kGuidedDrain == kWave && kGuidedT % kGroup == 0, "the thread mapping below is for these");
static_assert(kMaxRows <= (1 << 24), "a list entry packs the row into 24 bits");
constexpr MatchTiling kTiling{kGuidedQ, kGuidedT, APAP_GUIDED_WANT_BLOCKS, 1};   // the batch's partials are rounded once, together

struct GuidedPart {   // a query's running result over some train rows, and how many of them passed the gate
    Top2 m;
    int count;
    int pad;
};
static_assert(sizeof(GuidedPart) == 24, "GuidedPart");

__global__ __launch_bounds__(kThreads) void k_guided_records(const float *__restrict__ pts, int n, const double *__restrict__ model,
                                                             int what, double *__restrict__ rec) {
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const double X = (double)pts[2 * (size_t)i], Y = (double)pts[2 * (size_t)i + 1];
    double r0 = X, r1 = Y, r2 = 1.0;
    if (what != APAP_GUIDED_REC_POINT) {
        const double u = (model[0] * X + model[1] * Y) + model[2];
        const double v = (model[3] * X + model[4] * Y) + model[5];
        const double s = (model[6] * X + model[7] * Y) + model[8];
        if (what == APAP_GUIDED_REC_PROJECT) {
            r0 = u / s;
            r1 = v / s;
        } else {
            r0 = u;
            r1 = v;
            r2 = s;
        }
    }
    rec[3 * (size_t)i] = r0;
    rec[3 * (size_t)i + 1] = r1;
    rec[3 * (size_t)i + 2] = r2;
}

template <int kKind>
__global__ __launch_bounds__(kThreads) void k_guided_sweep(const double *__restrict__ rec_q, const double *__restrict__ rec_t,
                                                           const float *__restrict__ q, const float *__restrict__ t,
                                                           const MatchPair *__restrict__ tab, GuidedPart *__restrict__ parts,
                                                           unsigned long long *__restrict__ rbest) {
    const MatchPair P = tab[blockIdx.y];
    if (blockIdx.x >= (unsigned)(P.q_tiles * P.splits)) return;
    const PairRun<kGuidedT> run(P, blockIdx.x);
    const int qt = run.qt;

    __shared__ __attribute__((aligned(16))) double2 bs[kGuidedT];            // the chunk's records: the two coordinates
    __shared__ int lists[kThreads / kWave][2 * kGuidedDrain];                 // a wave's survivors: lane << 24 | train row

    const int tid = threadIdx.x, lane = tid & (kWave - 1);
    int *list = lists[tid / kWave];
    const int i = qt * kGuidedQ + tid;
    const bool valid = i < P.nq;
    const double *aq = rec_q + 3 * ((size_t)P.q0 + (valid ? i : 0));
    const double A0 = aq[0], A1 = aq[1], A2 = aq[2];
    const double nA = A0 * A0 + A1 * A1, r2 = P.r2;
    const double bound = kKind == APAP_GUIDED_LINE ? r2 * nA : r2;
    const float *qp = q + (size_t)P.q0 * kDim, *tp = t + (size_t)P.t0 * kDim;
    const int wave_q0 = qt * kGuidedQ + (tid - lane);   // the query of this wave's lane 0

    GuidedPart best{empty_top2(), 0, 0};
    int fill = 0;   // entries in the wave's list; wave-uniform

    // entries [fill - n, fill) of the list: lane e sums entry e, then every result goes to its owner lane
    auto drain = [&](int n) {
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");   // the wave's own appends are in LDS
        int entry = 0;
        float acc = 0.f;
        if (lane < n) {
            entry = list[fill - n + lane];
            const int j = entry & 0xFFFFFF, qi = wave_q0 + (entry >> 24);
            const float4 *a = (const float4 *)(qp + (size_t)qi * kDim), *b = (const float4 *)(tp + (size_t)j * kDim);
#pragma unroll 4
            for (int c = 0; c < kDim / 4; ++c) {
                const float4 av = a[c], bv = b[c];
                const float qa[4] = {av.x, av.y, av.z, av.w}, tv[4] = {bv.x, bv.y, bv.z, bv.w};
#pragma unroll
                for (int k = 0; k < 4; ++k) acc = d2_step(acc, qa[k], tv[k]);
            }
            // acc is finite here: not negative and not -0, so its bits order as it does
            if (rbest && acc < INFINITY)
                atomicMin(rbest + (size_t)P.rb0 + j, (unsigned long long)__float_as_uint(acc) << 32 | (unsigned)qi);
        }
        for (int e = 0; e < n; ++e) {
            const int en = __shfl(entry, e);
            const float d = __shfl(acc, e);
            if (lane == (en >> 24) && d < INFINITY) take(best.m, d, en & 0xFFFFFF);
        }
        fill -= n;
    };

    for (int chunk = run.c_begin; chunk < run.c_end; ++chunk) {
        const int rows = min(kGuidedT, P.nt - chunk * kGuidedT);
        __syncthreads();   // the previous chunk has been consumed
        // rows are walked in groups of kGroup: the chunk's last group is filled up with NaN, which passes no gate
        for (int r = tid; r < (rows + kGroup - 1) / kGroup * kGroup; r += kThreads) {
            const double *b = rec_t + 3 * ((size_t)P.t0 + (size_t)chunk * kGuidedT + min(r, rows - 1));
            bs[r] = r < rows ? make_double2(b[0], b[1]) : make_double2(NAN, NAN);
        }
        __syncthreads();
        for (int r = 0; r < rows; r += kGroup) {
            bool pass[kGroup];
            unsigned long long mask[kGroup], any = 0;
#pragma unroll
            for (int u = 0; u < kGroup; ++u) {   // the group's LDS reads are in flight together
                const double2 B = bs[r + u];
                if (kKind == APAP_GUIDED_LINE) {
                    const double e = (A0 * B.x + A1 * B.y) + A2;
                    pass[u] = e * e < bound;
                } else {
                    const double dx = B.x - A0, dy = B.y - A1;
                    pass[u] = dx * dx + dy * dy < bound;
                }
                pass[u] = pass[u] && valid;
                mask[u] = __ballot(pass[u]);
                any |= mask[u];
            }
            if (any == 0) continue;   // wave-uniform, as everything about the list
#pragma unroll
            for (int u = 0; u < kGroup; ++u) {
                if (mask[u] == 0) continue;
                if (pass[u]) {
                    best.count += 1;
                    list[fill + __popcll(mask[u] & ((1ull << lane) - 1))] = lane << 24 | (chunk * kGuidedT + r + u);
                }
                fill += __popcll(mask[u]);
                if (fill >= kGuidedDrain) drain(kGuidedDrain);
            }
        }
    }
    if (fill > 0) drain(fill);
    if (valid) parts[P.part0 + (long long)run.sp * P.nq + i] = best;
}

__global__ __launch_bounds__(kThreads) void k_guided_finish(const MatchPair *__restrict__ tab, const GuidedPart *__restrict__ parts,
                                                            const unsigned long long *__restrict__ rbest, int *__restrict__ idx,
                                                            float *__restrict__ dist, int *__restrict__ idx2, float *__restrict__ dist2,
                                                            int *__restrict__ count, int *__restrict__ ridx, float *__restrict__ rdist) {
    const MatchPair P = tab[blockIdx.y];
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i < P.nq) {
        GuidedPart m = parts[P.part0 + i];
        for (int s = 1; s < P.splits; ++s) {
            const GuidedPart b = parts[P.part0 + (long long)s * P.nq + i];
            m.m = merge(m.m, b.m);
            m.count += b.count;
        }
        write_top2(m.m, (size_t)P.q0 + i, idx, dist, idx2, dist2);
        if (count) count[(size_t)P.q0 + i] = m.count;
    }
    if (ridx && i < P.nt) {
        const size_t o = (size_t)P.t0 + i;
        const unsigned long long v = rbest[(size_t)P.rb0 + i];
        ridx[o] = v == kNone ? -1 : (int)(unsigned)v;
        rdist[o] = v == kNone ? INFINITY : (float)sqrt((double)__uint_as_float((unsigned)(v >> 32)));
    }
}

size_t reverse_bytes(size_t train_rows) { return apap::up256(train_rows * sizeof(unsigned long long)); }

}  // namespace

namespace apap {

// The argument checks of the guided matcher's entry points that need no device pointer: the matcher's, the kind, every r2.
int guided_check(const int *q_offset, const int *t_offset, int n_pairs, int kind, const double *r2, const char *who) {
    const int rc = match_check(q_offset, t_offset, n_pairs, who);
    if (rc) return rc;
    if (kind != APAP_GUIDED_POINT && kind != APAP_GUIDED_LINE)
        return fail(APAP_ERR_INVALID_ARG, "%s: kind = %d (APAP_GUIDED_POINT or APAP_GUIDED_LINE)", who, kind);
    if (!r2) return fail(APAP_ERR_INVALID_ARG, "%s: null r2", who);
    for (int p = 0; p < n_pairs; ++p)
        if (!(r2[p] >= 0.0)) return fail(APAP_ERR_INVALID_ARG, "%s: pair %d: r2 = %g (>= 0 or +inf)", who, p, r2[p]);
    return APAP_OK;
}

// ... and of its records.
int guided_records_check(int n, const void *model, int what, const char *who) {
    if (n < 1 || n > kMaxRows) return fail(APAP_ERR_INVALID_ARG, "%s: n = %d (1 .. 2^24 keypoints)", who, n);
    if (what != APAP_GUIDED_REC_POINT && what != APAP_GUIDED_REC_PROJECT && what != APAP_GUIDED_REC_LINE)
        return fail(APAP_ERR_INVALID_ARG, "%s: what = %d (APAP_GUIDED_REC_POINT, _PROJECT or _LINE)", who, what);
    if (what != APAP_GUIDED_REC_POINT && !model) return fail(APAP_ERR_INVALID_ARG, "%s: what = %d needs a model", who, what);
    return APAP_OK;
}

}  // namespace apap

extern "C" {

int apap_guided_records_device(apap_ctx *ctx, const float *d_pts, int n, const double *d_model, int what, double *d_rec_out,
                               void *stream) {
    const char *who = "apap_guided_records_device";
    (void)ctx;
    const int rc = apap::guided_records_check(n, d_model, what, who);
    if (rc) return rc;
    if (!d_pts || !d_rec_out) return apap::fail(APAP_ERR_INVALID_ARG, "%s: null device pointer", who);
    hipLaunchKernelGGL(k_guided_records, dim3((n + kThreads - 1) / kThreads), dim3(kThreads), 0, (hipStream_t)stream, d_pts, n,
                       d_model, what, d_rec_out);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return apap::hip_fail(e, "apap_guided_records_device launch");
    return APAP_OK;
}

size_t apap_match_guided_batch_workspace_bytes(const int *q_offset, const int *t_offset, int n_pairs) {
    if (apap::match_check(q_offset, t_offset, n_pairs, "apap_match_guided_batch_workspace_bytes")) return 0;
    return pair_table_bytes(n_pairs) + reverse_bytes((size_t)t_offset[n_pairs] - (size_t)t_offset[0]) +
           apap::up256(kTiling.parts(q_offset, t_offset, n_pairs) * sizeof(GuidedPart));
}

size_t apap_match_guided_workspace_bytes(int nq, int nt) {
    const int qo[2] = {0, nq}, to[2] = {0, nt};
    return apap_match_guided_batch_workspace_bytes(qo, to, 1);
}

int apap_match_guided_batch_device(apap_ctx *ctx, const double *d_rec_q, const double *d_rec_t, const float *d_q, const float *d_t,
                                   const int *q_offset, const int *t_offset, int n_pairs, int kind, const double *r2, int *d_idx,
                                   float *d_dist, int *d_idx2, float *d_dist2, int *d_count, int *d_ridx, float *d_rdist,
                                   void *d_work, size_t work_bytes, void *stream) {
    const char *who = "apap_match_guided_batch_device";
    (void)ctx;
    int rc = apap::guided_check(q_offset, t_offset, n_pairs, kind, r2, who);
    if (rc) return rc;
    const size_t need = apap_match_guided_batch_workspace_bytes(q_offset, t_offset, n_pairs);
    if ((rc = match_device_check(d_rec_q && d_rec_t && d_q && d_t && d_idx && d_dist && d_work, !d_ridx == !d_rdist, d_q, d_t, d_work,
                                 work_bytes, need, who)))
        return rc;

    // the workspace: the pairs' table, the train rows' packed minima (from t_offset[0] on), the partials
    const size_t train_rows = (size_t)t_offset[n_pairs] - (size_t)t_offset[0];
    const size_t at_rbest = pair_table_bytes(n_pairs), at_parts = at_rbest + reverse_bytes(train_rows);
    hipStream_t s = (hipStream_t)stream;
    MatchPair *d_tab = (MatchPair *)d_work;
    unsigned long long *d_rbest = d_ridx ? (unsigned long long *)((char *)d_work + at_rbest) : nullptr;
    GuidedPart *d_parts = (GuidedPart *)((char *)d_work + at_parts);
    PairExtent ext;
    hipError_t e = upload_pair_table(kTiling, q_offset, t_offset, n_pairs, r2, d_tab, s, &ext);
    if (e != hipSuccess) return apap::hip_fail(e, "apap_match_guided_batch_device: descriptor upload");
    const int max_blocks = ext.max_blocks, max_rows = std::max(ext.max_nq, d_ridx ? ext.max_nt : 0);
    if (d_ridx && (e = hipMemsetAsync((char *)d_work + at_rbest, 0xFF, train_rows * sizeof(unsigned long long), s)) != hipSuccess)
        return apap::hip_fail(e, "apap_match_guided_batch_device: reverse fill");
    if (kind == APAP_GUIDED_LINE)
        hipLaunchKernelGGL(k_guided_sweep<APAP_GUIDED_LINE>, dim3(max_blocks, n_pairs), dim3(kThreads), 0, s, d_rec_q, d_rec_t, d_q,
                           d_t, d_tab, d_parts, d_rbest);
    else
        hipLaunchKernelGGL(k_guided_sweep<APAP_GUIDED_POINT>, dim3(max_blocks, n_pairs), dim3(kThreads), 0, s, d_rec_q, d_rec_t, d_q,
                           d_t, d_tab, d_parts, d_rbest);
    hipLaunchKernelGGL(k_guided_finish, dim3((max_rows + kThreads - 1) / kThreads, n_pairs), dim3(kThreads), 0, s, d_tab, d_parts,
                       d_rbest, d_idx, d_dist, d_idx2, d_dist2, d_count, d_ridx, d_rdist);
    e = hipGetLastError();
    if (e != hipSuccess) return apap::hip_fail(e, "apap_match_guided_batch_device launch");
    return APAP_OK;
}

int apap_match_guided_device(apap_ctx *ctx, const double *d_rec_q, const float *d_q, int nq, const double *d_rec_t, const float *d_t,
                             int nt, int kind, double r2, int *d_idx, float *d_dist, int *d_idx2, float *d_dist2, int *d_count,
                             int *d_ridx, float *d_rdist, void *d_work, size_t work_bytes, void *stream) {
    const int qo[2] = {0, nq}, to[2] = {0, nt};
    return apap_match_guided_batch_device(ctx, d_rec_q, d_rec_t, d_q, d_t, qo, to, 1, kind, &r2, d_idx, d_dist, d_idx2, d_dist2,
                                          d_count, d_ridx, d_rdist, d_work, work_bytes, stream);
}

}  // extern "C"
