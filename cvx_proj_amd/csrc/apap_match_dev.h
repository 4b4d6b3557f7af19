// What the exact matcher (apap_match.hip) and the guided matcher (apap_match_guided.hip) share, defined once: one squared
// distance, one order of the candidates, one record per pair, one split of the train axis, one finish.  The two promise the
// same bytes (tests/test_gpu_guided_match.py); the rules that make those bytes are here.  The sweeps stay in their sources.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#include "apap_internal.h"

namespace apap {

constexpr int kMaxPairs = 65535;    // grid.y
constexpr int kMaxRows = 1 << 24;   // queries / train rows of a pair: the guided list packs a row into 24 bits

struct Top2 {   // a query's running result over some train rows: (d2, index) of the best and of the runner-up
    float d1;
    int i1;
    float d2;
    int i2;
};
static_assert(sizeof(Top2) == 16, "Top2");
__device__ __forceinline__ Top2 empty_top2() { return Top2{INFINITY, -1, INFINITY, -1}; }

struct alignas(16) MatchPair {   // one pair, in device memory
    int q0, t0, nq, nt;          // first query / train row in the concatenated arrays, counts
    int q_tiles, splits, cps;    // blocks along the queries, splits of the train axis, chunks per split
    int rb0;                     // guided: the pair's first train row in the workspace's packed minima (the matcher: 0)
    long long part0;             // first partial of the pair: partial of (split s, query i) at part0 + s nq + i
    double r2;                   // guided: the gate's squared radius (the matcher: 0)
};
static_assert(sizeof(MatchPair) == 48, "MatchPair");

// One step of d2(i, j) = sum_k (q[i, k] - t[j, k])^2: float32, from acc = 0, k ascending.
__device__ __forceinline__ float d2_step(float acc, float q, float t) {
    const float d = q - t;
    return fmaf(d, d, acc);
}

// (da, ia) before (db, ib) in the order of the candidates.  An empty slot is (+inf, -1): no candidate is infinite, so every
// candidate comes before it, and it comes before nothing.
__device__ __forceinline__ bool before(float da, int ia, float db, int ib) { return da < db || (da == db && ia < ib); }

// (d, j) into m, wherever it stands in the order.
__device__ __forceinline__ void take(Top2 &m, float d, int j) {
    if (before(d, j, m.d1, m.i1)) {
        m.d2 = m.d1;
        m.i2 = m.i1;
        m.d1 = d;
        m.i1 = j;
    } else if (before(d, j, m.d2, m.i2)) {
        m.d2 = d;
        m.i2 = j;
    }
}

// take() for a j above every index that m has seen - the matcher's fold: a thread's train rows come in ascending order,
// inside a chunk and from chunk to chunk.  Among equal distances the earlier, lower index then stays under the strict
// comparisons, which is take()'s result without its index comparisons: with take() in the 4 x 8 fold k_match_sweep's chunk
// loop is 102 instructions longer (2922 -> 3024 in the kernel).
__device__ __forceinline__ void take_ascending(Top2 &m, float d, int j) {
    if (d < m.d1) {
        m.d2 = m.d1;
        m.i2 = m.i1;
        m.d1 = d;
        m.i1 = j;
    } else if (d < m.d2) {
        m.d2 = d;
        m.i2 = j;
    }
}

// The two first of a and b together (over disjoint train rows), as take(a, b's best), take(a, b's runner-up) would leave
// them: the order is total, so the best is the earlier of the two bests and the runner-up the earlier of the winner's
// runner-up and the loser's best - the loser's runner-up is behind its best.  An empty slot needs no guard: it is before
// nothing, so it replaces nothing, and every candidate replaces it.
__device__ __forceinline__ Top2 merge(Top2 a, Top2 b) {
    if (before(b.d1, b.i1, a.d1, a.i1)) {
        const Top2 s = a;
        a = b;
        b = s;
    }
    if (before(b.d1, b.i1, a.d2, a.i2)) {
        a.d2 = b.d1;
        a.i2 = b.i1;
    }
    return a;
}

// The run of train chunks of kChunk rows that block `block` of pair P sweeps for its query tile.
template <int kChunk>
struct PairRun {
    int qt, sp, c_begin, c_end;
    __device__ __forceinline__ PairRun(const MatchPair &P, unsigned block) : qt(block % P.q_tiles), sp(block / P.q_tiles) {
        const int n_chunks = (P.nt + kChunk - 1) / kChunk;
        c_begin = sp * P.cps;
        c_end = min(n_chunks, c_begin + P.cps);
    }
};

// A query's outputs at o; where nothing was selected the index is -1 and the distance +inf.
__device__ __forceinline__ void write_top2(const Top2 &m, size_t o, int *__restrict__ idx, float *__restrict__ dist,
                                           int *__restrict__ idx2, float *__restrict__ dist2) {
    // float32(sqrt in float64) is the correctly rounded float32 square root: 53 >= 2 * 24 + 2 bits
    idx[o] = m.i1;
    dist[o] = m.i1 >= 0 ? (float)sqrt((double)m.d1) : INFINITY;
    if (idx2) idx2[o] = m.i2;
    if (dist2) dist2[o] = m.i2 >= 0 ? (float)sqrt((double)m.d2) : INFINITY;
}

// ---------------------------------------------------------------- host side

// How a pair of (nq, nt) rows is cut: a function of the pair alone.  Enough blocks for several rounds over the chip, so that
// the last round's idle share is small.
struct SplitPlan {
    int q_tiles, splits, cps;
};
inline SplitPlan plan_split(int nq, int nt, int q_tile, int t_chunk, int want_blocks) {
    SplitPlan p;
    p.q_tiles = (nq + q_tile - 1) / q_tile;
    const int n_chunks = (nt + t_chunk - 1) / t_chunk;
    const int want = std::min(n_chunks, (want_blocks + p.q_tiles - 1) / p.q_tiles);
    p.cps = (n_chunks + want - 1) / want;
    p.splits = (n_chunks + p.cps - 1) / p.cps;
    return p;
}

// A matcher's tiling.  part_round: a pair's partials (one per query and split) take a multiple of this many slots.
struct MatchTiling {
    int q_tile, t_chunk, want_blocks;
    size_t part_round;
    size_t pair_parts(int nq, int nt) const {
        return ((size_t)plan_split(nq, nt, q_tile, t_chunk, want_blocks).splits * nq + part_round - 1) / part_round * part_round;
    }
    size_t parts(const int *q_offset, const int *t_offset, int n_pairs) const {   // of a batch
        size_t n = 0;
        for (int p = 0; p < n_pairs; ++p) n += pair_parts(q_offset[p + 1] - q_offset[p], t_offset[p + 1] - t_offset[p]);
        return n;
    }
};

inline size_t pair_table_bytes(int n_pairs) { return up256((size_t)n_pairs * sizeof(MatchPair)); }

// Fills the pairs' table (r2 null: the matcher's) and uploads it to d_tab in stream order.
struct PairExtent {
    int max_blocks, max_nq, max_nt;   // over the pairs: what the launches cover
};
inline hipError_t upload_pair_table(const MatchTiling &g, const int *q_offset, const int *t_offset, int n_pairs, const double *r2,
                                    MatchPair *d_tab, hipStream_t s, PairExtent *ext) {
    std::vector<MatchPair> tab((size_t)n_pairs);
    size_t off = 0;   // in partials
    *ext = PairExtent{0, 0, 0};
    for (int p = 0; p < n_pairs; ++p) {
        MatchPair &d = tab[p];
        d.q0 = q_offset[p];
        d.t0 = t_offset[p];
        d.nq = q_offset[p + 1] - q_offset[p];
        d.nt = t_offset[p + 1] - t_offset[p];
        const SplitPlan plan = plan_split(d.nq, d.nt, g.q_tile, g.t_chunk, g.want_blocks);
        d.q_tiles = plan.q_tiles;
        d.splits = plan.splits;
        d.cps = plan.cps;
        d.rb0 = r2 ? t_offset[p] - t_offset[0] : 0;
        d.part0 = (long long)off;
        d.r2 = r2 ? r2[p] : 0.0;
        off += g.pair_parts(d.nq, d.nt);
        ext->max_blocks = std::max(ext->max_blocks, plan.q_tiles * plan.splits);
        ext->max_nq = std::max(ext->max_nq, d.nq);
        ext->max_nt = std::max(ext->max_nt, d.nt);
    }
    // from pageable memory in stream order: the copy returns once its source has been consumed
    return hipMemcpyAsync(d_tab, tab.data(), (size_t)n_pairs * sizeof(MatchPair), hipMemcpyHostToDevice, s);
}

// The checks of a "_device" entry point's pointers and workspace.  pointers: every required one is there; reverse_paired:
// ridx and rdist were given together or not at all (the matcher has neither).
inline int match_device_check(bool pointers, bool reverse_paired, const void *d_q, const void *d_t, const void *d_work,
                              size_t work_bytes, size_t need, const char *who) {
    if (!pointers) return fail(APAP_ERR_INVALID_ARG, "%s: null device pointer", who);
    if (!reverse_paired) return fail(APAP_ERR_INVALID_ARG, "%s: ridx and rdist go together (both or neither)", who);
    if (work_bytes < need) return fail(APAP_ERR_WORKSPACE, "%s: workspace %zu < %zu bytes", who, work_bytes, need);
    if (((uintptr_t)d_work & 255) != 0 || ((uintptr_t)d_q & 15) != 0 || ((uintptr_t)d_t & 15) != 0)
        return fail(APAP_ERR_INVALID_ARG, "%s: workspace must be 256-byte and descriptors 16-byte aligned", who);
    return APAP_OK;
}

}  // namespace apap
