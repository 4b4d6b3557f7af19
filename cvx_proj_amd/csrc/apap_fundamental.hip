// Fundamental matrix from matches by RANSAC, the contract of cv.findFundamentalMat(src, dst, cv.FM_RANSAC, thresh)
// (specification: tests/fundamental_spec.py, bit for bit; DESIGN.md "Fundamental matrix from matches").  The sibling of the
// seed homography's R1-R3 (apap_frontend.hip), for a batch of pairs: blockIdx.y is the pair in every kernel, the pairs'
// offsets come from a table in the workspace, and the number of launches does not depend on the number of pairs.  The
// sampler of F2 and the bodies of F3 and F4 are apap_ransac_dev.h's, shared with R1-R3; the system, its elimination and the
// predicate are here.
// F1 k_fund_box:    the bounding boxes of a pair's two point sets -> centre and scale of the normalisation.
// F2 k_fund_hyp:    one lane per hypothesis - the counter-based sampler (8 draws), the 8 x 9 system reduced by Gaussian
//    elimination with complete pivoting on a lane-private system kept in LDS (dynamic row and column indices; index-major
//    layout, so the 64 lanes never conflict), back substitution, de-normalisation.
// F3 k_fund_score:  one block per hypothesis and pair counts the matches within the Sampson threshold.
// F4 k_fund_select: first hypothesis with the most inliers, its matrix, its mask, {winner, count}.
// F5 k_fund_refit:  one block per pair: A^T A over the inliers in one fixed summation tree, cyclic Jacobi for its smallest
//    eigenvector, rank 2 by a one-sided Jacobi SVD, de-normalisation, scale and sign.
// Every product, sum and quotient is rounded on its own (the library is built with -ffp-contract=off; float64 division and
// square root are correctly rounded), in the order the specification writes down.  No atomics.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <vector>

#include "apap_internal.h"
#include "apap_ransac_dev.h"

namespace {

constexpr int kMinPoints = 8;
constexpr int kMaxPairs = 65535;      // gridDim.y
constexpr int kHypLanes = 64;
constexpr int kThreads = apap::kConsensusThreads;      // every block but the hypotheses'
constexpr int kSweepCap = 30;

// The parts of the workspace (include/apap_hip.h documents them): byte offsets, each a multiple of 256.
struct FundLayout {
    size_t table, boxes, hyps, winners, counts, total;
};
FundLayout fund_layout(int n_pairs, int iterations) {
    FundLayout L;
    size_t at = 0;
    L.table = at;   at += apap::up256(((size_t)n_pairs + 1) * sizeof(int));
    L.boxes = at;   at += apap::up256((size_t)n_pairs * 8 * sizeof(double));
    L.hyps = at;    at += apap::up256((size_t)n_pairs * iterations * 9 * sizeof(double));
    L.winners = at; at += apap::up256((size_t)n_pairs * 9 * sizeof(double));
    L.counts = at;  at += apap::up256((size_t)n_pairs * iterations * sizeof(int));
    L.total = at;
    return L;
}

// centre and scale of one point set
struct Norm {
    double cx, cy, s;
};
__device__ __forceinline__ Norm load_norm(const double *__restrict__ box) { return Norm{box[0], box[1], box[2]}; }

// T_d^T F_n T_s: G = F_n T_s column by column, then T_d^T G row by row
__device__ __forceinline__ void denormalise(const double (&f)[9], const Norm &ns, const Norm &nd, double (&out)[9]) {
    double g[9];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        g[3 * i] = f[3 * i] * ns.s;
        g[3 * i + 1] = f[3 * i + 1] * ns.s;
        const double a = g[3 * i] * ns.cx, b = g[3 * i + 1] * ns.cy;
        g[3 * i + 2] = (f[3 * i + 2] - a) - b;
    }
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        out[j] = g[j] * nd.s;
        out[3 + j] = g[3 + j] * nd.s;
        const double a = out[j] * nd.cx, b = out[3 + j] * nd.cy;
        out[6 + j] = (g[6 + j] - a) - b;
    }
}

// ---------------------------------------------------------------- F1
__global__ __launch_bounds__(kThreads) void k_fund_box(const float *__restrict__ src, const float *__restrict__ dst,
                                                       const int *__restrict__ offset, double *__restrict__ boxes) {
    __shared__ float s_part[kThreads / 64][8];
    const int pair = blockIdx.y, k0 = offset[pair], n = offset[pair + 1] - k0;
    const float2 *s2 = reinterpret_cast<const float2 *>(src) + k0, *d2 = reinterpret_cast<const float2 *>(dst) + k0;
    // lo x, lo y, -hi x, -hi y of src, then of dst: eight minima (min and max are exact in any order)
    float m[8];
    {
        const float2 s = s2[0], d = d2[0];      // n >= 8
        m[0] = s.x; m[1] = s.y; m[2] = -s.x; m[3] = -s.y;
        m[4] = d.x; m[5] = d.y; m[6] = -d.x; m[7] = -d.y;
    }
    for (int k = threadIdx.x; k < n; k += kThreads) {
        const float2 s = s2[k], d = d2[k];
        const float v[8] = {s.x, s.y, -s.x, -s.y, d.x, d.y, -d.x, -d.y};
#pragma unroll
        for (int i = 0; i < 8; ++i) m[i] = v[i] < m[i] ? v[i] : m[i];
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) {
            const float o = __shfl_down(m[i], d);
            m[i] = o < m[i] ? o : m[i];
        }
    }
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int i = 0; i < 8; ++i) s_part[threadIdx.x >> 6][i] = m[i];
    }
    __syncthreads();
    if (threadIdx.x < 2) {      // thread 0: src, thread 1: dst
        float q[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            q[i] = s_part[0][4 * threadIdx.x + i];
#pragma unroll
            for (int w = 1; w < kThreads / 64; ++w) {
                const float o = s_part[w][4 * threadIdx.x + i];
                q[i] = o < q[i] ? o : q[i];
            }
        }
        const double lox = (double)q[0], loy = (double)q[1], hix = -(double)q[2], hiy = -(double)q[3];
        const double ex = hix - lox, ey = hiy - loy;
        const double ext = ex > ey ? ex : ey;
        double *b = boxes + (size_t)pair * 8 + 4 * threadIdx.x;
        b[0] = (lox + hix) / 2.0;
        b[1] = (loy + hiy) / 2.0;
        b[2] = 2.0 / ext;      // extent 0: inf, and every normalised coordinate NaN
        b[3] = ext;
    }
}

// ---------------------------------------------------------------- F2
__global__ __launch_bounds__(kHypLanes) void k_fund_hyp(const float *__restrict__ src, const float *__restrict__ dst,
                                                        const int *__restrict__ offset, const double *__restrict__ boxes,
                                                        int iterations, unsigned long long seed,
                                                        double *__restrict__ hyps /* pairs x iterations x 9 */) {
    __shared__ double sys[72][kHypLanes];
    __shared__ int perm[9][kHypLanes];
    const int t = threadIdx.x;
    const int h = blockIdx.x * kHypLanes + t;
    if (h >= iterations) return;      // lane-private work below: no barriers
    const int pair = blockIdx.y, k0 = offset[pair], n = offset[pair + 1] - k0;
    const Norm ns = load_norm(boxes + (size_t)pair * 8), nd = load_norm(boxes + (size_t)pair * 8 + 4);
#define A(r, c) sys[(r) * 9 + (c)][t]
    int pick[8];      // eight distinct matches of the pair
    apap::draw_distinct<8>(seed, h, n, pick);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const float2 s = reinterpret_cast<const float2 *>(src)[k0 + pick[j]];
        const float2 d = reinterpret_cast<const float2 *>(dst)[k0 + pick[j]];
        const double x = ((double)s.x - ns.cx) * ns.s, y = ((double)s.y - ns.cy) * ns.s;
        const double u = ((double)d.x - nd.cx) * nd.s, v = ((double)d.y - nd.cy) * nd.s;
        A(j, 0) = u * x; A(j, 1) = u * y; A(j, 2) = u;
        A(j, 3) = v * x; A(j, 4) = v * y; A(j, 5) = v;
        A(j, 6) = x; A(j, 7) = y; A(j, 8) = 1.0;
    }
    for (int c = 0; c < 9; ++c) perm[c][t] = c;
    bool ok = true;
    for (int c = 0; c < 8; ++c) {
        // complete pivoting: the largest |a| of rows c .. 7, columns c .. 8, the first in row-major order; NaN never wins
        int pr = c, pc = c;
        double best = -1.0;
        for (int r = c; r < 8; ++r) {
            for (int cc = c; cc < 9; ++cc) {
                const double v = fabs(A(r, cc));
                if (v > best) { best = v; pr = r; pc = cc; }
            }
        }
        if (pr != c) {
            for (int cc = c; cc < 9; ++cc) {      // the columns before c are not read again
                const double tmp = A(pr, cc);
                A(pr, cc) = A(c, cc);
                A(c, cc) = tmp;
            }
        }
        if (pc != c) {
            for (int r = 0; r < 8; ++r) {
                const double tmp = A(r, pc);
                A(r, pc) = A(r, c);
                A(r, c) = tmp;
            }
            const int tmp = perm[pc][t];
            perm[pc][t] = perm[c][t];
            perm[c][t] = tmp;
        }
        const double piv = A(c, c);
        ok = ok && piv != 0.0 && isfinite(piv);
        for (int r = c + 1; r < 8; ++r) {
            const double f = A(r, c) / piv;
            for (int cc = c + 1; cc < 9; ++cc) {
                const double prod = f * A(c, cc);
                A(r, cc) = A(r, cc) - prod;
            }
        }
    }
    // the column never chosen is the free unknown and gets 1
    double sol[9];
    sol[8] = 1.0;
#pragma unroll
    for (int i = 7; i >= 0; --i) {
        double s = -A(i, 8);
#pragma unroll
        for (int j = i + 1; j < 8; ++j) {
            const double prod = A(i, j) * sol[j];
            s = s - prod;
        }
        sol[i] = s / A(i, i);
    }
#undef A
    // un-permute through LDS: the system is done with, its first nine slots take the matrix
#pragma unroll
    for (int k = 0; k < 9; ++k) sys[perm[k][t]][t] = sol[k];
    double fn[9], fp[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) fn[k] = sys[k][t];
    denormalise(fn, ns, nd, fp);
#pragma unroll
    for (int k = 0; k < 9; ++k) ok = ok && isfinite(fp[k]);
    const double nan = __builtin_nan("");
    double *out = hyps + ((size_t)pair * iterations + h) * 9;
#pragma unroll
    for (int k = 0; k < 9; ++k) out[k] = ok ? fp[k] : nan;
}

// squared Sampson distance against the threshold, operations in the specification's order
__device__ __forceinline__ bool fund_inlier(const double (&f)[9], double x, double y, double u, double v, double thr2) {
    const double a1 = (f[0] * x + f[1] * y) + f[2];
    const double a2 = (f[3] * x + f[4] * y) + f[5];
    const double a3 = (f[6] * x + f[7] * y) + f[8];
    const double r = (u * a1 + v * a2) + a3;
    const double b1 = (f[0] * u + f[3] * v) + f[6];
    const double b2 = (f[1] * u + f[4] * v) + f[7];
    const double den = ((a1 * a1 + a2 * a2) + b1 * b1) + b2 * b2;
    return (r * r) / den <= thr2;      // NaN compares false
}

// ---------------------------------------------------------------- F3
__global__ __launch_bounds__(kThreads) void k_fund_score(const float *__restrict__ src, const float *__restrict__ dst,
                                                         const int *__restrict__ offset, const double *__restrict__ hyps,
                                                         int iterations, double thr2, int *__restrict__ counts) {
    const int pair = blockIdx.y, k0 = offset[pair], n = offset[pair + 1] - k0;
    const size_t slot = (size_t)pair * iterations + blockIdx.x;
    apap::consensus_score(src, dst, apap::MatchRange{k0, n}, hyps + slot * 9, thr2, fund_inlier, counts + slot);
}

// ---------------------------------------------------------------- F4
__global__ __launch_bounds__(kThreads) void k_fund_select(const float *__restrict__ src, const float *__restrict__ dst,
                                                          const int *__restrict__ offset, const double *__restrict__ hyps,
                                                          const int *__restrict__ counts, int iterations, double thr2,
                                                          double *__restrict__ winners, uint8_t *__restrict__ mask,
                                                          int *__restrict__ result) {
    const int pair = blockIdx.y, k0 = offset[pair], n = offset[pair + 1] - k0;
    apap::consensus_select(src, dst, apap::MatchRange{k0, n}, hyps + (size_t)pair * iterations * 9, counts + (size_t)pair * iterations,
                           iterations, thr2, fund_inlier, winners + (size_t)pair * 9, mask, result + 2 * pair);
}

// ---------------------------------------------------------------- F5
// t, c, s of the Jacobi rotation that annihilates `off`, given the difference of the two diagonal terms
__device__ __forceinline__ void jacobi_angle(double diff, double off, double &t, double &c, double &s) {
    const double theta = diff / (off + off);
    t = 1.0 / (fabs(theta) + sqrt(theta * theta + 1.0));
    if (theta < 0.0) t = -t;
    c = 1.0 / sqrt(t * t + 1.0);
    s = t * c;
}

// What round r of a Jacobi sweep does to index x of the 9 x 9 matrix A (LDS, row-major): its partner (2 r - x) mod 9 (itself
// when x rests), whether x is the pair's smaller index p, and the pair's turn - kind 0: a_pq is zero, nothing; 1: a_pq is
// negligible beside both diagonal terms and is set to zero; 2: a rotation (t, c, s).
struct PairTurn {
    int partner, kind;
    bool is_p;
    double t, c, s, apq, app, aqq;
};
__device__ __forceinline__ PairTurn pair_turn(const double *A, int x, int r) {
    PairTurn R;
    R.partner = (2 * r - x + 9) % 9;
    R.is_p = x < R.partner;
    R.kind = 0;
    R.t = 0.0; R.c = 1.0; R.s = 0.0;
    const int p = R.is_p ? x : R.partner, q = R.is_p ? R.partner : x;
    R.apq = A[p * 9 + q]; R.app = A[p * 9 + p]; R.aqq = A[q * 9 + q];
    if (p == q || R.apq == 0.0) return R;
    const double g = 100.0 * fabs(R.apq);
    if (fabs(R.app) + g == fabs(R.app) && fabs(R.aqq) + g == fabs(R.aqq)) {
        R.kind = 1;
        return R;
    }
    R.kind = 2;
    jacobi_angle(R.aqq - R.app, R.apq, R.t, R.c, R.s);
    return R;
}
// The entry `self` of a row or column with index x after its pair's rotation, `other` being the partner's entry:
// p' = c p - s q, q' = s p + c q.
__device__ __forceinline__ double turn(double self, double other, const PairTurn &R) {
    if (R.kind != 2) return self;
    const double cs = R.c * self, so = R.s * other;
    return R.is_p ? cs - so : so + cs;
}

__device__ __forceinline__ double dot3(double a0, double a1, double a2, double b0, double b1, double b2) {
    return (a0 * b0 + a1 * b1) + a2 * b2;
}

__global__ __launch_bounds__(kThreads) void k_fund_refit(const float *__restrict__ src, const float *__restrict__ dst,
                                                         const int *__restrict__ offset, const double *__restrict__ boxes,
                                                         const uint8_t *__restrict__ mask, const int *__restrict__ result,
                                                         double *__restrict__ F_out /* pairs x 9 */) {
    __shared__ double s_wave[kThreads / 64][45];
    __shared__ double sA[81], sV[81];
    __shared__ double s_max[kThreads / 64];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int pair = blockIdx.y, k0 = offset[pair], n = offset[pair + 1] - k0;
    const double nan = __builtin_nan("");
    double *out = F_out + (size_t)pair * 9;
    if (result[2 * pair + 1] < kMinPoints) {      // uniform over the block
        if (t < 9) out[t] = nan;
        return;
    }
    const Norm ns = load_norm(boxes + (size_t)pair * 8), nd = load_norm(boxes + (size_t)pair * 8 + 4);
    const float2 *s2 = reinterpret_cast<const float2 *>(src) + k0, *d2 = reinterpret_cast<const float2 *>(dst) + k0;
    // step 7, the 45 sums: this lane's inliers in ascending order ...
    double acc[45];
#pragma unroll
    for (int i = 0; i < 45; ++i) acc[i] = 0.0;
    for (int k = t; k < n; k += kThreads) {
        if (!mask[(size_t)k0 + k]) continue;      // skipped, not added as zeros
        const float2 s = s2[k], d = d2[k];
        const double x = ((double)s.x - ns.cx) * ns.s, y = ((double)s.y - ns.cy) * ns.s;
        const double u = ((double)d.x - nd.cx) * nd.s, v = ((double)d.y - nd.cy) * nd.s;
        const double r[9] = {u * x, u * y, u, v * x, v * y, v, x, y, 1.0};
        int e = 0;
#pragma unroll
        for (int i = 0; i < 9; ++i) {
#pragma unroll
            for (int j = i; j < 9; ++j) {
                const double prod = r[i] * r[j];
                acc[e] = acc[e] + prod;
                ++e;
            }
        }
    }
    // ... then v[l] += v[l + d] for d = 32 .. 1 in each wave, then the four waves in ascending order
#pragma unroll
    for (int i = 0; i < 45; ++i) {
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) acc[i] = acc[i] + __shfl_down(acc[i], d);
    }
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < 45; ++i) s_wave[wave][i] = acc[i];
    }
    __syncthreads();
    if (t < 81) {
        const int i = t / 9, j = t % 9;
        const int a = i < j ? i : j, b = i < j ? j : i;
        const int e = a * 9 - a * (a - 1) / 2 + (b - a);      // entry (a, b), a <= b, of the row-major upper triangle
        sA[t] = ((s_wave[0][e] + s_wave[1][e]) + s_wave[2][e]) + s_wave[3][e];
        sV[t] = i == j ? 1.0 : 0.0;
    }
    __syncthreads();
    // cyclic Jacobi in the round-robin order: round r of a sweep turns the four disjoint pairs {(r + k) % 9, (r - k) % 9},
    // k = 1 .. 4, at once (index r rests), A <- J^T (A J) with the columns turned first.  Thread 9 i + j owns entry (i, j):
    // it works out the rotations of its row's and its column's pair itself (every thread that shares a pair computes the same
    // bits), entries with i <= j are computed and mirrored.  Two barriers a round.
    const int ei = t / 9, ej = t % 9;      // t < 81
    for (int sweep = 0; sweep < kSweepCap; ++sweep) {
        bool rotated = false;
        for (int r = 0; r < 9; ++r) {
            double a_new = 0.0, v_new = 0.0;
            bool mine = false;
            if (t < 81) {
                const PairTurn Ri = pair_turn(sA, ei, r), Rj = pair_turn(sA, ej, r);
                mine = Ri.kind == 2 || Rj.kind == 2;
                const int ip = Ri.partner, jp = Rj.partner;
                v_new = turn(sV[ei * 9 + ej], sV[ei * 9 + jp], Rj);
                if (ei <= ej) {
                    const double b_ij = turn(sA[ei * 9 + ej], sA[ei * 9 + jp], Rj);
                    const double b_pj = turn(sA[ip * 9 + ej], sA[ip * 9 + jp], Rj);
                    a_new = turn(b_ij, b_pj, Ri);
                    if (ej == ip && Ri.kind != 0) a_new = 0.0;      // the pair's own off-diagonal entry
                    if (ei == ej && Ri.kind == 2) a_new = Ri.is_p ? Ri.app - Ri.t * Ri.apq : Ri.aqq + Ri.t * Ri.apq;
                }
            }
            rotated = __syncthreads_or(mine ? 1 : 0) != 0 || rotated;      // all have read before any writes
            if (t < 81) {
                sV[t] = v_new;
                if (ei <= ej) {
                    sA[ei * 9 + ej] = a_new;
                    sA[ej * 9 + ei] = a_new;
                }
            }
            __syncthreads();
        }
        if (!rotated) break;
    }
    // the eigenvector of the smallest eigenvalue (the first such); from here every thread computes the same matrix
    int kmin = 0;
    {
        double dmin = sA[0];
        for (int i = 1; i < 9; ++i) {
            const double d = sA[i * 9 + i];
            if (d < dmin) { dmin = d; kmin = i; }
        }
    }
    double G[3][3], W[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            G[i][j] = sV[(3 * i + j) * 9 + kmin];
            W[i][j] = i == j ? 1.0 : 0.0;
        }
    }
    // rank 2: one-sided Jacobi on the columns, then the column of smallest norm zeroed and G W^T
    for (int sweep = 0; sweep < kSweepCap; ++sweep) {
        bool rotated = false;
#pragma unroll
        for (int p = 0; p < 2; ++p) {
#pragma unroll
            for (int q = p + 1; q < 3; ++q) {
                const double alpha = dot3(G[0][p], G[1][p], G[2][p], G[0][p], G[1][p], G[2][p]);
                const double beta = dot3(G[0][q], G[1][q], G[2][q], G[0][q], G[1][q], G[2][q]);
                const double gamma = dot3(G[0][p], G[1][p], G[2][p], G[0][q], G[1][q], G[2][q]);
                if (gamma == 0.0) continue;
                const double lim = sqrt(alpha * beta);
                if (lim + fabs(gamma) == lim) continue;
                rotated = true;
                double tn, c, s;
                jacobi_angle(beta - alpha, gamma, tn, c, s);
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    const double gp = G[i][p], gq = G[i][q];
                    const double a1 = c * gp, a2 = s * gq, a3 = s * gp, a4 = c * gq;
                    G[i][p] = a1 - a2;
                    G[i][q] = a3 + a4;
                    const double wp = W[i][p], wq = W[i][q];
                    const double b1 = c * wp, b2 = s * wq, b3 = s * wp, b4 = c * wq;
                    W[i][p] = b1 - b2;
                    W[i][q] = b3 + b4;
                }
            }
        }
        if (!rotated) break;
    }
    {
        double nrm[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) nrm[k] = dot3(G[0][k], G[1][k], G[2][k], G[0][k], G[1][k], G[2][k]);
        int kz = 0;
        if (nrm[1] < nrm[0]) kz = 1;
        if (nrm[2] < (kz == 1 ? nrm[1] : nrm[0])) kz = 2;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
#pragma unroll
            for (int k = 0; k < 3; ++k) G[i][k] = k == kz ? 0.0 : G[i][k];
        }
    }
    double fn[9], fp[9];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) fn[3 * i + j] = dot3(G[i][0], G[i][1], G[i][2], W[j][0], W[j][1], W[j][2]);
    }
    denormalise(fn, ns, nd, fp);
    // step 8: g = max over all n matches of |(F s)[:2]|; NaN terms are passed over, the maximum starts at 0
    double g = 0.0;
    for (int k = t; k < n; k += kThreads) {
        const float2 s = s2[k];
        const double x = (double)s.x, y = (double)s.y;
        const double a1 = (fp[0] * x + fp[1] * y) + fp[2];
        const double a2 = (fp[3] * x + fp[4] * y) + fp[5];
        const double v = sqrt(a1 * a1 + a2 * a2);
        if (v > g) g = v;
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        const double o = __shfl_down(g, d);
        if (o > g) g = o;
    }
    if (lane == 0) s_max[wave] = g;
    __syncthreads();
    if (t != 0) return;
    g = s_max[0];
    for (int w = 1; w < kThreads / 64; ++w) {
        if (s_max[w] > g) g = s_max[w];
    }
    bool ok = g > 0.0 && isfinite(g);
    double f[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        f[k] = fp[k] / g;
        ok = ok && isfinite(f[k]);
    }
    double big = fabs(f[0]), at = f[0];
#pragma unroll
    for (int k = 1; k < 9; ++k) {
        if (fabs(f[k]) > big) { big = fabs(f[k]); at = f[k]; }      // the first of largest magnitude
    }
    const bool flip = at < 0.0;
#pragma unroll
    for (int k = 0; k < 9; ++k) out[k] = ok ? (flip ? -f[k] : f[k]) : nan;
}

}  // namespace

namespace apap {

// The argument checks of the fundamental-matrix entry points that need no device pointer.
int fundamental_check(const int *pair_offset, int n_pairs, double thresh, int iterations, const char *who) {
    if (!pair_offset) return apap::fail(APAP_ERR_INVALID_ARG, "%s: null pair_offset", who);
    if (n_pairs < 1 || n_pairs > kMaxPairs) return apap::fail(APAP_ERR_INVALID_ARG, "%s: n_pairs = %d (1 .. %d)", who, n_pairs, kMaxPairs);
    if (pair_offset[0] < 0) return apap::fail(APAP_ERR_INVALID_ARG, "%s: pair_offset[0] = %d: negative", who, pair_offset[0]);
    for (int p = 0; p < n_pairs; ++p) {
        const long long n = (long long)pair_offset[p + 1] - pair_offset[p];
        if (n < kMinPoints)
            return apap::fail(APAP_ERR_INVALID_ARG, "%s: pair %d holds %lld matches, a fundamental matrix needs %d", who, p, n, kMinPoints);
    }
    if (iterations < 1 || iterations > (1 << 24) || !(thresh >= 0.0))
        return apap::fail(APAP_ERR_INVALID_ARG, "%s: iterations=%d (1 .. 2^24) thresh=%g (>= 0)", who, iterations, thresh);
    return APAP_OK;
}

}  // namespace apap

extern "C" {

size_t apap_fundamental_workspace_bytes(int n_total, int n_pairs, int iterations) {
    if (n_pairs < 1 || n_pairs > kMaxPairs || iterations < 1 || iterations > (1 << 24) || (long long)n_total < (long long)kMinPoints * n_pairs)
        return 0;
    return fund_layout(n_pairs, iterations).total;
}

int apap_fundamental_batch_device(apap_ctx *ctx, const float *d_src, const float *d_dst, const int *pair_offset, int n_pairs,
                                  double thresh, int iterations, unsigned long long seed, double *d_F, uint8_t *d_mask,
                                  int *d_result, void *d_work, size_t work_bytes, void *stream) {
    const char *who = "apap_fundamental_batch_device";
    int rc = apap::fundamental_check(pair_offset, n_pairs, thresh, iterations, who);
    if (rc) return rc;
    if (!d_src || !d_dst || !d_F || !d_mask || !d_result || !d_work) return apap::fail(APAP_ERR_INVALID_ARG, "%s: null device pointer", who);
    const FundLayout L = fund_layout(n_pairs, iterations);
    if (work_bytes < L.total) return apap::fail(APAP_ERR_WORKSPACE, "%s: workspace %zu < %zu bytes", who, work_bytes, L.total);
    if (((uintptr_t)d_work & 255) != 0 || ((uintptr_t)d_src & 7) != 0 || ((uintptr_t)d_dst & 7) != 0 || ((uintptr_t)d_F & 7) != 0)
        return apap::fail(APAP_ERR_INVALID_ARG, "%s: workspace must be 256-byte, points and F 8-byte aligned", who);
    if (((uintptr_t)d_result & 3) != 0) return apap::fail(APAP_ERR_INVALID_ARG, "%s: d_result must be 4-byte aligned", who);
    hipStream_t s = (hipStream_t)stream;
    char *w = (char *)d_work;
    int *d_offset = (int *)(w + L.table);
    double *d_boxes = (double *)(w + L.boxes), *d_hyps = (double *)(w + L.hyps), *d_winners = (double *)(w + L.winners);
    int *d_counts = (int *)(w + L.counts);
    // from pageable memory in stream order: the copy returns once its source has been consumed
    hipError_t e = hipMemcpyAsync(d_offset, pair_offset, ((size_t)n_pairs + 1) * sizeof(int), hipMemcpyHostToDevice, s);
    if (e != hipSuccess) return apap::hip_fail(e, "apap_fundamental_batch_device: offset upload");
    const double thr2 = thresh * thresh;
    {
        apap::ProfScope prof(ctx, APAP_PROF_RANSAC, s);
        hipLaunchKernelGGL(k_fund_box, dim3(1, n_pairs), dim3(kThreads), 0, s, d_src, d_dst, (const int *)d_offset, d_boxes);
        hipLaunchKernelGGL(k_fund_hyp, dim3((iterations + kHypLanes - 1) / kHypLanes, n_pairs), dim3(kHypLanes), 0, s, d_src, d_dst,
                           (const int *)d_offset, (const double *)d_boxes, iterations, seed, d_hyps);
        // grid.x carries the hypotheses: up to 2^24, within the 2^31 - 1 of that dimension
        hipLaunchKernelGGL(k_fund_score, dim3(iterations, n_pairs), dim3(kThreads), 0, s, d_src, d_dst, (const int *)d_offset,
                           (const double *)d_hyps, iterations, thr2, d_counts);
        hipLaunchKernelGGL(k_fund_select, dim3(1, n_pairs), dim3(kThreads), 0, s, d_src, d_dst, (const int *)d_offset,
                           (const double *)d_hyps, (const int *)d_counts, iterations, thr2, d_winners, d_mask, d_result);
        hipLaunchKernelGGL(k_fund_refit, dim3(1, n_pairs), dim3(kThreads), 0, s, d_src, d_dst, (const int *)d_offset,
                           (const double *)d_boxes, (const uint8_t *)d_mask, (const int *)d_result, d_F);
    }
    e = hipGetLastError();
    if (e != hipSuccess) return apap::hip_fail(e, "apap_fundamental_batch_device launch");
    return APAP_OK;
}

int apap_fundamental_device(apap_ctx *ctx, const float *d_src, const float *d_dst, int n, double thresh, int iterations,
                            unsigned long long seed, double *d_F, uint8_t *d_mask, int *d_result, void *d_work, size_t work_bytes,
                            void *stream) {
    const int off[2] = {0, n};
    return apap_fundamental_batch_device(ctx, d_src, d_dst, off, 1, thresh, iterations, seed, d_F, d_mask, d_result, d_work,
                                         work_bytes, stream);
}

}  // extern "C"
