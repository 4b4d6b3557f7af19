// Device half of the M-step, shared by apap_model.hip (one problem per launch), apap_em_batch.hip (one launch for a batch
// of problems) and apap_local_model.hip (one problem per mesh cell): constants, workspace layout, the interior-point method
// and the bodies of M1, M2 and the Huber kernel, every step that two of them share defined once.  A body takes the index of
// its block within its problem as `bx`; every form runs the same arithmetic in the same order.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "apap_internal.h"

namespace {

constexpr int kW = 64;            // one wave per block
constexpr int kC = 15;            // columns of K
constexpr int kD = 18;            // the LMI's order
constexpr int kDD = kD * kD;
constexpr int kV = 10;            // unknowns of the SDP: h (8), r, t
constexpr int kPair = 24;         // matches per Householder fold (48 rows in lanes 15..62)
constexpr int kMinRounds = 10;    // at least 240 matches per block
constexpr int kMaxBlocks = 1024;
constexpr int kDefaultIters = 80;
constexpr double kGapTol = 1e-10;   // tr(S Z) <= kGapTol (r + t)
constexpr double kRankTol = 1e-12;  // |R_jj| of the equilibrated factor (unit-scale columns) below this: rank-deficient
constexpr double kStep = 0.98;      // fraction of the step to the cone's boundary
constexpr int kBisect = 14;         // bisection steps of the step length

struct ModelLayout {
    int n, per_block, nb;
    size_t R, cnt, total;
};

ModelLayout model_layout(int n) {
    ModelLayout L{};
    L.n = n;
    int rounds = (n + kPair * kMaxBlocks - 1) / (kPair * kMaxBlocks);
    if (rounds < kMinRounds) rounds = kMinRounds;
    L.per_block = rounds * kPair;
    L.nb = (n + L.per_block - 1) / L.per_block;
    L.R = 0;
    L.cnt = L.R + apap::up256((size_t)L.nb * kC * kC * sizeof(double));
    L.total = L.cnt + apap::up256((size_t)L.nb * sizeof(int));
    return L;
}

struct ModelScalars {
    int mode, swap, use_floor, max_iter;
    float du32, dv32;
    double floor, du, dv;
};

// Whether a match of weight `w` takes part (model_solve: `if w <= floor: continue`).  numpy 1.x compares the float32 scalar
// with the Python float in float64, and so does this: float32(1e-3) > 1e-3 is kept.  A NaN weight is dropped.
__device__ __forceinline__ bool model_selected(float w, const ModelScalars &sc) { return !sc.use_floor || (double)w > sc.floor; }

__device__ __forceinline__ double wsum(double v) {
#pragma unroll
    for (int o = kW / 2; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// Householder QR of the wave's 64 x 15 panel (one row per lane), in place: afterwards lanes 0..14 hold R (upper triangular,
// diagonal of either sign) and the other lanes zeros.  Lanes 0..14 enter with an upper triangular R (or zeros).
__device__ __forceinline__ void hh_panel(double (&a)[kC], int lane) {
#pragma unroll
    for (int j = 0; j < kC; ++j) {
        const double x = a[j];
        const double sig = wsum(lane > j ? x * x : 0.0);
        const double x0 = __shfl(x, j);
        if (sig == 0.0) continue;   // wave-uniform: the column is reduced already
        const double mu = sqrt(x0 * x0 + sig);
        const double v0 = x0 <= 0.0 ? x0 - mu : -sig / (x0 + mu);
        const double tau = 2.0 * v0 * v0 / (sig + v0 * v0);
        const double v = lane == j ? 1.0 : (lane > j ? x / v0 : 0.0);
#pragma unroll
        for (int k = j + 1; k < kC; ++k) {
            const double d = wsum(v * a[k]);
            a[k] -= tau * v * d;
        }
        a[j] = lane == j ? mu : (lane > j ? 0.0 : x);
    }
}

// Row 2i + odd of K for match i (model.py:29-35, :77-93; every product rounded as numpy does, -ffp-contract=off):
//   A      even [xc w, yc w, w, 0, 0, 0, (-xo xc) w, (-xo yc) w]   odd [0, 0, 0, xc w, yc w, w, (-yo xc) w, (-yo yc) w]  float32
//   rhs    even xo w, odd yo w                                                                                          float32
//   A1     cols 0 3 6: even (du32 w, 0, (-xo du) w), odd (0, du32 w, (-yo du) w)                                         float64
//   A2     cols 1 4 7: even (dv32 w, 0, (-xo dv) w), odd (0, dv32 w, (-yo dv) w)                                         float64
__device__ __forceinline__ void k_row(double (&a)[kC], float2 c, float2 o, float w, int odd, const ModelScalars &sc) {
    const float p = odd ? o.y : o.x;   // xo or yo
    const float np_ = -p;
    const float r0 = (np_ * c.x) * w, r1 = (np_ * c.y) * w;
    const double wd = (double)w;
    const double diag_u = (double)sc.du32 * wd, diag_v = (double)sc.dv32 * wd;
    const double lu = ((double)np_ * sc.du) * wd, lv = ((double)np_ * sc.dv) * wd;
#pragma unroll
    for (int k = 0; k < kC; ++k) a[k] = 0.0;
    const int o3 = odd ? 3 : 0;
    a[o3 + 0] = (double)(c.x * w);
    a[o3 + 1] = (double)(c.y * w);
    a[o3 + 2] = (double)(1.0f * w);
    a[6] = (double)r0;
    a[7] = (double)r1;
    a[8] = -(double)(p * w);
    a[9] = odd ? 0.0 : diag_u;
    a[10] = odd ? diag_u : 0.0;
    a[11] = lu;
    a[12] = odd ? 0.0 : diag_v;
    a[13] = odd ? diag_v : 0.0;
    a[14] = lv;
}

// ---- M1 ------------------------------------------------------------------------------------------------------------------
// Where a match's float32 weight comes from: `weight(i, pc[i])`.  LoadWeight reads the caller's vector; apap_local_model.hip
// computes a cell's moving-DLT weight on the fly.  The body's arithmetic and summation order do not depend on the source.
struct LoadWeight {
    const float *__restrict__ w;
    __device__ __forceinline__ float operator()(int i, float2) const { return w[i]; }
};

template <class Weight>
__device__ __forceinline__ void model_tsqr_body(const float2 *__restrict__ pc, const float2 *__restrict__ po, const Weight weight,
                                                   int n, int per_block, ModelScalars sc, double *__restrict__ Rb,
                                                   int *__restrict__ cnt, unsigned bx) {
    const int lane = threadIdx.x;
    const int begin = bx * per_block;
    const int end = min(n, begin + per_block);
    double a[kC];
#pragma unroll
    for (int k = 0; k < kC; ++k) a[k] = 0.0;
    int count = 0;
    for (int base = begin; base < end; base += kPair) {
        const int r = lane - kC;
        const int i = base + (r >> 1);
        bool keep = false;
        if (r >= 0 && r < 2 * kPair && i < end) {
            const float2 c = pc[i];
            const float wi = weight(i, c);
            keep = model_selected(wi, sc);
            if (keep) k_row(a, c, po[i], wi, r & 1, sc);
        }
        if (lane >= kC && !keep) {
#pragma unroll
            for (int k = 0; k < kC; ++k) a[k] = 0.0;
        }
        count += __popcll(__ballot(keep && (r & 1) == 0));
        hh_panel(a, lane);
    }
    if (lane < kC) {
        double *row = Rb + ((size_t)bx * kC + lane) * kC;
#pragma unroll
        for (int k = 0; k < kC; ++k) row[k] = a[k];
    }
    if (lane == 0) cnt[bx] = count;
}

// ---- M2: LDS helpers (one wave; every helper ends with a barrier) ---------------------------------------------------------
struct Lds {
    double F[kV + 1][kDD];   // F0 and the ten basis matrices of S(x) = F0 + sum x_i F_i
    double S[kDD], Z[kDD], Si[kDD], T[kDD], W1[kDD], W2[kDD], dSa[kDD], dZa[kDD], C[kDD];
    double R[kC * kC];
    double M[kV * kV], Mc[kV * kV], x[kV], dx[kV], g[kV], rhs[kV], best_x[kV], best_z[9];
    double d[kC];
    int flag;
};

__device__ __forceinline__ void mm(double *C, const double *A, const double *B, int lane) {   // C = A B
    for (int e = lane; e < kDD; e += kW) {
        const int i = e / kD, j = e % kD;
        double s = 0.0;
        for (int k = 0; k < kD; ++k) s += A[i * kD + k] * B[k * kD + j];
        C[e] = s;
    }
    __syncthreads();
}

__device__ __forceinline__ double dot_dd(const double *A, const double *B, int lane) {   // sum A o B (wave-uniform)
    double s = 0.0;
    for (int e = lane; e < kDD; e += kW) s += A[e] * B[e];
    return wsum(s);
}

__device__ __forceinline__ double dot_dt(const double *A, const double *B, int lane) {   // sum A o B^T
    double s = 0.0;
    for (int e = lane; e < kDD; e += kW) s += A[e] * B[(e % kD) * kD + e / kD];
    return wsum(s);
}

// In-place Cholesky of the 18 x 18 A (lower triangle); false (wave-uniform) when A is not positive definite.
__device__ bool chol18(double *A, int lane) {
    for (int k = 0; k < kD; ++k) {
        const double p = A[k * kD + k];
        if (!(p > 0.0)) {
            __syncthreads();
            return false;
        }
        const double d = sqrt(p);
        __syncthreads();
        for (int i = k + 1 + lane; i < kD; i += kW) A[i * kD + k] /= d;
        if (lane == 0) A[k * kD + k] = d;
        __syncthreads();
        const int m = kD - k - 1;
        for (int e = lane; e < m * m; e += kW) {
            const int i = k + 1 + e / m, j = k + 1 + e % m;
            if (j <= i) A[i * kD + j] -= A[i * kD + k] * A[j * kD + k];
        }
        __syncthreads();
    }
    return true;
}

// The step length: 1 when A + dA / kStep is positive definite, else kStep x the largest feasible point of a kBisect-step
// bisection of [0, 1 / kStep] (tests/model_spec.py: max_step).
__device__ double max_step(const double *A, const double *dA, double *T, int lane) {
    auto ok = [&](double a) {
        for (int e = lane; e < kDD; e += kW) T[e] = A[e] + a * dA[e];
        __syncthreads();
        return chol18(T, lane);
    };
    double hi = 1.0 / kStep;
    if (ok(hi)) return 1.0;
    double lo = 0.0;
    for (int b = 0; b < kBisect; ++b) {
        const double mid = 0.5 * (lo + hi);
        if (ok(mid)) lo = mid;
        else hi = mid;
    }
    return kStep * lo;
}

// Si = S^-1 through the Cholesky factor in T (T = L L^T on entry): W2 = L^-1 by columns, Si = W2^T W2.
__device__ void inverse_from_chol(const double *T, double *W2, double *Si, int lane) {
    if (lane < kD) {
        const int c = lane;
        for (int i = 0; i < kD; ++i) {
            double s = i == c ? 1.0 : 0.0;
            for (int k = c; k < i; ++k) s -= T[i * kD + k] * W2[k * kD + c];
            W2[i * kD + c] = i < c ? 0.0 : s / T[i * kD + i];
        }
    }
    __syncthreads();
    for (int e = lane; e < kDD; e += kW) {
        const int a = e / kD, b = e % kD;
        double s = 0.0;
        for (int k = 0; k < kD; ++k) s += W2[k * kD + a] * W2[k * kD + b];
        Si[e] = s;
    }
    __syncthreads();
}

// Serial Cholesky solve of the N x N system M x = b on one thread: M = L L^T in place (row-major, the lower triangle is read
// and overwritten), L y = b, L^T x = y.  b and y may be the same array.  One operation order for every caller: pivot
// p = M[kk] - sum M[kj]^2, column (M[ik] - sum M[ij] M[kj]) / d.  `reject(p)` is the caller's test of a pivot: at the
// first rejected one the factorisation stops, x is left as it was and the result is false.  The factor loop is unrolled by
// name: rolled, as the compiler leaves it at N = 8, the Huber call measured 10 - 20 us (3 - 5 %) slower.
template <int N, class Reject>
__device__ __forceinline__ bool chol_solve(double *M, const double *b, double *y, double *x, Reject reject) {
    bool good = true;
#pragma unroll
    for (int k = 0; k < N && good; ++k) {
        double p = M[k * N + k];
        for (int j = 0; j < k; ++j) p -= M[k * N + j] * M[k * N + j];
        if (reject(p)) good = false;
        const double d = sqrt(p);
        M[k * N + k] = d;
        for (int i = k + 1; i < N; ++i) {
            double s = M[i * N + k];
            for (int j = 0; j < k; ++j) s -= M[i * N + j] * M[k * N + j];
            M[i * N + k] = s / d;
        }
    }
    if (good) {
        for (int i = 0; i < N; ++i) {
            double s = b[i];
            for (int j = 0; j < i; ++j) s -= M[i * N + j] * y[j];
            y[i] = s / M[i * N + i];
        }
        for (int i = N - 1; i >= 0; --i) {
            double s = y[i];
            for (int j = i + 1; j < N; ++j) s -= M[j * N + i] * x[j];
            x[i] = s / M[i * N + i];
        }
    }
    return good;
}

// 10 x 10 Cholesky solve of M dx = rhs on lane 0 (M in L.M, overwritten); dx to L.dx.  false: M not positive definite.  The
// only test is the pivot's sign: a stricter one would change which iterate an SDP that leaves the cone returns.  Forced
// inline: left to the compiler, the two calls in ipm() become calls of one out-of-line function.
__device__ __forceinline__ bool schur_solve(Lds &L, int lane) {
    if (lane == 0) {
        double y[kV];
        L.flag = chol_solve<kV>(L.M, L.rhs, y, L.dx, [](double p) { return !(p > 0.0); });
    }
    __syncthreads();
    return L.flag != 0;
}

// dS = sum dx_i F_i;  dZ = sym(E - Z - Si dS Z), E = extra_si x Si - (C if with_c).  W1 = Si dS on return.
__device__ void directions(Lds &L, double *dS, double *dZ, double extra_si, bool with_c, int lane) {
    for (int e = lane; e < kDD; e += kW) {
        double s = 0.0;
        for (int i = 0; i < kV; ++i) s += L.dx[i] * L.F[i + 1][e];
        dS[e] = s;
    }
    __syncthreads();
    mm(L.W1, L.Si, dS, lane);
    mm(L.W2, L.W1, L.Z, lane);
    for (int e = lane; e < kDD; e += kW) {
        const int a = e / kD, b = e % kD, et = b * kD + a;
        const double v1 = extra_si * L.Si[e] - (with_c ? L.C[e] : 0.0) - L.Z[e] - L.W2[e];
        const double v2 = extra_si * L.Si[et] - (with_c ? L.C[et] : 0.0) - L.Z[et] - L.W2[et];
        dZ[e] = 0.5 * (v1 + v2);
    }
    __syncthreads();
}

// The interior-point method (tests/model_spec.py: ipm) on the equilibrated R in L.R, from h0 in L.x[0..7].  Leaves the
// best iterate in L.best_x / L.best_z; returns (relative gap, iterations) through the references.
__device__ void ipm(Lds &L, int lane, int max_iter, double &best_rel, int &iters) {
    // the basis: F0 = [[I, R[:, 8] in column q]], F_{1+j} = R[:, j] in column q, plus A1 / A2's columns in u / v
    for (int e = lane; e < (kV + 1) * kDD; e += kW) (&L.F[0][0])[e] = 0.0;
    __syncthreads();
    if (lane < kC) {
        const int r = lane;
        auto put = [&](int k, int col, double v) {
            L.F[k][r * kD + kC + col] += v;
            L.F[k][(kC + col) * kD + r] += v;
        };
        L.F[0][r * kD + r] = 1.0;
        put(0, 2, L.R[r * kC + 8]);
        for (int j = 0; j < 8; ++j) {
            put(j + 1, 2, L.R[r * kC + j]);
            if (j % 3 == 0) put(j + 1, 0, L.R[r * kC + 9 + j / 3]);
            if (j % 3 == 1) put(j + 1, 1, L.R[r * kC + 12 + j / 3]);
        }
    }
    if (lane == 0) {
        L.F[9][15 * kD + 15] = L.F[9][16 * kD + 16] = 1.0;
        L.F[10][17 * kD + 17] = 1.0;
    }
    __syncthreads();
    // start: tau = 2 tr(G(h0)) + 1e-12, G = (R X)^T (R X); x = (h0, tau, tau), Z = diag(tau / 2 I_15, 1/2, 1/2, 1)
    double g_uu = 0.0, g_vv = 0.0, g_qq = 0.0;
    if (lane < kC) {
        const int r = lane;
        const double *Rr = L.R + r * kC;
        double u = 0.0, v = 0.0, q = Rr[8];
        for (int m = 0; m < 3; ++m) {
            u += Rr[9 + m] * L.x[3 * m];
            v += Rr[12 + m] * L.x[3 * m + 1];
        }
        for (int j = 0; j < 8; ++j) q += Rr[j] * L.x[j];
        g_uu = u * u;
        g_vv = v * v;
        g_qq = q * q;
    }
    const double tau = 2.0 * (wsum(g_uu) + wsum(g_vv) + wsum(g_qq)) + 1e-12;
    __syncthreads();
    if (lane == 0) L.x[8] = L.x[9] = tau;
    for (int e = lane; e < kDD; e += kW) {
        const int a = e / kD, b = e % kD;
        L.Z[e] = a != b ? 0.0 : a < kC ? 0.5 * tau : a < 17 ? 0.5 : 1.0;
    }
    __syncthreads();
    best_rel = INFINITY;
    iters = 0;
    for (int it = 0;; ++it) {
        for (int e = lane; e < kDD; e += kW) {
            double s = L.F[0][e];
            for (int i = 0; i < kV; ++i) s += L.x[i] * L.F[i + 1][e];
            L.S[e] = s;
        }
        __syncthreads();
        const double gap_abs = dot_dd(L.S, L.Z, lane);
        const double obj = L.x[8] + L.x[9];
        const double rel = gap_abs / fmax(obj, 1e-300);
        if (rel < best_rel) {   // wave-uniform
            best_rel = rel;
            iters = it;
            if (lane < kV) L.best_x[lane] = L.x[lane];
            if (lane < 9) L.best_z[lane] = L.Z[(kC + lane / 3) * kD + kC + lane % 3];
        }
        iters = it;
        if (rel <= kGapTol || it == max_iter) break;
        const double mu = gap_abs / kD;
        // S^-1
        for (int e = lane; e < kDD; e += kW) L.T[e] = L.S[e];
        __syncthreads();
        if (!chol18(L.T, lane)) break;   // rounding pushed S out of the cone: keep the best iterate
        inverse_from_chol(L.T, L.W2, L.Si, lane);
        // Schur complement M_ij = tr(F_i S^-1 F_j Z) and g_i = tr(S^-1 F_i)
        for (int j = 0; j < kV; ++j) {
            mm(L.W1, L.Si, L.F[j + 1], lane);
            mm(L.W2, L.W1, L.Z, lane);
            for (int i = 0; i < kV; ++i) {
                const double m = dot_dt(L.F[i + 1], L.W2, lane);
                if (lane == 0) L.M[i * kV + j] = m;
            }
        }
        for (int i = 0; i < kV; ++i) {
            const double gi = dot_dd(L.Si, L.F[i + 1], lane);
            if (lane == 0) {
                L.g[i] = gi;
                L.rhs[i] = i < 8 ? 0.0 : -1.0;   // predictor: -c
            }
        }
        __syncthreads();
        for (int e = lane; e < kV * kV; e += kW) L.Mc[e] = L.M[e];   // the corrector solves with M again
        __syncthreads();
        if (!schur_solve(L, lane)) break;
        directions(L, L.dSa, L.dZa, 0.0, false, lane);
        // C = S^-1 dSa dZa (W1 = S^-1 dSa)
        mm(L.C, L.W1, L.dZa, lane);
        const double ap = max_step(L.S, L.dSa, L.T, lane);
        const double ad = max_step(L.Z, L.dZa, L.T, lane);
        double s = 0.0;
        for (int e = lane; e < kDD; e += kW) s += (L.S[e] + ap * L.dSa[e]) * (L.Z[e] + ad * L.dZa[e]);
        const double mu_aff = wsum(s) / kD;
        const double ratio = mu_aff / mu;
        const double sig = fmin(1.0, ratio * ratio * ratio);
        // corrector: M dx = sig mu g - c - tr(F_i C)
        for (int e = lane; e < kV * kV; e += kW) L.M[e] = L.Mc[e];
        for (int i = 0; i < kV; ++i) {
            const double fc = dot_dt(L.F[i + 1], L.C, lane);
            if (lane == 0) L.rhs[i] = sig * mu * L.g[i] - (i < 8 ? 0.0 : 1.0) - fc;
        }
        __syncthreads();
        if (!schur_solve(L, lane)) break;
        directions(L, L.dSa, L.dZa, sig * mu, true, lane);   // dS, dZ reuse the predictor's buffers
        const double bp = max_step(L.S, L.dSa, L.T, lane);
        const double bd = max_step(L.Z, L.dZa, L.T, lane);
        if (lane < kV) L.x[lane] += bp * L.dx[lane];
        for (int e = lane; e < kDD; e += kW) L.Z[e] += bd * L.dZa[e];
        __syncthreads();
    }
}

// ---- M2 ------------------------------------------------------------------------------------------------------------------
// The power of two nearest x on a log scale: x = m 2^e, m in [1/2, 1) -> 2^e if m >= sqrt(1/2), else 2^(e-1); 1 for 0 / inf
// / NaN (tests/model_spec.py: pow2_near).
__device__ __forceinline__ double pow2_near(double x) {
    if (!(x > 0.0) || isinf(x)) return 1.0;
    int e;
    const double m = frexp(x, &e);
    return ldexp(1.0, m >= 0.70710678118654752440 ? e : e - 1);
}

// The tail of M2 and of the Huber kernel (model.py:50-56): float32 solution, [2, 2] = 1; with `invert` numpy.linalg.inv
// (fp64 LU, cast back) and / [2, 2] in float32.  ORs APAP_STATUS_SINGULAR into `word` when the inverse meets a zero pivot.
__device__ __forceinline__ void model_tail(const double (&h)[8], bool invert, float (&sol)[9], int &word) {
    for (int k = 0; k < 8; ++k) sol[k] = (float)h[k];
    sol[8] = 1.0f;
    if (invert) {
        double m[9], r[9];
        for (int k = 0; k < 9; ++k) m[k] = (double)sol[k];
        if (!apap::inv3(m, r)) word |= APAP_STATUS_SINGULAR;
        float q[9];
        for (int k = 0; k < 9; ++k) q[k] = (float)r[k];
        const float d = q[8];
        for (int k = 0; k < 9; ++k) sol[k] = q[k] / d;
    }
}

__device__ __forceinline__ void model_solve_body(const double *__restrict__ Rb, const int *__restrict__ cnt, int nb,
                                                    ModelScalars sc, float *__restrict__ H, double *__restrict__ info,
                                                    int *__restrict__ status) {
    __shared__ Lds L;
    const int lane = threadIdx.x;
    // fold the block factors, three per pass, in block order
    double a[kC];
#pragma unroll
    for (int k = 0; k < kC; ++k) a[k] = 0.0;
    for (int base = 0; base < nb; base += 3) {
        const int r = lane - kC;
        const int b = base + r / kC;
        const bool live = r >= 0 && r < 3 * kC && b < nb;
        if (lane >= kC) {
#pragma unroll
            for (int k = 0; k < kC; ++k) a[k] = live ? Rb[((size_t)b * kC + r % kC) * kC + k] : 0.0;
        }
        hh_panel(a, lane);
    }
    if (lane < kC) {
#pragma unroll
        for (int k = 0; k < kC; ++k) L.R[lane * kC + k] = a[k];
    }
    int count = 0;
    if (lane == 0)
        for (int b = 0; b < nb; ++b) count += cnt[b];
    count = __shfl(count, 0);
    __syncthreads();
    // signs (diagonal >= 0), column norms, power-of-two equilibration
    if (lane < kC && L.R[lane * kC + lane] < 0.0)
        for (int k = 0; k < kC; ++k) L.R[lane * kC + k] = -L.R[lane * kC + k];
    __syncthreads();
    if (lane < kC) {
        double s = 0.0;
        for (int r = 0; r < kC; ++r) s += L.R[r * kC + lane] * L.R[r * kC + lane];
        L.d[lane] = sqrt(s);
    }
    __syncthreads();
    double dsc = 1.0;   // this lane's column scale
    if (lane < kC) {
        const int c = lane;
        const int hj = c < 8 ? c : c == 8 ? -1 : c < 12 ? 3 * (c - 9) : 3 * (c - 12) + 1;
        dsc = hj < 0 ? 1.0 / pow2_near(L.d[8]) : 1.0 / pow2_near(L.d[hj]);
    }
    __syncthreads();
    if (lane < kC) {
        for (int r = 0; r < kC; ++r) L.R[r * kC + lane] *= dsc;
        L.d[lane] = dsc;   // s_j for j < 8, 1 / sigma at 8
    }
    __syncthreads();
    const double sigma = 1.0 / L.d[8];
    bool degenerate = count < 4;
    for (int j = 0; j < 8; ++j) degenerate = degenerate || !(fabs(L.R[j * kC + j]) > kRankTol);
    int word = degenerate ? APAP_STATUS_MODEL_DEGENERATE : 0;
    double hq[8];   // h'' (equilibrated)
    double objective = NAN, r_out = NAN, t_out = NAN, gap = 0.0;
    int iters = 0;
    if (!degenerate) {
        // LMS: R[0:8, 0:8] h'' = -R[0:8, 8]
        for (int i = 7; i >= 0; --i) {
            double s = -L.R[i * kC + 8];
            for (int k = i + 1; k < 8; ++k) s -= L.R[i * kC + k] * hq[k];
            hq[i] = s / L.R[i * kC + i];
        }
        objective = sigma * sigma * (L.R[8 * kC + 8] * L.R[8 * kC + 8]);
        if (sc.mode == APAP_MODEL_SDP) {
            if (lane < 8) L.x[lane] = hq[lane];
            __syncthreads();
            double rel;
            ipm(L, lane, sc.max_iter, rel, iters);
            __syncthreads();   // the loop may leave right after lanes 0..9 wrote best_x / best_z
            for (int k = 0; k < 8; ++k) hq[k] = L.best_x[k];
            r_out = sigma * sigma * L.best_x[8];
            t_out = sigma * sigma * L.best_x[9];
            objective = r_out + t_out;
            gap = rel;
            if (!(rel <= kGapTol)) word |= APAP_STATUS_MODEL_NO_CONVERGENCE;
        }
    }
    if (lane != 0) return;
    double h[8];
    for (int k = 0; k < 8; ++k) h[k] = degenerate ? NAN : sigma * L.d[k] * hq[k];
    float sol[9];
    model_tail(h, sc.swap && !degenerate, sol, word);
    for (int k = 0; k < 9; ++k) H[k] = degenerate ? NAN : sol[k];
    info[APAP_MODEL_INFO_OBJECTIVE] = objective;
    info[APAP_MODEL_INFO_R] = r_out;
    info[APAP_MODEL_INFO_T] = t_out;
    info[APAP_MODEL_INFO_GAP] = gap;
    info[APAP_MODEL_INFO_ITERS] = (double)iters;
    info[APAP_MODEL_INFO_STATUS] = (double)word;
    info[APAP_MODEL_INFO_COUNT] = (double)count;
    for (int k = 0; k < 9; ++k)
        info[APAP_MODEL_INFO_Z + k] = (sc.mode == APAP_MODEL_SDP && !degenerate) ? L.best_z[k] : NAN;
    for (int k = 0; k < 8; ++k) info[APAP_MODEL_INFO_H + k] = h[k];
    if (word && status) atomicOr(status, word);
}

// ---- Huber M-step (include/apap_hip.h; tests/huber_spec.py is the numpy specification) --------------------------------------
// One workgroup per problem, after M1 and M2 ran in LMS mode: the rows (k_row's columns 0..8) are regenerated from pc, po, w
// on every pass, match i always by thread i mod kHuberThreads in ascending order; a pass's sums are per-thread fp64
// accumulations, one butterfly per wave and the waves' partial sums added in wave order by thread 0, which also does the
// 8 x 8 work in LDS.  Unknowns are equilibrated: h'' = h / s, s_k = 1 / pow2_near(column norm), exact powers of two.
constexpr int kHuberThreads = APAP_MODEL_HUBER_THREADS;
constexpr int kHuberWaves = kHuberThreads / kW;
constexpr int kHuberDefaultIters = 100;   // accepted steps (DESIGN.md "Huber M-step" has the counts behind it)
constexpr int kHuberHalvings = 11;        // alpha = 1, 1/2, .., 2^-10
constexpr int kHuberMaxN = 1 << 20;
constexpr int kHuberAcc = 46;             // 36 Gram entries, 8 of the right-hand side, f, the clipped count

enum { kHuberNewton = 0, kHuberMajorise = 1, kHuberDual = 2 };

struct HuberLds {
    double part[kHuberWaves][kHuberAcc];
    double tot[kHuberAcc];
    double G[64], y[8];
    double s[8], h[8], d[8];
    double f;
    int nclip, ok, move;
};

// Row 2 i + odd of the scaled A, and rhs, of match i.
__device__ __forceinline__ void huber_row(double (&as)[8], double &rhs, float2 c, float2 o, float w, int odd, const ModelScalars &sc,
                                          const double (&s)[8]) {
    double a[kC];
    k_row(a, c, o, w, odd, sc);
#pragma unroll
    for (int k = 0; k < 8; ++k) as[k] = a[k] * s[k];
    rhs = -a[8];
}

__device__ __forceinline__ double huber_dot(const double (&as)[8], const double (&v)[8]) {
    double r = as[0] * v[0];
#pragma unroll
    for (int k = 1; k < 8; ++k) r += as[k] * v[k];
    return r;
}

// The residual of a row at h.
__device__ __forceinline__ double huber_residual(const double (&as)[8], const double (&h)[8], double rhs) {
    return huber_dot(as, h) - rhs;
}

// phi_M(r): r^2 within [-M, M], 2 M |r| - M^2 beyond.
__device__ __forceinline__ double huber_phi(double r, double M) {
    const double ar = fabs(r);
    return ar > M ? 2.0 * M * ar - M * M : r * r;
}

// The walk of every pass: f(as, rhs) for row 2 i + odd (scaled by s) of every selected match i = tid, tid + kHuberThreads, ..
// in ascending order, even row first.  Which matches a thread sums, and in which order, is what makes every entry form give
// the same bytes: it is decided here and nowhere else.  `f` captures the caller's accumulators by reference; all of this
// is inlined, so they stay in registers.
template <class F>
__device__ __forceinline__ void huber_rows(const float2 *__restrict__ pc, const float2 *__restrict__ po, const float *__restrict__ w,
                                           int n, const ModelScalars &sc, const double (&s)[8], int tid, F f) {
    for (int i = tid; i < n; i += kHuberThreads) {
        const float wi = w[i];
        if (!model_selected(wi, sc)) continue;
        const float2 c = pc[i], o = po[i];
#pragma unroll
        for (int odd = 0; odd < 2; ++odd) {
            double as[8], rhs;
            huber_row(as, rhs, c, o, wi, odd, sc, s);
            f(as, rhs);
        }
    }
}

// The sums of `acc` over the workgroup into L.tot (valid on thread 0 only, which goes on to use them; the caller ends the
// step with a barrier).
template <int K>
__device__ __forceinline__ void huber_reduce(double (&acc)[K], HuberLds &L, int tid) {
#pragma unroll
    for (int k = 0; k < K; ++k) acc[k] = wsum(acc[k]);
    if ((tid & (kW - 1)) == 0) {
#pragma unroll
        for (int k = 0; k < K; ++k) L.part[tid / kW][k] = acc[k];
    }
    __syncthreads();
    if (tid == 0) {
        for (int k = 0; k < K; ++k) {
            double t = L.part[0][k];
            for (int v = 1; v < kHuberWaves; ++v) t += L.part[v][k];
            L.tot[k] = t;
        }
    }
}

// Thread 0: L.d = G^-1 b for the packed upper triangle in L.tot[0..35] by Cholesky; false when G is not positive definite.
__device__ bool huber_chol_solve(HuberLds &L, double sign) {
    double *G = L.G;
    int e = 0;
    for (int k = 0; k < 8; ++k)
        for (int l = k; l < 8; ++l, ++e) G[k * 8 + l] = G[l * 8 + k] = L.tot[e];
    for (int i = 0; i < 8; ++i) L.y[i] = sign * L.tot[36 + i];
    // besides the sign, an infinite pivot (an overflowed Gram entry) and a non-finite solution are refused
    if (!chol_solve<8>(G, L.y, L.y, L.d, [](double p) { return !(p > 0.0) || isinf(p); })) return false;
    for (int i = 0; i < 8; ++i)
        if (!isfinite(L.d[i])) return false;
    return true;
}

// One pass at L.h: f, the clipped count, and G d = b solved into L.d (L.ok):
//   kHuberNewton    G = sum of a a^T over the unclipped rows, b = -(sum a r over them + M sum sign(r) a over the clipped)
//   kHuberMajorise  G = sum omega a a^T, b = -sum omega a r, omega = min(1, M / |r|) over all rows
//   kHuberDual      G = A^T A, b = A^T y, y = 2 clip(r, -M, M)
__device__ __forceinline__ void huber_pass_gram(const float2 *__restrict__ pc, const float2 *__restrict__ po,
                                                const float *__restrict__ w, int n, const ModelScalars &sc, HuberLds &L, int tid,
                                                int kind) {
    const double M = sc.du;
    double s[8], h[8], acc[kHuberAcc];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        s[k] = L.s[k];
        h[k] = L.h[k];
    }
#pragma unroll
    for (int k = 0; k < kHuberAcc; ++k) acc[k] = 0.0;
    huber_rows(pc, po, w, n, sc, s, tid, [&](const double (&as)[8], double rhs) {
        const double r = huber_residual(as, h, rhs);
        const double ar = fabs(r);
        const bool clipped = ar > M;
        const double sg = r > 0.0 ? M : -M;
        double omega, coef;
        if (kind == kHuberMajorise) {
            omega = clipped ? M / ar : 1.0;
            coef = omega * r;
        } else if (kind == kHuberDual) {
            // y = 2 clip(r, -M, M).  Not the gap walk's fmin / fmax spelling: the two differ at a NaN residual (NaN here,
            // -2 M there), so each keeps its own.
            omega = 1.0;
            coef = clipped ? 2.0 * sg : 2.0 * r;
        } else {
            omega = clipped ? 0.0 : 1.0;
            coef = clipped ? sg : r;
        }
        int e = 0;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const double t = omega * as[k];
#pragma unroll
            for (int l = k; l < 8; ++l, ++e) acc[e] += t * as[l];
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) acc[36 + k] += as[k] * coef;
        acc[44] += huber_phi(r, M);
        acc[45] += clipped ? 1.0 : 0.0;
    });
    huber_reduce(acc, L, tid);
    if (tid == 0) {
        L.f = L.tot[44];
        L.nclip = (int)L.tot[45];
        L.ok = huber_chol_solve(L, kind == kHuberDual ? 1.0 : -1.0);
    }
    __syncthreads();
}

// f(L.h + alpha L.d) for the kHuberHalvings step lengths and whether the clipped set at alpha = 1 is the one at L.h.  Thread 0
// then moves L.h: L.move = 2 when `newton` and the full step keeps the clipped set without raising f (the minimiser of the
// piece is the minimiser of f), 1 for the step length of the smallest f below L.f (the largest among equals), 0 for none.
__device__ __forceinline__ void huber_pass_line(const float2 *__restrict__ pc, const float2 *__restrict__ po,
                                                const float *__restrict__ w, int n, const ModelScalars &sc, HuberLds &L, int tid,
                                                bool newton) {
    const double M = sc.du;
    double s[8], h[8], d[8], acc[kHuberHalvings + 1];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        s[k] = L.s[k];
        h[k] = L.h[k];
        d[k] = L.d[k];
    }
#pragma unroll
    for (int k = 0; k <= kHuberHalvings; ++k) acc[k] = 0.0;
    huber_rows(pc, po, w, n, sc, s, tid, [&](const double (&as)[8], double rhs) {
        const double r = huber_residual(as, h, rhs);
        const double ad = huber_dot(as, d);
        double alpha = 1.0;
#pragma unroll
        for (int j = 0; j < kHuberHalvings; ++j, alpha *= 0.5) acc[j] += huber_phi(r + alpha * ad, M);
        const double r1 = r + ad;
        const int s0 = r > M ? 1 : (r < -M ? -1 : 0), s1 = r1 > M ? 1 : (r1 < -M ? -1 : 0);
        acc[kHuberHalvings] += s0 != s1 ? 1.0 : 0.0;
    });
    huber_reduce(acc, L, tid);
    if (tid == 0) {
        if (newton && L.tot[kHuberHalvings] == 0.0 && L.tot[0] <= L.f) {
            for (int k = 0; k < 8; ++k) L.h[k] += L.d[k];
            L.move = 2;
        } else {
            int best = 0;
            for (int j = 1; j < kHuberHalvings; ++j)
                if (L.tot[j] < L.tot[best]) best = j;
            if (L.tot[best] < L.f) {
                const double alpha = ldexp(1.0, -best);
                for (int k = 0; k < 8; ++k) L.h[k] += alpha * L.d[k];
                L.move = 1;
            } else {
                L.move = 0;
            }
        }
    }
    __syncthreads();
}

__device__ __forceinline__ void model_huber_body(const float2 *__restrict__ pc, const float2 *__restrict__ po,
                                                 const float *__restrict__ w, int n, ModelScalars sc, float *__restrict__ H,
                                                 double *__restrict__ info, int *__restrict__ status) {
    __shared__ HuberLds L;
    const int tid = threadIdx.x;
    const double M = sc.du;
    const int word0 = (int)info[APAP_MODEL_INFO_STATUS];   // M2's, in LMS mode (workgroup-uniform)
    if (word0 & APAP_STATUS_MODEL_DEGENERATE) {            // LMS's outputs stay
        if (tid == 0 && status) atomicOr(status, word0);
        return;
    }
    // column norms -> scales; h'' = h0 / s
    {
        double acc[8], one[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            acc[k] = 0.0;
            one[k] = 1.0;
        }
        huber_rows(pc, po, w, n, sc, one, tid, [&](const double (&a)[8], double) {
#pragma unroll
            for (int k = 0; k < 8; ++k) acc[k] += a[k] * a[k];
        });
        huber_reduce(acc, L, tid);
        if (tid == 0) {
            for (int k = 0; k < 8; ++k) {
                const double p = pow2_near(sqrt(L.tot[k]));
                L.s[k] = 1.0 / p;
                L.h[k] = info[APAP_MODEL_INFO_H + k] * p;
            }
        }
        __syncthreads();
    }
    int iters = 0;
    bool untouched = false;
    for (bool first = true;; first = false) {
        huber_pass_gram(pc, po, w, n, sc, L, tid, kHuberNewton);
        if (first && L.nclip == 0) {
            untouched = true;
            break;
        }
        if (iters == sc.max_iter) break;
        int move = 0;
        if (L.ok) {
            huber_pass_line(pc, po, w, n, sc, L, tid, true);
            move = L.move;
        }
        if (move == 0) {   // no Newton point, or no step length along it lowers f: one majorise-minimise step
            huber_pass_gram(pc, po, w, n, sc, L, tid, kHuberMajorise);
            if (!L.ok) break;
            huber_pass_line(pc, po, w, n, sc, L, tid, false);
            move = L.move;
            if (move == 0) break;
        }
        ++iters;
        if (move == 2) break;
    }
    // the gap of L.h: z = (A^T A)^-1 A^T y into L.d, then y' = y - A z
    huber_pass_gram(pc, po, w, n, sc, L, tid, kHuberDual);
    const double f = L.f;
    double gap = 0.0;
    if (f != 0.0) {   // workgroup-uniform
        double s[8], h[8], z[8], acc[2] = {0.0, 0.0}, big = 0.0;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            s[k] = L.s[k];
            h[k] = L.h[k];
            z[k] = L.d[k];
        }
        huber_rows(pc, po, w, n, sc, s, tid, [&](const double (&as)[8], double rhs) {
            const double r = huber_residual(as, h, rhs);
            const double y = 2.0 * fmin(fmax(r, -M), M);   // -2 M at a NaN residual (huber_pass_gram's spelling gives NaN)
            const double yp = y - huber_dot(as, z);
            acc[0] += yp * yp;
            acc[1] += rhs * yp;
            big = fmax(big, fabs(yp));
        });
#pragma unroll
        for (int o = kW / 2; o > 0; o >>= 1) big = fmax(big, __shfl_xor(big, o));
        if ((tid & (kW - 1)) == 0) L.part[tid / kW][2] = big;
        huber_reduce(acc, L, tid);
        if (tid == 0) {
            for (int v = 1; v < kHuberWaves; ++v) big = fmax(big, L.part[v][2]);
            const double theta = big > 0.0 ? fmin(1.0, 2.0 * M / big) : 1.0;
            const double D = -theta * theta * L.tot[0] / 4.0 - theta * L.tot[1];
            gap = L.ok ? (f - D) / f : INFINITY;
            if (!(gap == gap)) gap = INFINITY;
        }
    }
    if (tid != 0) return;
    int word = untouched ? word0 : 0;
    if (!untouched) {
        double h[8];
        for (int k = 0; k < 8; ++k) h[k] = L.s[k] * L.h[k];
        float sol[9];
        model_tail(h, sc.swap != 0, sol, word);
        for (int k = 0; k < 9; ++k) H[k] = sol[k];
        for (int k = 0; k < 8; ++k) info[APAP_MODEL_INFO_H + k] = h[k];
    }
    if (!(gap <= kGapTol)) word |= APAP_STATUS_MODEL_NO_CONVERGENCE;
    info[APAP_MODEL_INFO_OBJECTIVE] = f;
    info[APAP_MODEL_INFO_GAP] = gap;
    info[APAP_MODEL_INFO_ITERS] = (double)iters;
    info[APAP_MODEL_INFO_STATUS] = (double)word;
    if (word && status) atomicOr(status, word);
}

int model_check_params(const double *params, ModelScalars *sc, const char *who) {
    if (!params) return apap::fail(APAP_ERR_INVALID_ARG, "%s: null params", who);
    const double mode = params[APAP_MODEL_MODE], swap = params[APAP_MODEL_SWAP], it = params[APAP_MODEL_MAX_ITER];
    if (mode != APAP_MODEL_LMS && mode != APAP_MODEL_SDP && mode != APAP_MODEL_HUBER)
        return apap::fail(APAP_ERR_INVALID_ARG, "%s: mode %g (0 = LMS, 1 = SDP, 2 = Huber)", who, mode);
    if (swap != 0.0 && swap != 1.0) return apap::fail(APAP_ERR_INVALID_ARG, "%s: swap %g (0 or 1)", who, swap);
    if (!(it >= 0.0 && it <= 10000.0)) return apap::fail(APAP_ERR_INVALID_ARG, "%s: max_iter %g out of range", who, it);
    const double du = params[APAP_MODEL_DU], dv = params[APAP_MODEL_DV], fl = params[APAP_MODEL_FLOOR];
    if (!std::isfinite(du) || !std::isfinite(dv)) return apap::fail(APAP_ERR_INVALID_ARG, "%s: du / dv not finite", who);
    if (std::isnan(fl)) return apap::fail(APAP_ERR_INVALID_ARG, "%s: weight floor is NaN", who);
    if (mode == APAP_MODEL_HUBER && !(du > 1e-2))   // model.py:36: huber_param > 1e-2 selects the Huber loss
        return apap::fail(APAP_ERR_INVALID_ARG, "%s: Huber M %g (need a finite M > 1e-2)", who, du);
    sc->mode = (int)mode;
    sc->swap = (int)swap;
    sc->max_iter = it != 0.0 ? (int)it : mode == APAP_MODEL_HUBER ? kHuberDefaultIters : kDefaultIters;
    sc->use_floor = fl != -INFINITY;
    sc->floor = fl;
    sc->du = du;
    sc->dv = dv;
    sc->du32 = (float)du;   // np.float32([[self.du, 0]]) (model.py:85)
    sc->dv32 = (float)dv;
    return APAP_OK;
}

// The Huber M-step exists for one problem per call (apap_model.hip): `n` is that call's match count, or -1 from the entry
// points that have no Huber kernel (the batch, the per-cell solve), which refuse the mode by name.
int model_check_huber(const ModelScalars &sc, int n, const char *who) {
    if (sc.mode != APAP_MODEL_HUBER) return APAP_OK;
    if (n < 0)
        return apap::fail(APAP_ERR_INVALID_ARG, "%s: the Huber M-step (mode 2) is not available here: use apap_model_solve or "
                                                "apap_spectral_em", who);
    if (n > kHuberMaxN)
        return apap::fail(APAP_ERR_INVALID_ARG, "%s: n=%d (the Huber M-step serves 1 .. 2^20 matches)", who, n);
    return APAP_OK;
}

constexpr int kModelMaxN = 1 << 26;

int model_check_n(int n, const char *who) {
    if (n < 1 || n > kModelMaxN) return apap::fail(APAP_ERR_INVALID_ARG, "%s: n=%d (need 1 .. 2^26 matches)", who, n);
    return APAP_OK;
}

// What the EM loop fixes, whatever the caller's block says: model_solve's `if w <= 1e-3: continue` and its swap default.
void model_em_scalars(ModelScalars &sc) {
    sc.use_floor = 1;
    sc.floor = 1e-3;
    sc.swap = 1;
}

}  // namespace
