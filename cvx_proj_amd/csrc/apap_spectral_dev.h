// Device half of the spectral match weighting, shared by apap_spectral.hip (one problem per launch) and apap_em_batch.hip
// (one launch for a batch of problems): constants, workspace layout, and the body of every kernel of the path.  A body
// takes the index of its block within its problem as `bx`; the __global__ wrappers of the two sources pass blockIdx.x.
// Both forms therefore run the same arithmetic in the same order: the batch is bit-identical to the single calls.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "apap_internal.h"

namespace {

constexpr int kSpecBasis = 64;      // Krylov basis of at most 64 vectors
constexpr int kSpecThreads = 256;
constexpr int kSpecOrthRows = 256;  // rows per block of k_spec_orth / k_spec_ritz
constexpr int kSpecDim = APAP_SPECTRAL_DIM;
constexpr double kSpecTol = 1e-13;        // converged: |M v - lambda v| <= kSpecTol |lambda|
constexpr double kSpecBreakdown = 1e-15;  // beta_j <= this x |T| ends a cycle early (invariant Krylov subspace)
constexpr int kSpecDefaultRestarts = 30;

struct SpecState {
    int done;        // 1 once converged: V[:, 0] is the eigenvector, lambda its Rayleigh quotient
    int cycle_stop;  // the current cycle ended early at m_eff vectors
    int m_eff;
    int ritz_m;      // vectors in the last Ritz combination
    int steps;       // Lanczos steps (matrix-vector products)
    int restarts;    // tridiagonal solves
    int pad[2];      // keeps the doubles 8-byte aligned
    double lambda, theta, gap, resid;
};

// Workspace layout (every part 256-byte aligned).  Linear in n: 512 n bytes of basis plus ~100 n bytes of the rest.
struct SpecLayout {
    int n, m, R, nb_mv, nb_o;
    size_t state, tri, diag, pts, W, Y, V, D1, D2, NP, mask, total;
};

int spec_rows_per_block(int n) { return n <= 2048 ? 4 : n <= 4096 ? 8 : n <= 8192 ? 16 : 32; }

SpecLayout spec_layout(int n) {
    SpecLayout L{};
    L.n = n;
    L.m = n < kSpecBasis ? n : kSpecBasis;
    L.R = spec_rows_per_block(n);
    L.nb_mv = (n + L.R - 1) / L.R;
    L.nb_o = (n + kSpecOrthRows - 1) / kSpecOrthRows;
    size_t off = 0;
    auto take = [&](size_t bytes) {
        const size_t at = off;
        off += (bytes + 255) / 256 * 256;
        return at;
    };
    L.state = take(sizeof(SpecState));
    L.tri = take((3 * kSpecBasis + 1) * sizeof(double));      // alpha[64] | beta[65] | s[64]
    L.diag = take((size_t)n * sizeof(double));
    L.pts = take((size_t)n * 4 * sizeof(float));               // (src x, src y, dst x, dst y) per match
    L.W = take((size_t)n * sizeof(double));
    L.Y = take((size_t)n * sizeof(double));
    L.V = take((size_t)n * kSpecBasis * sizeof(double));       // basis, match-major: V[i * 64 + k]
    L.D1 = take((size_t)L.nb_mv * kSpecBasis * sizeof(double));
    L.D2 = take((size_t)L.nb_o * kSpecBasis * sizeof(double));
    L.NP = take((size_t)L.nb_o * sizeof(double));
    L.mask = take((size_t)n * sizeof(float));
    L.total = off;
    return L;
}

struct SpecPtrs {
    SpecState *st;
    double *alpha, *beta, *s;
    double *diag;
    float4 *pts;
    double *W, *Y, *V, *D1, *D2, *NP;
    float *mask;
};

SpecPtrs spec_ptrs(const SpecLayout &L, void *work) {
    char *b = (char *)work;
    SpecPtrs p;
    p.st = (SpecState *)(b + L.state);
    p.alpha = (double *)(b + L.tri);
    p.beta = p.alpha + kSpecBasis;
    p.s = p.beta + kSpecBasis + 1;
    p.diag = (double *)(b + L.diag);
    p.pts = (float4 *)(b + L.pts);
    p.W = (double *)(b + L.W);
    p.Y = (double *)(b + L.Y);
    p.V = (double *)(b + L.V);
    p.D1 = (double *)(b + L.D1);
    p.D2 = (double *)(b + L.D2);
    p.NP = (double *)(b + L.NP);
    p.mask = (float *)(b + L.mask);
    return p;
}

// Scalars of the call (opts of the reference), by value into every kernel that needs them.
struct SpecScalars {
    double epi_weight, aff_thresh, em_radius, score_thresh;
    float rcp;   // float32(1 / 2 / affinity_eps ** 2): the python float becomes float32 against the float32 matrix
};

// numpy's float32 add.reduce over a contiguous row of 128: pairwise_sum's 8 accumulators, r[j] += a[8 k + j] in k order,
// then ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7)).  `term(k)` yields the k-th float32 summand.
template <typename F>
__device__ __forceinline__ float np_sum128(F term) {
    float r[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) r[j] = term(j);
    for (int k = 8; k < kSpecDim; k += 8) {
#pragma unroll
        for (int j = 0; j < 8; ++j) r[j] += term(k + j);
    }
    return ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
}

// off_ij of spectral_method.py:118-123, every operation float32 and rounded separately (-ffp-contract=off):
//   s = dxs*dxs + dys*dys (src),  d = the same on dst,  max(4.5 - ((s - d)^2) * rcp, 0)
// np.maximum propagates a NaN; so does this.
__device__ __forceinline__ float spec_off(float4 a, float4 b, float rcp) {
    const float dxs = a.x - b.x, dys = a.y - b.y;
    const float s = dxs * dxs + dys * dys;
    const float dxd = a.z - b.z, dyd = a.w - b.w;
    const float d = dxd * dxd + dyd * dyd;
    const float t = s - d;
    const float o = 4.5f - (t * t) * rcp;
    return o > 0.0f ? o : (o == o ? 0.0f : o);
}

// ---- S1: per match --------------------------------------------------------------------------------------------------
// c_feats /= np.linalg.norm(c_feats, axis=-1, keepdims=True) (:109-110): norm = sqrt(add.reduce(c * c)), float32, summed as
// np_sum128; each element divided (IEEE float32 division: hipcc's default keeps it correctly rounded).
// match_score = sum(c * o, -1) (:113), the same order.  epi (:111-112): F @ [x, y, 1]^T in float64 as
// (F[r][0] x + F[r][1] y) + F[r][2] (the reference's goes through BLAS: a few fp64 ulp apart), then
// |(u e0 + v e1) + e2|.  M_ii = float64(match_score) + epi_weight / (1 + epi) (:114).
// With Hg: recompute_matching (:35-64) in float32 - kpt_o = Hg @ (u, v, 1), dehomogenised, dist = |kpt_o - (x, y)|;
// kept when dist < em_radius and feat_score > score_thresh.  feat_score is match_score: the reference's 1-D norm there is
// BLAS sdot (:155-160 of utils.py), whose order is its own; the two differ by an ulp at most.
__device__ __forceinline__ void spec_setup_body(const float *__restrict__ src, const float *__restrict__ dst,
                                                             const float *__restrict__ cf, const float *__restrict__ of, int n,
                                                             const double *__restrict__ F, SpecScalars sc,
                                                             const float *__restrict__ Hg, const float *__restrict__ mask_in,
                                                             SpecPtrs p, int nb_o, unsigned bx) {
    const int i = bx * kSpecThreads + threadIdx.x;
    if (bx == 0) {
        if (threadIdx.x == 0) {
            SpecState z{};
            z.m_eff = n < kSpecBasis ? n : kSpecBasis;
            z.lambda = z.theta = z.gap = z.resid = __builtin_nan("");
            *p.st = z;
        }
        for (int b = threadIdx.x; b < nb_o; b += kSpecThreads) p.NP[b] = b == 0 ? (double)n : 0.0;  // |ones|^2: v0 = 1/sqrt(n)
    }
    if (i >= n) return;
    const float *c = cf + (size_t)i * kSpecDim;
    const float *o = of + (size_t)i * kSpecDim;
    const float nc = sqrtf(np_sum128([&](int k) { return c[k] * c[k]; }));
    const float no = sqrtf(np_sum128([&](int k) { return o[k] * o[k]; }));
    const float ms = np_sum128([&](int k) { return (c[k] / nc) * (o[k] / no); });
    const float2 s2 = ((const float2 *)src)[i];
    const float2 d2 = ((const float2 *)dst)[i];
    const double x = s2.x, y = s2.y, u = d2.x, v = d2.y;
    const double e0 = (F[0] * x + F[1] * y) + F[2];
    const double e1 = (F[3] * x + F[4] * y) + F[5];
    const double e2 = (F[6] * x + F[7] * y) + F[8];
    const double epi = fabs((u * e0 + v * e1) + e2);
    p.diag[i] = (double)ms + sc.epi_weight / (1.0 + epi);
    p.pts[i] = make_float4(s2.x, s2.y, d2.x, d2.y);
    p.W[i] = 1.0;
    if (Hg) {
        const float k0 = (Hg[0] * d2.x + Hg[1] * d2.y) + Hg[2];
        const float k1 = (Hg[3] * d2.x + Hg[4] * d2.y) + Hg[5];
        const float k2 = (Hg[6] * d2.x + Hg[7] * d2.y) + Hg[8];
        const float ex = k0 / k2 - s2.x, ey = k1 / k2 - s2.y;
        const float dist = sqrtf(ex * ex + ey * ey);
        p.mask[i] = ((double)dist < sc.em_radius && (double)ms > sc.score_thresh) ? 1.0f : 0.0f;
    } else if (mask_in) {
        p.mask[i] = mask_in[i];
    }
}

// ---- S2: y = M x, x = W / |W| ---------------------------------------------------------------------------------------
// Block: R rows, 256 / R lanes per row (one row's lanes sit in one wave).  Lane c of a row takes columns c, c + L, ...
// of each 256-match chunk staged in LDS; the row's partial sums meet in a shuffle tree of fixed shape.
// beta = sqrt(sum of the previous step's |w|^2 partials, in block order): every block computes the same value.
// At step 1, beta is |M v0 - alpha0 v0| itself (v0 unit, alpha0 its Rayleigh quotient): the convergence test.
template <int R>
__device__ __forceinline__ void spec_matvec_body(SpecPtrs p, int n, int j, int nb_o, float rcp, unsigned bx) {
    constexpr int L = kSpecThreads / R;
    __shared__ float4 s_pt[kSpecThreads];
    __shared__ double s_x[kSpecThreads];
    __shared__ double s_y[R], s_xo[R];
    __shared__ double s_beta;
    __shared__ int s_stop;
    const SpecState *st = p.st;
    if (st->done || st->cycle_stop) return;
    const int tid = threadIdx.x;
    if (tid == 0) {
        double nn = 0.0;
        for (int b = 0; b < nb_o; ++b) nn += p.NP[b];
        const double beta = sqrt(nn);
        int stop = 0;
        if (j >= 1) {
            const double a0 = fabs(p.alpha[0]);
            double tnorm = 0.0;
            for (int k = 0; k < j; ++k) tnorm = fmax(tnorm, fabs(p.alpha[k]) + (k ? p.beta[k] : 0.0));
            const bool conv = j == 1 && beta <= kSpecTol * a0;
            stop = conv ? 1 : (beta <= kSpecBreakdown * tnorm ? 2 : 0);
            if (bx == 0) {
                SpecState *w = p.st;
                p.beta[j] = beta;
                if (j == 1) w->resid = beta / a0;
                if (conv) {
                    w->lambda = p.alpha[0];
                    w->done = 1;
                } else if (stop == 2) {
                    w->m_eff = j;
                    w->cycle_stop = 1;
                }
            }
        }
        s_beta = beta;
        s_stop = stop;
    }
    __syncthreads();
    if (s_stop) return;
    const double beta = s_beta;
    const int r = tid / L, c = tid % L;
    const int row0 = bx * R;
    const int i = row0 + r;
    const bool valid = i < n;
    const float4 me = valid ? p.pts[i] : make_float4(0.f, 0.f, 0.f, 0.f);
    double acc = 0.0;
    for (int base = 0; base < n; base += kSpecThreads) {
        const int cnt = min(kSpecThreads, n - base);
        __syncthreads();
        if (tid < cnt) {
            s_pt[tid] = p.pts[base + tid];
            s_x[tid] = p.W[base + tid] / beta;
        }
        __syncthreads();
        for (int k = c; k < cnt; k += L) {
            const float off = base + k == i ? 0.0f : spec_off(me, s_pt[k], rcp);   // fill_diagonal(off_score, 0)
            acc = __builtin_fma((double)off, s_x[k], acc);
        }
    }
#pragma unroll
    for (int o = L / 2; o > 0; o >>= 1) acc += __shfl_down(acc, o, L);
    if (c == 0) {
        double yi = 0.0, xi = 0.0;
        if (valid) {
            xi = p.W[i] / beta;
            yi = acc + p.diag[i] * xi;
            p.V[(size_t)i * kSpecBasis + j] = xi;
            p.Y[i] = yi;
        }
        s_y[r] = yi;
        s_xo[r] = xi;
    }
    __syncthreads();
    if (tid <= j) {   // first pass of the Gram-Schmidt: this block's share of V[:, k] . y
        double d = 0.0;
        for (int q = 0; q < R && row0 + q < n; ++q)
            d = __builtin_fma(s_y[q], tid == j ? s_xo[q] : p.V[(size_t)(row0 + q) * kSpecBasis + tid], d);
        p.D1[(size_t)bx * kSpecBasis + tid] = d;
    }
}

// ---- the two re-orthogonalisation passes ----------------------------------------------------------------------------
// pass 1: h = sum of D1 (fixed order); Y -= V h; D2 = this block's V^T Y.
// pass 2: h2 = sum of D2 (the same order); W = Y - V h2 (the next, unnormalised vector); alpha_j = h_j + h2_j; NP = this block's |W|^2.
__device__ __forceinline__ void spec_orth_body(SpecPtrs p, int n, int j, int nb_in, int pass, unsigned bx) {
    __shared__ double s_h[kSpecBasis];
    __shared__ double s_y[kSpecThreads];
    __shared__ double s_part[kSpecThreads];
    const SpecState *st = p.st;
    if (st->done || st->cycle_stop) return;
    const int tid = threadIdx.x;
    const double *Din = pass == 1 ? p.D1 : p.D2;
    {   // h = the blocks' partial dots summed: lane k of wave q takes blocks q, q + 4, ...; the four waves meet in LDS
        const int k = tid & 63, q = tid >> 6;
        double h = 0.0;
        if (k <= j)
            for (int b = q; b < nb_in; b += 4) h += Din[(size_t)b * kSpecBasis + k];
        s_part[tid] = h;
        __syncthreads();
        if (tid <= j) s_h[tid] = (s_part[tid] + s_part[tid + 64]) + (s_part[tid + 128] + s_part[tid + 192]);
        __syncthreads();
    }
    const int i = bx * kSpecOrthRows + tid;
    double y = 0.0;
    if (i < n) {
        y = p.Y[i];
        const double *v = p.V + (size_t)i * kSpecBasis;
        for (int k = 0; k <= j; ++k) y = __builtin_fma(-s_h[k], v[k], y);
        if (pass == 1) p.Y[i] = y;
        else p.W[i] = y;
    }
    s_y[tid] = y;
    __syncthreads();
    if (pass == 1) {
        // 4 waves x 64 rows each; lane k takes basis vector k
        const int k = tid & 63, part = tid >> 6;
        double d = 0.0;
        if (k <= j)
            for (int q = part * 64; q < part * 64 + 64; ++q) {
                const int row = bx * kSpecOrthRows + q;
                if (row < n) d = __builtin_fma(s_y[q], p.V[(size_t)row * kSpecBasis + k], d);
            }
        s_part[tid] = d;
        __syncthreads();
        if (tid <= j)
            p.D2[(size_t)bx * kSpecBasis + tid] = (s_part[tid] + s_part[tid + 64]) + (s_part[tid + 128] + s_part[tid + 192]);
        if (bx == 0 && tid == 0) p.alpha[j] = s_h[j];
    } else {
        s_part[tid] = y * y;
        __syncthreads();
        for (int o = kSpecThreads / 2; o > 0; o >>= 1) {
            if (tid < o) s_part[tid] += s_part[tid + o];
            __syncthreads();
        }
        if (tid == 0) {
            p.NP[bx] = s_part[0];
            if (bx == 0) {
                p.alpha[j] += s_h[j];   // pass 1 stored h_j
                p.st->steps += 1;
            }
        }
    }
}

// Sturm count: eigenvalues of the tridiagonal (a, b^2) below x.
__device__ int sturm_count(const double *a, const double *b2, int m, double x, double pivmin) {
    int cnt = 0;
    double q = a[0] - x;
    if (fabs(q) < pivmin) q = -pivmin;
    cnt += q < 0.0;
    for (int k = 1; k < m; ++k) {
        q = (a[k] - x) - b2[k] / q;
        if (fabs(q) < pivmin) q = -pivmin;
        cnt += q < 0.0;
    }
    return cnt;
}

// ---- the tridiagonal problem, one workgroup ---------------------------------------------------------------------
// Waves 0..3 find eigenvalues m-1, m-2, 0 and 1 of T (ascending) by 64-way multisection of the Gershgorin interval:
// each pass evaluates 64 Sturm counts and keeps the 1/65 of the interval that holds the eigenvalue.  The Ritz pair of
// largest |theta| is one of the two ends; the gap is measured against the larger |theta| of the two runners-up.  Its
// eigenvector: inverse iteration (three solves) with T - theta I factored by Gaussian elimination with partial pivoting.
__device__ __forceinline__ void spec_tri_body(SpecPtrs p, int m_max, int nb_o) {
    __shared__ double s_a[kSpecBasis], s_b2[kSpecBasis], s_b[kSpecBasis];
    __shared__ double s_theta[4];
    __shared__ double lu_d[kSpecBasis], lu_e[kSpecBasis], lu_f[kSpecBasis], lu_l[kSpecBasis], x[kSpecBasis];
    __shared__ int lu_p[kSpecBasis];
    SpecState *st = p.st;
    if (st->done) return;
    const int m = st->cycle_stop ? st->m_eff : m_max;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid < m) {
        s_a[tid] = p.alpha[tid];
        s_b[tid] = tid ? p.beta[tid] : 0.0;
        s_b2[tid] = s_b[tid] * s_b[tid];
    }
    __syncthreads();
    double lo = s_a[0], hi = s_a[0], tn = 0.0;
    for (int k = 0; k < m; ++k) {
        const double r = fabs(k ? s_b[k] : 0.0) + fabs(k + 1 < m ? s_b[k + 1] : 0.0);
        lo = fmin(lo, s_a[k] - r);
        hi = fmax(hi, s_a[k] + r);
        tn = fmax(tn, fabs(s_a[k]) + r);
    }
    const double pivmin = fmax(tn * 1e-300, 1e-300);
    const int want[4] = {m - 1, m - 2, 0, 1};
    const int idx = min(max(want[wave], 0), m - 1);
    double a = lo - 1e-14 * tn - 1e-300, b = hi + 1e-14 * tn + 1e-300;
    for (int pass = 0; pass < 16; ++pass) {
        const double w = b - a;
        if (!(w > 2.2e-16 * fmax(fabs(a), fabs(b)))) break;
        const double xl = a + w * (double)(lane + 1) / 65.0;
        const bool below = sturm_count(s_a, s_b2, m, xl, pivmin) <= idx;
        const int cntb = __popcll(__ballot(below));
        const double na = cntb > 0 ? a + w * (double)cntb / 65.0 : a;
        const double nb = cntb < 64 ? a + w * (double)(cntb + 1) / 65.0 : b;
        a = na;
        b = nb;
    }
    if (lane == 0) s_theta[wave] = 0.5 * (a + b);
    __syncthreads();
    if (tid != 0) return;
    const double tmax = s_theta[0], tmin = s_theta[2];
    const bool top = fabs(tmax) >= fabs(tmin);
    const double theta = top ? tmax : tmin;
    double gap = __builtin_nan("");
    if (m >= 2) {
        const double second = top ? fmax(fabs(s_theta[1]), fabs(tmin)) : fmax(fabs(tmax), fabs(s_theta[3]));
        gap = (fabs(theta) - second) / fabs(theta);
    }
    // LU of T - theta I with partial pivoting: row k holds (d, e, f) on columns k, k+1, k+2
    const double tiny = fmax(2.2e-16 * tn, 1e-300);
    for (int k = 0; k < m; ++k) {
        lu_d[k] = s_a[k] - theta;
        lu_e[k] = k + 1 < m ? s_b[k + 1] : 0.0;
        lu_f[k] = 0.0;
    }
    for (int k = 0; k + 1 < m; ++k) {
        const double sub = s_b[k + 1];
        double d = lu_d[k], e = lu_e[k], f = 0.0;
        double d1 = lu_d[k + 1], e1 = lu_e[k + 1], c = sub;
        int piv = 0;
        if (fabs(c) > fabs(d)) {   // swap rows k and k + 1
            double t;
            t = d; d = c; c = t;
            t = e; e = d1; d1 = t;
            f = e1; e1 = 0.0;
            piv = 1;
        }
        if (d == 0.0) d = tiny;
        const double l = c / d;
        lu_d[k] = d;
        lu_e[k] = e;
        lu_f[k] = f;
        lu_l[k] = l;
        lu_p[k] = piv;
        lu_d[k + 1] = d1 - l * e;
        lu_e[k + 1] = e1 - l * f;
    }
    if (lu_d[m - 1] == 0.0) lu_d[m - 1] = tiny;
    for (int k = 0; k < m; ++k) x[k] = 1.0 + 0.25 * (double)((k * 37) % 11) / 11.0;
    for (int it = 0; it < 3; ++it) {
        for (int k = 0; k + 1 < m; ++k) {
            if (lu_p[k]) {
                const double t = x[k];
                x[k] = x[k + 1];
                x[k + 1] = t;
            }
            x[k + 1] -= lu_l[k] * x[k];
        }
        for (int k = m - 1; k >= 0; --k) {
            double r = x[k];
            if (k + 1 < m) r -= lu_e[k] * x[k + 1];
            if (k + 2 < m) r -= lu_f[k] * x[k + 2];
            x[k] = r / lu_d[k];
        }
        double mx = 0.0;
        for (int k = 0; k < m; ++k) mx = fmax(mx, fabs(x[k]));
        double nn = 0.0;
        for (int k = 0; k < m; ++k) {
            x[k] /= mx;
            nn += x[k] * x[k];
        }
        const double inv = 1.0 / sqrt(nn);
        for (int k = 0; k < m; ++k) x[k] *= inv;
    }
    for (int k = 0; k < m; ++k) p.s[k] = x[k];
    st->theta = theta;
    st->gap = gap;
    st->ritz_m = m;
    st->restarts += 1;
    st->cycle_stop = 0;
    st->m_eff = m_max;
    if (m == 1) {   // the whole space, or an invariant line: the Ritz pair is exact up to |w| after step 0
        double nn = 0.0;
        for (int b = 0; b < nb_o; ++b) nn += p.NP[b];
        const double res = sqrt(nn);
        st->resid = res / fabs(s_a[0]);
        if (res <= kSpecTol * fabs(s_a[0])) {
            st->lambda = s_a[0];
            st->done = 1;
        }
    }
}

// W = V s (the restart vector), NP = this block's |W|^2.
__device__ __forceinline__ void spec_ritz_body(SpecPtrs p, int n, unsigned bx) {
    __shared__ double s_s[kSpecBasis];
    __shared__ double s_part[kSpecThreads];
    const SpecState *st = p.st;
    if (st->done) return;
    const int tid = threadIdx.x, m = st->ritz_m;
    if (tid < m) s_s[tid] = p.s[tid];
    __syncthreads();
    const int i = bx * kSpecOrthRows + tid;
    double y = 0.0;
    if (i < n) {
        const double *v = p.V + (size_t)i * kSpecBasis;
        for (int k = 0; k < m; ++k) y = __builtin_fma(s_s[k], v[k], y);
        p.W[i] = y;
    }
    s_part[tid] = y * y;
    __syncthreads();
    for (int o = kSpecThreads / 2; o > 0; o >>= 1) {
        if (tid < o) s_part[tid] += s_part[tid + o];
        __syncthreads();
    }
    if (tid == 0) p.NP[bx] = s_part[0];
}

// ---- S3: finish (spectral_method.py:115-116,129-132) ------------------------------------------------------------------
// segment = |v| / max|v| (float64), segment[segment < 1e-6] = 0, bool_mask = segment > aff_thresh,
// ransac_mask = mask * float32(aff_thresh), ransac_mask[bool_mask] = float32(segment[bool_mask]).
// v is the converged eigenvector, or - capped - the last Ritz vector (APAP_STATUS_NO_CONVERGENCE).
constexpr int kFinishThreads = 1024;
__device__ __forceinline__ void spec_finish_body(SpecPtrs p, int n, SpecScalars sc,
                                                                double *__restrict__ segment, float *__restrict__ ransac_mask,
                                                                float *__restrict__ original_mask, double *__restrict__ info,
                                                                int *__restrict__ status) {
    __shared__ double s_max[kFinishThreads];
    const SpecState *st = p.st;
    const bool done = st->done != 0;
    const int tid = threadIdx.x;
    auto vec = [&](int i) { return done ? p.V[(size_t)i * kSpecBasis] : p.W[i]; };
    double mx = 0.0;
    for (int i = tid; i < n; i += kFinishThreads) {
        const double a = fabs(vec(i));
        mx = (a > mx || a != a) ? a : mx;
    }
    s_max[tid] = mx;
    __syncthreads();
    for (int o = kFinishThreads / 2; o > 0; o >>= 1) {
        if (tid < o) {
            const double b = s_max[tid + o];
            if (b > s_max[tid] || b != b) s_max[tid] = b;
        }
        __syncthreads();
    }
    mx = s_max[0];
    const float aff32 = (float)sc.aff_thresh;
    for (int i = tid; i < n; i += kFinishThreads) {
        double sg = fabs(vec(i)) / mx;
        if (sg < 1e-6) sg = 0.0;
        segment[i] = sg;
        const float m0 = p.mask[i];
        original_mask[i] = m0;
        ransac_mask[i] = sg > sc.aff_thresh ? (float)sg : m0 * aff32;
    }
    if (tid == 0) {
        const int word = done ? 0 : APAP_STATUS_NO_CONVERGENCE;
        info[0] = done ? st->lambda : st->theta;
        info[1] = st->gap;
        info[2] = (double)st->steps;
        info[3] = (double)word;
        info[4] = (double)st->restarts;
        info[5] = st->resid;
        if (word && status) atomicOr(status, word);
    }
}

int spec_check_params(const double *params, SpecScalars *sc, int *restarts, const char *who) {
    if (!params) return apap::fail(APAP_ERR_INVALID_ARG, "%s: null params", who);
    const double eps = params[APAP_SPECTRAL_AFFINITY_EPS];
    sc->epi_weight = params[APAP_SPECTRAL_EPI_WEIGHT];
    sc->aff_thresh = params[APAP_SPECTRAL_AFF_THRESH];
    sc->em_radius = params[APAP_SPECTRAL_EM_RADIUS];
    sc->score_thresh = params[APAP_SPECTRAL_SCORE_THRESH];
    sc->rcp = (float)(1.0 / 2.0 / (eps * eps));   // rcp_value = 1 / 2 / (opts.affinity_eps ** 2) (:116)
    const double r = params[APAP_SPECTRAL_MAX_RESTARTS];
    if (!(r >= 0.0 && r <= 100000.0)) return apap::fail(APAP_ERR_INVALID_ARG, "%s: max_restarts %g out of range", who, r);
    *restarts = r == 0.0 ? kSpecDefaultRestarts : (int)r;
    return APAP_OK;
}

}  // namespace
