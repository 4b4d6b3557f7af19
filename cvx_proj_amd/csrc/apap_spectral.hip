// Spectral match weighting: calculate_M of the reference's spectral_method.py:66-133, device half.
//
// The reference builds a dense N x N affinity M over the N coarse matches, takes a full SVD of it and keeps U[:, 0].
// Here M is never stored: its off-diagonal entries are recomputed from the four float32 coordinates of each pair of
// matches inside every matrix-vector product, and the principal vector comes from a restarted Lanczos iteration in fp64.
//
//   S1 k_spec_setup    one lane per match: descriptor normalisation, match_score, epipolar score -> the fp64 diagonal;
//                      the initial mask (recompute_matching with Hg, or the caller's mask); the start vector; state reset.
//   S2 k_spec_matvec   y = M x for R rows per block, x = W / |W| staged through LDS in chunks of 256 matches; also the
//                      block's partial dots of y with the Krylov basis (first Gram-Schmidt pass).
//      k_spec_orth     two launches per step: subtract the projections (classical Gram-Schmidt, twice), alpha, |w|^2.
//      k_spec_tri      one workgroup: the extreme Ritz values of the tridiagonal by Sturm multisection (one wave per
//                      eigenvalue), the eigenvector of the one of largest |theta| by inverse iteration.
//      k_spec_ritz     the restart vector V s.
//   S3 k_spec_finish   one workgroup: |v| / max|v|, the 1e-6 zeroing, the threshold and both masks; the info block.
//
// Every kernel after S1 first reads the state's `done` word (set once |M v - lambda v| <= 1e-13 |lambda|) and returns at
// once when it is set, so the host can enqueue a fixed number of restart cycles.  No grid-wide barrier, no spin-wait:
// all communication between workgroups goes through kernel boundaries on one stream.  Every sum has a fixed order, so
// a call is deterministic.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>

#include "apap_internal.h"

#include "apap_spectral_dev.h"

namespace {

// The kernels of one problem: the bodies of apap_spectral_dev.h on this launch's blocks.
__global__ __launch_bounds__(kSpecThreads) void k_spec_setup(const float *__restrict__ src, const float *__restrict__ dst,
                                                             const float *__restrict__ cf, const float *__restrict__ of, int n,
                                                             const double *__restrict__ F, SpecScalars sc,
                                                             const float *__restrict__ Hg, const float *__restrict__ mask_in,
                                                             SpecPtrs p, int nb_o) {
    spec_setup_body(src, dst, cf, of, n, F, sc, Hg, mask_in, p, nb_o, blockIdx.x);
}

template <int R>
__global__ __launch_bounds__(kSpecThreads) void k_spec_matvec(SpecPtrs p, int n, int j, int nb_o, float rcp) {
    spec_matvec_body<R>(p, n, j, nb_o, rcp, blockIdx.x);
}

__global__ __launch_bounds__(kSpecThreads) void k_spec_orth(SpecPtrs p, int n, int j, int nb_in, int pass) {
    spec_orth_body(p, n, j, nb_in, pass, blockIdx.x);
}

__global__ __launch_bounds__(kSpecThreads) void k_spec_tri(SpecPtrs p, int m_max, int nb_o) { spec_tri_body(p, m_max, nb_o); }

__global__ __launch_bounds__(kSpecThreads) void k_spec_ritz(SpecPtrs p, int n) { spec_ritz_body(p, n, blockIdx.x); }

__global__ __launch_bounds__(kFinishThreads) void k_spec_finish(SpecPtrs p, int n, SpecScalars sc, double *__restrict__ segment,
                                                                float *__restrict__ ransac_mask, float *__restrict__ original_mask,
                                                                double *__restrict__ info, int *__restrict__ status) {
    spec_finish_body(p, n, sc, segment, ransac_mask, original_mask, info, status);
}

// ---- dense M (the reference's verbose path and the parity tests) ----------------------------------------------------
__global__ __launch_bounds__(kSpecThreads) void k_spec_affinity(SpecPtrs p, int n, float rcp, double *__restrict__ M) {
    const int j = blockIdx.x * kSpecThreads + threadIdx.x;
    const int i = blockIdx.y;
    if (j >= n) return;
    M[(size_t)i * n + j] = i == j ? p.diag[i] : (double)spec_off(p.pts[i], p.pts[j], rcp);
}


int spec_launch_setup(const SpecLayout &L, const SpecPtrs &P, const float *d_src, const float *d_dst, const float *d_c,
                      const float *d_o, const double *d_F, const SpecScalars &sc, const float *d_Hg, const float *d_mask,
                      hipStream_t s) {
    hipLaunchKernelGGL(k_spec_setup, dim3((L.n + kSpecThreads - 1) / kSpecThreads), dim3(kSpecThreads), 0, s, d_src, d_dst,
                       d_c, d_o, L.n, d_F, sc, d_Hg, d_mask, P, L.nb_o);
    return APAP_OK;
}

// One restart cycle: m Lanczos steps (3 launches each), the tridiagonal solve, the restart vector.
void spec_launch_cycle(const SpecLayout &L, const SpecPtrs &P, float rcp, hipStream_t s) {
    for (int j = 0; j < L.m; ++j) {
        switch (L.R) {
            case 4: hipLaunchKernelGGL(k_spec_matvec<4>, dim3(L.nb_mv), dim3(kSpecThreads), 0, s, P, L.n, j, L.nb_o, rcp); break;
            case 8: hipLaunchKernelGGL(k_spec_matvec<8>, dim3(L.nb_mv), dim3(kSpecThreads), 0, s, P, L.n, j, L.nb_o, rcp); break;
            case 16: hipLaunchKernelGGL(k_spec_matvec<16>, dim3(L.nb_mv), dim3(kSpecThreads), 0, s, P, L.n, j, L.nb_o, rcp); break;
            default: hipLaunchKernelGGL(k_spec_matvec<32>, dim3(L.nb_mv), dim3(kSpecThreads), 0, s, P, L.n, j, L.nb_o, rcp); break;
        }
        hipLaunchKernelGGL(k_spec_orth, dim3(L.nb_o), dim3(kSpecThreads), 0, s, P, L.n, j, L.nb_mv, 1);
        hipLaunchKernelGGL(k_spec_orth, dim3(L.nb_o), dim3(kSpecThreads), 0, s, P, L.n, j, L.nb_o, 2);
    }
    hipLaunchKernelGGL(k_spec_tri, dim3(1), dim3(kSpecThreads), 0, s, P, L.m, L.nb_o);
    hipLaunchKernelGGL(k_spec_ritz, dim3(L.nb_o), dim3(kSpecThreads), 0, s, P, L.n);
}

int spec_check_device_args(int n, const void *d_src, const void *d_dst, const void *d_c, const void *d_o, const void *d_F,
                           const void *d_work, size_t work_bytes, const char *who) {
    if (!d_src || !d_dst || !d_c || !d_o || !d_F || !d_work) return apap::fail(APAP_ERR_INVALID_ARG, "%s: null device pointer", who);
    if (n < 1 || n > (1 << 26)) return apap::fail(APAP_ERR_INVALID_ARG, "%s: n=%d (need 1 .. 2^26 matches)", who, n);
    if (work_bytes < spec_layout(n).total)
        return apap::fail(APAP_ERR_WORKSPACE, "%s: workspace %zu < %zu bytes", who, work_bytes, spec_layout(n).total);
    if (((uintptr_t)d_work & 255) != 0 || ((uintptr_t)d_src & 7) != 0 || ((uintptr_t)d_dst & 7) != 0)
        return apap::fail(APAP_ERR_INVALID_ARG, "%s: workspace must be 256-byte and points 8-byte aligned", who);
    return APAP_OK;
}

}  // namespace

namespace apap {

// The body of apap_spectral_device, with `sync_each` = 1 for the host-buffer entry point: it then waits for each restart
// cycle and stops enqueuing once the device reports convergence (the device form enqueues all of them; launches after
// convergence return at once).
int spectral_run(apap_ctx *ctx, const float *d_src, const float *d_dst, const float *d_c, const float *d_o, int n,
                 const double *d_F, const double *params, const float *d_Hg, const float *d_mask, double *d_segment,
                 float *d_ransac, float *d_original, double *d_info, int *d_status, void *d_work, size_t work_bytes,
                 void *stream, int sync_each) {
    const char *who = "apap_spectral_device";
    int rc = spec_check_device_args(n, d_src, d_dst, d_c, d_o, d_F, d_work, work_bytes, who);
    if (rc) return rc;
    if (!d_segment || !d_info) return apap::fail(APAP_ERR_INVALID_ARG, "%s: null output pointer", who);
    if (!d_Hg && !d_mask)
        return apap::fail(APAP_ERR_INVALID_ARG, "%s: no initial mask (neither Hg nor a mask): the reference's init_ransac=False "
                                                "path fails on `None *= float` (spectral_method.py:131)", who);
    if (!d_ransac || !d_original) return apap::fail(APAP_ERR_INVALID_ARG, "%s: null mask output", who);
    SpecScalars sc;
    int restarts;
    if ((rc = spec_check_params(params, &sc, &restarts, who))) return rc;
    const SpecLayout L = spec_layout(n);
    SpecPtrs P = spec_ptrs(L, d_work);
    hipStream_t s = (hipStream_t)stream;
    {
        apap::ProfScope prof(ctx, APAP_PROF_SPECTRAL, s);
        spec_launch_setup(L, P, d_src, d_dst, d_c, d_o, d_F, sc, d_Hg, d_mask, s);
        for (int c = 0; c < restarts; ++c) {
            spec_launch_cycle(L, P, sc.rcp, s);
            if (sync_each) {
                int done = 0;
                hipError_t e = hipMemcpyAsync(&done, &P.st->done, sizeof(int), hipMemcpyDeviceToHost, s);
                if (e == hipSuccess) e = hipStreamSynchronize(s);
                if (e != hipSuccess) return apap::hip_fail(e, "apap_spectral_device: cycle");
                if (done) break;
            }
        }
        hipLaunchKernelGGL(k_spec_finish, dim3(1), dim3(kFinishThreads), 0, s, P, n, sc, d_segment, d_ransac, d_original,
                           d_info, d_status);
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return apap::hip_fail(e, "apap_spectral_device launch");
    return APAP_OK;
}

int spectral_affinity_run(const float *d_src, const float *d_dst, const float *d_c, const float *d_o, int n, const double *d_F,
                          const double *params, double *d_M, void *d_work, size_t work_bytes, void *stream) {
    const char *who = "apap_spectral_affinity";
    int rc = spec_check_device_args(n, d_src, d_dst, d_c, d_o, d_F, d_work, work_bytes, who);
    if (rc) return rc;
    SpecScalars sc;
    int restarts;
    if ((rc = spec_check_params(params, &sc, &restarts, who))) return rc;
    const SpecLayout L = spec_layout(n);
    SpecPtrs P = spec_ptrs(L, d_work);
    hipStream_t s = (hipStream_t)stream;
    spec_launch_setup(L, P, d_src, d_dst, d_c, d_o, d_F, sc, nullptr, nullptr, s);
    hipLaunchKernelGGL(k_spec_affinity, dim3((n + kSpecThreads - 1) / kSpecThreads, n), dim3(kSpecThreads), 0, s, P, n, sc.rcp, d_M);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return apap::hip_fail(e, "apap_spectral_affinity launch");
    return APAP_OK;
}

}  // namespace apap

extern "C" {

size_t apap_spectral_workspace_bytes(int n) {
    if (n < 1) return 0;
    return spec_layout(n).total;
}

int apap_spectral_device(apap_ctx *ctx, const float *d_src, const float *d_dst, const float *d_c_feats, const float *d_o_feats,
                         int n, const double *d_F, const double *params, const float *d_Hg_or_null,
                         const float *d_mask_in_or_null, double *d_segment, float *d_ransac_mask, float *d_original_mask,
                         double *d_info, int *d_status, void *d_work, size_t work_bytes, void *stream) {
    return apap::spectral_run(ctx, d_src, d_dst, d_c_feats, d_o_feats, n, d_F, params, d_Hg_or_null, d_mask_in_or_null, d_segment,
                              d_ransac_mask, d_original_mask, d_info, d_status, d_work, work_bytes, stream, 0);
}

}  // extern "C"
