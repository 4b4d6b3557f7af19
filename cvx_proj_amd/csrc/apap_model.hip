// M-step of the spectral method: model_solve of the reference's spectral_method.py:165-186 with model.py's LMSSolver /
// SDPSolver, and the EM loop of spectral_method() (:188-241), device half.
//
//   M1 k_model_tsqr   one wave per block of matches: the rows of K = [A | -rhs | A1's 0 3 6 | A2's 1 4 7] of the selected
//                     matches, generated in the reference's dtypes (A, rhs float32; A1, A2 float64), folded 24 matches at a
//                     time into the block's 15 x 15 R by Householder reflections (lanes 0..14 hold R, lanes 15..62 the rows).
//   M2 k_model_solve  one wave: folds the block factors three at a time in block order, equilibrates, checks the rank,
//                     solves (LMS: back-substitution; SDP: interior-point method on the 18 x 18 LMI), applies model.py's
//                     float32 tail.
//   M3 k_model_huber  mode HUBER only, after M1 and M2 in LMS mode: one workgroup of 256; from M2's h0 the whole Newton / line
//                     search iteration on sum phi_M(A h - rhs) and its duality gap, the rows regenerated on every pass.
//
// Why 18 x 18: with P = [u v q] = K X(h) and K = Q R, P^T P = (R X)^T (R X), so [[I_2n, P], [P^T, D]] >= 0 (D = diag(r, r,
// t)) holds exactly when D - (R X)^T (R X) >= 0, i.e. when [[I_15, R X], [(R X)^T, D]] >= 0 (Schur complement, twice).
// Every sum has a fixed order (butterfly wave sums, whose every lane sees the same value, and serial loops): a call is
// deterministic.  No atomics but the status word's OR.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "apap_internal.h"

#include "apap_model_dev.h"

namespace {

// The kernels of one problem: the bodies of apap_model_dev.h on this launch's blocks.
__global__ __launch_bounds__(kW) void k_model_tsqr(const float2 *__restrict__ pc, const float2 *__restrict__ po,
                                                   const float *__restrict__ w, int n, int per_block, ModelScalars sc,
                                                   double *__restrict__ Rb, int *__restrict__ cnt) {
    model_tsqr_body(pc, po, LoadWeight{w}, n, per_block, sc, Rb, cnt, blockIdx.x);
}

__global__ __launch_bounds__(kW) void k_model_solve(const double *__restrict__ Rb, const int *__restrict__ cnt, int nb,
                                                    ModelScalars sc, float *__restrict__ H, double *__restrict__ info,
                                                    int *__restrict__ status) {
    model_solve_body(Rb, cnt, nb, sc, H, info, status);
}

__global__ __launch_bounds__(kHuberThreads) void k_model_huber(const float2 *__restrict__ pc, const float2 *__restrict__ po,
                                                               const float *__restrict__ w, int n, ModelScalars sc,
                                                               float *__restrict__ H, double *__restrict__ info,
                                                               int *__restrict__ status) {
    model_huber_body(pc, po, w, n, sc, H, info, status);
}

// The pointer, workspace and alignment checks of both entry points; n has passed model_check_n by then.
int model_check_device_args(const void *d_pc, const void *d_po, const void *d_w, const void *d_H, const void *d_info,
                            const void *d_work, size_t work_bytes, size_t need, const char *who) {
    if (!d_pc || !d_po || !d_w || !d_H || !d_info || !d_work) return apap::fail(APAP_ERR_INVALID_ARG, "%s: null device pointer", who);
    if (work_bytes < need) return apap::fail(APAP_ERR_WORKSPACE, "%s: workspace %zu < %zu bytes", who, work_bytes, need);
    if (((uintptr_t)d_work & 255) != 0 || ((uintptr_t)d_pc & 7) != 0 || ((uintptr_t)d_po & 7) != 0)
        return apap::fail(APAP_ERR_INVALID_ARG, "%s: workspace must be 256-byte and points 8-byte aligned", who);
    return APAP_OK;
}

// M1 + M2 on `stream` (both entry points and every round of the EM loop).  Mode HUBER: M1 and M2 in LMS mode give the count,
// the degenerate status and h0; the Huber kernel starts from them and reports the status word itself.
void model_launch(const ModelLayout &L, const ModelScalars &sc, const float *d_pc, const float *d_po, const float *d_w,
                  float *d_H, double *d_info, int *d_status, void *d_work, hipStream_t s) {
    char *b = (char *)d_work;
    double *Rb = (double *)(b + L.R);
    int *cnt = (int *)(b + L.cnt);
    hipLaunchKernelGGL(k_model_tsqr, dim3(L.nb), dim3(kW), 0, s, (const float2 *)d_pc, (const float2 *)d_po, d_w, L.n, L.per_block,
                       sc, Rb, cnt);
    if (sc.mode != APAP_MODEL_HUBER) {
        hipLaunchKernelGGL(k_model_solve, dim3(1), dim3(kW), 0, s, Rb, cnt, L.nb, sc, d_H, d_info, d_status);
        return;
    }
    ModelScalars lms = sc;
    lms.mode = APAP_MODEL_LMS;
    hipLaunchKernelGGL(k_model_solve, dim3(1), dim3(kW), 0, s, Rb, cnt, L.nb, lms, d_H, d_info, (int *)nullptr);
    hipLaunchKernelGGL(k_model_huber, dim3(1), dim3(kHuberThreads), 0, s, (const float2 *)d_pc, (const float2 *)d_po, d_w, L.n, sc,
                       d_H, d_info, d_status);
}

}  // namespace

extern "C" {

size_t apap_model_workspace_bytes(int n) {
    if (n < 1) return 0;
    return model_layout(n).total;
}

int apap_model_solve_device(apap_ctx *ctx, const float *d_pts_c, const float *d_pts_o, const float *d_weights, int n,
                            const double *params, float *d_H, double *d_info, int *d_status, void *d_work, size_t work_bytes,
                            void *stream) {
    const char *who = "apap_model_solve_device";
    ModelScalars sc;
    int rc = model_check_params(params, &sc, who);
    if (rc) return rc;
    if ((rc = model_check_huber(sc, n, who))) return rc;
    if ((rc = model_check_n(n, who))) return rc;
    const ModelLayout L = model_layout(n);
    if ((rc = model_check_device_args(d_pts_c, d_pts_o, d_weights, d_H, d_info, d_work, work_bytes, L.total, who))) return rc;
    hipStream_t s = (hipStream_t)stream;
    model_launch(L, sc, d_pts_c, d_pts_o, d_weights, d_H, d_info, d_status, d_work, s);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return apap::hip_fail(e, "apap_model_solve_device launch");
    return APAP_OK;
}

int apap_spectral_em_device(apap_ctx *ctx, const float *d_src, const float *d_dst, const float *d_c_feats, const float *d_o_feats,
                            int n, const double *d_F, const double *spec_params, const double *model_params, int em_steps,
                            const float *d_mask_in, float *d_H, double *d_info, double *d_segment, float *d_ransac_mask,
                            float *d_original_mask, double *d_spec_info, int *d_status, void *d_work, size_t work_bytes,
                            void *stream) {
    return apap::spectral_em_run(ctx, d_src, d_dst, d_c_feats, d_o_feats, n, d_F, spec_params, model_params, em_steps, d_mask_in,
                                 d_H, d_info, d_segment, d_ransac_mask, d_original_mask, d_spec_info, d_status, d_work, work_bytes,
                                 stream, 0);
}

}  // extern "C"

namespace apap {

// The body of apap_spectral_em_device; sync_each = 1 (the host-buffer entry point) waits for every restart cycle of the
// spectral rounds and stops enqueuing them at convergence, as apap_spectral_weights does (same results: the cycles after
// convergence change nothing).
int spectral_em_run(apap_ctx *ctx, const float *d_src, const float *d_dst, const float *d_c_feats, const float *d_o_feats, int n,
                    const double *d_F, const double *spec_params, const double *model_params, int em_steps, const float *d_mask_in,
                    float *d_H, double *d_info, double *d_segment, float *d_ransac_mask, float *d_original_mask,
                    double *d_spec_info, int *d_status, void *d_work, size_t work_bytes, void *stream, int sync_each) {
    const char *who = "apap_spectral_em_device";
    ModelScalars sc;
    int rc = model_check_params(model_params, &sc, who);
    if (rc) return rc;
    if ((rc = model_check_huber(sc, n, who))) return rc;
    model_em_scalars(sc);
    if (em_steps < 1 || em_steps > 64) return apap::fail(APAP_ERR_INVALID_ARG, "%s: em_steps %d (1 .. 64)", who, em_steps);
    if (!d_mask_in) return apap::fail(APAP_ERR_INVALID_ARG, "%s: null initial mask", who);
    if ((rc = model_check_n(n, who))) return rc;
    if (!d_segment || !d_ransac_mask || !d_original_mask || !d_spec_info)
        return apap::fail(APAP_ERR_INVALID_ARG, "%s: null spectral output", who);
    const size_t spec_bytes = apap_spectral_workspace_bytes(n);
    const ModelLayout L = model_layout(n);
    if ((rc = model_check_device_args(d_src, d_dst, d_ransac_mask, d_H, d_info, d_work, work_bytes, spec_bytes + L.total, who)))
        return rc;
    void *d_model_work = (char *)d_work + spec_bytes;
    hipStream_t s = (hipStream_t)stream;
    for (int k = 0; k < em_steps; ++k) {
        float *rm = d_ransac_mask + (size_t)k * n;
        rc = apap::spectral_run(ctx, d_src, d_dst, d_c_feats, d_o_feats, n, d_F, spec_params, k ? d_H + 9 * (k - 1) : nullptr,
                                k ? nullptr : d_mask_in, d_segment + (size_t)k * n, rm, d_original_mask + (size_t)k * n,
                                d_spec_info + (size_t)k * APAP_SPECTRAL_INFO, d_status, d_work, spec_bytes, stream, sync_each);
        if (rc) return rc;
        model_launch(L, sc, d_src, d_dst, rm, d_H + 9 * k, d_info + (size_t)k * APAP_MODEL_INFO, d_status, d_model_work, s);
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return apap::hip_fail(e, "apap_spectral_em_device launch");
    return APAP_OK;
}


}  // namespace apap
