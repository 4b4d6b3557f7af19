// Robust moving DLT: the M-step's weighted solve (LMS or the exact SDP, apap_model_dev.h) for every cell of a mesh, with
// the cell's moving-DLT weight (apap_weight_dev.h: cell_weight, the code of apap_local_weights) times an optional
// per-match weight as the weight vector.  It answers the comment above the SVD of the reference's cell loop
// (pyviz/apap.py:155-157): "what we should do is to replace this place / if we are to compute one SDP at a time ...".
//
//   L1 k_local_tsqr   grid (TSQR blocks, cells), one wave per block: model_tsqr_body with the weight of match i for the
//                     block's cell computed on the fly, w = float32(cell_weight(vertex, pts_c[i])) * match_weights[i] (one
//                     float32 multiply; -ffp-contract=off, so it cannot fuse with the row products that follow).  The
//                     cells x n weight tensor never exists.
//   L2 k_local_solve  one wave per cell: model_solve_body on the cell's block factors.  55 KB of LDS per wave: two cells
//                     per CU (derived from the LDS size: up to 512 cells in flight on 256 CUs).
//
// Both bodies see one cell's factors, counts and reduction order only, so a cell's H, info and status equal the bytes of
// apap_model_solve_device on that cell's weight vector, whatever else is in the call and wherever a chunk boundary falls.
// Cells are processed in chunks of as many cells as the workspace holds (kLocalChunk by apap_local_model_workspace_bytes):
// two launches per chunk, none in a loop over cells.  No floating-point atomics, no grid-wide barrier, no spin-wait; a
// cell's status bits go to its own word (integer atomicOr).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>

#include "apap_internal.h"
#include "apap_model_dev.h"
#include "apap_weight_dev.h"

namespace {

constexpr int kLocalChunk = APAP_LOCAL_MODEL_CHUNK;   // cells whose scratch apap_local_model_workspace_bytes asks for
constexpr int kMaxGridY = 65535;
constexpr size_t kInfoUnit = 256;                     // a cell's info block when the caller wants none
static_assert(APAP_MODEL_INFO * sizeof(double) <= kInfoUnit && kLocalChunk >= 4096 && kLocalChunk <= kMaxGridY, "chunk");

// a cell's scratch: the block factors and counts of model_layout(n), then the spare info block
size_t cell_bytes(const ModelLayout &L) { return L.total + kInfoUnit; }

// The weight of match i for one cell.  (float)W rounds the float64 weight once; the product is one float32 multiply.
struct LocalWeight {
    double vx, vy, inv_sigma, gamma;
    const float *__restrict__ mw;   // NULL: none
    __device__ __forceinline__ float operator()(int i, float2 c) const {
        const float w = (float)cell_weight(vx, vy, (double)c.x, (double)c.y, inv_sigma, gamma);
        return mw ? w * mw[i] : w;
    }
};

struct LocalArgs {
    const float2 *pc, *po;
    const float *mw;
    const double *vertices;   // this chunk's first vertex
    int n, per_block, nb;
    double gamma, inv_sigma;
    ModelScalars sc;
    char *work;               // this chunk's scratch: cell k at work + k * stride
    size_t stride, off_R, off_cnt, off_info;
    float *H;                 // this chunk's first cell
    double *info;             // NULL: the spare block of the cell's scratch
    int *status;              // NULL: none
};

__global__ __launch_bounds__(kW) void k_local_tsqr(const LocalArgs a) {
    const unsigned cell = blockIdx.y;
    char *w = a.work + (size_t)cell * a.stride;
    const LocalWeight weight{a.vertices[2 * (size_t)cell], a.vertices[2 * (size_t)cell + 1], a.inv_sigma, a.gamma, a.mw};
    model_tsqr_body(a.pc, a.po, weight, a.n, a.per_block, a.sc, (double *)(w + a.off_R), (int *)(w + a.off_cnt), blockIdx.x);
}

__global__ __launch_bounds__(kW) void k_local_solve(const LocalArgs a) {
    const unsigned cell = blockIdx.x;
    char *w = a.work + (size_t)cell * a.stride;
    double *info = a.info ? a.info + (size_t)cell * APAP_MODEL_INFO : (double *)(w + a.off_info);
    model_solve_body((const double *)(w + a.off_R), (const int *)(w + a.off_cnt), a.nb, a.sc, a.H + (size_t)cell * 9, info,
                     a.status ? a.status + cell : nullptr);
}

// Every argument check of the two entry points that needs no pointer into device or caller memory but `params`; the parsed
// scalars go to `sc_out` when it is given.
int local_check(int n, int cells, double gamma, double sigma, const double *params, const char *who, ModelScalars *sc_out) {
    ModelScalars mine, &sc = sc_out ? *sc_out : mine;
    int rc = model_check_params(params, &sc, who);
    if (rc) return rc;
    if ((rc = model_check_huber(sc, -1, who))) return rc;
    if (sc.du < 0.0 || sc.dv < 0.0) return apap::fail(APAP_ERR_INVALID_ARG, "%s: du / dv negative", who);
    if ((rc = model_check_n(n, who))) return rc;
    if (cells < 1 || cells > APAP_LOCAL_MODEL_MAX_CELLS)
        return apap::fail(APAP_ERR_INVALID_ARG, "%s: cells=%d (need 1 .. %d)", who, cells, APAP_LOCAL_MODEL_MAX_CELLS);
    if (!(sigma > 0.0) || !std::isfinite(sigma)) return apap::fail(APAP_ERR_INVALID_ARG, "%s: sigma %g (need a finite sigma > 0)", who, sigma);
    if (std::isnan(gamma)) return apap::fail(APAP_ERR_INVALID_ARG, "%s: gamma is NaN", who);
    return APAP_OK;
}

}  // namespace

namespace apap {

// local_check for the host-buffer entry point (apap_capi.hip), which checks before it stages anything.
int local_model_check(int n, int cells, double gamma, double sigma, const double *params, const char *who) {
    return local_check(n, cells, gamma, sigma, params, who, nullptr);
}

}  // namespace apap

extern "C" {

size_t apap_local_model_workspace_bytes(int n, int cells) {
    if (n < 1 || n > kModelMaxN || cells < 1 || cells > APAP_LOCAL_MODEL_MAX_CELLS) return 0;
    return (size_t)std::min(cells, kLocalChunk) * cell_bytes(model_layout(n));
}

int apap_local_model_solve_device(apap_ctx *ctx, const float *d_pts_c, const float *d_pts_o, const float *d_match_weights, int n,
                                  const double *d_vertices, int cells, double gamma, double sigma, const double *params,
                                  float *d_H, double *d_info, int *d_status, void *d_work, size_t work_bytes, void *stream) {
    const char *who = "apap_local_model_solve_device";
    LocalArgs a{};
    int rc = local_check(n, cells, gamma, sigma, params, who, &a.sc);
    if (rc) return rc;
    if (!d_pts_c || !d_pts_o || !d_vertices || !d_H || !d_work) return apap::fail(APAP_ERR_INVALID_ARG, "%s: null device pointer", who);
    const ModelLayout L = model_layout(n);
    const size_t unit = cell_bytes(L);
    if (work_bytes < unit) return apap::fail(APAP_ERR_WORKSPACE, "%s: workspace %zu < %zu bytes (one cell)", who, work_bytes, unit);
    if (((uintptr_t)d_work & 255) != 0 || ((uintptr_t)d_pts_c & 7) != 0 || ((uintptr_t)d_pts_o & 7) != 0 ||
        ((uintptr_t)d_vertices & 7) != 0)
        return apap::fail(APAP_ERR_INVALID_ARG, "%s: workspace must be 256-byte, points and vertices 8-byte aligned", who);
    const int chunk = (int)std::min<size_t>(std::min<size_t>(work_bytes / unit, (size_t)cells), (size_t)kMaxGridY);

    a.pc = (const float2 *)d_pts_c;
    a.po = (const float2 *)d_pts_o;
    a.mw = d_match_weights;
    a.n = n;
    a.per_block = L.per_block;
    a.nb = L.nb;
    a.gamma = gamma;
    a.inv_sigma = 1.0 / (sigma * sigma);   // apap.py:142, as apap_weights_device
    a.work = (char *)d_work;
    a.stride = unit;
    a.off_R = L.R;
    a.off_cnt = L.cnt;
    a.off_info = L.total;
    hipStream_t s = (hipStream_t)stream;
    for (int c0 = 0; c0 < cells; c0 += chunk) {   // over chunks, never over cells
        const int nc = std::min(chunk, cells - c0);
        a.vertices = d_vertices + (size_t)2 * c0;
        a.H = d_H + (size_t)9 * c0;
        a.info = d_info ? d_info + (size_t)APAP_MODEL_INFO * c0 : nullptr;
        a.status = d_status ? d_status + c0 : nullptr;
        {
            apap::ProfScope prof(ctx, APAP_PROF_ASSEMBLE, s);   // the weighted reduction, as K1
            hipLaunchKernelGGL(k_local_tsqr, dim3(L.nb, nc), dim3(kW), 0, s, a);
        }
        {
            apap::ProfScope prof(ctx, APAP_PROF_EIGEN, s);      // the per-cell solve, as K2
            hipLaunchKernelGGL(k_local_solve, dim3(nc), dim3(kW), 0, s, a);
        }
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return apap::hip_fail(e, "apap_local_model_solve_device launch");
    return APAP_OK;
}

}  // extern "C"
