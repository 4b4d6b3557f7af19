// Batched EM loop of the spectral method: B independent problems (a pair, a set of spectral options, a set of model
// options) advance in lockstep on one stream.  The number of launches per Lanczos step and per M-step does not depend on B.
//
// Every kernel here is the body of the single-problem kernel of the same name (apap_spectral_dev.h, apap_model_dev.h) run on
// the blocks of one problem: blockIdx.y selects the problem's descriptor in device memory, blockIdx.x is the block within
// the problem, and blocks beyond the problem's own count return at once.  The bodies see the n, the block counts and the
// reduction orders of their own problem only, so every output equals the single call's bit for bit, whatever else is in
// the batch.  The matvec's rows-per-block class is a template parameter: a ragged batch takes one matvec launch per class
// present (at most 4), each over the list of the problems of that class.
//
// As in the single-problem path: no grid-wide barrier, no spin-wait, no floating-point atomics; workgroups communicate
// through kernel boundaries.  A problem's status bits go to its own status word (integer atomicOr).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "apap_internal.h"
#include "apap_model_dev.h"
#include "apap_spectral_dev.h"

namespace {

constexpr int kMaxProblems = 65535;   // grid.y
constexpr int kClasses = 4;           // rows-per-block classes of the matvec: 4, 8, 16, 32

// One problem, in device memory.  The inputs of the problems of one pair are the same arrays.
struct alignas(256) EmProb {
    SpecPtrs p;
    SpecScalars sc;
    ModelScalars msc;
    int n, m, nb_mv, nb_o;       // spec_layout(n)
    int per_block, nb;           // model_layout(n)
    const float *src, *dst, *cf, *of, *mask_in;
    const double *F;
    double *Rb;
    int *cnt;
    // outputs, round-major: round k at + 9 k, + APAP_MODEL_INFO k, + n k, + APAP_SPECTRAL_INFO k
    float *H, *ransac, *original;
    double *info, *segment, *spec_info;
    int *status;                 // the problem's own word, or NULL
};

__global__ __launch_bounds__(kSpecThreads) void k_spec_setup_b(const EmProb *__restrict__ tab, int round) {
    const EmProb &d = tab[blockIdx.y];
    if (blockIdx.x * kSpecThreads >= (unsigned)d.n) return;
    spec_setup_body(d.src, d.dst, d.cf, d.of, d.n, d.F, d.sc, round ? d.H + 9 * (round - 1) : nullptr,
                    round ? nullptr : d.mask_in, d.p, d.nb_o, blockIdx.x);
}

// `list`: the problems of rows-per-block class R
template <int R>
__global__ __launch_bounds__(kSpecThreads) void k_spec_matvec_b(const EmProb *__restrict__ tab, const int *__restrict__ list, int j) {
    const EmProb &d = tab[list[blockIdx.y]];
    if (j >= d.m || blockIdx.x >= (unsigned)d.nb_mv) return;
    spec_matvec_body<R>(d.p, d.n, j, d.nb_o, d.sc.rcp, blockIdx.x);
}

__global__ __launch_bounds__(kSpecThreads) void k_spec_orth_b(const EmProb *__restrict__ tab, int j, int pass) {
    const EmProb &d = tab[blockIdx.y];
    if (j >= d.m || blockIdx.x >= (unsigned)d.nb_o) return;
    spec_orth_body(d.p, d.n, j, pass == 1 ? d.nb_mv : d.nb_o, pass, blockIdx.x);
}

__global__ __launch_bounds__(kSpecThreads) void k_spec_tri_b(const EmProb *__restrict__ tab) {
    const EmProb &d = tab[blockIdx.x];
    spec_tri_body(d.p, d.m, d.nb_o);
}

__global__ __launch_bounds__(kSpecThreads) void k_spec_ritz_b(const EmProb *__restrict__ tab) {
    const EmProb &d = tab[blockIdx.y];
    if (blockIdx.x >= (unsigned)d.nb_o) return;
    spec_ritz_body(d.p, d.n, blockIdx.x);
}

__global__ __launch_bounds__(kFinishThreads) void k_spec_finish_b(const EmProb *__restrict__ tab, int round) {
    const EmProb &d = tab[blockIdx.x];
    const size_t at = (size_t)round * d.n;
    spec_finish_body(d.p, d.n, d.sc, d.segment + at, d.ransac + at, d.original + at, d.spec_info + (size_t)round * APAP_SPECTRAL_INFO,
                     d.status);
}

__global__ __launch_bounds__(kW) void k_model_tsqr_b(const EmProb *__restrict__ tab, int round) {
    const EmProb &d = tab[blockIdx.y];
    if (blockIdx.x >= (unsigned)d.nb) return;
    model_tsqr_body((const float2 *)d.src, (const float2 *)d.dst, LoadWeight{d.ransac + (size_t)round * d.n}, d.n, d.per_block, d.msc,
                    d.Rb, d.cnt, blockIdx.x);
}

// One wave per problem; its 55 KB of LDS let two problems share a CU.
__global__ __launch_bounds__(kW) void k_model_solve_b(const EmProb *__restrict__ tab, int round) {
    const EmProb &d = tab[blockIdx.x];
    model_solve_body(d.Rb, d.cnt, d.nb, d.msc, d.H + 9 * round, d.info + (size_t)round * APAP_MODEL_INFO, d.status);
}

// Workspace: the descriptor table | the class lists | the states (contiguous: the host-buffer form reads every `done` word
// in one copy) | per problem, the single-problem spectral layout and model layout.  Each part is a whole number of
// 256-byte units per problem, so the size is additive over problems.
constexpr size_t kListUnit = 256, kStateUnit = 256;
static_assert(sizeof(SpecState) <= kStateUnit && sizeof(EmProb) % 256 == 0, "workspace units");

size_t problem_bytes(int n) { return sizeof(EmProb) + kListUnit + kStateUnit + spec_layout(n).total + model_layout(n).total; }

int pair_len(const int *pair_offset, int pair) { return pair_offset[pair + 1] - pair_offset[pair]; }

// The host-side argument checks shared by the size query and the run; N = pair_offset[n_pairs].
int check_shape(const int *pair_offset, int n_pairs, const int *pair_of, int n_problems, const char *who) {
    if (!pair_offset || !pair_of) return apap::fail(APAP_ERR_INVALID_ARG, "%s: null pair_offset / pair_of", who);
    if (n_pairs < 1 || n_problems < 1 || n_problems > kMaxProblems)
        return apap::fail(APAP_ERR_INVALID_ARG, "%s: n_pairs=%d, n_problems=%d (need >= 1 pair, 1 .. %d problems)", who, n_pairs,
                          n_problems, kMaxProblems);
    if (pair_offset[0] < 0) return apap::fail(APAP_ERR_INVALID_ARG, "%s: pair_offset[0] = %d is negative", who, pair_offset[0]);
    for (int p = 0; p < n_pairs; ++p)
        if (pair_offset[p + 1] <= pair_offset[p] || pair_offset[p + 1] - pair_offset[p] > (1 << 26))
            return apap::fail(APAP_ERR_INVALID_ARG, "%s: pair_offset must be strictly increasing, a pair at most 2^26 matches (pair "
                                                    "%d: %d -> %d)", who, p, pair_offset[p], pair_offset[p + 1]);
    for (int b = 0; b < n_problems; ++b)
        if (pair_of[b] < 0 || pair_of[b] >= n_pairs)
            return apap::fail(APAP_ERR_INVALID_ARG, "%s: problem %d: pair %d out of range (0 .. %d)", who, b, pair_of[b], n_pairs - 1);
    return APAP_OK;
}

template <int R>
void launch_matvec(int blocks, int count, const EmProb *tab, const int *list, int j, hipStream_t s) {
    hipLaunchKernelGGL(k_spec_matvec_b<R>, dim3(blocks, count), dim3(kSpecThreads), 0, s, tab, list, j);
}

// Every argument check of the batch entry points that needs no device pointer (the messages name the problem).  With `tab`,
// it is sized to the batch and every problem's parsed scalars go to its descriptor, the batch's cycle cap to `restarts_out`.
int batch_check(const int *pair_offset, int n_pairs, const int *pair_of, const double *spec_params, const double *model_params,
                int n_problems, int em_steps, const char *who, std::vector<EmProb> *tab, int *restarts_out) {
    int rc = check_shape(pair_offset, n_pairs, pair_of, n_problems, who);
    if (rc) return rc;
    if (em_steps < 1 || em_steps > 64) return apap::fail(APAP_ERR_INVALID_ARG, "%s: em_steps %d (1 .. 64)", who, em_steps);
    if (!spec_params || !model_params) return apap::fail(APAP_ERR_INVALID_ARG, "%s: null params", who);
    if (tab) tab->assign((size_t)n_problems, EmProb{});
    int restarts = 0;
    char msg[96];
    for (int b = 0; b < n_problems; ++b) {
        snprintf(msg, sizeof msg, "%s: problem %d", who, b);
        EmProb mine, &d = tab ? (*tab)[b] : mine;
        int r;
        if ((rc = spec_check_params(spec_params + (size_t)b * APAP_SPECTRAL_PARAMS, &d.sc, &r, msg))) return rc;
        if ((rc = model_check_params(model_params + (size_t)b * APAP_MODEL_PARAMS, &d.msc, msg))) return rc;
        if ((rc = model_check_huber(d.msc, -1, msg))) return rc;
        if (b && r != restarts)
            return apap::fail(APAP_ERR_INVALID_ARG, "%s: problem %d: max_restarts %d differs from problem 0's %d (the cap fixes how "
                                                    "many cycles are enqueued: it must be equal across a batch)", who, b, r, restarts);
        restarts = r;
    }
    if (restarts_out) *restarts_out = restarts;
    return APAP_OK;
}

}  // namespace

namespace apap {

// batch_check for the host-buffer entry point (apap_capi.hip), which checks before it stages anything.
int spectral_em_batch_check(const int *pair_offset, int n_pairs, const int *pair_of, const double *spec_params,
                            const double *model_params, int n_problems, int em_steps, const char *who) {
    return batch_check(pair_offset, n_pairs, pair_of, spec_params, model_params, n_problems, em_steps, who, nullptr, nullptr);
}

// The body of apap_spectral_em_batch_device; sync_each = 1 (the host-buffer entry point) waits for every restart cycle and
// enqueues no more of a round's cycles once every problem reports `done` (same bytes: the cycles after convergence change
// nothing).
int spectral_em_batch_run(apap_ctx *ctx, const float *d_src, const float *d_dst, const float *d_c_feats, const float *d_o_feats,
                          const double *d_F, const float *d_mask_in, const int *pair_offset, int n_pairs, const int *pair_of,
                          const double *spec_params, const double *model_params, int n_problems, int em_steps, float *d_H,
                          double *d_info, double *d_segment, float *d_ransac_mask, float *d_original_mask, double *d_spec_info,
                          int *d_status, void *d_work, size_t work_bytes, void *stream, int sync_each) {
    const char *who = "apap_spectral_em_batch_device";
    std::vector<EmProb> tab;
    int restarts = 0;
    int rc = batch_check(pair_offset, n_pairs, pair_of, spec_params, model_params, n_problems, em_steps, who, &tab, &restarts);
    if (rc) return rc;
    const int B = n_problems;
    std::vector<int> lists((size_t)B);
    size_t need = 0;
    for (int b = 0; b < B; ++b) {
        model_em_scalars(tab[b].msc);   // as apap_spectral_em_device
        need += problem_bytes(pair_len(pair_offset, pair_of[b]));
    }
    if (!d_src || !d_dst || !d_c_feats || !d_o_feats || !d_F || !d_mask_in || !d_work)
        return apap::fail(APAP_ERR_INVALID_ARG, "%s: null device pointer", who);
    if (!d_H || !d_info || !d_segment || !d_ransac_mask || !d_original_mask || !d_spec_info)
        return apap::fail(APAP_ERR_INVALID_ARG, "%s: null output pointer", who);
    if (work_bytes < need) return apap::fail(APAP_ERR_WORKSPACE, "%s: workspace %zu < %zu bytes", who, work_bytes, need);
    if (((uintptr_t)d_work & 255) != 0 || ((uintptr_t)d_src & 7) != 0 || ((uintptr_t)d_dst & 7) != 0)
        return apap::fail(APAP_ERR_INVALID_ARG, "%s: workspace must be 256-byte and points 8-byte aligned", who);

    char *w = (char *)d_work;
    EmProb *d_tab = (EmProb *)w;
    int *d_lists = (int *)(w + (size_t)B * sizeof(EmProb));
    SpecState *d_states = (SpecState *)((char *)d_lists + (size_t)B * kListUnit);
    size_t off = (size_t)B * (sizeof(EmProb) + kListUnit + kStateUnit);
    size_t match_off = 0;   // matches of the problems before b
    int max_m = 0, max_setup = 0, max_nb_o = 0, max_nb = 0;
    int cls_count[kClasses] = {0, 0, 0, 0}, cls_blocks[kClasses] = {0, 0, 0, 0}, cls_begin[kClasses];
    auto cls_of = [](int R) { return R == 4 ? 0 : R == 8 ? 1 : R == 16 ? 2 : 3; };
    for (int b = 0; b < B; ++b) {
        const int pair = pair_of[b], n = pair_len(pair_offset, pair);
        const size_t at = (size_t)pair_offset[pair];
        const SpecLayout L = spec_layout(n);
        const ModelLayout M = model_layout(n);
        EmProb &d = tab[b];
        d.p = spec_ptrs(L, w + off);
        d.p.st = d_states + b;
        off += L.total;
        d.Rb = (double *)(w + off + M.R);
        d.cnt = (int *)(w + off + M.cnt);
        off += M.total;
        d.n = n;
        d.m = L.m;
        d.nb_mv = L.nb_mv;
        d.nb_o = L.nb_o;
        d.per_block = M.per_block;
        d.nb = M.nb;
        d.src = d_src + at * 2;
        d.dst = d_dst + at * 2;
        d.cf = d_c_feats + at * APAP_SPECTRAL_DIM;
        d.of = d_o_feats + at * APAP_SPECTRAL_DIM;
        d.mask_in = d_mask_in + at;
        d.F = d_F + (size_t)pair * 9;
        d.H = d_H + (size_t)b * em_steps * 9;
        d.info = d_info + (size_t)b * em_steps * APAP_MODEL_INFO;
        d.spec_info = d_spec_info + (size_t)b * em_steps * APAP_SPECTRAL_INFO;
        d.segment = d_segment + match_off * em_steps;
        d.ransac = d_ransac_mask + match_off * em_steps;
        d.original = d_original_mask + match_off * em_steps;
        d.status = d_status ? d_status + b : nullptr;
        match_off += (size_t)n;
        max_m = std::max(max_m, L.m);
        max_setup = std::max(max_setup, (n + kSpecThreads - 1) / kSpecThreads);
        max_nb_o = std::max(max_nb_o, L.nb_o);
        max_nb = std::max(max_nb, M.nb);
        const int c = cls_of(L.R);
        cls_count[c] += 1;
        cls_blocks[c] = std::max(cls_blocks[c], L.nb_mv);
    }
    for (int c = 0, at = 0; c < kClasses; ++c) {
        cls_begin[c] = at;
        at += cls_count[c];
    }
    {
        int fill[kClasses] = {cls_begin[0], cls_begin[1], cls_begin[2], cls_begin[3]};
        for (int b = 0; b < B; ++b) lists[(size_t)fill[cls_of(spec_rows_per_block(tab[b].n))]++] = b;
    }
    hipStream_t s = (hipStream_t)stream;
    // both tables go up from pageable memory in stream order: the copies return once their source has been consumed
    hipError_t e = hipMemcpyAsync(d_tab, tab.data(), (size_t)B * sizeof(EmProb), hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(d_lists, lists.data(), (size_t)B * sizeof(int), hipMemcpyHostToDevice, s);
    if (e != hipSuccess) return apap::hip_fail(e, "apap_spectral_em_batch_device: descriptor upload");
    std::vector<SpecState> states(sync_each ? (size_t)B : 0);
    for (int k = 0; k < em_steps; ++k) {
        {
            apap::ProfScope prof(ctx, APAP_PROF_SPECTRAL, s);
            hipLaunchKernelGGL(k_spec_setup_b, dim3(max_setup, B), dim3(kSpecThreads), 0, s, d_tab, k);
            for (int c = 0; c < restarts; ++c) {
                // one restart cycle of every problem: a problem of m < max_m vectors sits out the steps beyond its own
                for (int j = 0; j < max_m; ++j) {
                    if (cls_count[0]) launch_matvec<4>(cls_blocks[0], cls_count[0], d_tab, d_lists + cls_begin[0], j, s);
                    if (cls_count[1]) launch_matvec<8>(cls_blocks[1], cls_count[1], d_tab, d_lists + cls_begin[1], j, s);
                    if (cls_count[2]) launch_matvec<16>(cls_blocks[2], cls_count[2], d_tab, d_lists + cls_begin[2], j, s);
                    if (cls_count[3]) launch_matvec<32>(cls_blocks[3], cls_count[3], d_tab, d_lists + cls_begin[3], j, s);
                    hipLaunchKernelGGL(k_spec_orth_b, dim3(max_nb_o, B), dim3(kSpecThreads), 0, s, d_tab, j, 1);
                    hipLaunchKernelGGL(k_spec_orth_b, dim3(max_nb_o, B), dim3(kSpecThreads), 0, s, d_tab, j, 2);
                }
                hipLaunchKernelGGL(k_spec_tri_b, dim3(B), dim3(kSpecThreads), 0, s, d_tab);
                hipLaunchKernelGGL(k_spec_ritz_b, dim3(max_nb_o, B), dim3(kSpecThreads), 0, s, d_tab);
                if (sync_each) {
                    e = hipMemcpyAsync(states.data(), d_states, (size_t)B * sizeof(SpecState), hipMemcpyDeviceToHost, s);
                    if (e == hipSuccess) e = hipStreamSynchronize(s);
                    if (e != hipSuccess) return apap::hip_fail(e, "apap_spectral_em_batch_device: cycle");
                    bool all = true;
                    for (int b = 0; b < B; ++b) all = all && states[b].done;
                    if (all) break;
                }
            }
            hipLaunchKernelGGL(k_spec_finish_b, dim3(B), dim3(kFinishThreads), 0, s, d_tab, k);
        }
        hipLaunchKernelGGL(k_model_tsqr_b, dim3(max_nb, B), dim3(kW), 0, s, d_tab, k);
        hipLaunchKernelGGL(k_model_solve_b, dim3(B), dim3(kW), 0, s, d_tab, k);
    }
    e = hipGetLastError();
    if (e != hipSuccess) return apap::hip_fail(e, "apap_spectral_em_batch_device launch");
    return APAP_OK;
}

}  // namespace apap

extern "C" {

size_t apap_spectral_em_batch_workspace_bytes(const int *pair_offset, int n_pairs, const int *pair_of, int n_problems) {
    if (!pair_offset || !pair_of || n_pairs < 1 || n_problems < 1) return 0;
    if (check_shape(pair_offset, n_pairs, pair_of, n_problems, "apap_spectral_em_batch_workspace_bytes")) return 0;
    size_t total = 0;
    for (int b = 0; b < n_problems; ++b) total += problem_bytes(pair_len(pair_offset, pair_of[b]));
    return total;
}

int apap_spectral_em_batch_device(apap_ctx *ctx, const float *d_src, const float *d_dst, const float *d_c_feats,
                                  const float *d_o_feats, const double *d_F, const float *d_mask_in, const int *pair_offset,
                                  int n_pairs, const int *pair_of, const double *spec_params, const double *model_params,
                                  int n_problems, int em_steps, float *d_H, double *d_info, double *d_segment, float *d_ransac_mask,
                                  float *d_original_mask, double *d_spec_info, int *d_status, void *d_work, size_t work_bytes,
                                  void *stream) {
    return apap::spectral_em_batch_run(ctx, d_src, d_dst, d_c_feats, d_o_feats, d_F, d_mask_in, pair_offset, n_pairs, pair_of,
                                       spec_params, model_params, n_problems, em_steps, d_H, d_info, d_segment, d_ransac_mask,
                                       d_original_mask, d_spec_info, d_status, d_work, work_bytes, stream, 0);
}

}  // extern "C"
