#!/usr/bin/env python3
"""Time the M-step (cvx_proj_amd.model: SDPSolver / LMSSolver, host-buffer form) and the EM loop (spectral_em) on the GPU.

    python tools/model_rate.py [--sizes 500 2000 5000] [--reps 5] [--em-n 2000] [--batch B [B ...]]

One JSON line per (solver, n): seconds per call (host clock around the synchronous call, after one warm-up call), the
interior-point iterations and the relative gap reached; then one line per form of a two-round SDP EM loop at --em-n matches:
the host-buffer spectral_em (waits for each spectral restart cycle, stops at convergence) and, when torch is installed, the
resident resident.hip_spectral_em (enqueues every cycle, then one synchronise), and for comparison the chain of public calls
it replaces (spectral_weights -> model_solve, twice).  Per-kernel times (k_model_tsqr, k_model_solve) come from running this
tool under `rocprofv3 --kernel-trace`; dispatches come in this order: per n four SDP then four LMS solves, then four calls of
each EM form (two rounds each) and of the chain.
With --batch (default off) the tool prints, instead of the lines above, one JSON line per B: a grid of B parameter sets
(two-round SDP EM loops; fluc and epi_weight vary) on the --em-n synthetic pair, timed three ways in this process after one
warm-up each - the batched host-buffer call (spectral_method.spectral_em_batch), the batched resident call
(resident.hip_spectral_em_batch, one synchronise) and a loop of B spectral_em calls -, the ratio loop / batch of the medians,
and whether every problem's final H equals the loop's bit for bit.
Inputs: seeded synthetic matches (a homography, 1 px noise, 20 % outliers, uniform weights in [0.1, 1))."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tools.spectral_rate import synth as spectral_synth  # noqa: E402


def synth(n, seed=0):
    rng = np.random.default_rng(seed)
    pc = rng.uniform(0, 1280, (n, 2))
    H = np.array([[0.97, 0.04, 35.0], [-0.03, 1.01, -12.0], [2e-5, -1e-5, 1.0]])
    q = np.hstack([pc, np.ones((n, 1))]) @ H.T
    po = q[:, :2] / q[:, 2:] + rng.normal(0, 1.0, (n, 2))
    out = rng.random(n) < 0.2
    po[out] = rng.uniform(0, 1280, (out.sum(), 2))
    return pc.astype(np.float32), po.astype(np.float32), (rng.random(n) * 0.9 + 0.1).astype(np.float32)


def timed(fn, reps):
    fn()
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        times.append(time.perf_counter() - t0)
    return out, times


def grid_options(B):
    """B distinct parameter sets: fluc varies fastest over 9 values, epi_weight over the rest."""
    return [dict(fluc=0.4 + 0.1 * (b % 9), epi_weight=0.25 + 0.05 * (b // 9)) for b in range(B)]


def batch_line(B, a, torch):
    import warnings

    from cvx_proj_amd import _native
    from cvx_proj_amd.spectral_method import spectral_em, spectral_em_batch
    src, dst, c, o, F, mask = spectral_synth(a.em_n)
    pair = (src, dst, c, o, F, mask)
    options = grid_options(B)
    problems = [(0, opt) for opt in options]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        got, t_batch = timed(lambda: spectral_em_batch([pair], problems, em_steps=2), a.reps)
        want, t_loop = timed(lambda: [spectral_em(src, dst, c, o, F, em_steps=2, mask=mask, **opt) for opt in options], a.reps)
    same = [g.rounds[-1].H_pred.tobytes() == w.rounds[-1].H_pred.tobytes() for g, w in zip(got, want)]
    line = {"em_batch": B, "em_steps": 2, "solver": "sdp", "n": a.em_n, "reps": a.reps,
            "batch_seconds_median": float(np.median(t_batch)), "batch_seconds_min": float(min(t_batch)),
            "loop_seconds_median": float(np.median(t_loop)), "loop_seconds_min": float(min(t_loop)),
            "loop_over_batch": float(np.median(t_loop) / np.median(t_batch)), "same_final_H": int(sum(same)),
            "every_final_H_equal": bool(all(same)), "ipm_iterations_max": max(r.model.iterations for g in got for r in g.rounds),
            "restarts_max": max(r.spectral.restarts for g in got for r in g.rounds)}
    if torch is not None and torch.cuda.is_available():
        from cvx_proj_amd import resident
        dev = torch.device("cuda", 0)
        t = [torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (src, dst, c, o, F[None], mask)]
        sp = np.stack([_native.spectral_params(epi_weight=opt["epi_weight"]) for opt in options])
        mp = np.stack([_native.model_params(_native.MODEL_SDP, opt["fluc"], opt["fluc"]) for opt in options])
        work = torch.empty(resident.em_batch_workspace_bytes([a.em_n], [0] * B), dtype=torch.uint8, device=dev)
        status = torch.zeros(B, dtype=torch.int32, device=dev)

        def run():
            out = resident.hip_spectral_em_batch(*t, [a.em_n], [0] * B, sp, mp, 2, status=status, work=work)
            torch.cuda.synchronize()
            return out
        out, t_res = timed(run, a.reps)
        H = out[0].cpu().numpy()
        line.update({"resident_seconds_median": float(np.median(t_res)), "resident_seconds_min": float(min(t_res)),
                     "resident_final_H_equal": bool(all(H[b, -1].tobytes() == want[b].rounds[-1].H_pred.tobytes() for b in range(B)))})
    print(json.dumps(line), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[500, 2000, 5000])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--em-n", type=int, default=2000)
    ap.add_argument("--batch", type=int, nargs="+", default=None, metavar="B",
                    help="time a grid of B parameter sets as one batched call against a loop of B spectral_em calls")
    a = ap.parse_args()
    try:
        import torch        # before the library: one HIP runtime in the process (cvx_proj_amd/_native.py)
    except ImportError:
        torch = None
    from cvx_proj_amd import _native
    from cvx_proj_amd.model import LMSSolver, SDPSolver
    from cvx_proj_amd.spectral_method import spectral_em
    if _native.lib().apap_device_count() < 1:
        raise SystemExit("model_rate: no HIP device (this tool measures the GPU; it has no CPU mode)")
    if a.batch:
        for B in a.batch:
            batch_line(B, a, torch)
        return
    for n in a.sizes:
        pc, po, w = synth(n)
        for name, solver in (("sdp", SDPSolver(8000, 0.5, 0.5)), ("lms", LMSSolver(8000))):
            _, times = timed(lambda: solver.solve(pc, po, w, verbose=0), a.reps)
            r = solver.last
            print(json.dumps({"solver": name, "n": n, "seconds_per_call_median": float(np.median(times)),
                              "seconds_per_call_min": float(min(times)), "reps": a.reps, "ipm_iterations": r.iterations,
                              "gap": r.gap, "status": r.status}), flush=True)
    src, dst, c, o, F, mask = spectral_synth(a.em_n)
    em, times = timed(lambda: spectral_em(src, dst, c, o, F, em_steps=2, fluc=0.5, mask=mask), a.reps)
    print(json.dumps({"em_steps": 2, "form": "host-buffer spectral_em", "solver": "sdp", "n": a.em_n,
                      "seconds_per_call_median": float(np.median(times)), "seconds_per_call_min": float(min(times)),
                      "reps": a.reps, "ipm_iterations": [r.model.iterations for r in em.rounds],
                      "gap": [r.model.gap for r in em.rounds], "lanczos_steps": [r.spectral.steps for r in em.rounds],
                      "restarts": [r.spectral.restarts for r in em.rounds], "selected": [r.model.count for r in em.rounds]}),
          flush=True)
    if torch is not None and torch.cuda.is_available():
        from cvx_proj_amd import resident
        dev = torch.device("cuda", 0)
        t = [torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (src, dst, c, o, F, mask)]
        sp = _native.spectral_params()
        mp = _native.model_params(_native.MODEL_SDP, 0.5, 0.5)
        work = torch.empty(resident.spectral_workspace_bytes(a.em_n) + resident.model_workspace_bytes(a.em_n), dtype=torch.uint8,
                           device=dev)

        def run():
            out = resident.hip_spectral_em(*t[:5], sp, mp, 2, t[5], work=work)
            torch.cuda.synchronize()
            return out
        _, times = timed(run, a.reps)
        print(json.dumps({"em_steps": 2, "form": "resident hip_spectral_em", "solver": "sdp", "n": a.em_n,
                          "seconds_per_call_median": float(np.median(times)), "seconds_per_call_min": float(min(times)),
                          "reps": a.reps}), flush=True)
    from cvx_proj_amd.spectral_method import model_solve, spectral_weights

    class KP:
        def __init__(self, p):
            self.pt = (float(p[0]), float(p[1]))

    class DM:
        def __init__(self, i):
            self.queryIdx = self.trainIdx = i
    kc, ko, m = [KP(p) for p in src], [KP(p) for p in dst], [DM(i) for i in range(a.em_n)]

    def chain():
        Hg = None
        for _ in range(2):
            r = spectral_weights(src, dst, c, o, F, Hg=Hg, mask=None if Hg is not None else mask)
            Hg = model_solve(kc, ko, m, r.ransac_mask, param=0.5, lms=False)
        return Hg
    H_chain, times = timed(chain, a.reps)
    print(json.dumps({"em_steps": 2, "form": "chain of public calls (spectral_weights -> model_solve)", "solver": "sdp",
                      "n": a.em_n, "seconds_per_call_median": float(np.median(times)), "seconds_per_call_min": float(min(times)),
                      "reps": a.reps, "same_H_as_spectral_em": bool(np.array_equal(H_chain, em.rounds[-1].H_pred))}), flush=True)


if __name__ == "__main__":
    main()
