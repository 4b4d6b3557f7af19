#!/usr/bin/env python3
"""Time the Huber M-step beside the least-squares and SDP M-steps (host-buffer apap_model_solve) on the GPU.

    python tools/huber_rate.py [--sizes 500 2000 5000] [--reps 20] [--M 0.5] [--out profiles/huber_rate.jsonl]

For every n and input (a synthetic 4K pair with 1 px noise: 'clean', and 'moderate' with 5 % of the matches displaced by
5 .. 30 px) the three modes are called in one alternation - HUBER, LMS, SDP, HUBER, LMS, SDP, .. - after one warm-up call
each, so that they share the clock state; one JSON line per (input, n, mode): the median and the minimum of the host clock
around the synchronous call, the iteration count and the gap reached.  The lines go to stdout and, with --out, to that file.
Per-kernel times (k_model_tsqr, k_model_solve, k_model_huber) come from running this tool under a kernel trace."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def synth(n, kind, seed=0):
    rng = np.random.default_rng(seed)
    pc = rng.uniform(0, 1, (n, 2)) * [3840, 2160]
    H = np.array([[0.97, 0.04, 35.0], [-0.03, 1.01, -12.0], [2e-6, -1e-6, 1.0]])
    q = np.hstack([pc, np.ones((n, 1))]) @ H.T
    po = q[:, :2] / q[:, 2:] + rng.normal(0, 1.0, (n, 2))
    if kind == "moderate":
        bad = rng.random(n) < 0.05
        ang = rng.uniform(0, 2 * np.pi, n)
        mag = rng.uniform(5, 30, n)
        po[bad] += (mag[:, None] * np.stack([np.cos(ang), np.sin(ang)], axis=1))[bad]
    return pc.astype(np.float32), po.astype(np.float32), (0.3 + 0.7 * rng.random(n)).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[500, 2000, 5000])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--M", type=float, default=0.5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    try:
        import torch        # noqa: F401  before the library: one HIP runtime in the process (cvx_proj_amd/_native.py)
    except ImportError:
        pass
    from cvx_proj_amd import _native
    from cvx_proj_amd.model import result_of
    if _native.lib().apap_device_count() < 1:
        raise SystemExit("huber_rate: no HIP device (this tool measures the GPU; it has no CPU mode)")
    modes = (("huber", _native.model_params(_native.MODEL_HUBER, a.M, floor=None)),
             ("lms", _native.model_params(_native.MODEL_LMS, floor=None)),
             ("sdp", _native.model_params(_native.MODEL_SDP, a.M, a.M, floor=None)))
    lines = []
    for kind in ("clean", "moderate"):
        for n in a.sizes:
            pc, po, w = synth(n, kind)
            times = {name: [] for name, _ in modes}
            last = {}
            for name, p in modes:
                _native.model_solve(pc, po, w, p)
            for _ in range(a.reps):
                for name, p in modes:
                    t0 = time.perf_counter()
                    _, info = _native.model_solve(pc, po, w, p)
                    times[name].append(time.perf_counter() - t0)
                    last[name] = result_of(info)
            for name, _ in modes:
                r = last[name]
                lines.append({"input": kind, "n": n, "mode": name, "M": a.M, "reps": a.reps,
                              "seconds_per_call_median": float(np.median(times[name])), "seconds_per_call_min": float(min(times[name])),
                              "iterations": r.iterations, "gap": r.gap, "status": r.status, "objective": r.objective})
                print(json.dumps(lines[-1]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
