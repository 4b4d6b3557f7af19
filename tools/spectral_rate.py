#!/usr/bin/env python3
"""Time the spectral weights (cvx_proj_amd.spectral_method.spectral_weights, host-buffer form) on the GPU.

    python tools/spectral_rate.py [--sizes 500 2000 5000 20000] [--reps 5] [--ref]

One JSON line per n: seconds per call (host clock around the synchronous call, after one warm-up call; the call ends in a
device synchronise), the Lanczos steps, the compute floor of the matrix-free products (n^2 entries x steps x 15 float32
operations per entry over the 157.3 TFLOP/s float32 vector peak), and, with --ref and where it fits, the time of the same
computation done the reference's way on this host's CPU (dense float64 M and a full np.linalg.svd), which is what
calculate_M spends its time on.  Inputs: seeded synthetic matches (a translation, 0.5 px noise, 20 % outliers)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

OPS_PER_ENTRY = 15          # 4 differences, 4 squares, 2 sums, s - d, its square, x rcp, 4.5 - q, max (float32)
PEAK_F32 = 157.3e12


def synth(n, seed=0):
    rng = np.random.default_rng(seed)
    src = rng.uniform(0, 1000, (n, 2))
    dst = src + [35.0, -18.0] + rng.normal(0, 0.5, (n, 2))
    out = rng.random(n) < 0.2
    dst[out] = rng.uniform(0, 1000, (out.sum(), 2))
    c = rng.integers(0, 120, (n, 128)).astype(np.float32)
    o = np.clip(c + rng.integers(-25, 25, (n, 128)), 0, 255).astype(np.float32)
    F = np.array([[0, -1e-6, 1e-3], [1e-6, 0, -2e-3], [-1e-3, 2e-3, 1e-2]])
    return src.astype(np.float32), dst.astype(np.float32), c, o, F, (~out).astype(np.float32)


def reference_way(src, dst, c, o, F):
    """The dense M and the full SVD of spectral_method.py:104-125, in numpy (float64 M, as the reference builds it)."""
    n = len(src)
    c = c / np.linalg.norm(c, axis=-1, keepdims=True)
    o = o / np.linalg.norm(o, axis=-1, keepdims=True)
    hs = np.hstack((src, np.ones((n, 1))))
    hd = np.hstack((dst, np.ones((n, 1))))
    M = np.diag(np.sum(c * o, -1) + 0.5 / (1. + np.abs(np.sum(hd * (F @ hs.T).T, -1))))
    s = np.sum((src.reshape(-1, 1, 2) - src.reshape(1, -1, 2)) ** 2, -1)
    d = np.sum((dst.reshape(-1, 1, 2) - dst.reshape(1, -1, 2)) ** 2, -1)
    off = np.maximum(4.5 - ((s - d) ** 2) * (1 / 2 / 30.0 ** 2), 0.)
    np.fill_diagonal(off, 0.)
    M += off
    U, _, _ = np.linalg.svd(M)
    return U[:, 0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[500, 2000, 5000, 20000])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--ref", action="store_true", help="also time the reference's dense way on the CPU (n <= 5000)")
    a = ap.parse_args()
    from cvx_proj_amd import _native
    from cvx_proj_amd.spectral_method import spectral_weights
    if _native.lib().apap_device_count() < 1:
        raise SystemExit("spectral_rate: no HIP device (this tool measures the GPU; it has no CPU mode)")
    for n in a.sizes:
        src, dst, c, o, F, mask = synth(n)
        r = spectral_weights(src, dst, c, o, F, mask=mask)           # warm-up
        times = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            r = spectral_weights(src, dst, c, o, F, mask=mask)
            times.append(time.perf_counter() - t0)
        floor = float(n) * n * r.steps * OPS_PER_ENTRY / PEAK_F32
        rec = {"n": n, "seconds_per_call_median": float(np.median(times)), "seconds_per_call_min": float(min(times)),
               "reps": a.reps, "lanczos_steps": r.steps, "restarts": r.restarts, "converged": r.converged,
               "residual": r.residual, "gap": r.gap, "matvec_compute_floor_s": floor,
               "floor_share_of_call": floor / float(np.median(times))}
        if a.ref and n <= 5000:
            t0 = time.perf_counter()
            reference_way(src, dst, c, o, F)
            rec["reference_cpu_seconds"] = time.perf_counter() - t0
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
