#!/usr/bin/env python3
"""Time the fundamental-matrix estimator (cvx_proj_amd.resident.hip_fundamental: five launches - boxes, 2048 eight-point
hypotheses, scoring, selection, re-fit) on the GPU, beside the seed homography's RANSAC (``apap_ransac_device``: three launches)
on the same matches as the yardstick, the two alternating call by call.

    python tools/fundamental_rate.py [--reps 20] [--warmup 3] [--out profiles/fundamental_rate.jsonl]

One JSON line per row, printed and written to --out (afresh: the file holds one run).  Rows: n = 500, 2000 and 20 000 matches at
2048 iterations; 4 pairs of 2000 in one batched call against 4 single calls.  Synthetic two-view matches (0.5 px noise, 30 %
contaminated), on the device before the clock starts, workspaces allocated once.  Every call is bracketed by two events on its
stream; median and minimum of --reps calls after --warmup.  Timing is reported, not judged: the tool fails only when the batched
call and the single calls give different bytes."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ITERATIONS = 2048


def scene(n, seed):
    """Matches of a random 3-D scene between two 4K views, 0.5 px noise, 30 % of the ``dst`` replaced by random points."""
    rng = np.random.default_rng(seed)
    K = np.array([[3000.0, 0, 1920], [0, 3000.0, 1080], [0, 0, 1]])
    P = np.column_stack([rng.uniform(-50, 50, n), rng.uniform(-30, 30, n), rng.uniform(40, 120, n)])
    a, b = 0.05, 0.03
    R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]]) @ \
        np.array([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]])
    Q = (P - [6.0, 1.5, 0.5]) @ R
    src = (P / P[:, 2:]) @ K.T
    dst = (Q / Q[:, 2:]) @ K.T
    src, dst = src[:, :2] + rng.normal(0, 0.5, (n, 2)), dst[:, :2] + rng.normal(0, 0.5, (n, 2))
    bad = rng.permutation(n)[:int(0.3 * n)]
    dst[bad] = rng.uniform(0, 1, (len(bad), 2)) * [3839, 2159]
    return src.astype(np.float32), dst.astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fundamental_rate.jsonl"))
    a = ap.parse_args()
    if a.reps < 20 or a.warmup < 3:
        raise SystemExit("fundamental_rate: at least 20 timed calls after 3 warm-ups")
    import torch      # before the library: one HIP runtime per process
    from cvx_proj_amd import _native, resident
    if _native.lib().apap_device_count() < 1 or not torch.cuda.is_available():
        raise SystemExit("fundamental_rate: no HIP device (this tool measures the GPU; it has no CPU mode)")
    dev = torch.device("cuda", 0)
    lib = _native.lib()

    def event_timed(fns):
        """The listed calls in alternation, each bracketed by events: a list of millisecond lists, one per call."""
        times = [[] for _ in fns]
        for rep in range(a.warmup + a.reps):
            for k, fn in enumerate(fns):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                if rep >= a.warmup:
                    times[k].append(e0.elapsed_time(e1))
        return times

    def stats(prefix, ms):
        return {prefix + "_us_median": float(np.median(ms)) * 1e3, prefix + "_us_min": float(min(ms)) * 1e3}

    def ransac_call(s, d, n):
        H = torch.empty(9, dtype=torch.float64, device=dev)
        mask = torch.empty(n, dtype=torch.uint8, device=dev)
        res = torch.empty(2, dtype=torch.int32, device=dev)
        work = torch.empty(lib.apap_ransac_workspace_bytes(n, ITERATIONS), dtype=torch.uint8, device=dev)
        stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        return lambda: _native.check(lib.apap_ransac_device(None, s.data_ptr(), d.data_ptr(), n, 5.0, ITERATIONS,
                                                            ctypes.c_ulonglong(_native.RANSAC_SEED), H.data_ptr(), mask.data_ptr(),
                                                            res.data_ptr(), work.data_ptr(), work.numel(), stream))

    lines, failed = [], []
    for n in (500, 2000, 20000):
        src, dst = scene(n, n)
        s, d = torch.from_numpy(src).to(dev), torch.from_numpy(dst).to(dev)
        work = torch.empty(resident.fundamental_workspace_bytes(n, 1, ITERATIONS), dtype=torch.uint8, device=dev)
        t_f, t_r = event_timed([lambda: resident.hip_fundamental(s, d, 3.0, ITERATIONS, work=work), ransac_call(s, d, n)])
        F, mask, res = resident.hip_fundamental(s, d, 3.0, ITERATIONS, work=work)
        line = {"row": f"n={n}", "n": n, "iterations": ITERATIONS, "reps": a.reps, "warmup": a.warmup, **stats("fundamental", t_f),
                **stats("ransac_homography", t_r), "inliers": int(res[1]), "model": bool(torch.isfinite(F).all())}
        line["ratio_fundamental_over_ransac"] = line["fundamental_us_median"] / line["ransac_homography_us_median"]
        lines.append(line)
    P, n = 4, 2000
    pts = [scene(n, 100 + p) for p in range(P)]
    S = torch.from_numpy(np.concatenate([p[0] for p in pts])).to(dev)
    D = torch.from_numpy(np.concatenate([p[1] for p in pts])).to(dev)
    wb = torch.empty(resident.fundamental_workspace_bytes(P * n, P, ITERATIONS), dtype=torch.uint8, device=dev)
    w1 = torch.empty(resident.fundamental_workspace_bytes(n, 1, ITERATIONS), dtype=torch.uint8, device=dev)
    batch = lambda: resident.hip_fundamental_batch(S, D, [n] * P, 3.0, ITERATIONS, work=wb)      # noqa: E731
    singles = lambda: [resident.hip_fundamental(S[p * n:(p + 1) * n], D[p * n:(p + 1) * n], 3.0, ITERATIONS, work=w1)      # noqa: E731
                       for p in range(P)]
    t_b, t_s = event_timed([batch, singles])
    Fb, mb, rb = batch()
    got = singles()
    same = all(Fb[p].cpu().numpy().tobytes() == got[p][0].cpu().numpy().tobytes() and torch.equal(mb[p * n:(p + 1) * n], got[p][1])
               and torch.equal(rb[p], got[p][2]) for p in range(P))
    line = {"row": f"{P} pairs of n={n}", "pairs": P, "n": n, "iterations": ITERATIONS, "reps": a.reps, "warmup": a.warmup,
            **stats("batch_call", t_b), **stats("single_calls", t_s), "batch_equals_single_calls": bool(same)}
    line["ratio_single_calls_over_batch"] = line["single_calls_us_median"] / line["batch_call_us_median"]
    if not same:
        failed.append("the batched call and the single calls differ")
    lines.append(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for line in lines:
            print(json.dumps(line))
            f.write(json.dumps(line) + "\n")
    if failed:
        raise SystemExit("fundamental_rate: " + "; ".join(failed))


if __name__ == "__main__":
    main()
