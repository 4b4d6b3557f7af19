#!/usr/bin/env python3
"""Time the exact descriptor matcher (cvx_proj_amd.resident.hip_match_descriptors: nearest and second-nearest train row of
every query, L2, one fused sweep that never stores the nq x nt distances) on the GPU, beside what one would write without it:
``torch.cdist(q, t)`` followed by ``topk(2, largest=False)``, which writes and re-reads the nq x nt matrix.

    python tools/match_rate.py [--reps 20] [--warmup 3] [--out profiles/match_rate.jsonl]

One JSON line per row, printed and written to --out (afresh: the file holds one run).  Rows: 2000 x 2000; 20 000 x 20 000;
16 pairs of 2000 x 2000 in one batched call against 16 single calls.  Seeded integer descriptors in 0 .. 255 (float32), on the
device before the clock starts.  Every timed call ends in a device synchronise inside a host clock; median and minimum of
--reps calls after --warmup.  Beside each time: the achieved pair-dimensions per second (nq nt 128 / seconds) and its fraction
of the ceiling, 3.93e13 (one (query, train row, dimension) costs a subtraction and a fused multiply-add; 157.3 TFLOP/s of
float32 are 78.6e12 such instructions per second).  The indices are checked against the comparator's in the same run: where
they differ (cdist goes through a float32 matrix product, which rounds), the squared distances of both choices are recomputed
in float64 and this matcher's must not be the larger.

Pass conditions (the tool exits non-zero otherwise): at 20 000 x 20 000 the call is not slower than the comparator (medians; a
fused sweep has no excuse to lose to one that stores 1.6 GB and reads it back), and the batched call is faster than its 16
single calls.  The 2000 x 2000 row is reported without a condition: at the ceiling it would take 13 us, the size of a launch."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CEILING = 157.3e12 / 2 / 2      # pair-dimensions per second
DIM = 128


def timed(fn, sync, reps, warmup):
    for _ in range(warmup):
        out = fn()
        sync()
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        sync()
        times.append(time.perf_counter() - t0)
    return out, times


def stats(prefix, times, pair_dims=None):
    med, lo = float(np.median(times)), float(min(times))
    d = {prefix + "_seconds_median": med, prefix + "_seconds_min": lo}
    if pair_dims is not None:
        d[prefix + "_pair_dims_per_second"] = pair_dims / med
        d[prefix + "_fraction_of_ceiling"] = pair_dims / med / CEILING
    return d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "match_rate.jsonl"))
    a = ap.parse_args()
    if a.reps < 20 or a.warmup < 3:
        raise SystemExit("match_rate: at least 20 timed calls after 3 warm-ups")
    import torch      # before the library: one HIP runtime per process
    from cvx_proj_amd import _native, resident
    if _native.lib().apap_device_count() < 1 or not torch.cuda.is_available():
        raise SystemExit("match_rate: no HIP device (this tool measures the GPU; it has no CPU mode)")
    dev = torch.device("cuda", 0)
    sync = lambda: torch.cuda.synchronize(dev)     # noqa: E731
    gen = torch.Generator(device="cpu").manual_seed(0)
    ints = lambda n: torch.randint(0, 256, (n, DIM), generator=gen).to(torch.float32).to(dev)     # noqa: E731

    def compare(q, t):
        d = torch.cdist(q, t)
        return d.topk(2, dim=1, largest=False)

    def check(q, t, idx, cidx):
        """Queries whose nearest index differs from the comparator's, and of those, the ones where this matcher's choice is the
        farther one in float64 (must be none)."""
        differ = torch.nonzero(idx.long() != cidx).ravel()
        q64 = q[differ].double()
        ours = ((q64 - t[idx[differ].long()].double()) ** 2).sum(1)
        theirs = ((q64 - t[cidx[differ]].double()) ** 2).sum(1)
        return int(differ.numel()), int(torch.count_nonzero(ours > theirs))

    lines, failed = [], []
    for n in (2000, 20000):
        q, t = ints(n), ints(n)
        work = torch.empty(resident.match_workspace_bytes(n, n), dtype=torch.uint8, device=dev)
        (idx, dist, idx2, dist2), t_ours = timed(lambda: resident.hip_match_descriptors(q, t, work=work), sync, a.reps, a.warmup)
        (cval, cidx), t_cmp = timed(lambda: compare(q, t), sync, a.reps, a.warmup)
        differ, worse = check(q, t, idx, cidx[:, 0])
        line = {"row": f"{n}x{n}", "nq": n, "nt": n, "reps": a.reps, "warmup": a.warmup, "splits": _native.match_splits(n, n)[0],
                **stats("call", t_ours, float(n) * n * DIM), **stats("cdist_topk", t_cmp, float(n) * n * DIM),
                "nearest_differs_from_cdist": differ, "nearest_farther_than_cdist": worse}
        line["ratio_cdist_topk_over_call"] = line["cdist_topk_seconds_median"] / line["call_seconds_median"]
        if worse:
            failed.append(f"{n} x {n}: {worse} queries got a farther neighbour than the comparator's")
        if n == 20000 and line["call_seconds_median"] > line["cdist_topk_seconds_median"]:
            failed.append(f"20000 x 20000: the call ({line['call_seconds_median']:.3e} s) is slower than cdist + topk "
                          f"({line['cdist_topk_seconds_median']:.3e} s)")
        lines.append(line)
        del work, cval, cidx
    P, n = 16, 2000
    Q, T = ints(P * n), ints(P * n)
    work = torch.empty(resident.match_workspace_bytes([n] * P, [n] * P), dtype=torch.uint8, device=dev)
    one = torch.empty(resident.match_workspace_bytes(n, n), dtype=torch.uint8, device=dev)
    batch, t_batch = timed(lambda: resident.hip_match_descriptors_batch(Q, T, [n] * P, [n] * P, work=work), sync, a.reps, a.warmup)
    singles, t_single = timed(lambda: [resident.hip_match_descriptors(Q[p * n:(p + 1) * n], T[p * n:(p + 1) * n], work=one)
                                       for p in range(P)], sync, a.reps, a.warmup)
    same = all(torch.equal(b[p * n:(p + 1) * n], s) for p in range(P) for b, s in zip(batch, singles[p]))
    cidx = torch.cat([compare(Q[p * n:(p + 1) * n], T[p * n:(p + 1) * n])[1][:, 0] for p in range(P)])
    offs = torch.arange(P, device=dev).repeat_interleave(n) * n
    differ, worse = check(Q, T, batch[0] + offs.int(), cidx + offs)
    line = {"row": f"{P} pairs of {n}x{n}", "pairs": P, "nq": n, "nt": n, "reps": a.reps, "warmup": a.warmup,
            **stats("batch_call", t_batch, float(P) * n * n * DIM), **stats("single_calls", t_single, float(P) * n * n * DIM),
            "batch_equals_single_calls": bool(same), "nearest_differs_from_cdist": differ, "nearest_farther_than_cdist": worse}
    line["ratio_single_calls_over_batch"] = line["single_calls_seconds_median"] / line["batch_call_seconds_median"]
    if not same:
        failed.append("the batched call and the single calls differ")
    if worse:
        failed.append(f"batch: {worse} queries got a farther neighbour than the comparator's")
    if line["batch_call_seconds_median"] >= line["single_calls_seconds_median"]:
        failed.append(f"the batched call ({line['batch_call_seconds_median']:.3e} s) is not faster than its {P} single calls "
                      f"({line['single_calls_seconds_median']:.3e} s)")
    lines.append(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for line in lines:
            print(json.dumps(line))
            f.write(json.dumps(line) + "\n")
    if failed:
        raise SystemExit("match_rate: " + "; ".join(failed))


if __name__ == "__main__":
    main()
