#!/usr/bin/env python3
"""Time guided descriptor matching (cvx_proj_amd.resident.hip_guided_match: the gate on all nq x nt pairs, the 128-term
distance only for the survivors) on the GPU, in one alternation with the unguided matcher (hip_match_descriptors) at the same
size and with the same definition written in torch ops (the float64 gate as an nq x nt mask over ``torch.cdist``, then
``topk(2)``).

    python tools/guided_match_rate.py [--reps 20] [--warmup 3] [--out profiles/guided_match_rate.jsonl]

One JSON line per row, printed and written to --out (afresh: the file holds one run).  Rows: the look-alike scene of
tests/guided_match_spec.py scaled to 2000 x 2000 and to 20 000 x 20 000 keypoints (the field grows with the count, so the
density, and with it the candidates per query at radius 6, stay what they are at 300), records and descriptors on the device
before the clock starts.  Every timed call ends in a device synchronise inside a host clock; the three calls take turns inside
one loop, median and minimum of --reps turns after --warmup.  Beside each row: the mean and the largest candidate count, the
share of queries that get their true partner with and without the gate, and the derived floor of the gate pass - nq nt pairs
at 6 float64 operations, over the chip's 78.6e12 float64 operations per second.

Pass condition (the tool exits non-zero otherwise): at 20 000 x 20 000 the guided call is not slower than the unguided matcher
(medians).  At 2000 x 2000 both are launch-bound: reported, no condition."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FP64_PER_SECOND = 78.6e12
GATE_OPS = 6
H_SCENE = np.array([[1.02, .01, 12], [-.015, .99, 7], [1e-5, -2e-5, 1]])     # train -> query


def scene(n, seed=0):
    """tests/guided_match_spec.py's scene with n train keypoints and n queries on a field of the same density as 300 on
    640 x 480.  The projective terms of H are scaled down with the field, so that the far corner stays a mild warp."""
    rng = np.random.default_rng(seed)
    s = np.sqrt(n / 300.0)
    H = H_SCENE.copy()
    H[2, :2] /= s
    t_pts = (rng.random((n, 2)) * [640 * s, 480 * s]).astype(np.float32)
    tex = rng.integers(0, 256, (10, 128))
    lab = rng.integers(0, 10, n)
    t_desc = np.clip(tex[lab] + rng.integers(-1, 2, (n, 128)), 0, 255)
    perm = rng.permutation(n)
    p = np.c_[t_pts[perm].astype(np.float64), np.ones(n)] @ H.T
    q_pts = (p[:, :2] / p[:, 2:] + rng.normal(0, .5, (n, 2))).astype(np.float32)
    q_desc = np.clip(t_desc[perm] + rng.integers(-12, 13, (n, 128)), 0, 255)
    return q_pts, q_desc.astype(np.float32), t_pts, t_desc.astype(np.float32), H, perm


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sizes", type=int, nargs="+", default=[2000, 20000])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "guided_match_rate.jsonl"))
    a = ap.parse_args()
    if a.reps < 20 or a.warmup < 3:
        raise SystemExit("guided_match_rate: at least 20 timed calls after 3 warm-ups")
    import torch      # before the library: one HIP runtime per process
    from cvx_proj_amd import _native, resident
    if _native.lib().apap_device_count() < 1 or not torch.cuda.is_available():
        raise SystemExit("guided_match_rate: no HIP device (this tool measures the GPU; it has no CPU mode)")
    dev = torch.device("cuda", 0)
    sync = lambda: torch.cuda.synchronize(dev)     # noqa: E731
    radius = 6.0
    r2 = radius * radius

    lines, failed = [], []
    for n in a.sizes:
        q_pts, q_desc, t_pts, t_desc, H, perm = scene(n)
        q, t = torch.from_numpy(q_desc).to(dev), torch.from_numpy(t_desc).to(dev)
        rec_q = resident.hip_guided_records(torch.from_numpy(q_pts).to(dev), None, "point")
        rec_t = resident.hip_guided_records(torch.from_numpy(t_pts).to(dev), torch.from_numpy(H).to(dev), "project")
        work_g = torch.empty(resident.guided_workspace_bytes(n, n), dtype=torch.uint8, device=dev)
        work_m = torch.empty(resident.match_workspace_bytes(n, n), dtype=torch.uint8, device=dev)

        def guided():
            return resident.hip_guided_match(q, t, rec_q, rec_t, "point", r2, work=work_g)

        def unguided():
            return resident.hip_match_descriptors(q, t, work=work_m)

        def in_torch():
            dx = rec_t[None, :, 0] - rec_q[:, None, 0]
            dy = rec_t[None, :, 1] - rec_q[:, None, 1]
            passes = dx * dx + dy * dy < r2
            d = torch.cdist(q, t).masked_fill_(~passes, float("inf"))
            val, idx = d.topk(2, dim=1, largest=False)
            return val, idx, passes.sum(1)

        calls = {"guided": guided, "unguided": unguided, "torch_ops": in_torch}
        times, out = {k: [] for k in calls}, {}
        for turn in range(a.warmup + a.reps):      # one alternation: the three calls take turns
            for name, fn in calls.items():
                sync()
                t0 = time.perf_counter()
                out[name] = fn()
                sync()
                if turn >= a.warmup:
                    times[name].append(time.perf_counter() - t0)
        idx, dist, idx2, dist2, count, _, _ = out["guided"]
        perm_d = torch.from_numpy(perm).to(dev)
        tval, tidx, tcount = out["torch_ops"]
        tidx0 = torch.where(torch.isfinite(tval[:, 0]), tidx[:, 0], torch.full_like(tidx[:, 0], -1))
        line = {"row": f"{n}x{n}", "nq": n, "nt": n, "radius": radius, "reps": a.reps, "warmup": a.warmup,
                "splits": _native.guided_splits(n, n)[0],
                "candidates_mean": float(count.double().mean()), "candidates_max": int(count.max()),
                "correct_partner_guided": float((idx.long() == perm_d).double().mean()),
                "correct_partner_unguided": float((out["unguided"][0].long() == perm_d).double().mean()),
                "count_equals_torch": bool(torch.equal(count.long(), tcount)),
                "nearest_differs_from_torch": int(torch.count_nonzero(idx.long() != tidx0)),
                "gate_pass_floor_seconds": float(n) * n * GATE_OPS / FP64_PER_SECOND}
        for name, ts in times.items():
            line[name + "_seconds_median"], line[name + "_seconds_min"] = float(np.median(ts)), float(min(ts))
        line["ratio_unguided_over_guided"] = line["unguided_seconds_median"] / line["guided_seconds_median"]
        line["ratio_torch_ops_over_guided"] = line["torch_ops_seconds_median"] / line["guided_seconds_median"]
        if not line["count_equals_torch"]:
            failed.append(f"{n} x {n}: the candidate counts differ from the torch definition's")
        if n >= 20000 and line["guided_seconds_median"] > line["unguided_seconds_median"]:
            failed.append(f"{n} x {n}: the guided call ({line['guided_seconds_median']:.3e} s) is slower than the unguided matcher "
                          f"({line['unguided_seconds_median']:.3e} s)")
        lines.append(line)
        del out, tval, tidx, tcount, work_g, work_m
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for line in lines:
            print(json.dumps(line))
            f.write(json.dumps(line) + "\n")
    if failed:
        raise SystemExit("guided_match_rate: " + "; ".join(failed))


if __name__ == "__main__":
    main()
