#!/usr/bin/env python3
"""Time the robust moving DLT (cvx_proj_amd._native.local_model_solve: the M-step's solve for every cell of a mesh in one
call) against the loop it replaces (local_weights, then one model_solve per cell), on the GPU.

    python tools/local_model_rate.py [--n 2000] [--meshes 16 32 100] [--loop-meshes 16 32] [--reps 3]
                                     [--out profiles/local_model_rate.jsonl]

One JSON line per (solver, mesh), printed and written to --out (afresh: the file holds one run): seconds per call of the
one-call form (host clock around the synchronous call, after one warm-up call; median and minimum of --reps), and for the
meshes of --loop-meshes the same for the loop, measured in the same process, the ratio loop / call of the medians and whether every cell's H and info equal
the loop's bit for bit.  Inputs: tools/model_rate.py's seeded synthetic pair (a homography, 1 px noise, 20 % outliers), its
weights as match weights, a mesh of get_vertice over the pair's 1280 x 1280 frame, gamma 0.5, sigma 100.

Pass condition: the tool exits non-zero when the 32 x 32 SDP call is not at least 10 x faster than its loop.  One SDP solve
keeps one wave busy for ~6.5 ms and two cells share a CU (55 KB of LDS each), so 512 of the 1024 cells solve at once: the
call should beat the loop by two orders of magnitude; 10 x leaves a 25 x margin on the 256-way parallelism that a
conservative count derives, for clocks, the reduction step and launch overhead."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.model_rate import synth, timed  # noqa: E402

GAMMA, SIGMA, FRAME = 0.5, 100.0, (1280, 1280)
REQUIRED_RATIO = 10.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=2000)
    ap.add_argument("--meshes", type=int, nargs="+", default=[16, 32, 100])
    ap.add_argument("--loop-meshes", type=int, nargs="+", default=[16, 32])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "local_model_rate.jsonl"))
    a = ap.parse_args()
    from cvx_proj_amd import _native
    from cvx_proj_amd.apap_utils import get_vertice
    if _native.lib().apap_device_count() < 1:
        raise SystemExit("local_model_rate: no HIP device (this tool measures the GPU; it has no CPU mode)")
    pc, po, mw = synth(a.n)
    lines, verdict = [], None
    for name, params in (("sdp", _native.model_params(_native.MODEL_SDP, 0.5, 0.5, swap=False)),
                         ("lms", _native.model_params(_native.MODEL_LMS, swap=False))):
        for m in a.meshes:
            v = get_vertice(FRAME, m, (0, 0))
            (H, info, status), t_call = timed(lambda: _native.local_model_solve(pc, po, v, GAMMA, SIGMA, params, match_weights=mw),
                                              a.reps)
            line = {"solver": name, "n": a.n, "mesh": m, "cells": m * m, "reps": a.reps,
                    "call_seconds_median": float(np.median(t_call)), "call_seconds_min": float(min(t_call)),
                    "cells_with_status": int(np.count_nonzero(status)),
                    "ipm_iterations_max": int(np.nanmax(info[..., _native.MODEL_INFO_ITERS]))}
            if m in a.loop_meshes:
                def loop():
                    W = _native.local_weights(pc, v, GAMMA, SIGMA).astype(np.float32) * mw
                    return [_native.model_solve(pc, po, w, params) for w in W.reshape(-1, a.n)]
                want, t_loop = timed(loop, a.reps)
                same = [H.reshape(-1, 3, 3)[k].tobytes() == want[k][0].tobytes() and
                        info.reshape(m * m, -1)[k].tobytes() == want[k][1].tobytes() for k in range(m * m)]
                line.update({"loop_seconds_median": float(np.median(t_loop)), "loop_seconds_min": float(min(t_loop)),
                             "loop_over_call": float(np.median(t_loop) / np.median(t_call)), "every_cell_equal": bool(all(same))})
                if name == "sdp" and m == 32:
                    verdict = line["loop_over_call"]
            print(json.dumps(line), flush=True)
            lines.append(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        for line in lines:
            fh.write(json.dumps(line) + "\n")
    if verdict is not None and not verdict >= REQUIRED_RATIO:
        raise SystemExit(f"local_model_rate: the 32 x 32 SDP call is {verdict:.1f} x faster than its loop; {REQUIRED_RATIO:.0f} x required")
    if verdict is None and 32 in a.meshes:
        raise SystemExit("local_model_rate: the 32 x 32 SDP loop was not measured (--loop-meshes), so the pass condition was not checked")


if __name__ == "__main__":
    main()
