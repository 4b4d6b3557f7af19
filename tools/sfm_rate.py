#!/usr/bin/env python3
"""Time the co-visibility tracks and the track triangulation on the GPU (cvx_proj_amd.resident.hip_covis_tracks: one fill and
five launches - scan, resolve, rows, last, index; hip_triangulate_tracks: one launch), beside the specification's sequential
loop (tests/sfm_spec.py) on the host as the yardstick.

    python tools/sfm_rate.py [--reps 20] [--warmup 3] [--out profiles/sfm_rate.jsonl] [--trace-dir DIR]
    rocprofv3 --kernel-trace -d DIR -- python tools/sfm_rate.py --only-run        # a run of its own, for --trace-dir

One JSON line per size, printed and written to --out (afresh: the file holds one run).  Sizes: 4 x 500, 4 x 2000 and 8 x 8000
observations (the last is the entry points' limit of 65 536 less 1536).  Seeded views of one keypoint set (each view sees a
random 1 / 1.2 of it, 0.05 px jitter), on the device before the clock starts, workspace allocated once.  Every call is
bracketed by two events on its stream; median and minimum of --reps calls after --warmup.  With --trace-dir the kernel rows
of a rocprofv3 trace of an --only-run run (same sizes, same order, ``--reps`` calls each and no warm-up) are read and each
kernel's share of the six kernels' time is added.  The host yardstick is the specification's array-search form at every size
and its plain loop at 4 x 500.  Timing is reported, not judged: the tool fails only when a call's result is not the
specification's."""
import argparse
import csv
import glob
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
SIZES = ((4, 500), (4, 2000), (8, 8000))
KERNELS = ("k_covis_scan", "k_covis_resolve", "k_covis_rows", "k_covis_last", "k_covis_index", "k_triangulate_tracks")
DST_POINTS = 1000       # other-picture points per view: the cases' indices are below it


def kernel_shares(trace_dir, reps):
    """Per size, each kernel's summed microseconds over ``reps`` calls, from the kernel rows of a rocprofv3 trace in order."""
    rows = []
    for path in glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True):
        with open(path, newline="") as f:
            for r in csv.DictReader(f):
                name = next((k for k in KERNELS if k in r.get("Kernel_Name", "")), None)
                if name:
                    rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), name))
    rows.sort()
    per_size = len(KERNELS) * reps
    if len(rows) != per_size * len(SIZES):
        raise SystemExit(f"sfm_rate: {len(rows)} kernel rows in {trace_dir}, {per_size * len(SIZES)} expected (an --only-run trace with --reps {reps})")
    out = []
    for k in range(len(SIZES)):
        total = {name: 0.0 for name in KERNELS}
        for a, b, name in rows[k * per_size:(k + 1) * per_size]:
            total[name] += (b - a) / 1e3
        out.append({name + "_us": total[name] / reps for name in KERNELS})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sfm_rate.jsonl"))
    ap.add_argument("--trace-dir", default=None)
    ap.add_argument("--only-run", action="store_true", help="--reps calls a size, no timing, no host loop: for a profiler")
    a = ap.parse_args()
    if not a.only_run and (a.reps < 20 or a.warmup < 3):
        raise SystemExit("sfm_rate: at least 20 timed calls after 3 warm-ups")
    import torch      # before the library: one HIP runtime per process
    from cvx_proj_amd import _native, resident
    import sfm_cases as C
    import sfm_spec as S
    if _native.lib().apap_device_count() < 1 or not torch.cuda.is_available():
        raise SystemExit("sfm_rate: no HIP device (this tool measures the GPU; it has no CPU mode)")
    dev = torch.device("cuda", 0)
    to = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)      # noqa: E731
    shares = kernel_shares(a.trace_dir, a.reps) if a.trace_dir else [{} for _ in SIZES]

    def event_timed(fn):
        ms = []
        for rep in range(a.warmup + a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if rep >= a.warmup:
                ms.append(e0.elapsed_time(e1))
        return ms

    def stats(prefix, ms):
        return {prefix + "_us_median": float(np.median(ms)) * 1e3, prefix + "_us_min": float(min(ms)) * 1e3}

    lines, failed = [], []
    for (V, n), share in zip(SIZES, shares):
        views = C.jittered_views(V, n, int(1.2 * n), 0.05, seed=1000 + n, spread=3000.0)
        pts, idx, off = S.flatten(views)
        cam = C.camera_case(V, 1, seed=7)
        d_pts, d_idx = to(pts), to(idx)
        d_dst = to((C.uniform(2 * DST_POINTS * V, 3, 0) * 768.0).astype(np.float32).reshape(-1, 2))
        d_K, d_R, d_o = to(cam["Kinv"]), to(cam["R"]), to(cam["origins"])
        work = torch.empty(resident.covis_workspace_bytes(len(pts), V), dtype=torch.uint8, device=dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        tracks = lambda: resident.hip_covis_tracks(d_pts, d_idx, [n] * V, status=status, work=work)      # noqa: E731
        table, tpts, ptrack, count = tracks()
        tri = lambda: resident.hip_triangulate_tracks(table, tpts, count, d_dst, [DST_POINTS] * V, d_K, d_R, d_o, cam["center_cam"],      # noqa: E731
                                                      cam["view_cam"])
        if a.only_run:
            for _ in range(a.reps - 1):
                tracks()
            for _ in range(a.reps):
                tri()
            torch.cuda.synchronize()
            continue
        t_tracks, t_tri = event_timed(tracks), event_timed(tri)
        t0 = time.perf_counter()
        want = S.covis_tracks(views)
        host_s = time.perf_counter() - t0
        T = int(count.cpu()[0])
        ok = T == len(want[0]) and np.array_equal(table[:T].cpu().numpy(), want[0]) and tpts[:T].cpu().numpy().tobytes() == want[1].tobytes() \
            and np.array_equal(ptrack.cpu().numpy(), want[2]) and int(status.cpu()[0]) == 0
        if not ok:
            failed.append(f"{V} x {n}: the tracks are not the specification's")
        _, _, n_rays = tri()
        line = {"row": f"{V} x {n}", "views": V, "per_view": n, "observations": V * n, "tracks": T,
                "tracks_seen_twice": int((n_rays[:T] > 0).sum()), "reps": a.reps, "warmup": a.warmup, **stats("covis_tracks", t_tracks),
                **stats("triangulate_tracks", t_tri), "host_spec_array_search_s": host_s, "tracks_equal_spec": bool(ok), **share}
        if share:
            whole = sum(share.values())
            line.update({k[:-3] + "_share": v / whole for k, v in share.items()})
        if (V, n) == SIZES[0]:
            t0 = time.perf_counter()
            S.covis_tracks(views, plain=True)
            line["host_spec_plain_loop_s"] = time.perf_counter() - t0
        lines.append(line)
    if a.only_run:
        return
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for line in lines:
            print(json.dumps(line))
            f.write(json.dumps(line) + "\n")
    if failed:
        raise SystemExit("sfm_rate: " + "; ".join(failed))


if __name__ == "__main__":
    main()
