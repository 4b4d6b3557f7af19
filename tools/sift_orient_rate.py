#!/usr/bin/env python3
"""Time the resident orientation calls (cvx_proj_amd.resident: ``hip_sift_orient``, ``hip_sift_describe_oriented`` at given
angles and fused) beside the unoriented ``hip_sift_describe`` on the GPU.

    python tools/sift_orient_rate.py [--reps 30] [--warmup 5] [--out profiles/sift_orient_rate.jsonl]

One JSON line per row, printed and written to --out (afresh: the file holds one run).  Rows: 4K (3840 x 2160 BGR) with 2000
keypoints; 4K with 20 000 keypoints; 16 images (1920 x 1080) of 2000 keypoints in one batched call.  Seeded images and
keypoints, on the device before the clock starts.  The four calls of a row are timed in ONE alternation - unoriented, orient,
given, fused, and round again - so that whatever else the host and the card are doing falls on all four alike; every timed call
ends in a device synchronise inside a host clock; median and minimum of --reps calls after --warmup rounds.  A sample of
keypoints of every row is checked against the numpy specification (tests/sift_orient_spec.py) bit for bit, and fused against
orient followed by given.  No time is asserted: the tool exits non-zero only when bytes differ."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

H4K, W4K = 2160, 3840
SAMPLE = 256        # keypoints checked against the specification per row


def alternate(calls, sync, reps, warmup):
    """name -> (last result, times): the calls in turn, round after round."""
    out, times = {}, {name: [] for name in calls}
    for rnd in range(warmup + reps):
        for name, fn in calls.items():
            t0 = time.perf_counter()
            out[name] = fn()
            sync()
            if rnd >= warmup:
                times[name].append(time.perf_counter() - t0)
    return out, times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sift_orient_rate.jsonl"))
    a = ap.parse_args()
    if a.reps < 20 or a.warmup < 3:
        raise SystemExit("sift_orient_rate: at least 20 timed rounds after 3 warm-ups")
    import torch      # before the library: one HIP runtime per process
    from cvx_proj_amd import _native, resident
    import sift_orient_spec as O
    from sift_rate import image
    if _native.lib().apap_device_count() < 1 or not torch.cuda.is_available():
        raise SystemExit("sift_orient_rate: no HIP device (this tool measures the GPU; it has no CPU mode)")
    dev = torch.device("cuda", 0)
    sync = lambda: torch.cuda.synchronize(dev)     # noqa: E731
    rng = np.random.default_rng(0)
    consts = dict(taps=_native.sift_taps(), orient_window=_native.sift_orient_window())
    dwin = _native.sift_descr_window()

    def differing(img, pts, pick, angles, feats):
        """Sampled keypoints whose angle bits or descriptor bytes differ from the specification (from 25 x 25 patches)."""
        want_a = O.orient(img, pts[pick], local=True, **consts)
        want_f = O.describe(img, pts[pick], want_a, descr_window=dwin, local=True, **consts)
        got_a, got_f = angles[pick].cpu().numpy(), feats[pick].cpu().numpy()
        return int(np.count_nonzero((got_a.view(np.int32) != want_a.view(np.int32)) | (got_f.view(np.int32) != want_f.view(np.int32)).any(axis=1)))

    def row(name, imgs, d_imgs, pts, lengths, extra):
        d_pts = torch.from_numpy(pts).to(dev)
        work = torch.empty(resident.sift_orient_workspace_bytes(len(imgs)), dtype=torch.uint8, device=dev)
        d_angles = resident.hip_sift_orient_batch(d_imgs, d_pts, lengths, work=work)
        calls = {"unoriented": lambda: resident.hip_sift_describe_batch(d_imgs, d_pts, lengths, work=work),
                 "orient": lambda: resident.hip_sift_orient_batch(d_imgs, d_pts, lengths, work=work),
                 "given": lambda: resident.hip_sift_describe_oriented_batch(d_imgs, d_pts, lengths, d_angles, work=work),
                 "fused": lambda: resident.hip_sift_describe_oriented_batch(d_imgs, d_pts, lengths, work=work)}
        out, times = alternate(calls, sync, a.reps, a.warmup)
        feats, angles = out["fused"]
        same = bool(torch.equal(angles, out["orient"]) and torch.equal(feats, out["given"]))
        last = len(pts) - lengths[-1]
        pick = np.linspace(0, lengths[-1] - 1, SAMPLE).astype(np.int64)
        bad = differing(imgs[-1], pts[last:], pick, angles[last:], feats[last:])
        line = {"row": name, **extra, "keypoints": int(len(pts)), "reps": a.reps, "warmup": a.warmup}
        for call, t in times.items():
            line[call + "_seconds_median"], line[call + "_seconds_min"] = float(np.median(t)), float(min(t))
        line["fused_over_unoriented"] = line["fused_seconds_median"] / line["unoriented_seconds_median"]
        line["fused_over_orient_plus_given"] = line["fused_seconds_median"] / (line["orient_seconds_median"] + line["given_seconds_median"])
        line.update(fused_equals_orient_then_given=same, checked_against_spec=SAMPLE, rows_differing_from_spec=bad)
        return line

    lines = []
    img = image(rng, H4K, W4K)
    d_img = torch.from_numpy(img).to(dev)
    for n in (2000, 20000):
        pts = rng.uniform(0, [W4K, H4K], (n, 2)).astype(np.float32)
        lines.append(row(f"4K, {n} keypoints", [img], [d_img], pts, [n], {"h": H4K, "w": W4K, "channels": 3, "images": 1}))
    del d_img
    P, n, h, w = 16, 2000, 1080, 1920
    imgs = [image(rng, h, w) for _ in range(P)]
    d_imgs = [torch.from_numpy(im).to(dev) for im in imgs]
    pts = rng.uniform(0, [w, h], (P * n, 2)).astype(np.float32)
    lines.append(row(f"{P} images of {n} keypoints, one batched call", imgs, d_imgs, pts, [n] * P, {"h": h, "w": w, "channels": 3, "images": P}))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for line in lines:
            print(json.dumps(line))
            f.write(json.dumps(line) + "\n")
    failed = [ln["row"] for ln in lines if ln["rows_differing_from_spec"] or not ln["fused_equals_orient_then_given"]]
    if failed:
        raise SystemExit("sift_orient_rate: bytes differ from the specification or between the forms in: " + "; ".join(failed))


if __name__ == "__main__":
    main()
