#!/usr/bin/env python3
"""Time SIFT descriptor extraction at given keypoints (cvx_proj_amd.resident.hip_sift_describe: one fused kernel, work
proportional to the keypoints, no intermediate image) on the GPU, beside the one step it avoids: the full-image separable blur
of the float32 grey image, two ``torch.nn.functional.conv2d`` passes (13 x 1 after 1 x 13) - the base image alone, without
gradients, histograms or normalisation.

    python tools/sift_rate.py [--reps 20] [--warmup 3] [--out profiles/sift_rate.jsonl]

One JSON line per row, printed and written to --out (afresh: the file holds one run).  Rows: 4K (3840 x 2160 BGR) with 2000
keypoints; 4K with 20 000 keypoints; 16 images of 2000 keypoints in one batched call against 16 single calls.  Seeded images and
keypoints, on the device before the clock starts.  Every timed call ends in a device synchronise inside a host clock; median
and minimum of --reps calls after --warmup.  The descriptors of a sample of keypoints are checked against the numpy
specification (tests/sift_spec.py) byte for byte.

Pass conditions (the tool exits non-zero otherwise): the 4K / 2000 call is not slower than the blur alone (medians), and the
batched call is faster than its 16 single calls."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

H4K, W4K = 2160, 3840
SAMPLE = 256        # keypoints checked against the specification per row


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


def stats(prefix, times):
    return {prefix + "_seconds_median": float(np.median(times)), prefix + "_seconds_min": float(min(times))}


def image(rng, h, w):
    """A seeded BGR image with structure at every scale a descriptor sees: sinusoids plus noise."""
    yy, xx = np.mgrid[:h, :w].astype(np.float32)
    planes = [127 + 60 * np.sin(xx / (5 + 2 * k)) * np.cos(yy / (7 - k)) + rng.normal(0, 8, (h, w)).astype(np.float32) for k in range(3)]
    return np.stack(planes, -1).clip(0, 255).astype(np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sift_rate.jsonl"))
    a = ap.parse_args()
    if a.reps < 20 or a.warmup < 3:
        raise SystemExit("sift_rate: at least 20 timed calls after 3 warm-ups")
    import torch      # before the library: one HIP runtime per process
    import torch.nn.functional as F
    from cvx_proj_amd import _native, resident
    import sift_spec as S
    if _native.lib().apap_device_count() < 1 or not torch.cuda.is_available():
        raise SystemExit("sift_rate: no HIP device (this tool measures the GPU; it has no CPU mode)")
    dev = torch.device("cuda", 0)
    sync = lambda: torch.cuda.synchronize(dev)     # noqa: E731
    rng = np.random.default_rng(0)
    taps, window = _native.sift_taps(), _native.sift_window()
    d_taps = torch.from_numpy(taps).to(dev)
    k_row, k_col = d_taps.reshape(1, 1, 1, -1), d_taps.reshape(1, 1, -1, 1)

    def blur(grey_f32):      # (1, 1, h, w) float32 -> the base image: what cv.GaussianBlur(grey, (13, 13), sigma) computes
        x = F.conv2d(F.pad(grey_f32, (6, 6, 0, 0), mode="reflect"), k_row)
        return F.conv2d(F.pad(x, (0, 0, 6, 6), mode="reflect"), k_col)

    def spec_check(img, pts, got):
        pick = np.linspace(0, len(pts) - 1, SAMPLE).astype(np.int64)
        want = S.describe(img, pts[pick], taps, window, local=True)     # from 21 x 21 patches: no 4K blur in numpy
        return int(np.count_nonzero((got[pick].cpu().numpy().view(np.int32) != want.view(np.int32)).any(axis=1)))

    lines, failed = [], []
    img = image(rng, H4K, W4K)
    d_img = torch.from_numpy(img).to(dev)
    d_grey = torch.from_numpy(S.grey(img).astype(np.float32)).to(dev).reshape(1, 1, H4K, W4K)
    work = torch.empty(resident.sift_workspace_bytes(1), dtype=torch.uint8, device=dev)
    _, t_blur = timed(lambda: blur(d_grey), sync, a.reps, a.warmup)
    for n in (2000, 20000):
        pts = rng.uniform(0, [W4K, H4K], (n, 2)).astype(np.float32)
        d_pts = torch.from_numpy(pts).to(dev)
        got, t_ours = timed(lambda: resident.hip_sift_describe(d_img, d_pts, work=work), sync, a.reps, a.warmup)
        bad = spec_check(img, pts, got)
        line = {"row": f"4K, {n} keypoints", "h": H4K, "w": W4K, "channels": 3, "keypoints": n, "reps": a.reps, "warmup": a.warmup,
                **stats("call", t_ours), **stats("blur_alone", t_blur), "keypoints_per_second": n / float(np.median(t_ours)),
                "checked_against_spec": SAMPLE, "rows_differing_from_spec": bad}
        line["ratio_blur_alone_over_call"] = line["blur_alone_seconds_median"] / line["call_seconds_median"]
        if bad:
            failed.append(f"4K / {n}: {bad} of {SAMPLE} sampled descriptors differ from the specification")
        if n == 2000 and line["call_seconds_median"] > line["blur_alone_seconds_median"]:
            failed.append(f"4K / 2000: the call ({line['call_seconds_median']:.3e} s) is slower than the full-image blur alone "
                          f"({line['blur_alone_seconds_median']:.3e} s)")
        lines.append(line)
    del d_img, d_grey
    P, n, h, w = 16, 2000, 1080, 1920
    imgs = [image(rng, h, w) for _ in range(P)]
    d_imgs = [torch.from_numpy(im).to(dev) for im in imgs]
    pts = rng.uniform(0, [w, h], (P * n, 2)).astype(np.float32)
    d_pts = torch.from_numpy(pts).to(dev)
    bwork = torch.empty(resident.sift_workspace_bytes(P), dtype=torch.uint8, device=dev)
    batch, t_batch = timed(lambda: resident.hip_sift_describe_batch(d_imgs, d_pts, [n] * P, work=bwork), sync, a.reps, a.warmup)
    singles, t_single = timed(lambda: [resident.hip_sift_describe(d_imgs[m], d_pts[m * n:(m + 1) * n], work=work) for m in range(P)],
                              sync, a.reps, a.warmup)
    same = all(torch.equal(batch[m * n:(m + 1) * n], singles[m]) for m in range(P))
    bad = spec_check(imgs[P - 1], pts[(P - 1) * n:], batch[(P - 1) * n:])
    line = {"row": f"{P} images of {n} keypoints", "images": P, "h": h, "w": w, "channels": 3, "keypoints": n, "reps": a.reps,
            "warmup": a.warmup, **stats("batch_call", t_batch), **stats("single_calls", t_single), "batch_equals_single_calls": bool(same),
            "checked_against_spec": SAMPLE, "rows_differing_from_spec": bad}
    line["ratio_single_calls_over_batch"] = line["single_calls_seconds_median"] / line["batch_call_seconds_median"]
    if not same:
        failed.append("the batched call and the single calls differ")
    if bad:
        failed.append(f"batch: {bad} of {SAMPLE} sampled descriptors differ from the specification")
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
        raise SystemExit("sift_rate: " + "; ".join(failed))


if __name__ == "__main__":
    main()
