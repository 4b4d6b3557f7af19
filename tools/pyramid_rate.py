#!/usr/bin/env python3
"""Time the image pyramid (cvx_proj_amd.resident.hip_pyramid: 1 + ceil((levels - 1) / 2) launches of k_pyramid_reduce) on the
GPU beside the same definition written with torch ops, and the chain over the pyramid beside the single-scale chain.

    python tools/pyramid_rate.py [--reps 20] [--warmup 3] [--out profiles/pyramid_rate.jsonl]

One JSON line per row, printed and written to --out (afresh: the file holds one run).

* ``hip_pyramid`` with six levels of a 2160 x 3840 BGR scene and of a 768 x 768 grey one.  The comparator: BGR -> grey in
  int64, H as a stride-2 ``conv2d`` of the reflect-padded plane with the 25 integer taps in float32 (every sum is an integer
  below 2^24: exact), Q from four gathers; its bytes must equal the call's before anything is timed.
* ``hip_pyramid_detect_describe_match`` with six levels against ``hip_detect_describe_match`` on the same pair of seeded
  1080 x 1920 scenes, the second area-reduced by two.  Derived expectation: the detector and the descriptor see
  1 + 9/16 + 1/4 + ... = about 2.1 times the base picture's pixels, plus the extra launches.

Seeded scenes, on the device before the clock starts.  Every timed call ends in a device synchronise inside a host clock;
median and minimum of --reps calls after --warmup, the two sides of a comparison alternated twice (rounds a and b).  Nothing
about speed is a pass condition; unequal bytes are (the tool exits non-zero)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LEVELS = 6


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


def stats(prefix, rounds):
    out = {}
    for tag, times in zip("ab", rounds):
        out[f"{prefix}_seconds_median_{tag}"] = float(np.median(times))
        out[f"{prefix}_seconds_min_{tag}"] = float(min(times))
    return out


def torch_pyramid(img, levels):
    """The definition of include/apap_hip.h "image pyramid" in torch ops, half steps on: a list of uint8 planes."""
    import torch
    import torch.nn.functional as F
    if img.dim() == 3:
        b, g, r = (img[..., k].to(torch.int64) for k in range(3))
        grey = ((3735 * b + 19235 * g + 9798 * r + 16384) >> 15).to(torch.float32)
    else:
        grey = img.to(torch.float32)
    b5 = torch.tensor([1.0, 4, 6, 4, 1], device=img.device)
    k25 = (b5[:, None] * b5[None, :])[None, None]

    def halve(g):
        s = F.conv2d(F.pad(g[None, None], (2, 2, 2, 2), mode="reflect"), k25, stride=2)[0, 0]
        return torch.floor((s + 128) / 256)          # a division by a power of two: exact

    def axis(n):
        x = torch.arange((3 * n) >> 2, device=img.device)
        r = x % 3
        return 4 * (x // 3) + r, (5 - 2 * r).float(), (1 + 2 * r).float()

    def three_quarter(g):
        (sy, wy0, wy1), (sx, wx0, wx1) = axis(g.shape[0]), axis(g.shape[1])
        top = wx0 * g[sy][:, sx] + wx1 * g[sy][:, sx + 1]
        bot = wx0 * g[sy + 1][:, sx] + wx1 * g[sy + 1][:, sx + 1]
        s = (wy0[:, None] * top + wy1[:, None] * bot).to(torch.int32)
        return torch.div(s + 18, 36, rounding_mode="floor").float()

    out = [grey]
    if levels > 1:
        out.append(three_quarter(grey))
    for level in range(2, levels):
        out.append(halve(out[level - 2]))
    return [a.to(torch.uint8) for a in out]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pyramid_rate.jsonl"))
    a = ap.parse_args()
    if a.reps < 20 or a.warmup < 3:
        raise SystemExit("pyramid_rate: at least 20 timed calls after 3 warm-ups")
    import torch      # before the library: one HIP runtime per process
    import torch.nn.functional as F
    from cvx_proj_amd import _native, resident
    if _native.lib().apap_device_count() < 1 or not torch.cuda.is_available():
        raise SystemExit("pyramid_rate: no HIP device (this tool measures the GPU; it has no CPU mode)")
    dev = torch.device("cuda", 0)
    sync = lambda: torch.cuda.synchronize(dev)     # noqa: E731

    def scene(h, w, seed, channels=1):
        gen = torch.Generator(device="cpu").manual_seed(seed)
        planes = []
        for _ in range(channels):
            g = torch.randint(0, 256, (1, 1, h + 4, w + 4), generator=gen).float()
            g = F.avg_pool2d(g, 5, stride=1)[0, 0].floor()
            for _ in range(max(30, h * w // 2000)):
                y, x = int(torch.randint(0, h - 8, (1,), generator=gen)), int(torch.randint(0, w - 8, (1,), generator=gen))
                hh, ww = int(torch.randint(6, 40, (1,), generator=gen)), int(torch.randint(6, 40, (1,), generator=gen))
                g[y:y + hh, x:x + ww] = float(torch.randint(0, 256, (1,), generator=gen))
            planes.append(g.to(torch.uint8))
        img = planes[0] if channels == 1 else torch.stack(planes, -1)
        return img.contiguous().to(dev)

    lines, failed = [], []
    for h, w, channels in ((2160, 3840, 3), (768, 768, 1)):
        img = scene(h, w, 1, channels)
        work = torch.empty(resident.pyramid_workspace_bytes(1, LEVELS), dtype=torch.uint8, device=dev)
        ours, theirs = resident.hip_pyramid(img, LEVELS, True, work=work), torch_pyramid(img, LEVELS)
        sync()
        equal = len(ours) == len(theirs) and all(torch.equal(x, y) for x, y in zip(ours, theirs))
        name = f"hip_pyramid {h}x{w} {'grey' if channels == 1 else 'BGR'}, {LEVELS} levels"
        if not equal:
            failed.append(f"{name}: the levels differ from the torch definition's")
        t_ours, t_cmp = [], []
        for _ in range(2):
            t_ours.append(timed(lambda: resident.hip_pyramid(img, LEVELS, True, work=work), sync, a.reps, a.warmup)[1])
            t_cmp.append(timed(lambda: torch_pyramid(img, LEVELS), sync, a.reps, a.warmup)[1])
        moved = h * w * channels + sum(int(x.numel()) for x in ours) + sum(int(x.numel()) for x in ours[1:-2])      # read, written, levels 1 .. read again
        line = {"row": name, "h": h, "w": w, "channels": channels, "levels": len(ours), "reps": a.reps, "warmup": a.warmup,
                "bytes_equal_torch_definition": bool(equal), "bytes_moved": moved, **stats("call", t_ours), **stats("torch_ops", t_cmp)}
        line["ratio_torch_ops_over_call"] = line["torch_ops_seconds_median_b"] / line["call_seconds_median_b"]
        line["bytes_per_second"] = moved / line["call_seconds_median_b"]
        lines.append(line)
        del img, ours, theirs

    h, w, max_corners = 1080, 1920, 2000
    c_img = scene(h, w, 2)
    o_img = F.avg_pool2d(c_img[None, None].float(), 2)[0, 0].floor().to(torch.uint8).contiguous()
    t_pyr, t_one = [], []
    for _ in range(2):
        out_p, t = timed(lambda: resident.hip_pyramid_detect_describe_match(c_img, o_img, max_corners, LEVELS), sync, a.reps, a.warmup)
        t_pyr.append(t)
        out_1, t = timed(lambda: resident.hip_detect_describe_match(c_img, o_img, max_corners), sync, a.reps, a.warmup)
        t_one.append(t)
    line = {"row": f"chain {h}x{w} against {h // 2}x{w // 2}, max_corners {max_corners}", "h": h, "w": w, "levels": LEVELS,
            "max_corners": max_corners, "reps": a.reps, "warmup": a.warmup, "keypoints_pyramid": [int(out_p[6].shape[0]), int(out_p[7].shape[0])],
            "keypoints_single_scale": [int(out_1[6].shape[0]), int(out_1[7].shape[0])], **stats("pyramid_chain", t_pyr),
            **stats("single_scale_chain", t_one), "derived_pixel_ratio": 2.1}
    line["ratio_pyramid_over_single_scale"] = line["pyramid_chain_seconds_median_b"] / line["single_scale_chain_seconds_median_b"]
    lines.append(line)

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for line in lines:
            print(json.dumps(line))
            f.write(json.dumps(line) + "\n")
    if failed:
        raise SystemExit("pyramid_rate: " + "; ".join(failed))


if __name__ == "__main__":
    main()
