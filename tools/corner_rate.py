#!/usr/bin/env python3
"""Time the exact integer Harris corner detector (cvx_proj_amd.resident.hip_corner_detect: a tile kernel and a selection
kernel, nothing but the image read from memory) on the GPU, beside the same detector written with torch ops: ``conv2d`` Sobel
in float64 on the reflect-padded grey image, a box ``conv2d`` of the three products, the response, ``max_pool2d`` non-maximum
suppression and ``topk``.  In float64 that chain is exact too (every intermediate is an integer below 2^53).

    python tools/corner_rate.py [--reps 20] [--warmup 3] [--out profiles/corner_rate.jsonl]

One JSON line per row, printed and written to --out (afresh: the file holds one run).  Rows: a 2160 x 3840 scene, grey and BGR,
with max_corners 2000 and 20 000 (radius 5, quality 10 permille); 16 grey images of 1024 x 1024 in one batched call against 16
single calls.  Seeded scenes (box-blurred noise with flat rectangles), on the device before the clock starts.  Every timed
call ends in a device synchronise inside a host clock; median and minimum of --reps calls after --warmup.  Beside each time:
pixels per second and the fraction of the derived ceiling, 26 us at 4K: about 250 integer vector operations per pixel (the
3 x 3 sums over a tile with its halo, the 64-bit row maxima) at 78.6e12 lane operations per second; the 8 to 25 MB read takes
a few us and does not bound it.  The corner set is checked against the comparator's in the same run: every corner returned
must be a positive local maximum of the comparator's response that passes the quality test, and the returned responses must
be the comparator's ``topk`` values (the comparator keeps every pixel of a plateau of equal maxima, the detector exactly one:
where such a plateau reaches the list the values are reported as differing, not failed).

Pass conditions (the tool exits non-zero otherwise): every 4K call is not slower than the comparator (medians), and the
batched call is faster than its 16 single calls."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

OPS_PER_PIXEL = 250.0
LANE_OPS_PER_SECOND = 157.3e12 / 2
RADIUS, PERMILLE = 5, 10


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


def stats(prefix, times, pixels):
    med, lo = float(np.median(times)), float(min(times))
    return {prefix + "_seconds_median": med, prefix + "_seconds_min": lo, prefix + "_pixels_per_second": pixels / med,
            prefix + "_fraction_of_ceiling": pixels * OPS_PER_PIXEL / LANE_OPS_PER_SECOND / med}


_KERNELS = {}


def response(img):
    """25 (det - 0.04 tr^2) of a uint8 image tensor with torch ops in float64: exact (integers below 2^53)."""
    import torch
    import torch.nn.functional as F
    if img.device not in _KERNELS:
        kx = torch.tensor([[-1.0, 0, 1], [-2, 0, 2], [-1, 0, 1]], dtype=torch.float64, device=img.device)
        _KERNELS[img.device] = torch.stack([kx, kx.t()])[:, None], torch.ones((3, 1, 3, 3), dtype=torch.float64, device=img.device)
    sobel, box = _KERNELS[img.device]
    if img.dim() == 3:
        b, g, r = (img[..., k].to(torch.int64) for k in range(3))
        grey = ((3735 * b + 19235 * g + 9798 * r + 16384) >> 15).to(torch.float64)
    else:
        grey = img.to(torch.float64)
    d = F.conv2d(F.pad(grey[None, None], (1, 1, 1, 1), mode="reflect"), sobel)[0]
    prod = torch.stack([d[0] * d[0], d[0] * d[1], d[1] * d[1]])[None]
    s = F.conv2d(F.pad(prod, (1, 1, 1, 1), mode="reflect"), box, groups=3)[0]
    return 25 * (s[0] * s[2] - s[1] * s[1]) - (s[0] + s[2]) ** 2


def compare(img, max_corners):
    """(values, flat indices, the response after suppression and the quality test): the torch chain."""
    import torch
    import torch.nn.functional as F
    R = response(img)
    peak = F.max_pool2d(R[None, None], 2 * RADIUS + 1, stride=1, padding=RADIUS)[0, 0]
    R = torch.where((R > 0) & (R == peak), R, torch.zeros_like(R))
    R = torch.where(1000 * R >= PERMILLE * R.max(), R, torch.zeros_like(R))
    val, idx = R.ravel().topk(max_corners)
    return val, idx, R


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "corner_rate.jsonl"))
    a = ap.parse_args()
    if a.reps < 20 or a.warmup < 3:
        raise SystemExit("corner_rate: at least 20 timed calls after 3 warm-ups")
    import torch      # before the library: one HIP runtime per process
    import torch.nn.functional as F
    from cvx_proj_amd import _native, resident
    if _native.lib().apap_device_count() < 1 or not torch.cuda.is_available():
        raise SystemExit("corner_rate: no HIP device (this tool measures the GPU; it has no CPU mode)")
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

    def check(img, pts, resp, count, cmp_out):
        """Corners returned that the comparator does not have, and whether the returned responses are the comparator's topk."""
        val, _, R = cmp_out
        n = int(count)
        x, y = pts[:n, 0].long(), pts[:n, 1].long()
        missing = int(torch.count_nonzero(R[y, x] != resp[:n].to(torch.float64)))
        k = int(torch.count_nonzero(val > 0))
        same = k == n and bool(torch.equal(val[:k], resp[:n].to(torch.float64)))
        return n, missing, same

    lines, failed = [], []
    h, w = 2160, 3840
    for channels in (1, 3):
        img = scene(h, w, 1, channels)
        work = torch.empty(resident.corner_workspace_bytes([(h, w)], RADIUS), dtype=torch.uint8, device=dev)
        for max_corners in (2000, 20000):
            (pts, resp, count), t_ours = timed(lambda: resident.hip_corner_detect(img, max_corners, RADIUS, PERMILLE, work=work), sync,
                                               a.reps, a.warmup)
            cmp_out, t_cmp = timed(lambda: compare(img, max_corners), sync, a.reps, a.warmup)
            n, missing, same = check(img, pts, resp, count, cmp_out)
            del cmp_out
            name = f"{h}x{w} {'grey' if channels == 1 else 'BGR'}, max_corners {max_corners}"
            line = {"row": name, "h": h, "w": w, "channels": channels, "max_corners": max_corners, "radius": RADIUS,
                    "quality_permille": PERMILLE, "reps": a.reps, "warmup": a.warmup, "corners": n, **stats("call", t_ours, float(h) * w),
                    **stats("torch_chain", t_cmp, float(h) * w), "corners_not_in_torch_chain": missing, "responses_equal_torch_topk": same}
            line["ratio_torch_chain_over_call"] = line["torch_chain_seconds_median"] / line["call_seconds_median"]
            if missing:
                failed.append(f"{name}: {missing} corners are not corners of the comparator")
            if line["call_seconds_median"] > line["torch_chain_seconds_median"]:
                failed.append(f"{name}: the call ({line['call_seconds_median']:.3e} s) is slower than the torch chain "
                              f"({line['torch_chain_seconds_median']:.3e} s)")
            lines.append(line)
        del img, work
    P, side, max_corners = 16, 1024, 2000
    imgs = [scene(side, side, 10 + p) for p in range(P)]
    work = torch.empty(resident.corner_workspace_bytes([(side, side)] * P, RADIUS), dtype=torch.uint8, device=dev)
    one = torch.empty(resident.corner_workspace_bytes([(side, side)], RADIUS), dtype=torch.uint8, device=dev)
    batch, t_batch = timed(lambda: resident.hip_corner_detect_batch(imgs, max_corners, RADIUS, PERMILLE, work=work), sync, a.reps, a.warmup)
    singles, t_single = timed(lambda: [resident.hip_corner_detect(im, max_corners, RADIUS, PERMILLE, work=one) for im in imgs], sync,
                              a.reps, a.warmup)
    same = all(torch.equal(b[p], s) for p in range(P) for b, s in zip(batch, singles[p]))
    missing, equal = 0, True
    for p in range(P):
        _, m, s = check(imgs[p], batch[0][p], batch[1][p], batch[2][p], compare(imgs[p], max_corners))
        missing, equal = missing + m, equal and s
    pixels = float(P) * side * side
    line = {"row": f"{P} images of {side}x{side}", "images": P, "h": side, "w": side, "channels": 1, "max_corners": max_corners,
            "radius": RADIUS, "quality_permille": PERMILLE, "reps": a.reps, "warmup": a.warmup,
            "corners": int(batch[2].sum()), **stats("batch_call", t_batch, pixels), **stats("single_calls", t_single, pixels),
            "batch_equals_single_calls": bool(same), "corners_not_in_torch_chain": missing, "responses_equal_torch_topk": equal}
    line["ratio_single_calls_over_batch"] = line["single_calls_seconds_median"] / line["batch_call_seconds_median"]
    if not same:
        failed.append("the batched call and the single calls differ")
    if missing:
        failed.append(f"batch: {missing} corners are not corners of the comparator")
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
        raise SystemExit("corner_rate: " + "; ".join(failed))


if __name__ == "__main__":
    main()
