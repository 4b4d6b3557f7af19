#!/usr/bin/env python3
"""Time the global warp and blend (cvx_proj_amd.resident.hip_image_warp / hip_image_warp_batch: one fused kernel over the
canvas) on the GPU at the 4K pair of configuration C3, beside ``torch.nn.functional.grid_sample`` on the same canvas.

    python tools/image_warp_rate.py [--reps 50] [--warmup 5] [--out profiles/image_warp_rate.jsonl]

One JSON line per row, printed and written to --out (afresh: the file holds one run).  Rows: the 3840 x 2160 pair on its
4009 x 2242 canvas with the base picture pasted (direct) and mean-blended; the batch of two problems on that pair (the
reference's baseline / result: two homographies, mean blend) against the same two as single calls; grid_sample (bilinear,
zeros padding, float32 planes, the sampling grid prepared beforehand) for the time only - it answers a different, floating-point
definition and does no blend.  Seeded pictures, resident on the device before the clock starts; every timed call sits between
two events on its stream (the call enqueues its 144-byte descriptor upload and its kernel, nothing else); median and minimum
of --reps calls after --warmup, each call's canvas written to the same resident tensor.

Yardsticks beside each time: the algorithmic bytes - 3 per canvas pixel written, 3 per pixel of the source picture and 3 per
pixel of the base rectangle read - over the time as a fraction of 8 TB/s, and that fraction over 0.43, what the fused
per-cell warp + blend kernel (k_warp_fast<true>) is recorded at on the same canvas.  No time is a pass condition; the tool
fails only when the batch and the single calls give different bytes."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_BYTES_PER_SECOND = 8.0e12
K3_FRACTION = 0.43


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "image_warp_rate.jsonl"))
    a = ap.parse_args()
    if a.reps < 20 or a.warmup < 3:
        raise SystemExit("image_warp_rate: at least 20 timed calls after 3 warm-ups")
    import torch      # before the library: one HIP runtime per process
    import torch.nn.functional as F
    from cvx_proj_amd import _native, resident
    if _native.lib().apap_device_count() < 1 or not torch.cuda.is_available():
        raise SystemExit("image_warp_rate: no HIP device (this tool measures the GPU; it has no CPU mode)")
    dev = torch.device("cuda", 0)

    def timed(fn):
        for _ in range(a.warmup):
            out = fn()
        torch.cuda.synchronize(dev)
        times = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = fn()
            e1.record()
            e1.synchronize()
            times.append(e0.elapsed_time(e1) * 1e-3)
        return out, times

    h, w = 2160, 3840
    gen = torch.Generator(device="cpu").manual_seed(3)
    base = torch.randint(0, 256, (h, w, 3), generator=gen, dtype=torch.uint8).to(dev)
    src = torch.randint(0, 256, (h, w, 3), generator=gen, dtype=torch.uint8).to(dev)
    c, s = np.cos(0.004), np.sin(0.004)
    H0 = np.array([[c, -s, 168.9], [s, c, 66.5], [1.0e-8, -2.0e-8, 1.0]], np.float32)       # the baseline's homography
    H1 = (H0.astype(np.float64) + np.array([[1e-4, -2e-4, 0.31], [2e-4, 1e-4, -0.22], [1e-10, 1e-10, 0.0]])).astype(np.float32)
    M, cw, ch, tx, ty = _native.image_warp_geometry(h, w, h, w, H0)
    _, cw1, ch1, _, _ = _native.image_warp_geometry(h, w, h, w, H1)
    bytes_one = 3.0 * (cw * ch + h * w + h * w)

    def stats(prefix, times, nbytes):
        med, lo = float(np.median(times)), float(min(times))
        frac = nbytes / PEAK_BYTES_PER_SECOND / med
        return {prefix + "_seconds_median": med, prefix + "_seconds_min": lo, prefix + "_algorithmic_bytes": nbytes,
                prefix + "_fraction_of_8TBps": frac, prefix + "_fraction_over_k_warp_fast_blend": frac / K3_FRACTION}

    lines, failed = [], []
    work = torch.empty(resident.image_warp_workspace_bytes(2), dtype=torch.uint8, device=dev)
    common = {"h": h, "w": w, "canvas_w": cw, "canvas_h": ch, "off_x": tx, "off_y": ty, "reps": a.reps, "warmup": a.warmup}
    out1 = torch.empty(cw * ch * 3, dtype=torch.uint8, device=dev)
    canvases = {}
    for direct in (True, False):
        (canvas,), t = timed(lambda: resident.hip_image_warp_batch([(base, src, H0, direct)], out=out1, work=work))
        canvases[direct] = canvas.clone()
        lines.append({"row": f"{w}x{h} pair, {'direct' if direct else 'mean'} blend", **common, "direct_blend": direct,
                      **stats("call", t, bytes_one)})
    # the baseline / result pair of spectral_method.warp_results: one launch against two
    sizes = [cw * ch * 3, cw1 * ch1 * 3]
    out2 = torch.empty(sum(sizes), dtype=torch.uint8, device=dev)
    outs = [torch.empty(n, dtype=torch.uint8, device=dev) for n in sizes]
    probs = [(base, src, H0, False), (base, src, H1, False)]
    batch, t_batch = timed(lambda: resident.hip_image_warp_batch(probs, out=out2, work=work))
    singles, t_single = timed(lambda: [resident.hip_image_warp_batch([p], out=o, work=work)[0] for p, o in zip(probs, outs)])
    same = all(torch.equal(b, s_) for b, s_ in zip(batch, singles)) and torch.equal(batch[0], canvases[False])
    bytes_two = bytes_one + 3.0 * (cw1 * ch1 + h * w + h * w)
    line = {"row": "batch of two (baseline + result, mean blend) against two single calls", **common, "canvas2_w": cw1, "canvas2_h": ch1,
            **stats("batch_call", t_batch, bytes_two), **stats("single_calls", t_single, bytes_two), "batch_equals_single_calls": bool(same)}
    line["ratio_single_calls_over_batch"] = line["single_calls_seconds_median"] / line["batch_call_seconds_median"]
    lines.append(line)
    if not same:
        failed.append("the batched call and the single calls differ")
    # the comparison row: grid_sample on the same canvas (float32 planes in, float32 planes out, the grid made beforehand)
    Minv = torch.from_numpy(np.linalg.inv(M)).to(dev)
    ys, xs = torch.meshgrid(torch.arange(ch, device=dev, dtype=torch.float64), torch.arange(cw, device=dev, dtype=torch.float64),
                            indexing="ij")
    X = Minv[0, 0] * xs + Minv[0, 1] * ys + Minv[0, 2]
    Y = Minv[1, 0] * xs + Minv[1, 1] * ys + Minv[1, 2]
    W = Minv[2, 0] * xs + Minv[2, 1] * ys + Minv[2, 2]
    grid = torch.stack([(X / W + 0.5) / w * 2 - 1, (Y / W + 0.5) / h * 2 - 1], dim=-1).float()[None]
    del xs, ys, X, Y, W
    planes = src.permute(2, 0, 1)[None].float().contiguous()
    _, t_gs = timed(lambda: F.grid_sample(planes, grid, mode="bilinear", padding_mode="zeros", align_corners=False))
    lines.append({"row": "torch.nn.functional.grid_sample on the same canvas (float32, no blend, grid prepared: the time only)", **common,
                  "grid_sample_seconds_median": float(np.median(t_gs)), "grid_sample_seconds_min": float(min(t_gs)),
                  "ratio_grid_sample_over_direct_call": float(np.median(t_gs)) / lines[0]["call_seconds_median"]})
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for line in lines:
            print(json.dumps(line))
            f.write(json.dumps(line) + "\n")
    if failed:
        raise SystemExit("image_warp_rate: " + "; ".join(failed))


if __name__ == "__main__":
    main()
