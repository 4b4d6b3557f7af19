#!/usr/bin/env python3
"""Time the dehazing (cvx_proj_amd.resident.hip_dehaze) on the GPU beside the same definition written with torch ops on resident
tensors - window minima by max_pool2d of the negated plane, the selection by bincount / cumsum / argmax, the box sums by two
int64 cumsums over the border-replicated plane, floor divisions by torch.div - the two alternating call by call.

    python tools/dehaze_rate.py [--reps 20] [--warmup 3] [--out profiles/dehaze_rate.jsonl]

One JSON line per shape (768 x 768 x 3 and 3840 wide x 2160 high x 3) and setting (the defaults, refine = 0, 8 and 32), printed and
written to --out (afresh).  Pictures on the device before the clock starts, the workspace allocated once; every call bracketed by
two events on its stream; median and minimum of --reps calls after --warmup.  Timing is reported, not judged; the two chains are
both exact integers, and the number of bytes in which their pictures differ is reported too (0 expected)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
# bytes a pixel that the kernels must move for a BGR picture (csrc/apap_dehaze.hip: I 3, D 1, p 2, a_q 4, b_q 8, J 3):
# D1 3 + 1, D2 1, D3 3 + 2, D4 3 + 2 + 12, D5 12 + 3 + 3; without refinement D4 goes and D5 reads p for a_q and b_q
BYTES_REFINED, BYTES_PLAIN = 45, 18


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dehaze_rate.jsonl"))
    a = ap.parse_args()
    if a.reps < 20 or a.warmup < 3:
        raise SystemExit("dehaze_rate: at least 20 timed calls after 3 warm-ups")
    import torch      # before the library: one HIP runtime per process
    import torch.nn.functional as F
    from cvx_proj_amd import _native, resident
    from cvx_proj_amd.dehaze import dehaze_arguments
    if _native.lib().apap_device_count() < 1 or not torch.cuda.is_available():
        raise SystemExit("dehaze_rate: no HIP device (this tool measures the GPU; it has no CPU mode)")
    dev = torch.device("cuda", 0)

    def event_timed(fns):
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

    def window_min(x, r):       # x (h, w) float32 holding integers below 2^24: max_pool2d pads with -inf, the clipped window
        return -F.max_pool2d(-x[None, None], 2 * r + 1, stride=1, padding=r)[0, 0] if r else x

    def box_sum(x, r):          # x (h, w) int64
        h, w = x.shape
        ys = torch.arange(-r - 1, h + r, device=dev).clamp(0, h - 1)
        xs = torch.arange(-r - 1, w + r, device=dev).clamp(0, w - 1)
        c = x[ys][:, xs].cumsum(0).cumsum(1)
        n = 2 * r + 1
        return c[n:, n:] - c[:-n, n:] - c[n:, :-n] + c[:-n, :-n]

    def torch_chain(pic, radius, omega_q, t0_q, refine, eps):
        h, w, _ = pic.shape
        I = pic.to(torch.int64)
        D = window_min(pic.amin(dim=2).to(torch.float32), radius).to(torch.int64)
        k = max(1, h * w // 1000)
        at_least = torch.bincount(D.reshape(-1), minlength=256).flip(0).cumsum(0).flip(0)
        T = ((at_least >= k) * torch.arange(256, device=dev)).max()
        sums = torch.where(D.reshape(-1) >= T, I.reshape(-1, 3).sum(1), -1)
        A = I.reshape(-1, 3)[sums.argmax()].clamp(min=1)
        n = torch.div(4096 * I, A, rounding_mode="floor").amin(dim=2).clamp(max=4096)
        Dn = window_min(n.to(torch.float32), radius).to(torch.int64)
        t = 4096 - ((omega_q * Dn + 128) >> 8)
        if refine:
            G = (3735 * I[..., 0] + 19235 * I[..., 1] + 9798 * I[..., 2] + 16384) >> 15
            W = (2 * refine + 1) ** 2
            sG, sp = box_sum(G, refine), box_sum(t, refine)
            covN = W * box_sum(G * t, refine) - sG * sp
            varN = W * box_sum(G * G, refine) - sG * sG
            a_q = torch.div(4096 * covN, varN + eps * W * W, rounding_mode="floor")
            b_q = 4096 * sp - a_q * sG
            t = torch.div(box_sum(a_q, refine) * G * W + box_sum(b_q, refine), 4096 * W * W, rounding_mode="floor")
        t = t.clamp(t0_q, 4096)[..., None]
        return (A + torch.div(8192 * (I - A) + t, 2 * t, rounding_mode="floor")).clamp(0, 255).to(torch.uint8)

    lines = []
    for h, w in ((768, 768), (2160, 3840)):
        rng = np.random.default_rng(h)
        # a hazy picture, not noise: blocks of colour under a depth ramp (noise has a dark channel of zero everywhere)
        J = np.repeat(np.repeat(rng.integers(0, 256, ((h + 7) // 8, (w + 7) // 8, 3), dtype=np.uint8), 8, axis=0), 8, axis=1)[:h, :w]
        t = np.linspace(0.9, 0.08, w)[None, :, None]
        pic = torch.from_numpy(np.floor(J * t + np.array([225.0, 232.0, 240.0]) * (1 - t) + 0.5).astype(np.uint8)).to(dev)
        out = torch.empty_like(pic)
        work = torch.empty(resident.dehaze_workspace_bytes(1, h, w, 3, 32), dtype=torch.uint8, device=dev)
        for name, kw in (("defaults", dict()), ("refine0", dict(refine=0)), ("refine8", dict(refine=8)), ("refine32", dict(refine=32))):
            q = dehaze_arguments(**kw)
            times = event_timed([lambda: resident.hip_dehaze(pic, out=out, work=work, **kw), lambda: torch_chain(pic, *q)])
            differ = int((resident.hip_dehaze(pic, out=out, work=work, **kw) != torch_chain(pic, *q)).sum())
            per_pixel = BYTES_REFINED if q[3] else BYTES_PLAIN
            line = {"row": f"{h}x{w}x3 {name}", "h": h, "w": w, "radius": q[0], "refine": q[3], "reps": a.reps, "warmup": a.warmup,
                    "bytes_that_differ": differ}
            for prefix, ms in zip(("engine", "torch_chain"), times):
                line.update({prefix + "_us_median": float(np.median(ms)) * 1e3, prefix + "_us_min": float(min(ms)) * 1e3})
            line["ratio_torch_chain_over_engine"] = line["torch_chain_us_median"] / line["engine_us_median"]
            line["algorithmic_bytes"] = per_pixel * h * w
            line["floor_us_at_8TBs"] = per_pixel * h * w / 8e12 * 1e6
            lines.append(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for line in lines:
            print(json.dumps(line))
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
