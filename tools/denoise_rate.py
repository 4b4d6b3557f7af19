#!/usr/bin/env python3
"""Time the notch denoising (cvx_proj_amd.resident.hip_notch_denoise) on the GPU beside the same chain written with torch ops on
resident tensors - per-channel equalisation left out of both, ``torch.fft.fft2`` in complex128, the notch as 308 masked
lexicographic medians, ``ifft2``, ``abs`` - the two alternating call by call.

    python tools/denoise_rate.py [--reps 20] [--warmup 3] [--out profiles/denoise_rate.jsonl]

One JSON line per shape (768 x 768 x 3 and 3840 wide x 2160 high x 3, both 5-smooth), printed and written to --out (afresh).
Besides the whole call: the equalisation alone, the forward transform alone (rows and columns: two launches) against
``torch.fft.fft2`` on the same planes, the notch launch alone, the inverse transform alone.  Pictures on the device before the
clock starts, workspaces allocated once; every call bracketed by two events on its stream; median and minimum of --reps calls
after --warmup.  Timing is reported, not judged, and so is the largest pixel difference of the two chains: a disc of a real
picture's spectrum can hold two values whose real parts agree to rounding (Hermitian symmetry), the two transforms may order them
differently, and a disc that takes another median moves pixels by about 1."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SPACING, R, SN = 48, 5, 9


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "denoise_rate.jsonl"))
    a = ap.parse_args()
    if a.reps < 20 or a.warmup < 3:
        raise SystemExit("denoise_rate: at least 20 timed calls after 3 warm-ups")
    import torch      # before the library: one HIP runtime per process
    from cvx_proj_amd import _native, denoise, resident
    if _native.lib().apap_device_count() < 1 or not torch.cuda.is_available():
        raise SystemExit("denoise_rate: no HIP device (this tool measures the GPU; it has no CPU mode)")
    dev = torch.device("cuda", 0)
    lib = _native.lib()

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

    def stats(prefix, ms):
        return {prefix + "_us_median": float(np.median(ms)) * 1e3, prefix + "_us_min": float(min(ms)) * 1e3}

    def torch_chain(planes, masks):
        """planes (c, h, w) uint8 -> (c, h, w) float64; masks: per assignment (write index, read index) into the flat plane."""
        f = torch.fft.fftshift(torch.fft.fft2(planes.to(torch.complex128)), dim=(-2, -1)).reshape(planes.shape[0], -1)
        for write, read in masks:
            v = f[:, read]
            n = v.shape[1]
            order = torch.sort(v.imag, dim=1, stable=True).indices
            order = torch.gather(order, 1, torch.sort(torch.gather(v.real, 1, order), dim=1, stable=True).indices)
            s = torch.gather(v, 1, order)
            f[:, write] = ((s[:, (n - 1) // 2] + s[:, n // 2]) / 2)[:, None]
        return torch.fft.ifft2(torch.fft.ifftshift(f.reshape(planes.shape), dim=(-2, -1))).abs()

    def masks_of(h, w):
        out = []
        for uk, vk, r1, r2 in denoise.notch_schedule(SPACING, R, SN):
            for cx, cy in ((w // 2 + uk, h // 2 + vk), (w // 2 + uk, h // 2 - vk), (w // 2 - uk, h // 2 + vk), (w // 2 - uk, h // 2 - vk)):
                ys, xs = np.arange(max(0, cy - r2), min(h, cy + r2 + 1)), np.arange(max(0, cx - r2), min(w, cx + r2 + 1))
                d2 = (xs[None, :] - cx) ** 2 + (ys[:, None] - cy) ** 2
                at = ys[:, None] * w + xs[None, :]
                if (d2 <= r2 * r2).any():
                    out.append((torch.from_numpy(at[d2 <= r1 * r1]).to(dev), torch.from_numpy(at[d2 <= r2 * r2]).to(dev)))
        return out

    lines = []
    for h, w, c in ((768, 768, 3), (2160, 3840, 3)):
        rng = np.random.default_rng(h)
        pic = torch.from_numpy(rng.integers(0, 256, (h, w, c), dtype=np.uint8)).to(dev)
        planes = pic.permute(2, 0, 1).contiguous()
        masks = masks_of(h, w)
        work = torch.empty(resident.notch_denoise_workspace_bytes(1, h, w, c), dtype=torch.uint8, device=dev)
        spec = torch.fft.fft2(planes.to(torch.complex128)).contiguous()
        spec_out = torch.empty_like(spec)
        fwork = torch.empty(max(lib.apap_fft2_workspace_bytes(c, h, w), 256), dtype=torch.uint8, device=dev)
        eq_out = torch.empty_like(pic)
        eq_work = torch.zeros(lib.apap_equalize_workspace_bytes(c), dtype=torch.uint8, device=dev)
        stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        calls = [
            lambda: resident.hip_notch_denoise(pic, SPACING, R, SN, equalize=False, work=work),
            lambda: torch_chain(planes, masks),
            lambda: resident.hip_notch_denoise(pic, SPACING, R, SN, equalize=True, work=work),
            lambda: _native.check(lib.apap_equalize_hist_device(None, pic.data_ptr(), h, w, c, eq_out.data_ptr(), eq_work.data_ptr(),
                                                                eq_work.numel(), stream)),
            lambda: resident.hip_fft2(spec, work=fwork, out=spec_out),
            lambda: torch.fft.fft2(spec),
            lambda: _native.check(lib.apap_notch_spectrum_device(None, spec_out.data_ptr(), c, h, w, SPACING, R, SN, stream)),
            lambda: resident.hip_fft2(spec, inverse=True, work=fwork, out=spec_out),
        ]
        names = ["engine_no_equalize", "torch_chain", "engine", "equalize", "fft2_forward", "torch_fft2", "notch", "fft2_inverse"]
        times = event_timed(calls)
        ours = resident.hip_notch_denoise(pic, SPACING, R, SN, equalize=False, work=work).permute(2, 0, 1)
        apart = float((ours - torch_chain(planes, masks)).abs().max())
        line = {"row": f"{h}x{w}x{c}", "h": h, "w": w, "channels": c, "reps": a.reps, "warmup": a.warmup, "max_abs_difference": apart}
        for name, t in zip(names, times):
            line.update(stats(name, t))
        line["ratio_torch_chain_over_engine"] = line["torch_chain_us_median"] / line["engine_no_equalize_us_median"]
        line["ratio_torch_fft2_over_engine_fft2"] = line["torch_fft2_us_median"] / line["fft2_forward_us_median"]
        line["floor_us_at_8TBs"] = 860e6 * c * h * w / (3840 * 2160) / 8e12 * 1e6
        lines.append(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for line in lines:
            print(json.dumps(line))
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
