#!/usr/bin/env python3
"""Time the panorama's two-band blend on the GPU, at the 4K five-view shape of tools/panorama_rate.py (a 3840 x 2160 centre,
four neighbours, meshes of 200 x 200) and at 768 x 768 (five views, meshes of 20 x 20), resident data, every form of a shape
in ONE alternation: call by call in one process, every timed call between two events on its stream, median and minimum of
--reps calls after --warmup.

    python tools/panorama_band_rate.py [--reps 20] [--warmup 3] [--baseline-lib libapap_hip_parent.so]
                                       [--out profiles/panorama_band_rate.jsonl]

Rows, one JSON line each, printed and APPENDED to --out:
  (a) <blend> [gained]  the untouched forms, mean / paste / ramp 64, ungained and under seeded gains - and, with
                        --baseline-lib (a build of the parent commit's library), the same call through that library in the same
                        alternation, twice, so that the spread of two runs of the parent stands beside the difference
  (b) band r, sampling  the two-band blend at ramp 64 and radii 0, 8 and 32, under nearest and bilinear sampling (the blur of
                        all five views is part of the call)
  (c) box blur r        k_box_blur alone on ONE picture of the shape, radii 8 and 32
  (d) torch chain       the same definition (radius 8, nearest) in torch operations: every picture's low-pass picture from a
                        summed-area table, three hip_warp_batch canvases per layer (the picture, its low-pass picture, and its
                        border distances as bytes), everything placed on the union canvas, then the sums, the best view and
                        the clip
A round runs every form once in this order; round r starts at form r, and one untimed plain call follows the torch chain.
The one pass / fail criterion: with --baseline-lib every untouched form's median lies within the spread of the two parent
runs, from the lowest lower quartile to the highest upper quartile of their timed calls.  The tool also fails without a GPU, when band 0 differs from the ramp blend, when
the parent library's canvas differs, and when the torch chain's canvas differs from the kernel's."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

RAMP = 64
BLENDS = (("mean", 1), ("paste", 1), ("ramp", RAMP))
PARENT_SYMBOLS = ("apap_panorama_device", "apap_panorama_ramp_device", "apap_panorama_gain_device", "apap_panorama_workspace_bytes",
                  "apap_panorama_bounds")


def run_shape(a, torch, _native, resident, this_lib, parent, label, w, h, mesh, seed, lines, failed):
    from panorama_rate import build_case
    dev = torch.device("cuda", 0)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)      # noqa: E731
    center_h, layers_h = build_case(w, h, mesh, seed)
    center = up(center_h)
    layers = [_native.PanoramaLayer(up(img), up(H), (up(e[0]), up(e[1])), size, off) for img, H, e, size, off in layers_h]
    K = len(layers)
    geo = np.array([list(l.final_size) + list(l.offset) for l in layers], dtype=np.int32)
    W, Hc, OX, OY = _native.panorama_bounds(center.shape, geo[:, 0], geo[:, 1], geo[:, 2], geo[:, 3])
    out = torch.empty((Hc, W, 3), dtype=torch.uint8, device=dev)
    work = torch.empty(resident.panorama_band_workspace_bytes(center, layers, 32), dtype=torch.uint8, device=dev)
    status = torch.zeros(K, dtype=torch.int32, device=dev)
    q_seeded = np.random.default_rng(7).integers(3000, 5500, K + 1).tolist()
    ch, cw = center.shape[:2]
    blur_out = torch.empty_like(center)

    def untouched(lib, blend, ramp, q):
        _native._lib = lib      # the resident wrapper calls through whatever library the binding holds
        try:
            status.zero_()
            return resident.hip_panorama(center, layers, blend=blend, out=out, status=status, work=work, ramp=ramp, gain=q)[0]
        finally:
            _native._lib = this_lib

    def band(r, sampling):
        status.zero_()
        return resident.hip_panorama(center, layers, blend="band", out=out, status=status, work=work, ramp=RAMP, band=r, sampling=sampling)[0]

    # the chain in torch
    def low_pass(img, r):
        n = 2 * r + 1
        hh, ww = img.shape[:2]
        ys = torch.arange(-r, hh + r, device=dev).clamp(0, hh - 1)
        xs = torch.arange(-r, ww + r, device=dev).clamp(0, ww - 1)
        c = torch.zeros((hh + 2 * r + 1, ww + 2 * r + 1, 3), dtype=torch.int32, device=dev)     # may wrap; the differences below are exact
        c[1:, 1:] = img[ys][:, xs].to(torch.int32).cumsum(0, dtype=torch.int32).cumsum(1, dtype=torch.int32)
        T = c[n:, n:] - c[:-n, n:] - c[n:, :-n] + c[:-n, :-n]
        return torch.div(T + (n * n >> 1), n * n, rounding_mode="floor").to(torch.uint8)

    def distance_bytes(hh, ww):
        x, y = torch.arange(ww, device=dev)[None, :], torch.arange(hh, device=dev)[:, None]
        d = torch.minimum(torch.minimum(x + 1, ww - x), torch.minimum(y + 1, hh - y))
        return torch.stack([d & 255, d >> 8, torch.ones_like(d)], dim=-1).to(torch.uint8).contiguous(), d

    dist = [distance_bytes(*l.img.shape[:2])[0] for l in layers]
    center_d = distance_bytes(ch, cw)[1]
    pair_out = [torch.empty((1, l.final_size[1], l.final_size[0], 3), dtype=torch.uint8, device=dev) for l in layers]
    pair_work = [torch.empty(resident.warp_workspace_bytes(l.local_homography.shape[:2], *l.final_size), dtype=torch.uint8, device=dev)
                 for l in layers]
    pair_status = [torch.zeros(1, dtype=torch.int32, device=dev) for _ in layers]
    stack = torch.empty((3, K + 1, Hc, W, 3), dtype=torch.uint8, device=dev)    # c, b, D as bytes
    chain_out = torch.empty((Hc, W, 3), dtype=torch.uint8, device=dev)

    def torch_chain(r=8):
        stack.zero_()
        stack[0, 0, OY:OY + ch, OX:OX + cw] = center
        stack[1, 0, OY:OY + ch, OX:OX + cw] = low_pass(center, r)
        D = torch.zeros((K + 1, Hc, W), dtype=torch.int32, device=dev)
        D[0, OY:OY + ch, OX:OX + cw] = center_d
        for k, (l, o, wk, st) in enumerate(zip(layers, pair_out, pair_work, pair_status)):
            rows, cols = l.local_homography.shape[:2]
            y0, x0 = OY - l.offset[1], OX - l.offset[0]
            for which, pic in enumerate((l.img, low_pass(l.img, r), dist[k])):
                resident.hip_warp_batch(pic, l.local_homography.view(1, rows * cols, 9), l.mesh[0], l.mesh[1], l.final_size[0],
                                        l.final_size[1], l.offset[0], l.offset[1], (rows, cols), out=o, work=wk, status=st)
                stack[which, k + 1, y0:y0 + o.shape[1], x0:x0 + o.shape[2]] = o[0]
            D[k + 1] = stack[2, k + 1, :, :, 0].to(torch.int32) | (stack[2, k + 1, :, :, 1].to(torch.int32) << 8)
        present = (stack[0] != 0).any(dim=-1)
        D = torch.where(present, D, torch.zeros_like(D))
        wt = D.clamp(max=RAMP)
        low = stack[1].to(torch.int32)
        L = torch.div((wt[..., None] * low).sum(dim=0), wt.sum(dim=0).clamp(min=1)[..., None], rounding_mode="floor")
        s = D.argmax(dim=0)             # the first index of the largest D
        idx = s[None, ..., None].expand(1, Hc, W, 3)
        detail = stack[0].to(torch.int32).gather(0, idx)[0] - low.gather(0, idx)[0]
        chain_out.copy_((L + detail).clamp(0, 255).to(torch.uint8))
        return chain_out

    forms = []
    for gained in (False, True):
        q = q_seeded if gained else None
        tag = ", gained" if gained else ""
        for blend, ramp in BLENDS:
            if parent is not None:
                forms.append((f"{blend}{tag}, parent library", "a", lambda b=blend, r=ramp, q=q: untouched(parent, b, r, q)))
            forms.append((f"{blend}{tag}", "a", lambda b=blend, r=ramp, q=q: untouched(this_lib, b, r, q)))
            if parent is not None:
                forms.append((f"{blend}{tag}, parent library again", "a", lambda b=blend, r=ramp, q=q: untouched(parent, b, r, q)))
    for sampling in ("nearest", "bilinear"):
        for r in (0, 8, 32):
            forms.append((f"band {r}, {sampling}", "b", lambda r=r, s=sampling: band(r, s)))
    for r in (8, 32):
        forms.append((f"box blur {r}, one picture", "c", lambda r=r: resident.hip_box_blur(center, r, out=blur_out)))
    forms.append(("torch chain band 8, nearest", "d", torch_chain))

    # the checks, outside the clock
    for sampling in ("nearest", "bilinear"):
        status.zero_()
        want = resident.hip_panorama(center, layers, blend="ramp", out=out, status=status, work=work, ramp=RAMP, sampling=sampling)[0].clone()
        if not torch.equal(band(0, sampling), want):
            failed.append(f"{label}: band 0 differs from the ramp blend ({sampling})")
    if parent is not None:
        for blend, ramp in BLENDS:
            for q in (None, q_seeded):
                want = untouched(this_lib, blend, ramp, q).clone()
                if not torch.equal(untouched(parent, blend, ramp, q), want):
                    failed.append(f"{label}: {blend}: the parent library's canvas differs")
    chain_equal = bool(torch.equal(torch_chain().clone(), band(8, "nearest")))
    if not chain_equal:
        failed.append(f"{label}: the torch chain's canvas differs from the kernel's")

    for _ in range(a.warmup):
        for _, _, fn in forms:
            fn()
    torch.cuda.synchronize(dev)
    times = [[] for _ in forms]
    for r in range(a.reps):
        # Round r starts at form r, so that no form always follows the same neighbour; one untimed plain call separates the
        # torch chain, with its gigabytes of temporaries, from the form after it.
        for i in range(len(forms)):
            (name, _, fn), t = forms[(r + i) % len(forms)], times[(r + i) % len(forms)]
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            t.append(e0.elapsed_time(e1) * 1e-3)
            if name.startswith("torch chain"):
                untouched(this_lib, "mean", 1, None)
    med = {name: float(np.median(t)) for (name, _, _), t in zip(forms, times)}
    by_name = {name: t for (name, _, _), t in zip(forms, times)}
    for (name, group, _), t in zip(forms, times):
        line = {"row": f"{label}: {w}x{h}, mesh {mesh}, K = {K}, {name}", "group": group, "canvas_w": W, "canvas_h": Hc, "reps": a.reps,
                "warmup": a.warmup, "seconds_median": med[name], "seconds_min": float(min(t)), "seconds_max": float(max(t))}
        if name.startswith("torch chain"):
            line["canvas_equal_band"] = chain_equal
        if group == "a" and parent is not None and "parent" not in name:
            # Two medians of 20 can lie closer together than either is known: the spread of a parent run is taken as the
            # quartiles of its timed calls, and the two runs' spread as the lowest lower and the highest upper quartile.
            runs = [by_name[name + ", parent library"], by_name[name + ", parent library again"]]
            lo = min(float(np.percentile(t, 25)) for t in runs)
            hi = max(float(np.percentile(t, 75)) for t in runs)
            line["parent_medians"] = [float(np.median(t)) for t in runs]
            line["parent_spread"] = [lo, hi]
            line["within_parent_spread"] = bool(lo <= med[name] <= hi)
            if not line["within_parent_spread"]:
                failed.append(f"{label}: {name}: {med[name] * 1e6:.1f} us outside the parent's {lo * 1e6:.1f} .. {hi * 1e6:.1f} us")
        lines.append(line)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--baseline-lib", default=None, help="a build of the parent commit's library for the rows (a)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "panorama_band_rate.jsonl"))
    a = ap.parse_args()
    if a.reps < 10 or a.warmup < 3:
        raise SystemExit("panorama_band_rate: at least 10 timed calls after 3 warm-ups")
    import torch      # before the library: one HIP runtime per process
    from cvx_proj_amd import _native, resident
    if _native.lib().apap_device_count() < 1 or not torch.cuda.is_available():
        raise SystemExit("panorama_band_rate: no HIP device (this tool measures the GPU; it has no CPU mode)")
    this_lib = _native.lib()
    parent = None
    if a.baseline_lib:
        parent = ctypes.CDLL(os.path.abspath(a.baseline_lib))
        for sym in PARENT_SYMBOLS:
            getattr(parent, sym).restype, getattr(parent, sym).argtypes = _native.SIGNATURES[sym]
    lines, failed = [], []
    run_shape(a, torch, _native, resident, this_lib, parent, "C3", 3840, 2160, 200, 2160, lines, failed)
    run_shape(a, torch, _native, resident, this_lib, parent, "C1", 768, 768, 20, 768, lines, failed)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        for line in lines:
            print(json.dumps(line))
            f.write(json.dumps(line) + "\n")
    if failed:
        raise SystemExit("panorama_band_rate: " + "; ".join(failed))


if __name__ == "__main__":
    main()
