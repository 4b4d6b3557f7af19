#!/usr/bin/env python3
"""Time the bilinear sampler (APAP_OPT_WARP_SAMPLING = 1: k_warp_bilinear, k_panorama's bilinear forms) on the GPU beside the
truncating kernels it stands next to.

    python tools/warp_bilinear_rate.py [--reps 30] [--warmup 5] [--burst 10] [--out profiles/warp_bilinear_rate.jsonl]

One JSON line per row, printed and APPENDED to --out.

Pair rows (configuration C3: 3840 x 2160 pictures, mesh 200 x 200, canvas 4009 x 2242; resident data, the set-up phases run
once on a ``WarpPlan``, only the gather is timed), the warp and the fused stitch: three forms in one alternation -
``bilinear`` (k_warp_bilinear), ``rows_f64`` (the truncating all-float64 strips, APAP_OPT_WARP_FAST = 0: the same coordinate
arithmetic) and ``fast`` (the default k_warp_fast).  A sample is --burst gathers back to back between two events, divided by
--burst; the forms take turns sample by sample; median and minimum of --reps samples after --warmup.  Beside each time the
algorithmic bytes - the source once, the canvas once, for the stitch the centre once - over it as a fraction of 8 TB/s.  The
warp row also times ``torch.nn.functional.grid_sample(mode="bilinear", align_corners=True)`` in the same alternation, on the
same canvas with everything it needs prepared outside the clock: the picture as float32 (1, 3, h, w), the normalised float32
grid of the engine's own coordinates; it writes float32 and does no presence test, no fixed point and no byte packing, so
it is an outside yardstick for the gather, not the same function.

Panorama rows (the 4K five-view case of tools/panorama_rate.py: C3's centre and four neighbours): every blend with both
samplers in one alternation, one fused call per sample.

No time is a pass condition; the tool fails without a GPU, when a canvas differs between two calls of one form, and when the
bilinear and truncating canvases have different footprints on pictures without a black pixel."""
import argparse
import hashlib
import importlib.util
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_BYTES_PER_SECOND = 8.0e12
RAMP = 64


def stats(ts):
    return {"seconds_median": float(np.median(ts)), "seconds_min": float(min(ts))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--burst", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "warp_bilinear_rate.jsonl"))
    ap.add_argument("--no-panorama", action="store_true", help="the pair rows only")
    ap.add_argument("--note", help="a string kept in every row (which build of the library, for instance)")
    a = ap.parse_args()
    if a.reps < 10 or a.warmup < 3 or a.burst < 1:
        raise SystemExit("warp_bilinear_rate: at least 10 timed samples after 3 warm-ups")
    import torch      # before the library: one HIP runtime per process
    from cvx_proj_amd import _native as N
    from cvx_proj_amd import resident
    from cvx_proj_amd.synth import config_pair
    if N.lib().apap_device_count() < 1 or not torch.cuda.is_available():
        raise SystemExit("warp_bilinear_rate: no HIP device (this tool measures the GPU; it has no CPU mode)")
    dev = torch.device("cuda", 0)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)      # noqa: E731
    sha = lambda t: hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()      # noqa: E731

    def alternate(forms, burst):
        """forms: [(name, fn)]; returns {name: [seconds per call]}"""
        for _ in range(a.warmup):
            for _, fn in forms:
                for _ in range(burst):
                    fn()
        torch.cuda.synchronize(dev)
        times = {name: [] for name, _ in forms}
        for _ in range(a.reps):
            for name, fn in forms:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(burst):
                    fn()
                e1.record()
                e1.synchronize()
                times[name].append(e0.elapsed_time(e1) * 1e-3 / burst)
        return times

    lines, failed = [], []
    contexts = {"bilinear": N.Context(warp_sampling=N.SAMPLING_BILINEAR), "rows_f64": N.Context(warp_fast=0), "fast": N.Context()}

    # ---- the C3 pair
    p = config_pair("C3")
    rows, cols = p.vertices.shape[:2]
    H0, _ = N.local_homography(p.src, p.dst, p.vertices, p.gamma, p.sigma, want_weights=False)
    img_h = np.maximum(p.img, 1)        # no black pixel: a footprint is then the set of non-zero canvas pixels
    img, H = up(img_h), up(H0.reshape(-1, 9))
    center = torch.randint(1, 256, p.shape, dtype=torch.uint8, device=dev)
    fw, fh = p.final_w, p.final_h
    plans = {k: resident.WarpPlan(p.mesh, (rows, cols), fw, fh, p.off_x, p.off_y, dev, ctx=c) for k, c in contexts.items()}
    outs = {k: torch.empty((1, fh, fw, 3), dtype=torch.uint8, device=dev) for k in contexts}
    for pl in plans.values():
        pl.begin()
        pl.cells(H)
    xy = torch.from_numpy(N.warp_coords(H0, p.mesh[0], p.mesh[1], fw, fh, p.off_x, p.off_y)).to(dev)
    grid = torch.stack([xy[..., 0] * (2.0 / (p.shape[1] - 1)) - 1.0, xy[..., 1] * (2.0 / (p.shape[0] - 1)) - 1.0], dim=-1).float()[None]
    grid = torch.nan_to_num(grid, nan=-2.0, posinf=-2.0, neginf=-2.0).contiguous()
    img_f = img.permute(2, 0, 1)[None].float().contiguous()
    del xy

    for what, cen in (("warp", None), ("stitch", center)):
        forms = [(k, (lambda k=k: plans[k].gather(img, out=outs[k], centers=cen))) for k in contexts]
        if cen is None:
            forms.append(("grid_sample_f32", lambda: torch.nn.functional.grid_sample(img_f, grid, mode="bilinear", padding_mode="zeros",
                                                                                    align_corners=True)))
        times = alternate(forms, a.burst)
        shas = {k: sha(outs[k]) for k in contexts}
        for k in contexts:
            plans[k].gather(img, out=outs[k], centers=cen)
            if sha(outs[k]) != shas[k]:
                failed.append(f"C3 {what}, {k}: two calls, two canvases")
        if shas["rows_f64"] != shas["fast"]:
            failed.append(f"C3 {what}: the two truncating kernels differ")
        if cen is None and not torch.equal((outs["bilinear"] != 0).any(dim=-1), (outs["fast"] != 0).any(dim=-1)):
            failed.append("C3 warp: the bilinear and the truncating footprints differ")
        nbytes = 3.0 * (img.shape[0] * img.shape[1] + fw * fh + (0 if cen is None else cen.shape[0] * cen.shape[1]))
        line = {"row": f"C3 pair, {what}: 3840x2160, mesh 200, canvas {fw}x{fh}", "reps": a.reps, "warmup": a.warmup, "burst": a.burst,
                "algorithmic_bytes": nbytes, "status": [plans[k].status_word() for k in contexts]}
        for k, ts in times.items():
            s = stats(ts)
            line[k] = dict(s, fraction_of_8TBps=nbytes / PEAK_BYTES_PER_SECOND / s["seconds_median"], **({"sha256": shas[k]} if k in shas else {}))
        line["ratio_bilinear_over_rows_f64"] = line["bilinear"]["seconds_median"] / line["rows_f64"]["seconds_median"]
        line["ratio_bilinear_over_fast"] = line["bilinear"]["seconds_median"] / line["fast"]["seconds_median"]
        lines.append(line)
    del grid, img_f, plans, outs

    # ---- the 4K five-view panorama of tools/panorama_rate.py
    spec = importlib.util.spec_from_file_location("panorama_rate", os.path.join(ROOT, "tools", "panorama_rate.py"))
    pano = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(pano)
    center_h, layers_h = pano.build_case(3840, 2160, 200, 2160)
    center = up(center_h)
    layers = [N.PanoramaLayer(up(im), up(Hl), (up(e[0]), up(e[1])), size, off) for im, Hl, e, size, off in layers_h]
    geo = np.array([list(l.final_size) + list(l.offset) for l in layers], dtype=np.int32)
    W, Hc, OX, OY = N.panorama_bounds(center.shape, geo[:, 0], geo[:, 1], geo[:, 2], geo[:, 3])
    work = torch.empty(resident.panorama_workspace_bytes(layers), dtype=torch.uint8, device=dev)
    status = torch.zeros(len(layers), dtype=torch.int32, device=dev)
    pouts = {k: torch.empty((Hc, W, 3), dtype=torch.uint8, device=dev) for k in ("bilinear", "fast")}
    nbytes = 3.0 * (sum(l.img.shape[0] * l.img.shape[1] for l in layers) + center.shape[0] * center.shape[1] + Hc * W)
    for mode in () if a.no_panorama else ("mean", "paste", "ramp"):
        forms = [(k, (lambda k=k: resident.hip_panorama(center, layers, blend=mode, out=pouts[k], status=status, work=work, ramp=RAMP,
                                                        ctx=contexts[k]))) for k in ("bilinear", "fast")]
        times = alternate(forms, 1)
        line = {"row": f"C3 panorama: 3840x2160, mesh 200, K = 4, {mode}" + (f" {RAMP}" if mode == "ramp" else ""), "canvas_w": W,
                "canvas_h": Hc, "reps": a.reps, "warmup": a.warmup, "algorithmic_bytes": nbytes, "status": status.tolist()}
        for k, name in (("bilinear", "bilinear"), ("fast", "nearest")):
            s = stats(times[k])
            line[name] = dict(s, fraction_of_8TBps=nbytes / PEAK_BYTES_PER_SECOND / s["seconds_median"], sha256=sha(pouts[k]))
        line["ratio_bilinear_over_nearest"] = line["bilinear"]["seconds_median"] / line["nearest"]["seconds_median"]
        lines.append(line)

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        for line in lines:
            if a.note:
                line["note"] = a.note
            print(json.dumps(line))
            f.write(json.dumps(line) + "\n")
    if failed:
        raise SystemExit("warp_bilinear_rate: " + "; ".join(failed))


if __name__ == "__main__":
    main()
