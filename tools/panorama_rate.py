#!/usr/bin/env python3
"""Time the panorama (cvx_proj_amd.resident.hip_panorama: K set-up launches and one fused pass over the union canvas) on the
GPU beside the chain a caller had to write before it: K ``hip_warp_batch`` calls, one pair canvas each, and the composition
in torch operations on the device.

    python tools/panorama_rate.py [--reps 20] [--warmup 3] [--out profiles/panorama_rate.jsonl]

One JSON line per row, printed and APPENDED to --out.  Rows: a centre picture of configuration C3's size (3840 x 2160, mesh
200 x 200) with K = 4 neighbours placed to its left, right, top and bottom, and the same at C1's size (768 x 768, mesh 20 x
20), each in the blends ``mean`` and ``paste`` and in ``ramp`` at ramp width 64.  Seeded pictures and grids (a global placement times I + 1e-3 x a smooth function of the cell),
resident on the device before the clock starts; outputs, workspaces and status words allocated beforehand.  The two forms
alternate call by call in one process, every timed call between two events on its stream; median and minimum of --reps
calls after --warmup.

Beside each time: the algorithmic bytes - every source once, the centre once, the canvas once - over the fused call's time as
a fraction of 8 TB/s, next to 0.43, what the fused per-pair warp + blend kernel is recorded at.  No time is a pass condition;
the tool fails without a GPU, and when the SHA-256 of the panorama differs from the baseline's.

The chain has no ramp: a weight of the source pixel is lost once a layer is a finished canvas.  A ``ramp`` row therefore times
three forms in the same alternation - the fused ramp, the fused ``mean`` and the ``mean`` chain - and reports the ramp over
each of the two yardsticks; its check is that ramp width 1 gives the SHA-256 of the fused ``mean``."""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_BYTES_PER_SECOND = 8.0e12
K3_FRACTION = 0.43
RAMP = 64       # the ramp width of the `ramp` rows


class _Shape:
    def __init__(self, shape):
        self.shape = shape


def build_case(w, h, mesh, seed):
    """Centre and four neighbours of w x h pixels, shifted by 0.4 of a side with a small rotation and perspective."""
    from cvx_proj_amd import geometry
    rng = np.random.default_rng(seed)
    center = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    layers = []
    for tx, ty, ang in ((-0.4 * w, 0.02 * h, 0.004), (0.4 * w, -0.03 * h, -0.003), (0.03 * w, -0.4 * h, 0.002), (-0.02 * w, 0.4 * h, -0.004)):
        c, s = np.cos(ang), np.sin(ang)
        Hg = np.array([[c, -s, tx], [s, c, ty], [1e-5 * 1920 / w, -2e-5 * 1920 / w, 1.0]])
        img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        fw, fh, ox, oy = (int(v) for v in geometry.final_size(_Shape(img.shape), _Shape(center.shape), Hg))
        edges = geometry.get_mesh((fw, fh), mesh + 1)
        r, q = np.meshgrid(np.arange(mesh) / mesh, np.arange(mesh) / mesh, indexing="ij")
        S = np.zeros((mesh, mesh, 3, 3))
        S[..., 0, 0], S[..., 0, 1], S[..., 0, 2] = np.sin(2 * r + q), np.cos(r - 3 * q), 0.3 * w * np.sin(3 * r) * np.cos(2 * q)
        S[..., 1, 0], S[..., 1, 1], S[..., 1, 2] = np.cos(r + 2 * q), np.sin(3 * r - q), 0.3 * h * np.cos(2 * r + q)
        S[..., 2, 0], S[..., 2, 1] = 1e-2 / w * np.sin(r + q), 1e-2 / h * np.cos(r - q)
        H = (Hg @ (np.eye(3) + 1e-3 * S)).astype(np.float32)
        layers.append((img, H, edges, (fw, fh), (ox, oy)))
    return center, layers


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "panorama_rate.jsonl"))
    a = ap.parse_args()
    if a.reps < 10 or a.warmup < 3:
        raise SystemExit("panorama_rate: at least 10 timed calls after 3 warm-ups")
    import torch      # before the library: one HIP runtime per process
    from cvx_proj_amd import _native, resident
    if _native.lib().apap_device_count() < 1 or not torch.cuda.is_available():
        raise SystemExit("panorama_rate: no HIP device (this tool measures the GPU; it has no CPU mode)")
    dev = torch.device("cuda", 0)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)      # noqa: E731

    def event_pair():
        return torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    lines, failed = [], []
    for name, w, h, mesh, seed in (("C3", 3840, 2160, 200, 2160), ("C1", 768, 768, 20, 31)):
        center_h, layers_h = build_case(w, h, mesh, seed)
        center = up(center_h)
        layers = [_native.PanoramaLayer(up(img), up(H), (up(e[0]), up(e[1])), size, off) for img, H, e, size, off in layers_h]
        K = len(layers)
        geo = np.array([list(l.final_size) + list(l.offset) for l in layers], dtype=np.int32)
        W, Hc, OX, OY = _native.panorama_bounds(center.shape, geo[:, 0], geo[:, 1], geo[:, 2], geo[:, 3])
        out = torch.empty((Hc, W, 3), dtype=torch.uint8, device=dev)
        work = torch.empty(resident.panorama_workspace_bytes(layers), dtype=torch.uint8, device=dev)
        status = torch.zeros(K, dtype=torch.int32, device=dev)
        # the chain: per layer its own canvas, workspace and status word, then torch on the device
        pair_out = [torch.empty((1, l.final_size[1], l.final_size[0], 3), dtype=torch.uint8, device=dev) for l in layers]
        pair_work = [torch.empty(resident.warp_workspace_bytes(l.local_homography.shape[:2], *l.final_size), dtype=torch.uint8, device=dev)
                     for l in layers]
        pair_status = [torch.zeros(1, dtype=torch.int32, device=dev) for _ in layers]
        total = torch.empty((Hc, W, 3), dtype=torch.int32, device=dev)
        count = torch.empty((Hc, W), dtype=torch.int32, device=dev)
        base_out = torch.empty((Hc, W, 3), dtype=torch.uint8, device=dev)
        ch, cw = center.shape[:2]

        def chain(mode):
            canvases = []
            for l, o, wk, st in zip(layers, pair_out, pair_work, pair_status):
                rows, cols = l.local_homography.shape[:2]
                resident.hip_warp_batch(l.img, l.local_homography.view(1, rows * cols, 9), l.mesh[0], l.mesh[1], l.final_size[0],
                                        l.final_size[1], l.offset[0], l.offset[1], (rows, cols), out=o, work=wk, status=st)
                canvases.append(o[0])
            if mode == "mean":
                total.zero_()
                count.zero_()
                total[OY:OY + ch, OX:OX + cw] += center
                count[OY:OY + ch, OX:OX + cw] += (center != 0).any(dim=-1)
                for l, c in zip(layers, canvases):
                    y0, x0 = OY - l.offset[1], OX - l.offset[0]
                    total[y0:y0 + c.shape[0], x0:x0 + c.shape[1]] += c
                    count[y0:y0 + c.shape[0], x0:x0 + c.shape[1]] += (c != 0).any(dim=-1)
                torch.div(total, count.clamp(min=1)[..., None], rounding_mode="floor", out=total)
                base_out.copy_(total)
            else:
                base_out.zero_()
                for l, c in reversed(list(zip(layers, canvases))):      # the first present layer wins: paste the last first
                    y0, x0 = OY - l.offset[1], OX - l.offset[0]
                    view = base_out[y0:y0 + c.shape[0], x0:x0 + c.shape[1]]
                    view.copy_(torch.where((c != 0).any(dim=-1, keepdim=True), c, view))
                base_out[OY:OY + ch, OX:OX + cw] = center
            return base_out

        def fused(mode, ramp=RAMP):
            status.zero_()
            return resident.hip_panorama(center, layers, blend=mode, out=out, status=status, work=work, ramp=ramp)[0]

        for mode in ("mean", "paste", "ramp"):
            # a ramp row: the fused ramp beside the fused mean and the mean chain, its two yardsticks
            forms = [(fused, mode), (chain, mode)] if mode != "ramp" else [(fused, "ramp"), (fused, "mean"), (chain, "mean")]
            for _ in range(a.warmup):
                for fn, m in forms:
                    fn(m)
            torch.cuda.synchronize(dev)
            times = [[] for _ in forms]
            for _ in range(a.reps):
                for (fn, m), t in zip(forms, times):
                    e0, e1 = event_pair()
                    e0.record()
                    fn(m)
                    e1.record()
                    e1.synchronize()
                    t.append(e0.elapsed_time(e1) * 1e-3)
            t_fused, t_chain = times[0], times[-1]
            sha = lambda t: hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()      # noqa: E731
            if mode == "ramp":      # `out` holds the fused mean, the form that ran last into it
                sha_c = sha(out)
                sha_f = sha(fused("ramp", 1))
                sha_ramp = sha(fused("ramp"))
            else:
                sha_f, sha_c = sha(out), sha(base_out)
            nbytes = 3.0 * (sum(l.img.shape[0] * l.img.shape[1] for l in layers) + ch * cw + Hc * W)
            med_f, med_c = float(np.median(t_fused)), float(np.median(t_chain))
            frac = nbytes / PEAK_BYTES_PER_SECOND / med_f
            line = {"row": f"{name}: {w}x{h}, mesh {mesh}, K = {K}, {mode}", "canvas_w": W, "canvas_h": Hc, "off_x": OX, "off_y": OY,
                    "reps": a.reps, "warmup": a.warmup, "fused_seconds_median": med_f, "fused_seconds_min": float(min(t_fused)),
                    "chain_seconds_median": med_c, "chain_seconds_min": float(min(t_chain)), "ratio_chain_over_fused": med_c / med_f,
                    "algorithmic_bytes": nbytes, "fused_fraction_of_8TBps": frac, "fused_fraction_over_k_warp_fast_blend": frac / K3_FRACTION,
                    "status": status.tolist(), "sha256_fused": sha_f, "sha256_equal": sha_f == sha_c}
            if mode == "ramp":
                med_m = float(np.median(times[1]))
                line.update({"row": f"{name}: {w}x{h}, mesh {mesh}, K = {K}, ramp {RAMP}", "mean_seconds_median": med_m,
                             "mean_seconds_min": float(min(times[1])), "ratio_ramp_over_mean": med_f / med_m,
                             "sha256_fused": sha_ramp, "sha256_ramp_1": sha_f, "sha256_equal": sha_f == sha_c})
            lines.append(line)
            if sha_f != sha_c:
                failed.append(f"{line['row']}: " + ("ramp width 1 and the mean differ" if mode == "ramp" else "the panorama and the chain differ"))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        for line in lines:
            print(json.dumps(line))
            f.write(json.dumps(line) + "\n")
    if failed:
        raise SystemExit("panorama_rate: " + "; ".join(failed))


if __name__ == "__main__":
    main()
