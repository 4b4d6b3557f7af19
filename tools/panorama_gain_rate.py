#!/usr/bin/env python3
"""Time the panorama's gain compensation on the GPU, at the 4K five-view shape of tools/panorama_rate.py (a 3840 x 2160
centre, four neighbours, meshes of 200 x 200), resident data, every form in ONE alternation: call by call in one process,
every timed call between two events on its stream, median and minimum of --reps calls after --warmup.

    python tools/panorama_gain_rate.py [--reps 20] [--warmup 3] [--baseline-lib libapap_hip_parent.so]
                                       [--out profiles/panorama_gain_rate.jsonl]

Rows, one JSON line each, printed and APPENDED to --out:
  (a) plain <blend>     the ungained mean / paste / ramp 64 - and, with --baseline-lib (a build of the parent commit's
                        library), the same call through that library in the same alternation, twice, so that the spread of
                        two runs of the parent stands beside the difference
  (b) gained <blend>    the same blends under seeded gains (apap_panorama_gain_device)
  (c) stats step s      the statistics pass at steps 1, 4 and 8
  (d) auto / torch      resident.hip_panorama(blend="mean", gain="auto", gain_step=4) beside the same chain in torch
                        operations: four hip_warp_batch canvases placed on the union canvas, the overlap counts and sums on
                        the step-4 lattice, a float64 solve, the scaled views and their mean
A round runs every form once in this order; round r starts at form r, and one untimed plain call follows the torch chain.
No time is a pass condition.  The tool fails without a GPU, when a gained canvas under q = 4096 differs from the plain one, and
when the torch chain's statistics differ from the kernel's."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--baseline-lib", default=None, help="a build of the parent commit's library for the rows (a)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "panorama_gain_rate.jsonl"))
    a = ap.parse_args()
    if a.reps < 10 or a.warmup < 3:
        raise SystemExit("panorama_gain_rate: at least 10 timed calls after 3 warm-ups")
    import torch      # before the library: one HIP runtime per process
    from cvx_proj_amd import _native, resident
    from panorama_rate import build_case
    if _native.lib().apap_device_count() < 1 or not torch.cuda.is_available():
        raise SystemExit("panorama_gain_rate: no HIP device (this tool measures the GPU; it has no CPU mode)")
    dev = torch.device("cuda", 0)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)      # noqa: E731
    this_lib = _native.lib()
    parent = None
    if a.baseline_lib:
        parent = ctypes.CDLL(os.path.abspath(a.baseline_lib))
        for sym in ("apap_panorama_device", "apap_panorama_ramp_device", "apap_panorama_workspace_bytes", "apap_panorama_bounds"):
            getattr(parent, sym).restype, getattr(parent, sym).argtypes = _native.SIGNATURES[sym]

    w, h, mesh = 3840, 2160, 200
    center_h, layers_h = build_case(w, h, mesh, 2160)
    center = up(center_h)
    layers = [_native.PanoramaLayer(up(img), up(H), (up(e[0]), up(e[1])), size, off) for img, H, e, size, off in layers_h]
    K = len(layers)
    geo = np.array([list(l.final_size) + list(l.offset) for l in layers], dtype=np.int32)
    W, Hc, OX, OY = _native.panorama_bounds(center.shape, geo[:, 0], geo[:, 1], geo[:, 2], geo[:, 3])
    out = torch.empty((Hc, W, 3), dtype=torch.uint8, device=dev)
    work = torch.empty(resident.panorama_workspace_bytes(layers), dtype=torch.uint8, device=dev)
    status = torch.zeros(K, dtype=torch.int32, device=dev)
    tab_n = torch.empty((K + 1, K + 1), dtype=torch.int64, device=dev)
    tab_s = torch.empty((K + 1, K + 1), dtype=torch.int64, device=dev)
    q_seeded = np.random.default_rng(7).integers(3000, 5500, K + 1).tolist()
    ch, cw = center.shape[:2]

    def plain(lib, blend, ramp):
        _native._lib = lib      # the resident wrapper calls through whatever library the binding holds
        try:
            status.zero_()
            return resident.hip_panorama(center, layers, blend=blend, out=out, status=status, work=work, ramp=ramp)[0]
        finally:
            _native._lib = this_lib

    def gained(blend, ramp, q):
        status.zero_()
        return resident.hip_panorama(center, layers, blend=blend, out=out, status=status, work=work, ramp=ramp, gain=q)[0]

    def stats(step):
        status.zero_()
        return resident.hip_panorama_gain_stats(center, layers, step=step, N=tab_n, S=tab_s, status=status, work=work)

    auto_gains = []

    def auto():
        status.zero_()
        r = resident.hip_panorama(center, layers, blend="mean", out=out, status=status, work=work, gain="auto", gain_step=4,
                                  return_gains=True)
        auto_gains[:] = [r[3]]
        return r[0]

    # the chain in torch: per layer its own canvas, then everything on the union canvas
    pair_out = [torch.empty((1, l.final_size[1], l.final_size[0], 3), dtype=torch.uint8, device=dev) for l in layers]
    pair_work = [torch.empty(resident.warp_workspace_bytes(l.local_homography.shape[:2], *l.final_size), dtype=torch.uint8, device=dev)
                 for l in layers]
    pair_status = [torch.zeros(1, dtype=torch.int32, device=dev) for _ in layers]
    stack = torch.empty((K + 1, Hc, W, 3), dtype=torch.uint8, device=dev)
    chain_out = torch.empty((Hc, W, 3), dtype=torch.uint8, device=dev)
    chain_tables = []

    def torch_chain():
        stack.zero_()
        stack[0, OY:OY + ch, OX:OX + cw] = center
        for k, (l, o, wk, st) in enumerate(zip(layers, pair_out, pair_work, pair_status)):
            rows, cols = l.local_homography.shape[:2]
            resident.hip_warp_batch(l.img, l.local_homography.view(1, rows * cols, 9), l.mesh[0], l.mesh[1], l.final_size[0],
                                    l.final_size[1], l.offset[0], l.offset[1], (rows, cols), out=o, work=wk, status=st)
            y0, x0 = OY - l.offset[1], OX - l.offset[0]
            stack[k + 1, y0:y0 + o.shape[1], x0:x0 + o.shape[2]] = o[0]
        lattice = stack[:, ::4, ::4]
        present = (lattice != 0).any(dim=-1).reshape(K + 1, -1).to(torch.float64)
        inten = lattice.sum(dim=-1, dtype=torch.int64).reshape(K + 1, -1).to(torch.float64)
        N = present @ present.T                  # exact: counts and sums stay far below 2^53
        S = (inten * present) @ present.T
        m = S / (3.0 * N.clamp(min=1.0))
        off = ~torch.eye(K + 1, dtype=torch.bool, device=dev)
        Noff = N * off
        A = -2.0 * Noff * m * m.T / 100.0
        A = A + torch.diag((Noff * (2.0 * m * m / 100.0 + 100.0)).sum(dim=1))
        g = torch.linalg.solve(A, (Noff * 100.0).sum(dim=1))
        q = torch.clamp(torch.round(4096.0 * g), 1024, 16383).to(torch.int32)
        gained_views = torch.clamp((stack.to(torch.int32) * q.view(-1, 1, 1, 1) + 2048) >> 12, max=255)
        count = (stack != 0).any(dim=-1).sum(dim=0).clamp(min=1)
        chain_out.copy_(torch.div(gained_views.sum(dim=0), count[..., None], rounding_mode="floor"))
        chain_tables[:] = [N, S, q]
        return chain_out

    forms = []
    for blend, ramp in BLENDS:
        # this library between the parent's two runs: it and the parent's second run both follow a call of the same blend
        if parent is not None:
            forms.append((f"plain {blend}, parent library", "a", lambda b=blend, r=ramp: plain(parent, b, r)))
        forms.append((f"plain {blend}", "a", lambda b=blend, r=ramp: plain(this_lib, b, r)))
        if parent is not None:
            forms.append((f"plain {blend}, parent library again", "a", lambda b=blend, r=ramp: plain(parent, b, r)))
    for blend, ramp in BLENDS:
        forms.append((f"gained {blend}", "b", lambda b=blend, r=ramp: gained(b, r, q_seeded)))
    for step in (1, 4, 8):
        forms.append((f"stats step {step}", "c", lambda s=step: stats(s)))
    forms.append(("auto mean, step 4", "d", auto))
    forms.append(("torch chain mean, step 4", "d", torch_chain))

    failed = []
    for blend, ramp in BLENDS:      # the checks, outside the clock
        want = plain(this_lib, blend, ramp).clone()
        if not torch.equal(gained(blend, ramp, [4096] * (K + 1)), want):
            failed.append(f"{blend}: q = 4096 differs from the plain canvas")
        if parent is not None and not torch.equal(plain(parent, blend, ramp), want):
            failed.append(f"{blend}: the parent library's canvas differs")
    auto_canvas = auto().clone()
    torch_chain()
    g = auto_gains[0]
    if not (torch.equal(chain_tables[0].to(torch.int64), g.N) and torch.equal(chain_tables[1].to(torch.int64), g.S)):
        failed.append("the torch chain's statistics differ from the kernel's")
    chain_equal = bool(torch.equal(chain_out, auto_canvas)) and bool(torch.equal(chain_tables[2], g.q))

    for _ in range(a.warmup):
        for _, _, fn in forms:
            fn()
    torch.cuda.synchronize(dev)
    times = [[] for _ in forms]
    for r in range(a.reps):
        # Round r starts at form r, so that no form always follows the same neighbour.  The torch chain takes half a second and
        # gigabytes of temporaries: one untimed plain call separates it from the form after it, which otherwise pays for the
        # chain's wake (measured: 572 us where its neighbours take 260).
        for i in range(len(forms)):
            (name, _, fn), t = forms[(r + i) % len(forms)], times[(r + i) % len(forms)]
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            t.append(e0.elapsed_time(e1) * 1e-3)
            if name.startswith("torch chain"):
                plain(this_lib, "mean", 1)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        for (name, group, _), t in zip(forms, times):
            line = {"row": f"C3: {w}x{h}, mesh {mesh}, K = {K}, {name}", "group": group, "canvas_w": W, "canvas_h": Hc, "reps": a.reps,
                    "warmup": a.warmup, "seconds_median": float(np.median(t)), "seconds_min": float(min(t)), "seconds_max": float(max(t))}
            if name.startswith("torch chain"):
                line["canvas_and_q_equal_auto"] = chain_equal
            if name.startswith("auto"):
                line["q"] = g.q.tolist()
            print(json.dumps(line))
            f.write(json.dumps(line) + "\n")
    if failed:
        raise SystemExit("panorama_gain_rate: " + "; ".join(failed))


if __name__ == "__main__":
    main()
