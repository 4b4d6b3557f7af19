"""Every form of K1 at its tiling edges, bit for bit.

The solve has four K1 kernels (VALU, MFMA 16x16x4, MFMA 4x4x4 with 16 or 32 cells per wave) and the fused small-mesh launch,
in 30-sum and 24-sum forms, the latter with a float64 or a float32 weight chain.  They share their staging, weight chain, MFMA
step and result layouts; this file pins the float32 grid of each form at the shapes where those shared
steps turn a corner: partial and exactly full 16-cell groups and 64-cell tiles, the 4x2 form's overhanging second tile,
keypoint counts just below, at and just above one and two 64-keypoint chunks, last chunks and last splits of 1, 2 and 3
keypoints, many chunks on one cell.

(a) the SHA-256 of every grid equals tests/golden/k1_forms_edges_sha.npz (recorded on an MI355X by
    tests/golden/make_k1_forms_edges_golden.py, before the shared steps were given one definition each);
(b) the 30-sum forms stay within RMSE_BAR of the oracle's loop on the first 64 cells;
(c) every grid is finite.
"""
import ctypes
import hashlib

import numpy as np
import pytest

from oracle import apap_oracle as O
from cvx_proj_amd.synth import synth_pair

pytestmark = pytest.mark.gpu

RMSE_BAR = 1e-4          # px, north_star (tests/test_gpu_parity.py)
GAMMA, SIGMA = 0.5, 40.0

# (cells, n, batch)
SHAPES = [(1, 5, 1), (15, 63, 1), (16, 64, 1), (17, 65, 3), (63, 62, 1), (64, 128, 1), (65, 130, 1), (127, 67, 1),
          (128, 200, 2), (129, 257, 1), (257, 192, 1), (1, 1000, 1)]

# name -> context options; variant 1..4 = VALU, MFMA, MFMA4, MFMA4X2; eigen 1 = Jacobi, 2 = inverse iteration
FORMS = {
    "auto": {},
    "auto-nofuse": {"fused_max_cells": 0},
    "valu-invit": {"variant": 1, "eigen": 2},
    "mfma-invit": {"variant": 2, "eigen": 2},
    "mfma4-invit": {"variant": 3, "eigen": 2},
    "mfma4x2-invit": {"variant": 4, "eigen": 2},
    "mfma-jacobi": {"variant": 2, "eigen": 1},
}
FORMS.update({f"{name}-m24-{'f32' if w else 'f64'}": {"variant": v, "moments": 24, "weights_f32": w}
              for v, name in ((2, "mfma"), (3, "mfma4"), (4, "mfma4x2")) for w in (0, 1)})


def key(cells, n, batch, form):
    return f"{cells}_{n}_{batch}_{form}"


def solve_forms(native, cells, n, batch):
    """The inputs of test_fused_small_mesh_launch_around_its_limits, solved by every form on the same device buffers.
    Returns ({form: (batch, cells, 9) float32}, keypoints per pair, vertices)."""
    import torch
    rng = np.random.default_rng(cells * 7 + n)
    dev = torch.device("cuda:0")
    tabs, dens, srcs, dsts = {24: [], 30: []}, [], [], []
    for b in range(batch):
        p = synth_pair(640, 480, n, 4, seed=900 + b + n)
        q = native.host_prepare(p.src, p.dst)
        for m in (24, 30):
            tabs[m].append(native.host_build_table(p.src, q["cf1"], q["cf2"], moments=m))
        dens.append(native.host_build_denorm(q["iC2"], q["C1"], q["iN2"], q["N1"]))
        srcs.append(p.src)
        dsts.append(p.dst)
    verts = rng.random((cells, 2)) * [640, 480]
    d_tab = {m: torch.from_numpy(np.stack(t)).to(dev) for m, t in tabs.items()}
    d_den = torch.from_numpy(np.stack(dens)).to(dev)
    d_vert = torch.from_numpy(verts).to(dev)
    out = {}
    for form, options in FORMS.items():
        ctx = native.Context(**options)
        H = torch.empty((batch, cells, 9), dtype=torch.float32, device=dev)
        nbytes = max(native.lib().apap_solve_batch_workspace_bytes(native._h(ctx), n, cells, batch), 256)
        work = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        native.check(native.lib().apap_solve_batch_device(native._h(ctx), d_tab[options.get("moments", 30)].data_ptr(), n,
                                                          d_vert.data_ptr(), 0, cells, GAMMA, SIGMA, d_den.data_ptr(),
                                                          H.data_ptr(), batch, work.data_ptr(), nbytes, ctypes.c_void_p(0)))
        torch.cuda.synchronize()
        out[form] = H.cpu().numpy()
        ctx.close()
    return out, srcs, dsts, verts


def sha(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), dtype=np.uint8)


@pytest.mark.parametrize("cells,n,batch", SHAPES)
def test_every_k1_form_at_the_tiling_edges(native, golden, cells, n, batch):
    assert native.lib().apap_device_count() >= 1, "these tests need a GPU; the library found none"
    g = golden("k1_forms_edges_sha")
    out, srcs, dsts, verts = solve_forms(native, cells, n, batch)
    refs = [O.local_homography_loop(srcs[b], dsts[b], verts[None, :64], GAMMA, SIGMA, want_weights=False)[0] for b in range(batch)]
    wrong = []
    for form, H in out.items():
        if not np.isfinite(H).all():                                        # (c)
            wrong.append(f"{form}: {int((~np.isfinite(H)).sum())} values are not finite")
        if not np.array_equal(sha(H), g[key(cells, n, batch, form)]):       # (a)
            wrong.append(f"{form}: the grid's SHA-256 differs from the recorded one")
        if "moments" not in FORMS[form]:                                    # (b)
            d = max(O.reprojection_rmse_delta(H[b, :64].reshape(1, -1, 3, 3), refs[b], srcs[b]).max() for b in range(batch))
            print(f"cells={cells} n={n} batch={batch} {form}: rmse-delta max {d:.3e} px")
            if not d < RMSE_BAR:
                wrong.append(f"{form}: rmse delta {d:.3e} px against the oracle's loop")
    assert not wrong, "; ".join(wrong)
