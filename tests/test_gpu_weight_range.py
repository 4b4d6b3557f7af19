"""K1's squared weights where they leave their format's range (oracle/weight_spec.py restates both chains).

A tight keypoint cluster sits at controlled distances from the mesh's vertices, so that the nearest keypoint's d / sigma^2 lands
on both sides of each edge: the float32 edge (x = -126, d / sigma^2 = 43.7: v_exp_f32 flushes what would be subnormal to 0;
41-43.4 put the cluster across it, 50-52.5 past it), float64 w^2 under K2's trace floor (~320), subnormal (354.2) and zero
(372.6).  gamma runs from 0 through values whose gamma^2 leaves the float32
(1e-25) or float64 (1e-170) range at the bottom, the control 0.5, and values whose gamma^2 overflows float32 (1e20) or float64
(1e155).  Every form of tests/test_gpu_parity.py's `variant` list, the two-launch path on these small meshes, a batched solve and
the 24-sum forms with float64 and float32 weights are compared with the reference; where the reference's own float64 SVD is
unreliable (cond_out * eps), with its 60-digit answer instead.

Bars: the default forms as tests/test_gpu_parity.py's edge cases (finite exactly where the reference is, RMSE_BAR, the same
weight tensor).  The 24-sum forms: weight_spec.bar = BAR_C (eps_cell + 2^-53) cond scale + FLOOR_ULPS 2^-24 scale px,
eps_cell being the spec's bound on the relative perturbation of the normal matrix by the weights the engine solves with (0 on
the careful path), cond = trace(M) / (lambda_8 - lambda_9), scale the size of the projected coordinates; both constants are
calibrated on the CPU (tests/test_weight_spec.py).  Against the library before the float32-weight routing, the float32-weight
forms fail this bar where the cluster lies across x = -126 (sigma = 3, nearest d / sigma^2 = 41 and 42, gamma 0, 1e-25 and
1e-170: part of the weights flushed, trace ~1e-38, solved as it stood; 0.04-0.07 px against a bar of 8e-5 px in the spec's
emulation).  Cells with EVERY w^2 flushed have trace 0 and took the careful path before the fix as well."""
import functools

import numpy as np
import pytest

from oracle import apap_oracle as O
from oracle import weight_spec as S
from cvx_proj_amd.synth import synth_pair

pytestmark = pytest.mark.gpu
RMSE_BAR = 1e-4
GAMMAS = [0.0, 1e-25, 1e-170, 0.5, 1e20, 1e155]
SIGMAS = [1.0, 3.0, 10.0]
# nearest keypoint's d / sigma^2: controls, the float32 edges (43.7, 52.0; 41-43.4 put the cluster ACROSS x = -126), the float64
# ones (~320, 354.2, 372.6)
TARGETS = [0.3, 5.0, 20.0, 40.0, 41.0, 42.0, 42.5, 43.0, 43.4, 44.2, 50.0, 51.5, 52.5, 60.0, 300.0, 318.0, 330.0, 353.5, 355.0,
           372.0, 373.5]
UNRELIABLE = RMSE_BAR / 10       # px: where cond_out * eps * scale passes this, the 60-digit answer is the yardstick


@pytest.fixture(scope="module", autouse=True)
def need_gpu(native):
    assert native.lib().apap_device_count() >= 1, "these tests need a GPU; the library found none"


DEFAULT_FORMS = [dict(variant=0, eigen=0), dict(variant=0, eigen=1), dict(variant=1, eigen=1), dict(variant=1, eigen=2),
                 dict(variant=2, eigen=1), dict(variant=2, eigen=2), dict(variant=3, eigen=2), dict(variant=4, eigen=2),
                 dict(variant=0, eigen=0, fused_max_cells=0)]
DEFAULT_IDS = ["auto", "auto-jacobi", "valu-jacobi", "valu-invit", "mfma-jacobi", "mfma-invit", "mfma4-invit", "mfma4x2-invit",
               "auto-two-launch"]
M24_FORMS = [dict(variant=v, moments=24, weights_f32=w) for v in (2, 3, 4) for w in (0, 1)]
M24_IDS = [f"{n}-m24-w{'32' if w else '64'}" for n in ("mfma", "mfma4", "mfma4x2") for w in (0, 1)]


@functools.lru_cache(maxsize=None)
def case(sigma, seed=0):
    """48 keypoints in a 24-px box around (320, 240), dst a mild homography of them plus noise; one vertex per target, placed
    along its own direction so that its NEAREST keypoint is at target * sigma^2."""
    rng = np.random.default_rng(1000 + int(sigma * 10) + seed)
    centre = np.array([320.0, 240.0])
    src = (centre + rng.uniform(-12.0, 12.0, (48, 2))).astype(np.float32)
    Ht = np.array([[1.02, 0.01, 5.0], [-0.01, 0.99, -3.0], [1e-5, 2e-5, 1.0]])
    dst = (O.project(Ht[None], src)[0] + rng.normal(0.0, 0.3, src.shape)).astype(np.float32)
    s = src.astype(np.float64)
    verts = []
    for j, q in enumerate(TARGETS):
        e = np.array([np.cos(0.7 + 2.4 * j), np.sin(0.7 + 2.4 * j)])
        want = q * sigma * sigma
        R = want + 12.0
        for _ in range(60):                  # nearest distance along the ray, by fixed-point steps (monotone outside the box)
            R += want - np.hypot(*(centre + R * e - s).T).min()
        verts.append(centre + R * e)
    return src, dst, np.array(verts).reshape(1, -1, 2)


@functools.lru_cache(maxsize=None)
def reference(sigma, gamma, seed=0):
    """The reference's grid and weights, cond_out, and per cell the yardstick (its own answer, or the 60-digit one where its
    SVD is unreliable), the normal-matrix condition and the coordinate scale."""
    src, dst, verts = case(sigma, seed)
    cond = np.zeros(verts.shape[:2])
    with np.errstate(all="ignore"):
        H_ref, W_ref = O.local_homography_loop(src, dst, verts, gamma, sigma, cond_out=cond)
    p = O.prepare(src, dst)
    yard = H_ref.copy()
    ncond = np.zeros(verts.shape[:2])
    scale = np.zeros(verts.shape[:2])
    for j in range(verts.shape[1]):
        if np.isfinite(H_ref[0, j]).all():
            scale[0, j] = max(1.0, float(np.abs(O.project(H_ref[0, j][None].astype(np.float64), src)).max()))
        if not (cond[0, j] * 2.0 ** -53 * max(scale[0, j], 1.0) < UNRELIABLE):
            yard[0, j] = O.local_homography_exact_cell(src, dst, verts[0, j], gamma, sigma)
        w2 = S.w2_exact(verts[0, j], src, gamma, sigma)
        ncond[0, j] = S.normal_cond(S.normal_matrix((w2 / w2.max()).astype(np.float64), p["aa"]))
    return dict(H=H_ref, W=W_ref, cond=cond, yard=yard, ncond=ncond, scale=scale)


def _ctx(native, form):
    return native.Context(**form)


@pytest.mark.parametrize("sigma", SIGMAS)
@pytest.mark.parametrize("gamma", GAMMAS)
@pytest.mark.parametrize("form", DEFAULT_FORMS, ids=DEFAULT_IDS)
def test_default_forms_across_the_weight_range(native, form, gamma, sigma):
    src, dst, verts = case(sigma)
    ref = reference(sigma, gamma)
    ctx = _ctx(native, form)
    try:
        H, W = native.local_homography(src, dst, verts, gamma, sigma, ctx=ctx)
    finally:
        ctx.close()
    fin_ref, fin = np.isfinite(ref["H"]).all(axis=(2, 3)), np.isfinite(H).all(axis=(2, 3))
    assert (fin == fin_ref).all(), f"finite cells: engine {fin.ravel().tolist()}, reference {fin_ref.ravel().tolist()}"
    assert np.allclose(W, ref["W"], rtol=1e-14, atol=1e-300)
    d = O.reprojection_rmse_delta(H[fin][None], ref["yard"][fin][None], src)[0]
    worst = int(np.argmax(d))
    print(f"gamma={gamma:g} sigma={sigma:g}: max delta {d.max():.2e} px at d/sigma^2 = {TARGETS[worst]}")
    bad = [(TARGETS[j], float(d[j])) for j in range(d.size) if not d[j] < RMSE_BAR]
    assert not bad, f"cells over {RMSE_BAR} px (nearest d/sigma^2, delta): {bad}"


def _m24_bar(ref, src, verts, gamma, sigma, w32):
    """Per cell, the 24-sum forms' bar in px and the spec's region (for the message)."""
    bars, regions = [], []
    for j in range(verts.shape[1]):
        r = S.cell(verts[0, j], src, gamma, sigma, "f32" if w32 else "f64", aa=_aa(sigma))
        bars.append(S.bar(r["eps_cell"], ref["ncond"][0, j], ref["scale"][0, j]))
        regions.append(r["cell_region"])
    return np.array(bars), regions


@functools.lru_cache(maxsize=None)
def _aa(sigma):
    src, dst, _ = case(sigma)
    return O.prepare(src, dst)["aa"]


@pytest.mark.parametrize("sigma", SIGMAS)
@pytest.mark.parametrize("gamma", GAMMAS)
@pytest.mark.parametrize("form", M24_FORMS, ids=M24_IDS)
def test_24_sum_forms_across_the_weight_range(native, form, gamma, sigma):
    src, dst, verts = case(sigma)
    ref = reference(sigma, gamma)
    ctx = _ctx(native, form)
    try:
        H, _ = native.local_homography(src, dst, verts, gamma, sigma, want_weights=False, ctx=ctx)
    finally:
        ctx.close()
    fin_ref, fin = np.isfinite(ref["H"]).all(axis=(2, 3)), np.isfinite(H).all(axis=(2, 3))
    assert (fin == fin_ref).all(), f"finite cells: engine {fin.ravel().tolist()}, reference {fin_ref.ravel().tolist()}"
    bars, regions = _m24_bar(ref, src, verts, gamma, sigma, form["weights_f32"] == 1)
    d = O.reprojection_rmse_delta(H[fin][None], ref["yard"][fin][None], src)[0]
    bars = bars[fin.ravel()]
    print(f"gamma={gamma:g} sigma={sigma:g}: max delta {d.max():.2e} px, max delta / bar {np.max(d / bars):.2e}")
    bad = [(TARGETS[j], regions[j], float(d[j]), float(bars[j])) for j in range(d.size) if not d[j] <= bars[j]]
    assert not bad, f"cells over the bar (nearest d/sigma^2, spec region, delta px, bar px): {bad}"


@pytest.mark.parametrize("gamma", [0.0, 1e-170, 1e155])
def test_batched_solve_across_the_weight_range(native, gamma):
    """hip_solve_batch (blockIdx.z = pair) on two pairs of the sigma = 3 case: each within the bar of the reference and the
    bits of its own single solve."""
    import torch
    from cvx_proj_amd.dist import hip_solve, hip_solve_batch
    dev = torch.device("cuda:0")
    sigma = 3.0
    tabs, dens, cases = [], [], []
    for seed in (0, 1):
        src, dst, verts = case(sigma, seed)
        q = native.host_prepare(src, dst)
        tabs.append(torch.from_numpy(native.host_build_table(src, q["cf1"], q["cf2"])))
        dens.append(torch.from_numpy(native.host_build_denorm(q["iC2"], q["C1"], q["iN2"], q["N1"])))
        cases.append((src, dst, verts))
    # each seed has its own cluster; the batch shares pair 0's mesh
    vert = torch.from_numpy(np.ascontiguousarray(cases[0][2].reshape(-1, 2))).to(dev)
    tables, denorms = torch.stack(tabs).to(dev), torch.stack(dens).to(dev)
    Hb = hip_solve_batch(tables, denorms, vert, gamma, sigma)
    torch.cuda.synchronize()
    for k, (src, dst, _) in enumerate(cases):
        Hk = hip_solve(tables[k].contiguous(), denorms[k].contiguous(), vert, gamma, sigma)
        assert torch.equal(Hb[k], Hk), k
        verts0 = cases[0][2]
        with np.errstate(all="ignore"):
            H_ref, _ = O.local_homography_loop(src, dst, verts0, gamma, sigma, want_weights=False)
        H = Hb[k].cpu().numpy().reshape(H_ref.shape)
        fin_ref, fin = np.isfinite(H_ref).all(axis=(2, 3)), np.isfinite(H).all(axis=(2, 3))
        assert (fin == fin_ref).all()
        cond = np.zeros(verts0.shape[:2])
        with np.errstate(all="ignore"):
            O.local_homography_loop(src, dst, verts0, gamma, sigma, want_weights=False, cond_out=cond)
        for j in np.flatnonzero(fin.ravel()):
            yard = H_ref[0, j]
            if not cond[0, j] * 2.0 ** -53 * 1e3 < UNRELIABLE:
                yard = O.local_homography_exact_cell(src, dst, verts0[0, j], gamma, sigma)
            d = O.reprojection_rmse_delta(H[0, j][None, None], yard[None, None], src).max()
            assert d < RMSE_BAR, (k, TARGETS[j], d)


# ------------------------------------------------------------------------------------------- ragged shapes, 24-sum forms
RAGGED_MESH = {1: (1, 1), 15: (3, 5), 17: (1, 17), 31: (1, 31), 33: (3, 11), 1025: (25, 41)}


@functools.lru_cache(maxsize=None)
def ragged_case(cells, n):
    rows, cols = RAGGED_MESH[cells]
    rng = np.random.default_rng(cells * 10007 + n)
    p = synth_pair(640, 480, n, 4, seed=n)
    xs = np.linspace(0, p.final_w, cols) + 3.0
    ys = np.linspace(0, p.final_h, rows) + 2.0
    verts = np.stack(np.meshgrid(xs, ys), axis=-1) + rng.normal(0, 1, (rows, cols, 2))
    H_ref, _ = O.local_homography_loop(p.src, p.dst, verts, 0.5, 100.0, want_weights=False)
    return p.src, p.dst, verts, H_ref


@pytest.mark.parametrize("n", [5, 9, 65, 1023, 4097])
@pytest.mark.parametrize("cells", sorted(RAGGED_MESH))
@pytest.mark.parametrize("form", M24_FORMS, ids=M24_IDS)
def test_24_sum_forms_on_ragged_shapes(native, form, cells, n):
    """The cell and keypoint tails of the 24-sum kernels (cell counts off the 16- and 64-cell tiles, keypoint counts off the
    4-keypoint step and the 64-keypoint chunk) at BASELINE's gamma = 0.5, sigma = 100: the one-ulp class of
    tests/test_gpu_moments24.py where it is defined - n >= 65 keypoints and a grid of more than one cell (its fraction bar is
    < 1 entry of a single cell's 9).  With 10 or 18 DLT rows (n = 5, 9) the systems are ill-conditioned enough that the sums'
    rounding moves H by up to ~15 ulp (measured; RMSE delta 5e-5 px): there, and on single cells, every cell is held to
    the conditioning bar of oracle/weight_spec.py and to RMSE_BAR instead."""
    from test_gpu_moments24 import check
    src, dst, verts, H_ref = ragged_case(cells, n)
    ctx = _ctx(native, form)
    try:
        H, _ = native.local_homography(src, dst, verts, 0.5, 100.0, want_weights=False, ctx=ctx)
    finally:
        ctx.close()
    if n >= 65 and cells > 1:
        check(f"{cells} cells n={n}", H, H_ref, src[:128])
        return
    assert np.isfinite(H).all()
    aa = O.prepare(src, dst)["aa"]
    chain = "f32" if form["weights_f32"] else "f64"
    d = O.reprojection_rmse_delta(H, H_ref, src)
    print(f"[{cells} cells n={n}] rmse-delta max {d.max():.3e} px")
    assert d.max() < RMSE_BAR
    for (i, j), dij in np.ndenumerate(d):
        r = S.cell(verts[i, j], src, 0.5, 100.0, chain, aa=aa)
        scale = max(1.0, float(np.abs(O.project(H_ref[i, j][None].astype(np.float64), src)).max()))
        bar = S.bar(r["eps_cell"], S.normal_cond(S.normal_matrix((r["exact"] / r["exact"].max()).astype(np.float64), aa)), scale)
        assert dij <= bar, (i, j, dij, bar)
