"""CPU checks of oracle/weight_spec.py, the restatement of K1's two w^2 chains and K2's route to the careful path: where each
chain's w^2 turns subnormal and zero, where gamma^2 leaves a chain's range, that the float64 chain is exp(-2 d / sigma^2) to a
few ulp over its normal range, that every cell the engine keeps on float32 weights is inside the bound include/apap_hip.h
states, and the calibration of the reprojection bar tests/test_gpu_weight_range.py holds the 24-sum forms to."""
import os
import re

import numpy as np
import pytest

from oracle import apap_oracle as O
from oracle import weight_spec as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LN2 = np.log(2.0)


def _at(q, sigma=1.0, gamma=0.0, chain="f32", vx=0.0):
    """w^2 of one keypoint at the origin seen from a vertex at d / sigma^2 = q (along x, from vx on)."""
    r = S.cell((vx + q * sigma * sigma, 0.0), np.array([[vx, 0.0]]), gamma, sigma, chain)
    return r["w2"][0], r["region"][0]


def test_the_exp_table_is_the_kernels():
    with open(os.path.join(ROOT, "cvx_proj_amd", "csrc", "apap_kernels.hip")) as f:
        src = f.read()
    body = src[src.index("kExp2Tab[kExpN] = {"):]
    body = body[:body.index("};")]
    tab = np.array([float.fromhex(v) for v in re.findall(r"0x[0-9a-f.]+p[+-]\d+", body)])
    assert np.array_equal(tab, S.EXP2_TAB)
    for name, value in (("kTraceFloorW32", "0x1p-40"), ("kGammaCutF64", "0x1p128"), ("kTraceFloorF64", "1e-280")):
        assert re.search(rf"constexpr double {name} = {re.escape(value)};", src), name
    assert float.fromhex("0x1p-40") == S.TRACE_FLOOR_W32 and float.fromhex("0x1p128") == S.GAMMA_CUT_F64


def test_float32_band_edge():
    """x = -2 log2(e) q: below x = -126 the correctly rounded 2^x would be subnormal (0 below x = -150); v_exp_f32 flushes
    it to 0, so the float32 chain has ONE edge, normal -> zero, at q = 43.67."""
    edge = 126 / (2 * S.LOG2E)
    for sigma in (1.0, 3.0, 10.0):
        w_lo, r_lo = _at(edge * (1 - 1e-4), sigma)
        w_hi, r_hi = _at(edge * (1 + 1e-4), sigma)
        assert (r_lo, r_hi) == ("normal", "zero") and w_lo >= S.F32_NORMAL_MIN and w_hi == 0.0, sigma
    assert _at(149.5 / (2 * S.LOG2E))[0] == 0.0


@pytest.mark.parametrize("edge,below,above", [
    (1022 * LN2 / 2, "normal", "subnormal"),       # 354.2
    (1075 * LN2 / 2, "subnormal", "zero"),         # 372.6
])
def test_float64_band_edges(edge, below, above):
    for sigma in (1.0, 3.0, 10.0):
        _, r_lo = _at(edge * (1 - 1e-5), sigma, chain="f64")
        _, r_hi = _at(edge * (1 + 1e-5), sigma, chain="f64")
        assert (r_lo, r_hi) == (below, above), sigma


def test_gamma_squared_edges():
    f32 = lambda g: float(np.float32(S.k1_gamma2(g, "f32")))       # noqa: E731  what K1's float32 chain clamps at
    f64 = lambda g: S.k1_gamma2(g, "f64")                          # noqa: E731
    # float32: gamma^2 subnormal below gamma = 2^-63 (1.1e-19), zero below ~2^-75; overflow above 2^64 (1.8e19) - never
    # reached: from gamma = 1 on the chain clamps at 1 (every weight is gamma there)
    assert f32(2.0 ** -63 * 1.001) >= S.F32_NORMAL_MIN > f32(2.0 ** -63 * 0.999) > 0.0
    assert f32(1e-25) == 0.0
    assert f32(0.999) == np.float32(0.999 ** 2) and f32(1.0) == 1.0 and f32(1e20) == 1.0 and f32(1e155) == 1.0
    # float64: subnormal below 2^-511 (1.5e-154), zero below ~1e-162; the cut at 2^128 keeps every gamma^2 and the sums finite
    assert f64(2.0 ** -511 * 1.001) >= S.F64_NORMAL_MIN > f64(2.0 ** -511 * 0.999) > 0.0
    assert f64(1e-170) == 0.0
    assert f64(2.0 ** 128 * 0.999) == (2.0 ** 128 * 0.999) ** 2 and f64(2.0 ** 128) == 1.0 and f64(1e155) == 1.0
    # below the cut the value is gamma * gamma as ever: the default grids keep their bits
    for g in (0.0, 1e-170, 1e-25, 0.5, 3.0, 1e20, 1e38):
        assert f64(g) == (g * g if g > 0 else 0.0)
    # the clamp decides where exp falls under it: gamma = 1e-25 on the float32 chain clamps at 0 (the clamp is lost),
    # on the float64 one at 1e-50
    assert _at(60.0, gamma=1e-25)[0] == 0.0 and _at(60.0, gamma=1e-25, chain="f64")[0] == 1e-25 * 1e-25


def test_float64_chain_is_exp_over_its_normal_range():
    rng = np.random.default_rng(3)
    src = np.column_stack([rng.uniform(-4000, 4000, 4000), rng.uniform(-3000, 3000, 4000)])
    for sigma in (1.0, 3.0, 10.0, 100.0):
        for q_max in (1.0, 40.0, 354.0):
            v = np.array([0.5, -0.25])
            s = v + (src / np.abs(src).max()) * q_max * sigma * sigma
            r = S.cell(v, s, 0.0, sigma, "f64")
            w = r["w2"]
            ex = r["exact"].astype(np.float64)
            normal = ex >= S.F64_NORMAL_MIN
            d = np.hypot(*(v - s).T)
            rel = np.abs(w[normal] - ex[normal]) / ex[normal]
            assert (rel <= S.rel_bound_f64(2 * d[normal] / sigma ** 2)).all(), (sigma, q_max, rel.max())
            assert rel.max() < 4e-13


def test_k2_routing():
    """trace below the floor / not finite, n < 5, a small eigen-gap: the careful path; the float32 chain's floor is 2^-40."""
    rng = np.random.default_rng(9)
    src = (rng.random((30, 2)) * [640, 480]).astype(np.float32)
    dst = (src * 1.01 + rng.normal(0, 1, src.shape) + [4, -2]).astype(np.float32)
    aa = O.prepare(src, dst)["aa"]
    M = S.normal_matrix(np.ones(30), aa)
    assert not S.route(M, 30, "f64")["careful"] and not S.route(M, 30, "f32")["careful"]
    assert S.route(M, 4, "f64")["careful"]
    for scale, f64, f32 in ((1e-10, False, False), (1e-17, False, True), (1e-295, True, True), (np.inf, True, True)):
        with np.errstate(invalid="ignore"):
            Ms = M * scale
        assert S.route(Ms, 30, "f64")["careful"] == f64 and S.route(Ms, 30, "f32")["careful"] == f32, scale
    assert S.route(M, 30, "f64", careful=False)["careful"] is False
    degenerate = S.normal_matrix(np.ones(30), np.repeat(aa[:2], 30, axis=0))      # one keypoint 30 times: no gap
    assert S.route(degenerate, 30, "f64")["gap_small"]


def _cluster(q, sigma, n=48, seed=0):
    """A 24-px cluster of n keypoints and a vertex whose nearest keypoint is at q sigma^2."""
    rng = np.random.default_rng(seed)
    c = np.array([320.0, 240.0])
    src = (c + rng.uniform(-12, 12, (n, 2))).astype(np.float32)
    dst = (src * 1.02 + [5.0, -3.0] + rng.normal(0, 0.3, src.shape)).astype(np.float32)
    e = np.array([np.cos(0.3 + seed), np.sin(0.3 + seed)])
    want, R = q * sigma * sigma, q * sigma * sigma + 12
    for _ in range(60):
        R += want - np.hypot(*(c + R * e - src.astype(np.float64)).T).min()
    return src, dst, c + R * e


def test_float32_cells_kept_are_inside_the_stated_bound():
    """Dense sweep of the nearest keypoint's x = -2 log2(e) d / sigma^2 from 0 to -160 (and beyond the image: vertices at up
    to 40 000 px): in every cell that K2 keeps on float32 weights, (a) each normal w^2 is within the header's per-weight bound
    of the exact one, (b) the cell's measured perturbation of the normal matrix is within eps_cell, and (c) eps_cell is below
    the header's 5e-5 at x = -126 plus the coordinate term."""
    kept = routed = 0
    for sigma in (1.0, 3.0, 10.0, 30.0):
        for gamma in (0.0, 1e-25, 1e-10, 0.5):
            for x in np.concatenate([np.linspace(0.2, 160, 90), [126, 149, 150]]):
                q = x / (2 * S.LOG2E)
                src, dst, v = _cluster(q, sigma, seed=int(x * 7) % 5)
                aa = O.prepare(src, dst)["aa"]
                r = S.cell(v, src, gamma, sigma, "f32", aa=aa)
                if r["route"]["careful"]:
                    routed += 1
                    continue
                kept += 1
                ex = r["exact"].astype(np.float64)
                normal = (r["region"] == "normal") & (ex >= S.F32_NORMAL_MIN)
                rel = np.abs(r["w2"][normal] - ex[normal]) / ex[normal]
                bound = S.rel_bound_f32(v, src, sigma, r["x"])[normal]
                assert (rel <= bound).all(), (sigma, gamma, x)
                assert r["eps_actual"] <= r["eps_cell"], (sigma, gamma, x)
                coord = 2.0 * 2.0 ** -24 * (2 * np.abs(v).max() + 2 * 400.0) / sigma ** 2
                assert r["eps_cell"] <= 5e-5 + coord, (sigma, gamma, x, r["eps_cell"])
                assert r["cell_region"] == "normal"
    assert kept > 100 and routed > 100


def test_float32_cells_across_the_edge_are_routed():
    """A cluster whose nearest keypoint lies just above x = -126 and whose others lie below it: some w^2 normal, the rest
    flushed to 0 - a normal matrix off by the flushed keypoints' whole share, with a trace (~1e-38) far above the float64
    chain's floor.  The float32 floor sends these cells to the careful path; cells with every w^2 flushed have trace 0."""
    straddling = 0
    for sigma in (3.0, 10.0):
        for x in (118.0, 120.0, 121.0, 123.0, 125.0, 127.0, 135.0, 151.0):
            src, dst, v = _cluster(x / (2 * S.LOG2E), sigma)
            r = S.cell(v, src, 0.0, sigma, "f32", aa=O.prepare(src, dst)["aa"])
            assert r["route"]["careful"] and r["eps_cell"] == 0.0, (sigma, x)
            if (r["region"] == "normal").any() and (r["region"] == "zero").any():
                straddling += 1
                assert r["route"]["trace"] > S.TRACE_FLOOR_F64      # the float64 chain's floor alone keeps them
            if x > 126:
                assert (r["region"] == "zero").all() and r["route"]["trace"] == 0.0
    assert straddling >= 4


def _emulate(src, dst, v, gamma, sigma, chain, fixed=True):
    """What a 24-sum form computes for one cell, in float64 LAPACK: the careful path (rows with the exact weights) where K2
    routes the cell, else the normal matrix of the chain's weights."""
    p = O.prepare(src, dst)
    r = S.cell(v, src, gamma, sigma, chain, aa=p["aa"])
    M = S.normal_matrix(r["w2"], p["aa"])
    careful = r["route"]["careful"] if fixed else S.route(M, src.shape[0], "f64")["careful"]
    if careful:
        H = S.solve_rows((r["exact"] / r["exact"].max()).astype(np.float64), p)
    else:
        H = S.solve_normal(M / max(np.abs(M).max(), 1e-300), p)
    return H, r, p


def test_bar_calibration():
    """BAR_C and FLOOR_ULPS of weight_spec.bar, from the emulation: over clusters at a sweep of distances, gammas and sigmas
    the emulated 24-sum forms stay within a quarter of the bar, and the float32-weight cells that the trace floor of the
    float64 chain alone would leave on float32 weights (clusters across x = -126, part of them flushed) break it."""
    worst = 0.0
    broken = 0
    for sigma in (1.0, 3.0, 10.0):
        for gamma in (0.0, 1e-25, 0.5):
            for x in (1.0, 10.0, 30.0, 60.0, 100.0, 118.0, 120.0, 121.0, 123.0, 125.0, 127.0, 140.0):
                src, dst, v = _cluster(x / (2 * S.LOG2E), sigma, seed=int(x) % 3)
                cond = np.zeros((1, 1))
                with np.errstate(all="ignore"):
                    H_ref, _ = O.local_homography_loop(src, dst, v.reshape(1, 1, 2), gamma, sigma, want_weights=False,
                                                       cond_out=cond)
                scale = max(1.0, float(np.abs(O.project(H_ref[0, 0][None].astype(np.float64), src)).max()))
                ex = S.w2_exact(v, src, gamma, sigma)
                ncond = S.normal_cond(S.normal_matrix((ex / ex.max()).astype(np.float64), O.prepare(src, dst)["aa"]))
                for chain in ("f32", "f64"):
                    H, r, _ = _emulate(src, dst, v, gamma, sigma, chain)
                    d = O.reprojection_rmse_delta(H[None, None], H_ref, src).max()
                    worst = max(worst, d / S.bar(r["eps_cell"], ncond, scale))
                Hu, r, _ = _emulate(src, dst, v, gamma, sigma, "f32", fixed=False)
                du = O.reprojection_rmse_delta(Hu[None, None], H_ref, src).max()
                if du > S.bar(r["eps_cell"], ncond, scale):
                    broken += 1
                    assert r["route"]["careful"] and (r["region"] == "zero").any()
    print(f"worst delta / bar {worst:.3f}; {broken} cells break the bar without the float32 route")
    assert worst < 0.25
    assert broken >= 3
