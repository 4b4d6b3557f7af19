"""Exposure gain compensation of the panorama without a GPU (DESIGN.md "Panorama, gain compensation"): the host functions
of the C ABI against tests/panorama_gain_spec.py, the specification against its own normal equations and on a planted pair,
and every refusal."""
import math
from fractions import Fraction

import numpy as np
import pytest

import panorama_cases as E
import panorama_gain_spec as G
import panorama_ramp_cases as RC


def random_tables(rng, v, hole=0.3):
    """Symmetric counts (some pairs without overlap) and sums with S_ab <= 765 N_ab; the diagonal a view by itself."""
    N = np.zeros((v, v), np.uint64)
    S = np.zeros((v, v), np.uint64)
    for a in range(v):
        for b in range(a, v):
            n = 0 if (a != b and rng.random() < hole) else int(rng.integers(1, 2_000_000))
            N[a, b] = N[b, a] = n
            S[a, b] = int(n * rng.uniform(0.0, 765.0))
            S[b, a] = int(n * rng.uniform(0.0, 765.0))
    return N, S


def same_as_spec(native, N, S, sigma_n=10.0, sigma_g=0.1):
    g, q, flag = native.panorama_gain_solve(N, S, sigma_n, sigma_g)
    want_g, want_q, want_flag = G.solve(N, S, sigma_n, sigma_g)
    assert g.dtype == np.float64 and g.tobytes() == np.array(want_g, np.float64).tobytes(), (g, want_g)
    assert q.tolist() == want_q and flag == want_flag
    return g, q, flag


def test_apply_is_the_spec_for_every_value_and_gain(native):
    values = np.arange(256, dtype=np.uint8)
    for q in range(G.MIN_Q, G.MAX_Q + 1):
        assert np.array_equal(native.panorama_gain_apply(values, q), G.apply(values, q)), q
    assert np.array_equal(native.panorama_gain_apply(values, G.UNIT), values)
    assert native.panorama_gain_apply(values, G.MAX_Q).max() == 255 and native.panorama_gain_apply(values, G.MIN_Q)[1] == 0
    for bad in (G.MIN_Q - 1, G.MAX_Q + 1, 0, -4096):
        with pytest.raises(native.ApapError) as e:
            native.panorama_gain_apply(values, bad)
        assert e.value.code == native.ERR_INVALID_ARG


def test_solve_is_the_spec_bit_for_bit(native):
    rng = np.random.default_rng(2007)
    for k in range(200):
        v = 2 + k % 16
        N, S = random_tables(rng, v)
        g, q, flag = same_as_spec(native, N, S, *((10.0, 0.1) if k % 4 else (rng.uniform(1.0, 30.0), rng.uniform(0.02, 1.0))))
        assert flag == 0 and len(g) == v


def test_solve_on_chosen_tables(native):
    # a view without overlap: its gain is 1.0 exactly, whatever the others do
    N = np.array([[9, 5, 0], [5, 9, 0], [0, 0, 7]], np.uint64)
    S = np.array([[900, 500, 0], [800, 1400, 0], [0, 0, 2100]], np.uint64)
    g, q, _ = same_as_spec(native, N, S)
    assert g[2] == 1.0 and q[2] == G.UNIT and g[0] != 1.0
    # two views with equal statistics
    N = np.array([[100, 60], [60, 100]], np.uint64)
    S = np.array([[30000, 18000], [18000, 30000]], np.uint64)
    g, q, _ = same_as_spec(native, N, S)
    assert q.tolist() == [G.UNIT, G.UNIT] and abs(g[0] - 1.0) < 1e-12 and abs(g[1] - 1.0) < 1e-12
    # one view twice as bright as the other: the dark one is raised, the bright one lowered
    S = np.array([[30000, 36000], [18000, 15000]], np.uint64)
    g, q, _ = same_as_spec(native, N, S)
    assert g[1] > 1.0 > g[0] and q[1] > G.UNIT > q[0]
    # all 17 views overlap everywhere on the largest canvas, with the largest sums and with none
    n = 2 ** 31 - 1
    N = np.full((17, 17), n, np.uint64)
    for S in (np.full((17, 17), 765 * n, np.uint64), np.zeros((17, 17), np.uint64)):
        g, q, flag = same_as_spec(native, N, S)
        assert flag == 0 and q.tolist() == [G.UNIT] * 17 and np.abs(g - 1.0).max() < 1e-9


def test_spec_solves_its_normal_equations():
    """In exact fractions: the residual of the float64 solution is below 1e-12 of the sizes involved."""
    rng = np.random.default_rng(6)
    for k in range(40):
        N, S = random_tables(rng, 2 + k % 16)
        g, _, flag = G.solve(N, S)
        assert flag == 0
        A, rhs = G.normal_equations(N, S)
        x = [Fraction(v) for v in g]
        for row, r in zip(A, rhs):
            resid = abs(sum(a * v for a, v in zip(row, x)) - r)
            scale = sum(abs(a * v) for a, v in zip(row, x)) + abs(r)
            assert resid <= Fraction(1, 10 ** 12) * scale, float(resid / scale)


def smooth_picture(w, h):
    """No pixel black, no channel near 255 after a gain of 1.25: a pattern that a shift of a pixel barely changes."""
    y, x = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    return np.stack([120 + 70 * np.sin(0.05 * x + 0.5 * c) * np.cos(0.04 * y - 0.3 * c) for c in range(3)], axis=-1).astype(np.uint8)


def test_spec_on_a_planted_pair():
    """One layer that shows the centre's content at 0.8 of its brightness, placed on the centre: the gains bring the two
    views together, and the prior keeps the ratio short of 1 / 0.8."""
    rng = np.random.default_rng(80)
    center = smooth_picture(96, 64)
    dark = (center.astype(np.float64) * 0.8).astype(np.uint8)
    layer = E.make_layer(rng, center.shape, 96, 64, E.placement(0.0, 0.0), 1, 1, img=dark)
    geos = [tuple(layer.final_size) + tuple(layer.offset)]
    values, _ = G.samples(center, [layer], geos, [RC.layer_coords(layer)])
    N, S = G.stats(values, 1)
    assert N[0, 1] == N[1, 0] > 0.9 * 96 * 64 and S[0, 1] > S[1, 0]
    g, q, flag = G.solve(N, S)
    assert flag == 0 and 1.0 < g[1] / g[0] < 1.25
    both = values[0].any(axis=-1) & values[1].any(axis=-1)
    before = np.abs(values[0].astype(np.int64) - values[1].astype(np.int64))[both].mean()
    after = np.abs(G.apply(values[0], q[0]).astype(np.int64) - G.apply(values[1], q[1]).astype(np.int64))[both].mean()
    assert after < 0.5 * before, (before, after)


def test_spec_application_keeps_presence():
    """A (1, 0, 0) sample under the smallest gain turns black and still counts; q = 4096 composes the ungained canvas."""
    values = np.zeros((3, 1, 2, 3), np.uint8)
    values[0, 0, 0] = (200, 100, 50)
    values[1, 0, 0] = (1, 0, 0)
    values[1, 0, 1] = (1, 0, 0)
    values[2, 0, 1] = (9, 9, 9)
    one = lambda ramp: np.ones((3, 1, 2), np.int64)     # noqa: E731
    rect = (0, 0, 1, 1)
    q = [G.UNIT, G.MIN_Q, G.UNIT]
    assert G.compose(values, one, rect, q, "mean").tolist() == [[[100, 50, 25], [4, 4, 4]]]      # (0 + 9) // 2: the black one counts
    assert G.compose(values, one, rect, q, "paste").tolist() == [[[200, 100, 50], [0, 0, 0]]]    # layer 0 wins as black
    assert G.compose(values, one, rect, [G.UNIT] * 3, "mean").tolist() == [[[100, 50, 25], [5, 4, 4]]]


def small_case():
    case = E.TILING_CASES["two_pixels"]()
    return case["center"], case["layers"]


def test_refusals_come_before_any_device(native):
    center, layers = small_case()
    bad = lambda call: pytest.raises(native.ApapError, match=r"apap_hip error 1\]")       # noqa: E731  APAP_ERR_INVALID_ARG
    for step in (0, -1, 65):
        with bad(None):
            native.panorama_gain_stats(center, layers, step=step)
        with bad(None):
            native.panorama_auto_gain(center, layers, step=step)
    for q in ([4096, 1023, 4096], [4096, 4096, 16384], [0, 4096, 4096]):
        for blend in ("mean", "paste", "ramp"):
            with bad(None):
                native.panorama(center, layers, blend=blend, ramp=8, gain_q=q)
    for q in ([4096, 4096], [4096] * 4, [4096.0] * 3, "auto"):
        with pytest.raises(ValueError, match="gain_q"):
            native.panorama(center, layers, gain_q=q)
    for sigma in (0.0, -1.0, math.inf, math.nan):
        with bad(None):
            native.panorama_auto_gain(center, layers, sigma_n=sigma)
        with bad(None):
            native.panorama_auto_gain(center, layers, sigma_g=sigma)
        with bad(None):
            native.panorama_gain_solve(np.ones((2, 2), np.uint64), np.ones((2, 2), np.uint64), sigma_n=sigma)
        with bad(None):
            native.panorama_gain_solve(np.ones((2, 2), np.uint64), np.ones((2, 2), np.uint64), sigma_g=sigma)
    for v in (1, 18):
        with bad(None):
            native.panorama_gain_solve(np.ones((v, v), np.uint64), np.ones((v, v), np.uint64))
    # what apap_panorama refuses: an unknown mode, a ramp outside 1 .. 256, a picture of one pixel
    import ctypes as C
    args, keep, n, (W, H, _, _) = native._panorama_inputs(center, layers, "t")
    out, status, q = np.zeros((H, W, 3), np.uint8), np.zeros(n, np.int32), np.full(n + 1, 4096, np.int32)
    for mode, ramp in ((3, 8), (-1, 8), (native.PANORAMA_RAMP, 0), (native.PANORAMA_RAMP, 257)):
        code = native.lib().apap_panorama_gain(None, *args, mode, ramp, native._ip(q), native._ptr(out, C.c_uint8), native._ip(status), -1)
        assert code == native.ERR_INVALID_ARG, (mode, ramp)
    with pytest.raises(ValueError, match="ramp"):
        native.panorama(center, layers, blend="ramp", ramp=0, gain_q=[4096] * 3)
    with bad(None):
        native.panorama(center[:1, :1], layers, gain_q=[4096] * 3)
    from cvx_proj_amd import apap
    with pytest.raises(ValueError, match="gain"):
        apap.panorama(center, layers, gain="manual")


def test_no_cpu_fallback(native):
    if native.lib().apap_device_count() > 0:
        pytest.skip("a GPU is visible")
    from cvx_proj_amd import apap
    center, layers = small_case()
    for call in (lambda: native.panorama_gain_stats(center, layers, step=1),
                 lambda: native.panorama(center, layers, gain_q=[4096, 5000, 3000]),
                 lambda: native.panorama(center, layers, blend="ramp", ramp=4, gain_q=[4096, 5000, 3000]),
                 lambda: native.panorama_auto_gain(center, layers),
                 lambda: apap.panorama(center, layers, gain="auto"),
                 lambda: apap.panorama_gains(center, layers)):
        with pytest.raises(native.ApapError) as e:
            call()
        assert e.value.code == native.ERR_NO_DEVICE
