"""CPU checks that the inputs of tests/warp_integer_cases.py reach the edges they were built for, from the specifications
alone (oracle/warp_fast_spec.py, the oracle's coordinates): these are conditions on the inputs, not measurements of the
engine.  They also extend tests/test_warp_fast_bound.py's claim - an unflagged pixel has the reference's integer source pixel
and no integer coordinate, whatever legal value v_rcp_f32 returns - from random inputs to inputs concentrated at the doubt
window's edge.  tests/test_gpu_warp_integer.py then holds the kernels to the oracle on the same inputs."""
import numpy as np
import pytest

import warp_integer_cases as W

ULPS = (-1, 0, 1)


def counts(name, ulps):
    k = W.classify(name, ulps)
    return dict(pixels=k["doubt"].size, doubt=int(k["doubt"].sum()), integer=int(k["integer"].sum()),
                above=int(k["above"].sum()), below=int(k["below"].sum()),
                far_above=int((k["above"] & k["far"]).sum()), far_below=int((k["below"] & k["far"]).sum()))


def near_in(name, ulps, kind, **where):
    """Near misses (above, below) in the cells of one kind of a case."""
    k = W.classify(name, ulps)
    kinds = W.get(name)["kinds"]
    a = b = 0
    for rc in np.ndindex(kinds.shape):
        if kinds[rc]["kind"] == kind and all(kinds[rc][key] == v for key, v in where.items()):
            m = (k["cr"] == rc[0]) & (k["cc"] == rc[1])
            a, b = a + int((k["above"] & m).sum()), b + int((k["below"] & m).sum())
    return a, b


def test_the_picture_tells_neighbours_apart():
    img = W.picture(300, 600).astype(np.int64)
    assert img.any(axis=-1).all(), "no pixel is black"
    for dy, dx in ((0, 1), (1, 0), (1, 1), (1, -1)):
        a = img[max(dy, 0):, max(dx, 0):img.shape[1] + min(dx, 0)]
        b = img[:img.shape[0] - dy, max(-dx, 0):img.shape[1] - max(dx, 0)]
        assert (a != b).all(), (dy, dx)


def test_geometries():
    """Every case but ``coarse`` meets the launcher's condition for the float32-estimate kernel (restated in
    ``takes_estimate_kernel``: 254 px cells alone would not - their meshes carry 1 px cells beyond the canvas edge), ``coarse``
    does not; canvas widths 4 k + 1, 4 k + 2 and 4 k + 3, non-zero offsets and a negative one, the six sweep cases on one
    geometry and one picture (one batched launch), a centre that fits wherever the stitch runs, inverses bit for bit numpy's
    (asserted by the builder)."""
    for n in W.FAST_CASES:
        c = W.get(n)
        assert W.takes_estimate_kernel(c), n
        fw, fh = c["final"][:2]
        rows, cols = c["H"].shape[:2]
        assert fw // cols <= 128 and fh // rows <= 128, n                 # warp_impl's fast_ok, literally
        assert max(np.diff(c["mesh"][0]).max(), np.diff(c["mesh"][1]).max()) >= 254 or n == "cap", n
        beyond = [k["kind"] == "beyond the canvas" for k in c["kinds"].ravel()]
        k = W.classify(n)
        used = {(int(r), int(q)) for r, q in zip(k["cr"].ravel()[::97], k["cc"].ravel()[::97])}
        assert any(beyond) and all(c["kinds"][rc]["kind"] != "beyond the canvas" for rc in used), n
    coarse = W.get("coarse")
    assert not W.takes_estimate_kernel(coarse) and coarse["H"].shape[:2] == (2, 4)
    assert np.array_equal(coarse["H"], W.get("sweep_turned")["H"][:2, :4]) and coarse["final"] == W.get("sweep_turned")["final"]
    assert W.takes_estimate_kernel(W.get("f64"))
    finals = [W.get(n)["final"] for n in W.F32_CASES]
    assert {f[0] % 4 for f in finals} >= {1, 2, 3}
    assert any(f[2] > 0 for f in finals) and any(f[3] > 0 for f in finals) and any(f[2] < 0 for f in finals) and any(f[3] < 0 for f in finals)
    assert all(f[0] <= 1016 and f[1] <= 508 for f in finals)
    first = W.get(W.BATCH_CASES[0])
    for n in W.BATCH_CASES:
        c = W.get(n)
        assert c["final"] == first["final"] and c["img"].shape == first["img"].shape
        assert all(np.array_equal(a, b) for a, b in zip(c["mesh"], first["mesh"]))
    assert all(W.get(n)["center"] is not None for n in W.STITCH_CASES)
    with pytest.raises(ValueError):
        first["H"][0, 0, 0, 0] = 0.0          # read-only


@pytest.mark.parametrize("ulps", ULPS)
def test_sweep_cap_and_wide_reach_the_window_s_edge(ulps):
    """sweep + cap + wide together: at least 5 % of the pixels in doubt, at least 2 000 near misses above and 2 000 below, at
    least 200 on each side at a cell's far corner, and near misses in a turned cell, a perspective cell and an m = 3 cell."""
    total = dict(pixels=0, doubt=0, integer=0, above=0, below=0, far_above=0, far_below=0)
    for n in W.EDGE_CASES:
        c = counts(n, ulps)
        print(f"{n} (rcp {ulps:+d} ulp): {c['doubt'] / c['pixels']:.3f} in doubt, {c['integer']} exact integers, near misses "
              f"{c['above']} above / {c['below']} below, at the far corners {c['far_above']} / {c['far_below']}")
        for key in total:
            total[key] += c[key]
    print(f"together (rcp {ulps:+d} ulp): {total}")
    assert total["doubt"] >= 0.05 * total["pixels"]
    assert total["above"] >= 2000 and total["below"] >= 2000
    assert total["far_above"] >= 200 and total["far_below"] >= 200
    for kind, name, where in (("turned", "sweep_turned", {}), ("perspective", "sweep_turned", {}), ("plain", "sweep_m3p", dict(m=3)),
                              ("plain", "sweep_m3n", dict(m=3)), ("cap", "cap", dict(m=3))):
        a, b = near_in(name, ulps, kind, **where)
        print(f"    {kind} cells of {name}: {a} above, {b} below")
        assert a > 0 and b > 0, (kind, name)


def test_every_exponent_multiplier_and_sign_is_there():
    seen = {(k["m"], k["e"], k["s"]) for n in W.BATCH_CASES for k in W.get(n)["kinds"].ravel() if k["kind"] == "plain"}
    assert seen == {(m, e, s) for m in (1, 2, 3) for e in range(16, 22) for s in (1, -1)}
    assert all(W.classify(n)["good"].all() for n in W.BATCH_CASES), "every 254 px sweep cell keeps its bound"


@pytest.mark.parametrize("name", ["integers_a", "integers_b"])
def test_integer_translations(name):
    """At least 20 000 pixels with an exactly integer coordinate (here: all), every one flagged; t = 0 and t = size and their
    inside neighbours 1 and size - 1 occur on both axes in every one of the eight cells."""
    case = W.get(name)
    ih, iw = case["img"].shape[:2]
    for ulps in ULPS:
        k = W.classify(name, ulps)
        c = counts(name, ulps)
        print(f"{name} (rcp {ulps:+d} ulp): {c['doubt'] / c['pixels']:.3f} in doubt, {c['integer']} exact integers, near misses "
              f"{c['above']} above / {c['below']} below, at the far corners {c['far_above']} / {c['far_below']}")
        assert c["integer"] >= 20000 and (k["doubt"] | ~k["integer"]).all(), "an exact integer that is not flagged"
    assert k["integer"].all() and (k["tx"] == np.round(k["tx"])).all() and (k["ty"] == np.round(k["ty"])).all()
    for row in range(2):
        for col in range(4):
            m = (k["cr"] == row) & (k["cc"] == col)
            assert case["kinds"][row, col]["kind"] == "integer" and m.any()
            assert {0.0, 1.0, iw - 1.0, float(iw)} <= set(np.unique(k["tx"][m])), (row, col)
            assert {0.0, 1.0, ih - 1.0, float(ih)} <= set(np.unique(k["ty"][m])), (row, col)
    # the division is a real one: third components 1, 3, 5 and, for 7, its float32 neighbour (see the cases' text)
    assert sorted({float(h[2, 2]) for h in case["hinv"].reshape(-1, 3, 3)}) == [1.0, 3.0, 5.0, 7.0 - 2.0 ** -21]
    inside = (0 < k["tx"]) & (k["tx"] < iw) & (0 < k["ty"]) & (k["ty"] < ih)
    assert inside.mean() > 0.5, "most integer coordinates gather a pixel"


def test_cap_holds_both_kinds_of_cell():
    """Cells 254 px wide: bound of |estimate| above 500 px, no record, every pixel exact.  Cells 200 px wide: a record with a
    window wider than any 254 px sweep cell's."""
    k = W.classify("cap")
    good = {(int(r), int(c)): bool(k["good"][(k["cr"] == r) & (k["cc"] == c)].all()) for r in range(3) for c in range(4)}
    assert all(good[r, c] == (c % 2 == 1) for r in range(3) for c in range(4)), good
    assert k["doubt"][~k["good"]].all()
    widest = max(W.classify(n)["win"].max() for n in W.BATCH_CASES)
    assert np.isfinite(widest) and k["win"][k["good"]].min() > widest


def test_wide_reaches_the_extra_column_and_a_third_cell_in_a_group():
    case, k = W.get("wide"), W.classify("wide")
    widths = np.diff(case["mesh"][0])
    assert {254.0, 255.0, 256.0, 2.0} <= set(widths)
    cols = np.arange(case["final"][0])
    past = ((cols >= 254 + 254) & (cols < 509)) | ((cols >= 509 + 254) & (cols < 765))       # past the clamped span
    assert past.sum() == 3 and k["doubt"][:, past].all() and not k["good"][:, past].any()
    groups = k["cc"][0, :case["final"][0] // 4 * 4].reshape(-1, 4)
    assert (np.array([len(set(g)) for g in groups]) == 3).any(), "a lane's four pixels in three cells"


@pytest.mark.parametrize("name", W.F32_CASES)
def test_the_spec_s_claim_on_these_inputs(name):
    """No unflagged pixel has floor(t) != estimate or an integer t: for the reciprocal -1, 0 and +1 ulp off and a random mix."""
    case = W.get(name)
    fw, fh = case["final"][:2]
    rng = np.random.default_rng(31)
    for ulps in ULPS + (rng.integers(-1, 2, size=(fh, fw)),):
        k = W.classify(name, ulps)
        sure = ~k["doubt"]
        assert (np.floor(k["tx"][sure]) == k["ix"][sure]).all() and (np.floor(k["ty"][sure]) == k["iy"][sure]).all()
        assert not k["integer"][sure].any()
        assert not (sure & ~k["good"]).any(), "a pixel without a bound must be flagged"


def test_float64_case():
    """On numpy's float64 inverses: on each side at least 1 000 non-integer coordinates within 2^-36 of an integer, at least
    1 000 exact integers, third component 3 (up to the inverse's last bits)."""
    from oracle import apap_oracle as O
    case = W.get("f64")
    H = case["H"]
    assert H.dtype == np.float64 and not np.array_equal(H.astype(np.float32).astype(np.float64), H)
    hinv = np.linalg.inv(H)
    assert np.allclose(hinv[..., 2, 2], 3.0, rtol=1e-15)
    fw, fh, ox, oy = case["final"]
    above = below = integer = 0
    for t in O.warp_coords_fast(hinv, case["mesh"], (fw, fh), (ox, oy)):
        whole = t == np.floor(t)
        integer += int(whole.sum())
        above += int((~whole & (t - np.floor(t) < 2.0 ** -36)).sum())
        below += int((~whole & (np.ceil(t) - t < 2.0 ** -36)).sum())
    print(f"f64: {above} coordinates within 2^-36 above an integer, {below} below, {integer} exact integers")
    assert above >= 1000 and below >= 1000 and integer >= 1000
