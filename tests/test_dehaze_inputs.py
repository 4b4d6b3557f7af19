"""The dehazing's named cases (tests/dehaze_cases.py) reach the edges they are named after - asserted from the specification
(tests/dehaze_spec.py) alone, so that tests/test_gpu_dehaze.py, which runs the kernels on them, tests what it says it tests."""
import numpy as np
import pytest

import dehaze_cases as C
import dehaze_spec as S

CASES = C.cases()


def terms(name):
    """The stages of a case: D, (k, T), A, n before the cap, p, the guided filter's terms (refine > 0), t, the recovery's terms."""
    img, p = CASES[name]
    D = S.dark_channel(img, p["radius"])
    A = S.atmospheric_light(img, p["radius"])
    raw_n = ((S.ONE * S.planes(img).astype(np.int64)) // A.astype(np.int64)).min(axis=2)
    praw = S.raw_transmission(img, A, p["radius"], p["omega_q"])
    g = S.guided_terms(S.grey(img), praw, p["refine"], p["eps"]) if p["refine"] else None
    t = S.transmission_q(img, **p)
    num, den = S.recover_terms(img, A, t)
    return dict(img=img, p=p, D=D, kT=S.airlight_threshold(D), A=A, raw_n=raw_n, praw=praw, g=g, t=t, num=num, den=den)


def test_the_cases_follow_the_kernels_tiles(native):
    assert C.TILES == native.DEHAZE_TILES and C.AIR_CHUNK == native.DEHAZE_AIR_CHUNK
    import os
    import re
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "apap_hip.h")).read()
    value = lambda name: int(re.search(rf"#define APAP_DEHAZE_{name} (\d+)", text).group(1))      # noqa: E731
    assert {"min": (value("MIN_TILE_ROWS"), value("MIN_TILE_COLS")), "ab": (value("AB_TILE_ROWS"), value("AB_TILE_COLS")),
            "recover": (value("REC_TILE_ROWS"), value("REC_TILE_COLS"))} == native.DEHAZE_TILES
    assert value("AIR_CHUNK") == native.DEHAZE_AIR_CHUNK and value("MAX_RADIUS") == native.DEHAZE_MAX_RADIUS == S.MAX_RADIUS == S.MAX_REFINE
    assert value("AIR_MAX_BLOCKS") == native.DEHAZE_AIR_MAX_BLOCKS == C.AIR_MAX_BLOCKS and C.AIR_PASS == C.AIR_MAX_BLOCKS * C.AIR_CHUNK
    source = open(os.path.join(os.path.dirname(native.__file__), "csrc", "apap_dehaze.hip")).read()
    assert "kAirMaxBlocks = APAP_DEHAZE_AIR_MAX_BLOCKS;" in source and "kAirChunk = APAP_DEHAZE_AIR_CHUNK;" in source     # the kernel's own
    assert native.DEHAZE_ONE == S.ONE


def test_shapes_and_windows():
    shapes = {name: img.shape[:2] for name, (img, _) in CASES.items()}
    assert shapes["one_pixel"] == (1, 1) and shapes["row_1x40"] == (1, 40) and shapes["col_40x1"] == (40, 1)
    img, p = CASES["all_clamped_5x7"]
    assert img.shape == (5, 7, 3) and p["radius"] == 7 and p["refine"] == 32        # every tap beyond the centre's row and column is clamped
    assert min(p["radius"], p["refine"]) >= max(img.shape[:2]) - 1
    for rows, cols in C.TILES.values():         # one less, equal, one more, in both directions
        for d in (-1, 0, 1):
            assert (rows + d, cols + d) in shapes.values()
    assert any(img.ndim == 2 for img, _ in CASES.values()) and any(img.ndim == 3 for img, _ in CASES.values())
    assert {p["radius"] for _, p in CASES.values()} >= {0, 1, 7, 32} and {p["refine"] for _, p in CASES.values()} >= {0, 1, 32}
    # more than one block of every kernel in some case, in both directions
    assert any(s[0] > 16 and s[1] > 128 for s in shapes.values())


def test_airlight_cases():
    c = terms("air_k1")
    assert c["img"].shape[0] * c["img"].shape[1] < 1000 and c["kT"][0] == 1
    for name, exact in (("air_exact", True), ("air_jump", False)):
        c = terms(name)
        k, T = c["kT"]
        assert k == 3 and T == 200
        assert (int((c["D"] >= T).sum()) == k) == exact and int((c["D"] >= T).sum()) >= k > int((c["D"] > T).sum())
        if not exact:       # ties at the threshold are all in: the winner is one of them only if they are
            assert int((c["D"] >= T).sum()) == 7
    c = terms("air_constant")
    assert (c["D"] == c["D"][0, 0]).all() and c["D"].size > C.AIR_CHUNK and (c["A"] == c["img"][0, 0]).all()
    c = terms("air_two_best")
    img = c["img"]
    first, last = img[0, 0].astype(int), img[-1, -1].astype(int)
    assert first.sum() == last.sum() and (first != last).any() and c["D"][0, 0] >= c["kT"][1] <= c["D"][-1, -1]
    assert img.shape[0] * img.shape[1] > C.AIR_CHUNK                  # the two sit in different blocks of the selection
    sums = img.reshape(-1, 3).astype(int).sum(axis=1)
    assert (sums[1:-1][c["D"].ravel()[1:-1] >= c["kT"][1]] < first.sum()).all() and (c["A"] == img[0, 0]).all()
    c = terms("air_black")
    assert not c["img"].any() and (c["A"] == 1).all()


def test_airlight_cases_beyond_one_pass_of_the_grid():
    """The selection runs min(chunks, AIR_MAX_BLOCKS) blocks; block b scans the chunks b, b + grid, ...  Both cases have more
    pixels than one pass of the whole grid takes, and their marked pixels are the only ones that can win."""
    h, w = C.AIR_PASSES_SHAPE
    N = h * w
    assert N > C.AIR_MAX_BLOCKS * C.AIR_CHUNK == C.AIR_PASS and N % C.AIR_CHUNK != 0 and N < 2 * C.AIR_PASS
    last_block = C.air_place(N - 1, N)[0]

    def candidates(c, marked):
        """The marked pixels are candidates (D >= T); every other candidate's sum is smaller than theirs."""
        flat = c["img"].reshape(-1, 3).astype(int)
        D, T = c["D"].ravel(), c["kT"][1]
        sums = flat.sum(axis=1)
        assert c["img"].shape == (h, w, 3) and c["p"]["radius"] == 0 and (D[list(marked)] >= T).all()
        others = np.ones(N, bool)
        others[list(marked)] = False
        assert len({int(sums[m]) for m in marked}) == 1 and (sums[others & (D >= T)] < sums[marked[0]]).all()
        assert (others & (D >= T)).sum() >= c["kT"][0]          # and there are such: T lies among the background's levels
        return flat

    c = terms("air_second_pass")
    flat = candidates(c, [N - 1])
    block, turn, chunk = C.air_place(N - 1, N)
    assert turn == 1 and chunk < C.AIR_CHUNK and block == last_block > 0 and c["p"]["refine"] == 1       # the second pass's partial chunk
    assert (c["A"] == flat[N - 1]).all() and (flat[:C.AIR_PASS] < c["A"].astype(int)).all()     # no pixel of the first pass comes near

    c = terms("air_ties_across_passes")
    at = list(C.AIR_TIES_AT)
    flat = candidates(c, at)
    assert at == [7, 2 ** 20 + 7, 2 ** 20 + 1024 + 3] or (C.AIR_CHUNK, C.AIR_MAX_BLOCKS) != (1024, 1024)
    assert [C.air_place(i, N)[:2] for i in at] == [(0, 0), (0, 1), (1, 1)] and c["p"]["refine"] == 0
    assert len({tuple(flat[i]) for i in at}) == 3 and all((flat[at[0]] != flat[i]).any() for i in at[1:])      # unlike colours
    assert (c["A"] == flat[at[0]]).all()                      # the lowest index among equals, whatever the launch


def test_transmission_cases():
    for name in ("cap_grey", "cap_bgr"):
        c = terms(name)
        assert (c["raw_n"] > S.ONE).any(), name               # brighter than A in every channel: the cap at 4096 acts
        assert (c["raw_n"] < S.ONE).any()
    c = terms("omega0")
    assert c["p"]["omega_q"] == 0 and (c["praw"] == S.ONE).all()
    c = terms("omega256")
    assert c["p"]["omega_q"] == 256 and c["praw"].min() == 0       # all of the haze taken out where the pixel is A
    c = terms("t0_one")
    assert c["p"]["t0_q"] == S.ONE and (c["t"] == S.ONE).all() and (c["praw"] < S.ONE).any()


def test_guide_cases():
    c = terms("air_constant")
    assert (c["g"]["varN"] == 0).all() and (c["g"]["a_q"] == 0).all()
    widest = 0
    for name in ("noise_eps1_rho32", "noise_eps1_rho1", "step_eps1_rho32", "step_eps1_rho2"):
        c = terms(name)
        g = c["g"]
        assert c["p"]["eps"] == 1 and set(np.unique(c["img"])) == {0, 255}
        inexact = (g["covN"] < 0) & ((S.ONE * g["covN"]) % g["den"] != 0)
        assert inexact.any(), name                            # floor and truncation differ there
        if c["p"]["radius"] == 0:                             # p follows the guide pixel by pixel: |a_q| = 4096 omega (4096 / 255) nearly
            assert np.abs(g["a_q"]).max() > 60000, name
        widest = max(widest, int(np.abs(S.ONE * g["covN"]).max()), int(np.abs(g["num"]).max()))
    assert 1 << 50 < widest < S.LIMIT                         # the int64 bound assertion ran at its widest
    assert CASES["noise_eps1_rho32"][1]["refine"] == 32 == CASES["step_eps1_rho32"][1]["refine"]


def test_recovery_cases():
    c = terms("floor_clips")
    t0_q = c["p"]["t0_q"]
    pre = c["A"].astype(np.int64) + c["num"] // c["den"]
    floor = (c["t"] == t0_q)[..., None]
    assert (floor & (pre < 0)).any() and (floor & (pre > 255)).any()       # t on the floor, I far from A on both sides
    neg = (c["num"] < 0) & (c["num"] % c["den"] != 0)
    assert neg.any()                                          # negative numerators that 2 t does not divide
    seen = False
    for name in CASES:
        c = terms(name)
        neg = (c["num"] < 0) & (c["num"] % c["den"] != 0) & (c["den"] > 2)
        seen = seen or bool(neg.any())
    assert seen


@pytest.mark.parametrize("name", sorted(CASES))
def test_every_case_stays_inside_the_bounds(name):
    """The specification asserts < 2^62 on every intermediate and |a_q| < 2^23; running it is the check."""
    img, p = CASES[name]
    J, t, A = S.dehaze_q(img, **p)
    assert J.shape == img.shape and J.dtype == np.uint8 and t.dtype == np.uint16 and t.shape == img.shape[:2]
    assert p["t0_q"] <= t.min() and t.max() <= S.ONE and A.min() >= 1
