"""The pictures of tests/pyramid_cases.py reach the edges they are named for: asserted from the specification alone (numpy,
no GPU), so that the GPU tests over them cannot pass by missing their point."""
import numpy as np

import corner_spec
import pyramid_cases as C
import pyramid_spec as P


def test_every_residue_and_parity_is_there():
    cases = C.cases()
    assert all(min(a.shape[:2]) >= P.MIN_SIDE for a in cases.values())
    for s in (32, 33, 34, 35):      # level 0 alone: a 3/4 level of 24 .. 26 pixels does not exist
        assert len(P.levels(cases[f"side{s}"], 16)) == 1
    q_sources = {cases[f"side{s}"].shape[0] % 4 for s in (43, 44, 45, 46)} | {cases[f"side{s}"].shape[1] % 4 for s in (43, 44, 45, 46)}
    assert q_sources == {0, 1, 2, 3}
    assert all(len(P.levels(cases[f"side{s}"], 16)) >= 2 for s in (43, 44, 45, 46))
    h_sources = [a.shape for name in ("side63", "side64", "side65") for a in P.levels(cases[name], 16)[:1]]
    assert {s[0] % 2 for s in h_sources} == {0, 1}
    assert all(len(P.levels(cases[name], 16)) >= 3 for name in ("side63", "side64", "side65"))     # H of the picture exists


def test_tiles_and_strip():
    cases = C.cases()
    h, w = cases["past_tile_w"].shape
    assert w == 2 * C.TILE_W + 1 and h > C.TILE_H                       # a last tile column one pixel wide, two tile rows
    h, w = cases["past_tile_h"].shape
    assert h == 3 * C.TILE_H + 1 and w < C.TILE_W
    assert cases["strip"].shape == (32, 300) and len(P.levels(cases["strip"], 16)) == 1      # no level below 32 rows
    assert cases["bgr_wide"].shape[1] * 3 % 4 != 0                      # BGR rows start at unlike byte alignments
    assert len(P.levels(cases["scene"], 6)) == 6 and len(P.levels(cases["scene"], 16)) == 6


def test_rounding_keeps_the_extremes():
    for name, value in (("white", 255), ("black", 0)):
        lv = P.levels(C.cases()[name], 16)
        assert len(lv) >= 3 and all((a == value).all() for a in lv)
        assert corner_spec.detect(lv[0], 50)[0].shape == (0, 2)        # a level with no corner: the pack's empty level


def test_a_reflected_tap_contributes():
    """On the framed picture H's corner pixel differs from what a replicated border (or a zero border) would give."""
    g = C.cases()["framed"].astype(np.int64)
    got = P.halve(g)
    h, w = g.shape
    for mode in ("edge", "constant"):
        pad = np.pad(g, 2, mode=mode)
        k = np.outer(P.B, P.B)
        other = np.array([[((k * pad[2 * y:2 * y + 5, 2 * x:2 * x + 5]).sum() + 128) >> 8 for x in range((w + 1) >> 1)] for y in range((h + 1) >> 1)])
        assert (other != got).any() and other[0, 0] != got[0, 0]
    assert (h % 2, w % 2) == (0, 1)                                     # the far edges reflect from an even and an odd side


def test_the_chains_end_at_different_depths():
    """Some pictures end on a 3/4 level and some on an octave level; the batch's first picture has level 0 alone."""
    counts = {name: len(P.layout(a.shape[0], a.shape[1], 16, True)[0]) for name, a in C.cases().items()}
    assert {c % 2 for c in counts.values()} == {0, 1} and max(counts.values()) == 6
    batch = C.batch()
    assert len(batch) == 6 and len(P.levels(batch[0], 16)) == 1
    assert len({a.shape for a in batch}) == 6 and {a.ndim for a in batch} == {2, 3}
    assert len({len(P.levels(a, 16)) for a in batch}) >= 3
    assert len(P.levels(C.cases()["side64"], 16, False)) == 2 and len(P.levels(C.cases()["scene"], 16, False)) == 3


def test_both_bounds_of_the_corner_budget_bind():
    caps = P.level_caps(100, 6)
    assert caps == [100, 56, 25, 16, 16, 16]                            # max(16, ...) binds from level 3 on
    assert P.level_caps(10, 4) == [10, 10, 10, 10]                      # min(max_corners, ...) binds: 16 > max_corners
    assert P.level_caps(600, 6) == [600, 337, 150, 84, 37, 21] and P.level_caps(600, 3, False) == [600, 150, 37]
    # on the scene the cap cuts a level's list (more corners than its cap) and leaves another whole
    lv = P.levels(C.cases()["scene"], 6)
    found = [len(corner_spec.detect(a, 10 ** 6)[0]) for a in lv]
    assert any(f > c for f, c in zip(found, caps)) and any(0 < f < c for f, c in zip(found, caps)), (found, caps)
