"""The image pyramid's specification (tests/pyramid_spec.py) against independent restatements of its definition, and the claim
that it exists for: on a pair of pictures of unlike scale the chain over the pyramid finds more, and more reliable, matches
than the single-scale chain.  CPU only: numpy against numpy."""
from fractions import Fraction

import numpy as np
import pytest

import corner_spec
import match_spec
import pyramid_cases as C
import pyramid_spec as P
import sift_spec


@pytest.mark.parametrize("side", [32, 33, 34, 35, 63, 64, 65])
def test_halving_equals_the_unrounded_convolution(side):
    """H against the same definition as a float64 convolution on an explicitly padded picture, rounded half up: every sum is an
    integer below 2^16, exact in float64."""
    g = C.noise((side, side + 3), side)
    h, w = g.shape
    pad = np.pad(g.astype(np.float64), 2, mode="reflect")          # numpy's "reflect" is reflect-101
    k = np.outer([1, 4, 6, 4, 1], [1, 4, 6, 4, 1]) / 256.0
    full = sum(k[i, j] * pad[i:i + h, j:j + w] for i in range(5) for j in range(5))
    want = np.floor(full[::2, ::2] + 0.5)
    got = P.halve(g)
    assert got.shape == ((h + 1) >> 1, (w + 1) >> 1) and got.dtype == np.uint8
    assert np.array_equal(got, want)


@pytest.mark.parametrize("side", [32, 33, 34, 35])
def test_three_quarter_equals_bilinear_interpolation_in_rationals(side):
    """Q against bilinear interpolation at source coordinate 4x/3 + 1/6 in exact rationals, rounded half up; and no source
    index leaves the picture, for every residue of the side mod 4."""
    g = C.noise((side, side + 1), side)
    got = P.three_quarter(g)
    assert got.shape == ((3 * side) >> 2, (3 * (side + 1)) >> 2)
    rng = np.random.default_rng(side)
    for y, x in [(0, 0), (got.shape[0] - 1, got.shape[1] - 1)] + [(int(rng.integers(got.shape[0])), int(rng.integers(got.shape[1]))) for _ in range(60)]:
        sy, sx = Fraction(4 * y, 3) + Fraction(1, 6), Fraction(4 * x, 3) + Fraction(1, 6)
        y0, x0 = sy.numerator // sy.denominator, sx.numerator // sx.denominator
        fy, fx = sy - y0, sx - x0
        assert y0 + 1 <= g.shape[0] - 1 and x0 + 1 <= g.shape[1] - 1
        v = ((1 - fy) * ((1 - fx) * int(g[y0, x0]) + fx * int(g[y0, x0 + 1])) + fy * ((1 - fx) * int(g[y0 + 1, x0]) + fx * int(g[y0 + 1, x0 + 1])))
        half_up = (v + Fraction(1, 2)).numerator // (v + Fraction(1, 2)).denominator
        assert int(got[y, x]) == half_up, (y, x)


@pytest.mark.parametrize("value", [0, 1, 127, 254, 255])
def test_a_constant_picture_stays_constant(value):
    lv = P.levels(np.full((200, 131), value, np.uint8), 16, True)
    assert len(lv) == 5 and all((a == value).all() for a in lv)      # widths 131, 98, 66, 49, 33; the next would be 25
    bgr = np.full((90, 90, 3), value, np.uint8)
    assert all((a == P.levels(bgr, 1)[0][0, 0]).all() for a in P.levels(bgr, 16, True))


def test_the_coordinate_map_is_the_centroid_of_the_taps():
    """A level pixel's base-frame coordinate is the weighted mean of the base pixels it averages: H's taps are symmetric about
    2x, Q's two taps (5, 1), (3, 3), (1, 5) have their centroid at 4x/3 + 1/6, and the maps compose."""
    for x in range(40):
        k, r = divmod(x, 3)
        w0, w1 = P.QW[r]
        centroid = Fraction(w0 * (4 * k + r) + w1 * (4 * k + r + 1), 6)
        assert centroid == Fraction(4 * x, 3) + Fraction(1, 6) == Fraction(8 * x + 1, 6)
        assert Fraction(sum(b * (2 * x + i) for b, i in zip(P.B.tolist(), range(-2, 3))), 16) == 2 * x
    hs, ws, off, num, shift = P.layout(2000, 2000, 16, True)
    assert len(hs) == 13 and num == [1, 3] * 6 + [1] and shift == [0, 2, 1, 3, 2, 4, 3, 5, 4, 6, 5, 7, 6]
    x = np.arange(0, 33)
    for level in range(13):
        k = level >> 1
        # level pixel x is pixel 2^k x of the 3/4 level, and that one is base coordinate (8 q + 1) / 6
        exact = [Fraction(8 * 2 ** k * int(v) + 1, 6) if level & 1 else Fraction(2 ** k * int(v)) for v in x]
        got = P.base_coord(x, num[level], shift[level])
        assert got.dtype == np.float32
        assert all(g == np.float32(float(e)) for g, e in zip(got, exact))      # one rounding of the exact rational


def test_level_0_is_the_single_scale_detection_and_description():
    img = C.cases()["scene"]
    for bgr in (False, True):
        pic = np.stack([img, img[::-1], img[:, ::-1]], axis=2) if bgr else img
        pts, feats, level, resp = P.detect_and_describe(pic, 120, n_levels=4)
        n0 = int((level == 0).sum())
        want_pts, want_resp = corner_spec.detect(pic, 120)
        assert n0 == len(want_pts) > 16
        assert pts[:n0].tobytes() == want_pts.tobytes() and resp[:n0].tobytes() == want_resp.tobytes()
        assert feats[:n0].tobytes() == sift_spec.describe(pic, want_pts).tobytes()
        assert (np.diff(level) >= 0).all() and level.max() == 3


# ---------------------------------------------------------------------------------------------- the scale claim
MAX_CORNERS, RATIO, TOL = 600, 0.8, 1.5


def mutual_matches(fa, fb):
    """(query rows, train rows) of the mutual nearest neighbours that pass the ratio test: match_spec's exact matcher."""
    idx, dist, _, dist2 = match_spec.match_int(fa, fb)
    back = match_spec.match_int(fb, fa)[0]
    keep = match_spec.filters(idx, dist, dist2, back, ratio=RATIO, cross_check=True)
    return keep, idx[keep]


def chain(pair, levels):
    """(correct, accepted) of the specification chain on a pair of `scaled_pair` pictures: single scale (levels None) or over
    the pyramid.  A match is correct within TOL pixels of the truth in the coarser picture's frame."""
    (a, ra), (b, rb) = pair
    if levels is None:
        pa, pb = corner_spec.detect(a, MAX_CORNERS)[0], corner_spec.detect(b, MAX_CORNERS)[0]
        fa, fb = sift_spec.describe(a, pa), sift_spec.describe(b, pb)
    else:
        pa, fa = P.detect_and_describe(a, MAX_CORNERS, n_levels=levels)[:2]
        pb, fb = P.detect_and_describe(b, MAX_CORNERS, n_levels=levels)[:2]
    q, t = mutual_matches(fa, fb)
    # pixel x of a picture reduced by r has its centre at scene coordinate r x + (r - 1) / 2
    truth = (ra * pa[q].astype(np.float64) + (ra - 1) / 2 - (rb - 1) / 2) / rb
    err = np.abs(truth - pb[t]).max(axis=1)           # rb >= ra: the second picture is the coarser one
    return int((err <= TOL).sum()), len(q)


@pytest.fixture(scope="module")
def scene_reductions():
    r2, r3, r4 = C.scaled_pair((2, 3, 4))
    return {2: r2, 3: r3, 4: r4}


# measured on the CPU from the specifications alone (seed 11, 720 px scene): correct / accepted
#   s      single scale      levels=6
MEASURED = {
    2.0: ((13, 42), (154, 183)),       # 360 px against 180 px
    1.5: ((33, 60), (238, 268)),       # 360 px against 240 px
    1.0: ((273, 273), (813, 813)),     # 360 px against itself
}


@pytest.mark.parametrize("s", [2.0, 1.5, 1.0])
def test_the_pyramid_chain_survives_a_change_of_scale(scene_reductions, s):
    """At s = 2 and s = 1.5 the chain over six levels finds more correct mutual matches, and a higher correct share of the
    accepted ones, than the single-scale chain (the parent's behaviour) on the same pair; at s = 1 no fewer.  The required
    factor is half the measured ratio of correct matches: the count moves with the seed."""
    rb = {2.0: 4, 1.5: 3, 1.0: 2}[s]
    pair = ((scene_reductions[2], 2), (scene_reductions[rb], rb))
    single, pyramid = chain(pair, None), chain(pair, 6)
    print(f"s = {s}: single scale {single[0]} / {single[1]}, levels=6 {pyramid[0]} / {pyramid[1]}")
    if s == 1.0:
        assert pyramid[0] >= single[0]
        return
    measured_ratio = MEASURED[s][1][0] / max(1, MEASURED[s][0][0])
    assert measured_ratio > 2                        # so that half of it still means "more"
    assert pyramid[0] > single[0] and pyramid[0] >= 0.5 * measured_ratio * single[0]
    assert pyramid[0] * max(1, single[1]) > single[0] * pyramid[1]      # the correct share, cross-multiplied
