"""The inputs of tests/sift_orient_cases.py reach the edges they were built for: asserted from the numpy specification alone
(tests/sift_orient_spec.py), so that tests/test_gpu_sift_orient.py cannot pass without exercising them.  The inputs are hashed."""
import numpy as np

import sift_orient_cases as K
import sift_orient_spec as O

DIGEST = "df34d1e7905d5df3553a1b1b95e01eca6d7cda2255bda85758aba11820a5da1f"
U22 = np.float32(2.0 ** -22)      # one ulp of a rotated coordinate near +-2.5


def test_the_inputs_are_the_hashed_ones():
    assert K.digest(K.cases()) == DIGEST


def _orient_detail(name):
    img, pts, _ = K.cases()[name]
    d = {}
    d["angle"] = O.orient(img, pts, detail=d)
    return d


def test_gradient_angles_on_the_octants_and_the_half_bins():
    """Valid samples with a non-zero gradient whose angle is exactly 0, 45, .. 315; ang 0.1 exactly on a half, where rint to
    even decides (45 -> 4.5 -> 4, 135 -> 13.5 -> 14, 225 -> 22, 315 -> 32); rint = 36 wrapped to bin 0."""
    seen, halves, wraps = set(), {}, 0
    for name in K.cases():
        d = _orient_detail(name)
        live = d["valid"] & (d["hist"].any(axis=1))[:, None]
        ang, sc, b = d["ang"][live], d["scaled"][live], d["bin"][live]
        seen |= {int(a) for a in (0, 45, 90, 135, 180, 225, 270, 315) if np.any(ang == a)}
        on_half = sc - np.floor(sc) == 0.5
        for s, k in zip(sc[on_half], b[on_half]):
            halves[float(s)] = int(k)
        wraps += int(np.count_nonzero((np.rint(sc) == 36) & (b == 0)))
    assert seen == {0, 45, 90, 135, 180, 225, 270, 315}
    assert halves == {4.5: 4, 13.5: 14, 22.5: 22, 31.5: 32}
    assert wraps >= 100


def test_the_histogram_edges():
    zero = ties = neg = high = wrapped36 = flushed = den0 = 0
    for name in K.cases():
        d = _orient_detail(name)
        some = d["hist"].any(axis=1)
        zero += int(np.count_nonzero(~some))
        assert np.all(d["angle"][~some] == 0) and np.all(d["den"][~some] == 0)       # the all-zero histogram: angle 0
        den0 += int(np.count_nonzero(d["den"] == 0))
        top = np.sort(d["smooth"], axis=1)
        tie = some & (top[:, -1] == top[:, -2])
        ties += int(np.count_nonzero(tie))
        for k in np.nonzero(tie)[0]:                                                  # the first of the equal bins is the peak
            assert d["peak"][k] == np.nonzero(d["smooth"][k] == top[k, -1])[0][0]
        neg += int(np.count_nonzero(d["raw"] < 0))
        high += int(np.count_nonzero(d["raw"] >= 36))
        flushed += int(np.count_nonzero(d["flushed"] & some))
        assert np.all((d["angle"] >= 0) & (d["angle"] < 360))
    assert zero >= 1000 and den0 >= zero and ties >= 10 and neg >= 10 and flushed >= 100
    # |off| <= 0.5 at a largest bin (l, r <= c), so 35 + off never reaches 36: OpenCV's upper wrap cannot be entered here
    assert high == 0
    d = _orient_detail("bright column 13 x 13")
    img, pts, _ = K.cases()["bright column 13 x 13"]
    k = int(np.nonzero((pts[:, 0] == 6) & (pts[:, 1] == -1))[0][0])
    assert d["hist"][k, 0] == d["hist"][k, 18] > 0 and d["peak"][k] == 0


def test_the_given_angles_and_the_bin_coordinates_at_their_limits():
    want = set(np.float32([0, 90, 180, 270, 360, 45]).tolist())
    for v in (90, 180, 270, 45):
        want |= {float(np.nextafter(np.float32(v), np.float32(0))), float(np.nextafter(np.float32(v), np.float32(999)))}
    want |= {float(np.nextafter(np.float32(0), np.float32(1))), float(np.nextafter(np.float32(360), np.float32(0)))}
    assert want <= set(K.SPECIAL_ANGLES.tolist())
    counts = dict(integer=0, m1=0, m1_below=0, m1_above=0, p4=0, p4_below=0, p4_above=0)
    for name, (img, pts, angles) in K.cases().items():
        d = {}
        O.describe(img, pts, angles, detail=d)
        both = np.concatenate([d["rbin"][d["valid"]], d["cbin"][d["valid"]]])
        counts["integer"] += int(np.count_nonzero(both == np.rint(both)))
        counts["m1"] += int(np.count_nonzero(both == -1))
        counts["m1_below"] += int(np.count_nonzero(both == np.float32(-1) - U22))
        counts["m1_above"] += int(np.count_nonzero(both == np.float32(-1) + U22))
        counts["p4"] += int(np.count_nonzero(both == 4))
        counts["p4_below"] += int(np.count_nonzero(both == np.nextafter(np.float32(4), np.float32(0))))
        counts["p4_above"] += int(np.count_nonzero(both == np.nextafter(np.float32(4), np.float32(9))))
    print(counts)
    assert all(v >= 1 for v in counts.values()), counts
    assert counts["integer"] >= 100


def test_the_small_images():
    shapes = {c[0].shape[:2] for c in K.cases().values()}
    assert {(13, 13), (13, 40), (40, 13), (40, 50)} <= shapes
