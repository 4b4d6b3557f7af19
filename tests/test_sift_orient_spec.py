"""Keypoint orientation without a GPU: the specification's own consistency (tests/sift_orient_spec.py) - patch form against
full-image form, the library's tables, the sin and cos polynomials, float32 against the float64 definition, equivariance under
a quarter turn, and what orientation buys on a turned picture.  The recorded figures are those of DESIGN.md "Keypoint
orientation"; each assertion allows twice its recording."""
import numpy as np
import pytest

import sift_orient_cases as K
import sift_orient_spec as O
import sift_spec as S
from conftest import ulp_diff_f32
from test_sift_host import scene

SINCOS_ERROR = 2.07e-7          # recorded: the largest |error| of the float32 sin and cos on the grid below
ANGLE_ERROR_DEG = 7.0e-4        # recorded: float32 angle against the float64 definition, kept keypoints of the scene below
TURN_ANGLE_ERROR_DEG = 5.7e-14  # recorded: float64 definition, angle after the quarter turn against angle - 90
TURN_DESCR_ERROR = 0.0          # recorded: float64 definition, descriptors after the quarter turn; asserted as < 1 (integers)


def circular(a, b):
    return np.abs((np.asarray(a, np.float64) - np.asarray(b, np.float64) + 180) % 360 - 180)


@pytest.mark.parametrize("shape", [(13, 13), (15, 40), (37, 53, 3)], ids=str)
def test_patch_form_equals_full_image_form_at_every_pixel(shape):
    img = np.random.default_rng(sum(shape)).integers(0, 256, shape).astype(np.uint8)
    pts = K.E.every_pixel_and_a_ring(*shape[:2])
    a = O.orient(img, pts)
    assert a.tobytes() == O.orient(img, pts, local=True).tobytes()
    given = K.given_angles(len(pts), 3)
    for angles in (None, a, given):
        assert O.describe(img, pts, angles).tobytes() == O.describe(img, pts, angles, local=True).tobytes()
    assert O.describe(img, pts).tobytes() == O.describe(img, pts, a).tobytes()           # fused = orient, then given
    assert len(np.unique(a)) > 20 and O.describe(img, pts).any()


def test_library_tables_equal_the_specification(native):
    wo, wd = native.sift_orient_window(), native.sift_descr_window()
    assert wo.dtype == wd.dtype == np.float32 and wo.shape == (25,) and wd.shape == (121,)
    assert ulp_diff_f32(wo, O.orient_window_f64().astype(np.float32)).max() <= 1
    assert ulp_diff_f32(wd, O.descr_window_f64().astype(np.float32)).max() <= 1
    assert wo[12] == 1 and wd[60] == 1 and np.array_equal(wo, wo[::-1]) and np.array_equal(wd, wd[::-1])
    # OpenCV's exp(-(c_rot^2 + r_rot^2) / 8) at two angles: the table does not depend on the angle
    ii, jj = O.offsets(5)
    for deg in (0.0, 33.0):
        cs, sn = np.cos(np.radians(deg)) / 1.5, np.sin(np.radians(deg)) / 1.5
        c_rot, r_rot = jj * cs - ii * sn, jj * sn + ii * cs
        assert np.allclose(np.exp(-(c_rot ** 2 + r_rot ** 2) / 8), O.descr_window_f64(), rtol=1e-14)
    assert native.lib().apap_sift_orient_window(None) == native.ERR_INVALID_ARG
    assert native.lib().apap_sift_descr_window(None) == native.ERR_INVALID_ARG


def test_sin_and_cos_against_float64():
    deg = np.concatenate([np.linspace(0, 360, 2_000_001, endpoint=False), K.SPECIAL_ANGLES.astype(np.float64)]).astype(np.float32)
    deg = deg[deg < 360]
    cs, sn = O.sincos_deg32(deg)
    cs64, sn64 = O.sincos_deg64(deg)
    err = max(float(np.abs(cs - cs64).max()), float(np.abs(sn - sn64).max()))
    print("largest |error| of sin and cos:", err)
    assert err <= 2 * SINCOS_ERROR < 2e-6
    quarter = O.sincos_deg32(np.float32([0, 90, 180, 270]))
    assert np.array_equal(quarter[0], np.float32([1, 0, -1, 0])) and np.array_equal(quarter[1], np.float32([0, 1, 0, -1]))
    # the reduction is exact: ori - 90 q in float32 is the real difference
    q = (deg >= 90).astype(np.int64) + (deg >= 180) + (deg >= 270)
    assert np.array_equal((deg - np.float32(90) * q.astype(np.float32)).astype(np.float64), deg.astype(np.float64) - 90.0 * q)


def test_float32_against_the_float64_definition(native):
    img = scene()                                                     # 128 x 96 BGR
    h, w = img.shape[:2]
    pts = np.random.default_rng(1).uniform(-2, [w + 2, h + 2], (2000, 2)).astype(np.float32)
    d = {}
    a64 = O.orient64(img, pts, detail=d)
    a32 = O.orient(img, pts, native.sift_taps(), native.sift_orient_window())
    # excluded: a sample within 1e-4 degrees of a bin boundary (bins are 10 degrees wide, boundaries at 5, 15, ..), or the two
    # largest smoothed bins within 1e-5 relative - in the float64 definition alone
    on_boundary = ((np.abs(d["scaled"] - np.floor(d["scaled"]) - 0.5) < 1e-5) & d["valid"]).any(axis=1)
    top = np.sort(d["smooth"], axis=1)
    close = d["hist"].any(axis=1) & (top[:, -1] - top[:, -2] < 1e-5 * top[:, -1])
    out = on_boundary | close
    print("excluded:", int(out.sum()), "of", len(pts))
    assert out.sum() <= 0.01 * len(pts)
    err = circular(a32, a64)[~out].max()
    print("largest angle difference of the kept keypoints:", err, "degrees")
    assert err <= 2 * ANGLE_ERROR_DEG
    assert a32.dtype == np.float32 and np.all((a32 >= 0) & (a32 < 360)) and len(np.unique(a32)) > 1500
    f32 = O.describe(img, pts, a32, native.sift_taps(), native.sift_orient_window(), native.sift_descr_window())
    f64 = O.describe64(img, pts, a64)
    assert np.array_equal(f32, np.rint(f32)) and f32.min() >= 0 and f32.max() <= 255 and not np.isnan(f32).any()
    diff = np.abs(f32 - f64)[~out]
    print("descriptors: max difference", float(diff.max()), "share of differing values", np.count_nonzero(diff) / diff.size)
    assert diff.max() <= 1
    assert np.count_nonzero(f32.any(axis=1)) >= 1900


@pytest.fixture(scope="module")
def turn():
    return K.quarter_turn_pair()


def test_quarter_turn_in_the_float64_definition(turn):
    img, turned, pts, tpts = turn
    assert len(pts) >= 50
    d = {}
    a1, a2 = O.orient64(img, pts, detail=d), O.orient64(turned, tpts)
    assert not np.any(np.abs(d["scaled"] - np.floor(d["scaled"]) - 0.5) < 1e-9)          # the scene's premise (sift_orient_cases.py)
    err = circular(a2, a1 - 90).max()
    f1, f2 = O.describe64(img, pts, a1), O.describe64(turned, tpts, a2)
    print("quarter turn: angle", err, "descriptors", np.abs(f1 - f2).max())
    assert err <= 2 * TURN_ANGLE_ERROR_DEG
    assert TURN_DESCR_ERROR == 0 and np.abs(f1 - f2).max() < 1
    assert f1.any(axis=1).all() and np.ptp(a1) > 180


def test_orientation_finds_the_partners_on_a_turned_picture(turn, native):
    img, turned, pts, tpts = turn
    consts = (native.sift_taps(), native.sift_orient_window(), native.sift_descr_window())
    oriented = K.partner_share(O.describe(img, pts, None, *consts), O.describe(turned, tpts, None, *consts))
    plain = K.partner_share(S.describe(img, pts), S.describe(turned, tpts))
    exact = K.partner_share(O.describe64(img, pts), O.describe64(turned, tpts))
    print("true-partner share on the quarter turn: oriented", oriented, "unoriented", plain, "float64 definition", exact)
    assert oriented > plain
    assert oriented >= exact - 1.0 / len(pts) - 1e-12
