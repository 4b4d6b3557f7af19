"""SIFT descriptor extraction without a GPU: the specification's own consistency (tests/sift_spec.py), the library's
constants against it, argument refusals before any device is touched, and the no-device error."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import sift_spec as S
from conftest import ROOT, ulp_diff_f32


def i32(*v):
    return np.array(v, np.int32)


def p(a, t=C.c_int):
    return a.ctypes.data_as(C.POINTER(t))


def scene(h=96, w=128, seed=0):
    """A seeded (h, w, 3) BGR image: sinusoids plus noise."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[:h, :w]
    planes = [127 + 60 * np.sin(xx / (5 + 2 * k)) * np.cos(yy / (7 - k)) + rng.normal(0, 8, (h, w)) for k in range(3)]
    return np.stack(planes, -1).clip(0, 255).astype(np.uint8)


def test_window_table_is_the_49_offsets():
    """window_f64 walks OpenCV's radius of 5 and asserts itself that exactly |i|, |j| <= 3 pass -1 < rbin, cbin < 4."""
    t = S.window_f64()
    assert t.shape == (49, 8) == (S.SAMPLES, S.WINDOW_COLS)
    assert np.all((t[:, 0] > -1) & (t[:, 0] < 4) & (t[:, 1] > -1) & (t[:, 1] < 4))
    assert np.array_equal(t[:, 5], np.floor(t[:, 0])) and np.array_equal(t[:, 6], np.floor(t[:, 1]))
    assert t[:, 5].min() == -1 and t[:, 5].max() == 3 and t[:, 6].min() == -1 and t[:, 6].max() == 3
    assert np.all((t[:, 2] > 0) & (t[:, 2] <= 1)) and t[24, 2] == 1.0                 # the centre sample


def test_library_constants_equal_the_specification(native):
    w, t = native.sift_window(), native.sift_taps()
    assert w.dtype == np.float32 and w.shape == (49, 8) and t.dtype == np.float32 and t.shape == (13,)
    assert ulp_diff_f32(w, S.window_f64().astype(np.float32)).max() <= 1
    assert ulp_diff_f32(t, S.taps_f64().astype(np.float32)).max() <= 1
    assert abs(t.sum(dtype=np.float64) - 1) <= 1e-6 and np.array_equal(t, t[::-1]) and np.all(t > 0)
    assert native.lib().apap_sift_window(None) == native.ERR_INVALID_ARG and native.lib().apap_sift_taps(None) == native.ERR_INVALID_ARG
    header = open(os.path.join(ROOT, "include", "apap_hip.h")).read()
    for name in ("DIM", "SAMPLES", "TAPS", "PATCH", "WINDOW_COLS", "BLOCK_KEYPOINTS"):
        assert f"#define APAP_SIFT_{name} {getattr(native, 'SIFT_' + name)}" in header
    assert (native.SIFT_DIM, native.SIFT_SAMPLES, native.SIFT_TAPS, native.SIFT_PATCH) == (S.DIM, S.SAMPLES, S.TAPS, S.PATCH) == \
        (native.MATCH_DIM, 49, 13, 21)


def test_atan2_within_2e_6_rad():
    """The float32 atan2 of the specification (the kernel's, restated) against math.atan2 of the same float32 arguments."""
    worst = 0.0
    ang = np.arange(2 ** 16) * (2 * np.pi / 2 ** 16)
    for m in (1e-3, 1.0, 255.0):
        y, x = (m * np.sin(ang)).astype(np.float32), (m * np.cos(ang)).astype(np.float32)
        err = np.abs(S.atan2_rad32(y, x).astype(np.float64) - np.arctan2(y.astype(np.float64), x.astype(np.float64)))
        err = np.minimum(err, 2 * np.pi - err)         # -pi and pi are one angle
        worst = max(worst, float(err.max()))
    print("atan2: worst error on the sweeps", worst, "rad")
    assert worst <= 2e-6
    for y, x in ((0, 1), (1, 0), (0, -1), (-1, 0), (0, 255), (-1e-3, 0), (3, 3), (-3, 3), (3, -3), (-3, -3)):
        got = float(S.atan2_rad32(np.float32([y]), np.float32([x]))[0])
        assert abs(got - math.atan2(y, x)) <= 2e-6, (y, x, got)
    assert float(S.atan2_rad32(np.float32([0]), np.float32([0]))[0]) == 0.0          # defined: atan2(0, 0) = 0
    assert float(S.atan2_deg32(np.float32([0]), np.float32([0]))[0]) == 0.0
    deg = S.atan2_deg32(np.float32([0, 1, 0, -1, -1e-9]), np.float32([1, 0, -1, 0, 1]))
    assert np.all((deg >= 0) & (deg <= 360)) and abs(deg[1] - 90) < 1e-4 and abs(deg[2] - 180) < 1e-4 and abs(deg[3] - 270) < 1e-4


@pytest.mark.parametrize("shape", [(7, 7), (9, 40), (37, 53)], ids=str)
def test_patch_local_blur_equals_full_image_blur(shape):
    """At every pixel, borders included: the 9 x 9 base patch made from the 21 x 21 grey patch alone, at its centre and at the
    four neighbours a valid sample's differences read, equals the whole image's blur bit for bit."""
    h, w = shape
    rng = np.random.default_rng(h * 100 + w)
    g = rng.integers(0, 256, (h, w)).astype(np.uint8)
    taps = S.taps_f64().astype(np.float32)
    full = S.blur_full(g, taps)
    assert full.dtype == np.float32
    yy, xx = (a.ravel() for a in np.mgrid[:h, :w])
    local = S.blur_patch(g, yy, xx, taps)
    assert local[:, 4, 4].tobytes() == full[yy, xx].tobytes()
    for dy, dx in ((0, 1), (0, -1), (1, 0), (-1, 0), (3, 4), (-4, -3), (4, 4), (-4, -4)):
        ok = (yy + dy >= 0) & (yy + dy < h) & (xx + dx >= 0) & (xx + dx < w)
        assert local[ok, 4 + dy, 4 + dx].tobytes() == full[yy[ok] + dy, xx[ok] + dx].tobytes(), (dy, dx)
    # and the descriptors of the two routes, a keypoint on every pixel
    pts = np.stack([xx, yy], -1).astype(np.float32)
    assert S.describe(g, pts).tobytes() == S.describe(g, pts, local=True).tobytes()


def test_float32_against_the_float64_definition(native):
    img = scene()
    h, w = img.shape[:2]
    rng = np.random.default_rng(1)
    pts = np.concatenate([rng.uniform(-2, [w + 2, h + 2], (400, 2)),
                          [[0, 0], [w - 1, 0], [0, h - 1], [w - 1, h - 1], [10.5, 20.5], [11.5, 21.5], [64.5, 48.5], [-0.5, 3.5]]])
    pts = pts.astype(np.float32)
    f32 = S.describe(img, pts, native.sift_taps(), native.sift_window())
    f64 = S.describe64(img, pts)
    assert f32.dtype == np.float32 and f32.shape == (408, 128) and not np.isnan(f32).any()
    assert np.array_equal(f32, np.rint(f32)) and f32.min() >= 0 and f32.max() <= 255
    d = np.abs(f32 - f64)
    share = float(np.count_nonzero(d)) / d.size
    print("float32 against float64: max difference", float(d.max()), "share of differing values", share)
    assert d.max() <= 1 and share <= 1e-3
    assert np.count_nonzero(f32.any(axis=1)) >= 390                   # a real input: nearly every keypoint has a descriptor
    norms = np.linalg.norm(f32[f32.any(axis=1)], axis=1)
    assert np.all(norms <= 512 + 0.5 * np.sqrt(128)), norms.max()     # scaled to 512; 128 roundings of at most 0.5 each
    # grey input equals the BGR input's own grey plane, and the two routes to the base image agree
    assert S.describe(S.grey(img), pts).tobytes() == S.describe(img, pts).tobytes() == S.describe(img, pts, local=True).tobytes()
    # half coordinates round to even
    assert S.describe(img, np.float32([[10.5, 20.5], [11.5, 21.5]])).tobytes() == S.describe(img, np.float32([[10, 20], [12, 22]])).tobytes()


def test_invalid_arguments_are_refused_before_any_device_is_touched(native):
    """ERR_INVALID_ARG also on a machine without a GPU (there the next check would answer ERR_NO_DEVICE), and device 1 << 20
    cannot exist: an argument error means the device was not looked at."""
    lib = native.lib()
    img = np.zeros((9, 8, 3), np.uint8)
    pts = np.ones((4, 2), np.float32)
    out = np.zeros((4, 128), np.float32)
    f, u8, far = C.c_float, C.c_uint8, 1 << 20
    host = lib.apap_sift_describe
    good = [None, p(img, u8), 9, 8, 3, p(pts, f), 4, p(out, f), far]
    assert host(*good) == native.ERR_NO_DEVICE        # valid arguments: only now is the device looked at
    nan, inf = pts.copy(), pts.copy()
    nan[3, 1], inf[0, 0] = np.nan, -np.inf
    for at, bad in ((1, None), (5, None), (7, None), (2, 6), (3, 6), (2, 32769), (3, 32769), (2, -1), (4, 2), (4, 4), (4, 0), (6, 0),
                    (6, -1), (6, (1 << 24) + 1), (5, p(nan, f)), (5, p(inf, f))):
        args = list(good)
        args[at] = bad
        assert host(*args) == native.ERR_INVALID_ARG, (at, bad)
        assert "apap_sift_describe" in native.last_error()
    batch = lib.apap_sift_describe_batch
    ptrs = (C.c_void_p * 2)(img.ctypes.data, img.ctypes.data)
    hs, ws, cs, off = i32(9, 8), i32(8, 9), i32(3, 1), i32(0, 1, 4)
    good = [None, ptrs, p(hs), p(ws), p(cs), 2, p(pts, f), p(off), p(out, f), far]
    assert batch(*good) == native.ERR_NO_DEVICE
    for at, bad in ((1, None), (2, None), (3, None), (4, None), (6, None), (7, None), (8, None), (5, 0), (5, 65536), (7, p(i32(0, 4, 4))),
                    (7, p(i32(2, 1, 4))), (7, p(i32(-1, 1, 4))), (2, p(i32(9, 6))), (3, p(i32(32769, 9))), (4, p(i32(3, 2))),
                    (1, (C.c_void_p * 2)(img.ctypes.data, None)), (6, p(nan, f))):
        args = list(good)
        args[at] = bad
        assert batch(*args) == native.ERR_INVALID_ARG, (at, bad)
    # the resident forms: pointers are only compared and counted here, never followed
    fake, work = 1 << 20, 1 << 20
    assert lib.apap_sift_workspace_bytes(1) == 256 and lib.apap_sift_workspace_bytes(9) == 512 and lib.apap_sift_workspace_bytes(65535) == -(-65535 * 32 // 256) * 256
    assert lib.apap_sift_workspace_bytes(0) == 0 and lib.apap_sift_workspace_bytes(65536) == 0 and lib.apap_sift_workspace_bytes(-1) == 0
    dev = lib.apap_sift_describe_device
    good = [None, fake, 9, 8, 3, fake, 4, fake, work, 256, None]
    for at, bad, code in ((1, None, native.ERR_INVALID_ARG), (5, None, native.ERR_INVALID_ARG), (7, None, native.ERR_INVALID_ARG),
                          (8, None, native.ERR_INVALID_ARG), (2, 6, native.ERR_INVALID_ARG), (4, 2, native.ERR_INVALID_ARG),
                          (6, 0, native.ERR_INVALID_ARG), (9, 255, native.ERR_WORKSPACE), (9, 0, native.ERR_WORKSPACE),
                          (8, work + 128, native.ERR_INVALID_ARG), (5, fake + 4, native.ERR_INVALID_ARG)):
        args = list(good)
        args[at] = bad
        assert dev(*args) == code, (at, bad)
    bdev = lib.apap_sift_describe_batch_device
    fakes = (C.c_void_p * 2)(fake, fake)
    good = [None, fakes, p(hs), p(ws), p(cs), 2, fake, p(off), fake, work, 256, None]
    for at, bad, code in ((1, None, native.ERR_INVALID_ARG), (1, (C.c_void_p * 2)(fake, None), native.ERR_INVALID_ARG),
                          (6, None, native.ERR_INVALID_ARG), (7, p(i32(0, 2, 2)), native.ERR_INVALID_ARG), (5, 0, native.ERR_INVALID_ARG),
                          (10, 0, native.ERR_WORKSPACE), (9, work + 16, native.ERR_INVALID_ARG)):
        args = list(good)
        args[at] = bad
        assert bdev(*args) == code, (at, bad)


def test_python_wrappers_refuse_bad_input(native):
    from cvx_proj_amd import features
    z = np.zeros
    ok_img, ok_pts = z((9, 9), np.uint8), z((3, 2))
    bad = [(z((9, 9), np.float32), ok_pts), (z((9, 9), np.int16), ok_pts), (z((9, 9, 2), np.uint8), ok_pts), (z((9, 9, 4), np.uint8), ok_pts),
           (z((9,), np.uint8), ok_pts), (z((2, 9, 9, 3), np.uint8), ok_pts), (z((6, 9), np.uint8), ok_pts), (z((9, 6, 3), np.uint8), ok_pts),
           (z((32769, 7), np.uint8), ok_pts), (ok_img, z((3, 3))), (ok_img, z((6,))), (ok_img, z((0, 2))),
           (ok_img, np.array([[1.0, np.nan]])), (ok_img, np.array([[np.inf, 1.0]]))]
    for img, pts in bad:
        with pytest.raises(ValueError):
            native.sift_describe(img, pts)
    for img, pts in bad[:9] + bad[11:]:
        with pytest.raises(ValueError):
            features.compute(img, pts)
    with pytest.raises(ValueError):
        native.sift_describe_batch([ok_img, ok_img], z((4, 2)), [1, 2])          # the counts do not sum to the rows
    with pytest.raises(ValueError):
        native.sift_describe_batch([ok_img, ok_img], z((4, 2)), [4, 0])
    with pytest.raises(ValueError):
        native.sift_describe_batch([ok_img], z((4, 2)), [2, 2])
    with pytest.raises(ValueError):
        native.sift_describe_batch([], z((4, 2)), [])
    with pytest.raises(ValueError):
        native.sift_describe_batch([ok_img, z((9, 9), np.float64)], z((4, 2)), [2, 2])
    with pytest.raises(ValueError):
        features.coarse_matching(ok_img, z((5, 9), np.uint8), ok_pts, ok_pts)
    assert native.as_sift_points(np.arange(6).reshape(3, 2)).dtype == np.float32
    assert native.as_sift_image(z((7, 8, 1), np.uint8))[1] == 1 and native.as_sift_image(z((7, 8, 3), np.uint8))[1] == 3


def test_no_device_no_fallback(native):
    if native.lib().apap_device_count() > 0:
        pytest.skip("a GPU is visible")
    from cvx_proj_amd import features
    img, pts = scene(20, 24), np.array([[5.0, 6.0], [10.0, 11.0]])
    with pytest.raises(native.ApapError) as e:
        features.compute(img, pts)
    assert e.value.code == native.ERR_NO_DEVICE
    with pytest.raises(native.ApapError) as e:
        native.sift_describe_batch([img, img[:, :, 0]], np.concatenate([pts, pts]), [2, 2])
    assert e.value.code == native.ERR_NO_DEVICE
    for fn in (features.coarse_matching, features.matched_arrays):
        with pytest.raises(native.ApapError) as e:
            fn(img, img, pts, pts, ratio=0.8)
        assert e.value.code == native.ERR_NO_DEVICE


def test_features_imports_without_torch_scipy_and_cv2():
    code = ("import sys; import cvx_proj_amd.features as F; from cvx_proj_amd import _native; _native.lib(); "
            "_native.sift_window(); _native.sift_taps(); "
            "assert 'torch' not in sys.modules, 'torch was imported'; assert 'scipy' not in sys.modules, 'scipy was imported'; "
            "assert 'cv2' not in sys.modules; print(sorted(F.__all__))")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-1500:]
    assert r.stdout.strip() == str(sorted(["compute", "describe_pair", "coarse_matching", "matched_arrays"]))
