"""Corner detection without a GPU: the specification's own consistency (tests/corner_spec.py) against a float64 restatement
and its stated properties, argument refusals before any device is touched, the no-device error and the workspace size."""
import ctypes as C
import subprocess
import sys

import numpy as np
import pytest

import corner_spec as S
from conftest import ROOT


def i32(*v):
    return np.array(v, np.int32)


def p(a, t=C.c_int):
    return a.ctypes.data_as(C.POINTER(t))


def rectangle():
    g = np.full((64, 80), 40, np.uint8)
    g[20:44, 24:50] = 200
    return g


def edge():
    g = np.full((40, 60), 40, np.uint8)
    g[:, 30:] = 200
    return g


def shifted_crops(radius, h=150, w=200, dx=7, dy=11):
    """Two crops of one scene, o(y, x) = c(y + dy, x + dx), and the test of a corner (x, y) of c for lying at least
    radius + 2 from every border in both crops."""
    world = S.prototype_scene()
    c_img, o_img = np.ascontiguousarray(world[:h, :w]), np.ascontiguousarray(world[dy:dy + h, dx:dx + w])
    m = radius + 2

    def inner(pts_c):
        pts_o = pts_c - [dx, dy]
        return np.all((pts_c >= m) & (pts_c <= [w - 1 - m, h - 1 - m]) & (pts_o >= m) & (pts_o <= [w - 1 - m, h - 1 - m]), axis=1)
    return c_img, o_img, inner, (dx, dy)


def response_f64(g):
    """Harris's det - 0.04 tr^2 from float Sobel and box sums, written independently of the specification: numpy's own
    reflect padding (reflect-101) and float64 throughout.  Returns it with the sum of the magnitudes of its terms."""
    g = np.pad(g.astype(np.float64), 1, mode="reflect")
    ix = (g[:-2, 2:] + 2 * g[1:-1, 2:] + g[2:, 2:]) - (g[:-2, :-2] + 2 * g[1:-1, :-2] + g[2:, :-2])
    iy = (g[2:, :-2] + 2 * g[2:, 1:-1] + g[2:, 2:]) - (g[:-2, :-2] + 2 * g[:-2, 1:-1] + g[:-2, 2:])

    def box(a):
        a = np.pad(a, 1, mode="reflect")
        h, w = a.shape[0] - 2, a.shape[1] - 2
        return sum(a[dy:dy + h, dx:dx + w] for dy in range(3) for dx in range(3))
    a, b, c = box(ix * ix), box(ix * iy), box(iy * iy)
    return a * c - b * b - 0.04 * (a + c) ** 2, a * c + b * b + 0.04 * (a + c) ** 2


@pytest.mark.parametrize("shape", [(7, 7), (9, 40), (37, 53), (37, 53, 3)], ids=str)
def test_specification_against_float64(shape):
    """R = 25 (det - 0.04 tr^2) up to float64 rounding: a handful of roundings, each at most 2^-53 of the sum of the terms'
    magnitudes (0.04 itself is rounded), so 64 x 2^-53 of that sum bounds the difference.  Beyond it the signs agree, and so does
    the order of any two responses further apart than twice the largest bound."""
    rng = np.random.default_rng(sum(shape))
    img = rng.integers(0, 256, shape).astype(np.uint8)
    R = S.response(img)
    Rf, mag = response_f64(S.grey(img))
    tol = 25 * 64 * 2.0 ** -53 * mag
    assert R.dtype == np.int64 and R.shape == shape[:2]
    assert np.all(np.abs(25 * Rf - R.astype(np.float64)) <= tol + 1)          # + 1: R itself rounds when cast to float64 above 2^53
    sure = np.abs(R) > tol + 1
    assert sure.mean() > 0.99 and np.array_equal(np.sign(Rf[sure]), np.sign(R[sure]))
    order = np.argsort(R, axis=None, kind="stable")
    r, rf = R.ravel()[order], Rf.ravel()[order]
    apart = np.diff(r) > 2 * (tol.max() + 1)
    assert apart.sum() > 0.5 * r.size and np.all(np.diff(rf)[apart] > 0)
    assert (R > 0).any() and (R < 0).any()


def test_bgr_uses_the_descriptors_grey():
    import sift_spec
    img = np.random.default_rng(0).integers(0, 256, (20, 30, 3)).astype(np.uint8)
    assert np.array_equal(S.grey(img), sift_spec.grey(img))
    assert np.array_equal(S.response(img), S.response(S.grey(img).astype(np.uint8)))


@pytest.mark.parametrize("radius", [1, 5, 16])
def test_corner_count_is_bounded_and_corners_are_apart(radius):
    """Also on a periodic image, where equal responses abound: the index orders them."""
    for img in (S.prototype_scene(60, 75, seed=radius), np.random.default_rng(radius).integers(0, 256, (33, 65)).astype(np.uint8),
                np.tile(np.random.default_rng(3).integers(0, 256, (16, 16)).astype(np.uint8), (4, 5))):
        h, w = img.shape
        pts, resp = S.detect(img, h * w, radius, 0)
        assert 0 < len(pts) <= S.bound(h, w, radius)
        d = np.abs(pts[:, None, :] - pts[None, :, :]).max(axis=2)              # Chebyshev distance of every two corners
        np.fill_diagonal(d, radius + 1)
        assert d.min() > radius
        assert np.all(resp > 0) and np.all(np.diff(resp) <= 0)
        idx = pts[:, 1].astype(np.int64) * w + pts[:, 0].astype(np.int64)
        tie = np.diff(resp) == 0
        assert np.all(np.diff(idx)[tie] > 0)
    # the last image is periodic; at radius 16 every copy of its strongest pixel has an earlier copy in its window but the first
    assert tie.any() if radius < 16 else len(pts) < 4


def test_rectangle_flat_and_edge():
    pts, resp = S.detect(rectangle(), 100, 5, 10)
    assert sorted(map(tuple, pts.tolist())) == [(24.0, 20.0), (24.0, 43.0), (49.0, 20.0), (49.0, 43.0)]
    assert pts.dtype == np.float32 and resp.dtype == np.int64
    for img in (np.zeros((30, 40), np.uint8), np.full((7, 7, 3), 255, np.uint8), edge(), edge().T.copy()):
        full_pts, full_resp, n = S.detect_full(img, 50, 5, 0)
        assert n == 0 and not full_pts.any() and not full_resp.any() and full_pts.shape == (50, 2)


def test_shift_property():
    radius = 5
    c_img, o_img, inner, (dx, dy) = shifted_crops(radius)
    h, w = c_img.shape
    pc, rc = S.detect(c_img, S.bound(h, w, radius), radius, 0)
    po, ro = S.detect(o_img, S.bound(h, w, radius), radius, 0)
    a = {(x, y, r) for (x, y), r in zip(pc[inner(pc)].tolist(), rc[inner(pc)].tolist())}
    b = {(x + dx, y + dy, r) for (x, y), r in zip(po.tolist(), ro.tolist()) if inner(np.array([[x + dx, y + dy]]))[0]}
    assert a == b and len(a) > 50


def test_prefix_and_quality_properties():
    img = S.prototype_scene()
    h, w = img.shape
    full_pts, full_resp = S.detect(img, S.bound(h, w, 5), 5, 0)
    assert len(full_pts) > 200 and len(full_pts) <= S.bound(h, w, 5)
    for k in (1, 2, 17, len(full_pts) - 1, len(full_pts), len(full_pts) + 5):
        pts, resp, n = S.detect_full(img, k, 5, 0)
        assert n == min(k, len(full_pts)) and np.array_equal(pts[:n], full_pts[:n]) and np.array_equal(resp[:n], full_resp[:n])
        assert not pts[n:].any() and not resp[n:].any()
    for q in (0, 1, 10, 500, 1000):
        pts, resp = S.detect(img, S.bound(h, w, 5), 5, q)
        keep = 1000 * full_resp >= q * full_resp[0]
        assert np.array_equal(pts, full_pts[keep]) and np.array_equal(resp, full_resp[keep]) and len(pts) >= 1
    assert len(S.detect(img, 10 ** 6, 5, 10)[0]) < len(full_pts)


def test_invalid_arguments_are_refused_before_any_device_is_touched(native):
    """ERR_INVALID_ARG also on a machine without a GPU (there the next check would answer ERR_NO_DEVICE), and device 1 << 20
    cannot exist: an argument error means the device was not looked at."""
    lib = native.lib()
    img = np.zeros((9, 8, 3), np.uint8)
    pts, resp, cnt = np.zeros((4, 2), np.float32), np.zeros(4, np.int64), np.zeros(2, np.int32)
    f, u8, ll, far = C.c_float, C.c_uint8, C.c_longlong, 1 << 20
    host = lib.apap_corner_detect
    good = [None, p(img, u8), 9, 8, 3, 4, 5, 10, p(pts, f), p(resp, ll), p(cnt), far]
    assert host(*good) == native.ERR_NO_DEVICE        # valid arguments: only now is the device looked at
    for at, bad in ((1, None), (8, None), (9, None), (10, None), (2, 6), (3, 6), (2, 32769), (3, 32769), (2, -1), (4, 2), (4, 4), (4, 0),
                    (5, 0), (5, -1), (6, 0), (6, 17), (6, -1), (7, -1), (7, 1001)):
        args = list(good)
        args[at] = bad
        assert host(*args) == native.ERR_INVALID_ARG, (at, bad)
        assert "apap_corner_detect" in native.last_error()
    for at, ok in ((2, 7), (3, 7), (2, 32768), (5, 1), (5, 2 ** 31 - 1), (6, 1), (6, 16), (7, 0), (7, 1000)):     # the limits themselves pass
        args = list(good)
        args[at] = ok
        assert host(*args) == native.ERR_NO_DEVICE, (at, ok)
    batch = lib.apap_corner_detect_batch
    ptrs = (C.c_void_p * 2)(img.ctypes.data, img.ctypes.data)
    hs, ws, cs = i32(9, 8), i32(8, 9), i32(3, 1)
    good = [None, ptrs, p(hs), p(ws), p(cs), 2, 2, 5, 10, p(pts, f), p(resp, ll), p(cnt), far]
    assert batch(*good) == native.ERR_NO_DEVICE
    for at, bad in ((1, None), (2, None), (3, None), (4, None), (9, None), (10, None), (11, None), (5, 0), (5, 65536), (5, -1), (6, 0),
                    (7, 0), (7, 17), (8, 1001), (8, -1), (2, p(i32(9, 6))), (3, p(i32(32769, 9))), (4, p(i32(3, 2))),
                    (1, (C.c_void_p * 2)(img.ctypes.data, None))):
        args = list(good)
        args[at] = bad
        assert batch(*args) == native.ERR_INVALID_ARG, (at, bad)
    # the resident forms: pointers are only compared and counted here, never followed
    fake, work = 1 << 20, 1 << 20
    h1, w1 = i32(9), i32(8)
    need = lib.apap_corner_workspace_bytes(p(h1), p(w1), 1, 5)
    dev = lib.apap_corner_detect_device
    good = [None, fake, 9, 8, 3, 4, 5, 10, fake, fake, fake, work, need, None]
    for at, bad, code in ((1, None, native.ERR_INVALID_ARG), (8, None, native.ERR_INVALID_ARG), (9, None, native.ERR_INVALID_ARG),
                          (10, None, native.ERR_INVALID_ARG), (11, None, native.ERR_INVALID_ARG), (2, 6, native.ERR_INVALID_ARG),
                          (4, 2, native.ERR_INVALID_ARG), (5, 0, native.ERR_INVALID_ARG), (6, 17, native.ERR_INVALID_ARG),
                          (7, 1001, native.ERR_INVALID_ARG), (12, need - 1, native.ERR_WORKSPACE), (12, 0, native.ERR_WORKSPACE),
                          (11, work + 128, native.ERR_INVALID_ARG), (8, fake + 4, native.ERR_INVALID_ARG),
                          (9, fake + 4, native.ERR_INVALID_ARG), (10, fake + 2, native.ERR_INVALID_ARG)):
        args = list(good)
        args[at] = bad
        assert dev(*args) == code, (at, bad)
    bdev = lib.apap_corner_detect_batch_device
    fakes = (C.c_void_p * 2)(fake, fake)
    need2 = lib.apap_corner_workspace_bytes(p(hs), p(ws), 2, 5)
    good = [None, fakes, p(hs), p(ws), p(cs), 2, 2, 5, 10, fake, fake, fake, work, need2, None]
    for at, bad, code in ((1, None, native.ERR_INVALID_ARG), (1, (C.c_void_p * 2)(fake, None), native.ERR_INVALID_ARG),
                          (9, None, native.ERR_INVALID_ARG), (5, 0, native.ERR_INVALID_ARG), (13, need2 - 1, native.ERR_WORKSPACE),
                          (12, work + 16, native.ERR_INVALID_ARG)):
        args = list(good)
        args[at] = bad
        assert bdev(*args) == code, (at, bad)


def test_workspace_bytes(native):
    lib = native.lib()

    def ws(shapes, radius):
        hs, ws_ = i32(*[s[0] for s in shapes]), i32(*[s[1] for s in shapes])
        return lib.apap_corner_workspace_bytes(p(hs), p(ws_), len(shapes), radius)
    last = 0
    for side in (7, 8, 9, 31, 32, 33, 64, 65, 100, 1000, 2160, 4096, 32767):
        for radius in (1, 5, 16):
            got = ws([(side, side)], radius)
            assert got > 0 and got % 256 == 0
            # the table and counters, and 16 bytes per possible corner twice (the second rounded up to a power of two)
            cap = S.bound(side, side, radius)
            up = lambda b: -(-b // 256) * 256           # noqa: E731
            assert got == 256 + 256 + up(16 * cap) + up(16 * (1 << (cap - 1).bit_length()))
        assert ws([(side, side)], 5) >= last and ws([(side, side + 1)], 5) >= ws([(side, side)], 5) and ws([(side + 1, side)], 5) >= ws([(side, side)], 5)
        last = ws([(side, side)], 5)
    assert ws([(100, 120), (50, 60)], 5) > ws([(100, 120)], 5)
    assert ws([(6, 9)], 5) == 0 and ws([(9, 32769)], 5) == 0 and ws([(9, 9)], 0) == 0 and ws([(9, 9)], 17) == 0
    assert lib.apap_corner_workspace_bytes(None, None, 1, 5) == 0 and lib.apap_corner_workspace_bytes(p(i32(9)), p(i32(9)), 0, 5) == 0
    assert native.corner_bound(2160, 3840, 5) == 230400 == S.bound(2160, 3840, 5)
    header = open(ROOT + "/include/apap_hip.h").read()
    assert f"#define APAP_CORNER_TILE_W {native.CORNER_TILE_W}" in header and f"#define APAP_CORNER_TILE_H {native.CORNER_TILE_H}" in header
    assert f"#define APAP_CORNER_MAX_RADIUS {native.CORNER_MAX_RADIUS}" in header


def test_python_wrappers_refuse_bad_input(native):
    from cvx_proj_amd import features
    z = np.zeros
    ok = z((9, 9), np.uint8)
    for img in (z((9, 9), np.float32), z((9, 9, 2), np.uint8), z((9,), np.uint8), z((6, 9), np.uint8), z((9, 32769), np.uint8)):
        with pytest.raises(ValueError):
            native.corner_detect(img, 10)
        with pytest.raises(ValueError):
            features.detect(img)
        with pytest.raises(ValueError):
            features.detect_pair(ok, img)
    for kw in ({"max_corners": 0}, {"radius": 0}, {"radius": 17}, {"quality": -0.001}, {"quality": 1.001}):
        with pytest.raises(ValueError):
            features.detect(ok, **kw)
    with pytest.raises(ValueError):
        native.corner_detect_batch([], 10)
    assert features._permille(0.01) == 10 and features._permille(0.0005) == 0 and features._permille(1) == 1000 and features._permille(0.0015) == 2


def test_no_device_no_fallback(native):
    if native.lib().apap_device_count() > 0:
        pytest.skip("a GPU is visible")
    from cvx_proj_amd import features
    img = rectangle()
    for fn in (lambda: features.detect(img), lambda: features.detect_pair(img, img[:, :40]), lambda: features.detect_and_match(img, img),
               lambda: features.matched_arrays_from_images(img, img, ratio=0.8), lambda: native.corner_detect(img, 5),
               lambda: native.corner_detect_batch([img, np.stack([img] * 3, -1)], 5)):
        with pytest.raises(native.ApapError) as e:
            fn()
        assert e.value.code == native.ERR_NO_DEVICE


def test_features_still_imports_without_torch_scipy_and_cv2():
    code = ("import sys; import cvx_proj_amd.features as F; from cvx_proj_amd import _native; _native.lib(); "
            "assert all(callable(getattr(F, n)) for n in ('detect', 'detect_pair', 'detect_and_match', 'matched_arrays_from_images')); "
            "assert 'torch' not in sys.modules, 'torch was imported'; assert 'scipy' not in sys.modules, 'scipy was imported'; "
            "assert 'cv2' not in sys.modules; print('ok')")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stderr[-1500:]
