"""The image pyramid's host side, without a GPU: every argument rule with its message, APAP_ERR_NO_DEVICE, the layout and the
corner budget against the specification, the Python signatures, and that ``levels=None`` reaches no new symbol."""
import ctypes as C
import inspect
import os
import subprocess
import sys

import numpy as np
import pytest

import pyramid_spec as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def p(a, t=C.c_int):
    return a.ctypes.data_as(C.POINTER(t))


def i32(*v):
    return np.array(v, np.int32)


def refused(native, fn, good, at, bad, code, words):
    args = list(good)
    args[at] = bad
    assert fn(*args) == code, (at, bad)
    msg = native.last_error()
    assert all(w in msg for w in words), (at, bad, msg)


def test_layout_equals_the_specification(native):
    lib = native.lib()
    hs, ws, num, shift = (np.zeros(16, np.int32) for _ in range(4))
    off = np.zeros(17, np.int64)
    for side in list(range(32, 301)) + [32768]:
        for other in (side, 32, 32768 if side == 32768 else side + 37):
            for half in (0, 1):
                for n_levels in (1, 2, 3, 6, 16):
                    n = lib.apap_pyramid_layout(side, other, n_levels, half, p(hs), p(ws), p(off, C.c_longlong), p(num), p(shift))
                    want = P.layout(side, other, n_levels, bool(half))
                    got = (hs[:n].tolist(), ws[:n].tolist(), off[:n + 1].tolist(), num[:n].tolist(), shift[:n].tolist())
                    assert n == len(want[0]) >= 1 and got == tuple(want), (side, other, half, n_levels)
                    assert all(o % 256 == 0 for o in got[2]) and min(got[0] + got[1]) >= 32
                    assert got[0] == sorted(got[0], reverse=True) and got[1] == sorted(got[1], reverse=True)     # sizes fall
    assert lib.apap_pyramid_layout(100, 100, 6, 1, None, None, None, None, None) == 4                  # every output is optional
    assert lib.apap_pyramid_layout(32768, 32768, 16, 1, None, None, None, None, None) == 16
    for h, w, n, words in ((31, 100, 6, ("31 x 100", "32 .. 32768")), (100, 32769, 6, ("100 x 32769",)), (100, 100, 0, ("n_levels = 0",)),
                           (100, 100, 17, ("n_levels = 17", "1 .. 16"))):
        assert lib.apap_pyramid_layout(h, w, n, 1, None, None, None, None, None) == 0
        assert "apap_pyramid_layout" in native.last_error() and all(x in native.last_error() for x in words)
    a = native.pyramid_layout(200, 260)
    assert [x.dtype for x in a] == [np.int32, np.int32, np.int64, np.int32, np.int32] and a[0].tolist() == [200, 150, 100, 75, 50, 38]
    with pytest.raises(ValueError):
        native.pyramid_layout(31, 100)
    with pytest.raises(ValueError):
        native.pyramid_layout(100, 100, 17)


def test_level_caps_equal_the_specification(native):
    lib = native.lib()
    caps = np.zeros(16, np.int32)
    for mc in list(range(1, 301)) + [600, 2000, 32768, 10 ** 6, 2 ** 31 - 1]:
        for half in (0, 1):
            for n_levels in (1, 6, 16):
                assert lib.apap_pyramid_level_caps(mc, n_levels, half, p(caps)) == native.OK
                assert caps[:n_levels].tolist() == P.level_caps(mc, n_levels, bool(half)), (mc, half, n_levels)
    for args, words in (((0, 6, 1, p(caps)), ("max_corners = 0",)), ((10, 0, 1, p(caps)), ("n_levels = 0",)),
                        ((10, 17, 1, p(caps)), ("n_levels = 17",)), ((10, 6, 1, None), ("null",))):
        assert lib.apap_pyramid_level_caps(*args) == native.ERR_INVALID_ARG
        assert "apap_pyramid_level_caps" in native.last_error() and all(w in native.last_error() for w in words)
    assert native.pyramid_level_caps(600).tolist() == [600, 337, 150, 84, 37, 21]


def test_argument_rules_of_the_build(native):
    lib = native.lib()
    bad_arg, short = native.ERR_INVALID_ARG, native.ERR_WORKSPACE
    img, out = np.zeros(40 * 50 * 3, np.uint8), np.zeros(1 << 16, np.uint8)
    u8, far = C.c_uint8, 1 << 20
    host = lib.apap_pyramid_build
    good = [None, p(img, u8), 40, 50, 3, 6, 1, p(out, u8), far]
    assert host(*good) == native.ERR_NO_DEVICE           # valid arguments: only now is the device (number 2^20) looked at
    who = "apap_pyramid_build_batch"                    # the single call is the batch of one
    for at, bad, words in ((1, None, ("null",)), (7, None, ("null",)), (2, 31, ("31 x 50", "32 .. 32768")), (3, 31, ("40 x 31",)),
                           (2, 32769, ("32769 x 50",)), (3, -1, ("40 x -1",)), (4, 2, ("2 channels",)), (4, 0, ("0 channels",)),
                           (4, 4, ("4 channels",)), (5, 0, ("n_levels = 0", "1 .. 16")), (5, 17, ("n_levels = 17",)), (5, -1, ("n_levels = -1",))):
        refused(native, host, good, at, bad, bad_arg, (who,) + words)
    for at, ok in ((2, 32), (3, 32), (5, 1), (5, 16), (4, 1), (6, 0), (6, 7)):      # the limits themselves pass
        args = list(good)
        args[at] = ok
        assert host(*args) == native.ERR_NO_DEVICE, (at, ok)
    batch = lib.apap_pyramid_build_batch
    ptrs = (C.c_void_p * 2)(img.ctypes.data, img.ctypes.data)
    hs, ws, cs = i32(40, 50), i32(50, 40), i32(3, 1)
    good = [None, ptrs, p(hs), p(ws), p(cs), 2, 6, 1, p(out, u8), far]
    assert batch(*good) == native.ERR_NO_DEVICE
    for at, bad, words in ((1, None, ("null",)), (2, None, ("null",)), (3, None, ("null",)), (4, None, ("null",)), (8, None, ("null",)),
                           (5, 0, ("n_images = 0", "1 .. 65535")), (5, 65536, ("n_images = 65536",)), (5, -1, ("n_images = -1",)),
                           (2, p(i32(40, 31)), ("image 1 is 31 x 40",)), (3, p(i32(32769, 40)), ("image 0 is 40 x 32769",)),
                           (4, p(i32(3, 2)), ("image 1 has 2 channels",)), (1, (C.c_void_p * 2)(img.ctypes.data, None), ("image 1: null",))):
        refused(native, batch, good, at, bad, bad_arg, (who,) + words)

    # the resident forms: pointers are only compared and counted here, never followed
    fake, work = 1 << 20, 1 << 21
    need = lib.apap_pyramid_workspace_bytes(1, 6)
    assert need == 512 and lib.apap_pyramid_workspace_bytes(2, 6) == 768 and lib.apap_pyramid_workspace_bytes(1, 16) == 1024
    assert [lib.apap_pyramid_workspace_bytes(*a) for a in ((0, 6), (65536, 6), (1, 0), (1, 17))] == [0, 0, 0, 0]
    total = int(native.pyramid_layout(40, 50, 6, True)[2][-1])
    dev = lib.apap_pyramid_build_device
    who = "apap_pyramid_build_batch_device"
    good = [None, fake, 40, 50, 3, 6, 1, fake, total, work, need, None]
    for at, bad, code, words in ((1, None, bad_arg, ("null device pointer",)), (7, None, bad_arg, ("null device pointer",)),
                                 (9, None, bad_arg, ("null device pointer",)), (2, 31, bad_arg, ("31 x 50",)), (4, 2, bad_arg, ("2 channels",)),
                                 (5, 17, bad_arg, ("n_levels = 17",)), (10, need - 1, short, ("workspace 511 < 512",)),
                                 (10, 0, short, ("workspace 0 < 512",)), (8, total - 1, short, ("level buffer",)),
                                 (9, work + 128, bad_arg, ("256-byte aligned",)), (7, fake + 64, bad_arg, ("256-byte aligned",))):
        refused(native, dev, good, at, bad, code, (who,) + words)
    bdev = lib.apap_pyramid_build_batch_device
    fakes = (C.c_void_p * 2)(fake, fake)
    need2 = lib.apap_pyramid_workspace_bytes(2, 6)
    total2 = int(native.pyramid_layout(40, 50, 6, True)[2][-1]) + int(native.pyramid_layout(50, 40, 6, True)[2][-1])
    good = [None, fakes, p(hs), p(ws), p(cs), 2, 6, 1, fake, total2, work, need2, None]
    for at, bad, code, words in ((1, None, bad_arg, ("null device pointer",)), (1, (C.c_void_p * 2)(fake, None), bad_arg, ("image 1: null",)),
                                 (5, 0, bad_arg, ("n_images = 0",)), (11, need2 - 1, short, ("workspace",)), (9, total2 - 1, short, ("level buffer",)),
                                 (10, work + 16, bad_arg, ("256-byte aligned",))):
        refused(native, bdev, good, at, bad, code, (who,) + words)


def test_argument_rules_of_the_pack(native):
    lib = native.lib()
    bad_arg, short = native.ERR_INVALID_ARG, native.ERR_WORKSPACE
    f, ll, far = C.c_float, C.c_longlong, 1 << 20
    spts, sresp = np.zeros((2, 8, 2), np.float32), np.zeros((2, 8), np.int64)
    pts, lpts, level, resp, off = np.zeros((16, 2), np.float32), np.zeros((16, 2), np.float32), np.zeros(16, np.int32), np.zeros(16, np.int64), np.zeros(3, np.int32)
    counts, num, shift, index = i32(8, 0), i32(1, 3), i32(0, 2), i32(0, 1)
    host = lib.apap_pyramid_keypoints
    who = "apap_pyramid_keypoints"
    good = [None, p(spts, f), p(sresp, ll), 8, p(counts), p(num), p(shift), p(index), 2, p(pts, f), p(lpts, f), p(level), p(resp, ll), p(off), far]
    assert host(*good) == native.ERR_NO_DEVICE
    for at in (1, 2, 4, 5, 6, 7, 9, 10, 11, 12, 13):
        refused(native, host, good, at, None, bad_arg, (who, "null"))
    for at, bad, words in ((3, 0, ("slab_rows = 0",)), (8, 0, ("n_level_images = 0", "1 .. 65535")), (8, 65536, ("n_level_images = 65536",)),
                           (4, p(i32(8, 9)), ("level image 1: count 9", "slab_rows = 8")), (4, p(i32(-1, 0)), ("level image 0: count -1",)),
                           (5, p(i32(1, 2)), ("level image 1: scale 2",)), (6, p(i32(0, 19)), ("level image 1: scale 3 / 2^19",)),
                           (6, p(i32(-1, 2)), ("level image 0",))):
        refused(native, host, good, at, bad, bad_arg, (who,) + words)
    fake, work = 1 << 20, 1 << 21
    need = lib.apap_pyramid_keypoints_workspace_bytes(2)
    assert need == 256 and lib.apap_pyramid_keypoints_workspace_bytes(17) == 512
    assert lib.apap_pyramid_keypoints_workspace_bytes(0) == 0 and lib.apap_pyramid_keypoints_workspace_bytes(65536) == 0
    dev = lib.apap_pyramid_keypoints_device
    who = "apap_pyramid_keypoints_device"
    good = [None, fake, fake, 8, p(counts), p(num), p(shift), p(index), 2, fake, fake, fake, fake, p(off), work, need, None]
    for at in (1, 2, 9, 10, 11, 12, 14):
        refused(native, dev, good, at, None, bad_arg, (who, "null device pointer"))
    refused(native, dev, good, 13, None, bad_arg, (who, "null level_offset"))
    for at, bad, code, words in ((15, need - 1, short, ("workspace 255 < 256",)), (14, work + 128, bad_arg, ("256-byte",)),
                                 (1, fake + 4, bad_arg, ("8-byte",)), (12, fake + 4, bad_arg, ("8-byte",)), (11, fake + 2, bad_arg, ("4-byte",)),
                                 (4, p(i32(9, 0)), bad_arg, ("count 9",))):
        refused(native, dev, good, at, bad, code, (who,) + words)


def test_python_wrappers_refuse_bad_input(native):
    from cvx_proj_amd import features
    z = np.zeros
    ok = z((40, 40), np.uint8)
    for img in (z((40, 40), np.float32), z((40, 40, 2), np.uint8), z((40,), np.uint8), z((31, 40), np.uint8), z((40, 32769), np.uint8)):
        for fn in (lambda: native.pyramid(img), lambda: features.pyramid(img), lambda: features.detect(img, levels=6),
                   lambda: features.detect_pair(ok, img, levels=6), lambda: features.detect_and_describe(img)):
            with pytest.raises(ValueError):
                fn()
    for levels in (0, 17, -1):
        for fn in (lambda: features.pyramid(ok, levels=levels), lambda: features.detect(ok, levels=levels),
                   lambda: features.detect_and_match(ok, ok, levels=levels), lambda: features.detect_and_describe(ok, levels=levels)):
            with pytest.raises(ValueError):
                fn()
    with pytest.raises(ValueError):
        native.pyramid_batch([])
    with pytest.raises(ValueError):
        native.pyramid_keypoints(z((2, 4, 2), np.float32), z((2, 4), np.int64), [5, 0], [1, 3], [0, 2], [0, 1])      # a count beyond the slab
    with pytest.raises(ValueError):
        native.pyramid_keypoints(z((2, 4, 2), np.float32), z((2, 5), np.int64), [4, 0], [1, 3], [0, 2], [0, 1])


def test_python_signatures(native):
    from cvx_proj_amd import features

    def defaults(fn):
        return {k: v.default for k, v in inspect.signature(fn).parameters.items() if v.default is not inspect.Parameter.empty}
    assert defaults(native.pyramid) == {"n_levels": 6, "half_steps": True, "device": -1, "ctx": None}
    assert defaults(features.pyramid) == {"levels": 6, "half_steps": True, "device": -1, "ctx": None}
    for fn in (features.detect, features.detect_pair, features.detect_and_match, features.matched_arrays_from_images):
        d = defaults(fn)
        assert d["levels"] is None and d["half_steps"] is True and d["max_corners"] == 2000, fn.__name__      # opt-in: today's call by default
    d = defaults(features.detect_and_describe)
    assert (d["levels"], d["oriented"], d["max_corners"], d["radius"], d["quality"]) == (6, False, 2000, 5, 0.01)
    assert callable(native.pyramid_layout) and callable(native.pyramid_keypoints) and callable(native.pyramid_level_caps)
    header = open(ROOT + "/include/apap_hip.h").read()
    for name, value in (("MAX_LEVELS", native.PYRAMID_MAX_LEVELS), ("MIN_SIDE", native.PYRAMID_MIN_SIDE), ("TILE_W", native.PYRAMID_TILE_W),
                        ("TILE_H", native.PYRAMID_TILE_H)):
        assert f"#define APAP_PYRAMID_{name} {value}" in header
    assert (P.MAX_LEVELS, P.MIN_SIDE) == (native.PYRAMID_MAX_LEVELS, native.PYRAMID_MIN_SIDE)


def test_levels_none_reaches_no_new_symbol(native, monkeypatch):
    """The default call of the four functions is today's code path: no pyramid function of the binding is entered before the
    library refuses (here, without a GPU) or answers."""
    from cvx_proj_amd import features
    entered = []
    for name in ("pyramid", "pyramid_batch", "pyramid_layout", "pyramid_level_caps", "pyramid_keypoints", "pyramid_levels_arg"):
        monkeypatch.setattr(native, name, lambda *a, _n=name, **k: entered.append(_n) or (_ for _ in ()).throw(AssertionError(_n)))
    img = np.zeros((40, 40), np.uint8)
    img[10:30, 10:30] = 200
    for fn in (lambda: features.detect(img), lambda: features.detect_pair(img, img), lambda: features.detect_and_match(img, img),
               lambda: features.matched_arrays_from_images(img, img), lambda: features.detect_and_describe(img, levels=None)):
        try:
            fn()
        except native.ApapError as e:
            assert e.code == native.ERR_NO_DEVICE
    assert entered == []
    with pytest.raises(AssertionError):
        features.detect(img, levels=6)
    assert entered == ["pyramid_levels_arg"]


def test_no_device_no_fallback(native):
    if native.lib().apap_device_count() > 0:
        pytest.skip("a GPU is visible")
    from cvx_proj_amd import features
    img = np.zeros((40, 48), np.uint8)
    for fn in (lambda: features.pyramid(img), lambda: features.detect(img, levels=6), lambda: features.detect_pair(img, img, levels=3),
               lambda: features.detect_and_match(img, img, levels=6), lambda: features.matched_arrays_from_images(img, img, levels=6, ratio=0.8),
               lambda: features.detect_and_describe(img), lambda: native.pyramid_batch([img, np.stack([img] * 3, -1)]),
               lambda: native.pyramid_keypoints(np.zeros((1, 4, 2), np.float32), np.zeros((1, 4), np.int64), [2], [1], [0], [0])):
        with pytest.raises(native.ApapError) as e:
            fn()
        assert e.value.code == native.ERR_NO_DEVICE


def test_features_still_imports_without_torch_scipy_and_cv2():
    code = ("import sys; import cvx_proj_amd.features as F; from cvx_proj_amd import _native; _native.lib(); "
            "assert all(callable(getattr(F, n)) for n in ('pyramid', 'detect_and_describe')); "
            "assert _native.pyramid_layout(64, 64)[0].tolist() == [64, 48, 32]; "
            "assert 'torch' not in sys.modules, 'torch was imported'; assert 'scipy' not in sys.modules; assert 'cv2' not in sys.modules; print('ok')")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stderr[-1500:]
