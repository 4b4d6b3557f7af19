"""The orientation entry points without a GPU: argument refusals before any device is touched, the no-device error, the Python
wrappers' refusals and the ctypes signatures against the header."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from test_sift_host import i32, p

FAR = 1 << 20          # a device that cannot exist: an argument error means that the device was not looked at


def refused(fn, good, cases, native, name):
    for at, bad, *code in cases:
        args = list(good)
        args[at] = bad
        assert fn(*args) == (code[0] if code else native.ERR_INVALID_ARG), (name, at, bad)
        assert name in native.last_error()


def test_host_buffer_forms_refuse_before_any_device_is_touched(native):
    lib, f, u8 = native.lib(), C.c_float, C.c_uint8
    img = np.zeros((13, 14, 3), np.uint8)
    pts = np.ones((4, 2), np.float32)
    angles = np.float32([0, 90, 359.5, 360])
    out = np.zeros((4, 128), np.float32)
    nan, inf = pts.copy(), pts.copy()
    nan[3, 1], inf[0, 0] = np.nan, -np.inf
    sides = [(2, 12), (3, 12), (2, 32769), (3, 32769), (2, -1), (4, 2), (4, 4), (4, 0), (6, 0), (6, -1), (6, (1 << 24) + 1)]
    # apap_sift_orient(ctx, img, h, w, c, pts, n, angles, device)
    good = [None, p(img, u8), 13, 14, 3, p(pts, f), 4, p(angles, f), FAR]
    assert lib.apap_sift_orient(*good) == native.ERR_NO_DEVICE           # valid arguments, sides 13: only now is the device looked at
    refused(lib.apap_sift_orient, good, [(1, None), (5, None), (7, None), (5, p(nan, f)), (5, p(inf, f))] + sides, native, "apap_sift_orient")
    # apap_sift_describe_oriented(ctx, img, h, w, c, pts, n, angles, angles_out, out, device)
    found = np.zeros(4, np.float32)
    given = [None, p(img, u8), 13, 14, 3, p(pts, f), 4, p(angles, f), None, p(out, f), FAR]
    fused = [None, p(img, u8), 13, 14, 3, p(pts, f), 4, None, p(found, f), p(out, f), FAR]
    assert lib.apap_sift_describe_oriented(*given) == native.ERR_NO_DEVICE
    assert lib.apap_sift_describe_oriented(*fused) == native.ERR_NO_DEVICE
    bad_angles = [np.float32(v) for v in ([0, -1, 1, 2], [0, 1, 360.0001, 2], [np.nan, 1, 2, 3], [0, 1, 2, np.inf], [0, -np.inf, 1, 2])]
    refused(lib.apap_sift_describe_oriented, given,
            [(1, None), (5, None), (9, None), (8, p(found, f)), (5, p(nan, f))] + [(7, p(a, f)) for a in bad_angles] + sides,
            native, "apap_sift_describe_oriented")
    refused(lib.apap_sift_describe_oriented, fused, [(8, None), (9, None), (5, p(inf, f))] + sides, native, "apap_sift_describe_oriented")
    # the batches
    ptrs = (C.c_void_p * 2)(img.ctypes.data, img.ctypes.data)
    hs, ws, cs, off = i32(13, 14), i32(14, 13), i32(3, 1), i32(0, 1, 4)
    shape_cases = [(2, None), (3, None), (4, None), (7, None), (5, 0), (5, 65536), (7, p(i32(0, 4, 4))), (7, p(i32(2, 1, 4))),
                   (7, p(i32(-1, 1, 4))), (2, p(i32(13, 12))), (3, p(i32(32769, 13))), (4, p(i32(3, 2))),
                   (1, (C.c_void_p * 2)(img.ctypes.data, None)), (1, None), (6, None), (6, p(nan, f))]
    good = [None, ptrs, p(hs), p(ws), p(cs), 2, p(pts, f), p(off), p(angles, f), FAR]
    assert lib.apap_sift_orient_batch(*good) == native.ERR_NO_DEVICE
    refused(lib.apap_sift_orient_batch, good, shape_cases + [(8, None)], native, "apap_sift_orient_batch")
    good = [None, ptrs, p(hs), p(ws), p(cs), 2, p(pts, f), p(off), p(angles, f), None, p(out, f), FAR]
    assert lib.apap_sift_describe_oriented_batch(*good) == native.ERR_NO_DEVICE
    refused(lib.apap_sift_describe_oriented_batch, good, shape_cases + [(10, None), (9, p(found, f))] + [(8, p(a, f)) for a in bad_angles],
            native, "apap_sift_describe_oriented_batch")
    # only the rows that the offsets address are looked at: a bad angle and a NaN in front of pt_offset[0] pass
    off2, pts2, ang2 = i32(1, 2, 4), pts.copy(), angles.copy()
    pts2[0], ang2[0] = np.nan, -5
    good[6], good[7], good[8] = p(pts2, f), p(off2), p(ang2, f)
    assert lib.apap_sift_describe_oriented_batch(*good) == native.ERR_NO_DEVICE


def test_device_forms_refuse_without_following_a_pointer(native):
    lib = native.lib()
    fake, work = 1 << 20, 1 << 20
    ws = lib.apap_sift_orient_workspace_bytes
    assert ws(1) == 256 and ws(9) == 512 and ws(65535) == -(-65535 * 32 // 256) * 256 and ws(0) == ws(65536) == ws(-1) == 0
    INV, WS = native.ERR_INVALID_ARG, native.ERR_WORKSPACE
    # apap_sift_orient_device(ctx, d_img, h, w, c, d_pts, n, d_angles, d_work, work_bytes, stream)
    good = [None, fake, 13, 13, 3, fake, 4, fake, work, 256, None]
    refused(lib.apap_sift_orient_device, good,
            [(1, None), (5, None), (7, None), (8, None), (2, 12), (3, 12), (4, 2), (6, 0), (9, 255, WS), (9, 0, WS), (8, work + 128),
             (5, fake + 4), (7, fake + 2)], native, "apap_sift_orient")
    # apap_sift_describe_oriented_device(ctx, d_img, h, w, c, d_pts, n, d_angles, d_angles_out, d_out, d_work, work_bytes, stream)
    given = [None, fake, 13, 13, 3, fake, 4, fake, None, fake, work, 256, None]
    fused = [None, fake, 13, 13, 3, fake, 4, None, fake, fake, work, 256, None]
    common = [(1, None), (5, None), (9, None), (10, None), (2, 12), (3, 32769), (4, 4), (6, 0), (11, 255, WS), (11, 0, WS), (10, work + 16),
              (5, fake + 4), (9, fake + 1)]
    refused(lib.apap_sift_describe_oriented_device, given, common + [(8, fake), (7, fake + 2)], native, "apap_sift_describe_oriented")
    refused(lib.apap_sift_describe_oriented_device, fused, common + [(8, None), (8, fake + 2)], native, "apap_sift_describe_oriented")
    hs, wds, cs, off = i32(13, 14), i32(14, 13), i32(3, 1), i32(0, 1, 4)
    fakes = (C.c_void_p * 2)(fake, fake)
    good = [None, fakes, p(hs), p(wds), p(cs), 2, fake, p(off), fake, work, 256, None]
    refused(lib.apap_sift_orient_batch_device, good,
            [(1, None), (1, (C.c_void_p * 2)(fake, None)), (6, None), (8, None), (7, p(i32(0, 2, 2))), (5, 0), (10, 0, WS), (9, work + 16),
             (2, p(i32(13, 12)))], native, "apap_sift_orient_batch_device")
    good = [None, fakes, p(hs), p(wds), p(cs), 2, fake, p(off), None, fake, fake, work, 256, None]
    refused(lib.apap_sift_describe_oriented_batch_device, good,
            [(1, None), (1, (C.c_void_p * 2)(fake, None)), (6, None), (9, None), (10, None), (7, p(i32(0, 2, 2))), (5, 0), (12, 0, WS),
             (11, work + 16), (3, p(i32(12, 13)))], native, "apap_sift_describe_oriented_batch_device")


def test_python_wrappers_refuse_bad_input(native):
    from cvx_proj_amd import features
    z = np.zeros
    ok_img, ok_pts = z((13, 13), np.uint8), z((3, 2))
    bad = [(z((13, 13), np.float32), ok_pts), (z((13, 13, 2), np.uint8), ok_pts), (z((12, 13), np.uint8), ok_pts), (z((13, 12, 3), np.uint8), ok_pts),
           (z((32769, 13), np.uint8), ok_pts), (ok_img, z((3, 3))), (ok_img, z((0, 2))), (ok_img, np.array([[1.0, np.nan]]))]
    for img, pts in bad:
        for call in (native.sift_orient, native.sift_describe_oriented, features.orient, lambda i, q: features.compute(i, q, angles="auto")):
            with pytest.raises(ValueError):
                call(img, pts)
    for angles in ([0, 1], [0, 1, -1], [0, 1, 360.5], [0, np.nan, 1], z((3, 1))):
        with pytest.raises(ValueError):
            native.sift_describe_oriented(ok_img, ok_pts, angles)
        with pytest.raises(ValueError):
            features.compute(ok_img, ok_pts, angles=angles)
    with pytest.raises(ValueError):
        features.compute(ok_img, ok_pts, angles="fastest")
    with pytest.raises(ValueError):
        native.sift_orient_batch([ok_img, ok_img], z((4, 2)), [1, 2])
    with pytest.raises(ValueError):
        native.sift_describe_oriented_batch([ok_img], z((4, 2)), [2, 2])
    with pytest.raises(ValueError):
        features.coarse_matching(ok_img, z((12, 13), np.uint8), ok_pts, ok_pts, oriented=True)
    if native.lib().apap_device_count() < 1:       # valid input reaches the library, which has no CPU fallback
        with pytest.raises(native.ApapError) as e:
            features.compute(ok_img, ok_pts, angles=[0, 90, 360])
        assert e.value.code == native.ERR_NO_DEVICE


def test_signatures_follow_the_header(native):
    """Every new entry point's ctypes argument list has the header's length and kinds (pointer, int, size_t)."""
    text = open(os.path.join(ROOT, "include", "apap_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    names = [n for n in native.SIGNATURES if n.startswith(("apap_sift_orient", "apap_sift_describe_oriented", "apap_sift_descr_window"))]
    assert len(names) == 11
    for name in names:
        m = re.search(rf"\b(int|size_t)\s+{name}\s*\(([^)]*)\)\s*;", text)
        assert m, name
        restype, argtypes = native.SIGNATURES[name]
        assert restype is (C.c_int if m.group(1) == "int" else C.c_size_t), name
        params = [a.strip() for a in m.group(2).split(",")]
        assert len(params) == len(argtypes), (name, params)
        for prm, ct in zip(params, argtypes):
            if "*" in prm:
                assert ct is C.c_void_p or issubclass(ct, C._Pointer), (name, prm, ct)
            elif prm.startswith("size_t"):
                assert ct is C.c_size_t, (name, prm)
            else:
                assert prm.startswith("int ") and ct is C.c_int, (name, prm)
    for const in ("ORIENT_SAMPLES", "DESCR_SAMPLES", "ORIENT_PATCH"):
        assert int(re.search(rf"#define APAP_SIFT_{const} (\d+)", text).group(1)) == getattr(native, "SIFT_" + const)
