"""Guided matching without a GPU: symbols, constants, refusals before any device is touched, the Python argument rules."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("apap_guided_records", "apap_guided_records_device", "apap_match_guided", "apap_match_guided_device",
           "apap_match_guided_batch", "apap_match_guided_batch_device", "apap_match_guided_workspace_bytes",
           "apap_match_guided_batch_workspace_bytes")


def p(a, ct=C.c_int):
    return a.ctypes.data_as(C.POINTER(ct))


def i32(*v):
    return np.array(v, dtype=np.int32)


def test_symbols_exported_and_bound(native):
    handle = C.CDLL(native.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "apap_hip.h")).read()
    for sym in SYMBOLS:
        assert hasattr(handle, sym) and sym in native.SIGNATURES and re.search(rf"\b{sym}\(", header), sym
    assert native.lib().apap_abi_version() == native.ABI_VERSION == 6      # additive
    make = open(os.path.join(ROOT, "cvx_proj_amd", "csrc", "Makefile")).read()
    src, ksrc = re.search(r"^SRC\s*:=(.*)$", make, re.M).group(1), re.search(r"^KSRC\s*:=(.*)$", make, re.M).group(1)
    assert "apap_match_guided.hip" in src and "apap_match_guided.hip" in ksrc and "-ffp-contract=off" in make


def test_constants_equal_the_headers(native):
    header = open(os.path.join(ROOT, "include", "apap_hip.h")).read()
    for name in ("REC_POINT", "REC_PROJECT", "REC_LINE", "POINT", "LINE", "QUERY_TILE", "TRAIN_CHUNK", "DRAIN", "WANT_BLOCKS"):
        assert f"#define APAP_GUIDED_{name} {getattr(native, 'GUIDED_' + name)}\n" in header, name
    assert native.GUIDED_DRAIN == 64 and native.GUIDED_TRAIN_CHUNK % 4 == 0


def test_the_source_keeps_the_projects_rules():
    text = open(os.path.join(ROOT, "cvx_proj_amd", "csrc", "apap_match_guided.hip")).read()
    assert "getenv" not in text and not re.search(r"cooperative_groups|grid\.sync|hipLaunchCooperativeKernel", text)
    assert not re.search(r"atomicAdd|atomicMin\s*\(\s*\(?\s*float|atomicMax", text)      # the one atomic is an integer minimum
    assert not re.search(r"^\s*(static\s+)?(int|bool)\s+g_\w+\s*=", text, flags=re.M)
    # the matcher's d2 step - the subtraction, then the fused multiply-add - is written once, in the header both sources
    # include, and both sum by it: neither spells a sum of its own
    matcher = open(os.path.join(ROOT, "cvx_proj_amd", "csrc", "apap_match.hip")).read()
    shared = open(os.path.join(ROOT, "cvx_proj_amd", "csrc", "apap_match_dev.h")).read()
    assert len(re.findall(r"const float d = q - t;\s*return fmaf\(d, d, acc\);", shared)) == 1 and shared.count("fmaf(") == 1
    for source in (text, matcher):
        assert '#include "apap_match_dev.h"' in source and "fmaf(" not in source and "_rn(" not in source
    assert "acc = d2_step(acc, qa[k], tv[k]);" in text and "acc[a][b] = d2_step(acc[a][b], qa[a], tv[b]);" in matcher
    assert "apap_match_guided" not in matcher


def test_workspace_sizes(native):
    lib = native.lib()
    nq, nt = 257, 300
    splits, per = native.guided_splits(nq, nt)
    up = lambda b: -(-b // 256) * 256      # noqa: E731
    assert lib.apap_match_guided_workspace_bytes(nq, nt) == up(48) + up(8 * nt) + up(24 * splits * nq)
    qo, to = i32(3, 4, 260), i32(0, 300, 301)
    assert lib.apap_match_guided_batch_workspace_bytes(p(qo), p(to), 2) == up(96) + up(8 * 301) + up(24 * (3 * 1 + 256))
    for a, b in ((0, 4), (4, 0), (-1, 4), ((1 << 24) + 1, 4)):
        assert lib.apap_match_guided_workspace_bytes(a, b) == 0
    assert lib.apap_match_guided_batch_workspace_bytes(p(i32(0, 4, 4)), p(to), 2) == 0
    assert native.guided_splits(1, 1) == (1, 1)


def test_invalid_arguments_are_refused_before_any_device_is_touched(native):
    """ERR_INVALID_ARG also on a machine without a GPU (there the next check would answer ERR_NO_DEVICE), and device 1 << 20
    cannot exist: an argument error means the device was not looked at."""
    lib = native.lib()
    q, rec = np.zeros((4, 128), np.float32), np.zeros((4, 3))
    idx, dist = np.zeros(4, np.int32), np.zeros(4, np.float32)
    f, d, far = C.c_float, C.c_double, 1 << 20
    INV, NODEV, WS = native.ERR_INVALID_ARG, native.ERR_NO_DEVICE, native.ERR_WORKSPACE
    host = lib.apap_match_guided
    good = [None, p(rec, d), p(q, f), 4, p(rec, d), p(q, f), 4, 0, 36.0, p(idx), p(dist, f), None, None, None, None, None, far]
    assert host(*good) == NODEV        # valid arguments: only now is the device looked at
    for at, bad in ((1, None), (2, None), (4, None), (5, None), (9, None), (10, None), (3, 0), (3, (1 << 24) + 1), (6, 0), (6, -2),
                    (7, 2), (7, -1), (8, float("nan")), (8, -1.0), (8, float("-inf")), (14, p(idx)), (15, p(dist, f))):
        args = list(good)
        args[at] = bad
        assert host(*args) == INV, (at, bad)
        assert "apap_match_guided" in native.last_error()
    for ok in ((8, float("inf")), (8, 0.0), (7, 1)):
        args = list(good)
        args[ok[0]] = ok[1]
        assert host(*args) == NODEV, ok
    batch = lib.apap_match_guided_batch
    qo, to, r2 = i32(0, 1, 4), i32(0, 2, 4), np.array([1.0, np.inf])
    good = [None, p(rec, d), p(rec, d), p(q, f), p(q, f), p(qo), p(to), 2, 1, p(r2, d), p(idx), p(dist, f), None, None, None, None, None, far]
    assert batch(*good) == NODEV
    for at, bad in ((1, None), (2, None), (3, None), (4, None), (5, None), (6, None), (9, None), (10, None), (11, None), (7, 0),
                    (7, 65536), (5, p(i32(0, 4, 4))), (6, p(i32(0, 0, 4))), (5, p(i32(-1, 1, 4))), (8, 2),
                    (9, p(np.array([1.0, np.nan]), d)), (9, p(np.array([-0.5, 1.0]), d)), (15, p(idx))):
        args = list(good)
        args[at] = bad
        assert batch(*args) == INV, (at, bad)
    # the resident forms: pointers are only compared and counted here, never followed
    fake, work = 1 << 20, 1 << 20
    need = lib.apap_match_guided_workspace_bytes(4, 4)
    dev = lib.apap_match_guided_device
    good = [None, fake, fake, 4, fake, fake, 4, 0, 36.0, fake, fake, None, None, None, None, None, work, need, None]
    for at, bad, code in ((1, None, INV), (2, None, INV), (4, None, INV), (5, None, INV), (9, None, INV), (10, None, INV),
                          (16, None, INV), (3, 0, INV), (6, (1 << 24) + 1, INV), (7, 5, INV), (8, float("nan"), INV), (8, -4.0, INV),
                          (14, fake, INV), (15, fake, INV), (17, need - 1, WS), (17, 0, WS), (16, work + 128, INV),
                          (2, fake + 4, INV), (5, fake + 8, INV)):
        args = list(good)
        args[at] = bad
        assert dev(*args) == code, (at, bad)
    bdev = lib.apap_match_guided_batch_device
    need = lib.apap_match_guided_batch_workspace_bytes(p(qo), p(to), 2)
    good = [None, fake, fake, fake, fake, p(qo), p(to), 2, 0, p(r2, d), fake, fake, None, None, None, None, None, work, need, None]
    for at, bad, code in ((1, None, INV), (5, None, INV), (6, p(i32(0, 2, 2)), INV), (7, 0, INV), (9, None, INV),
                          (9, p(np.array([np.nan, 1.0]), d), INV), (18, need - 256, WS), (17, work + 16, INV)):
        args = list(good)
        args[at] = bad
        assert bdev(*args) == code, (at, bad)
    # records
    pts, out, M = np.zeros((4, 2), np.float32), np.zeros((4, 3)), np.eye(3)
    good = [None, p(pts, f), 4, p(M, d), 1, p(out, d), far]
    assert lib.apap_guided_records(*good) == NODEV
    args = list(good)
    args[3], args[4] = None, 0
    assert lib.apap_guided_records(*args) == NODEV       # POINT ignores the model: NULL is fine
    for at, bad in ((1, None), (5, None), (2, 0), (2, (1 << 24) + 1), (4, 3), (4, -1), (3, None)):
        args = list(good)
        args[at] = bad
        assert lib.apap_guided_records(*args) == INV, (at, bad)
    args = list(good)
    args[3], args[4] = None, 2
    assert lib.apap_guided_records(*args) == INV         # LINE without a model
    rdev = lib.apap_guided_records_device
    assert rdev(None, fake, 4, None, 1, fake, None) == INV and rdev(None, None, 4, fake, 1, fake, None) == INV
    assert rdev(None, fake, 4, fake, 7, fake, None) == INV and rdev(None, fake, 0, fake, 1, fake, None) == INV


def test_python_argument_rules(native):
    from cvx_proj_amd import guided, matching
    z = np.zeros
    kp, fe = z((4, 2)), z((4, 128))
    for kw in ({}, {"H": np.eye(3), "F": np.eye(3)}, {"H": np.eye(3), "grid": (z((1, 1, 3, 3)), None, (0, 0))},
               {"H": np.eye(3), "F": np.eye(3), "grid": (z((1, 1, 3, 3)), None, (0, 0))}):
        with pytest.raises(ValueError, match="exactly one"):
            guided.guided_match(kp, fe, kp, fe, **kw)
        with pytest.raises(ValueError, match="exactly one"):
            guided.guided_matched_arrays(kp, fe, kp, fe, **kw)
    with pytest.raises(ValueError):
        guided.guided_match(z((3, 2)), fe, kp, fe, H=np.eye(3))           # keypoints and descriptors must pair up
    with pytest.raises(ValueError):
        guided.guided_match(kp, z((4, 64)), kp, fe, H=np.eye(3))
    with pytest.raises(TypeError):
        guided.guided_matched_arrays(kp, fe, kp, fe, H=np.eye(3), radios=3)
    rec = z((4, 3))
    for radius in (np.nan, -1.0):
        with pytest.raises(ValueError):
            guided.guided_match_descriptors(fe, fe, rec, rec, "point", radius)
        with pytest.raises(ValueError):
            native.match_guided(fe, fe, rec, rec, "point", radius)
    for bad in ((fe, fe, z((3, 3)), rec, "point"), (fe, fe, rec, z((4, 2)), "point"), (fe, fe, rec, rec, "circle"), (z((4, 12)), fe, rec, rec, 0)):
        with pytest.raises(ValueError):
            native.match_guided(*bad, 1.0)
    with pytest.raises(ValueError):
        native.match_guided_batch(fe, fe, rec, rec, [1, 2], [4], "point", 1.0)
    with pytest.raises(ValueError):
        native.match_guided_batch(fe, fe, rec, rec, [2, 2], [2, 2], "point", [1.0, 2.0, 3.0])
    for pts, model, what in ((z((4, 3)), None, "point"), (kp, None, "project"), (kp, None, "line"), (kp, z((2, 3)), "line"),
                             (kp, np.eye(3), "circle"), (z((0, 2)), None, "point")):
        with pytest.raises(ValueError):
            guided.records(pts, model, what)
    # the pinned surfaces have not grown
    assert matching.__all__ == ["MatchResult", "DMatch", "KeyPoint", "match_descriptors", "match", "coarse_matching", "matched_arrays"]
    assert guided.GuidedResult._fields == ("train_idx", "distance", "second_idx", "second_distance", "count", "query_idx", "query_distance")


def test_no_device_no_fallback(native):
    if native.lib().apap_device_count() > 0:
        pytest.skip("a GPU is visible")
    from types import SimpleNamespace
    from cvx_proj_amd import guided
    kp, fe = np.ones((3, 2)), np.ones((3, 128), np.uint8)
    calls = (lambda: guided.records(kp), lambda: guided.guided_match(kp, fe, kp, fe, H=np.eye(3)),
             lambda: guided.guided_match(kp, fe, kp, fe, F=np.eye(3), cross_check=True),
             lambda: native.match_guided(fe, fe, np.ones((3, 3)), np.ones((3, 3)), "point", 4.0),
             lambda: guided.rematch(kp, fe, kp, fe, np.eye(3), SimpleNamespace(em_radius=6.0, score_thresh=0.4)))
    for call in calls:
        with pytest.raises(native.ApapError) as e:
            call()
        assert e.value.code == native.ERR_NO_DEVICE


def test_the_module_imports_without_torch_scipy_or_cv2():
    code = ("import sys; import cvx_proj_amd.guided as G; from cvx_proj_amd import _native; _native.lib(); "
            "bad = [m for m in ('torch', 'scipy', 'cv2') if m in sys.modules]; assert not bad, bad; "
            "assert set(G.__all__) == {'GuidedResult', 'records', 'guided_match_descriptors', 'guided_match', "
            "'guided_matched_arrays', 'rematch'}; print('ok')")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stderr[-1500:]
