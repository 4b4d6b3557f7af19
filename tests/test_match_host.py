"""Descriptor matching without a GPU: argument refusals before any device is touched, the workspace sizes, the no-device
error, the OpenCV stand-ins, and the specification's own consistency (tests/match_spec.py)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import match_spec as S
from conftest import ROOT


def i32(*v):
    return np.array(v, np.int32)


def p(a, t=C.c_int):
    return a.ctypes.data_as(C.POINTER(t))


def test_workspace_sizes(native):
    lib = native.lib()
    for nq, nt in ((1, 1), (64, 128), (65, 129), (2000, 2000), (3, 5000), (20000, 20000), (1 << 24, 1), (1, 1 << 24)):
        b = lib.apap_match_workspace_bytes(nq, nt)
        splits, per = native.match_splits(nq, nt)
        assert b > 0 and b % 256 == 0 and b >= 16 * splits * nq, (nq, nt, b)
        assert (splits - 1) * per * native.MATCH_TRAIN_CHUNK < nt <= splits * per * native.MATCH_TRAIN_CHUNK      # no empty split
        assert b == lib.apap_match_batch_workspace_bytes(p(i32(0, nq)), p(i32(0, nt)), 1) == \
            lib.apap_match_batch_workspace_bytes(p(i32(7, 7 + nq)), p(i32(3, 3 + nt)), 1)                         # the batch of one
    for nq, nt in ((0, 5), (5, 0), (-1, 5), (5, -3), ((1 << 24) + 1, 5), (5, (1 << 24) + 1)):
        assert lib.apap_match_workspace_bytes(nq, nt) == 0, (nq, nt)
    ok_q, ok_t = i32(0, 5, 9), i32(0, 300, 301)
    both = lib.apap_match_batch_workspace_bytes(p(ok_q), p(ok_t), 2)
    assert both > 0 and both % 256 == 0
    # additive over pairs but for the descriptor table's 256 bytes
    assert both == lib.apap_match_workspace_bytes(5, 300) + lib.apap_match_workspace_bytes(4, 1) - 256
    for qo, to, n in ((None, p(ok_t), 2), (p(ok_q), None, 2), (p(ok_q), p(ok_t), 0), (p(ok_q), p(ok_t), -1), (p(ok_q), p(ok_t), 65536),
                      (p(i32(0, 5, 5)), p(ok_t), 2), (p(i32(0, 5, 4)), p(ok_t), 2), (p(ok_q), p(i32(0, 300, 300)), 2),
                      (p(i32(-1, 5, 9)), p(ok_t), 2), (p(ok_q), p(i32(-2, 300, 301)), 2),
                      (p(i32(0, (1 << 24) + 1, (1 << 24) + 2)), p(ok_t), 2)):
        assert lib.apap_match_batch_workspace_bytes(qo, to, n) == 0


def test_invalid_arguments_are_refused_before_any_device_is_touched(native):
    """ERR_INVALID_ARG also on a machine without a GPU (there the next check would answer ERR_NO_DEVICE), and device 1 << 20
    cannot exist: an argument error means the device was not looked at."""
    lib = native.lib()
    q = np.zeros((4, 128), np.float32)
    idx, dist = np.zeros(4, np.int32), np.zeros(4, np.float32)
    f, far = C.c_float, 1 << 20
    host = lib.apap_match_descriptors
    good = [None, p(q, f), 4, p(q, f), 4, p(idx), p(dist, f), None, None, far]
    assert host(*good) == native.ERR_NO_DEVICE        # valid arguments: only now is the device looked at
    for at, bad in ((1, None), (3, None), (5, None), (6, None), (2, 0), (2, -4), (2, (1 << 24) + 1), (4, 0), (4, (1 << 24) + 1)):
        args = list(good)
        args[at] = bad
        assert host(*args) == native.ERR_INVALID_ARG, (at, bad)
        assert "apap_match_descriptors" in native.last_error()
    batch = lib.apap_match_descriptors_batch
    qo, to = i32(0, 1, 4), i32(0, 2, 4)
    good = [None, p(q, f), p(q, f), p(qo), p(to), 2, p(idx), p(dist, f), None, None, far]
    assert batch(*good) == native.ERR_NO_DEVICE
    for at, bad in ((1, None), (2, None), (3, None), (4, None), (6, None), (7, None), (5, 0), (5, 65536), (3, p(i32(0, 4, 4))),
                    (3, p(i32(2, 1, 4))), (4, p(i32(0, 0, 4))), (3, p(i32(-1, 1, 4)))):
        args = list(good)
        args[at] = bad
        assert batch(*args) == native.ERR_INVALID_ARG, (at, bad)
    # the resident forms: pointers are only compared and counted here, never followed
    fake, work = 1 << 20, 1 << 20
    need = lib.apap_match_workspace_bytes(4, 4)
    dev = lib.apap_match_descriptors_device
    good = [None, fake, 4, fake, 4, fake, fake, None, None, work, need, None]
    for at, bad, code in ((1, None, native.ERR_INVALID_ARG), (3, None, native.ERR_INVALID_ARG), (5, None, native.ERR_INVALID_ARG),
                          (6, None, native.ERR_INVALID_ARG), (9, None, native.ERR_INVALID_ARG), (2, 0, native.ERR_INVALID_ARG),
                          (4, (1 << 24) + 1, native.ERR_INVALID_ARG), (10, need - 1, native.ERR_WORKSPACE), (10, 0, native.ERR_WORKSPACE),
                          (9, work + 128, native.ERR_INVALID_ARG), (1, fake + 4, native.ERR_INVALID_ARG), (3, fake + 8, native.ERR_INVALID_ARG)):
        args = list(good)
        args[at] = bad
        assert dev(*args) == code, (at, bad)
    bdev = lib.apap_match_descriptors_batch_device
    need = lib.apap_match_batch_workspace_bytes(p(qo), p(to), 2)
    good = [None, fake, fake, p(qo), p(to), 2, fake, fake, None, None, work, need, None]
    for at, bad, code in ((1, None, native.ERR_INVALID_ARG), (3, None, native.ERR_INVALID_ARG), (4, p(i32(0, 2, 2)), native.ERR_INVALID_ARG),
                          (5, 0, native.ERR_INVALID_ARG), (11, need - 256, native.ERR_WORKSPACE), (10, work + 16, native.ERR_INVALID_ARG)):
        args = list(good)
        args[at] = bad
        assert bdev(*args) == code, (at, bad)


def test_python_wrappers_refuse_bad_shapes(native):
    z = np.zeros
    for q, t in ((z((4, 127)), z((4, 128))), (z((4, 128)), z((128,))), (z((4, 128)), z((2, 4, 128))), (z((0, 128)), z((4, 128))),
                 (z((4, 128)), z((0, 128)))):
        with pytest.raises(ValueError):
            native.match_descriptors(q, t)
    with pytest.raises(ValueError):
        native.match_descriptors_batch(z((4, 128)), z((4, 128)), [1, 2], [4])       # the counts do not sum to the rows
    with pytest.raises(ValueError):
        native.match_descriptors_batch(z((4, 128)), z((4, 128)), [4, 0], [2, 2])
    with pytest.raises(ValueError):
        native.match_descriptors_batch(z((4, 128)), z((4, 128)), [4], [2, 2])
    assert native.as_descriptors(np.arange(256, dtype=np.uint8).reshape(2, 128)).dtype == np.float32
    assert native.MATCH_DIM == native.SPECTRAL_DIM == 128
    header = open(os.path.join(ROOT, "include", "apap_hip.h")).read()
    for name in ("DIM", "QUERY_TILE", "TRAIN_CHUNK", "WANT_BLOCKS"):
        assert f"#define APAP_MATCH_{name} {getattr(native, 'MATCH_' + name)}" in header


def test_no_device_no_fallback(native):
    if native.lib().apap_device_count() > 0:
        pytest.skip("a GPU is visible")
    q = np.ones((3, 128), np.uint8)
    with pytest.raises(native.ApapError) as e:
        native.match_descriptors(q, q)
    assert e.value.code == native.ERR_NO_DEVICE
    with pytest.raises(native.ApapError) as e:
        native.match_descriptors_batch(q, q, [1, 2], [2, 1])
    assert e.value.code == native.ERR_NO_DEVICE
    from cvx_proj_amd import matching
    with pytest.raises(native.ApapError) as e:
        matching.match(q, q, ratio=0.8, cross_check=True)
    assert e.value.code == native.ERR_NO_DEVICE


def test_the_stand_ins_behave_as_cv_to_array_needs():
    from cvx_proj_amd import matching
    from cvx_proj_amd.spectral_method import cv_to_array, normalized_feature
    kc = [matching.KeyPoint(1.5, 2.25), matching.KeyPoint(np.float32(0.1), 7, 1)]
    ko = [matching.KeyPoint(10, 20), matching.KeyPoint(30, 40), matching.KeyPoint(50.5, 60.5)]
    assert kc[0].pt == (1.5, 2.25) and kc[0].size == 1.0 and type(kc[1].pt[0]) is float and kc[1].pt[0] == float(np.float32(0.1))
    m = [matching.DMatch(1, 2, np.float32(3.5)), matching.DMatch(0, 0, 0.0)]
    assert (m[0].queryIdx, m[0].trainIdx, m[0].distance, m[0].imgIdx) == (1, 2, 3.5, 0) and type(m[0].distance) is float
    assert m[0] == matching.DMatch(1, 2, 3.5) and m[0] != m[1] and "trainIdx=2" in repr(m[0])
    src, dst = cv_to_array(kc, ko, m)
    assert src.dtype == np.float32 and src.tolist() == [[float(np.float32(0.1)), 7.0], [1.5, 2.25]] and dst.tolist() == [[50.5, 60.5], [10.0, 20.0]]
    fc, fo = np.arange(256, dtype=np.float32).reshape(2, 128) + 1, np.ones((3, 128), np.float32)
    c, o = cv_to_array(fc, fo, m, is_pts=False)
    assert np.array_equal(c, fc[[1, 0]]) and np.array_equal(o, fo[[2, 0]])
    a, b = normalized_feature(fc, fo, m[0])
    assert np.isclose(np.linalg.norm(a), 1) and np.isclose(np.linalg.norm(b), 1)
    r = matching.MatchResult(1, 2, 3, 4)
    assert r._fields == ("train_idx", "distance", "second_idx", "second_distance")
    with pytest.raises(ValueError):       # keypoints and descriptors must pair up (checked before any matching)
        matching.coarse_matching(np.zeros((3, 2)), np.zeros((4, 128)), np.zeros((4, 2)), np.zeros((4, 128)))
    with pytest.raises(ValueError):
        matching.matched_arrays(np.zeros((4, 2)), np.zeros((4, 128)), np.zeros((4, 2)), np.zeros((4, 64)))


def test_matching_imports_without_torch_and_scipy():
    code = ("import sys; import cvx_proj_amd.matching as M; from cvx_proj_amd import _native; _native.lib(); "
            "assert 'torch' not in sys.modules, 'torch was imported'; assert 'scipy' not in sys.modules, 'scipy was imported'; "
            "assert 'cv2' not in sys.modules; print(sorted(M.__all__))")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-1500:]
    assert r.stdout.strip() == str(sorted(["MatchResult", "DMatch", "KeyPoint", "match_descriptors", "match", "coarse_matching",
                                           "matched_arrays"]))


def test_the_specification_agrees_with_itself():
    """match_spec: the expanded int64 d2 equals the plain sum of squared differences; the two ways to the two smallest agree
    on tie-heavy rows; the filters do what they say; and the issue's claim about the expansion in float32."""
    rng = np.random.default_rng(0)
    q, t = rng.integers(0, 256, (9, 128)), rng.integers(0, 256, (40, 128))
    plain = ((q[:, None, :] - t[None, :, :]) ** 2).sum(-1)
    assert plain.dtype == np.int64 and np.array_equal(S.d2_int(q.astype(np.float32), t.astype(np.uint8)), plain)
    assert np.array_equal(S.d2_f64(q.astype(np.float32), t.astype(np.float32)), plain.astype(np.float64))
    ties = rng.integers(0, 3, (50, 30))
    for d in (ties, ties.astype(np.float64), ties[:, :1], ties[:, :2]):
        a, b = S.two_smallest(d), S.two_smallest_by_argmin(d)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    idx, dist, idx2, dist2 = S.match_int(np.zeros((1, 128)), np.array([[255] * 128, [0] * 127 + [3], [0] * 127 + [3]]))
    assert (idx[0], idx2[0], dist[0], dist2[0]) == (1, 2, 3.0, 3.0) and dist.dtype == np.float32 and idx.dtype == np.int32
    one = S.match_int(np.zeros((2, 128)), np.ones((1, 128)))
    assert one[2].tolist() == [-1, -1] and np.all(np.isinf(one[3])) and one[3].dtype == np.float32
    keep = S.filters(np.array([2, 0, -1, 1]), np.float32([1, 5, np.inf, 2]), np.float32([2, 5.5, np.inf, 2]), np.array([1, 3, 0]),
                     ratio=0.8, cross_check=True)
    assert keep.tolist() == [0]
    assert 1.57e-5 < S.EPS < 1.58e-5
    # the difference form in float32 picks every neighbour of the near-duplicate set right, the expansion does not
    base = 100 + rng.normal(0, 1, (75, 128))
    train = np.empty((150, 128), np.float32)
    train[0::2], train[1::2] = base, base + rng.normal(0, 2e-2, base.shape)
    qs = (base[rng.integers(0, 75, 130)] + rng.normal(0, 1.5e-2, (130, 128))).astype(np.float32)
    truth = S.d2_f64(qs, train).argmin(1)
    diff = qs[:, None, :] - train[None, :, :]
    assert np.array_equal((diff * diff).sum(-1, dtype=np.float32).argmin(1), truth)
    expansion = (qs * qs).sum(1)[:, None] + (train * train).sum(1)[None, :] - 2 * (qs @ train.T)
    assert np.count_nonzero(expansion.argmin(1) != truth) > 10
