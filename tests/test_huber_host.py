"""The Huber M-step without a GPU: the C ABI's new constants, every refusal (before any device is touched: the data pointers
here are null) and the Python spellings' argument rules."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT


def header():
    return open(os.path.join(ROOT, "include", "apap_hip.h")).read()


def test_constants_match_the_header(native):
    text = header()
    assert int(re.search(r"#define APAP_MODEL_HUBER (\d+)", text).group(1)) == native.MODEL_HUBER == 2
    assert int(re.search(r"#define APAP_MODEL_HUBER_THREADS (\d+)", text).group(1)) == native.MODEL_HUBER_THREADS
    assert re.search(r"#define APAP_MODEL_HUBER_M APAP_MODEL_DU\b", text)
    assert int(re.search(r"#define APAP_MODEL_PARAMS (\d+)", text).group(1)) == native.MODEL_PARAMS == 6
    from huber_cases import T
    assert T == native.MODEL_HUBER_THREADS
    p = native.model_params(native.MODEL_HUBER, 0.5)
    assert p.shape == (6,) and p[0] == 2 and p[1] == 0.5 and p[5] == 0


def device_call(native, params, n):
    """apap_model_solve_device with null pointers: only the host checks can answer."""
    return native.lib().apap_model_solve_device(None, None, None, None, n, params.ctypes.data_as(native._f64p), None, None, None,
                                                None, 0, None)


def test_mode_2_passes_the_parameter_check(native):
    """With good Huber parameters the call gets as far as the null data pointers; mode 3 stays invalid."""
    E = native.ERR_INVALID_ARG
    assert device_call(native, native.model_params(native.MODEL_HUBER, 0.5), 8) == E
    assert b"null device pointer" in native.lib().apap_last_error()
    assert device_call(native, native.model_params(native.MODEL_HUBER, 0.5, max_iter=1), 1 << 20) == E
    assert b"null device pointer" in native.lib().apap_last_error()
    bad = native.model_params(native.MODEL_HUBER, 0.5)
    bad[0] = 3
    assert device_call(native, bad, 8) == E
    assert b"mode 3" in native.lib().apap_last_error()


@pytest.mark.parametrize("M", [1e-2, 0.0, -1.0, 9.9e-3, np.nan, np.inf, -np.inf])
def test_bad_M_is_refused_without_a_device(native, M):
    assert device_call(native, native.model_params(native.MODEL_HUBER, M), 8) == native.ERR_INVALID_ARG
    msg = native.lib().apap_last_error()
    assert b"null" not in msg and (b"Huber M" in msg or b"not finite" in msg)
    pc = (np.arange(16, dtype=np.float32).reshape(8, 2) * 7) % 13
    with pytest.raises(native.ApapError) as e:
        native.model_solve(pc, pc, np.ones(8, np.float32), native.model_params(native.MODEL_HUBER, M))
    assert e.value.code in (native.ERR_INVALID_ARG, native.ERR_NO_DEVICE) and np.isnan(e.value.info).all()


def test_dv_must_be_finite_and_the_smallest_M_passes(native):
    p = native.model_params(native.MODEL_HUBER, 0.5, np.nan)
    assert device_call(native, p, 8) == native.ERR_INVALID_ARG and b"not finite" in native.lib().apap_last_error()
    p = native.model_params(native.MODEL_HUBER, np.nextafter(1e-2, 1.0))
    assert device_call(native, p, 8) == native.ERR_INVALID_ARG and b"null device pointer" in native.lib().apap_last_error()


def test_more_than_2_to_20_matches_are_refused_without_a_device(native):
    p = native.model_params(native.MODEL_HUBER, 0.5)
    assert device_call(native, p, (1 << 20) + 1) == native.ERR_INVALID_ARG
    assert b"2^20" in native.lib().apap_last_error()
    # the other modes keep their range
    assert device_call(native, native.model_params(native.MODEL_LMS), (1 << 20) + 1) == native.ERR_INVALID_ARG
    assert b"null device pointer" in native.lib().apap_last_error()
    # the EM loop's resident form
    sp = native.spectral_params()
    rc = native.lib().apap_spectral_em_device(None, None, None, None, None, (1 << 20) + 1, None, sp.ctypes.data_as(native._f64p),
                                              p.ctypes.data_as(native._f64p), 2, None, None, None, None, None, None, None, None,
                                              None, 0, None)
    assert rc == native.ERR_INVALID_ARG and b"2^20" in native.lib().apap_last_error()


def test_workspace_does_not_depend_on_the_mode(native):
    lib = native.lib()
    assert lib.apap_model_workspace_bytes(1 << 24) <= 1024 * 15 * 15 * 8 + 8192


def test_the_batch_refuses_mode_2(native):
    i32 = lambda a: np.asarray(a, np.int32)      # noqa: E731
    off, po = i32([0, 5, 12]), i32([0, 1])
    sp = np.stack([native.spectral_params()] * 2)
    mp = np.stack([native.model_params(native.MODEL_SDP, 0.5, 0.5), native.model_params(native.MODEL_HUBER, 0.5)])
    ip = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_int))      # noqa: E731
    f64 = native._f64p
    rc = native.lib().apap_spectral_em_batch_device(None, None, None, None, None, None, None, ip(off), 2, ip(po),
                                                    sp.ctypes.data_as(f64), mp.ctypes.data_as(f64), 2, 2, None, None, None, None,
                                                    None, None, None, None, 0, None)
    assert rc == native.ERR_INVALID_ARG
    msg = native.lib().apap_last_error()
    assert b"problem 1" in msg and b"Huber" in msg and b"not available" in msg
    rng = np.random.default_rng(0)
    src = (rng.random((6, 2)) * 900).astype(np.float32)
    d = rng.random((6, 128), dtype=np.float32)
    with pytest.raises(native.ApapValueError, match="Huber.*not available"):      # the host-buffer form, with or without a GPU
        native.spectral_em_batch(src, src + np.float32(3), d, d, np.eye(3)[None], np.ones(6, np.float32), [6], [0],
                                 native.spectral_params()[None], native.model_params(native.MODEL_HUBER, 0.5)[None], 2)


def test_the_local_model_refuses_mode_2(native):
    p = native.model_params(native.MODEL_HUBER, 0.5)
    rc = native.lib().apap_local_model_solve_device(None, None, None, None, 50, None, 4, 0.1, 10.0, p.ctypes.data_as(native._f64p),
                                                    None, None, None, None, 0, None)
    assert rc == native.ERR_INVALID_ARG
    msg = native.lib().apap_last_error()
    assert b"Huber" in msg and b"not available" in msg
    pc = (np.arange(100, dtype=np.float32).reshape(50, 2) * 7) % 13
    with pytest.raises(native.ApapValueError, match="Huber.*not available"):
        native.local_model_solve(pc, pc, np.zeros((4, 2)), 0.1, 10.0, p)


def test_huber_solver_argument_rules(native):
    from cvx_proj_amd import model
    from cvx_proj_amd.model import HuberSolver, LMSSolver
    assert "HuberSolver" in model.__all__ and issubclass(HuberSolver, LMSSolver)
    for bad in (1e-2, 0.0, -1.0, np.nan, np.inf):
        with pytest.raises(ValueError):
            HuberSolver(100, bad)
    s = HuberSolver(8000, 0.5, device=-1)
    assert s.max_iter == 8000 and s.huber_param == 0.5 and s.last is None
    for swap in (True, False):
        p = s._params(swap)
        assert p[0] == native.MODEL_HUBER and p[1] == 0.5 and p[3] == -np.inf and p[4] == float(swap) and p[5] == 0
    e = np.zeros((0, 2), np.float32)
    with pytest.raises(IndexError):                     # the reference's exception for no point, before any device
        s.solve(e, e, np.zeros(0, np.float32), verbose=1)
    # the reference's spelling keeps its refusal
    with pytest.raises(NotImplementedError, match="Huber"):
        LMSSolver(100, 0.5)._params(True)


class KP:
    def __init__(self, p):
        self.pt = (float(p[0]), float(p[1]))


class DM:
    def __init__(self, i):
        self.queryIdx = self.trainIdx = i


def test_loss_keyword_rules(native):
    from cvx_proj_amd import spectral_method as sm
    pts = [KP((i, 2 * i + 1)) for i in range(6)]
    m = [DM(i) for i in range(6)]
    w = np.ones(6, np.float32)
    with pytest.raises(ValueError, match="lms"):
        sm.model_solve(pts, pts, m, w, param=0.5, lms=False, loss="huber")
    with pytest.raises(ValueError, match="1e-2"):
        sm.model_solve(pts, pts, m, w, param=1e-2, lms=True, loss="huber")
    with pytest.raises(ValueError, match="loss"):
        sm.model_solve(pts, pts, m, w, loss="l1")
    with pytest.raises(IndexError):                     # as every mode: no selected match
        sm.model_solve(pts, pts, m, np.full(6, 9e-4, np.float32), loss="huber")
    with pytest.raises(NotImplementedError, match="Huber"):      # loss=None: today's behaviour
        sm.model_solve(pts, pts, m, w)
    pc = (np.arange(10, dtype=np.float32).reshape(5, 2) * 37) % 101
    d = np.ones((5, 128), np.float32)
    kw = dict(mask=np.ones(5, np.float32))
    with pytest.raises(ValueError, match="lms"):
        sm.spectral_em(pc, pc, d, d, np.eye(3), lms=False, huber_param=0.5, loss="huber", **kw)
    with pytest.raises(ValueError, match="1e-2"):
        sm.spectral_em(pc, pc, d, d, np.eye(3), lms=True, huber_param=-1.0, loss="huber", **kw)
    with pytest.raises(NotImplementedError, match="Huber"):
        sm.spectral_em(pc, pc, d, d, np.eye(3), lms=True, huber_param=0.5, **kw)
    assert sm._model_mode(True, 0.5, 0.25, "huber").tolist() == native.model_params(native.MODEL_HUBER, 0.25).tolist()
    assert sm._model_mode(True, 0.5, -1.0).tolist() == native.model_params(native.MODEL_LMS).tolist()


def test_no_convergence_warning_names_the_method(native):
    from cvx_proj_amd.model import result_of, warn_no_convergence
    info = np.full(native.MODEL_INFO, np.nan)
    info[native.MODEL_INFO_STATUS] = native.STATUS_MODEL_NO_CONVERGENCE
    info[[native.MODEL_INFO_GAP, native.MODEL_INFO_ITERS, native.MODEL_INFO_COUNT]] = 1e-3, 100, 50
    with pytest.warns(RuntimeWarning, match="Huber"):
        warn_no_convergence(result_of(info))
    info[[native.MODEL_INFO_R, native.MODEL_INFO_T]] = 1.0, 2.0
    with pytest.warns(RuntimeWarning, match="SDP"):
        warn_no_convergence(result_of(info))


def test_the_kernel_source_follows_the_library_conventions():
    text = open(os.path.join(ROOT, "cvx_proj_amd", "csrc", "apap_model.hip")).read()
    assert "k_model_huber" in text and "hipLaunchCooperativeKernel" not in text
    launch = text[text.index("void model_launch("):text.index("}  // namespace")]
    assert "hipStreamSynchronize" not in launch and "hipDeviceSynchronize" not in launch and "hipMemcpy" not in launch
