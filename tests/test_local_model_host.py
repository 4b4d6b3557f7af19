"""The robust moving DLT without a GPU: the C ABI's three symbols, the workspace rule (a chunk of cells, not the mesh),
every refusal the header lists - before any device is touched -, and the Python method's argument checks."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT

SYMBOLS = ("apap_local_model_workspace_bytes", "apap_local_model_solve_device", "apap_local_model_solve")


def test_symbols_exported_and_bound(native):
    text = open(os.path.join(ROOT, "include", "apap_hip.h")).read()
    handle = ctypes.CDLL(native.LIB_PATH)
    for sym in SYMBOLS:
        assert re.search(rf"\b{sym}\s*\(", text), sym
        assert hasattr(handle, sym) and sym in native.SIGNATURES, sym
    assert int(re.search(r"#define APAP_LOCAL_MODEL_CHUNK (\d+)", text).group(1)) == native.LOCAL_MODEL_CHUNK >= 4096
    assert "#define APAP_LOCAL_MODEL_MAX_CELLS (1 << 24)" in text and native.LOCAL_MODEL_MAX_CELLS == 1 << 24
    assert "apap_local_model.hip" in open(os.path.join(ROOT, "cvx_proj_amd", "csrc", "Makefile")).read()


def test_workspace_is_a_chunk_of_cells(native):
    ws = native.lib().apap_local_model_workspace_bytes
    chunk = native.LOCAL_MODEL_CHUNK
    for n, cells in ((0, 4), (-1, 4), (4, 0), (4, -3), ((1 << 26) + 1, 4), (4, native.LOCAL_MODEL_MAX_CELLS + 1)):
        assert ws(n, cells) == 0, (n, cells)
    for n in (1, 50, 240, 241, 2000, 1 << 20):
        one = ws(n, 1)
        assert one > 0 and one % 256 == 0
        assert one >= native.lib().apap_model_workspace_bytes(n)        # at least the single solve's scratch
        last = 0
        for cells in (1, 2, 5, 108, chunk - 1, chunk, chunk + 1, 40000, native.LOCAL_MODEL_MAX_CELLS):
            b = ws(n, cells)
            assert b % 256 == 0 and b >= last and b == min(cells, chunk) * one, (n, cells)
            last = b
        assert ws(n, chunk) == ws(n, chunk + 1) == ws(n, 10 * chunk)    # constant beyond the chunk
    # a 200 x 200 mesh at n = 2000 asks for a chunk's scratch (well under 100 MB), not the mesh's 650 MB
    assert ws(2000, 40000) < 100 << 20


def problem(n=8, cells=3):
    pc = ((np.arange(2 * n, dtype=np.float32).reshape(n, 2) * 37) % 101).astype(np.float32)
    po = pc + np.float32(3)
    v = (np.arange(2 * cells, dtype=np.float64).reshape(cells, 2) * 11) % 97
    return pc, po, v


def host_call(native, pc, po, mw, n, v, cells, gamma, sigma, params, H, info=None, status=None, ctx=None):
    f32, f64, i32 = native._f32p, native._f64p, native._i32p
    p = lambda a, t: None if a is None else a.ctypes.data_as(t)      # noqa: E731
    return native.lib().apap_local_model_solve(ctx, p(pc, f32), p(po, f32), p(mw, f32), n, p(v, f64), cells, gamma, sigma,
                                               p(params, f64), p(H, f32), p(info, f64), p(status, i32), -1)


def bad_params(native):
    ok = native.model_params(native.MODEL_SDP, 0.5, 0.5)
    out = []
    for idx, val, what in ((0, 3.0, "mode"), (0, 0.5, "mode"), (1, -0.1, "du negative"), (2, -1.0, "dv negative"),
                           (1, np.inf, "du inf"), (2, np.nan, "dv NaN"), (4, 2.0, "swap"), (5, -1.0, "max_iter"),
                           (3, np.nan, "floor NaN")):
        p = ok.copy()
        p[idx] = val
        out.append((p, what))
    return ok, out


def test_host_buffer_form_refuses_bad_arguments_and_leaves_nan(native):
    """Every refusal comes back as INVALID_ARG whether or not a device is visible (so: before any device is touched), and
    H_out / info_out are NaN, status_out zero, after it."""
    pc, po, v = problem()
    n, cells = len(pc), len(v)
    ok, bad = bad_params(native)

    def refused(what, **kw):
        a = dict(pc=pc, po=po, mw=None, n=n, v=v, cells=cells, gamma=0.5, sigma=100.0, params=ok)
        a.update(kw)
        H = np.zeros((cells, 9), np.float32)
        info = np.zeros((cells, native.MODEL_INFO))
        status = np.full(cells, 77, np.int32)
        code = host_call(native, a["pc"], a["po"], a["mw"], a["n"], a["v"], a["cells"], a["gamma"], a["sigma"], a["params"], H, info,
                         status)
        assert code == native.ERR_INVALID_ARG, (what, code, native.last_error())
        if 1 <= a["cells"] <= cells:
            k = a["cells"]
            assert np.isnan(H[:k]).all() and np.isnan(info[:k]).all() and not status[:k].any(), what

    refused("null pts_c", pc=None)
    refused("null pts_o", po=None)
    refused("null vertices", v=None)
    refused("null params", params=None)
    refused("n = 0", n=0)
    refused("n < 0", n=-4)
    refused("cells = 0", cells=0)
    refused("cells < 0", cells=-1)
    refused("cells above the limit", cells=native.LOCAL_MODEL_MAX_CELLS + 1)
    for sigma in (0.0, -5.0, np.nan, np.inf):
        refused(f"sigma {sigma}", sigma=sigma)
    refused("gamma NaN", gamma=np.nan)
    for p, what in bad:
        refused(what, params=p)
    assert host_call(native, pc, po, None, n, v, cells, 0.5, 100.0, ok, None) == native.ERR_INVALID_ARG      # null H_out


def test_device_form_refuses_before_any_device_is_touched(native):
    """The resident form with made-up, never dereferenced pointers: every argument error returns without a launch."""
    lib = native.lib()
    ok, bad = bad_params(native)
    f64 = native._f64p
    one = lib.apap_local_model_workspace_bytes(8, 1)
    P, V, W = 0x10000, 0x20000, 0x40000          # aligned, fake

    def call(pc=P, po=P + 256, mw=None, n=8, v=V, cells=3, gamma=0.5, sigma=100.0, params=ok, H=P + 512, info=None, status=None,
             work=W, work_bytes=None):
        return lib.apap_local_model_solve_device(None, pc, po, mw, n, v, cells, gamma, sigma,
                                                 None if params is None else params.ctypes.data_as(f64), H, info, status, work,
                                                 3 * one if work_bytes is None else work_bytes, None)

    E = native.ERR_INVALID_ARG
    assert call(pc=None) == call(po=None) == call(v=None) == call(H=None) == call(work=None) == call(params=None) == E
    assert call(n=0) == call(n=-1) == call(cells=0) == call(cells=-2) == call(cells=native.LOCAL_MODEL_MAX_CELLS + 1) == E
    assert call(sigma=0.0) == call(sigma=-1.0) == call(sigma=float("nan")) == call(gamma=float("nan")) == E
    for p, what in bad:
        assert call(params=p) == E, what
    assert call(work_bytes=one - 1) == native.ERR_WORKSPACE and call(work_bytes=0) == native.ERR_WORKSPACE
    assert "one cell" in native.last_error()
    assert call(work=W + 8) == E and "aligned" in native.last_error()             # misaligned workspace
    assert call(pc=P + 4) == E and call(po=P + 260) == E and call(v=V + 4) == E   # misaligned points / vertices


def test_bad_params_are_refused_with_or_without_a_device(native):
    pc, po, v = problem()
    bad = native.model_params(native.MODEL_SDP)
    bad[0] = 3
    with pytest.raises(native.ApapValueError):
        native.local_model_solve(pc, po, v, 0.5, 100.0, bad)


def test_no_cpu_fallback(native):
    if native.lib().apap_device_count() > 0:
        pytest.skip("a GPU is visible")
    pc, po, v = problem()
    H = np.zeros((len(v), 9), np.float32)
    code = host_call(native, pc, po, None, len(pc), v, len(v), 0.5, 100.0, native.model_params(native.MODEL_LMS), H)
    assert code == native.ERR_NO_DEVICE and np.isnan(H).all()
    with pytest.raises(native.ApapError) as e:
        native.local_model_solve(pc, po, v, 0.5, 100.0, native.model_params(native.MODEL_SDP, 0.5, 0.5))
    assert e.value.code == native.ERR_NO_DEVICE
    from cvx_proj_amd.apap import APAP
    with pytest.raises(native.ApapError) as e:
        APAP(0.5, 100.0, [64, 64], [0, 0]).local_robust_homography(pc, po, v.reshape(1, 3, 2))
    assert e.value.code == native.ERR_NO_DEVICE


def test_python_argument_errors(native):
    from cvx_proj_amd.apap import APAP
    pc, po, v = problem()
    eng = APAP(0.5, 100.0, [64, 64], [0, 0])
    for bad_v in (np.zeros((2, 2, 3)), np.zeros(7), np.float64(1.0)):
        with pytest.raises(ValueError, match="vertices"):
            eng.local_robust_homography(pc, po, bad_v)
        with pytest.raises(ValueError, match="vertices"):
            native.local_model_solve(pc, po, bad_v, 0.5, 100.0, native.model_params(native.MODEL_LMS))
    for bad_w in (np.ones(len(pc) - 1, np.float32), np.ones(len(pc) + 1, np.float32), np.ones((2, len(pc)), np.float32)):
        with pytest.raises(ValueError, match="match_weights"):
            eng.local_robust_homography(pc, po, v.reshape(1, 3, 2), bad_w)
    with pytest.raises(ValueError):
        eng.local_robust_homography(pc, po[:-1], v.reshape(1, 3, 2))
    with pytest.raises(ValueError):
        native.local_model_solve(pc, po, v, 0.5, 100.0, np.zeros(5))
    # no cell: nothing to solve, nothing to touch
    H, info, status = native.local_model_solve(pc, po, np.zeros((0, 2)), 0.5, 100.0, native.model_params(native.MODEL_LMS))
    assert H.shape == (0, 3, 3) and info.shape == (0, native.MODEL_INFO) and status.shape == (0,)


def test_the_weight_has_one_definition():
    """sqrt_pos, exp_nonpos and cell_weight were moved to a shared header, not copied."""
    csrc = os.path.join(ROOT, "cvx_proj_amd", "csrc")
    kernels = open(os.path.join(csrc, "apap_kernels.hip")).read()
    local = open(os.path.join(csrc, "apap_local_model.hip")).read()
    header = open(os.path.join(csrc, "apap_weight_dev.h")).read()
    for fn in ("sqrt_pos", "exp_nonpos", "cell_weight"):
        assert len(re.findall(rf"double {fn}\(", header)) == 1, fn
        assert not re.search(rf"double {fn}\(", kernels) and not re.search(rf"double {fn}\(", local), fn
    assert '#include "apap_weight_dev.h"' in kernels and '#include "apap_weight_dev.h"' in local
