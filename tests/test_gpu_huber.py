"""The Huber M-step on the MI355X (mode APAP_MODEL_HUBER), checked by the duality gap recomputed in numpy's extended precision
from the original rows (tests/huber_spec.py): the certificate does not depend on the kernel's method.  Inputs:
tests/huber_cases.py, whose edges tests/test_huber_inputs.py confirms on the specification."""
import ctypes
import os
import warnings

import numpy as np
import pytest

from conftest import GOLDEN
import huber_cases as HC
import huber_spec as HS
import model_spec as S

pytestmark = pytest.mark.gpu

CASES = HC.cases()
GUARD = 64          # float32 / float64 guard elements on either side of H and info


@pytest.fixture(scope="module")
def native_gpu(native):
    if native.lib().apap_device_count() < 1:
        pytest.skip("no HIP device")
    return native


def params_of(native, c, mode=None, swap=True):
    return native.model_params(native.MODEL_HUBER if mode is None else mode, c["M"], floor=c["floor"], swap=swap, max_iter=c["cap"])


def rows_of(c):
    pc, po, w = S.select(c["pc"], c["po"], c["w"], c["floor"])
    return HS.problem(pc, po, w)


def device_form(native, c, params, dirty=0xA5):
    """apap_model_solve_device itself: H and info sit inside guarded buffers, the workspace is filled with ``dirty`` bytes.
    Returns (H, info, status word, guards intact)."""
    import torch
    dev = torch.device("cuda", 0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)      # noqa: E731
    pc, po, w = t(c["pc"]), t(c["po"]), t(c["w"])
    n = len(c["pc"])
    Hb = torch.full((2 * GUARD + 9,), -7.0, dtype=torch.float32, device=dev)
    Ib = torch.full((2 * GUARD + native.MODEL_INFO,), -7.0, dtype=torch.float64, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    nbytes = native.lib().apap_model_workspace_bytes(n)
    work = torch.full((nbytes + 256,), dirty, dtype=torch.uint8, device=dev)
    off = (-work.data_ptr()) % 256
    rc = native.lib().apap_model_solve_device(
        None, pc.data_ptr(), po.data_ptr(), w.data_ptr(), n, params.ctypes.data_as(native._f64p),
        Hb.data_ptr() + 4 * GUARD, Ib.data_ptr() + 8 * GUARD, status.data_ptr(), work.data_ptr() + off, nbytes,
        ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    native.check(rc)
    torch.cuda.synchronize()
    Hh, Ih = Hb.cpu().numpy(), Ib.cpu().numpy()
    intact = bool((Hh[:GUARD] == -7).all() and (Hh[GUARD + 9:] == -7).all() and (Ih[:GUARD] == -7).all()
                  and (Ih[GUARD + native.MODEL_INFO:] == -7).all())
    return Hh[GUARD:GUARD + 9].reshape(3, 3), Ih[GUARD:GUARD + native.MODEL_INFO], int(status.item()), intact


def resident_form(native, c, params):
    import torch
    from cvx_proj_amd import resident
    dev = torch.device("cuda", 0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)      # noqa: E731
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    H, info = resident.hip_model_solve(t(c["pc"]), t(c["po"]), t(c["w"]), params, status=status)
    torch.cuda.synchronize()
    return H.cpu().numpy(), info.cpu().numpy(), int(status.item())


def same(a, b):
    return a.tobytes() == b.tobytes()


def h_of(info, native):
    return info[native.MODEL_INFO_H:native.MODEL_INFO_H + 8]


@pytest.mark.parametrize("name", HC.CONVERGING)
def test_converging_case(native_gpu, name):
    native = native_gpu
    c = CASES[name]
    p = params_of(native, c)
    H, info = native.model_solve(c["pc"], c["po"], c["w"], p)
    H2, info2 = native.model_solve(c["pc"], c["po"], c["w"], p)
    Hd, infod, status_d, intact = device_form(native, c, p)
    Hd2, infod2, _, intact2 = device_form(native, c, p, dirty=0x3C)
    Hr, infor, status_r = resident_form(native, c, p)
    for Hx, ix in ((H2, info2), (Hd, infod), (Hd2, infod2), (Hr, infor)):
        assert same(H, Hx) and same(info, ix)
    assert intact and intact2
    A, rhs = rows_of(c)
    h = h_of(info, native)
    gap = HS.gap(A, rhs, h, c["M"])
    f = float(HS.objective(A, rhs, h, c["M"]))
    print(f"{name}: steps {int(info[native.MODEL_INFO_ITERS])} reported gap {info[native.MODEL_INFO_GAP]:.3e} extended {gap:.3e} "
          f"f {info[native.MODEL_INFO_OBJECTIVE]:.12g}")
    assert int(info[native.MODEL_INFO_STATUS]) == 0 and status_d == 0 and status_r == 0
    assert info[native.MODEL_INFO_GAP] <= 1e-10
    assert gap <= 1e-9
    assert abs(info[native.MODEL_INFO_OBJECTIVE] - f) <= 1e-12 * f
    assert int(info[native.MODEL_INFO_COUNT]) == len(rhs) // 2
    assert 1 <= info[native.MODEL_INFO_ITERS] <= 100 or name == "n5"
    assert np.isnan(info[[native.MODEL_INFO_R, native.MODEL_INFO_T]]).all()
    assert np.isnan(info[native.MODEL_INFO_Z:native.MODEL_INFO_Z + 9]).all()
    np.testing.assert_array_equal(H, S.tail(h, True))
    # the specification reaches the same optimum
    spec = HS.solve_points(c["pc"], c["po"], c["w"], c["M"], HS.DEFAULT_CAP, c["floor"])[2]
    assert abs(spec.f - f) <= 1e-9 * f


def test_swap_off_is_the_same_h(native_gpu):
    native = native_gpu
    c = CASES["moderate_2000"]
    _, a = native.model_solve(c["pc"], c["po"], c["w"], params_of(native, c, swap=True))
    H, b = native.model_solve(c["pc"], c["po"], c["w"], params_of(native, c, swap=False))
    assert same(h_of(a, native), h_of(b, native))
    np.testing.assert_array_equal(H, S.tail(h_of(b, native), False))


@pytest.mark.parametrize("name", ["M_1e6", "n4"])
def test_nothing_clipped_is_least_squares(native_gpu, name):
    """No row clipped at the least-squares solution: it is returned untouched, H byte for byte mode LMS's."""
    native = native_gpu
    c = CASES[name]
    H, info = native.model_solve(c["pc"], c["po"], c["w"], params_of(native, c))
    Hl, infol = native.model_solve(c["pc"], c["po"], c["w"], params_of(native, c, mode=native.MODEL_LMS))
    Hd, infod, _, intact = device_form(native, c, params_of(native, c))
    assert same(H, Hl) and same(h_of(info, native), h_of(infol, native)) and same(H, Hd) and same(info, infod) and intact
    assert info[native.MODEL_INFO_ITERS] == 0 and np.isfinite(H).all()
    gap = info[native.MODEL_INFO_GAP]
    assert bool(int(info[native.MODEL_INFO_STATUS]) & native.STATUS_MODEL_NO_CONVERGENCE) == bool(gap > 1e-10)
    A, rhs = rows_of(c)
    f = float(HS.objective(A, rhs, h_of(info, native), c["M"]))
    if name == "M_1e6":
        assert int(info[native.MODEL_INFO_STATUS]) == 0
        assert HS.gap(A, rhs, h_of(info, native), c["M"]) <= 1e-9
        assert abs(info[native.MODEL_INFO_OBJECTIVE] - f) <= 1e-12 * f
    else:
        # four matches: an exact fit, f is the rounding noise of the residuals (and so is its relative gap)
        assert info[native.MODEL_INFO_OBJECTIVE] <= 1e-18 * float(rhs @ rhs) and f <= 1e-18 * float(rhs @ rhs)


@pytest.mark.parametrize("name", HC.HARD)
def test_hard_case(native_gpu, name):
    """The cap at 1 and the near-L1 problem with gross outliers: the status follows the reported gap, which bounds the true
    one, and no step has raised f."""
    native = native_gpu
    c = CASES[name]
    p = params_of(native, c)
    H, info = native.model_solve(c["pc"], c["po"], c["w"], p)
    Hd, infod, status_d, intact = device_form(native, c, p)
    assert same(H, Hd) and same(info, infod) and intact
    word = int(info[native.MODEL_INFO_STATUS])
    reported = info[native.MODEL_INFO_GAP]
    A, rhs = rows_of(c)
    h = h_of(info, native)
    gap = HS.gap(A, rhs, h, c["M"])
    pc, po, w = S.select(c["pc"], c["po"], c["w"], c["floor"])
    f0 = float(HS.objective(A, rhs, S.solve(pc, po, w, "lms")[0], c["M"]))
    f = float(HS.objective(A, rhs, h, c["M"]))
    print(f"{name}: steps {int(info[native.MODEL_INFO_ITERS])} reported gap {reported:.3e} extended {gap:.3e} f {f:.9g} f(h0) {f0:.9g}")
    assert np.isfinite(H).all() and np.isfinite(h).all()
    assert bool(word & native.STATUS_MODEL_NO_CONVERGENCE) == bool(reported > 1e-10) and word == status_d
    assert word & ~native.STATUS_MODEL_NO_CONVERGENCE == 0
    assert gap <= max(1e-9, 10 * reported)
    assert f <= f0 * (1 + 1e-12)       # h0 here is numpy's least-squares solution: the engine's agrees to rounding
    assert 1 <= info[native.MODEL_INFO_ITERS] <= (c["cap"] or 100)
    assert abs(info[native.MODEL_INFO_OBJECTIVE] - f) <= 1e-12 * f
    np.testing.assert_array_equal(H, S.tail(h, True))


def test_cap_warns_through_the_solver_class(native_gpu, capsys):
    from cvx_proj_amd.model import HuberSolver
    c = CASES["M_0p011_gross"]
    s = HuberSolver(8000, c["M"])
    with pytest.warns(RuntimeWarning, match="Huber"):
        H = s.solve(c["pc"], c["po"], c["w"], verbose=1)
    out = capsys.readouterr().out
    assert f"Start solving... point num: {len(c['pc'])}. Huber Loss Used = [True]" in out and "The optimal value is" in out
    assert s.last.status & native_gpu.STATUS_MODEL_NO_CONVERGENCE and 1 <= s.last.iterations <= 100 and np.isfinite(H).all()


def test_solver_class_and_model_solve(native_gpu):
    from cvx_proj_amd import spectral_method as SM
    from cvx_proj_amd.model import HuberSolver, ModelResult
    native = native_gpu
    c = CASES["empty_fold"]
    keep = c["w"].astype(np.float64) > 1e-3
    s = HuberSolver(8000, 0.5)
    H = s.solve(c["pc"][keep], c["po"][keep], c["w"][keep], verbose=0)
    assert isinstance(s.last, ModelResult) and s.last.status == 0 and s.last.gap <= 1e-10 and s.last.count == keep.sum()
    He, _ = native.model_solve(c["pc"], c["po"], c["w"], params_of(native, c))
    assert same(H, He)

    class KP:
        def __init__(self, p):
            self.pt = (float(p[0]), float(p[1]))

    class DM:
        def __init__(self, i):
            self.queryIdx = self.trainIdx = i
    n = len(c["pc"])
    kc, ko, m = [KP(p) for p in c["pc"]], [KP(p) for p in c["po"]], [DM(i) for i in range(n)]
    assert same(SM.model_solve(kc, ko, m, c["w"], param=0.5, loss="huber"), H)
    with pytest.raises(NotImplementedError):
        SM.model_solve(kc, ko, m, c["w"], param=0.5)


@pytest.mark.parametrize("name", HC.DEGENERATE)
def test_degenerate_as_least_squares(native_gpu, name):
    native = native_gpu
    c = CASES[name]
    out = []
    for mode in (native.MODEL_HUBER, native.MODEL_LMS):
        with pytest.raises(native.ApapValueError) as e:
            native.model_solve(c["pc"], c["po"], c["w"], params_of(native, c, mode=mode))
        out.append((str(e.value), e.value.info))
    (msg_h, info_h), (msg_l, info_l) = out
    assert msg_h == msg_l and same(info_h, info_l)
    assert int(info_h[native.MODEL_INFO_STATUS]) == native.STATUS_MODEL_DEGENERATE
    assert int(info_h[native.MODEL_INFO_COUNT]) == len(c["pc"]) and np.isnan(h_of(info_h, native)).all()
    H, info, status, intact = device_form(native, c, params_of(native, c))
    assert np.isnan(H).all() and status == native.STATUS_MODEL_DEGENERATE and same(info, info_l) and intact


# ---------------------------------------------------------------- the EM loop
def load(path):
    g = dict(np.load(path))
    if "codebook" in g:
        g["c_feats"], g["o_feats"] = g["codebook"][g["c_index"]], g["codebook"][g["o_index"]]
    g["c"] = g["c_feats"].astype(np.float32)
    g["o"] = g["o_feats"].astype(np.float32)
    return g


def test_em_is_the_composition(native_gpu):
    from cvx_proj_amd import resident, spectral_method as SM
    import torch
    native = native_gpu
    g = load(os.path.join(GOLDEN, "spectral_n500.npz"))
    e, a, t, r, s = (float(x) for x in g["opts"])
    kw = dict(epi_weight=e, affinity_eps=a, aff_thresh=t, em_radius=r, score_thresh=s)
    n = len(g["src"])

    class KP:
        def __init__(self, p):
            self.pt = (float(p[0]), float(p[1]))

    class DM:
        def __init__(self, i):
            self.queryIdx = self.trainIdx = i
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        em = SM.spectral_em(g["src"], g["dst"], g["c"], g["o"], g["F"], em_steps=2, lms=True, huber_param=0.5, loss="huber",
                            mask=g["mask"], **kw)
        kc, ko, m = [KP(p) for p in g["src"]], [KP(p) for p in g["dst"]], [DM(i) for i in range(n)]
        Hg = None
        for k in range(2):
            res = SM.spectral_weights(g["src"], g["dst"], g["c"], g["o"], g["F"], Hg=Hg, mask=None if Hg is not None else g["mask"],
                                      **kw)
            H = SM.model_solve(kc, ko, m, res.ransac_mask, param=0.5, lms=True, loss="huber")
            got = em.rounds[k]
            assert same(got.H_pred, H), k
            assert same(got.spectral.ransac_mask, res.ransac_mask) and same(got.spectral.segment, res.segment), k
            assert np.isnan(got.model.r) and got.model.iterations >= 1, k
            Hg = H
    # the resident form: the same bytes, no host wait in between
    dev = torch.device("cuda", 0)
    tt = lambda x, dt: torch.from_numpy(np.ascontiguousarray(x, dtype=dt)).to(dev)      # noqa: E731
    sp = native.spectral_params(**kw)
    mp = native.model_params(native.MODEL_HUBER, 0.5)
    out = resident.hip_spectral_em(tt(g["src"], np.float32), tt(g["dst"], np.float32), tt(g["c"], np.float32), tt(g["o"], np.float32),
                                   tt(g["F"], np.float64), sp, mp, 2, tt(g["mask"], np.float32))
    torch.cuda.synchronize()
    for k in range(2):
        assert same(out[0][k].cpu().numpy(), em.rounds[k].H_pred), k
