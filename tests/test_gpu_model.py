"""The M-step and the EM loop on the MI355X, checked by certificates computed in numpy from the original rows
(tests/model_spec.py): cvxpy is not needed.  SDP: phi(h) - psi(Z) <= 1e-9 phi(h) and r + t = phi(h) to 1e-9; LMS: numpy's
float64 lstsq to 1e-9 in equilibrated coordinates; the float32 H is the numpy tail of the engine's h, bit for bit; the EM loop
is the composition of the public calls, bit for bit, on either path and on every run."""
import glob
import os
import warnings

import numpy as np
import pytest

from conftest import GOLDEN
import model_spec as S

pytestmark = pytest.mark.gpu

FIXTURES = sorted(glob.glob(os.path.join(GOLDEN, "spectral_*.npz")))


def selected(path):
    g = np.load(path)
    return S.select(g["src"], g["dst"], g["ransac_mask"])


SOLVABLE = [p for p in FIXTURES if len(selected(p)[0]) >= 4]
SMALL = [p for p in FIXTURES if len(selected(p)[0]) < 4]


def synthetic(kind, n=400, seed=0):
    rng = np.random.default_rng(seed)
    pc = (rng.random((n, 2)) * np.float32([1280, 960])).astype(np.float32)
    Ht = np.array([[0.97, 0.04, 35.0], [-0.03, 1.01, -12.0], [2e-5, -1e-5, 1.0]])
    q = np.hstack([pc.astype(np.float64), np.ones((n, 1))]) @ Ht.T
    po = q[:, :2] / q[:, 2:]
    if kind != "exact":
        po = po + rng.normal(0, 1.0, po.shape)
    if kind == "outliers":
        bad = rng.random(n) < 0.2
        po[bad] = rng.random((bad.sum(), 2)) * 1000
    w = (rng.random(n) * 0.9 + 0.1).astype(np.float32)
    return pc, po.astype(np.float32), w, Ht


CASES = [(os.path.basename(p), p) for p in SOLVABLE] + [("synthetic_" + k, k) for k in ("exact", "noisy", "outliers")]


def case(spec):
    if spec in ("exact", "noisy", "outliers"):
        pc, po, w, _ = synthetic(spec)
        return pc, po, w
    return selected(spec)


@pytest.fixture(scope="module")
def native_gpu(native):
    if native.lib().apap_device_count() < 1:
        pytest.skip("no HIP device")
    return native


def solve(native, pc, po, w, mode, du=1.0, dv=1.0, swap=True):
    return native.model_solve(pc, po, w, native.model_params(mode, du, dv, floor=None, swap=swap))


def h_of(info, native):
    return info[native.MODEL_INFO_H:native.MODEL_INFO_H + 8]


@pytest.mark.parametrize("name,spec", CASES, ids=[c[0] for c in CASES])
@pytest.mark.parametrize("fluc", [0.2, 0.5, 1.25])
def test_sdp_certificate(native_gpu, name, spec, fluc):
    native = native_gpu
    pc, po, w = case(spec)
    H, info = solve(native, pc, po, w, native.MODEL_SDP, fluc, fluc)
    h = h_of(info, native)
    status = int(info[native.MODEL_INFO_STATUS])
    gap = info[native.MODEL_INFO_GAP]
    assert status == 0 and gap <= 1e-10, (status, gap, info[native.MODEL_INFO_ITERS])
    Z = info[native.MODEL_INFO_Z:native.MODEL_INFO_Z + 9].reshape(3, 3)
    ph = S.phi(pc, po, w, h, fluc, fluc)
    ps = S.psi(pc, po, w, Z, fluc, fluc)
    assert ps <= ph * (1 + 1e-12)
    assert ph - ps <= 1e-9 * ph, (ph, ps, (ph - ps) / ph)
    rt = info[native.MODEL_INFO_R] + info[native.MODEL_INFO_T]
    assert abs(rt - ph) <= 1e-9 * ph and info[native.MODEL_INFO_OBJECTIVE] == rt
    assert int(info[native.MODEL_INFO_COUNT]) == len(pc)
    np.testing.assert_array_equal(H, S.tail(h, True))


@pytest.mark.parametrize("name,spec", CASES, ids=[c[0] for c in CASES])
def test_lms_is_least_squares(native_gpu, name, spec):
    native = native_gpu
    pc, po, w = case(spec)
    H, info = solve(native, pc, po, w, native.MODEL_LMS, swap=False)
    h = h_of(info, native)
    A, rhs, _, _ = S.rows(pc, po, w)
    A = A.astype(np.float64)
    b = rhs.astype(np.float64).ravel()
    cn = np.sqrt((A * A).sum(axis=0))
    ref = np.linalg.lstsq(A / cn, b, rcond=None)[0]
    assert np.abs(h * cn - ref).max() <= 1e-9 * max(np.abs(ref).max(), 1.0)
    res = b - A @ h
    assert np.abs((A / cn).T @ res).max() <= 1e-12 * np.linalg.norm(b) * np.sqrt(len(b))   # normal equations at rounding level
    assert abs(info[native.MODEL_INFO_OBJECTIVE] - res @ res) <= 1e-6 * max(res @ res, 1e-300) + 1e-9 * (b @ b) * 1e-12
    np.testing.assert_array_equal(H, S.tail(h, False))
    H2, info2 = solve(native, pc, po, w, native.MODEL_LMS, swap=True)
    np.testing.assert_array_equal(h_of(info2, native), h)
    np.testing.assert_array_equal(H2, S.tail(h, True))


def test_lms_exact_homography(native_gpu):
    native = native_gpu
    pc, po, w, Ht = synthetic("exact", n=300, seed=3)
    _, info = solve(native, pc, po, w, native.MODEL_LMS)
    h = h_of(info, native)
    # float32 points: the fit is exact to the points' rounding
    assert np.abs(h - Ht.ravel()[:8]).max() <= 1e-5 * np.abs(Ht.ravel()[:8]).max()
    A, rhs, _, _ = S.rows(pc, po, w)
    assert np.abs(A.astype(np.float64) @ h - rhs.ravel()).max() <= 1e-3


@pytest.mark.parametrize("spec", ["noisy"] + [p for p in SOLVABLE if "n500.npz" in p], ids=os.path.basename)
def test_sdp_tends_to_lms(native_gpu, spec):
    native = native_gpu
    pc, po, w = case(spec)
    _, i_sdp = solve(native, pc, po, w, native.MODEL_SDP, 1e-7, 1e-7)
    _, i_lms = solve(native, pc, po, w, native.MODEL_LMS)
    A = S.rows(pc, po, w)[0].astype(np.float64)
    cn = np.sqrt((A * A).sum(axis=0))
    a, b = h_of(i_sdp, native) * cn, h_of(i_lms, native) * cn
    assert np.abs(a - b).max() <= 1e-6 * np.abs(b).max()


def test_model_is_deterministic(native_gpu):
    native = native_gpu
    pc, po, w = case("outliers")
    a = solve(native, pc, po, w, native.MODEL_SDP, 0.5, 0.5)
    b = solve(native, pc, po, w, native.MODEL_SDP, 0.5, 0.5)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


def test_solver_classes(native_gpu, capsys):
    from cvx_proj_amd.model import SDPSolver, LMSSolver
    pc, po, w = case("noisy")
    H = SDPSolver(8000, 0.5, 0.5).solve(pc, po, w, verbose=1)
    out = capsys.readouterr().out
    assert f"Start solving SDP Problem... point num: {len(pc)}" in out and "The optimal value is" in out
    s = SDPSolver(8000, 0.5, 0.5)
    H2 = s.solve(pc, po, w, verbose=0)
    assert np.array_equal(H, H2) and H.dtype == np.float32 and s.last.gap <= 1e-10 and s.last.iterations > 0
    np.testing.assert_array_equal(H, S.tail(s.last.h, True))
    lm = LMSSolver(8000)
    Hl = lm.solve(pc, po, w, verbose=0, swap=False)
    assert Hl[2, 2] == 1.0 and lm.last.iterations == 0


@pytest.mark.parametrize("path", SMALL, ids=os.path.basename)
def test_fewer_than_four_matches(native_gpu, path):
    native = native_gpu
    pc, po, w = selected(path)
    with pytest.raises(native.ApapValueError) as e:
        solve(native, pc, po, w, native.MODEL_SDP, 0.5, 0.5)
    info = e.value.info
    assert int(info[native.MODEL_INFO_STATUS]) & native.STATUS_MODEL_DEGENERATE
    assert int(info[native.MODEL_INFO_COUNT]) == len(pc)
    assert np.isnan(info[native.MODEL_INFO_H:native.MODEL_INFO_H + 8]).all()


def test_three_points_and_collinear(native_gpu):
    native = native_gpu
    pc = np.float32([[10, 20], [30, 5], [50, 70]])
    with pytest.raises(native.ApapValueError):
        solve(native, pc, pc + 3, np.ones(3, np.float32), native.MODEL_LMS)
    x = np.arange(12, dtype=np.float32) * 16
    line = np.stack([x, 2 * x + 8], axis=1).astype(np.float32)      # exactly collinear in float32
    for mode in (native.MODEL_LMS, native.MODEL_SDP):
        with pytest.raises(native.ApapValueError) as e:
            solve(native, line, line + np.float32([5, 3]), np.ones(12, np.float32), mode, 0.5, 0.5)
        assert int(e.value.info[native.MODEL_INFO_STATUS]) & native.STATUS_MODEL_DEGENERATE
        assert int(e.value.info[native.MODEL_INFO_COUNT]) == 12


def test_all_weights_below_the_floor(native_gpu):
    from cvx_proj_amd import spectral_method as SM
    native = native_gpu
    pc, po, w, _ = synthetic("noisy", n=50)

    class KP:
        def __init__(self, p):
            self.pt = (float(p[0]), float(p[1]))

    class DM:
        def __init__(self, i):
            self.queryIdx = self.trainIdx = i
    kc, ko, m = [KP(p) for p in pc], [KP(p) for p in po], [DM(i) for i in range(50)]
    with pytest.raises(IndexError):
        SM.model_solve(kc, ko, m, np.full(50, 9e-4, np.float32), param=0.5, lms=False)
    with pytest.raises(NotImplementedError):
        SM.model_solve(kc, ko, m, w)                       # the reference's defaults: lms=True, param 0.5 = Huber
    H = SM.model_solve(kc, ko, m, w, param=0.5, lms=False)
    H_direct, _ = native.model_solve(pc, po, w, native.model_params(native.MODEL_SDP, 0.5, 0.5))
    assert np.array_equal(H, H_direct)
    # the floor: weights at or below 1e-3 are dropped, the rest kept in order
    w2 = w.copy()
    w2[::3] = 1e-4
    w2[1::7] = 1e-3     # float32(1e-3) > 1e-3 in float64 (numpy 1.x compares the float32 scalar so): kept
    Hf = SM.model_solve(kc, ko, m, w2, param=0.5, lms=False)
    keep = w2.astype(np.float64) > 1e-3
    Hk, _ = native.model_solve(pc[keep], po[keep], w2[keep], native.model_params(native.MODEL_SDP, 0.5, 0.5, floor=None))
    assert np.array_equal(Hf, Hk)


# ---------------------------------------------------------------- the EM loop
def load(path):
    g = dict(np.load(path))
    if "codebook" in g:
        g["c_feats"], g["o_feats"] = g["codebook"][g["c_index"]], g["codebook"][g["o_index"]]
    g["c"] = g["c_feats"].astype(np.float32)
    g["o"] = g["o_feats"].astype(np.float32)
    return g


def kw(g):
    e, a, t, r, s = (float(x) for x in g["opts"])
    return dict(epi_weight=e, affinity_eps=a, aff_thresh=t, em_radius=r, score_thresh=s)


EM_FIXTURES = [p for p in FIXTURES if os.path.basename(p) in ("spectral_n500.npz", "spectral_n2000.npz")]


class KP:
    def __init__(self, p):
        self.pt = (float(p[0]), float(p[1]))


class DM:
    def __init__(self, i):
        self.queryIdx = self.trainIdx = i


@pytest.mark.parametrize("path", EM_FIXTURES, ids=os.path.basename)
@pytest.mark.parametrize("lms", [False, True])
def test_em_is_the_composition(native_gpu, path, lms):
    from cvx_proj_amd import spectral_method as SM
    g = load(path)
    n = len(g["src"])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        em = SM.spectral_em(g["src"], g["dst"], g["c"], g["o"], g["F"], em_steps=3, lms=lms, fluc=0.5, mask=g["mask"], **kw(g))
        kc, ko, m = [KP(p) for p in g["src"]], [KP(p) for p in g["dst"]], [DM(i) for i in range(n)]
        Hg, mask = None, g["mask"]
        for k in range(3):
            r = SM.spectral_weights(g["src"], g["dst"], g["c"], g["o"], g["F"], Hg=Hg, mask=None if Hg is not None else mask, **kw(g))
            H = SM.model_solve(kc, ko, m, r.ransac_mask, param=-1.0 if lms else 0.5, lms=lms)
            got = em.rounds[k]
            assert got.H_pred.tobytes() == H.tobytes(), k
            for a, b in zip(got.spectral, r):
                if isinstance(a, np.ndarray):
                    assert a.tobytes() == b.tobytes(), k
                elif a is not None and b is not None:
                    assert a == b or (a != a and b != b), k
            Hg = H
    H_save = np.linalg.inv(em.rounds[-1].H_pred).astype(np.float64)
    H_save /= H_save[-1, -1]
    assert em.H_save.tobytes() == H_save.tobytes()


def test_em_resident_equals_host_and_repeats(native_gpu):
    import torch
    from cvx_proj_amd import resident
    native = native_gpu
    g = load([p for p in FIXTURES if "n2000" in p][0])
    sp = native.spectral_params(**kw(g))
    mp = native.model_params(native.MODEL_SDP, 0.5, 0.5)
    host = native.spectral_em(g["src"], g["dst"], g["c"], g["o"], g["F"], sp, mp, 2, g["mask"])
    host2 = native.spectral_em(g["src"], g["dst"], g["c"], g["o"], g["F"], sp, mp, 2, g["mask"])
    for a, b in zip(host, host2):
        assert a.tobytes() == b.tobytes()
    dev = torch.device("cuda", 0)
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)      # noqa: E731
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    out = resident.hip_spectral_em(t(g["src"], np.float32), t(g["dst"], np.float32), t(g["c"], np.float32), t(g["o"], np.float32),
                                   t(g["F"], np.float64), sp, mp, 2, t(g["mask"], np.float32), status=status)
    torch.cuda.synchronize()
    for a, b in zip(out, host):
        assert a.cpu().numpy().tobytes() == b.tobytes()
    assert int(status.item()) & ~native.STATUS_NO_CONVERGENCE == 0
