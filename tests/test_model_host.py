"""The M-step without a GPU: the reduction of the reference's (2n+3)-sized LMI to 18 x 18, the numpy rehearsal of the
interior-point method against its certificate on the spectral fixtures, and the C ABI's new symbols, constants and
refusals (tests/model_spec.py is the specification)."""
import glob
import os
import re

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
import model_spec as S

FIXTURES = sorted(glob.glob(os.path.join(GOLDEN, "spectral_*.npz")))


def random_problem(rng, n):
    pc = (rng.random((n, 2)) * 1000).astype(np.float32)
    H = np.array([[1.02, 0.03, 12.0], [-0.02, 0.98, -7.0], [1e-5, -2e-5, 1.0]])
    q = np.hstack([pc, np.ones((n, 1))]) @ H.T
    po = (q[:, :2] / q[:, 2:] + rng.normal(0, 1.5, (n, 2))).astype(np.float32)
    w = rng.random(n).astype(np.float32) * 0.9 + 0.1
    return pc, po, w


@pytest.mark.parametrize("seed", range(4))
def test_reduction_identity(seed):
    """R^T R = K^T K to rounding, and PSD of the full LMI agrees with PSD of the 18 x 18 one away from the boundary."""
    rng = np.random.default_rng(seed)
    n = 6 + seed * 3
    pc, po, w = random_problem(rng, n)
    du = dv = 0.5
    K, R = S.reduced(pc, po, w, du, dv)
    G = K.T @ K
    assert np.abs(R.T @ R - G).max() <= 1e-12 * np.abs(G).max()
    A, rhs, A1, A2 = S.rows(pc, po, w, du, dv)
    h0 = np.linalg.lstsq(A.astype(np.float64), rhs.astype(np.float64).ravel(), rcond=None)[0]
    agree = 0
    for _ in range(40):
        h = h0 * (1 + 0.05 * rng.normal(size=8))
        X = np.zeros((15, 3))
        X[:8, 2], X[8, 2], X[9:12, 0], X[12:15, 1] = h, 1.0, h[[0, 3, 6]], h[[1, 4, 7]]
        P = K @ X
        lam = np.linalg.eigvalsh(P.T @ P).max()
        r, t = np.exp(rng.uniform(np.log(lam) - 2, np.log(lam) + 2, 2))
        D = np.diag([r, r, t])
        full = np.block([[np.eye(2 * n), P], [P.T, D]])
        small = np.block([[np.eye(15), R @ X], [(R @ X).T, D]])
        ef, es = np.linalg.eigvalsh(full).min(), np.linalg.eigvalsh(small).min()
        margin = np.linalg.eigvalsh(D - P.T @ P).min()
        if abs(margin) < 1e-6 * lam:
            continue
        assert (ef >= 0) == (es >= 0) == (margin >= 0)
        agree += 1
    assert agree >= 20


def load_selected(path):
    g = np.load(path)
    return S.select(g["src"], g["dst"], g["ransac_mask"])


@pytest.mark.parametrize("path", [p for p in FIXTURES if len(load_selected(p)[0]) >= 4 and "n2000" not in p and "n5000" not in p],
                         ids=os.path.basename)
def test_numpy_ipm_certificate(path):
    """The rehearsal of the kernel's interior-point method reaches the 1e-10 gap, and the certificate psi(Z) closes phi(h)
    to 1e-9 from the original rows."""
    pc, po, w = load_selected(path)
    for fluc in (0.2, 0.5, 1.25):
        h, r, t, Z, gap, it = S.solve(pc, po, w, "sdp", fluc, fluc)
        assert gap <= S.GAP_TOL and it < S.MAX_IT
        ph = S.phi(pc, po, w, h, fluc, fluc)
        ps = S.psi(pc, po, w, Z, fluc, fluc)
        assert ps <= ph * (1 + 1e-12)
        assert ph - ps <= 1e-9 * ph, (fluc, ph, ps)
        assert abs(r + t - ph) <= 1e-9 * ph


def test_numpy_lms_is_least_squares():
    rng = np.random.default_rng(5)
    pc, po, w = random_problem(rng, 50)
    h = S.solve(pc, po, w, "lms")[0]
    A, rhs, _, _ = S.rows(pc, po, w)
    ref = np.linalg.lstsq(A.astype(np.float64), rhs.astype(np.float64).ravel(), rcond=None)[0]
    cn = np.sqrt((A.astype(np.float64) ** 2).sum(axis=0))
    assert np.abs((h - ref) * cn).max() <= 1e-9 * np.abs(ref * cn).max()


def test_guarded_ipm_on_near_collinear_points():
    """The reference's own standing on the 72 near-collinear inputs of tests/test_gpu_model_edges.py: none is degenerate
    (smallest equilibrated pivot far above the kernel's 1e-12), at most a third end above the 1e-10 gap (the Schur matrix
    loses positive definiteness first; the guarded ipm keeps the best iterate), and every certificate holds to 1e-9."""
    from test_gpu_model_edges import COLLINEAR, collinear_spec
    gap, pivot, cert, rt = collinear_spec().T
    late = int((gap > S.GAP_TOL).sum())
    print(f"near-collinear family, guarded specification: {late} of {len(COLLINEAR)} above {S.GAP_TOL:g}, largest gap "
          f"{gap.max():.3e}, smallest pivot {pivot.min():.3e}, largest (phi - psi) / phi {cert.max():.3e}, largest "
          f"|r + t - phi| / phi {rt.max():.3e}")
    assert len(COLLINEAR) == 72 and (pivot > 1e-12).all()
    assert late <= 24
    assert (cert <= 1e-9).all() and (cert >= -1e-12).all() and (rt <= 1e-9).all()


@pytest.mark.parametrize("k", [1, 3, 6])
def test_capped_ipm_keeps_the_duality_bound(k):
    """The iteration cap on the specification: the capped iterate is primal feasible (r + t >= phi) and its reported gap
    bounds the certificate, phi - psi <= gap (r + t), the conditions tests/test_gpu_model_edges.py puts on the engine."""
    from test_gpu_model import synthetic
    from test_gpu_model_edges import problem
    pc, po, w = problem(400)
    for a, b in zip((pc, po, w), synthetic("noisy", 400, 0)):
        assert a.tobytes() == b.tobytes()       # the generator extends synthetic(): the same draws
    old = S.MAX_IT
    S.MAX_IT = k
    try:
        h, r, t, Z, gap, it = S.solve(pc, po, w, "sdp", 0.5, 0.5)
    finally:
        S.MAX_IT = old
    ph, ps = S.phi(pc, po, w, h, 0.5, 0.5), S.psi(pc, po, w, Z, 0.5, 0.5)
    print(f"max_iter={k}: gap={gap:.3e} (phi - psi) / phi={(ph - ps) / ph:.3e}")
    assert it == k and gap > S.GAP_TOL
    assert r + t >= ph * (1 - 1e-12)
    assert ph - ps <= gap * (r + t) * (1 + 1e-6) + 1e-9 * ph


# ---------------------------------------------------------------- the C ABI
def header():
    return open(os.path.join(ROOT, "include", "apap_hip.h")).read()


def test_model_constants_match_the_header(native):
    text = header()
    for name, val in (("STATUS_MODEL_DEGENERATE", native.STATUS_MODEL_DEGENERATE),
                      ("STATUS_MODEL_NO_CONVERGENCE", native.STATUS_MODEL_NO_CONVERGENCE), ("MODEL_LMS", native.MODEL_LMS),
                      ("MODEL_SDP", native.MODEL_SDP), ("MODEL_PARAMS", native.MODEL_PARAMS), ("MODEL_INFO", native.MODEL_INFO),
                      ("MODEL_INFO_STATUS", native.MODEL_INFO_STATUS), ("MODEL_INFO_COUNT", native.MODEL_INFO_COUNT),
                      ("MODEL_INFO_Z", native.MODEL_INFO_Z), ("MODEL_INFO_H", native.MODEL_INFO_H)):
        assert int(re.search(rf"#define APAP_{name} (\d+)", text).group(1)) == val, name
    bits = [native.STATUS_SINGULAR, native.STATUS_INDEX, native.STATUS_UNPREPARED, native.STATUS_NO_CONVERGENCE,
            native.STATUS_MODEL_DEGENERATE, native.STATUS_MODEL_NO_CONVERGENCE]
    assert sum(bits) == 63 and len(set(bits)) == 6     # distinct bits
    for sym in ("apap_model_solve", "apap_model_solve_device", "apap_model_workspace_bytes", "apap_spectral_em",
                "apap_spectral_em_device"):
        assert sym in native.SIGNATURES and hasattr(native.lib(), sym)


def test_status_to_code_keeps_its_three_bits():
    src = open(os.path.join(ROOT, "cvx_proj_amd", "csrc", "apap_capi.hip")).read()
    body = src[src.index("int status_to_code("):]
    body = body[:body.index("return APAP_OK;")]
    assert "MODEL" not in body


def test_model_workspace_is_linear_and_aligned(native):
    lib = native.lib()
    assert lib.apap_model_workspace_bytes(0) == 0
    for n in (1, 4, 240, 241, 5000, 1 << 20):
        b = lib.apap_model_workspace_bytes(n)
        assert b > 0 and b % 256 == 0
    assert lib.apap_model_workspace_bytes(1 << 24) <= 1024 * 15 * 15 * 8 + 8192     # at most 1024 block factors


def test_model_argument_errors(native):
    pc = np.zeros((5, 2), np.float32)
    with pytest.raises(ValueError):
        native.model_solve(pc, np.zeros((4, 2), np.float32), np.ones(5, np.float32), native.model_params(native.MODEL_SDP))
    with pytest.raises(ValueError):
        native.model_solve(pc, pc, np.ones(5, np.float32), np.zeros(3))
    from cvx_proj_amd.model import LMSSolver
    with pytest.raises(NotImplementedError, match="Huber"):
        LMSSolver(100, 0.5).solve(pc, pc, np.ones(5, np.float32), verbose=0)
    from cvx_proj_amd import spectral_method
    with pytest.raises(NotImplementedError, match="Huber"):
        spectral_method.spectral_em(pc, pc, np.ones((5, 128), np.float32), np.ones((5, 128), np.float32), np.eye(3), lms=True,
                                    huber_param=0.5, mask=np.ones(5, np.float32))


def test_model_refuses_without_a_device(native):
    """No CPU fallback: the M-step's entry points fail with ERR_NO_DEVICE when no GPU is visible; bad parameters are refused
    before any device is touched."""
    lib = native.lib()
    pc = (np.arange(16, dtype=np.float32).reshape(8, 2) * 7) % 13
    w = np.ones(8, np.float32)
    bad = native.model_params(native.MODEL_SDP)
    bad[0] = 3
    with pytest.raises(native.ApapError) as e:
        native.model_solve(pc, pc, w, bad)
    assert e.value.code in (native.ERR_INVALID_ARG, native.ERR_NO_DEVICE)
    assert lib.apap_model_solve_device(None, None, None, None, 8, bad.ctypes.data_as(native._f64p), None, None, None, None, 0,
                                       None) == native.ERR_INVALID_ARG
    if lib.apap_device_count() > 0:
        pytest.skip("a GPU is visible")
    with pytest.raises(native.ApapError) as e:
        native.model_solve(pc, pc, w, native.model_params(native.MODEL_SDP))
    assert e.value.code == native.ERR_NO_DEVICE
    with pytest.raises(native.ApapError) as e:
        native.spectral_em(pc, pc, np.ones((8, 128), np.float32), np.ones((8, 128), np.float32), np.eye(3), native.spectral_params(),
                           native.model_params(native.MODEL_SDP), 2, w)
    assert e.value.code == native.ERR_NO_DEVICE


def test_product_does_not_import_the_spec():
    for dirpath, _, files in os.walk(os.path.join(ROOT, "cvx_proj_amd")):
        for f in files:
            if f.endswith(".py"):
                assert "model_spec" not in open(os.path.join(dirpath, f)).read(), f


@pytest.mark.parametrize("shape", [(0, 2), (0,)], ids=["n_by_2", "one_dimensional"])
def test_no_point_raises_index_error(native, capsys, shape):
    """The reference's `pts_c[:, None, :]` on np.float32([]): IndexError, every time, before anything is printed and
    before any device is needed."""
    from cvx_proj_amd.model import LMSSolver, SDPSolver
    e = np.zeros(shape, np.float32)
    for _ in range(4):
        for solver in (SDPSolver(10, 0.5, 0.5), LMSSolver(10)):
            with pytest.raises(IndexError):
                solver.solve(e, e, np.zeros(0, np.float32), verbose=1)
    assert capsys.readouterr().out == ""


def test_argument_errors_leave_the_info_block_nan(native):
    """An argument error returns before the kernels run: the info block the error carries is NaN, never stale memory."""
    for _ in range(4):
        with pytest.raises(native.ApapValueError) as e:
            native.model_solve(np.zeros((0, 2), np.float32), np.zeros((0, 2), np.float32), np.zeros(0, np.float32),
                               native.model_params(native.MODEL_SDP))
        assert np.isnan(e.value.info).all()
    info = np.zeros(native.MODEL_INFO)
    H = np.zeros(9, np.float32)
    p = native.model_params(native.MODEL_SDP)
    f32 = native._f32p
    code = native.lib().apap_model_solve(None, H.ctypes.data_as(f32), H.ctypes.data_as(f32), H.ctypes.data_as(f32), 0,
                                         p.ctypes.data_as(native._f64p), H.ctypes.data_as(f32), info.ctypes.data_as(native._f64p), -1)
    assert code == native.ERR_INVALID_ARG and np.isnan(info).all() and np.isnan(H).all()


@pytest.mark.parametrize("steps", [0, 65])
def test_em_steps_out_of_range(native, steps):
    from cvx_proj_amd import spectral_method
    pc = (np.arange(10, dtype=np.float32).reshape(5, 2) * 37) % 101
    d = np.ones((5, 128), np.float32)
    with pytest.raises(native.ApapValueError, match="em_steps"):
        spectral_method.spectral_em(pc, pc, d, d, np.eye(3), em_steps=steps, mask=np.ones(5, np.float32))
    with pytest.raises(native.ApapValueError) as e:
        native.spectral_em(pc, pc, d, d, np.eye(3), native.spectral_params(), native.model_params(native.MODEL_SDP), steps,
                           np.ones(5, np.float32))
    assert np.isnan(e.value.info[1]).all() and np.isnan(e.value.info[0]).all()


def test_model_solve_with_no_selected_match(native):
    from cvx_proj_amd import spectral_method

    class KP:
        def __init__(self, p):
            self.pt = (float(p[0]), float(p[1]))

    class DM:
        def __init__(self, i):
            self.queryIdx = self.trainIdx = i
    pts = [KP((i, 2 * i + 1)) for i in range(6)]
    m = [DM(i) for i in range(6)]
    with pytest.raises(IndexError):
        spectral_method.model_solve(pts, pts, m, np.full(6, 9e-4, np.float32), param=0.5, lms=False)
    with pytest.raises(IndexError):
        spectral_method.model_solve([], [], [], np.zeros(0, np.float32), param=0.5, lms=False)
