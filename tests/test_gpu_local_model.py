"""The robust moving DLT on the MI355X.  The yardstick is the single-problem path: for every cell, H, info and status equal
``apap_model_solve`` on ``float32(local_weights(...)[cell]) * match_weights``, byte for byte, whatever else is in the call and
wherever a chunk boundary falls.  Certificates and the exact-data check use tests/model_spec.py as tests/test_gpu_model.py
does."""
import ctypes as C
import warnings

import numpy as np
import pytest

import model_spec as S
from test_gpu_model import synthetic

pytestmark = pytest.mark.gpu

SIGMA = 12.0          # exp(-d / sigma^2) reaches the 1e-3 floor at d = 995 px on the 1280 x 960 pairs: some cells drop matches
SMALL_GAMMA = 1e-4    # below the floor: distant weights are not lifted, so the floor selects per cell
SIZES = (50, 300, 700)     # 1, 2 and 3 TSQR blocks of 240 matches


@pytest.fixture(scope="module")
def native_gpu(native):
    if native.lib().apap_device_count() < 1:
        pytest.skip("no HIP device")
    return native


def mesh(cols=12, rows=9):
    """(rows, cols, 2) float64 sample points over the synthetic pairs' 1280 x 960 frame, off the round numbers."""
    x = np.linspace(0.0, 1280.0, cols) + 1280.0 / (2 * cols) + 0.37
    y = np.linspace(0.0, 960.0, rows) + 960.0 / (2 * rows) - 0.21
    v = np.empty((rows, cols, 2))
    v[..., 0] = x[None, :]
    v[..., 1] = y[:, None]
    return v


def pair(n):
    pc, po, _, _ = synthetic("outliers", n=n, seed=n)
    return pc, po


def match_weights(kind, n):
    if kind == "none":
        return None
    if kind == "ones":
        return np.ones(n, np.float32)
    rng = np.random.default_rng(n + 1)        # spectral-like: exact zeros, values at or below the floor, the rest in (0, 1]
    mw = rng.random(n).astype(np.float32)
    u = rng.random(n)
    mw[u < 0.3] = 0.0
    mw[(u >= 0.3) & (u < 0.4)] = np.float32(1e-3)     # float32(1e-3) > 1e-3 in float64: kept
    mw[(u >= 0.4) & (u < 0.5)] = np.float32(5e-4)
    mw[(u >= 0.5) & (u < 0.55)] = np.float32(9.99e-4)
    return mw


def cell_weights(native, pc, vertices, gamma, sigma, mw):
    """(cells, n) float32: the contract's w_k, with numpy."""
    W = native.local_weights(pc, vertices.reshape(-1, 2), gamma, sigma).astype(np.float32)
    return W if mw is None else W * mw[None, :]


def single(native, pc, po, w, params):
    """apap_model_solve on one weight vector: (H (3, 3), info (24,), return code) - the outputs also when the code is an error."""
    H = np.full((3, 3), np.nan, np.float32)
    info = np.full(native.MODEL_INFO, np.nan)
    w = np.ascontiguousarray(w, np.float32)
    code = native.lib().apap_model_solve(None, native._ptr(pc, C.c_float), native._ptr(po, C.c_float), native._ptr(w, C.c_float),
                                         len(pc), native._ptr(params, C.c_double), native._ptr(H, C.c_float),
                                         native._ptr(info, C.c_double), -1)
    return H, info, code


def assert_cell(native, got, want, what):
    """got = (H, info, status word) of a cell of the grid call; want = single()'s triple."""
    H, info, word = got
    Hs, infos, code = want
    assert H.tobytes() == Hs.tobytes(), (what, H, Hs)
    assert info.tobytes() == infos.tobytes(), (what, info, infos)
    assert int(word) == int(infos[native.MODEL_INFO_STATUS]), what
    assert np.array_equal(H, Hs, equal_nan=True) and np.array_equal(info, infos, equal_nan=True)
    degenerate = bool(int(word) & native.STATUS_MODEL_DEGENERATE)
    assert degenerate == bool(np.isnan(H).all()), what
    assert (code != native.OK) == bool(int(word) & (native.STATUS_MODEL_DEGENERATE | native.STATUS_SINGULAR)), (what, code)


SOLVERS = [("sdp", 0.2), ("sdp", 1.25), ("lms", 1.0)]


def params_of(native, solver, fluc, swap, floor=1e-3, max_iter=0):
    mode = native.MODEL_SDP if solver == "sdp" else native.MODEL_LMS
    return native.model_params(mode, fluc, fluc, floor=floor, swap=swap, max_iter=max_iter)


@pytest.mark.parametrize("gamma", [SMALL_GAMMA, 0.5], ids=["gamma_small", "gamma_default"])
@pytest.mark.parametrize("kind", ["none", "ones", "spectral"])
@pytest.mark.parametrize("swap", [False, True], ids=["noswap", "swap"])
@pytest.mark.parametrize("solver,fluc", SOLVERS, ids=[f"{s}_{f}" for s, f in SOLVERS])
@pytest.mark.parametrize("n", SIZES)
def test_every_cell_equals_its_own_model_solve(native_gpu, n, solver, fluc, swap, kind, gamma):
    native = native_gpu
    pc, po = pair(n)
    v = mesh()
    mw = match_weights(kind, n)
    params = params_of(native, solver, fluc, swap)
    before = [a.copy() for a in (pc, po, v)] + ([mw.copy()] if mw is not None else [])
    H, info, status = native.local_model_solve(pc, po, v, gamma, SIGMA, params, match_weights=mw)
    assert H.shape == (9, 12, 3, 3) and H.dtype == np.float32
    assert info.shape == (9, 12, native.MODEL_INFO) and info.dtype == np.float64
    assert status.shape == (9, 12) and status.dtype == np.int32
    w = cell_weights(native, pc, v, gamma, SIGMA, mw)
    counts = []
    for k in range(108):
        i, j = divmod(k, 12)
        want = single(native, pc, po, w[k], params)
        assert_cell(native, (H[i, j], info[i, j], status[i, j]), want, (n, solver, fluc, swap, kind, gamma, k))
        counts.append(int(want[1][native.MODEL_INFO_COUNT]))
    print(f"n={n} {solver} fluc={fluc} swap={swap} mw={kind} gamma={gamma}: selected per cell {min(counts)} .. {max(counts)}, "
          f"status words {sorted(set(int(s) for s in status.ravel()))}")
    if gamma == SMALL_GAMMA:
        assert min(counts) < max(counts)      # the floor selects differently per cell: distant weights were not lifted
    elif kind != "spectral":
        assert min(counts) == n               # gamma 0.5 lifts every weight over the floor
    for a, b in zip((pc, po, v) + ((mw,) if mw is not None else ()), before):
        assert a.tobytes() == b.tobytes()     # inputs untouched


@pytest.mark.parametrize("n", [240, 241, 720, 721])
def test_unequal_fluctuations_at_the_block_edges(native_gpu, n):
    """du != dv (params_of passes one value for both) with n on the 240-match block and on the three-block fold of M2."""
    native = native_gpu
    pc, po = pair(n)
    v = np.stack(np.meshgrid(np.float64([320.37, 960.37]), np.float64([239.79, 719.79])), axis=-1)      # (2, 2, 2)
    mw = match_weights("spectral", n)
    params = native.model_params(native.MODEL_SDP, 0.2, 1.25, floor=1e-3, swap=True)
    H, info, status = native.local_model_solve(pc, po, v, SMALL_GAMMA, SIGMA, params, match_weights=mw)
    assert H.shape == (2, 2, 3, 3) and info.shape == (2, 2, native.MODEL_INFO) and status.shape == (2, 2)
    w = cell_weights(native, pc, v, SMALL_GAMMA, SIGMA, mw)
    for k in range(4):
        i, j = divmod(k, 2)
        assert_cell(native, (H[i, j], info[i, j], status[i, j]), single(native, pc, po, w[k], params), (n, k))


def test_floor_off_keeps_every_match(native_gpu):
    """floor = None (-inf): zero-weight matches stay in as zero rows; the count is n in every cell."""
    native = native_gpu
    pc, po = pair(300)
    v, mw = mesh(4, 3), match_weights("spectral", 300)
    params = params_of(native, "sdp", 0.5, False, floor=None)
    H, info, status = native.local_model_solve(pc, po, v, SMALL_GAMMA, SIGMA, params, match_weights=mw)
    w = cell_weights(native, pc, v, SMALL_GAMMA, SIGMA, mw)
    for k in range(12):
        assert_cell(native, (H[k // 4, k % 4], info[k // 4, k % 4], status[k // 4, k % 4]), single(native, pc, po, w[k], params), k)
    assert (info[..., native.MODEL_INFO_COUNT] == 300).all()


def test_no_cross_talk_between_cells(native_gpu):
    native = native_gpu
    pc, po = pair(300)
    v = mesh().reshape(-1, 2)
    mw = match_weights("spectral", 300)
    params = params_of(native, "sdp", 0.5, True)
    full = native.local_model_solve(pc, po, v, SMALL_GAMMA, SIGMA, params, match_weights=mw)
    again = native.local_model_solve(pc, po, v, SMALL_GAMMA, SIGMA, params, match_weights=mw)
    for a, b in zip(full, again):
        assert a.tobytes() == b.tobytes()     # the same call twice: the same bytes
    rng = np.random.default_rng(11)
    perm = rng.permutation(108)
    subsets = [perm, np.arange(108)[::-1], rng.choice(108, 17, replace=False), np.array([5]), np.array([107]),
               np.array([3, 3, 3, 40, 3])]    # a permutation, the reverse, a subset, single cells, a cell repeated
    for idx in subsets:
        H, info, status = native.local_model_solve(pc, po, v[idx], SMALL_GAMMA, SIGMA, params, match_weights=mw)
        assert H.shape == (len(idx), 3, 3)
        for at, k in enumerate(idx):
            assert H[at].tobytes() == full[0][k].tobytes() and info[at].tobytes() == full[1][k].tobytes(), (len(idx), at, k)
            assert status[at] == full[2][k]


def resident_call(native, pc, po, v, gamma, sigma, params, mw, work_cells=None, ctx=None):
    import torch
    from cvx_proj_amd import resident
    dev = torch.device("cuda", 0)
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)      # noqa: E731
    work = None
    if work_cells is not None:
        work = torch.empty(resident.local_model_workspace_bytes(len(pc), work_cells), dtype=torch.uint8, device=dev)
    out = resident.hip_local_model_solve(t(pc), t(po), t(v), gamma, sigma, params, match_weights=t(mw), work=work, ctx=ctx)
    torch.cuda.synchronize()
    return tuple(x.cpu().numpy() for x in out)


@pytest.mark.parametrize("solver", ["sdp", "lms"])
def test_a_workspace_of_five_cells_gives_the_same_bytes(native_gpu, solver):
    """108 cells through a workspace that holds 5: 22 chunks, the last of 3 cells.  Same bytes as one chunk."""
    native = native_gpu
    pc, po = pair(300)
    v, mw = mesh(), match_weights("spectral", 300)
    params = params_of(native, solver, 0.5, False)
    whole = resident_call(native, pc, po, v, SMALL_GAMMA, SIGMA, params, mw)
    for cells in (5, 1, 107):
        parts = resident_call(native, pc, po, v, SMALL_GAMMA, SIGMA, params, mw, work_cells=cells)
        for a, b in zip(parts, whole):
            assert a.shape == b.shape and a.tobytes() == b.tobytes(), cells
    host = native.local_model_solve(pc, po, v, SMALL_GAMMA, SIGMA, params, match_weights=mw)
    for a, b in zip(whole, host):
        assert a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def test_chunked_launch_count(native_gpu):
    """Launches per call are 2 x chunks: one reduction and one solve per chunk, counted by the context's profile scopes."""
    native = native_gpu
    pc, po = pair(300)
    params = params_of(native, "lms", 1.0, False)
    for work_cells, chunks in ((None, 1), (108, 1), (54, 2), (5, 22), (1, 108)):
        ctx = native.Context(profile=1)
        resident_call(native, pc, po, mesh(), 0.5, SIGMA, params, None, work_cells=work_cells, ctx=ctx)
        prof = ctx.profile_read()
        ctx.close()
        assert (prof["assemble"][1], prof["eigen"][1]) == (chunks, chunks), (work_cells, prof)


def test_one_cell_beyond_the_chunk(native_gpu):
    """cells = chunk + 1 with the default workspace: two chunks, the second of one cell."""
    native = native_gpu
    cells = native.LOCAL_MODEL_CHUNK + 1
    pc, po = pair(240)
    rng = np.random.default_rng(5)
    v = rng.random((cells, 2)) * np.float64([1280, 960])
    mw = match_weights("spectral", 240)
    params = params_of(native, "lms", 1.0, False)
    ctx = native.Context(profile=1)
    H, info, status = native.local_model_solve(pc, po, v, 0.5, 100.0, params, match_weights=mw, ctx=ctx)
    prof = ctx.profile_read()
    ctx.close()
    assert (prof["assemble"][1], prof["eigen"][1]) == (2, 2), prof
    assert not np.isnan(H).any() and not status.any()
    sample = sorted(set([0, 1, cells - 3, cells - 2, cells - 1] + [int(k) for k in rng.choice(cells, 40, replace=False)]))
    w = cell_weights(native, pc, v[sample], 0.5, 100.0, mw)
    for at, k in enumerate(sample):
        assert_cell(native, (H[k], info[k], status[k]), single(native, pc, po, w[at], params), k)


def test_resident_form_equals_the_host_buffer_form(native_gpu):
    native = native_gpu
    for n, solver, kind in ((700, "sdp", "none"), (50, "sdp", "spectral"), (300, "lms", "ones")):
        pc, po = pair(n)
        v, mw = mesh(), match_weights(kind, n)
        params = params_of(native, solver, 0.5, True)
        host = native.local_model_solve(pc, po, v, SMALL_GAMMA, SIGMA, params, match_weights=mw)
        dev = resident_call(native, pc, po, v, SMALL_GAMMA, SIGMA, params, mw)
        for a, b in zip(dev, host):
            assert a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes(), (n, solver, kind)


def test_a_degenerate_cell_is_its_own(native_gpu):
    """gamma 0, sigma 6: a weight passes the 1e-3 floor within 249 px of the vertex.  Every match within 320 px of the
    corner carries match weight 0, so the vertex at (40, 40) selects none: that cell alone is degenerate."""
    from cvx_proj_amd.apap import APAP
    native = native_gpu
    pc, po = pair(700)
    mw = np.ones(700, np.float32)
    mw[(pc[:, 0] < 320) & (pc[:, 1] < 320)] = 0.0
    assert (mw == 0).sum() >= 10
    x, y = np.float64([40, 450, 860, 1240]), np.float64([40, 480, 920])
    v = np.stack(np.meshgrid(x, y), axis=-1)      # (3, 4, 2): cell (0, 0) is the corner
    gamma, sigma = 0.0, 6.0
    params = params_of(native, "sdp", 0.5, False)
    H, info, status = native.local_model_solve(pc, po, v, gamma, sigma, params, match_weights=mw)      # returns: no exception
    assert status[0, 0] == native.STATUS_MODEL_DEGENERATE and np.isnan(H[0, 0]).all()
    assert int(info[0, 0, native.MODEL_INFO_STATUS]) == native.STATUS_MODEL_DEGENERATE and info[0, 0, native.MODEL_INFO_COUNT] < 4
    rest = np.ones((3, 4), bool)
    rest[0, 0] = False
    assert not (status[rest] & native.STATUS_MODEL_DEGENERATE).any() and not np.isnan(H[rest]).any()
    assert (info[rest][:, native.MODEL_INFO_COUNT] >= 4).all()
    w = cell_weights(native, pc, v, gamma, sigma, mw)
    for k in range(12):
        assert_cell(native, (H[k // 4, k % 4], info[k // 4, k % 4], status[k // 4, k % 4]), single(native, pc, po, w[k], params), k)
    # the neighbours without the degenerate cell in the call: unchanged
    alone = native.local_model_solve(pc, po, v.reshape(-1, 2)[1:], gamma, sigma, params, match_weights=mw)
    for a, b in zip(alone, (H.reshape(-1, 3, 3)[1:], info.reshape(12, -1)[1:], status.ravel()[1:])):
        assert a.tobytes() == np.ascontiguousarray(b).tobytes()
    eng = APAP(gamma, sigma, [1280, 960], [0, 0])
    with pytest.warns(RuntimeWarning, match=r"1 of 12 cells degenerate") as rec:
        grid = eng.local_robust_homography(pc, po, v, mw)
    assert len([r for r in rec if issubclass(r.category, RuntimeWarning)]) == 1
    assert grid.tobytes() == H.tobytes() and np.isnan(grid[0, 0]).all()
    grid2, info2, status2 = eng.local_robust_homography(pc, po, v[1:], mw, return_info=True)      # no degenerate cell: no warning
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        eng.local_robust_homography(pc, po, v[1:], mw)
    assert info2.tobytes() == info[1:].tobytes() and not status2.any()


def test_sdp_certificate_per_cell(native_gpu):
    """phi(h) - psi(Z) <= 1e-9 phi(h) on each sampled cell's own selected matches and weights (test_sdp_certificate's bar)."""
    native = native_gpu
    pc, po = pair(300)
    v, mw = mesh(), match_weights("spectral", 300)
    for fluc, gamma in ((0.2, 0.5), (1.25, SMALL_GAMMA)):
        params = params_of(native, "sdp", fluc, False)
        H, info, status = native.local_model_solve(pc, po, v, gamma, SIGMA, params, match_weights=mw)
        w = cell_weights(native, pc, v, gamma, SIGMA, mw)
        for k in (0, 7, 11, 50, 53, 59, 96, 107):
            i, j = divmod(k, 12)
            spc, spo, sw = S.select(pc, po, w[k])
            assert int(info[i, j, native.MODEL_INFO_COUNT]) == len(spc) >= 4
            gap = info[i, j, native.MODEL_INFO_GAP]
            assert status[i, j] == 0 and gap <= 1e-10, (k, status[i, j], gap)
            h = info[i, j, native.MODEL_INFO_H:native.MODEL_INFO_H + 8]
            Z = info[i, j, native.MODEL_INFO_Z:native.MODEL_INFO_Z + 9].reshape(3, 3)
            ph, ps = S.phi(spc, spo, sw, h, fluc, fluc), S.psi(spc, spo, sw, Z, fluc, fluc)
            print(f"fluc={fluc} gamma={gamma} cell {k}: selected {len(spc)} phi={ph:.6e} (phi - psi) / phi={(ph - ps) / ph:.3e}")
            assert ps <= ph * (1 + 1e-12)
            assert ph - ps <= 1e-9 * ph, (k, ph, ps, (ph - ps) / ph)
            np.testing.assert_array_equal(H[i, j], S.tail(h, False))


def test_exact_data_gives_the_homography_in_every_cell(native_gpu):
    """Outlier-free points on one homography: the LMS grid is that homography in every cell (test_lms_exact_homography's
    tolerance), and local_warp takes the grid as it stands."""
    from cvx_proj_amd.apap import APAP
    from cvx_proj_amd.apap_utils import get_mesh, get_vertice
    native = native_gpu
    pc, po, _, Ht = synthetic("exact", n=300, seed=3)
    m, size = 10, (1280, 960)
    eng = APAP(0.5, 100.0, list(size), [0, 0])
    v = get_vertice(size, m, (0, 0))
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        H, info, status = eng.local_robust_homography(pc, po, v, lms=True, return_info=True)
    assert H.shape == (m, m, 3, 3) and H.dtype == np.float32 and not status.any()
    h = info[..., native.MODEL_INFO_H:native.MODEL_INFO_H + 8]
    err = np.abs(h - Ht.ravel()[:8]).max()
    print(f"exact data: max |h - Ht| over {m * m} cells = {err:.3e}")
    assert err <= 1e-5 * np.abs(Ht.ravel()[:8]).max()
    assert (H[..., 2, 2] == 1.0).all()
    img = np.random.default_rng(0).integers(0, 256, (960, 1280, 3), dtype=np.uint8)
    canvas = eng.local_warp(img, H.copy(), get_mesh(size, m + 1))
    assert canvas.shape == (960, 1280, 3) and canvas.dtype == np.uint8 and canvas.any()
    plain, _ = eng.local_homography(pc, po, v, return_weights=False)      # the plain moving DLT: the same direction
    assert np.abs(plain / plain[..., 2:, 2:] - H).max() <= 1e-2 * np.abs(Ht).max()


def test_launch_count_does_not_depend_on_the_cells(native_gpu):
    native = native_gpu
    pc, po = pair(300)
    params = params_of(native, "sdp", 0.5, False)
    counts = []
    for v in (mesh(2, 2), mesh()):
        ctx = native.Context(profile=1)
        native.local_model_solve(pc, po, v, 0.5, SIGMA, params, ctx=ctx)
        prof = ctx.profile_read()
        counts.append((prof["assemble"][1], prof["eigen"][1]))
        ctx.close()
    assert counts == [(1, 1), (1, 1)], counts
