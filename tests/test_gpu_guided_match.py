"""Guided descriptor matching on the MI355X (apap_guided_records, apap_match_guided and its batch, resident and Python forms)
against the numpy specification of tests/guided_match_spec.py, byte for byte: the gate is float64 in a written order and the
descriptors are integer-valued, so the float32 sum of squared differences is exact.  Float descriptors are held, byte for byte
too, against apap_match_descriptors itself, whose d2 the guided matcher restates."""
import ctypes as C

import numpy as np
import pytest

import guided_match_cases as GC
import guided_match_spec as S

pytestmark = pytest.mark.gpu

NAMES = ("idx", "dist", "idx2", "dist2", "count", "ridx", "rdist")
INF = np.inf


@pytest.fixture(scope="module")
def native_gpu(native):
    if native.lib().apap_device_count() < 1:
        pytest.skip("no HIP device")
    return native


def same_bytes(got, want, what="", names=NAMES):
    for name, g, w in zip(names, got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, w.dtype, g.shape, w.shape)
        assert g.tobytes() == w.tobytes(), (what, name, int(np.count_nonzero(g.view(np.int32) != w.view(np.int32))), g[:8], w[:8])


def same_f64(got, want, what=""):
    """Byte for byte, but for the sign and payload of a NaN, which IEEE 754 leaves to the implementation."""
    nan = np.isnan(want)
    assert got.dtype == want.dtype == np.float64 and got.shape == want.shape and np.array_equal(np.isnan(got), nan), what
    assert got[~nan].tobytes() == want[~nan].tobytes(), (what, np.flatnonzero((got != want).any(1) & ~nan.any(1))[:5])


def run(native, case, **kw):
    return native.match_guided(case.q, case.t, case.rec_q, case.rec_t, case.kind, case.r2, reverse=True, **kw)


def check(native, case, what=""):
    got, want = run(native, case), S.match_int(*case)
    same_bytes(got, want, what)
    return got


def test_sizes_at_the_tiling_edges(native_gpu):
    """nq, nt in {1, 2} and one below, at and one above the query tile, the train chunk, the drain and the last shape with
    one chunk per split."""
    for nq, nt in GC.size_shapes(native_gpu):
        case = GC.sized(nq, nt)
        check(native_gpu, case, (nq, nt))


def test_empty_and_single_candidates(native_gpu):
    case = GC.sized(257, 129)
    idx, dist, idx2, dist2, count, _, _ = check(native_gpu, case)
    none, one = np.flatnonzero(count == 0), np.flatnonzero(count == 1)
    assert len(none) and len(one)
    for i in none:
        assert (idx[i], dist[i], idx2[i], dist2[i], count[i]) == (-1, INF, -1, INF, 0)
    assert (idx[one] >= 0).all() and (idx2[one] == -1).all() and np.isinf(dist2[one]).all()


def test_one_query_admits_every_train_row(native_gpu):
    case, special = GC.one_admits_all()
    idx, dist, idx2, dist2, count, ridx, rdist = check(native_gpu, case)
    assert count[special] == 300 and np.delete(count, special).max() <= 2
    plain = native_gpu.match_descriptors(case.q[special:special + 1], case.t)      # all admitted: the unguided answer
    assert (idx[special], idx2[special]) == (plain[0][0], plain[2][0]) and dist[special] == plain[1][0] and dist2[special] == plain[3][0]


def test_equal_d2_goes_to_the_lowest_admitted_index(native_gpu):
    inside = check(native_gpu, GC.duplicates(True))
    assert (inside[0][0], inside[2][0]) == (3, 9) and inside[1][0] == 0 and inside[3][0] == 0
    outside = check(native_gpu, GC.duplicates(False))
    assert outside[0][0] == 9 and outside[1][0] == 0 and outside[2][0] != 3


def test_the_gate_is_strict(native_gpu):
    at = check(native_gpu, GC.three_four(25.0))
    above = check(native_gpu, GC.three_four(float(np.nextafter(25.0, INF))))
    assert (at[0][0], at[4][0]) == (-1, 0) and (above[0][0], above[4][0]) == (0, 1)


def test_lines(native_gpu):
    """A null line passes nothing; points exactly at distance r from a horizontal line fail, whatever the line's scale."""
    idx, dist, idx2, dist2, count, ridx, rdist = check(native_gpu, GC.line_cases())
    assert count.tolist() == [0, 4, 4, 0, 0, 2]


def test_non_finite_records_r2_zero_and_infinite(native_gpu):
    case = GC.non_finite_records()
    got = check(native_gpu, case)
    assert got[4].tolist() == [2, 0, 0, 0, 2]
    zero = check(native_gpu, case._replace(r2=0.0))
    assert not zero[4].any() and (zero[0] == -1).all() and (zero[5] == -1).all()
    everything = check(native_gpu, case._replace(r2=INF))
    assert everything[4].tolist() == [3, 0, 0, 0, 3]      # the finite train records: inf < inf fails, and so does NaN
    finite = GC.sized(5, 7)
    assert check(native_gpu, finite._replace(r2=INF))[4].tolist() == [7] * 5


def test_non_finite_descriptors_are_counted_and_never_selected(native_gpu):
    idx, dist, idx2, dist2, count, ridx, rdist = check(native_gpu, GC.non_finite_descriptors())
    assert count.tolist() == [5, 5, 5] and idx[2] == -1 and not np.isin(idx[:2], (1, 2)).any() and not np.isin(idx2[:2], (1, 2)).any()
    assert ridx[1] == -1 and ridx[2] == -1 and np.isinf(rdist[1:3]).all()


@pytest.mark.parametrize("descriptors", ["integer", "float"])
def test_everything_admitted_equals_the_unguided_matcher(native_gpu, descriptors):
    rng = np.random.default_rng(21)
    nq, nt = 130, 300
    if descriptors == "integer":
        q, t = GC.ints(rng, nq), GC.ints(rng, nt)
    else:
        q, t = rng.normal(0, 1, (nq, S.MS.DIM)).astype(np.float32), rng.normal(0, 1, (nt, S.MS.DIM)).astype(np.float32)
    rec_q, rec_t = GC.point_recs(rng.random((nq, 2)) * 100), GC.point_recs(rng.random((nt, 2)) * 100)
    got = native_gpu.match_guided(q, t, rec_q, rec_t, S.KIND_POINT, INF)
    same_bytes(got[:4], native_gpu.match_descriptors(q, t), descriptors, NAMES[:4])
    assert got[4].tolist() == [nt] * nq


def test_float_descriptors_equal_the_matcher_on_each_gated_subset(native_gpu):
    rng = np.random.default_rng(22)
    nq, nt = 40, 300
    q, t = rng.normal(0, 1, (nq, S.MS.DIM)).astype(np.float32), rng.normal(0, 1, (nt, S.MS.DIM)).astype(np.float32)
    t[1::2] = t[0::2] + rng.normal(0, 1e-3, (nt // 2, S.MS.DIM)).astype(np.float32)      # near-duplicates: the order is decided in the last bits
    rec_q, rec_t = GC.point_recs(rng.random((nq, 2)) * 100), GC.point_recs(rng.random((nt, 2)) * 100)
    r2 = 400.0
    idx, dist, idx2, dist2, count, _, _ = native_gpu.match_guided(q, t, rec_q, rec_t, S.KIND_POINT, r2)
    passes = S.gate(rec_q, rec_t, S.KIND_POINT, r2)
    assert np.array_equal(count, passes.sum(1)) and count.max() >= 8
    for i in range(nq):
        rows = np.flatnonzero(passes[i])
        if not len(rows):
            assert (idx[i], idx2[i]) == (-1, -1)
            continue
        p = native_gpu.match_descriptors(q[i:i + 1], t[rows])
        back = lambda k: -1 if k < 0 else rows[k]      # noqa: E731
        assert (idx[i], idx2[i]) == (back(p[0][0]), back(p[2][0])), i
        assert dist[i].tobytes() == p[1][0].tobytes() and dist2[i].tobytes() == p[3][0].tobytes(), i


def test_reverse_outputs(native_gpu):
    """POINT: the reverse outputs are the forward outputs of the call with the sides swapped.  LINE: the specification's."""
    case = GC.sized(257, 300)
    fwd = run(native_gpu, case)
    swapped = native_gpu.match_guided(case.t, case.q, case.rec_t, case.rec_q, case.kind, case.r2, reverse=True)
    same_bytes(fwd[5:7], swapped[0:2], "reverse = swapped forward", ("ridx", "rdist"))
    same_bytes(swapped[5:7], fwd[0:2], "swapped reverse = forward", ("ridx", "rdist"))
    rng = np.random.default_rng(23)
    F = np.array([[0, -1e-3, 0.2], [1e-3, 0, -0.3], [-0.25, 0.31, 1.0]])
    qp, tp = (rng.random((130, 2)) * 100).astype(np.float32), (rng.random((300, 2)) * 100).astype(np.float32)
    line = GC.Case(GC.ints(rng, 130), GC.ints(rng, 300), S.records(qp, F, S.LINE), S.records(tp), S.KIND_LINE, 9.0)
    got = check(native_gpu, line)
    assert (got[5] >= 0).sum() > 30


def batch_arrays():
    cases, q0, t0 = GC.batch_pairs()
    rng = np.random.default_rng(24)
    q = np.concatenate([GC.ints(rng, q0)] + [c.q for c in cases])
    t = np.concatenate([GC.ints(rng, t0)] + [c.t for c in cases])
    rec_q = np.concatenate([np.full((q0, 3), np.nan)] + [c.rec_q for c in cases])
    rec_t = np.concatenate([np.full((t0, 3), np.nan)] + [c.rec_t for c in cases])
    qo = np.cumsum([q0] + [len(c.q) for c in cases]).astype(np.int32)
    to = np.cumsum([t0] + [len(c.t) for c in cases]).astype(np.int32)
    return cases, q, t, rec_q, rec_t, qo, to, np.array([c.r2 for c in cases])


def raw_batch(native, q, t, rec_q, rec_t, qo, to, r2, kind, guard=16):
    """apap_match_guided_batch on buffers with guard elements before and after every output and sentinel rows before the first
    offsets; returns the seven outputs (whole arrays) after checking the guards."""
    nq, nt = len(q), len(t)
    spec = (("idx", nq, np.int32), ("dist", nq, np.float32), ("idx2", nq, np.int32), ("dist2", nq, np.float32),
            ("count", nq, np.int32), ("ridx", nt, np.int32), ("rdist", nt, np.float32))
    bufs = {name: np.full(n + 2 * guard, -77, dtype) for name, n, dtype in spec}
    ptr = lambda a, ct: a[guard:].ctypes.data_as(C.POINTER(ct))      # noqa: E731
    ct = {np.int32: C.c_int, np.float32: C.c_float}
    native.check(native.lib().apap_match_guided_batch(
        None, native._dp(rec_q), native._dp(rec_t), native._ptr(q, C.c_float), native._ptr(t, C.c_float), native._ip(qo),
        native._ip(to), len(qo) - 1, kind, native._dp(r2), *[ptr(bufs[name], ct[dtype]) for name, _, dtype in spec], -1))
    out = []
    for name, n, dtype in spec:
        b, first = bufs[name], (to if name in ("ridx", "rdist") else qo)[0]
        assert (b[:guard + first] == -77).all() and (b[guard + n:] == -77).all(), name      # guards and sentinel rows untouched
        out.append(b[guard:guard + n])
    return out


def test_batch_equals_the_single_calls(native_gpu):
    cases, q, t, rec_q, rec_t, qo, to, r2 = batch_arrays()
    out = raw_batch(native_gpu, q, t, rec_q, rec_t, qo, to, r2, S.KIND_POINT)
    for p, case in enumerate(cases):
        single = run(native_gpu, case)
        same_bytes(single, S.match_int(*case), f"pair {p} single")
        for name, o, s in zip(NAMES, out, single):
            lo, hi = (to if name in ("ridx", "rdist") else qo)[p:p + 2]
            assert o[lo:hi].tobytes() == s.tobytes(), (p, name)
    py = native_gpu.match_guided_batch(q[qo[0]:], t[to[0]:], rec_q[qo[0]:], rec_t[to[0]:], np.diff(qo), np.diff(to), S.KIND_POINT, r2,
                                       reverse=True)
    for name, o, b in zip(NAMES, out, py):
        assert o[(to if name in ("ridx", "rdist") else qo)[0]:].tobytes() == b.tobytes(), name


def test_the_three_entry_forms_and_a_dirty_workspace(native_gpu):
    import torch
    from cvx_proj_amd import resident
    cases, q, t, rec_q, rec_t, qo, to, r2 = batch_arrays()
    host = native_gpu.match_guided_batch(q[qo[0]:], t[to[0]:], rec_q[qo[0]:], rec_t[to[0]:], np.diff(qo), np.diff(to), S.KIND_POINT, r2,
                                         reverse=True)
    dev = torch.device("cuda", 0)
    tq, tt = torch.from_numpy(q[qo[0]:]).to(dev), torch.from_numpy(t[to[0]:]).to(dev)
    trq, trt = torch.from_numpy(rec_q[qo[0]:]).to(dev), torch.from_numpy(rec_t[to[0]:]).to(dev)
    need = resident.guided_workspace_bytes(np.diff(qo), np.diff(to))
    assert need > 0 and need % 256 == 0
    work = torch.full((need,), 0x5A, dtype=torch.uint8, device=dev)      # dirty
    res = resident.hip_guided_match_batch(tq, tt, trq, trt, np.diff(qo), np.diff(to), S.KIND_POINT, r2, reverse=True, work=work)
    same_bytes([x.cpu().numpy() for x in res], host, "resident batch")
    lo, hi, a, b = qo[2] - qo[0], qo[3] - qo[0], to[2] - to[0], to[3] - to[0]      # pair 2 alone, through the _device single form
    one = resident.hip_guided_match(tq[lo:hi].contiguous(), tt[a:b].contiguous(), trq[lo:hi].contiguous(), trt[a:b].contiguous(),
                                    S.KIND_POINT, float(r2[2]), reverse=True, work=work)
    same_bytes([x.cpu().numpy() for x in one], S.match_int(*cases[2]), "resident single")
    # the single host-buffer C entry point, without the optional outputs
    c = cases[2]
    idx, dist = np.full(len(c.q), -5, np.int32), np.full(len(c.q), -5, np.float32)
    native_gpu.check(native_gpu.lib().apap_match_guided(
        None, native_gpu._dp(c.rec_q), native_gpu._ptr(c.q, C.c_float), len(c.q), native_gpu._dp(c.rec_t),
        native_gpu._ptr(c.t, C.c_float), len(c.t), S.KIND_POINT, float(c.r2), native_gpu._ip(idx), native_gpu._ptr(dist, C.c_float),
        None, None, None, None, None, -1))
    same_bytes((idx, dist), S.match_int(*c)[:2], "C single")


def test_records_byte_for_byte(native_gpu):
    import torch
    from cvx_proj_amd import resident
    rng = np.random.default_rng(25)
    pts = (rng.random((300, 2)) * [640, 480]).astype(np.float32)
    pts[7] = [np.nan, 3]
    pts[8] = [np.inf, -np.inf]
    pts[9] = [0, 0]
    dev = torch.device("cuda", 0)
    tp = torch.from_numpy(pts).to(dev)
    for M in (S.H_SCENE, np.array([[1, 0, 0], [0, 1, 0], [1, 1, 0.0]]), rng.normal(0, 1, (3, 3))):      # the second: s = 0 at (0, 0)
        for name, what in (("point", S.POINT), ("project", S.PROJECT), ("line", S.LINE)):
            want = S.records(pts, M, what)
            got = native_gpu.guided_records(pts, None if what == S.POINT else M, name)
            same_f64(got, want, name)
            res = resident.hip_guided_records(tp, None if what == S.POINT else torch.from_numpy(M).to(dev), name)
            assert res.cpu().numpy().tobytes() == got.tobytes(), name      # host-buffer against _device: every byte
            assert np.isnan(want[7]).any() and not np.isfinite(want[8, :2]).any()
    one = native_gpu.guided_records(pts[:1], S.H_SCENE, "project")
    same_f64(one, S.records(pts[:1], S.H_SCENE, S.PROJECT))


def test_python_surface(native_gpu):
    """guided_match under H, F and a grid against the specification; ratio and cross_check from one call; rematch."""
    from cvx_proj_amd import guided
    q_pts, q_desc, t_pts, t_desc, H, perm = S.scene(0)
    # H maps train (other) -> query (centre): the convention of guided_match
    ms = guided.guided_match(q_pts, q_desc, t_pts, t_desc, H=H, radius=6.0)
    want = S.match_int(q_desc, t_desc, *S.scene_records(q_pts, t_pts, H), S.KIND_POINT, 36.0)
    keep = np.flatnonzero(want[0] >= 0)
    assert [m.queryIdx for m in ms] == keep.tolist() and [m.trainIdx for m in ms] == want[0][keep].tolist()
    assert np.array_equal(np.float32([m.distance for m in ms]), want[1][keep])
    assert np.mean(want[0] == perm) >= 0.95
    mutual = guided.guided_match(q_pts, q_desc, t_pts, t_desc, H=H, radius=6.0, ratio=0.9, cross_check=True)
    ok = S.MS.filters(want[0], want[1], want[3], want[5], ratio=0.9, cross_check=True)
    assert [m.queryIdx for m in mutual] == ok.tolist() and 0 < len(mutual) <= len(ms)
    # F: the epipolar line of the centre keypoint in the other picture
    F = np.array([[0, -1e-3, 0.2], [1e-3, 0, -0.3], [-0.25, 0.31, 1.0]])
    mf = guided.guided_match(q_pts, q_desc, t_pts, t_desc, F=F, radius=2.0)
    wf = S.match_int(q_desc, t_desc, S.records(q_pts, F, S.LINE), S.records(t_pts), S.KIND_LINE, 4.0)
    assert [(m.queryIdx, m.trainIdx) for m in mf] == [(int(i), int(wf[0][i])) for i in np.flatnonzero(wf[0] >= 0)]
    # a 1 x 1 grid: centre -> other through the one cell
    Hinv = np.linalg.inv(H)
    grid = (Hinv[None, None], np.array([[0.0, 700.0], [0.0, 500.0]]), (0, 0))
    mg = guided.guided_match(q_pts, q_desc, t_pts, t_desc, grid=grid, radius=6.0)
    from cvx_proj_amd.evaluate import project_through_grid
    proj = project_through_grid(*grid, q_pts)
    wg = S.match_int(q_desc, t_desc, np.c_[proj, np.ones(len(proj))], S.records(t_pts), S.KIND_POINT, 36.0)
    assert [(m.queryIdx, m.trainIdx) for m in mg] == [(int(i), int(wg[0][i])) for i in np.flatnonzero(wg[0] >= 0)]
    src, dst, cf, of = guided.guided_matched_arrays(q_pts, q_desc, t_pts, t_desc, H=H, radius=6.0)
    assert np.array_equal(src, q_pts[keep]) and np.array_equal(dst, t_pts[want[0][keep]]) and np.array_equal(of, t_desc[want[0][keep]])


def test_rematch_keeps_what_the_reference_keeps(native_gpu, golden):
    from types import SimpleNamespace
    from cvx_proj_amd import guided
    g = golden("guided_ref")
    opts = SimpleNamespace(em_radius=float(g["em_radius"]), score_thresh=float(g["score_thresh"]))
    kc, fc, ko, fo, matches = guided.rematch(g["pts_c"], g["feats_c"].astype(np.float32), g["pts_o"], g["feats_o"].astype(np.float32),
                                             g["H"], opts)
    assert [m.queryIdx for m in matches] == g["query_idx"].tolist() and [m.trainIdx for m in matches] == g["train_idx"].tolist()
    assert np.array_equal(np.float32([m.distance for m in matches]), g["distance"])
    assert kc[3].pt == tuple(float(v) for v in g["pts_c"][3]) and fc.dtype == np.float32 and len(ko) == len(fo)
    assert g["reference_mask"].all()
