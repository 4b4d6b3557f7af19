"""Exact descriptor matching on the MI355X (apap_match_descriptors and its batch, resident and Python forms) against the
numpy brute force of tests/match_spec.py: bit for bit on integer-valued descriptors (the float32 sum of squared differences
is exact there), within a derived bound on float descriptors."""
import types

import numpy as np
import pytest

import match_spec as S

pytestmark = pytest.mark.gpu

NAMES = ("idx", "dist", "idx2", "dist2")


@pytest.fixture(scope="module")
def native_gpu(native):
    if native.lib().apap_device_count() < 1:
        pytest.skip("no HIP device")
    return native


def ints(rng, n):
    return rng.integers(0, 256, (n, S.DIM)).astype(np.float32)


def same_bytes(got, want, what=""):
    for name, g, w in zip(NAMES, got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, w.dtype, g.shape, w.shape)
        assert g.tobytes() == w.tobytes(), (what, name, int(np.count_nonzero(g.view(np.int32) != w.view(np.int32))))


def edge_shapes(native):
    """Shapes at the edges of the implementation's own tiling, from the constants the binding exposes: nt one below and one
    above the train chunk, and one below and one above the largest nt that still gets one chunk per split."""
    T, QT, want = native.MATCH_TRAIN_CHUNK, native.MATCH_QUERY_TILE, native.MATCH_WANT_BLOCKS
    nq = 64 * QT + 1                       # 65 query tiles
    splits = -(-want // 65)                # ... so up to this many one-chunk splits
    below, above = (nq, splits * T - 1), (nq, splits * T + 1)
    assert native.match_splits(*below) == (splits, 1) and native.match_splits(*above) == (-(-(splits + 1) // 2), 2)
    assert native.match_splits(QT + 1, T - 1) == (1, 1) and native.match_splits(QT + 1, T + 1) == (2, 1)
    return [(QT + 1, T - 1), (QT + 1, T + 1), below, above]


SHAPES = [(1, 1), (1, 2), (2, 1), (63, 64), (64, 65), (65, 63), (257, 300), (3, 5000), (5000, 3)]


@pytest.mark.parametrize("shape", SHAPES + ["chunk-1", "chunk+1", "splits-1", "splits+1"], ids=str)
def test_exact_on_integer_descriptors(native_gpu, shape):
    if isinstance(shape, str):
        shape = edge_shapes(native_gpu)[("chunk-1", "chunk+1", "splits-1", "splits+1").index(shape)]
    nq, nt = shape
    rng = np.random.default_rng(1000 * nq + nt)
    q, t = ints(rng, nq), ints(rng, nt)
    want = S.match_int(q, t)
    same_bytes(native_gpu.match_descriptors(q, t), want, "float32 input")
    same_bytes(native_gpu.match_descriptors(q.astype(np.uint8), t.astype(np.uint8)), want, "uint8 input")


def test_ties_go_to_the_lowest_index(native_gpu):
    rng = np.random.default_rng(2)
    nt = 5000
    t = ints(rng, nt)
    t[nt - 1] = t[1]
    q = np.stack([t[1], t[1]])
    idx, dist, idx2, dist2 = native_gpu.match_descriptors(q, t)
    assert idx.tolist() == [1, 1] and idx2.tolist() == [nt - 1, nt - 1] and dist.tolist() == [0.0, 0.0] and dist2.tolist() == [0.0, 0.0]
    # every train row the same: the two lowest indices
    idx, dist, idx2, dist2 = native_gpu.match_descriptors(q, np.tile(t[1], (300, 1)))
    assert idx.tolist() == [0, 0] and idx2.tolist() == [1, 1] and dist2.tolist() == [0.0, 0.0]


@pytest.mark.parametrize("first,second", [(5, 6), (6, 5), (3, 3 + 64), (130, 2), (2, 130), (127, 128), (700, 100), (4999, 0)])
def test_planted_nearest_and_second(native_gpu, first, second):
    """Nearest and runner-up at chosen rows: in one thread's tile, in one chunk, in different chunks and splits."""
    rng = np.random.default_rng(3)
    t = rng.integers(100, 256, (5000, S.DIM)).astype(np.float32)
    q = np.zeros((2, S.DIM), np.float32)
    t[first] = 0
    t[first, 0] = 1
    t[second] = 0
    t[second, :4] = 1
    idx, dist, idx2, dist2 = native_gpu.match_descriptors(q, t)
    assert idx.tolist() == [first] * 2 and idx2.tolist() == [second] * 2 and dist.tolist() == [1.0] * 2 and dist2.tolist() == [2.0] * 2
    same_bytes((idx, dist, idx2, dist2), S.match_int(q, t))


def test_largest_exact_distance(native_gpu):
    q = np.zeros((1, S.DIM), np.float32)
    t = np.full((2, S.DIM), 255, np.float32)
    t[1, 0] = 254
    idx, dist, idx2, dist2 = native_gpu.match_descriptors(q, t)
    assert (idx[0], idx2[0]) == (1, 0)
    assert dist2[0] == np.sqrt(np.float32(8323200)) and dist[0] == np.sqrt(np.float32(8323200 - 509))
    same_bytes((idx, dist, idx2, dist2), S.match_int(q, t))


def test_nearest_only(native_gpu):
    rng = np.random.default_rng(4)
    q, t = ints(rng, 130), ints(rng, 700)
    idx, dist, idx2, dist2 = native_gpu.match_descriptors(q, t, second=False)
    assert idx2 is None and dist2 is None
    want = S.match_int(q, t)
    same_bytes((idx, dist), want[:2])
    r = native_gpu.match_descriptors(q[:1], t[:1])
    assert (r[0][0], r[2][0], r[3][0]) == (0, -1, np.inf)


def float_sets():
    rng = np.random.default_rng(5)
    nq, nt = 130, 150
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)     # noqa: E731
    sets = {"N(0,1)": (f32(rng.normal(0, 1, (nq, S.DIM))), f32(rng.normal(0, 1, (nt, S.DIM)))),
            "N(0,1e4)": (f32(rng.normal(0, 1e4, (nq, S.DIM))), f32(rng.normal(0, 1e4, (nt, S.DIM))))}
    a, b = rng.normal(0, 1, (nq, S.DIM)), rng.normal(0, 1, (nt, S.DIM))
    sets["unit"] = (f32(a / np.linalg.norm(a, axis=1, keepdims=True)), f32(b / np.linalg.norm(b, axis=1, keepdims=True)))
    base = 100 + rng.normal(0, 1, (75, S.DIM))
    train = np.empty((nt, S.DIM))
    train[0::2], train[1::2] = base, base + rng.normal(0, 2e-2, base.shape)
    sets["near-duplicate"] = (f32(base[rng.integers(0, 75, nq)] + rng.normal(0, 1.5e-2, (nq, S.DIM))), f32(train))
    return sets


@pytest.mark.parametrize("name", ["N(0,1)", "N(0,1e4)", "unit", "near-duplicate"])
def test_float_descriptors_within_the_derived_bound(native_gpu, name):
    q, t = float_sets()[name]
    idx, dist, idx2, dist2 = native_gpu.match_descriptors(q, t)
    d = S.d2_f64(q, t)
    rows = np.arange(len(q))
    assert idx.min() >= 0 and idx2.min() >= 0 and not np.any(idx == idx2)
    chosen, best = d[rows, idx], d.min(axis=1)
    print(name, "nearest: max d64(chosen) / min d64 - 1 =", float((chosen / best - 1).max()), "wrong neighbours:",
          int(np.count_nonzero(idx != d.argmin(axis=1))))
    assert np.all(chosen <= (1 + S.EPS) * best)
    rest = d.copy()
    rest[rows, idx] = np.inf
    chosen2, best2 = d[rows, idx2], rest.min(axis=1)
    print(name, "second: max ratio - 1 =", float((chosen2 / best2 - 1).max()))
    assert np.all(chosen2 <= (1 + S.EPS) * best2)
    for got, true in ((dist, chosen), (dist2, chosen2)):
        err = np.abs(got.astype(np.float64) - np.sqrt(true))
        print(name, "distance: max relative error", float((err / np.sqrt(true)).max()), "bound", S.GAMMA)
        assert np.all(err <= S.GAMMA * np.sqrt(true))


def test_nan_is_never_selected(native_gpu):
    rng = np.random.default_rng(6)
    q, t = ints(rng, 70), ints(rng, 200)
    clean = S.match_int(np.delete(q, 5, axis=0), np.delete(t, 7, axis=0))
    q[5, 17] = np.nan
    t[7, 100] = np.nan
    idx, dist, idx2, dist2 = native_gpu.match_descriptors(q, t)
    assert (idx[5], idx2[5], dist[5], dist2[5]) == (-1, -1, np.inf, np.inf)
    assert not np.any(idx == 7) and not np.any(idx2 == 7)
    others = np.arange(70) != 5
    lift = lambda i: i + (i >= 7)     # noqa: E731   indices of the train set without row 7 -> with it
    same_bytes((idx[others], dist[others], idx2[others], dist2[others]), (lift(clean[0]), clean[1], lift(clean[2]), clean[3]))
    # a train set of NaN rows only: nothing to select
    r = native_gpu.match_descriptors(q[:3], np.full((2, S.DIM), np.nan, np.float32))
    assert r[0].tolist() == [-1] * 3 and r[2].tolist() == [-1] * 3 and np.all(np.isinf(r[1])) and np.all(np.isinf(r[3]))


RAGGED = [(1, 1), (2, 7), (65, 64), (300, 257), (40, 5000), (2000, 2000)]


@pytest.fixture(scope="module")
def ragged(native_gpu):
    """The ragged pairs and every pair's own single call, computed once."""
    rng = np.random.default_rng(7)
    pairs = [(ints(rng, nq), ints(rng, nt)) for nq, nt in RAGGED]
    return pairs, [native_gpu.match_descriptors(q, t) for q, t in pairs]


def split_like(arrays, lengths):
    at = np.cumsum([0] + list(lengths))
    return [tuple(a[at[p]:at[p + 1]] for a in arrays) for p in range(len(lengths))]


@pytest.mark.parametrize("order", [(0, 1, 2, 3, 4, 5), (5, 3, 0, 4, 2, 1)], ids=["in order", "permuted"])
def test_batch_equals_the_single_calls(native_gpu, ragged, order):
    pairs, singles = ragged
    qs, ts = [pairs[p][0] for p in order], [pairs[p][1] for p in order]
    out = native_gpu.match_descriptors_batch(np.concatenate(qs), np.concatenate(ts), [len(x) for x in qs], [len(x) for x in ts])
    for p, got in zip(order, split_like(out, [len(x) for x in qs])):
        same_bytes(got, singles[p], f"pair {p}")
    # one of the singles against the specification, so that the chain ends in numpy
    same_bytes(singles[3], S.match_int(*pairs[3]))


def test_two_calls_give_the_same_bytes(native_gpu, ragged):
    pairs, singles = ragged
    same_bytes(native_gpu.match_descriptors(*pairs[5]), singles[5])
    same_bytes(native_gpu.match_descriptors(*pairs[4]), singles[4])


def test_resident_forms_equal_the_host_buffer_forms(native_gpu, ragged):
    import torch
    from cvx_proj_amd import resident
    pairs, singles = ragged
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    ql, tl = [len(q) for q, _ in pairs], [len(t) for _, t in pairs]
    with torch.cuda.stream(stream):
        q, t = torch.from_numpy(pairs[3][0]).to(dev), torch.from_numpy(pairs[3][1]).to(dev)
        nbytes = resident.match_workspace_bytes(len(q), len(t))
        assert nbytes > 0 and nbytes % 256 == 0
        work = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        one = resident.hip_match_descriptors(q, t, work=work)
        near = resident.hip_match_descriptors(q, t, second=False, work=work)
        Q = torch.from_numpy(np.concatenate([q for q, _ in pairs])).to(dev)
        T = torch.from_numpy(np.concatenate([t for _, t in pairs])).to(dev)
        bwork = torch.empty(resident.match_workspace_bytes(ql, tl), dtype=torch.uint8, device=dev)
        many = resident.hip_match_descriptors_batch(Q, T, ql, tl, work=bwork)
    stream.synchronize()
    same_bytes([x.cpu().numpy() for x in one], singles[3], "single")
    assert near[2] is None and near[3] is None
    same_bytes([x.cpu().numpy() for x in near[:2]], singles[3][:2], "nearest only")
    for p, got in enumerate(split_like([x.cpu().numpy() for x in many], ql)):
        same_bytes(got, singles[p], f"pair {p}")
    with pytest.raises(native_gpu.ApapError):     # a short workspace is refused, not replaced: _scratch replaces only None
        native_gpu.check(native_gpu.lib().apap_match_descriptors_device(None, q.data_ptr(), len(q), t.data_ptr(), len(t), one[0].data_ptr(),
                                                                        one[1].data_ptr(), None, None, work.data_ptr(), 256, None))


def scene():
    """400 train keypoints with integer descriptors; 300 queries: a permuted subset moved by a known homography, 15 % of
    them with unrelated descriptors."""
    rng = np.random.default_rng(8)
    pts_o = rng.uniform(0, 1000, (400, 2))
    feats_o = rng.integers(0, 256, (400, S.DIM)).astype(np.uint8)
    pick = rng.permutation(400)[:300]
    Hm = np.array([[1.02, 0.01, 30.0], [-0.015, 0.99, -12.0], [1e-5, -2e-5, 1.0]])
    h = np.hstack([pts_o[pick], np.ones((300, 1))]) @ np.linalg.inv(Hm).T
    pts_c = h[:, :2] / h[:, 2:]
    feats_c = np.clip(feats_o[pick].astype(np.int64) + rng.integers(-6, 7, (300, S.DIM)), 0, 255).astype(np.uint8)
    unrelated = rng.random(300) < 0.15
    feats_c[unrelated] = rng.integers(0, 256, (int(unrelated.sum()), S.DIM))
    F = np.array([[0, -1e-6, 1e-3], [1e-6, 0, -2e-3], [-1e-3, 2e-3, 1e-2]])
    return pts_c, feats_c, pts_o, feats_o, F, (~unrelated).astype(np.float32), Hm.astype(np.float32)


def test_composition_with_the_spectral_path(native_gpu):
    from cvx_proj_amd import matching
    from cvx_proj_amd import spectral_method as SM
    pts_c, feats_c, pts_o, feats_o, F, mask, Hm = scene()
    idx = S.match_int(feats_c, feats_o)[0]
    assert np.count_nonzero(idx[mask > 0] >= 0) == int(mask.sum())
    want_arrays = (pts_c.astype(np.float32), pts_o[idx].astype(np.float32), feats_c.astype(np.float32), feats_o[idx].astype(np.float32))
    got_arrays = matching.matched_arrays(pts_c, feats_c, pts_o, feats_o)
    for g, w in zip(got_arrays, want_arrays):
        assert g.dtype == w.dtype and g.tobytes() == w.tobytes()
    got = SM.spectral_em(*got_arrays, F, em_steps=2, mask=mask)
    want = SM.spectral_em(*want_arrays, F, em_steps=2, mask=mask)
    assert got.H_save.tobytes() == want.H_save.tobytes()
    for g, w in zip(got.rounds, want.rounds):
        assert g.H_pred.tobytes() == w.H_pred.tobytes()
        for name in ("segment", "ransac_mask", "original_mask"):
            assert getattr(g.spectral, name).tobytes() == getattr(w.spectral, name).tobytes(), name
    # the reference's tuple through calculate_M
    opts = types.SimpleNamespace(epi_weight=0.5, affinity_eps=30.0, aff_thresh=0.5, em_radius=6.0, score_thresh=0.4)
    kc, fc, ko, fo, matches = matching.coarse_matching(pts_c, feats_c, pts_o, feats_o)
    assert [m.queryIdx for m in matches] == list(range(300)) and [m.trainIdx for m in matches] == idx.tolist()
    seg, H, rm, om = SM.calculate_M(kc, fc, ko, fo, F, matches, opts, Hg=Hm)
    ref = SM.spectral_weights(*want_arrays, F, Hg=Hm)
    assert seg.tobytes() == ref.segment.tobytes() and rm.tobytes() == ref.ransac_mask.tobytes() and \
        om.tobytes() == ref.original_mask.tobytes()


def test_python_filters(native_gpu):
    from cvx_proj_amd import matching
    _, feats_c, _, feats_o, _, _, _ = scene()
    idx, dist, idx2, dist2 = S.match_int(feats_c, feats_o)
    back = S.match_int(feats_o, feats_c)[0]
    plain = matching.match(feats_c, feats_o)
    assert [(m.queryIdx, m.trainIdx, m.distance, m.imgIdx) for m in plain] == [(i, int(idx[i]), float(dist[i]), 0) for i in range(300)]
    for kw in ({"ratio": 0.8}, {"cross_check": True}, {"ratio": 0.8, "cross_check": True}):
        keep = S.filters(idx, dist, dist2, back, **kw)
        got = matching.match(feats_c, feats_o, **kw)
        assert 0 < len(keep) < 300, kw       # the filter bites, and not everything
        assert [(m.queryIdx, m.trainIdx, m.distance) for m in got] == [(int(i), int(idx[i]), float(dist[i])) for i in keep], kw
    r = matching.match_descriptors(feats_c, feats_o)
    same_bytes(tuple(r), (idx, dist, idx2, dist2))
