"""The exact matcher's bytes on float descriptors, on the MI355X: all four outputs against tests/match_spec.py's match_f32,
the float32 sum restated step by step in numpy (128 sequential subtractions and single-rounding fused multiply-adds from 0,
the (d2, index) order, the correctly rounded root).  The guided matcher's float tests compare against the matcher
(test_gpu_guided_match.py), so this pins their bytes as well.

Shapes: (1, 1), and (65, 129) - two query tiles, two train chunks and two splits, the last of each ragged - alone and
together in one batch.  Inputs: N(0, 1), and near-duplicate train rows (odd rows are even rows plus 1e-3 noise), where the
order is decided in the last bits of d2.  Beside them, equal distances where the block's merge does not meet the train rows
in the order of their indices, so that the index comparison alone decides."""
import numpy as np
import pytest

import match_spec as S

pytestmark = pytest.mark.gpu

NAMES = ("idx", "dist", "idx2", "dist2")
SHAPES = [(1, 1), (65, 129)]


@pytest.fixture(scope="module")
def native_gpu(native):
    if native.lib().apap_device_count() < 1:
        pytest.skip("no HIP device")
    return native


def descriptors(kind, nq, nt):
    rng = np.random.default_rng(31 + nq + nt)
    q, t = rng.normal(0, 1, (nq, S.DIM)).astype(np.float32), rng.normal(0, 1, (nt, S.DIM)).astype(np.float32)
    if kind == "near-duplicate":
        t[1::2] = t[0::2][:nt // 2] + rng.normal(0, 1e-3, (nt // 2, S.DIM)).astype(np.float32)
    return q, t


@pytest.fixture(scope="module")
def cases():
    """Every (kind, shape): the descriptors and the specification's four arrays, computed once."""
    out = {}
    for kind in ("N(0,1)", "near-duplicate"):
        for nq, nt in SHAPES:
            q, t = descriptors(kind, nq, nt)
            out[kind, (nq, nt)] = (q, t, S.match_f32(q, t))
    return out


def same_bytes(got, want, what):
    for name, g, w in zip(NAMES, got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, w.dtype, g.shape, w.shape)
        differ = np.flatnonzero(g.view(np.int32) != w.view(np.int32))
        print(what, name, "values that differ:", len(differ), "of", g.size)
        assert g.tobytes() == w.tobytes(), (what, name, differ[:8].tolist(), g[differ[:8]].tolist(), w[differ[:8]].tolist())


@pytest.mark.parametrize("kind", ["N(0,1)", "near-duplicate"])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_float_bytes_equal_the_restated_sum(native_gpu, cases, kind, shape):
    assert native_gpu.match_splits(65, 129) == (2, 1) and -(-65 // native_gpu.MATCH_QUERY_TILE) == 2
    q, t, want = cases[kind, shape]
    same_bytes(native_gpu.match_descriptors(q, t), want, f"{kind} {shape}")
    if kind == "near-duplicate" and shape == (65, 129):
        # the construction bites: the two nearest of most queries are a pair of duplicates, closer to each other in d2 than
        # the derived bound of the float32 sum could tell apart from a float64 distance
        d = S.d2_f64(q, t)
        rows = np.arange(len(q))
        gap = np.abs(d[rows, want[0]] - d[rows, want[2]]) / d[rows, want[0]]
        assert np.count_nonzero((want[0] // 2 == want[2] // 2) & (gap < 100 * S.EPS)) >= len(q) // 2


def test_ties_that_the_merge_meets_out_of_index_order(native_gpu):
    """A thread of k_match_sweep owns rows 4 tx .. 4 tx + 3 and 64 + 4 tx .. 64 + 4 tx + 3 of a chunk, and a query's 16
    threads are merged in the order of tx: thread 0's row 64 comes before thread 1's row 4.  Equal distances there are
    decided by the index comparison of the shared order alone (the fold's strict comparisons never see them)."""
    rng = np.random.default_rng(32)
    q, t = (rng.integers(0, 256, (n, S.DIM)).astype(np.float32) for n in (3, 200))
    t[4] = t[64] = q[0]                      # the best, twice: 4 before 64
    t[130] = q[1]                            # the best in the next chunk ...
    t[9] = t[70] = q[1]
    t[9, 0] = t[70, 0] = q[1, 0] + 1         # ... and the runner-up twice: 9 before 70
    t[68] = t[8] = q[2]                      # thread 1's second half before thread 2's first
    want = S.match_int(q, t)
    assert (want[0].tolist(), want[2].tolist()) == ([4, 130, 8], [64, 9, 68])
    same_bytes(native_gpu.match_descriptors(q, t), want, "ties")


@pytest.mark.parametrize("kind", ["N(0,1)", "near-duplicate"])
def test_float_bytes_in_a_batch(native_gpu, cases, kind):
    qs, ts, wants = zip(*(cases[kind, shape] for shape in SHAPES))
    got = native_gpu.match_descriptors_batch(np.concatenate(qs), np.concatenate(ts), [len(q) for q in qs], [len(t) for t in ts])
    same_bytes(got, tuple(np.concatenate(w) for w in zip(*wants)), f"{kind} batch")
