"""The inputs of the guided-matching tests reach the edges they are made for, by the specification alone (no GPU)."""
import numpy as np

import guided_match_cases as GC
import guided_match_spec as S


def test_the_cases_are_the_ones_that_were_checked():
    named = GC.named()
    assert set(named) == set(GC.DIGEST)
    for name, case in named.items():
        assert GC.digest(case) == GC.DIGEST[name], name
        assert case.q.dtype == case.t.dtype == np.float32 and case.rec_q.dtype == case.rec_t.dtype == np.float64, name
        assert case.q.shape == (len(case.rec_q), 128) and case.t.shape == (len(case.rec_t), 128), name


def test_size_shapes_sit_on_the_tiling_constants(native):
    QT, T, D, want = native.GUIDED_QUERY_TILE, native.GUIDED_TRAIN_CHUNK, native.GUIDED_DRAIN, native.GUIDED_WANT_BLOCKS
    shapes = GC.size_shapes(native)
    nqs, nts = {a for a, _ in shapes}, {b for _, b in shapes}
    assert {1, 2, QT - 1, QT, QT + 1, D - 1, D, D + 1} <= nqs and {1, 2, T - 1, T, T + 1, D - 1, D, D + 1} <= nts
    assert {want * T - 1, want * T, want * T + 1} <= nts
    assert native.guided_splits(2, want * T - 1) == (want, 1) and native.guided_splits(2, want * T + 1)[1] == 2
    assert native.guided_splits(QT + 1, T + 1) == (2, 1) and native.guided_splits(2 * QT + 1, 2 * T + 1) == (3, 1)
    # more than one block along the queries, more than one chunk, more than one drain of a wave's list in one run
    case = GC.sized(2 * QT + 1, 2 * T + 1)
    count = S.match_int(*case)[4]
    assert count[:D].sum() > 2 * D


def test_named_cases_reach_their_edges():
    case, special = GC.one_admits_all()
    count = S.match_int(*case)[4]
    assert count[special] == len(case.t) == 300 and 0 < special < 199
    assert set(np.delete(count, special).tolist()) == {0, 1, 2}
    inside, outside = GC.duplicates(True), GC.duplicates(False)
    d = S.d2_int(inside.q, inside.t)
    assert d[0, 3] == d[0, 9] == 0 and (np.delete(d[0], [3, 9]) > 0).all()
    assert S.gate(inside.rec_q, inside.rec_t, 0, inside.r2)[0, [3, 9]].tolist() == [True, True]
    assert S.gate(outside.rec_q, outside.rec_t, 0, outside.r2)[0, [3, 9]].tolist() == [False, True]
    at = GC.three_four(25.0)
    assert S.gate_value(at.rec_q, at.rec_t, 0)[0][0, 0] == 25.0 and np.nextafter(25.0, np.inf) > 25.0
    lines = GC.line_cases()
    left, n = S.gate_value(lines.rec_q, lines.rec_t, 1)
    assert n[0] == 0 and (left[1, :2] == 25.0).all() and (left[2, :2] == 100.0).all() and n[2] == 4.0      # exactly at distance r
    assert (left[1, 2:4] < 25.0).all() and np.isnan(left[3]).all()
    nf = GC.non_finite_records()
    assert np.isnan(nf.rec_q[1, 0]) and np.isposinf(nf.rec_q[2, 0]) and np.isneginf(nf.rec_q[3, 0])
    assert np.isnan(nf.rec_t[4, 0]) and np.isposinf(nf.rec_t[4, 1])      # s = 0 in PROJECT: 0 / 0 and 3 / 0
    nd = GC.non_finite_descriptors()
    assert S.gate(nd.rec_q, nd.rec_t, 0, nd.r2).all()
    assert np.isnan(nd.t[1]).any() and np.isinf(nd.t[2]).any() and np.isnan(nd.q[2]).any()
    cases, q0, t0 = GC.batch_pairs()
    assert q0 > 0 and t0 > 0 and {1, 300} <= {len(c.q) for c in cases} | {len(c.t) for c in cases}
    assert len({c.r2 for c in cases}) == len(cases) and 0.0 in {c.r2 for c in cases} and np.inf in {c.r2 for c in cases}
    for c in cases:      # no gate value on the edge of its own r2: neither arithmetic decides a pair
        g = S.gate_value(c.rec_q, c.rec_t, 0)[0]
        assert c.r2 in (0.0, np.inf) or np.abs(g / c.r2 - 1).min() > 1e-9


def test_order_count_and_reverse_side_of_the_specification():
    d = np.array([[5.0, 1.0, 1.0, np.inf], [2.0, 2.0, 7.0, 0.0], [3.0, np.nan, 3.0, 3.0]])
    passes = np.array([[True, True, True, True], [False, True, True, False], [False, True, False, False]])
    idx, dist, idx2, dist2, count, ridx, rdist = S.select(d, passes)
    assert idx.tolist() == [1, 1, -1] and idx2.tolist() == [2, 2, -1] and count.tolist() == [4, 2, 1]
    assert dist.tolist() == [1.0, np.float32(np.sqrt(np.float32(2))), np.inf] and dist2[2] == np.inf
    assert ridx.tolist() == [0, 0, 0, -1] and rdist.tolist() == [np.float32(np.sqrt(np.float32(5))), 1.0, 1.0, np.inf]
    one = S.select(np.array([[4.0]]), np.array([[True]]))
    assert (one[0][0], one[2][0], one[3][0], one[5][0]) == (0, -1, np.inf, 0)
