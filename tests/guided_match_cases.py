"""Inputs of the guided-matching tests (tests/test_guided_match_*.py, tests/test_gpu_guided_match.py).  Every case is a
``Case``: descriptors, records, kind and r2, generated from a seed; ``DIGEST`` pins the bytes of those built from integer
draws and correctly rounded operations alone (sha256, first 16 hex digits), so that a change of numpy's generators cannot move
a case off its edge unnoticed.  What each case is meant to reach is asserted
from the specification in tests/test_guided_match_inputs.py."""
from __future__ import annotations

import hashlib
from typing import NamedTuple

import numpy as np

import guided_match_spec as S

DIM = 128
INF = np.inf


class Case(NamedTuple):
    q: np.ndarray        # (nq, 128) float32, integer-valued unless the case says otherwise
    t: np.ndarray        # (nt, 128) float32
    rec_q: np.ndarray    # (nq, 3) float64
    rec_t: np.ndarray    # (nt, 3) float64
    kind: int
    r2: float


def digest(case):
    h = hashlib.sha256()
    for a in case[:4]:
        h.update(np.ascontiguousarray(a).tobytes())
    h.update(np.array([case.kind, case.r2], dtype=np.float64).tobytes())
    return h.hexdigest()[:16]


def ints(rng, n):
    return rng.integers(0, 256, (n, DIM)).astype(np.float32)


def point_recs(pts):
    return S.records(np.asarray(pts, dtype=np.float32))


def sized(nq, nt, seed=None):
    """``nq`` queries on a 100 x 100 field against ``nt`` train points, radius 12: a handful of candidates per query, some
    queries with none."""
    rng = np.random.default_rng(10_000 * nq + nt if seed is None else seed)
    qp, tp = rng.random((nq, 2)) * 100, rng.random((nt, 2)) * 100
    return Case(ints(rng, nq), ints(rng, nt), point_recs(qp), point_recs(tp), S.KIND_POINT, 144.0)


def size_shapes(native):
    """nq, nt in {1, 2} and one below, at and one above every tiling constant: the query tile, the train chunk, the drain (a
    wave's lanes), and the largest nt that still gets one chunk per split (one query tile)."""
    QT, T, D, want = native.GUIDED_QUERY_TILE, native.GUIDED_TRAIN_CHUNK, native.GUIDED_DRAIN, native.GUIDED_WANT_BLOCKS
    small = [(a, b) for a in (1, 2) for b in (1, 2)]
    edges = [(QT + d, 3) for d in (-1, 0, 1)] + [(3, T + d) for d in (-1, 0, 1)] + [(D + d, 70) for d in (-1, 0, 1)] + \
            [(70, D + d) for d in (-1, 0, 1)] + [(QT + 1, T + 1), (2 * QT + 1, 2 * T + 1)]
    assert native.guided_splits(1, want * T) == (want, 1) and native.guided_splits(1, want * T + 1) == (-(-(want + 1) // 2), 2)
    return small + edges + [(2, want * T - 1), (2, want * T), (2, want * T + 1)]


def look_alike(seed=0, radius=6.0):
    q_pts, q_desc, t_pts, t_desc, H, perm = S.scene(seed)
    rec_q, rec_t = S.scene_records(q_pts, t_pts, H)
    return Case(q_desc, t_desc, rec_q, rec_t, S.KIND_POINT, radius * radius), perm


def one_admits_all():
    """300 train points inside a disc of radius 5.9 px; query ``special`` at its centre admits every one of them at r2 = 36.
    The other 199 queries stand around the disc, each moved inwards from 12 px until its own disc holds 0, 1 or 2 train points
    (in turn).  Returns (case, special): the admitting query's row, somewhere inside the block."""
    rng = np.random.default_rng(77)
    c = np.array([1000.0, 1000.0])
    unit = lambda v: v / np.sqrt((v * v).sum(axis=-1, keepdims=True))      # noqa: E731  (+, *, /, sqrt only: the same bits everywhere)
    tp = (c + unit(rng.random((300, 2)) - 0.5) * (5.9 * np.sqrt(rng.random((300, 1))))).astype(np.float32)
    qp = [c]
    for k, a in enumerate(unit(rng.random((199, 2)) - 0.5)):
        p = None
        for D in np.arange(12.0, 6.0, -0.01):
            before, p = p, (c + D * a).astype(np.float32)
            admitted = S.gate(S.records(p[None]), S.records(tp), S.KIND_POINT, 36.0).sum()
            if admitted >= k % 3:
                break
        qp.append(p if admitted <= 2 else before)      # a step that took in several points at once: one step back
    order = rng.permutation(200)
    qp = np.asarray(qp, dtype=np.float32)[order]
    return Case(ints(rng, 200), ints(rng, 300), S.records(qp), S.records(tp), S.KIND_POINT, 36.0), int(np.flatnonzero(order == 0)[0])


def duplicates(lower_inside):
    """Train rows 3 and 9 hold the query's own descriptor (d2 = 0 both).  Both inside the gate: row 3 wins; row 3 outside
    the gate: row 9 wins."""
    rng = np.random.default_rng(5)
    q, t = ints(rng, 2), ints(rng, 12)
    t[3] = t[9] = q[0]
    tp = np.full((12, 2), 50.0) + rng.random((12, 2))
    qp = np.array([[50.5, 50.5], [50.5, 50.5]])
    if not lower_inside:
        tp[3] = [70.0, 70.0]
    return Case(q, t, point_recs(qp), point_recs(tp), S.KIND_POINT, 36.0)


def three_four(r2):
    """Integer coordinates, dx, dy = 3, 4: g = 25 exactly."""
    rng = np.random.default_rng(6)
    return Case(ints(rng, 1), ints(rng, 2), point_recs([[10, 20]]), point_recs([[13, 24], [100, 100]]), S.KIND_POINT, r2)


def line_cases():
    """LINE records: a null line (n = 0), a horizontal line y = 40 with train points exactly at distance 5, inside and outside;
    a NaN line; an infinite line."""
    rng = np.random.default_rng(8)
    rec_q = np.array([[0.0, 0.0, 1.0],            # n = 0: passes nothing
                      [0.0, 1.0, -40.0],          # y = 40
                      [0.0, 2.0, -80.0],          # the same line, scaled
                      [np.nan, 1.0, 0.0],
                      [np.inf, 1.0, 0.0],
                      [0.6, 0.8, -50.0]])         # 3-4-5 normal
    tp = np.array([[7, 45], [7, 35], [9, 44.5], [9, 35.5], [11, 40], [30, 40], [50, 25], [0, 0]], dtype=np.float64)
    return Case(ints(rng, 6), ints(rng, 8), rec_q, point_recs(tp), S.KIND_LINE, 25.0)


def non_finite_records():
    """POINT: NaN and +-inf records on both sides, and PROJECT records with s = 0 (inf or NaN coordinates)."""
    rng = np.random.default_rng(9)
    qp = np.array([[5, 5], [np.nan, 5], [np.inf, 5], [-np.inf, 5], [6, 6]], dtype=np.float32)
    tp = np.array([[5, 6], [np.nan, 6], [np.inf, 5], [6, 5], [0, 3], [2, 0]], dtype=np.float32)
    M = np.array([[1, 0, 0], [0, 1, 0], [1, 0, 0]], dtype=np.float64)      # s = X: train row 4 has s = 0, its record is (NaN, inf, 1)
    rec_t = S.records(tp, M, S.PROJECT)
    rec_t[:4] = S.records(tp[:4])
    return Case(ints(rng, 5), ints(rng, 6), S.records(qp), rec_t, S.KIND_POINT, 4.0)


def non_finite_descriptors():
    """Train row 1 holds a NaN, train row 2 an infinity, query 2 a NaN: inside the gate they are counted and never selected."""
    rng = np.random.default_rng(11)
    q, t = ints(rng, 3), ints(rng, 5)
    t[1, 17] = np.nan
    t[2, 100] = np.inf
    q[2, 0] = np.nan
    pts = np.full((5, 2), 10.0)
    return Case(q, t, point_recs(pts[:3]), point_recs(pts), S.KIND_POINT, 1.0)


def batch_pairs():
    """Pairs of 1 to 300 rows mixed, each with its own r2 (0 and +inf among them); the first offsets are above 0."""
    shapes = [(1, 300), (300, 1), (130, 300), (2, 2), (257, 129), (64, 65)]
    r2 = [144.0, INF, 100.0, 0.0, 225.0, 400.0]
    cases = []
    for k, ((nq, nt), r) in enumerate(zip(shapes, r2)):
        c = sized(nq, nt, seed=500 + k)
        cases.append(c._replace(r2=r))
    return cases, 5, 7       # the first query row and the first train row of the batch


def named():
    """The named cases, for the digests and the tests that walk them all."""
    out = {"one_admits_all": one_admits_all()[0], "duplicates_inside": duplicates(True),
           "duplicates_outside": duplicates(False), "three_four_at": three_four(25.0),
           "three_four_above": three_four(float(np.nextafter(25.0, np.inf))), "lines": line_cases(),
           "non_finite_records": non_finite_records(), "non_finite_descriptors": non_finite_descriptors(),
           "sized_257_129": sized(257, 129)}
    out.update({f"batch_{k}": c for k, c in enumerate(batch_pairs()[0])})
    return out


DIGEST = {'one_admits_all': '5a3adc21644b1af7',
 'duplicates_inside': '623326e6095b9c01',
 'duplicates_outside': '4110c9adbf5ff8d8',
 'three_four_at': '27ed7c8b1240f25d',
 'three_four_above': '9f86dfb91dc9909b',
 'lines': '1f49d5396e5a7d6d',
 'non_finite_records': 'c44cb0bd89d7ce96',
 'non_finite_descriptors': '7194343b2d19c1e6',
 'sized_257_129': 'cffe0c84db39d8e2',
 'batch_0': '0c7dfc5677552b38',
 'batch_1': 'c5e74a827c8d9f9e',
 'batch_2': 'fdfbd7da5593a7fb',
 'batch_3': 'd6fa5a29d8d2695c',
 'batch_4': '22b4f55b0d24be12',
 'batch_5': '66fda9bc25585fe3'}
