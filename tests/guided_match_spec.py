"""Specification of guided descriptor matching in numpy (test infrastructure; the product never imports it).

* ``records`` and ``gate``: float64, one IEEE operation per numpy call, in the order include/apap_hip.h writes them.
* ``select``: the outputs from a matrix of squared distances and the gate's matrix - candidates ordered by (d2, index), a
  non-finite d2 counted and never selected, the reverse side from the transposed matrices.
* ``match_int``: the whole call for integer-valued descriptors, d2 in int64 (tests/match_spec.py), with rows that hold a NaN
  or an infinity struck out: their d2 is non-finite whatever the other row holds.
* ``scene``: the look-alike scene of the issue, draw by draw; ``rematch``: what ``guided.rematch`` selects.
"""
import numpy as np

import match_spec as MS

POINT, PROJECT, LINE = 0, 1, 2          # APAP_GUIDED_REC_*
KIND_POINT, KIND_LINE = 0, 1            # APAP_GUIDED_*
H_SCENE = np.array([[1.02, .01, 12], [-.015, .99, 7], [1e-5, -2e-5, 1]])     # train -> query


def records(pts, model=None, what=POINT):
    """(n, 3) float64 records of (n, 2) float32 points."""
    pts = np.asarray(pts, dtype=np.float32)
    X, Y = pts[:, 0].astype(np.float64), pts[:, 1].astype(np.float64)
    one = np.ones_like(X)
    if what == POINT:
        return np.stack([X, Y, one], axis=1)
    M = np.asarray(model, dtype=np.float64).reshape(9)
    with np.errstate(all="ignore"):
        u = (M[0] * X + M[1] * Y) + M[2]
        v = (M[3] * X + M[4] * Y) + M[5]
        s = (M[6] * X + M[7] * Y) + M[8]
        if what == PROJECT:
            return np.stack([u / s, v / s, one], axis=1)
    return np.stack([u, v, s], axis=1)


def gate_value(A, B, kind):
    """(left, right factor) of the comparison ``left < r2 * factor`` for every (query, train) pair: POINT (g, 1), LINE (e e, n)."""
    A, B = np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64)
    with np.errstate(all="ignore"):
        if kind == KIND_POINT:
            dx = B[None, :, 0] - A[:, None, 0]
            dy = B[None, :, 1] - A[:, None, 1]
            return dx * dx + dy * dy, None
        e = (A[:, None, 0] * B[None, :, 0] + A[:, None, 1] * B[None, :, 1]) + A[:, None, 2]
        n = A[:, 0] * A[:, 0] + A[:, 1] * A[:, 1]
        return e * e, n


def gate(A, B, kind, r2):
    """(nq, nt) bool: the pairs that pass.  Strict; a NaN fails."""
    left, n = gate_value(A, B, kind)
    with np.errstate(all="ignore"):
        bound = np.float64(r2) if n is None else (np.float64(r2) * n)[:, None]
        return left < bound


def _side(d, ok):
    """One side: rows of ``d`` (float64, inf = not selectable) over the columns where ``ok``."""
    n, m = d.shape
    d = np.where(ok, d, np.inf)
    order = np.argsort(d, axis=1, kind="stable")      # (d2, index): ties to the lowest index
    rows = np.arange(n)
    i1 = order[:, 0]
    d1 = d[rows, i1]
    i2 = order[:, 1] if m > 1 else np.zeros(n, np.intp)
    d2 = d[rows, i2] if m > 1 else np.full(n, np.inf)
    idx = np.where(np.isfinite(d1), i1, -1).astype(np.int32)
    idx2 = np.where(np.isfinite(d2), i2, -1).astype(np.int32)
    with np.errstate(all="ignore"):
        dist = np.where(idx >= 0, np.sqrt(np.where(idx >= 0, d1, 0).astype(np.float32)), np.float32(np.inf)).astype(np.float32)
        dist2 = np.where(idx2 >= 0, np.sqrt(np.where(idx2 >= 0, d2, 0).astype(np.float32)), np.float32(np.inf)).astype(np.float32)
    return idx, dist, idx2, dist2


def select(d, passes):
    """(idx, dist, idx2, dist2, count, ridx, rdist) from ``d`` (nq, nt): squared distances that float32 holds exactly, inf or
    NaN where the kernel's d2 is not finite; and ``passes`` (nq, nt) bool."""
    d = np.asarray(d, dtype=np.float64)
    d = np.where(np.isfinite(d), d, np.inf)
    idx, dist, idx2, dist2 = _side(d, passes)
    ridx, rdist, _, _ = _side(d.T, passes.T)
    return idx, dist, idx2, dist2, passes.sum(axis=1).astype(np.int32), ridx, rdist


def d2_int(q, t):
    """(nq, nt) float64 squared distances of integer-valued descriptors, exact; inf for every pair with a row that holds a
    NaN or an infinity (the kernel's float32 sum is NaN or inf there)."""
    q, t = np.asarray(q, dtype=np.float64), np.asarray(t, dtype=np.float64)
    bad_q, bad_t = ~np.isfinite(q).all(axis=1), ~np.isfinite(t).all(axis=1)
    d = MS.d2_int(np.where(bad_q[:, None], 0, q), np.where(bad_t[:, None], 0, t)).astype(np.float64)
    assert d.max(initial=0) < 2 ** 24
    d[bad_q, :] = np.inf
    d[:, bad_t] = np.inf
    return d


def match_int(q, t, rec_q, rec_t, kind, r2):
    """The whole call for integer-valued descriptors."""
    return select(d2_int(q, t), gate(rec_q, rec_t, kind, r2))


def project(H, pts):
    p = np.c_[pts, np.ones(len(pts))] @ np.asarray(H, dtype=np.float64).T
    return p[:, :2] / p[:, 2:]


def scene(seed, n_train=300, n_query=200, size=(640, 480)):
    """The look-alike scene: train keypoints that share 10 descriptor textures (train noise +-1), queries with descriptor noise
    +-12 and 0.5 px position noise under a mild projective H (train -> query).  Returns (q_pts, q_desc, t_pts, t_desc, H, perm):
    query i's partner is train row perm[i]."""
    rng = np.random.default_rng(seed)
    t_pts = (rng.random((n_train, 2)) * [size[0], size[1]]).astype(np.float32)
    tex = rng.integers(0, 256, (10, 128))
    lab = rng.integers(0, 10, n_train)
    t_desc = np.clip(tex[lab] + rng.integers(-1, 2, (n_train, 128)), 0, 255)
    perm = rng.permutation(n_train)[:n_query]
    q_pts = (project(H_SCENE, t_pts[perm]) + rng.normal(0, .5, (n_query, 2))).astype(np.float32)
    q_desc = np.clip(t_desc[perm] + rng.integers(-12, 13, (n_query, 128)), 0, 255)
    return q_pts, q_desc.astype(np.float32), t_pts, t_desc.astype(np.float32), H_SCENE.copy(), perm


def scene_records(q_pts, t_pts, H):
    """Queries as points, the train side projected into the query picture (H: train -> query): kind POINT."""
    return records(q_pts), records(t_pts, H, PROJECT)


def score(feats_cp, feats_op, qi, ti):
    """The reference's second condition (utils.py:153-160, spectral_method.py:61): the normalised descriptors' dot product."""
    c = np.asarray(feats_cp)[qi]
    o = np.asarray(feats_op)[ti]
    c = c / np.linalg.norm(c, axis=-1, keepdims=True)
    o = o / np.linalg.norm(o, axis=-1, keepdims=True)
    return np.sum(c * o, axis=-1)


def rematch(pts_c, feats_cp, pts_o, feats_op, H, em_radius, score_thresh):
    """(query indices, train indices, distances) that ``guided.rematch`` selects under H (other -> centre), integer descriptors."""
    rec_q, rec_t = records(pts_c), records(pts_o, H, PROJECT)
    r2 = np.float64(em_radius) * np.float64(em_radius)
    idx, dist = match_int(feats_cp, feats_op, rec_q, rec_t, KIND_POINT, r2)[:2]
    qi = np.flatnonzero(idx >= 0)
    keep = score(np.float32(feats_cp), np.float32(feats_op), qi, idx[qi]) > score_thresh
    return qi[keep], idx[qi][keep], dist[qi][keep]
