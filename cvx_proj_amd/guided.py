"""Guided descriptor matching on the GPU: the matcher, searched only where the geometry allows.

The reference's ``recompute_matching`` (spectral_method.py:35-64) says what it wants - "SIFT descriptor not similar enough but
warped points are actually close - therefore, after computing the global Homography, we should recompute the matches and start
all over" - and then only re-masks the matches that the unguided matcher produced.  A query whose globally nearest descriptor
is the wrong one of several look-alikes never sees its partner again.  ``apap_match_guided`` (include/apap_hip.h, DESIGN.md
"Guided matching") does recompute: for every query the nearest and second-nearest train descriptor among the train keypoints
that pass a geometric gate, with ``matching``'s exact distances and tie rules.

* ``records``: the three float64 a keypoint carries into the gate - the point, the point under a 3 x 3 model, or its line.
* ``guided_match_descriptors``: arrays and records in, ``GuidedResult`` out.
* ``guided_match``: a list of ``matching.DMatch`` under a homography ``H`` (other -> centre), a fundamental matrix ``F``
  (``calculate_M``'s ``F @ homo_src_pts``) or a local-homography ``grid``; ``ratio`` and ``cross_check`` as ``matching.match``.
* ``guided_matched_arrays``: ``(src_pts, dst_pts, c_feats, o_feats)``, what ``spectral_em`` takes.
* ``rematch``: the re-matching the reference's docstring asks for, ready for ``calculate_M``.

Neither torch nor scipy nor OpenCV is imported.  No CPU fallback.  The resident forms are ``resident.hip_guided_records`` and
``resident.hip_guided_match[_batch]``.
"""
from __future__ import annotations

from typing import NamedTuple

import numpy as np

from . import _native
from .matching import DMatch, KeyPoint, MatchResult, _keep

__all__ = ["GuidedResult", "records", "guided_match_descriptors", "guided_match", "guided_matched_arrays", "rematch"]


class GuidedResult(NamedTuple):
    train_idx: np.ndarray         # (nq,) int32: the nearest train row inside the gate; -1 where none can be selected
    distance: np.ndarray          # (nq,) float32: its L2 distance; +inf where none
    second_idx: np.ndarray        # (nq,) int32: the runner-up inside the gate; None when not asked for
    second_distance: np.ndarray   # (nq,) float32
    count: np.ndarray             # (nq,) int32: the train rows that pass the query's gate
    query_idx: np.ndarray         # (nt,) int32: for every train row the best query under the same gate; None without reverse
    query_distance: np.ndarray    # (nt,) float32


def records(pts, model=None, what="point", device=-1, ctx=None):
    """The (n, 3) float64 records of the keypoints ``pts`` (n, 2), taken as float32: ``what='point'`` (x, y, 1), ``'project'``
    the point under the 3 x 3 ``model`` (u / s, v / s, 1), ``'line'`` the line ``model @ (x, y, 1)``."""
    return _native.guided_records(pts, model, what, device=device, ctx=ctx)


def guided_match_descriptors(feats_cp, feats_op, rec_q, rec_t, kind, radius, second=True, reverse=False, device=-1, ctx=None):
    """``GuidedResult`` of the queries ``feats_cp`` (nq, 128) against the train set ``feats_op`` (nt, 128) under the gate
    ``kind`` ('point': the records closer than ``radius``; 'line': the train point closer than ``radius`` to the query's
    line), strictly: r2 = float64(radius)^2, one multiplication.  ``rec_q`` (nq, 3) and ``rec_t`` (nt, 3) come from ``records``."""
    radius = np.float64(radius)
    if not radius >= 0:
        raise ValueError(f"radius must be >= 0 (or +inf); got {radius!r}")
    return GuidedResult(*_native.match_guided(feats_cp, feats_op, rec_q, rec_t, kind, radius * radius, second=second,
                                              reverse=reverse, device=device, ctx=ctx))


def _points(kpts, name):
    """(n, 2) float32 of raw coordinates or of ``KeyPoint``-like objects (``.pt``)."""
    if len(kpts) and hasattr(kpts[0], "pt"):
        kpts = [k.pt for k in kpts]
    pts = np.asarray(kpts, dtype=np.float32).reshape(-1, 2)
    if len(pts) < 1:
        raise ValueError(f"{name}: no keypoints")
    return pts


def _gate_records(pts_c, pts_o, H, F, grid, device, ctx):
    given = [name for name, v in (("H", H), ("F", F), ("grid", grid)) if v is not None]
    if len(given) != 1:
        raise ValueError(f"guided_match: exactly one of H, F, grid must be given; got {given or 'none'}")
    if H is not None:       # other -> centre, the convention of recompute_matching
        return records(pts_c, None, "point", device, ctx), records(pts_o, H, "project", device, ctx), "point"
    if F is not None:       # the centre keypoint's epipolar line in the other image: calculate_M's F @ homo_src_pts
        return records(pts_c, F, "line", device, ctx), records(pts_o, None, "point", device, ctx), "line"
    from .evaluate import project_through_grid
    cells, mesh, offsets = grid   # centre -> other through each point's own cell, on the host
    proj = project_through_grid(np.asarray(cells), mesh, offsets, pts_c)
    return np.concatenate([proj, np.ones((len(proj), 1))], axis=1), records(pts_o, None, "point", device, ctx), "point"


def _guided(raw_kpts_cp, feats_cp, raw_kpts_op, feats_op, H, F, grid, radius, ratio, cross_check, device, ctx):
    pts_c, pts_o = _points(raw_kpts_cp, "raw_kpts_cp"), _points(raw_kpts_op, "raw_kpts_op")
    feats_cp, feats_op = _native.as_descriptors(feats_cp, "feats_cp"), _native.as_descriptors(feats_op, "feats_op")
    if len(pts_c) != len(feats_cp) or len(pts_o) != len(feats_op):
        raise ValueError(f"guided_match: {len(pts_c)} / {len(pts_o)} keypoints for {len(feats_cp)} / {len(feats_op)} descriptors")
    rec_q, rec_t, kind = _gate_records(pts_c, pts_o, H, F, grid, device, ctx)
    res = guided_match_descriptors(feats_cp, feats_op, rec_q, rec_t, kind, radius, second=ratio is not None, reverse=cross_check,
                                   device=device, ctx=ctx)
    fwd = MatchResult(res.train_idx, res.distance, res.second_idx, res.second_distance)
    bwd = MatchResult(res.query_idx, res.query_distance, None, None) if cross_check else None
    keep = _keep(fwd, bwd, ratio, cross_check)
    matches = [DMatch(i, res.train_idx[i], res.distance[i]) for i in np.flatnonzero(keep)]
    return pts_c, feats_cp, pts_o, feats_op, matches


def guided_match(raw_kpts_cp, feats_cp, raw_kpts_op, feats_op, *, H=None, F=None, grid=None, radius=6.0, ratio=None,
                 cross_check=False, device=-1, ctx=None):
    """``matching.match`` under a geometric gate of ``radius`` pixels: a list of ``DMatch``, at most one per centre keypoint, in
    query order.  Exactly one model: ``H`` (3 x 3, other -> centre: an other keypoint is a candidate when its image under H lies
    within ``radius`` of the centre keypoint), ``F`` (3 x 3: when it lies within ``radius`` of the centre keypoint's epipolar
    line ``F @ (x, y, 1)``) or ``grid=(grid, mesh, offsets)`` (per-cell centre -> other matrices, as
    ``evaluate.project_through_grid`` takes them: when it lies within ``radius`` of the centre keypoint's projection).
    ``ratio`` / ``cross_check``: ``matching.match``'s filters, over the gated candidates; the mutual check comes from the same
    call's reverse outputs."""
    return _guided(raw_kpts_cp, feats_cp, raw_kpts_op, feats_op, H, F, grid, radius, ratio, cross_check, device, ctx)[4]


def guided_matched_arrays(raw_kpts_cp, feats_cp, raw_kpts_op, feats_op, **guided_kw):
    """``(src_pts, dst_pts (n, 2) float32, c_feats, o_feats (n, 128) float32)`` of ``guided_match``'s matches: the 4-tuple that
    ``spectral_weights`` / ``spectral_em`` take, as ``matching.matched_arrays`` makes it."""
    kw = dict(H=None, F=None, grid=None, radius=6.0, ratio=None, cross_check=False, device=-1, ctx=None)
    unknown = set(guided_kw) - set(kw)
    if unknown:
        raise TypeError(f"guided_matched_arrays: unexpected arguments {sorted(unknown)}")
    kw.update(guided_kw)
    pts_c, feats_cp, pts_o, feats_op, matches = _guided(raw_kpts_cp, feats_cp, raw_kpts_op, feats_op, **kw)
    qi = np.fromiter((m.queryIdx for m in matches), np.intp, len(matches))
    ti = np.fromiter((m.trainIdx for m in matches), np.intp, len(matches))
    return pts_c[qi], pts_o[ti], feats_cp[qi], feats_op[ti]


def rematch(kpts_cp, feats_cp, kpts_op, feats_op, H, opts, device=-1, ctx=None):
    """What ``recompute_matching``'s docstring asks for: the matches recomputed under the global homography ``H`` (other ->
    centre).  For every centre keypoint the nearest descriptor among the other keypoints that H maps within ``opts.em_radius``
    of it; of those matches the ones whose normalised descriptors' dot product exceeds ``opts.score_thresh`` (the reference's
    second condition, on the host via ``spectral_method.normalized_feature``).  Every match returned is one that the
    reference's ``recompute_matching`` keeps.  Returns ``(kpts_cp, feats_cp, kpts_op, feats_op, matches)`` with the keypoints as
    ``KeyPoint`` and the descriptors as float32 arrays: what ``calculate_M`` takes."""
    from .spectral_method import normalized_feature
    pts_c, feats_cp, pts_o, feats_op, matches = _guided(kpts_cp, feats_cp, kpts_op, feats_op, H, None, None,
                                                        getattr(opts, "em_radius", 6.0), None, False, device, ctx)
    thresh = getattr(opts, "score_thresh", 0.4)
    kept = []
    for m in matches:
        feat_c, feat_o = normalized_feature(feats_cp, feats_op, m)
        if np.sum(feat_c * feat_o) > thresh:
            kept.append(m)
    as_kp = lambda ks, pts: list(ks) if len(ks) and hasattr(ks[0], "pt") else [KeyPoint(*p, 1) for p in pts]      # noqa: E731
    return as_kp(kpts_cp, pts_c), feats_cp, as_kp(kpts_op, pts_o), feats_op, kept
