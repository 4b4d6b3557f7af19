"""Descriptor matching on the GPU: the front of the spectral path, without OpenCV.

The reference takes its matches from ``coarse_matching`` (utils.py:142-151): ``cv.FlannBasedMatcher().match(feats_cp,
feats_op)`` over 128-d SIFT descriptors.  FLANN's randomised kd-trees approximate one well-defined answer: for every query
descriptor, the train descriptor at the smallest L2 distance.  ``apap_match_descriptors`` computes that answer exactly
(include/apap_hip.h, DESIGN.md "Descriptor matching"), with the runner-up for a ratio test.

* ``match_descriptors``: arrays in, ``MatchResult`` out.
* ``match``: the shape of ``cv.DescriptorMatcher.match`` - one ``DMatch`` per query, in query order - with two optional
  host-side filters, ``ratio`` (Lowe's test against the runner-up) and ``cross_check`` (mutual nearest neighbours).
* ``coarse_matching``: the reference's 5-tuple ``(kpts_cp, feats_cp, kpts_op, feats_op, matches)`` from keypoint
  coordinates and descriptors; ``calculate_M``, ``match_RANSAC`` and ``model_solve`` of ``spectral_method`` take it as it is.
* ``matched_arrays``: ``(src_pts, dst_pts, c_feats, o_feats)``, what ``spectral_weights`` / ``spectral_em`` /
  ``spectral_em_batch`` take.

Descriptors are this module's input; ``cvx_proj_amd.features`` extracts them from images (SIFT at given keypoints) and hands
on to it.  ``DMatch`` and ``KeyPoint`` are the plain stand-ins for OpenCV's classes that the rest of the package duck-types.
Neither torch nor scipy is imported.  No CPU fallback.
"""
from __future__ import annotations

from typing import NamedTuple

import numpy as np

from . import _native

__all__ = ["MatchResult", "DMatch", "KeyPoint", "match_descriptors", "match", "coarse_matching", "matched_arrays"]


class MatchResult(NamedTuple):
    train_idx: np.ndarray         # (nq,) int32: the nearest train row; -1 where none can be selected
    distance: np.ndarray          # (nq,) float32: its L2 distance; +inf where none
    second_idx: np.ndarray        # (nq,) int32: the runner-up (-1 with a single train row); None when not asked for
    second_distance: np.ndarray   # (nq,) float32


class DMatch:
    """cv.DMatch's fields."""
    __slots__ = ("queryIdx", "trainIdx", "distance", "imgIdx")

    def __init__(self, queryIdx, trainIdx, distance, imgIdx=0):
        self.queryIdx, self.trainIdx, self.distance, self.imgIdx = int(queryIdx), int(trainIdx), float(distance), int(imgIdx)

    def __repr__(self):
        return f"DMatch(queryIdx={self.queryIdx}, trainIdx={self.trainIdx}, distance={self.distance!r}, imgIdx={self.imgIdx})"

    def __eq__(self, other):
        return isinstance(other, DMatch) and (self.queryIdx, self.trainIdx, self.distance, self.imgIdx) == \
            (other.queryIdx, other.trainIdx, other.distance, other.imgIdx)

    __hash__ = None


class KeyPoint:
    """cv.KeyPoint(x, y, size): ``.pt`` is the (x, y) tuple of Python floats, as OpenCV's."""
    __slots__ = ("pt", "size")

    def __init__(self, x, y, size=1):
        self.pt, self.size = (float(x), float(y)), float(size)

    def __repr__(self):
        return f"KeyPoint(x={self.pt[0]!r}, y={self.pt[1]!r}, size={self.size!r})"


def match_descriptors(feats_cp, feats_op, second=True, device=-1, ctx=None):
    """``MatchResult`` of the queries ``feats_cp`` (nq, 128) against the train set ``feats_op`` (nt, 128); uint8 or float."""
    return MatchResult(*_native.match_descriptors(feats_cp, feats_op, second=second, device=device, ctx=ctx))


def _keep(forward, backward, ratio, cross_check):
    """The queries that pass the filters: forward / backward are MatchResults (backward: the roles swapped, or None)."""
    keep = forward.train_idx >= 0
    if ratio is not None:
        keep &= forward.distance < np.float32(ratio) * forward.second_distance
    if cross_check:
        back = backward.train_idx[np.maximum(forward.train_idx, 0)]
        keep &= back == np.arange(len(keep))
    return keep


def match(feats_cp, feats_op, *, ratio=None, cross_check=False, device=-1, ctx=None):
    """``cv.DescriptorMatcher.match(feats_cp, feats_op)``, exact: a list with one ``DMatch`` per query, in query order.
    ``ratio``: keep a match only if ``distance < ratio * second_distance`` (float32 arithmetic).  ``cross_check``: keep it
    only if the query is in turn the nearest neighbour of its train row (a second call with the roles swapped)."""
    fwd = match_descriptors(feats_cp, feats_op, second=ratio is not None, device=device, ctx=ctx)
    bwd = match_descriptors(feats_op, feats_cp, second=False, device=device, ctx=ctx) if cross_check else None
    keep = _keep(fwd, bwd, ratio, cross_check)
    return [DMatch(i, fwd.train_idx[i], fwd.distance[i]) for i in np.flatnonzero(keep)]


def coarse_matching(raw_kpts_cp, feats_cp, raw_kpts_op, feats_op, **match_kw):
    """utils.py:142-151 from the descriptors on: ``(kpts_cp, feats_cp, kpts_op, feats_op, matches)`` with the keypoints as
    ``KeyPoint(x, y, 1)``, the descriptors as float32 arrays (what SIFT returns) and ``matches = match(feats_cp, feats_op,
    **match_kw)``."""
    kpts_cp = [KeyPoint(*pt, 1) for pt in np.asarray(raw_kpts_cp).reshape(-1, 2)]
    kpts_op = [KeyPoint(*pt, 1) for pt in np.asarray(raw_kpts_op).reshape(-1, 2)]
    feats_cp, feats_op = _native.as_descriptors(feats_cp, "feats_cp"), _native.as_descriptors(feats_op, "feats_op")
    if len(kpts_cp) != len(feats_cp) or len(kpts_op) != len(feats_op):
        raise ValueError(f"coarse_matching: {len(kpts_cp)} / {len(kpts_op)} keypoints for {len(feats_cp)} / {len(feats_op)} descriptors")
    return kpts_cp, feats_cp, kpts_op, feats_op, match(feats_cp, feats_op, **match_kw)


def matched_arrays(raw_kpts_cp, feats_cp, raw_kpts_op, feats_op, **match_kw):
    """``(src_pts, dst_pts (n, 2) float32, c_feats, o_feats (n, 128) float32)`` of the matches ``match(feats_cp, feats_op,
    **match_kw)``: what ``cv_to_array`` makes of ``coarse_matching``'s tuple, gathered by index."""
    pts_c = np.asarray(raw_kpts_cp).reshape(-1, 2)
    pts_o = np.asarray(raw_kpts_op).reshape(-1, 2)
    feats_cp, feats_op = _native.as_descriptors(feats_cp, "feats_cp"), _native.as_descriptors(feats_op, "feats_op")
    if len(pts_c) != len(feats_cp) or len(pts_o) != len(feats_op):
        raise ValueError(f"matched_arrays: {len(pts_c)} / {len(pts_o)} keypoints for {len(feats_cp)} / {len(feats_op)} descriptors")
    matches = match(feats_cp, feats_op, **match_kw)
    qi = np.fromiter((m.queryIdx for m in matches), np.intp, len(matches))
    ti = np.fromiter((m.trainIdx for m in matches), np.intp, len(matches))
    return pts_c[qi].astype(np.float32), pts_o[ti].astype(np.float32), feats_cp[qi], feats_op[ti]
