"""SIFT descriptors at given keypoints on the GPU: from an image pair and keypoint coordinates to matches, without OpenCV.

The reference's ``coarse_matching`` (utils.py:142-151) starts from two images and the keypoint coordinates of
``keypoints.mat``: ``cv.SIFT.create(nfeatures=128).compute(img, [cv.KeyPoint(x, y, 1) ...])`` on each, then the matcher.
``apap_sift_describe`` computes those descriptors - OpenCV 4.x's definition for ``KeyPoint(x, y, 1)``, restated in DESIGN.md
"Descriptor extraction"; parity with OpenCV itself is not pinned, OpenCV being absent - and ``matching`` does the rest.

* ``compute``: ``(kpts, feats)`` like ``extractor.compute(img, kpts)``.
* ``coarse_matching``: the reference's own signature and 5-tuple ``(kpts_cp, feats_cp, kpts_op, feats_op, matches)``; both
  images are described in one batched call.
* ``matched_arrays``: ``(src_pts, dst_pts, c_feats, o_feats)``, what ``spectral_weights`` / ``spectral_em`` take.

Images are uint8, (h, w) grey or (h, w, 3) BGR (what ``cv.imread`` returns).  Neither torch nor scipy nor cv2 is imported.
No CPU fallback.
"""
from __future__ import annotations

import numpy as np

from . import _native, matching
from .matching import KeyPoint

__all__ = ["compute", "describe_pair", "coarse_matching", "matched_arrays"]


def _points(raw_kpts):
    return np.asarray(raw_kpts).reshape(-1, 2)


def compute(img, raw_kpts, device=-1, ctx=None):
    """``cv.SIFT.create().compute(img, [cv.KeyPoint(x, y, 1) for x, y in raw_kpts])``: the keypoints as ``KeyPoint(x, y, 1)``
    and their float32 (n, 128) descriptors.  Every keypoint keeps its row: one with no valid sample has a zero descriptor."""
    pts = _points(raw_kpts)
    feats = _native.sift_describe(img, pts, device=device, ctx=ctx)
    return [KeyPoint(*pt, 1) for pt in pts], feats


def describe_pair(c_img, o_img, raw_kpts_cp, raw_kpts_op, device=-1, ctx=None):
    """The descriptors of both images in one batched call: (feats_cp, feats_op), float32 (n, 128) each."""
    pts_c, pts_o = _points(raw_kpts_cp), _points(raw_kpts_op)
    feats = _native.sift_describe_batch([c_img, o_img], np.concatenate([pts_c, pts_o]).astype(np.float32), [len(pts_c), len(pts_o)],
                                        device=device, ctx=ctx)
    return feats[:len(pts_c)], feats[len(pts_c):]


def coarse_matching(c_img, o_img, raw_kpts_cp, raw_kpts_op, device=-1, ctx=None, **match_kw):
    """utils.py:142-151: ``(kpts_cp, feats_cp, kpts_op, feats_op, matches)`` from the two images and their keypoint
    coordinates; ``matches = matching.match(feats_cp, feats_op, **match_kw)`` (``ratio``, ``cross_check``)."""
    feats_cp, feats_op = describe_pair(c_img, o_img, raw_kpts_cp, raw_kpts_op, device=device, ctx=ctx)
    return matching.coarse_matching(raw_kpts_cp, feats_cp, raw_kpts_op, feats_op, device=device, ctx=ctx, **match_kw)


def matched_arrays(c_img, o_img, raw_kpts_cp, raw_kpts_op, device=-1, ctx=None, **match_kw):
    """``(src_pts, dst_pts (n, 2) float32, c_feats, o_feats (n, 128) float32)`` of the matches of the two images' descriptors:
    the arrays ``spectral_em`` takes."""
    feats_cp, feats_op = describe_pair(c_img, o_img, raw_kpts_cp, raw_kpts_op, device=device, ctx=ctx)
    return matching.matched_arrays(raw_kpts_cp, feats_cp, raw_kpts_op, feats_op, device=device, ctx=ctx, **match_kw)
