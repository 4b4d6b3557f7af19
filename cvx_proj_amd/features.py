"""SIFT descriptors at given keypoints on the GPU: from an image pair and keypoint coordinates to matches, without OpenCV.

The reference's ``coarse_matching`` (utils.py:142-151) starts from two images and the keypoint coordinates of
``keypoints.mat``: ``cv.SIFT.create(nfeatures=128).compute(img, [cv.KeyPoint(x, y, 1) ...])`` on each, then the matcher.
``apap_sift_describe`` computes those descriptors - OpenCV 4.x's definition for ``KeyPoint(x, y, 1)``, restated in DESIGN.md
"Descriptor extraction"; parity with OpenCV itself is not pinned, OpenCV being absent - and ``matching`` does the rest.

* ``compute``: ``(kpts, feats)`` like ``extractor.compute(img, kpts)``; ``angles`` describes at given or found orientations.
* ``orient``: the keypoints' dominant orientations.  ``oriented=True`` on the functions below describes every keypoint in its
  own orientation (DESIGN.md "Keypoint orientation"): matches then survive an in-plane rotation between the two pictures.
* ``coarse_matching``: the reference's own signature and 5-tuple ``(kpts_cp, feats_cp, kpts_op, feats_op, matches)``; both
  images are described in one batched call.
* ``matched_arrays``: ``(src_pts, dst_pts, c_feats, o_feats)``, what ``spectral_weights`` / ``spectral_em`` take.

The keypoint coordinates need not come from outside: ``apap_corner_detect`` finds exact integer Harris corners (DESIGN.md
"Corner detection"), which is all the descriptor can use - it rounds its coordinates and reads the base level only.

* ``detect`` / ``detect_pair``: (n, 2) float32 corners, directly usable as ``raw_kpts``; the pair in one batched call.
* ``detect_and_match``: ``coarse_matching``'s 5-tuple from the two images alone.
* ``matched_arrays_from_images``: ``matched_arrays`` from the two images alone.

Images are uint8, (h, w) grey or (h, w, 3) BGR (what ``cv.imread`` returns).  Neither torch nor scipy nor cv2 is imported.
No CPU fallback.
"""
from __future__ import annotations

import numpy as np

from . import _native, matching
from .matching import KeyPoint

# the descriptor stage's names, which tests/test_sift_host.py pins; the detection functions below are public all the same
__all__ = ["compute", "describe_pair", "coarse_matching", "matched_arrays"]


def _points(raw_kpts):
    return np.asarray(raw_kpts).reshape(-1, 2)


def orient(img, raw_kpts, device=-1, ctx=None):
    """The dominant orientation of every keypoint: float32 (n,) angles in [0, 360), what ``cv.KeyPoint.angle`` would hold
    (DESIGN.md "Keypoint orientation").  A keypoint with no valid sample, or on a flat patch, has angle 0."""
    return _native.sift_orient(img, _points(raw_kpts), device=device, ctx=ctx)


def compute(img, raw_kpts, device=-1, ctx=None, angles=None):
    """``cv.SIFT.create().compute(img, [cv.KeyPoint(x, y, 1) for x, y in raw_kpts])``: the keypoints as ``KeyPoint(x, y, 1)``
    and their float32 (n, 128) descriptors.  Every keypoint keeps its row: one with no valid sample has a zero descriptor.
    ``angles``: ``None`` is that call (OpenCV's default angle); an array (n,) of angles in [0, 360] describes
    ``KeyPoint(x, y, 1, angle)``; ``"auto"`` finds every keypoint's orientation first (``orient``) in the same pass."""
    pts = _points(raw_kpts)
    if angles is None:
        feats = _native.sift_describe(img, pts, device=device, ctx=ctx)
    elif isinstance(angles, str):
        if angles != "auto":
            raise ValueError(f"compute: angles must be None, \"auto\" or an array; got {angles!r}")
        feats, _ = _native.sift_describe_oriented(img, pts, device=device, ctx=ctx)
    else:
        feats = _native.sift_describe_oriented(img, pts, angles, device=device, ctx=ctx)
    return [KeyPoint(*pt, 1) for pt in pts], feats


def describe_pair(c_img, o_img, raw_kpts_cp, raw_kpts_op, device=-1, ctx=None, oriented=False):
    """The descriptors of both images in one batched call: (feats_cp, feats_op), float32 (n, 128) each.  ``oriented``: every
    keypoint in its own dominant orientation, so that matching survives an in-plane rotation between the images."""
    pts_c, pts_o = _points(raw_kpts_cp), _points(raw_kpts_op)
    both, counts = np.concatenate([pts_c, pts_o]).astype(np.float32), [len(pts_c), len(pts_o)]
    if oriented:
        feats, _ = _native.sift_describe_oriented_batch([c_img, o_img], both, counts, device=device, ctx=ctx)
    else:
        feats = _native.sift_describe_batch([c_img, o_img], both, counts, device=device, ctx=ctx)
    return feats[:len(pts_c)], feats[len(pts_c):]


def coarse_matching(c_img, o_img, raw_kpts_cp, raw_kpts_op, device=-1, ctx=None, oriented=False, **match_kw):
    """utils.py:142-151: ``(kpts_cp, feats_cp, kpts_op, feats_op, matches)`` from the two images and their keypoint
    coordinates; ``matches = matching.match(feats_cp, feats_op, **match_kw)`` (``ratio``, ``cross_check``)."""
    feats_cp, feats_op = describe_pair(c_img, o_img, raw_kpts_cp, raw_kpts_op, device=device, ctx=ctx, oriented=oriented)
    return matching.coarse_matching(raw_kpts_cp, feats_cp, raw_kpts_op, feats_op, device=device, ctx=ctx, **match_kw)


def matched_arrays(c_img, o_img, raw_kpts_cp, raw_kpts_op, device=-1, ctx=None, oriented=False, **match_kw):
    """``(src_pts, dst_pts (n, 2) float32, c_feats, o_feats (n, 128) float32)`` of the matches of the two images' descriptors:
    the arrays ``spectral_em`` takes."""
    feats_cp, feats_op = describe_pair(c_img, o_img, raw_kpts_cp, raw_kpts_op, device=device, ctx=ctx, oriented=oriented)
    return matching.matched_arrays(raw_kpts_cp, feats_cp, raw_kpts_op, feats_op, device=device, ctx=ctx, **match_kw)


def _permille(quality):
    return int(round(1000 * float(quality)))


def detect(img, max_corners=2000, radius=5, quality=0.01, device=-1, ctx=None):
    """The image's corners as (n, 2) float32 (x, y), integer-valued, strongest first: ``raw_kpts`` for ``compute`` and
    ``coarse_matching``.  A corner is the strict maximum of the integer Harris response over its (2 radius + 1)^2 window and
    reaches ``quality`` (rounded to a permille) of the strongest corner's response; at most ``max_corners`` are returned.  An
    image without corners gives a (0, 2) array."""
    return _native.corner_detect(img, max_corners, radius, _permille(quality), device=device, ctx=ctx)[0]


def detect_pair(c_img, o_img, max_corners=2000, radius=5, quality=0.01, device=-1, ctx=None):
    """The corners of both images in one batched call: (kpts_cp, kpts_op), each as ``detect`` returns it."""
    (pc, _), (po, _) = _native.corner_detect_batch([c_img, o_img], max_corners, radius, _permille(quality), device=device, ctx=ctx)
    return pc, po


def detect_and_match(c_img, o_img, max_corners=2000, radius=5, quality=0.01, device=-1, ctx=None, oriented=False, **match_kw):
    """``coarse_matching``'s 5-tuple ``(kpts_cp, feats_cp, kpts_op, feats_op, matches)`` from the two images alone: their
    corners (``detect_pair``), the descriptors there, the matches."""
    pc, po = detect_pair(c_img, o_img, max_corners, radius, quality, device=device, ctx=ctx)
    return coarse_matching(c_img, o_img, pc, po, device=device, ctx=ctx, oriented=oriented, **match_kw)


def matched_arrays_from_images(c_img, o_img, max_corners=2000, radius=5, quality=0.01, device=-1, ctx=None, oriented=False,
                               **match_kw):
    """``matched_arrays``'s ``(src_pts, dst_pts, c_feats, o_feats)`` from the two images alone: what ``spectral_em`` takes."""
    pc, po = detect_pair(c_img, o_img, max_corners, radius, quality, device=device, ctx=ctx)
    return matched_arrays(c_img, o_img, pc, po, device=device, ctx=ctx, oriented=oriented, **match_kw)
