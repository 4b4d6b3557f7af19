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
* ``pyramid``, ``detect_and_describe`` and ``levels=`` on the four functions above: corners and descriptors over the levels of
  an image pyramid (DESIGN.md "Image pyramid and scale"), so that matches survive a change of scale between the pictures.

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


def _levels(levels, who):
    return _native.pyramid_levels_arg(levels, who)


def pyramid(img, levels=6, half_steps=True, device=-1, ctx=None):
    """The grey pyramid of a picture as a list of uint8 arrays (DESIGN.md "Image pyramid and scale"): level 0 the grey picture,
    even levels halved k times (a 5 x 5 binomial filter, every second pixel), odd levels the 3/4 reduction halved k times;
    ``half_steps=False`` keeps the halvings only.  Fewer than ``levels`` where the next one would have a side under 32."""
    return _native.pyramid(img, _levels(levels, "pyramid"), half_steps, device=device, ctx=ctx)


def _pyramid_keypoints(imgs, max_corners, radius, quality, levels, half_steps, device, ctx):
    """Per picture ``(level_images, pts, level_pts, level, response, level_offset)``: the pyramids of all pictures in one call,
    one batched detection over all their level images, the pack."""
    levels = _levels(levels, "detect")
    max_corners, radius, permille = _native.corner_params(max_corners, radius, _permille(quality), "detect")
    pyrs = _native.pyramid_batch(imgs, levels, half_steps, device=device, ctx=ctx)
    flat = [a for lv in pyrs for a in lv]
    slab_pts, slab_resp, count = _native.corner_detect_batch(flat, max_corners, radius, permille, device=device, ctx=ctx, full=True)
    caps = _native.pyramid_level_caps(max_corners, levels, half_steps)
    num, shift, index = [], [], []
    for lv in pyrs:
        _, _, _, n, s = _native.pyramid_layout(lv[0].shape[0], lv[0].shape[1], levels, half_steps)
        num += n.tolist()
        shift += s.tolist()
        index += range(len(lv))
    keep = np.minimum(count, caps[index])
    pts, lpts, level, resp, off = _native.pyramid_keypoints(slab_pts, slab_resp, keep, num, shift, index, device=device, ctx=ctx)
    out, m0 = [], 0
    for lv in pyrs:
        a, b = off[m0], off[m0 + len(lv)]
        out.append((lv, pts[a:b], lpts[a:b], level[a:b], resp[a:b], off[m0:m0 + len(lv) + 1] - a))
        m0 += len(lv)
    return out


def _describe_levels(found, oriented, device, ctx):
    """The descriptors of every picture's keypoints, each on its own level image, in one batched call: a list of (n, 128)."""
    imgs, lengths, lpts = [], [], []
    for lv, _, level_pts, _, _, off in found:
        for m, a in enumerate(lv):
            if off[m + 1] > off[m]:     # the batch takes no image without a keypoint
                imgs.append(a)
                lengths.append(int(off[m + 1] - off[m]))
        lpts.append(level_pts)
    lpts = np.concatenate(lpts).astype(np.float32)
    if not len(lpts):
        return [np.zeros((0, _native.SIFT_DIM), np.float32) for _ in found]
    if oriented:
        feats, _ = _native.sift_describe_oriented_batch(imgs, lpts, lengths, device=device, ctx=ctx)
    else:
        feats = _native.sift_describe_batch(imgs, lpts, lengths, device=device, ctx=ctx)
    ends = np.cumsum([len(f[1]) for f in found])
    return [feats[e - len(f[1]):e] for e, f in zip(ends, found)]


def detect_and_describe(img, max_corners=2000, radius=5, quality=0.01, device=-1, ctx=None, levels=6, half_steps=True, oriented=False):
    """``(pts, feats, level, response)`` of one picture over its pyramid: float32 (n, 2) keypoints in the picture's own frame,
    their float32 (n, 128) descriptors, each taken on the keypoint's level image (the descriptor of the picture at scale
    1 / s_level), int32 (n,) level numbers and int64 (n,) Harris responses; levels ascending, strongest first within a
    level.  Level l holds at most its share of ``max_corners`` (a constant number per unit area, at least 16).
    ``levels=None``: the single-scale ``detect`` + ``compute``."""
    if levels is None:
        pts, resp = _native.corner_detect(img, max_corners, radius, _permille(quality), device=device, ctx=ctx)
        if not len(pts):
            return pts, np.zeros((0, _native.SIFT_DIM), np.float32), np.zeros(0, np.int32), resp
        feats = compute(img, pts, device=device, ctx=ctx, angles="auto" if oriented else None)[1]
        return pts, feats, np.zeros(len(pts), np.int32), resp
    found = _pyramid_keypoints([img], max_corners, radius, quality, levels, half_steps, device, ctx)
    _, pts, _, level, resp, _ = found[0]
    return pts, _describe_levels(found, oriented, device, ctx)[0], level, resp


def _pair_over_levels(c_img, o_img, max_corners, radius, quality, levels, half_steps, oriented, device, ctx):
    """(kpts_cp, feats_cp, kpts_op, feats_op) over the pyramids of both pictures: base-frame keypoints and their descriptors."""
    found = _pyramid_keypoints([c_img, o_img], max_corners, radius, quality, levels, half_steps, device, ctx)
    feats_cp, feats_op = _describe_levels(found, oriented, device, ctx)
    return found[0][1], feats_cp, found[1][1], feats_op


def detect(img, max_corners=2000, radius=5, quality=0.01, device=-1, ctx=None, levels=None, half_steps=True):
    """The image's corners as (n, 2) float32 (x, y), integer-valued, strongest first: ``raw_kpts`` for ``compute`` and
    ``coarse_matching``.  A corner is the strict maximum of the integer Harris response over its (2 radius + 1)^2 window and
    reaches ``quality`` (rounded to a permille) of the strongest corner's response; at most ``max_corners`` are returned.  An
    image without corners gives a (0, 2) array.  ``levels``: the corners of every level of the picture's pyramid instead, in
    the picture's own frame (no longer integer-valued), levels ascending - ``detect_and_describe`` also returns the levels."""
    if levels is not None:
        return _pyramid_keypoints([img], max_corners, radius, quality, levels, half_steps, device, ctx)[0][1]
    return _native.corner_detect(img, max_corners, radius, _permille(quality), device=device, ctx=ctx)[0]


def detect_pair(c_img, o_img, max_corners=2000, radius=5, quality=0.01, device=-1, ctx=None, levels=None, half_steps=True):
    """The corners of both images in one batched call: (kpts_cp, kpts_op), each as ``detect`` returns it."""
    if levels is not None:
        found = _pyramid_keypoints([c_img, o_img], max_corners, radius, quality, levels, half_steps, device, ctx)
        return found[0][1], found[1][1]
    (pc, _), (po, _) = _native.corner_detect_batch([c_img, o_img], max_corners, radius, _permille(quality), device=device, ctx=ctx)
    return pc, po


def detect_and_match(c_img, o_img, max_corners=2000, radius=5, quality=0.01, device=-1, ctx=None, oriented=False, levels=None,
                     half_steps=True, **match_kw):
    """``coarse_matching``'s 5-tuple ``(kpts_cp, feats_cp, kpts_op, feats_op, matches)`` from the two images alone: their
    corners (``detect_pair``), the descriptors there, the matches.  ``levels``: over the pyramids of both pictures, so that
    the matches survive a change of scale between them: both pyramids in one call, one batched detection over all level
    images, every keypoint described on its own level, then the same matcher on the unions.  The keypoints are in the
    pictures' own frames: ``find_homography``, ``estimate_fundamental`` and ``spectral_em`` take the result unchanged."""
    if levels is not None:
        pc, fc, po, fo = _pair_over_levels(c_img, o_img, max_corners, radius, quality, levels, half_steps, oriented, device, ctx)
        return matching.coarse_matching(pc, fc, po, fo, device=device, ctx=ctx, **match_kw)
    pc, po = detect_pair(c_img, o_img, max_corners, radius, quality, device=device, ctx=ctx)
    return coarse_matching(c_img, o_img, pc, po, device=device, ctx=ctx, oriented=oriented, **match_kw)


def matched_arrays_from_images(c_img, o_img, max_corners=2000, radius=5, quality=0.01, device=-1, ctx=None, oriented=False,
                               levels=None, half_steps=True, **match_kw):
    """``matched_arrays``'s ``(src_pts, dst_pts, c_feats, o_feats)`` from the two images alone: what ``spectral_em`` takes.
    ``levels``: over the pyramids of both pictures, as ``detect_and_match``."""
    if levels is not None:
        pc, fc, po, fo = _pair_over_levels(c_img, o_img, max_corners, radius, quality, levels, half_steps, oriented, device, ctx)
        return matching.matched_arrays(pc, fc, po, fo, device=device, ctx=ctx, **match_kw)
    pc, po = detect_pair(c_img, o_img, max_corners, radius, quality, device=device, ctx=ctx)
    return matched_arrays(c_img, o_img, pc, po, device=device, ctx=ctx, oriented=oriented, **match_kw)
