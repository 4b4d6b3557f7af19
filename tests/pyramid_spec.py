"""The image pyramid's contract (include/apap_hip.h "image pyramid", DESIGN.md "Image pyramid and scale") in numpy int64: plain
array code, index arrays for reflect-101.  No float anywhere but the base-frame coordinate, one float64 division.

* ``halve`` (H), ``three_quarter`` (Q), ``layout``, ``levels``, ``base_coord``, ``level_caps``: the definition.
* ``keypoints``: the keypoint list of a picture - every level's corners (``corner_spec.detect`` trimmed to the level's cap),
  levels ascending, with the base-frame coordinates.
* ``detect_and_describe``: the composition with ``corner_spec`` and ``sift_spec`` / ``sift_orient_spec`` that
  ``features.detect_and_describe(levels=...)`` must equal byte for byte; ``match_spec`` on two of them is the chain.
"""
import numpy as np

import corner_spec

MAX_LEVELS, MIN_SIDE = 16, 32
B = np.array([1, 4, 6, 4, 1], np.int64)
QW = ((5, 1), (3, 3), (1, 5))


def reflect(i, n):
    """reflect-101 of an index array, once (enough for -2 .. n + 1 when n >= 4)."""
    i = np.where(i < 0, -i, i)
    return np.where(i > n - 1, 2 * (n - 1) - i, i)


def halve(g):
    """H(g): ((h + 1) >> 1, (w + 1) >> 1); 5 x 5 binomial taps on reflect-101 indices, (sum + 128) >> 8, one rounding."""
    g = np.asarray(g).astype(np.int64)
    h, w = g.shape
    oh, ow = (h + 1) >> 1, (w + 1) >> 1
    acc = np.zeros((oh, ow), np.int64)
    for i in range(-2, 3):
        ys = reflect(2 * np.arange(oh) + i, h)
        for j in range(-2, 3):
            xs = reflect(2 * np.arange(ow) + j, w)
            acc += B[i + 2] * B[j + 2] * g[ys[:, None], xs[None, :]]
    return ((acc + 128) >> 8).astype(np.uint8)


def _q_axis(n):
    """Per output index of an axis of n source pixels: (first source index, weight of it, weight of the next)."""
    x = np.arange((3 * n) >> 2)
    k, r = x // 3, x % 3
    src = 4 * k + r
    assert len(x) == 0 or src.max() + 1 <= n - 1
    return src, 5 - 2 * r, 1 + 2 * r


def three_quarter(g):
    """Q(g): ((3h) >> 2, (3w) >> 2); (sum of wy wx g + 18) // 36."""
    g = np.asarray(g).astype(np.int64)
    h, w = g.shape
    sy, wy0, wy1 = _q_axis(h)
    sx, wx0, wx1 = _q_axis(w)
    top = wx0[None, :] * g[sy[:, None], sx[None, :]] + wx1[None, :] * g[sy[:, None], sx[None, :] + 1]
    bot = wx0[None, :] * g[sy[:, None] + 1, sx[None, :]] + wx1[None, :] * g[sy[:, None] + 1, sx[None, :] + 1]
    return ((wy0[:, None] * top + wy1[:, None] * bot + 18) // 36).astype(np.uint8)


def chain_of(level, half_steps):
    """(odd, k) of level `level`: the 3/4 chain or the octave chain, and the number of halvings."""
    if half_steps:
        return bool(level & 1), level >> 1
    return False, level


def layout(h, w, n_levels=6, half_steps=True):
    """(heights, widths, offsets (count + 1), scale_num, scale_shift): the levels that exist, at most n_levels."""
    assert MIN_SIDE <= h and MIN_SIDE <= w and 1 <= n_levels <= MAX_LEVELS
    hs, ws, off, num, shift = [], [], [0], [], []
    for level in range(n_levels):
        odd, k = chain_of(level, half_steps)
        lh, lw = ((3 * h) >> 2, (3 * w) >> 2) if odd else (h, w)
        for _ in range(k):
            lh, lw = (lh + 1) >> 1, (lw + 1) >> 1
        if lh < MIN_SIDE or lw < MIN_SIDE:
            break
        hs.append(lh)
        ws.append(lw)
        num.append(3 if odd else 1)
        shift.append(k + 2 if odd else k)
        off.append(off[-1] + (lh * lw + 255) // 256 * 256)
    return hs, ws, off, num, shift


def levels(img, n_levels=6, half_steps=True):
    """The list of uint8 levels of a (h, w) grey or (h, w, 3) BGR picture."""
    g = corner_spec.grey(img).astype(np.uint8)
    count = len(layout(g.shape[0], g.shape[1], n_levels, half_steps)[0])
    out = []
    for level in range(count):
        odd, k = chain_of(level, half_steps)
        a = three_quarter(g) if odd else g
        for _ in range(k):
            a = halve(a)
        out.append(a)
    return out


def base_coord(x, num, shift):
    """The base-frame coordinate of integer level coordinates x, float32: x 2^k, or (2^(k + 3) x + 1) / 6 in float64."""
    x = np.asarray(x).astype(np.int64)
    if num == 1:
        return (x << shift).astype(np.float64).astype(np.float32)
    return (((x << (shift + 1)) + 1).astype(np.float64) / 6.0).astype(np.float32)


def level_caps(max_corners, n_levels=6, half_steps=True):
    caps = []
    for level in range(n_levels):
        odd, k = chain_of(level, half_steps)
        share = (9 * max_corners) >> (2 * k + 4) if odd else max_corners >> (2 * k)
        caps.append(min(max_corners, max(16, share)))
    return caps


def keypoints(img, max_corners, radius=5, quality_permille=10, n_levels=6, half_steps=True, lv=None):
    """(pts (N, 2) float32 base frame, level_pts (N, 2) float32, level (N) int32, response (N) int64, level_offset, levels)."""
    lv = levels(img, n_levels, half_steps) if lv is None else lv
    _, _, _, num, shift = layout(lv[0].shape[0], lv[0].shape[1], n_levels, half_steps)
    caps = level_caps(max_corners, n_levels, half_steps)
    pts, lpts, level, resp, off = [], [], [], [], [0]
    for m, a in enumerate(lv):
        p, r = corner_spec.detect(a, caps[m], radius, quality_permille)
        lpts.append(p)
        pts.append(np.stack([base_coord(p[:, 0], num[m], shift[m]), base_coord(p[:, 1], num[m], shift[m])], axis=1))
        level.append(np.full(len(p), m, np.int32))
        resp.append(r)
        off.append(off[-1] + len(p))
    return (np.concatenate(pts).astype(np.float32).reshape(-1, 2), np.concatenate(lpts).astype(np.float32).reshape(-1, 2),
            np.concatenate(level), np.concatenate(resp).astype(np.int64), np.array(off, np.int32), lv)


def detect_and_describe(img, max_corners, radius=5, quality_permille=10, n_levels=6, half_steps=True, describe=None):
    """(pts, feats, level, response): every level's corners described on their own level image by ``describe(level_img,
    level_pts)`` (default ``sift_spec.describe``)."""
    if describe is None:
        import sift_spec
        describe = sift_spec.describe
    pts, lpts, level, resp, off, lv = keypoints(img, max_corners, radius, quality_permille, n_levels, half_steps)
    feats = [describe(a, lpts[off[m]:off[m + 1]]) for m, a in enumerate(lv) if off[m + 1] > off[m]]
    feats = np.concatenate(feats) if feats else np.zeros((0, 128), np.float32)
    return pts, feats.astype(np.float32), level, resp
