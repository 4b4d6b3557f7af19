"""Bilinear sampling of the local warp in numpy (DESIGN.md "Bilinear sampling"): int64 / float64, nothing fused.

The functions take the float64 source coordinates of a canvas, ``tx, ty`` of shape (fh, fw) - the oracle's
``warp_coords_fast`` or the engine's ``_native.warp_coords`` - and a source picture (h, w, 3) uint8, the way
``panorama_ramp_spec`` does.

1. presence   a pixel is present iff ``tx > 0 and ty > 0 and int(tx) < w and int(ty) < h``: the truncating warp's test; an
              absent pixel is 0.
2. fixed      ``X = rint(32 tx)`` (the product is exact, rint rounds half to even), ``sx = X >> 5``, ``ax = X & 31``; Y alike.
3. taps       columns ``min(sx, w - 1)``, ``min(sx + 1, w - 1)``, rows ``min(sy, h - 1)``, ``min(sy + 1, h - 1)``: the border
              is replicated.  No lower clamp: X, Y >= 0 for a present pixel.
4. blend      ``((32 - ax)(32 - ay) p00 + ax (32 - ay) p01 + (32 - ax) ay p10 + ax ay p11 + 512) >> 10`` per channel.
"""
import numpy as np

import panorama_ramp_spec as R
from panorama_spec import panorama_size

BITS, ONE = 5, 32


def present(tx, ty, w, h):
    """Step 1.  NaN fails ``t > 0``; the truncation is taken where t > 0 only (elsewhere the answer is already False)."""
    with np.errstate(invalid="ignore"):
        pos = (tx > 0) & (ty > 0)
    ix = np.where(pos, np.minimum(np.where(pos, tx, 0), 2.0 ** 62), 0).astype(np.int64)
    iy = np.where(pos, np.minimum(np.where(pos, ty, 0), 2.0 ** 62), 0).astype(np.int64)
    return pos & (ix < w) & (iy < h)


def fixed(t, ok):
    """Step 2: X (int64) where ``ok``, 0 elsewhere."""
    return np.rint(32.0 * np.where(ok, t, 0.0)).astype(np.int64)


def taps(X, n):
    """Step 3 on one axis of length n: (first tap, second tap, weight of the second)."""
    s = X >> BITS
    return np.minimum(s, n - 1), np.minimum(s + 1, n - 1), X & (ONE - 1)


def blend(p00, p01, p10, p11, ax, ay):
    """Step 4 on int64 arrays (..., 3); ax, ay (...)."""
    ax, ay = ax[..., None], ay[..., None]
    return ((ONE - ax) * (ONE - ay) * p00 + ax * (ONE - ay) * p01 + (ONE - ax) * ay * p10 + ax * ay * p11 + 512) >> 10


def sample(src, tx, ty):
    """The bilinear warp of ``src`` over the coordinates: (fh, fw, 3) uint8."""
    src = np.asarray(src)
    assert src.dtype == np.uint8 and src.ndim == 3 and src.shape[2] == 3
    h, w = src.shape[:2]
    ok = present(tx, ty, w, h)
    x0, x1, ax = taps(fixed(tx, ok), w)
    y0, y1, ay = taps(fixed(ty, ok), h)
    s = src.astype(np.int64)
    out = blend(s[y0, x0], s[y0, x1], s[y1, x0], s[y1, x1], ax, ay)
    return np.where(ok[..., None], out, 0).astype(np.uint8)


def truncate(src, tx, ty):
    """The truncating warp over the same coordinates (apap.py:211-215): source pixel (int(tx), int(ty)) where present."""
    src = np.asarray(src)
    h, w = src.shape[:2]
    ok = present(tx, ty, w, h)
    ix = np.where(ok, tx, 0).astype(np.int64)
    iy = np.where(ok, ty, 0).astype(np.int64)
    return np.where(ok[..., None], src[iy, ix], 0).astype(np.uint8)


def stitch(warped, center, offset):
    """``local_stitch``'s downstream stage on a warped canvas: the centre pasted at the offsets on a black canvas, then
    ``uniform_blend`` (apap_utils.py:75-88): both present (any channel non-zero) -> floor((a + b) / 2), else a + b."""
    ox, oy = offset
    pasted = np.zeros_like(warped)
    pasted[oy:oy + center.shape[0], ox:ox + center.shape[1]] = center
    a, b = warped.astype(np.int64), pasted.astype(np.int64)
    both = warped.any(axis=-1, keepdims=True) & pasted.any(axis=-1, keepdims=True)
    return np.where(both, (a + b) >> 1, a + b).astype(np.uint8)


def compose_ramp(center, layers, geometries, coords, ramp):
    """``panorama_ramp_spec.compose_ramp`` with every layer's sample taken bilinearly; its weight is still that of the source
    pixel (int(tx), int(ty)).  Returns the canvas."""
    W, H, OX, OY = panorama_size(center.shape, geometries)
    total = np.zeros((H, W, 3), np.int64)
    wsum = np.zeros((H, W), np.int64)

    def add(rows, cols, values, weights):
        wt = np.where(values.any(axis=-1), weights, 0)
        total[rows, cols] += wt[..., None] * values.astype(np.int64)
        wsum[rows, cols] += wt

    ch, cw = center.shape[:2]
    add(slice(OY, OY + ch), slice(OX, OX + cw), center, R.weight_map(ch, cw, ramp))
    for layer, (fw, fh, ox, oy), (tx, ty) in zip(layers, geometries, coords):
        img = np.asarray(layer.img)
        _, ix, iy = R.gathered(img, tx, ty)
        add(slice(OY - oy, OY - oy + fh), slice(OX - ox, OX - ox + fw), sample(img, tx, ty), R.weight_map(*img.shape[:2], ramp)[iy, ix])
    return (total // np.maximum(wsum, 1)[..., None]).astype(np.uint8)
