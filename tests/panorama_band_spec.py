"""The panorama's two-band blend in numpy (DESIGN.md "Panorama, two-band blend"): exact integers.

Canvas, layer geometry, coordinates, the strict bounds test, truncation, presence and sampling are the panorama's
(``panorama_spec``, ``panorama_ramp_spec``, ``warp_bilinear_spec``); the gain is the gain spec's ``apply``.  View 0 is the
centre, view k layer k - 1.  Like ``panorama_ramp_spec`` the composition starts from the target coordinates of every pair
canvas - the oracle's ``warp_coords_fast`` or the engine's ``_native.warp_coords``.

1. low-pass    of an (h, w, 3) uint8 picture I with radius r = ``band``, 0 .. 32, n = 2 r + 1:
               ``T[y, x, c]`` = the sum of ``I[clamp(y + dy, 0, h - 1), clamp(x + dx, 0, w - 1), c]`` over |dx|, |dy| <= r (the
               border is replicated); ``B = (T + (n^2 >> 1)) // n^2``; r = 0 gives B = I.  The blur lives in SOURCE space.
2. per view    ``c_v``: the panorama's sample of I_v (nearest: pixel (ix, iy); bilinear: the fixed-point blend of four taps);
               ``b_v``: the sample of B_v at the same place (the same pixel; the same taps and weights);
               ``D_v = min(x + 1, w - x, y + 1, h - y)`` of the source pixel (x, y) = (ix, iy), for the centre (X - OX, Y - OY);
               ``w_v = min(D_v, ramp)``.  v is present iff any byte of ``c_v`` is non-zero.
3. gains       ``c'_v = gain(c_v, q_v)``, ``b'_v = gain(b_v, q_v)`` with ``min(255, (c q + 2048) >> 12)``; none: c' = c, b' = b.
4. blend       ``L = floor(sum w_v b'_v / sum w_v)`` per channel over the present views; ``s`` = the present view with the
               largest ``D_v``, the lowest index on ties; ``out = clip(L + c'_s - b'_s, 0, 255)``; (0, 0, 0) where no view
               is present.
"""
from typing import NamedTuple

import numpy as np

import panorama_gain_spec as G
import panorama_ramp_spec as R
import warp_bilinear_spec as B
from panorama_spec import panorama_size

MAX_BAND = 32
UNCAPPED = 1 << 14          # D < 2^14 for every picture below 2 GiB: weight_map(h, w, UNCAPPED) is D itself


def box_blur(img, r):
    """Step 1: (h, w, 3) uint8."""
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.ndim == 3 and img.shape[2] == 3
    if not (isinstance(r, (int, np.integer)) and not isinstance(r, bool) and 0 <= r <= MAX_BAND):
        raise ValueError("band 0 .. 32")
    if r == 0:
        return img.copy()
    h, w = img.shape[:2]
    n = 2 * r + 1
    ys, xs = np.clip(np.arange(-r, h + r), 0, h - 1), np.clip(np.arange(-r, w + r), 0, w - 1)
    padded = img[ys][:, xs].astype(np.int64)
    c = np.zeros((h + 2 * r + 1, w + 2 * r + 1, 3), np.int64)       # c[y, x] = the sum of padded[:y, :x]
    c[1:, 1:] = padded.cumsum(axis=0).cumsum(axis=1)
    T = c[n:, n:] - c[:-n, n:] - c[n:, :-n] + c[:-n, :-n]
    assert T.shape == img.shape and T.max() <= 255 * n * n
    return ((T + (n * n >> 1)) // (n * n)).astype(np.uint8)


def box_blur_brute(img, r):
    """Step 1 as the double loop it is written as; for tiny pictures."""
    img = np.asarray(img)
    h, w = img.shape[:2]
    n2 = (2 * r + 1) ** 2
    out = np.zeros_like(img)
    for y in range(h):
        for x in range(w):
            T = np.zeros(3, np.int64)
            for dy in range(-r, r + 1):
                for dx in range(-r, r + 1):
                    T += img[min(max(y + dy, 0), h - 1), min(max(x + dx, 0), w - 1)]
            out[y, x] = (T + (n2 >> 1)) // n2
    return out


def views(center, layers, geometries, coords, band, sampling="nearest"):
    """Step 2 on the union canvas: ``c``, ``b`` (K + 1, H, W, 3) uint8 and ``D`` (K + 1, H, W) int64; all 0 where a view has
    no sample (D: any value where the sample is black)."""
    W, H, OX, OY = panorama_size(center.shape, geometries)
    c = np.zeros((len(layers) + 1, H, W, 3), np.uint8)
    b = np.zeros_like(c)
    D = np.zeros(c.shape[:3], np.int64)
    ch, cw = center.shape[:2]
    rows, cols = slice(OY, OY + ch), slice(OX, OX + cw)
    c[0, rows, cols], b[0, rows, cols], D[0, rows, cols] = center, box_blur(center, band), R.weight_map(ch, cw, UNCAPPED)
    blurred = {}                    # layers may share a picture
    for k, (layer, (fw, fh, ox, oy), (tx, ty)) in enumerate(zip(layers, geometries, coords)):
        img = np.asarray(layer.img)
        if id(layer.img) not in blurred:
            blurred[id(layer.img)] = box_blur(img, band)
        low = blurred[id(layer.img)]
        assert tx.shape == ty.shape == (fh, fw)
        inside, ix, iy = R.gathered(img, tx, ty)
        rows, cols = slice(OY - oy, OY - oy + fh), slice(OX - ox, OX - ox + fw)
        if sampling == "bilinear":
            c[k + 1, rows, cols], b[k + 1, rows, cols] = B.sample(img, tx, ty), B.sample(low, tx, ty)
        else:
            assert sampling == "nearest"
            c[k + 1, rows, cols] = np.where(inside[..., None], img[iy, ix], 0)
            b[k + 1, rows, cols] = np.where(inside[..., None], low[iy, ix], 0)
        D[k + 1, rows, cols] = np.where(inside, R.weight_map(*img.shape[:2], UNCAPPED)[iy, ix], 0)
    return c, b, D


class Band(NamedTuple):
    canvas: object      # (H, W, 3) uint8
    raw: object         # (H, W, 3) int64: L + c'_s - b'_s before the clip
    wsum: object        # (H, W) int64: the sum of the present views' weights
    total: object       # (H, W, 3) int64: the sums of weight x low band
    count: object       # (H, W) int64: the present views
    best: object        # (H, W) int64: D_s, 0 where no view is present
    source: object      # (H, W) int64: s, -1 where no view is present
    tied: object        # (H, W) int64: the present views whose D equals D_s


def blend(c, b, D, ramp, q=None):
    """Steps 3 and 4 on the views of ``views``."""
    if not (isinstance(ramp, (int, np.integer)) and 1 <= ramp <= R.MAX_RAMP):
        raise ValueError("ramp 1 .. 256")
    V, H, W = D.shape
    total, wsum, count = np.zeros((H, W, 3), np.int64), np.zeros((H, W), np.int64), np.zeros((H, W), np.int64)
    best, source, detail = np.zeros((H, W), np.int64), np.full((H, W), -1, np.int64), np.zeros((H, W, 3), np.int64)
    Dp = np.zeros((V, H, W), np.int64)
    for v in range(V):
        present = c[v].any(axis=-1)
        cg, bg = (c[v], b[v]) if q is None else (G.apply(c[v], int(q[v])), G.apply(b[v], int(q[v])))
        cg, bg = cg.astype(np.int64), bg.astype(np.int64)
        wt = np.where(present, np.minimum(D[v], ramp), 0)
        assert (D[v][present] >= 1).all()
        total += wt[..., None] * bg
        wsum += wt
        count += present
        Dp[v] = np.where(present, D[v], 0)
        better = Dp[v] > best           # strictly: the lowest index wins a tie
        detail[better] = (cg - bg)[better]
        source[better] = v
        best = np.where(better, Dp[v], best)
    raw = total // np.maximum(wsum, 1)[..., None] + detail
    tied = ((Dp == best[None]) & (Dp > 0)).sum(axis=0)
    return Band(np.clip(raw, 0, 255).astype(np.uint8), raw, wsum, total, count, best, source, tied)


def compose_band(center, layers, geometries, coords, ramp, band, sampling="nearest", q=None):
    """The two-band blend of the centre and ``layers[k].img`` sampled at ``coords[k] = (tx, ty)``: a :class:`Band`."""
    return blend(*views(center, layers, geometries, coords, band, sampling), ramp, q)
