"""The panorama's edge-ramp blend in numpy (DESIGN.md "Panorama", blend ``ramp``): exact integers.

Unlike ``panorama_spec.compose`` this composition cannot start from finished layer canvases: a sample's weight is a function
of the SOURCE pixel it was gathered from.  It starts from the target coordinates of every pair canvas - the oracle's
``warp_coords_fast`` or the engine's ``_native.warp_coords`` - and derives the strict bounds test, the truncation, the gathered
pixel, its presence and its weight from them.  Canvas and geometries are ``panorama_spec``'s."""
import numpy as np

from panorama_spec import panorama_size

MAX_RAMP = 256


def weight_map(h, w, R):
    """(h, w) int64: min(d, R) with d = min(x + 1, w - x, y + 1, h - y), the pixel's distance from the border counted from 1."""
    x, y = np.arange(w, dtype=np.int64)[None, :], np.arange(h, dtype=np.int64)[:, None]
    d = np.minimum(np.minimum(x + 1, w - x), np.minimum(y + 1, h - y))
    return np.minimum(d, R)


def gathered(img, tx, ty):
    """Of one pair canvas: ``inside`` (the strict test 0 < t < size of local_warp) and the truncated source pixel (ix, iy),
    (0, 0) where the sample is outside."""
    h, w = img.shape[:2]
    with np.errstate(invalid="ignore"):
        inside = (0 < tx) & (tx < w) & (0 < ty) & (ty < h)
    ix = np.where(inside, tx, 0).astype(np.int64)
    iy = np.where(inside, ty, 0).astype(np.int64)
    return inside, ix, iy


def compose_ramp(center, layers, geometries, coords, R):
    """``layers[k].img`` sampled at ``coords[k] = (tx, ty)``, both (fh_k, fw_k) float64, and the centre, each sample weighted by
    ``weight_map`` of its own picture at its own pixel; a sample is present when it lies inside its picture and any of its
    bytes is non-zero.  Returns ``(canvas, wsum, count)``: per channel floor(sum of weight x value / sum of weight) over the
    present samples and 0 where there is none; the sum of their weights; their number."""
    if not (isinstance(R, (int, np.integer)) and 1 <= R <= MAX_RAMP):
        raise ValueError("ramp 1 .. 256")
    W, H, OX, OY = panorama_size(center.shape, geometries)
    total = np.zeros((H, W, 3), np.int64)
    wsum = np.zeros((H, W), np.int64)
    count = np.zeros((H, W), np.int64)

    def add(rows, cols, values, weights):
        present = values.any(axis=-1)
        wt = np.where(present, weights, 0)
        total[rows, cols] += wt[..., None] * values.astype(np.int64)
        wsum[rows, cols] += wt
        count[rows, cols] += present

    ch, cw = center.shape[:2]
    add(slice(OY, OY + ch), slice(OX, OX + cw), center, weight_map(ch, cw, R))
    for layer, (fw, fh, ox, oy), (tx, ty) in zip(layers, geometries, coords):
        img = np.asarray(layer.img)
        assert tx.shape == ty.shape == (fh, fw)
        inside, ix, iy = gathered(img, tx, ty)
        values = np.where(inside[..., None], img[iy, ix], 0).astype(np.uint8)
        add(slice(OY - oy, OY - oy + fh), slice(OX - ox, OX - ox + fw), values, weight_map(*img.shape[:2], R)[iy, ix])
    return (total // np.maximum(wsum, 1)[..., None]).astype(np.uint8), wsum, count
