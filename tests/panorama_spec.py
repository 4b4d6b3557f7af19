"""The panorama in numpy: the union canvas and the composition of finished layer canvases (DESIGN.md "Panorama").

Nothing here computes a warp: a layer canvas is ``local_warp`` of its pair, from the oracle or from the engine's own
single-pair call, and the composition is integer arithmetic on bytes.  A geometry is ``(fw, fh, ox, oy)``: the pair canvas
and the offsets of the centre picture on it, what ``final_size`` returns for the pair."""
import numpy as np

MAX_LAYERS = 16


def panorama_size(center_shape, geometries):
    """(W, H, OX, OY): the centre sits at (OX, OY) = (max ox, max oy); the canvas reaches as far right of it and below it as
    the farthest pair canvas.  ValueError for no layer or more than 16, a centre outside a pair canvas, 2^31 pixels or more."""
    if not 1 <= len(geometries) <= MAX_LAYERS:
        raise ValueError("1 .. 16 layers")
    ch, cw = center_shape[:2]
    for fw, fh, ox, oy in geometries:
        if fw < 1 or fh < 1 or ox < 0 or oy < 0 or ox + cw > fw or oy + ch > fh:
            raise ValueError("the centre does not fit a pair canvas")
    OX = max(g[2] for g in geometries)
    OY = max(g[3] for g in geometries)
    W = OX + max(g[0] - g[2] for g in geometries)
    H = OY + max(g[1] - g[3] for g in geometries)
    if W * H >= 2 ** 31:
        raise ValueError("canvas of 2^31 pixels or more")
    return W, H, OX, OY


def placed(center, layer_canvases, geometries):
    """The centre and every layer canvas on the union canvas, black elsewhere: an array (K + 1, H, W, 3), the centre first."""
    W, H, OX, OY = panorama_size(center.shape, geometries)
    stack = np.zeros((len(geometries) + 1, H, W, 3), np.uint8)
    stack[0, OY:OY + center.shape[0], OX:OX + center.shape[1]] = center
    for k, (canvas, (fw, fh, ox, oy)) in enumerate(zip(layer_canvases, geometries)):
        assert canvas.shape == (fh, fw, 3) and canvas.dtype == np.uint8
        stack[k + 1, OY - oy:OY - oy + fh, OX - ox:OX - ox + fw] = canvas
    return stack


def present_count(center, layer_canvases, geometries):
    """Per canvas pixel, how many of the K + 1 pictures have a non-zero byte there."""
    return placed(center, layer_canvases, geometries).any(axis=-1).sum(axis=0)


def compose(center, layer_canvases, geometries, mode):
    """mean: per channel floor(sum of the present values / their number), 0 where none is present (a value is present when
    any of its bytes is non-zero; an absent value is all zero, so the plain sum is the sum of the present ones).
    paste: the centre inside its rectangle, black pixels included; elsewhere the first present layer, or 0."""
    stack = placed(center, layer_canvases, geometries)
    if mode == "mean":
        count = stack.any(axis=-1).sum(axis=0).astype(np.int64)
        total = stack.astype(np.int64).sum(axis=0)
        return (total // np.maximum(count, 1)[..., None]).astype(np.uint8)
    if mode != "paste":
        raise ValueError(mode)
    W, H, OX, OY = panorama_size(center.shape, geometries)
    out = np.zeros((H, W, 3), np.uint8)
    open_ = np.ones((H, W), bool)
    for layer in stack[1:]:
        take = open_ & layer.any(axis=-1)
        out[take] = layer[take]
        open_ &= ~take
    out[OY:OY + center.shape[0], OX:OX + center.shape[1]] = center
    return out
