"""The specification of the global warp and blend (DESIGN.md "Global warp and blend") in plain numpy: int64 and float64,
vectorised, no fused operation.  It restates, without OpenCV,

* ``cv.perspectiveTransform`` on the four corners (``perspective_transform``) and the bounds arithmetic of the reference's
  ``image_warping`` (utils.py:99-107) - ``bounds``;
* ``cv.warpPerspective(src, M, (w, h))`` with its defaults INTER_LINEAR / BORDER_CONSTANT(0), in OpenCV 4.x's fixed-point
  form with exact integer weights - ``warp_perspective``;
* the paste and the mean blend of utils.py:115-126 - ``blend``;

and ``image_warping`` puts them together with the reference's own ``Ht.dot(H)``.  The library's kernel must give these bytes.

Deviation from OpenCV's binaries, stated once: OpenCV evaluates the coordinates block-wise (``X0 + M0 * x1`` from a block
origin) and has SIMD variants, so a binary of it may differ from this canonical left-to-right order in the last bit of ``X``
at rounding ties.  OpenCV is absent here; the definition is OpenCV's, restated, and is not pinned against OpenCV itself.
"""
import numpy as np

INTER_BITS = 5
INTER_TAB_SIZE = 1 << INTER_BITS          # 32
MAX_SIDE = 32767


def _f64_3x3(H):
    H = np.asarray(H)
    if H.shape != (3, 3):
        raise ValueError(f"expected a 3 x 3 matrix, got {H.shape}")
    return H.astype(np.float64)


def perspective_transform(pts, H):
    """``cv.perspectiveTransform`` for (n, 1, 2) float32 points: w = H20 x + H21 y + H22 in fp64, w = w ? 1 / w : 0, each
    coordinate (Hk0 x + Hk1 y + Hk2) * w rounded to float32."""
    H = _f64_3x3(H)
    pts = np.asarray(pts, np.float32)
    x, y = pts[..., 0].astype(np.float64), pts[..., 1].astype(np.float64)
    with np.errstate(all="ignore"):
        w = H[2, 0] * x + H[2, 1] * y + H[2, 2]
        w = np.where(w != 0.0, 1.0 / np.where(w != 0.0, w, 1.0), 0.0)
        out = np.stack([(H[0, 0] * x + H[0, 1] * y + H[0, 2]) * w, (H[1, 0] * x + H[1, 1] * y + H[1, 2]) * w], axis=-1)
        return out.astype(np.float32)


def bounds(h1, w1, h2, w2, H):
    """(xmin, ymin, xmax, ymax) of utils.py:101-106: the base picture's corners and the source's through ``H``; float32
    ``min - 0.5`` / ``max + 0.5`` truncated toward zero."""
    def corners(h, w):
        return np.array([[0, 0], [0, h], [w, h], [w, 0]], np.float32).reshape(4, 1, 2)

    pts = np.concatenate([corners(h1, w1), perspective_transform(corners(h2, w2), H)]).reshape(8, 2)
    lo = (pts.min(axis=0) - np.float32(0.5)).astype(np.float32)
    hi = (pts.max(axis=0) + np.float32(0.5)).astype(np.float32)
    xmin, ymin = (int(np.trunc(v)) for v in lo)
    xmax, ymax = (int(np.trunc(v)) for v in hi)
    return xmin, ymin, xmax, ymax


def det3(m):
    return m[0, 0] * (m[1, 1] * m[2, 2] - m[1, 2] * m[2, 1]) - m[0, 1] * (m[1, 0] * m[2, 2] - m[1, 2] * m[2, 0]) + \
        m[0, 2] * (m[1, 0] * m[2, 1] - m[1, 1] * m[2, 0])


def invert3(M):
    """``cv::invert`` of a 3 x 3 float64 matrix: the cofactors times ``1 / det3`` (scalar float64 operations, none fused)."""
    m = _f64_3x3(M)
    with np.errstate(all="ignore"):
        det = det3(m)
        if not np.isfinite(m).all() or det == 0.0 or not np.isfinite(det):
            raise ValueError("M is singular or not finite")
        d = np.float64(1.0) / det
        out = np.array([
            [(m[1, 1] * m[2, 2] - m[1, 2] * m[2, 1]) * d, (m[0, 2] * m[2, 1] - m[0, 1] * m[2, 2]) * d, (m[0, 1] * m[1, 2] - m[0, 2] * m[1, 1]) * d],
            [(m[1, 2] * m[2, 0] - m[1, 0] * m[2, 2]) * d, (m[0, 0] * m[2, 2] - m[0, 2] * m[2, 0]) * d, (m[0, 2] * m[1, 0] - m[0, 0] * m[1, 2]) * d],
            [(m[1, 0] * m[2, 1] - m[1, 1] * m[2, 0]) * d, (m[0, 1] * m[2, 0] - m[0, 0] * m[2, 1]) * d, (m[0, 0] * m[1, 1] - m[0, 1] * m[1, 0]) * d],
        ], np.float64)
    if not np.isfinite(out).all():
        raise ValueError("the inverse of M is not finite")
    return out


def fixed_coords(M, size):
    """X, Y (int64, (h, w)) of every canvas pixel: the source coordinate in 1/32 px."""
    w, h = size
    Minv = invert3(M)
    x = np.arange(w, dtype=np.float64)[None, :]
    y = np.arange(h, dtype=np.float64)[:, None]
    with np.errstate(all="ignore"):
        X0 = Minv[0, 0] * x + Minv[0, 1] * y + Minv[0, 2]
        Y0 = Minv[1, 0] * x + Minv[1, 1] * y + Minv[1, 2]
        W0 = Minv[2, 0] * x + Minv[2, 1] * y + Minv[2, 2]
        W = np.where(W0 != 0.0, np.float64(INTER_TAB_SIZE) / np.where(W0 != 0.0, W0, 1.0), 0.0)
        # fmax / fmin: a NaN product takes the lower bound
        fX = np.fmin(np.fmax(X0 * W, -2147483648.0), 2147483647.0)
        fY = np.fmin(np.fmax(Y0 * W, -2147483648.0), 2147483647.0)
    return np.rint(fX).astype(np.int64), np.rint(fY).astype(np.int64)     # round half to even


def sample(src, X, Y):
    """The bilinear sample at the fixed-point coordinates: exact integer weights, a tap outside the source is 0."""
    h2, w2 = src.shape[:2]
    sx, sy = np.clip(X >> INTER_BITS, -32768, 32767), np.clip(Y >> INTER_BITS, -32768, 32767)
    ax, ay = (X & (INTER_TAB_SIZE - 1))[..., None], (Y & (INTER_TAB_SIZE - 1))[..., None]
    s = src.astype(np.int64)

    def tap(yy, xx):
        ok = (xx >= 0) & (xx < w2) & (yy >= 0) & (yy < h2)
        return np.where(ok[..., None], s[np.clip(yy, 0, h2 - 1), np.clip(xx, 0, w2 - 1)], 0)

    p00, p01, p10, p11 = tap(sy, sx), tap(sy, sx + 1), tap(sy + 1, sx), tap(sy + 1, sx + 1)
    out = ((32 - ax) * (32 - ay) * p00 + ax * (32 - ay) * p01 + (32 - ax) * ay * p10 + ax * ay * p11 + 512) >> 10
    return out.astype(np.uint8)


def warp_perspective(src, M, size):
    """``cv.warpPerspective(src, M, size)`` (``size`` = (width, height)) for an (h, w, 3) uint8 picture."""
    src = np.asarray(src)
    if src.dtype != np.uint8 or src.ndim != 3 or src.shape[2] != 3:
        raise ValueError(f"expected an (h, w, 3) uint8 picture, got {src.dtype} {src.shape}")
    X, Y = fixed_coords(M, size)
    return sample(src, X, Y)


def blend(canvas, img_base, t, direct_blend=True):
    """utils.py:115-126 on a warped canvas: the paste, or the mean blend (the float32 mean truncated to uint8) where any
    channel of the warped pixel is non-zero."""
    out = canvas.copy()
    h1, w1 = img_base.shape[:2]
    region = out[t[1]:h1 + t[1], t[0]:w1 + t[0]]
    if region.shape != img_base.shape:
        raise ValueError("the base picture does not fit the canvas at the offsets")
    if direct_blend:
        region[...] = img_base
    else:
        mean = ((img_base.astype(np.int64) + region.astype(np.int64)) >> 1).astype(np.uint8)
        region[...] = np.where(region.any(axis=-1, keepdims=True), mean, img_base)
    return out


def matrix(H, t):
    """The reference's own ``Ht.dot(H)`` (utils.py:108-114)."""
    Ht = np.array([
        [1, 0, t[0]],
        [0, 1, t[1]],
        [0, 0, 1]])
    return Ht.dot(H)


def image_warping(img_base, img2warp, H, direct_blend=True):
    h1, w1 = img_base.shape[:2]
    h2, w2 = img2warp.shape[:2]
    xmin, ymin, xmax, ymax = bounds(h1, w1, h2, w2, H)
    t = [-xmin, -ymin]
    result = warp_perspective(img2warp, matrix(np.asarray(H), t), (xmax - xmin, ymax - ymin))
    return blend(result, img_base, t, direct_blend)
