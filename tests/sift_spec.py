"""Specification of SIFT descriptor extraction at given keypoints, in numpy (test infrastructure; the product never imports
it): OpenCV 4.x's ``SIFT.compute`` for ``KeyPoint(x, y, 1)`` - size 1, angle -1, octave 0 - restated operation by operation
as csrc/apap_sift.hip computes it, vectorised over the keypoints.

* ``describe(img, pts)``: the float32 specification.  Every operation is a single IEEE float32 operation in the kernel's
  order, with the kernel's own constants (``taps``, ``window``: pass ``_native.sift_taps()`` / ``_native.sift_window()``;
  the defaults are this module's float64 evaluation rounded to float32).  The GPU's bytes must equal its bytes.
* ``describe64(img, pts)``: the "mathematical" definition in float64 - exact atan2 and exp, unrounded constants.

Definition.  grey: (h, w) uint8 as it is, (h, w, 3) is BGR -> (3735 B + 19235 G + 9798 R + 16384) >> 15.  base = grey as
float under a separable 13-tap Gaussian, sigma = sqrt(1.6^2 - 0.5^2), reflect-101, rows (horizontal pass) first, each pass
starting from 0 with the taps ascending.  pt = (rint(x), rint(y)).  The angle is 361 degrees, hist_width = 1.5; a sample (i, j),
|i|, |j| <= 3 (the only offsets with -1 < rbin, cbin < 4: ``window_f64`` asserts it) counts if 0 < pt.y + i < h - 1 and
0 < pt.x + j < w - 1.  dx, dy by central differences; mag = sqrt(dx^2 + dy^2) w; obin = (atan2(dy, dx) in degrees - 361)
8 / 360; trilinear spread OpenCV's way (v1 = v f, v0 = v - v1) over rows, columns, orientations, the orientation index wrapped
into 0 .. 7; a bin's contributions are added in ascending sample order.  Then thr = 0.2 sqrt(sum v^2), v = min(v, thr),
scale = 512 / max(sqrt(sum v^2), FLT_EPSILON), out = rint(v scale) clamped to 0 .. 255.  The two sums of squares go by a
fixed binary tree: x[b] + x[b + 64], then the halves of what is left added again and again (64 -> 32 -> .. -> 1).
"""
import numpy as np

DIM, SAMPLES, TAPS, PATCH, WINDOW_COLS = 128, 49, 13, 21, 8
RADIUS = 5                      # OpenCV's: round(1.5 sqrt(2) (4 + 1) / 2)
EPS32 = np.float32(np.finfo(np.float32).eps)

# atan(a) = a p(a^2) on [0, 1]: the kernel's coefficients, highest power first
ATAN_P = [np.float32(c) for c in (-4.054558929e-03, 2.186292969e-02, -5.591228977e-02, 9.642194957e-02, -1.390862912e-01,
                                  1.994656622e-01, -3.332985938e-01, 9.999993443e-01)]
PI_F, HALF_PI_F, DEG_F, BINS_F = np.float32(3.141592741), np.float32(1.570796371), np.float32(57.29578018), np.float32(2.222222276e-02)
assert PI_F == np.float32(np.pi) and HALF_PI_F == np.float32(np.pi / 2) and DEG_F == np.float32(180 / np.pi) and \
    BINS_F == np.float32(8) / np.float32(360)


def taps_f64():
    t = np.arange(TAPS) - 6.0
    g = np.exp(-t * t / (2.0 * (1.6 * 1.6 - 0.5 * 0.5)))
    return g / g.sum()


def window_f64():
    """The (49, 8) table of the samples in float64: rbin, cbin, w, frac(rbin), frac(cbin), floor(rbin), floor(cbin), 0; rows in
    the order (i, j) ascending.  Walks OpenCV's whole radius and asserts that exactly |i|, |j| <= 3 pass the bin test."""
    ang = 361.0 * (np.pi / 180.0)
    cs, sn = np.cos(ang) / 1.5, np.sin(ang) / 1.5
    rows, offsets = [], []
    for i in range(-RADIUS, RADIUS + 1):
        for j in range(-RADIUS, RADIUS + 1):
            c_rot, r_rot = j * cs - i * sn, j * sn + i * cs
            rbin, cbin = r_rot + 1.5, c_rot + 1.5
            if -1 < rbin < 4 and -1 < cbin < 4:
                offsets.append((i, j))
                rows.append([rbin, cbin, np.exp(-(c_rot * c_rot + r_rot * r_rot) / 8.0), rbin - np.floor(rbin), cbin - np.floor(cbin),
                             np.floor(rbin), np.floor(cbin), 0.0])
    assert offsets == [(i, j) for i in range(-3, 4) for j in range(-3, 4)]
    return np.array(rows)


def grey(img):
    img = np.asarray(img)
    assert img.dtype == np.uint8
    if img.ndim == 2:
        return img
    if img.shape[2] == 1:
        return img[:, :, 0]
    b, g, r = (img[:, :, k].astype(np.int64) for k in range(3))
    return ((3735 * b + 19235 * g + 9798 * r + 16384) >> 15).astype(np.uint8)


def reflect101(i, n):
    """Reflect-101 of an index array, once (enough for -6 .. n + 5 when n >= 7), then clamped like the kernel's."""
    i = np.where(i < 0, -i, i)
    i = np.where(i > n - 1, 2 * (n - 1) - i, i)
    return np.clip(i, 0, n - 1)


def blur_full(g, taps):
    """The base image of a whole grey image, in taps.dtype: horizontal pass, then vertical, each from 0 with the taps ascending."""
    dt = taps.dtype
    g = g.astype(dt)
    h, w = g.shape
    cols = reflect101(np.arange(w)[None, :] + np.arange(TAPS)[:, None] - 6, w)
    hb = np.zeros((h, w), dt)
    for t in range(TAPS):
        hb = hb + taps[t] * g[:, cols[t]]
    rows = reflect101(np.arange(h)[None, :] + np.arange(TAPS)[:, None] - 6, h)
    out = np.zeros((h, w), dt)
    for t in range(TAPS):
        out = out + taps[t] * hb[rows[t], :]
    return out


def blur_patch(g, py, px, taps):
    """The kernel's way: the (n, 9, 9) base-image patches around (py, px) from (n, 21, 21) grey patches alone."""
    dt = taps.dtype
    h, w = g.shape
    ys = reflect101(py[:, None] - 10 + np.arange(PATCH)[None, :], h)
    xs = reflect101(px[:, None] - 10 + np.arange(PATCH)[None, :], w)
    patch = g[ys[:, :, None], xs[:, None, :]].astype(dt)
    hb = np.zeros((len(py), PATCH, 9), dt)
    for t in range(TAPS):
        hb = hb + taps[t] * patch[:, :, t:t + 9]
    out = np.zeros((len(py), 9, 9), dt)
    for t in range(TAPS):
        out = out + taps[t] * hb[:, t:t + 9, :]
    return out


def atan2_rad32(y, x):
    """The kernel's atan2 in radians, (-pi, pi], float32 arrays in and out: a = min / max of the magnitudes in [0, 1],
    atan(a) = a p(a^2) by Horner (a multiply and an add per step), then the octant.  atan2(0, 0) = 0."""
    y, x = np.asarray(y, np.float32), np.asarray(x, np.float32)
    ax, ay = np.abs(x), np.abs(y)
    mx, mn = np.maximum(ax, ay), np.minimum(ax, ay)
    zero = mx == 0
    a = mn / np.where(zero, np.float32(1), mx)
    s = a * a
    p = np.full_like(a, ATAN_P[0])
    for c in ATAN_P[1:]:
        p = p * s + c
    r = a * p
    r = np.where(ay > ax, HALF_PI_F - r, r)
    r = np.where(x < 0, PI_F - r, r)
    r = np.where(y < 0, -r, r)
    return np.where(zero, np.float32(0), r).astype(np.float32)


def atan2_deg32(y, x):
    """The kernel's atan2 in degrees, [0, 360], float32 arrays in and out: one multiply, and 360 added below 0."""
    deg = atan2_rad32(y, x) * DEG_F
    return np.where(deg < 0, deg + np.float32(360), deg).astype(np.float32)


def atan2_deg64(y, x):
    deg = np.degrees(np.arctan2(y, x))
    return np.where(deg < 0, deg + 360.0, deg)


def tree_sum(x):
    """Sum over the last axis (128) by the kernel's tree: x[b] + x[b + 64], then halves again and again."""
    while x.shape[-1] > 1:
        half = x.shape[-1] // 2
        x = x[..., :half] + x[..., half:]
    return x[..., 0]


def _describe(img, pts, taps, window, atan2_deg, local):
    dt = taps.dtype.type
    g = grey(img)
    h, w = g.shape
    pts = np.ascontiguousarray(pts, dtype=np.float32).reshape(-1, 2)
    n = len(pts)
    finite = np.isfinite(pts).all(axis=1)
    rp = np.rint(np.where(finite[:, None], pts, np.float32(-100)))
    near = finite & (rp[:, 0] > -3) & (rp[:, 0] < w + 2) & (rp[:, 1] > -3) & (rp[:, 1] < h + 2)      # can have a valid sample at all
    px = np.where(near, rp[:, 0], -100).astype(np.int64)
    py = np.where(near, rp[:, 1], -100).astype(np.int64)
    ii, jj = np.divmod(np.arange(SAMPLES), 7)
    ii, jj = ii - 3, jj - 3
    sy, sx = py[:, None] + ii[None, :], px[:, None] + jj[None, :]
    valid = (sy > 0) & (sy < h - 1) & (sx > 0) & (sx < w - 1)
    if local:
        base = blur_patch(g, np.clip(py, -50, h + 50), np.clip(px, -50, w + 50), taps)
        rows = np.arange(n)[:, None]
        r, c = 4 + ii[None, :], 4 + jj[None, :]
        dx = base[rows, r, c + 1] - base[rows, r, c - 1]
        dy = base[rows, r - 1, c] - base[rows, r + 1, c]
    else:
        base = blur_full(g, taps)
        cy, cx = np.clip(sy, 1, h - 2), np.clip(sx, 1, w - 2)
        dx = base[cy, cx + 1] - base[cy, cx - 1]
        dy = base[cy - 1, cx] - base[cy + 1, cx]
    wgt, fr, fc = (window[:, k].astype(dt)[None, :] for k in (2, 3, 4))
    r0, c0 = window[:, 5].astype(np.int64), window[:, 6].astype(np.int64)
    mag = np.sqrt(dx * dx + dy * dy) * wgt
    mag = np.where(valid, mag, dt(0))
    obin = (atan2_deg(dy, dx) - dt(361)) * (BINS_F if dt is np.float32 else 8.0 / 360.0)
    o0f = np.floor(obin)
    fo = obin - o0f
    o0 = (o0f.astype(np.int64) + 16) & 7
    v_r1 = mag * fr
    v_r0 = mag - v_r1
    v11 = v_r1 * fc
    v10 = v_r1 - v11
    v01 = v_r0 * fc
    v00 = v_r0 - v01
    spatial = {(0, 0): v00, (0, 1): v01, (1, 0): v10, (1, 1): v11}
    hist = np.zeros((n, 6, 6, 8), dt)           # rows, columns with OpenCV's border of one; the orientation already wrapped
    rows = np.arange(n)
    for k in range(SAMPLES):                     # ascending sample order: a bin receives at most one share per sample
        for (dr, dc), v in spatial.items():
            v1 = v[:, k] * fo[:, k]
            hist[rows, r0[k] + 1 + dr, c0[k] + 1 + dc, o0[:, k]] += v[:, k] - v1
            hist[rows, r0[k] + 1 + dr, c0[k] + 1 + dc, (o0[:, k] + 1) & 7] += v1
    vec = hist[:, 1:5, 1:5, :].reshape(n, DIM)
    thr = dt(0.2) * np.sqrt(tree_sum(vec * vec))
    vec = np.minimum(vec, thr[:, None])
    nrm = np.maximum(np.sqrt(tree_sum(vec * vec)), np.finfo(np.float32).eps if dt is np.float64 else EPS32)
    scale = dt(512) / nrm
    out = np.clip(np.rint(vec * scale[:, None]), 0, 255)
    return out.astype(np.float32)


def describe(img, pts, taps=None, window=None, local=False):
    """The float32 specification: (n, 128) float32.  ``local``: the base image from 21 x 21 patches (the kernel's way) instead
    of the whole image's blur - the same bits (tests/test_sift_host.py)."""
    taps = taps_f64().astype(np.float32) if taps is None else np.asarray(taps, np.float32)
    window = window_f64().astype(np.float32) if window is None else np.asarray(window, np.float32)
    assert taps.shape == (TAPS,) and window.shape == (SAMPLES, WINDOW_COLS)
    return _describe(img, pts, taps, window, atan2_deg32, local)


def describe64(img, pts):
    """The mathematical definition in float64: exact atan2 and exp, unrounded constants, float64 sums."""
    return _describe(img, pts, taps_f64(), window_f64(), atan2_deg64, False)
