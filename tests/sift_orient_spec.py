"""Specification of keypoint orientation and of the SIFT descriptor at a given orientation, in numpy (test infrastructure; the
product never imports it): OpenCV 4.x's ``calcOrientationHist`` and ``calcSIFTDescriptor`` for a size-1, octave-0 keypoint,
restated operation by operation as csrc/apap_sift_orient.hip computes them, vectorised over the keypoints.  DESIGN.md
"Keypoint orientation" holds the contract in words.

* ``orient(img, pts)`` / ``describe(img, pts, angles)``: the float32 specification.  Every operation is a single IEEE float32
  operation in the kernel's order with the kernel's own constants (``taps``, ``orient_window``, ``descr_window``: pass
  ``_native.sift_taps()``, ``_native.sift_orient_window()``, ``_native.sift_descr_window()``; the defaults are this module's
  float64 evaluation rounded to float32).  The GPU's bytes must equal its bytes.  ``describe(img, pts, None)`` is the fused
  form: the descriptor at ``orient``'s angle.
* ``orient64`` / ``describe64``: the "mathematical" definition in float64 - exact atan2, sin, cos and exp, unrounded constants.

Shared with tests/sift_spec.py: the grey image, the virtual base image, pt = (rint x, rint y), the central differences, the
project's atan2 in degrees and the rule that a sample counts only if 0 < r < h - 1 and 0 < c < w - 1; the threshold, the tree
sums, the scaling, rint and the clamp at the descriptor's end.

Orientation.  25 offsets (i, j), |i|, |j| <= 2, i ascending, then j; W = exp(-(i^2 + j^2) / (2 0.75^2)); bin = rint(ang 0.1),
half to even, 36 -> 0; hist[b] = sum of W sqrt(dx^2 + dy^2) over the valid samples of bin b in ascending sample order;
smoothed = (t[b-2] + t[b+2]) / 16 + (t[b-1] + t[b+1]) 4 / 16 + t[b] 6 / 16, circular; j = the FIRST largest smoothed bin;
off = 0.5 (l - r) / ((l - 2 c) + r), 0 where the denominator is 0; bin = j + off wrapped into [0, 36); angle = 360 - 10 bin,
0 where |angle - 360| < FLT_EPSILON.

Descriptor at ``angle``.  ori = 360 - angle, 0 where |ori - 360| < FLT_EPSILON; q = the quadrant of ori, r = ori - 90 q (exact),
x = r (pi / 180), sin x = x S(x^2), cos x = C(x^2) by Horner, turned back by the quadrant; 121 offsets |i|, |j| <= 5;
c_rot = (j cos - i sin) / 1.5, r_rot = (j sin + i cos) / 1.5, rbin = r_rot + 1.5, cbin = c_rot + 1.5; a sample counts if
-1 < rbin < 4, -1 < cbin < 4 and the image test holds; weight exp(-(i^2 + j^2) / 18); obin = (ang - ori) 8 / 360; floors and
fractions per sample; the trilinear spread and everything after it as tests/sift_spec.py.
"""
import numpy as np

import sift_spec as S

DIM, TAPS = S.DIM, S.TAPS
PATCH, BASE = 25, 13            # the grey patch one keypoint reads, and the base-image patch it gives
ORI_RADIUS, ORI_SAMPLES, ORI_BINS = 2, 25, 36
DESCR_RADIUS, DESCR_SAMPLES = 5, 121
MIN_SIDE = 13
EPS32 = S.EPS32

# sin x = x S(x^2), cos x = C(x^2) on [0, pi / 2]: the kernel's coefficients (the Taylor series' own), highest power first
SIN_P = [np.float32(c) for c in (-2.505210794e-08, 2.755731884e-06, -1.984127011e-04, 8.333333768e-03, -1.666666716e-01, 1.0)]
COS_P = [np.float32(c) for c in (2.087675588e-09, -2.755731998e-07, 2.480158764e-05, -1.388888923e-03, 4.166666791e-02, -0.5, 1.0)]
RAD_F = np.float32(1.745329238e-02)
ORI_BINS_F = np.float32(0.1)
assert RAD_F == np.float32(np.pi / 180) and ORI_BINS_F == np.float32(36) / np.float32(360)
assert SIN_P == [np.float32(v) for v in (-1 / 39916800, 1 / 362880, -1 / 5040, 1 / 120, -1 / 6, 1)]
assert COS_P == [np.float32(v) for v in (1 / 479001600, -1 / 3628800, 1 / 40320, -1 / 720, 1 / 24, -1 / 2, 1)]


def offsets(radius):
    """The offsets (i, j) of a (2 radius + 1)^2 window, i ascending, then j: two int64 arrays."""
    side = 2 * radius + 1
    ii, jj = np.divmod(np.arange(side * side), side)
    return ii - radius, jj - radius


def orient_window_f64():
    """The 25 weights of the orientation samples in float64; asserts OpenCV's radius round(3 * 1.5 * 0.5) = 2."""
    assert int(np.rint(3 * 1.5 * 0.5)) == ORI_RADIUS
    ii, jj = offsets(ORI_RADIUS)
    return np.exp(-(ii * ii + jj * jj) / (2.0 * 0.75 * 0.75))


def descr_window_f64():
    """The 121 weights of the descriptor samples in float64: exp(-(c_rot^2 + r_rot^2) / 8) with c_rot^2 + r_rot^2 =
    (i^2 + j^2) / 1.5^2, whatever the angle."""
    assert int(np.rint(1.5 * np.sqrt(2) * 5 * 0.5)) == DESCR_RADIUS
    ii, jj = offsets(DESCR_RADIUS)
    return np.exp(-(ii * ii + jj * jj) / (2.25 * 8.0))


def sincos_deg32(ori):
    """The kernel's (cos, sin) of an angle in degrees in [0, 360): float32 arrays in and out."""
    ori = np.asarray(ori, np.float32)
    q = (ori >= np.float32(90)).astype(np.int64) + (ori >= np.float32(180)) + (ori >= np.float32(270))
    r = ori - np.float32(90) * q.astype(np.float32)
    x = r * RAD_F
    s = x * x
    p = np.full_like(x, SIN_P[0])
    for c in SIN_P[1:]:
        p = p * s + c
    sn = x * p
    cs = np.full_like(x, COS_P[0])
    for c in COS_P[1:]:
        cs = cs * s + c
    cos = np.select([q == 0, q == 1, q == 2], [cs, -sn, -cs], sn)
    sin = np.select([q == 0, q == 1, q == 2], [sn, cs, -sn], -cs)
    return cos.astype(np.float32), sin.astype(np.float32)


def sincos_deg64(ori):
    rad = np.radians(np.asarray(ori, np.float64))
    return np.cos(rad), np.sin(rad)


def blur_patch(g, py, px, taps):
    """The kernel's way: the (n, 13, 13) base-image patches around (py, px) from (n, 25, 25) grey patches alone."""
    dt = taps.dtype
    h, w = g.shape
    ys = S.reflect101(py[:, None] - 12 + np.arange(PATCH)[None, :], h)
    xs = S.reflect101(px[:, None] - 12 + np.arange(PATCH)[None, :], w)
    patch = g[ys[:, :, None], xs[:, None, :]].astype(dt)
    hb = np.zeros((len(py), PATCH, BASE), dt)
    for t in range(TAPS):
        hb = hb + taps[t] * patch[:, :, t:t + BASE]
    out = np.zeros((len(py), BASE, BASE), dt)
    for t in range(TAPS):
        out = out + taps[t] * hb[:, t:t + BASE, :]
    return out


class Frame:
    """What both stages read of one image: the rounded keypoints and the gradients of the base image around them."""

    def __init__(self, img, pts, taps, local):
        self.taps, self.local = taps, local
        self.g = S.grey(img)
        self.h, self.w = self.g.shape
        assert min(self.h, self.w) >= MIN_SIDE
        pts = np.ascontiguousarray(pts, dtype=np.float32).reshape(-1, 2)
        self.n = len(pts)
        finite = np.isfinite(pts).all(axis=1)
        rp = np.rint(np.where(finite[:, None], pts, np.float32(-100)))
        # can have a valid descriptor sample at all (the kernel's gate; orientation samples lie further in)
        self.near = finite & (rp[:, 0] > -5) & (rp[:, 0] < self.w + 4) & (rp[:, 1] > -5) & (rp[:, 1] < self.h + 4)
        self.px = np.where(self.near, rp[:, 0], -100).astype(np.int64)
        self.py = np.where(self.near, rp[:, 1], -100).astype(np.int64)
        self.base = None if local else S.blur_full(self.g, taps)
        self.patches = blur_patch(self.g, np.clip(self.py, -50, self.h + 50), np.clip(self.px, -50, self.w + 50), taps) if local else None

    def gradients(self, radius):
        """(dx, dy, valid), each (n, (2 radius + 1)^2), of the samples at the offsets of ``offsets(radius)``."""
        ii, jj = offsets(radius)
        sy, sx = self.py[:, None] + ii[None, :], self.px[:, None] + jj[None, :]
        valid = (sy > 0) & (sy < self.h - 1) & (sx > 0) & (sx < self.w - 1)
        if self.local:
            rows = np.arange(self.n)[:, None]
            r, c = 6 + ii[None, :], 6 + jj[None, :]
            b = self.patches
            dx = b[rows, r, c + 1] - b[rows, r, c - 1]
            dy = b[rows, r - 1, c] - b[rows, r + 1, c]
        else:
            cy, cx = np.clip(sy, 1, self.h - 2), np.clip(sx, 1, self.w - 2)
            b = self.base
            dx = b[cy, cx + 1] - b[cy, cx - 1]
            dy = b[cy - 1, cx] - b[cy + 1, cx]
        return dx, dy, valid


def _orient(fr, window, atan2_deg, detail=None):
    dt = fr.taps.dtype.type
    f32 = dt is np.float32
    dx, dy, valid = fr.gradients(ORI_RADIUS)
    n = fr.n
    term = window.astype(dt)[None, :] * np.sqrt(dx * dx + dy * dy)
    ang = atan2_deg(dy, dx)
    scaled = ang * (ORI_BINS_F if f32 else 36.0 / 360.0)
    b = np.rint(scaled)
    b = np.where(b >= 36, b - 36, b).astype(np.int64)
    hist = np.zeros((n, ORI_BINS), dt)
    rows = np.arange(n)
    for k in range(ORI_SAMPLES):                 # ascending sample order
        hist[rows, b[:, k]] += np.where(valid[:, k], term[:, k], dt(0))
    t = hist
    sm = (np.roll(t, 2, 1) + np.roll(t, -2, 1)) * dt(1 / 16) + (np.roll(t, 1, 1) + np.roll(t, -1, 1)) * dt(4 / 16) + t * dt(6 / 16)
    j = np.argmax(sm, axis=1)                    # the first of the largest
    c, l, r = sm[rows, j], sm[rows, (j + 35) % 36], sm[rows, (j + 1) % 36]
    num = dt(0.5) * (l - r)
    den = (l - dt(2) * c) + r
    off = np.where(den == 0, dt(0), num / np.where(den == 0, dt(1), den))
    raw = j.astype(dt) + off
    bn = np.where(raw < 0, dt(36) + raw, np.where(raw >= 36, raw - dt(36), raw))
    angle = dt(360) - dt(10) * bn
    eps = EPS32 if f32 else np.finfo(np.float32).eps
    flushed = np.abs(angle - dt(360)) < eps
    angle = np.where(flushed, dt(0), angle)
    if detail is not None:
        detail.update(ang=ang, scaled=scaled, bin=b, valid=valid, hist=hist, smooth=sm, peak=j, den=den, raw=raw, flushed=flushed)
    return angle.astype(dt)


def _describe(fr, angles, window, atan2_deg, sincos, detail=None):
    dt = fr.taps.dtype.type
    f32 = dt is np.float32
    eps = EPS32 if f32 else np.finfo(np.float32).eps
    n = fr.n
    angles = np.asarray(angles, dt).reshape(n)
    good = np.isfinite(angles) & (angles >= 0) & (angles <= 360)
    angle = np.where(good, angles, dt(0))
    ori = dt(360) - angle
    ori = np.where(np.abs(ori - dt(360)) < eps, dt(0), ori)
    cs, sn = sincos(ori)
    cs, sn = cs[:, None], sn[:, None]
    dx, dy, valid = fr.gradients(DESCR_RADIUS)
    ii, jj = offsets(DESCR_RADIUS)
    fi, fj = ii.astype(dt)[None, :], jj.astype(dt)[None, :]
    c_rot = (fj * cs - fi * sn) / dt(1.5)
    r_rot = (fj * sn + fi * cs) / dt(1.5)
    rbin, cbin = r_rot + dt(1.5), c_rot + dt(1.5)
    counted = valid & (rbin > -1) & (rbin < 4) & (cbin > -1) & (cbin < 4) & good[:, None]
    mag = np.sqrt(dx * dx + dy * dy) * window.astype(dt)[None, :]
    mag = np.where(counted, mag, dt(0))
    ang = atan2_deg(dy, dx)
    obin = (ang - ori[:, None]) * (S.BINS_F if f32 else 8.0 / 360.0)
    r0f, c0f, o0f = np.floor(rbin), np.floor(cbin), np.floor(obin)
    frac_r, frac_c, fo = rbin - r0f, cbin - c0f, obin - o0f
    r0 = np.where(counted, r0f, 0).astype(np.int64)
    c0 = np.where(counted, c0f, 0).astype(np.int64)
    o0 = (o0f.astype(np.int64) + 16) & 7
    v_r1 = mag * frac_r
    v_r0 = mag - v_r1
    v11 = v_r1 * frac_c
    v10 = v_r1 - v11
    v01 = v_r0 * frac_c
    v00 = v_r0 - v01
    spatial = {(0, 0): v00, (0, 1): v01, (1, 0): v10, (1, 1): v11}
    hist = np.zeros((n, 6, 6, 8), dt)           # rows, columns with OpenCV's border of one; the orientation already wrapped
    rows = np.arange(n)
    for k in range(DESCR_SAMPLES):               # ascending sample order: a bin receives at most one share per sample
        for (dr, dc), v in spatial.items():
            v1 = v[:, k] * fo[:, k]
            hist[rows, r0[:, k] + 1 + dr, c0[:, k] + 1 + dc, o0[:, k]] += v[:, k] - v1
            hist[rows, r0[:, k] + 1 + dr, c0[:, k] + 1 + dc, (o0[:, k] + 1) & 7] += v1
    vec = hist[:, 1:5, 1:5, :].reshape(n, DIM)
    thr = dt(0.2) * np.sqrt(S.tree_sum(vec * vec))
    vec = np.minimum(vec, thr[:, None])
    nrm = np.maximum(np.sqrt(S.tree_sum(vec * vec)), eps)
    scale = dt(512) / nrm
    out = np.clip(np.rint(vec * scale[:, None]), 0, 255)
    if detail is not None:
        detail.update(ori=ori, cos=cs[:, 0], sin=sn[:, 0], rbin=rbin, cbin=cbin, valid=valid, counted=counted, obin=obin)
    return out.astype(np.float32)


def _consts32(taps, window, default):
    taps = S.taps_f64().astype(np.float32) if taps is None else np.asarray(taps, np.float32)
    window = default().astype(np.float32) if window is None else np.asarray(window, np.float32)
    assert taps.shape == (TAPS,) and window.shape == default().shape
    return taps, window


def orient(img, pts, taps=None, orient_window=None, local=False, detail=None):
    """The float32 specification of the orientation: (n,) float32 in [0, 360), what ``cv.KeyPoint.angle`` would hold.
    ``local``: the base image from 25 x 25 patches (the kernel's way) instead of the whole image's blur - the same bits.
    ``detail``: a dict that receives the intermediate arrays."""
    taps, window = _consts32(taps, orient_window, orient_window_f64)
    return _orient(Frame(img, pts, taps, local), window, S.atan2_deg32, detail)


def describe(img, pts, angles=None, taps=None, orient_window=None, descr_window=None, local=False, detail=None):
    """The float32 specification of the descriptor at ``angles`` (n,), or at ``orient``'s when ``angles`` is None (the fused
    form): (n, 128) float32.  A keypoint with a non-finite coordinate, or an angle that is not in [0, 360], is a zero row."""
    taps, dwin = _consts32(taps, descr_window, descr_window_f64)
    fr = Frame(img, pts, taps, local)
    if angles is None:
        angles = _orient(fr, _consts32(taps, orient_window, orient_window_f64)[1], S.atan2_deg32)
    return _describe(fr, angles, dwin, S.atan2_deg32, sincos_deg32, detail)


def orient64(img, pts, detail=None):
    """The mathematical definition of the orientation in float64."""
    return _orient(Frame(img, pts, S.taps_f64(), False), orient_window_f64(), S.atan2_deg64, detail)


def describe64(img, pts, angles=None, detail=None):
    """The mathematical definition of the descriptor in float64, at ``angles`` or at ``orient64``'s."""
    fr = Frame(img, pts, S.taps_f64(), False)
    if angles is None:
        angles = _orient(fr, orient_window_f64(), S.atan2_deg64)
    return _describe(fr, angles, descr_window_f64(), S.atan2_deg64, sincos_deg64, detail)
