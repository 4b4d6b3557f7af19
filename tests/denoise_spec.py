"""The specification of the notch denoising (csrc/apap_denoise.hip), in numpy: what the kernels compute, byte for byte.

The chain is ``apply_median_filter`` of the reference's pyviz/median_filter.py restated: equalise, 2-D transform, the notch
schedule on the shifted spectrum, inverse transform, magnitude.  The transform is the engine's own - a mixed-radix (4, 2, 3, 5)
Stockham transform in float64 whose every complex product is ``(ac - bd, ad + bc)``, each operation a numpy ufunc of its own (no
fused multiply-add), on the twiddle table the engine uses (``_native.fft_twiddles``: one table serves both sides).  Forward
is rows then columns; the inverse is columns then rows on the conjugate table, scaled once by the double ``1.0 / (H * W)``.
"""
import numpy as np

SIN3 = 0.8660254037844386        # sin(2 pi / 3)
COS5A = 0.30901699437494745      # cos(2 pi / 5)
COS5B = -0.8090169943749475      # cos(4 pi / 5)
SIN5A = 0.9510565162951535       # sin(2 pi / 5)
SIN5B = 0.5877852522924731       # sin(4 pi / 5)

MIN_LENGTH, MAX_LENGTH, MAX_R = 2, 4096, 6


def radix(rem):
    """The radix of the next stage of a length whose remaining factor is ``rem``: 4 while it divides, then 2, 3, 5."""
    for p in (4, 2, 3, 5):
        if rem % p == 0:
            return p
    raise ValueError(f"{rem} is not 5-smooth")


def five_smooth(n):
    for p in (2, 3, 5):
        while n % p == 0:
            n //= p
    return n == 1


def twiddles(n):
    """(n, 2) float64: cos, sin of -2 pi k / n - the engine's own table."""
    from cvx_proj_amd import _native
    return _native.fft_twiddles(n)


def _add(a, b):
    return a[0] + b[0], a[1] + b[1]


def _sub(a, b):
    return a[0] - b[0], a[1] - b[1]


def _scale(c, a):
    return c * a[0], c * a[1]


def _turn(u, sg):
    """-i sg u"""
    return sg * u[1], -(sg * u[0])


def _mul(a, w):
    return a[0] * w[0] - a[1] * w[1], a[0] * w[1] + a[1] * w[0]


def butterfly(p, a, sg):
    if p == 2:
        return [_add(a[0], a[1]), _sub(a[0], a[1])]
    if p == 4:
        t0, t1, t2, t3 = _add(a[0], a[2]), _sub(a[0], a[2]), _add(a[1], a[3]), _turn(_sub(a[1], a[3]), sg)
        return [_add(t0, t2), _add(t1, t3), _sub(t0, t2), _sub(t1, t3)]
    if p == 3:
        t1, t2 = _add(a[1], a[2]), _sub(a[1], a[2])
        m, u = _sub(a[0], _scale(0.5, t1)), _turn(_scale(SIN3, t2), sg)
        return [_add(a[0], t1), _add(m, u), _sub(m, u)]
    t1, t2, t3, t4 = _add(a[1], a[4]), _add(a[2], a[3]), _sub(a[1], a[4]), _sub(a[2], a[3])
    m1 = _add(_add(a[0], _scale(COS5A, t1)), _scale(COS5B, t2))
    m2 = _add(_add(a[0], _scale(COS5B, t1)), _scale(COS5A, t2))
    u1 = _turn(_add(_scale(SIN5A, t3), _scale(SIN5B, t4)), sg)
    u2 = _turn(_sub(_scale(SIN5B, t3), _scale(SIN5A, t4)), sg)
    return [_add(_add(a[0], t1), t2), _add(m1, u1), _add(m2, u2), _sub(m2, u2), _sub(m1, u1)]


def fft1_spec(re, im, tw, sg):
    """The transforms of the rows of (B, n) float64 ``re``, ``im``.  Stage of radix p, s the product of the earlier radices,
    m = n / (s p): butterfly (q, j) reads elements j + s (q + m k), writes j + s (p q + k) after the twiddle w^(q k s)."""
    B, n = re.shape
    wr, wi = tw[:, 0], sg * tw[:, 1]
    s, rem = 1, n
    while rem > 1:
        p = radix(rem)
        m = rem // p
        ar, ai = re.reshape(B, p, m, s), im.reshape(B, p, m, s)
        y = butterfly(p, [(ar[:, k], ai[:, k]) for k in range(p)], sg)
        outr, outi = np.empty((B, m, p, s)), np.empty((B, m, p, s))
        q = np.arange(m)
        for k in range(p):
            v = y[k]
            if k > 0:
                at = q * k * s
                v = _mul(v, (wr[at][None, :, None], wi[at][None, :, None]))
            outr[:, :, k, :], outi[:, :, k, :] = v
        re, im = outr.reshape(B, n), outi.reshape(B, n)
        s *= p
        rem = m
    return re, im


def fft2_parts(x, twiddles_h, twiddles_w, inverse=False):
    """(re, im) of the 2-D transform of the (H, W) complex plane ``x``."""
    x = np.asarray(x, dtype=np.complex128)
    H, W = x.shape
    re, im = np.ascontiguousarray(x.real), np.ascontiguousarray(x.imag)
    sg = -1.0 if inverse else 1.0

    def rows(re, im):
        return fft1_spec(re, im, twiddles_w, sg)

    def cols(re, im):
        r, i = fft1_spec(np.ascontiguousarray(re.T), np.ascontiguousarray(im.T), twiddles_h, sg)
        return np.ascontiguousarray(r.T), np.ascontiguousarray(i.T)

    if not inverse:
        return cols(*rows(re, im))
    re, im = rows(*cols(re, im))
    scale = 1.0 / (float(H) * float(W))
    return scale * re, scale * im


def fft2_spec(x, twiddles_h=None, twiddles_w=None, inverse=False):
    x = np.asarray(x)
    th = twiddles(x.shape[0]) if twiddles_h is None else twiddles_h
    tw = twiddles(x.shape[1]) if twiddles_w is None else twiddles_w
    re, im = fft2_parts(x, th, tw, inverse)
    return re + 1j * im


def shift_index(n):
    """``shifted[i] = plain[shift_index(n)[i]]``: np.fft.fftshift as index arithmetic (plain index k sits at (k + n // 2) % n)."""
    return (np.arange(n) - n // 2) % n


def notch_schedule(spacing=48, r=5, sn=9):
    """The calls of median_filter.py:149-155 in order, each (uk, vk, r1, r2): 77 for the defaults."""
    calls = []
    for i in range(2, sn):
        calls.append((i * spacing, i * spacing, r, 5 * r))
        for j in range(1, i):
            calls.append((j * spacing, i * spacing, r, 5 * r))
            calls.append((i * spacing, j * spacing, r, 5 * r))
        calls.append((0, i * spacing, 3, 3 * r))
        calls.append((i * spacing, 0, 3, 3 * r))
    return calls


def notch_check(spacing, r, sn):
    if not 1 <= r <= MAX_R:
        raise ValueError(f"r={r} (1 .. {MAX_R})")
    if sn < 2:
        raise ValueError(f"sn={sn} (at least 2)")
    if spacing <= max(6 * r, 5 * r + 3):
        raise ValueError(f"spacing={spacing} must exceed max(6 r, 5 r + 3) = {max(6 * r, 5 * r + 3)}")


def lex_median(values, info=None):
    """np.median of complex values: ordered by real part, then imaginary part; (a + b) / 2 of the two middle ones for an even
    count.  ``info`` receives the gap in real part between the median element(s) and the nearest elements of another value."""
    order = np.lexsort((values.imag, values.real))
    v = values[order]
    n = len(v)
    lo, hi = (n - 1) // 2, n // 2
    if info is not None:
        below = v.real[:lo][v[:lo] != v[lo]]
        above = v.real[hi + 1:][v[hi + 1:] != v[hi]]
        gaps = ([v.real[lo] - below[-1]] if len(below) else []) + ([above[0] - v.real[hi]] if len(above) else [])
        info["gap"] = min(gaps) if gaps else np.inf
    if lo == hi:
        return v[lo]
    return complex((v[lo].real + v[hi].real) / 2, (v[lo].imag + v[hi].imag) / 2)


def notch_spec(f_shifted, spacing=48, r=5, sn=9, trace=None):
    """The reference's sequential in-place loop on a shifted (H, W) complex128 spectrum; returns the new spectrum.  ``trace``
    (a list) receives one dict per assignment: call, centre (x, y), n (points read), full (points of the unclipped disc),
    written, median, gap."""
    f = np.array(f_shifted, dtype=np.complex128)
    H, W = f.shape
    for c, (uk, vk, r1, r2) in enumerate(notch_schedule(spacing, r, sn)):
        for cx, cy in ((W // 2 + uk, H // 2 + vk), (W // 2 + uk, H // 2 - vk), (W // 2 - uk, H // 2 + vk), (W // 2 - uk, H // 2 - vk)):
            y0, y1, x0, x1 = max(0, cy - r2), min(H, cy + r2 + 1), max(0, cx - r2), min(W, cx + r2 + 1)
            if y0 >= y1 or x0 >= x1:
                n, written = 0, 0
            else:
                d2 = (np.arange(x0, x1)[None, :] - cx) ** 2 + (np.arange(y0, y1)[:, None] - cy) ** 2
                window = f[y0:y1, x0:x1]        # a view: the assignment below is in place
                read = d2 <= r2 * r2
                n = int(read.sum())
                written = int((d2 <= r1 * r1).sum())
            info = {}
            if n:
                med = lex_median(window[read], info)
                window[d2 <= r1 * r1] = med
            if trace is not None:
                rr = np.arange(-r2, r2 + 1)
                full = int(((rr[None, :] ** 2 + rr[:, None] ** 2) <= r2 * r2).sum())
                trace.append(dict(call=c, centre=(cx, cy), n=n, full=full, written=written, median=med if n else None,
                                  gap=info.get("gap", np.inf)))
    return f


def denoise_stages(plane, spacing=48, r=5, sn=9, equalize=True, tables=None):
    """The chain on one (H, W) uint8 plane; returns dict(equalized, spectrum (shifted), filtered (shifted), out float64)."""
    from oracle import frontend_oracle as F
    plane = np.ascontiguousarray(plane, dtype=np.uint8)
    H, W = plane.shape
    th, tw = tables if tables is not None else (twiddles(H), twiddles(W))
    eq = F.equalize_hist_channel(plane) if equalize else plane
    spec = fft2_spec(eq.astype(np.float64), th, tw)
    iy, ix = shift_index(H), shift_index(W)
    shifted = spec[np.ix_(iy, ix)]
    filtered = notch_spec(shifted, spacing, r, sn)
    plain = np.empty_like(filtered)
    plain[np.ix_(iy, ix)] = filtered
    re, im = fft2_parts(plain, th, tw, inverse=True)
    return dict(equalized=eq, spectrum=shifted, filtered=filtered, out=np.sqrt(re * re + im * im))


def to_uint8(x):
    return np.minimum(255.0, np.floor(x + 0.5)).astype(np.uint8)


def denoise_spec(img, spacing=48, r=5, sn=9, equalize=True, out="float64"):
    """``notch_denoise`` of an (H, W) or (H, W, C) uint8 picture, channel by channel."""
    img = np.asarray(img, dtype=np.uint8)
    planes = img[..., None] if img.ndim == 2 else img
    H, W = planes.shape[:2]
    tables = (twiddles(H), twiddles(W))
    res = np.stack([denoise_stages(planes[..., c], spacing, r, sn, equalize, tables)["out"] for c in range(planes.shape[-1])], axis=-1)
    res = res[..., 0] if img.ndim == 2 else res
    return to_uint8(res) if out == "uint8" else res
