"""The dark-channel dehazing in numpy, stage by stage: the definition that csrc/apap_dehaze.hip equals byte for byte.

He, Sun, Tang: the dark channel prior (CVPR 2009) with the guided filter (ECCV 2010) as the transmission's refinement, in
exact integers.  A picture is uint8, (h, w, 3) in BGR order or (h, w); every window is (2 r + 1)^2 with the border replicated;
every ``//`` is a floor division.  Every int64 intermediate is asserted below 2^62.
"""
import numpy as np

MAX_RADIUS, MAX_REFINE = 32, 32
ONE = 4096              # 12 fractional bits
LIMIT = 1 << 62


def arguments(radius=7, omega=0.95, t0=0.1, refine=30, eps=64):
    """The parameter rules; returns the integer forms ``(radius, omega_q, t0_q, refine, eps)``."""
    radius, refine, eps = int(radius), int(refine), int(eps)
    if not 0 <= radius <= MAX_RADIUS:
        raise ValueError(f"radius={radius} (0 .. {MAX_RADIUS})")
    if not 0 <= refine <= MAX_REFINE:
        raise ValueError(f"refine={refine} (0 .. {MAX_REFINE})")
    if not 1 <= eps <= 65535:
        raise ValueError(f"eps={eps} (1 .. 65535)")
    if not 0.0 <= float(omega) <= 1.0:
        raise ValueError(f"omega={omega} (0 .. 1)")
    if not 0.0 <= float(t0) <= 1.0:
        raise ValueError(f"t0={t0} (0 .. 1)")
    return radius, int(np.rint(256 * float(omega))), max(1, int(np.rint(ONE * float(t0)))), refine, eps


def planes(img):
    """The picture as (h, w, c) with c = 1 or 3."""
    a = np.asarray(img)
    if a.dtype != np.uint8 or a.ndim not in (2, 3) or a.size == 0 or (a.ndim == 3 and a.shape[2] != 3):
        raise ValueError(f"an (h, w) or (h, w, 3) uint8 picture expected; got {a.dtype} {a.shape}")
    return a[..., None] if a.ndim == 2 else a


def bounded(x):
    assert np.abs(x).max(initial=0) < LIMIT, "an intermediate reached 2^62"
    return x


def window_min(a, r):
    """The minimum over the (2 r + 1)^2 window, border replicated (for a minimum: the clipped window)."""
    out = a
    for axis in (0, 1):
        pad = [(r, r) if k == axis else (0, 0) for k in range(2)]
        p = np.pad(out, pad, mode="edge")
        n = out.shape[axis]
        out = np.minimum.reduce([np.take(p, np.arange(d, d + n), axis=axis) for d in range(2 * r + 1)])
    return out


def box_sum(a, r):
    """The int64 sum over the (2 r + 1)^2 window, border replicated: the count is (2 r + 1)^2 everywhere."""
    out = np.asarray(a, dtype=np.int64)
    for axis in (0, 1):
        pad = [(r + 1, r) if k == axis else (0, 0) for k in range(2)]
        c = np.cumsum(np.pad(out, pad, mode="edge"), axis=axis, dtype=np.int64)
        n = out.shape[axis]
        out = np.take(c, np.arange(2 * r + 1, 2 * r + 1 + n), axis=axis) - np.take(c, np.arange(0, n), axis=axis)
    return out


def grey(img):
    """``grey_at`` of csrc/apap_image_dev.h: the guide."""
    a = planes(img).astype(np.int64)
    if a.shape[2] == 1:
        return a[..., 0]
    return (3735 * a[..., 0] + 19235 * a[..., 1] + 9798 * a[..., 2] + 16384) >> 15


def dark_channel(img, radius=7):
    """D: the window minimum of the channel minimum, uint8."""
    return window_min(planes(img).min(axis=2), radius)


def airlight_threshold(D):
    """``(k, T)``: T the largest level v with at least k = max(1, N // 1000) pixels of D >= v."""
    k = max(1, D.size // 1000)
    at_least = np.cumsum(np.bincount(D.ravel(), minlength=256)[::-1])[::-1]     # at_least[v] = #{D >= v}
    return k, int(np.nonzero(at_least >= k)[0].max())


def atmospheric_light(img, radius=7):
    """A, uint8 per channel: among ALL pixels with D >= T the one with the largest channel sum, the lowest flat index among
    equals; every channel raised to at least 1."""
    a = planes(img)
    D = dark_channel(img, radius)
    _, T = airlight_threshold(D)
    flat = a.reshape(-1, a.shape[2])
    sums = flat.astype(np.int64).sum(axis=1)
    sums[D.ravel() < T] = -1
    return np.maximum(flat[int(np.argmax(sums))], 1).astype(np.uint8)           # argmax: the first of equals


def normalised_min(img, A):
    """n = min(4096, min_c (4096 I_c) // A_c)."""
    a = planes(img).astype(np.int64)
    return np.minimum(ONE, ((ONE * a) // A.astype(np.int64)).min(axis=2))


def raw_transmission(img, A, radius=7, omega_q=243):
    """p = 4096 - ((omega_q Dn + 128) >> 8), Dn the window minimum of n; in 0 .. 4096."""
    Dn = window_min(normalised_min(img, A), radius)
    return ONE - ((omega_q * Dn + 128) >> 8)


def guided_terms(G, p, rho, eps):
    """The guided filter's intermediates for rho > 0: ``dict(covN, varN, den, a_q, b_q, num)``, all int64."""
    G, p = G.astype(np.int64), p.astype(np.int64)
    W = (2 * rho + 1) ** 2
    sG, sp, sGp, sGG = box_sum(G, rho), box_sum(p, rho), box_sum(G * p, rho), box_sum(G * G, rho)
    covN = bounded(bounded(W * sGp) - bounded(sG * sp))
    varN = bounded(bounded(W * sGG) - sG * sG)
    assert varN.min() >= 0
    den = bounded(varN + eps * W * W)
    a_q = bounded(ONE * covN) // den
    assert np.abs(a_q).max() < 1 << 23
    b_q = bounded(bounded(ONE * sp) - bounded(a_q * sG))
    num = bounded(bounded(box_sum(a_q, rho) * G * W) + bounded(box_sum(b_q, rho)))
    return dict(covN=covN, varN=varN, den=den, a_q=a_q, b_q=b_q, num=num)


def guided(G, p, rho, eps):
    """The guided filter's output, int64, before the clip."""
    if rho == 0:
        return p.astype(np.int64)
    W = (2 * rho + 1) ** 2
    return guided_terms(G, p, rho, eps)["num"] // (ONE * W * W)


def transmission_q(img, radius=7, omega_q=243, t0_q=410, refine=30, eps=64, A=None):
    """t as uint16, 12 fractional bits, clipped to t0_q .. 4096."""
    if A is None:
        A = atmospheric_light(img, radius)
    p = raw_transmission(img, A, radius, omega_q)
    return np.clip(guided(grey(img), p, refine, eps), t0_q, ONE).astype(np.uint16)


def recover_terms(img, A, t):
    """``(numerator, denominator)`` of the recovery's division, int64 (h, w, c) and (h, w, 1)."""
    a = planes(img).astype(np.int64)
    t = t.astype(np.int64)[..., None]
    return 2 * ONE * (a - A.astype(np.int64)) + t, 2 * t


def recover(img, A, t):
    """J_c = clip(A_c + (8192 (I_c - A_c) + t) // (2 t), 0, 255): round-half-up of A + (I - A) / t."""
    num, den = recover_terms(img, A, t)
    J = np.clip(A.astype(np.int64) + num // den, 0, 255).astype(np.uint8)
    return J.reshape(np.asarray(img).shape)


def dehaze_q(img, radius=7, omega_q=243, t0_q=410, refine=30, eps=64):
    """``(J, t, A)`` from the integer parameters."""
    A = atmospheric_light(img, radius)
    t = transmission_q(img, radius, omega_q, t0_q, refine, eps, A=A)
    return recover(img, A, t), t, A


def transmission(img, radius=7, omega=0.95, t0=0.1, refine=30, eps=64):
    radius, omega_q, t0_q, refine, eps = arguments(radius, omega, t0, refine, eps)
    return transmission_q(img, radius, omega_q, t0_q, refine, eps)


def dehaze(img, radius=7, omega=0.95, t0=0.1, refine=30, eps=64):
    radius, omega_q, t0_q, refine, eps = arguments(radius, omega, t0, refine, eps)
    return dehaze_q(img, radius, omega_q, t0_q, refine, eps)
