"""Single-picture dehazing on the GPU: the dark channel prior (He, Sun, Tang, CVPR 2009) with the guided filter (ECCV 2010) as
the refinement of the transmission.

The reference answers its haze with a per-channel equalisation in front of every stage.  ``dehaze`` estimates the atmospheric
light A and the transmission t of ``I = J t + A (1 - t)`` from one picture and returns J, a uint8 picture that the corner
detector, the descriptor and the panorama read as they read any other.  Everything is defined in exact integers (12 fractional
bits of t; include/apap_hip.h states the definition, tests/dehaze_spec.py restates it in numpy), all pictures of a call share one
fixed set of kernel launches (csrc/apap_dehaze.hip).  No torch, no OpenCV, no CPU fallback.
"""
import numpy as np

from . import _native

__all__ = ["dark_channel", "atmospheric_light", "transmission", "dehaze", "dehaze_batch", "dehaze_arguments"]


def dehaze_arguments(radius=7, omega=0.95, t0=0.1, refine=30, eps=64, who="dehaze"):
    """The parameter rules, checked before the library is touched (the library checks them again); returns the integer forms
    of the C ABI, ``(radius, omega_q, t0_q, refine, eps)`` with ``omega_q = rint(256 omega)`` and ``t0_q = max(1, rint(4096 t0))``."""
    radius, refine, eps = int(radius), int(refine), int(eps)
    if not 0 <= radius <= _native.DEHAZE_MAX_RADIUS:
        raise ValueError(f"{who}: radius={radius} (0 .. {_native.DEHAZE_MAX_RADIUS})")
    if not 0 <= refine <= _native.DEHAZE_MAX_RADIUS:
        raise ValueError(f"{who}: refine={refine} (0 .. {_native.DEHAZE_MAX_RADIUS})")
    if not 1 <= eps <= 65535:
        raise ValueError(f"{who}: eps={eps} (1 .. 65535, grey levels squared)")
    if not 0.0 <= float(omega) <= 1.0:          # a NaN fails both
        raise ValueError(f"{who}: omega={omega} (0 .. 1)")
    if not 0.0 <= float(t0) <= 1.0:
        raise ValueError(f"{who}: t0={t0} (0 .. 1)")
    return radius, int(np.rint(256 * float(omega))), max(1, int(np.rint(_native.DEHAZE_ONE * float(t0)))), refine, eps


def _one(img, who):
    """A picture as a batch of one, (1, h, w, c)."""
    a = np.asarray(img)
    if a.dtype != np.uint8 or a.ndim not in (2, 3) or a.size == 0 or (a.ndim == 3 and a.shape[2] != 3):
        raise ValueError(f"{who}: an (h, w) or (h, w, 3) uint8 picture expected; got {a.dtype} {a.shape}")
    return a[None, ..., None] if a.ndim == 2 else a[None]


def dark_channel(img, radius=7, *, device=-1, ctx=None):
    """The dark channel of an (h, w, 3) BGR or (h, w) uint8 picture: the minimum over the channels and over the
    ``(2 radius + 1)^2`` window; (h, w) uint8."""
    radius = dehaze_arguments(radius=radius, who="dark_channel")[0]
    return _native.dark_channel(_one(img, "dark_channel"), radius, device=device, ctx=ctx)[0]


def atmospheric_light(img, radius=7, *, device=-1, ctx=None):
    """The atmospheric light A, uint8 per channel: the brightest (largest channel sum) of the haziest pixels - every pixel whose
    dark channel reaches the level that the top 0.1 % reach; each channel at least 1."""
    radius = dehaze_arguments(radius=radius, who="atmospheric_light")[0]
    return _native.atmospheric_light(_one(img, "atmospheric_light"), radius, device=device, ctx=ctx)[0]


def transmission(img, radius=7, omega=0.95, t0=0.1, refine=30, eps=64, *, device=-1, ctx=None):
    """The transmission t as (h, w) uint16 with 12 fractional bits (4096 = 1.0), clipped to ``t0`` .. 1: ``1 - omega`` times the
    dark channel of ``I / A``, refined by a guided filter of radius ``refine`` under the picture's grey value (``refine=0``:
    as it is).  ``eps`` is the filter's regulariser in grey levels squared (64 is about 1e-3 on the unit scale)."""
    q = dehaze_arguments(radius, omega, t0, refine, eps, who="transmission")
    return _native.transmission(_one(img, "transmission"), *q, device=device, ctx=ctx)[0]


def dehaze_batch(images, radius=7, omega=0.95, t0=0.1, refine=30, eps=64, return_parts=False, *, device=-1, ctx=None):
    """``dehaze`` of pictures of one shape, (n, h, w) or (n, h, w, 3) uint8 (or a sequence of such pictures), in one call: an
    array of that shape, each picture byte-identical to its own call; with ``return_parts`` ``(J, t, A)`` with t (n, h, w)
    uint16 and A (n, channels) uint8."""
    q = dehaze_arguments(radius, omega, t0, refine, eps)
    a = np.ascontiguousarray(np.stack([np.asarray(m) for m in images]) if not isinstance(images, np.ndarray) else images)
    if a.dtype != np.uint8 or a.ndim not in (3, 4) or a.size == 0 or (a.ndim == 4 and a.shape[3] != 3):
        raise ValueError(f"dehaze: uint8 pictures of one shape, (n, h, w) or (n, h, w, 3), expected; got {a.dtype} {a.shape}")
    res = _native.dehaze(a[..., None] if a.ndim == 3 else a, *q, parts=return_parts, device=device, ctx=ctx)
    if not return_parts:
        return res[..., 0] if a.ndim == 3 else res
    J, t, A = res
    return (J[..., 0] if a.ndim == 3 else J), t, A


def dehaze(img, radius=7, omega=0.95, t0=0.1, refine=30, eps=64, return_parts=False, *, device=-1, ctx=None):
    """The dehazed picture, uint8 of the shape of ``img`` ((h, w, 3) BGR or (h, w)): ``A + (I - A) / t`` rounded half up and
    clipped; with ``return_parts`` ``(J, t, A)``."""
    _one(img, "dehaze")
    res = dehaze_batch(np.asarray(img)[None], radius, omega, t0, refine, eps, return_parts, device=device, ctx=ctx)
    return (res[0][0], res[1][0], res[2][0]) if return_parts else res[0]
