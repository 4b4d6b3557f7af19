"""Notch denoising of periodic noise on the GPU: the reference's pyviz/median_filter.py as a library module.

The dataset's pictures carry sine-like noise, and the per-channel equalisation in front of every stage amplifies it; a
detector that reads the pixels sees a field of corners.  ``notch_denoise`` equalises, transforms, replaces small discs
around the noise lattice's harmonics by the median of a larger disc, inverts and takes the magnitude - all channels and
pictures of a call in one fixed set of kernel launches (csrc/apap_denoise.hip).  No torch, no OpenCV, no CPU fallback.
"""
import numpy as np

from . import _native

__all__ = ["apply_median_filter", "notch_denoise", "notch_denoise_batch", "fft2", "notch_spectrum", "notch_schedule"]


def notch_arguments(spacing, r, sn, who):
    """The notch's parameter rules, checked before the library is touched (the library checks them again)."""
    spacing, r, sn = int(spacing), int(r), int(sn)
    if not 1 <= r <= _native.NOTCH_MAX_R:
        raise ValueError(f"{who}: r={r} (1 .. {_native.NOTCH_MAX_R})")
    if not 2 <= sn <= _native.FFT_MAX_LENGTH:      # beyond a plane's longest side no harmonic lies on it
        raise ValueError(f"{who}: sn={sn} (2 .. {_native.FFT_MAX_LENGTH})")
    bound = max(6 * r, 5 * r + 3)
    if spacing <= bound:
        raise ValueError(f"{who}: spacing={spacing} must exceed max(6 r, 5 r + 3) = {bound}, or a write disc meets another "
                         "centre's read disc")
    return spacing, r, sn


def notch_schedule(spacing=48, r=5, sn=9):
    """The calls of median_filter.py:149-155 in order, each ``(uk, vk, r1, r2)``: the four centres of a call are
    ``(w // 2 +- uk, h // 2 +- vk)``, the disc of radius r1 around each is set to the median of the disc of radius r2."""
    spacing, r, sn = notch_arguments(spacing, r, sn, "notch_schedule")
    calls = []
    for i in range(2, sn):
        calls.append((i * spacing, i * spacing, r, 5 * r))
        for j in range(1, i):
            calls.append((j * spacing, i * spacing, r, 5 * r))
            calls.append((i * spacing, j * spacing, r, 5 * r))
        calls.append((0, i * spacing, 3, 3 * r))
        calls.append((i * spacing, 0, 3, 3 * r))
    return calls


def fft2(x, inverse=False, device=-1, ctx=None):
    """The engine's 2-D transform of (h, w) or (planes, h, w) complex planes in complex128; 5-smooth lengths 2 .. 4096."""
    return _native.fft2(x, inverse=inverse, device=device, ctx=ctx)


def notch_spectrum(f, *, spacing=48, r=5, sn=9, device=-1, ctx=None):
    """The notch schedule on shifted spectra (``np.fft.fftshift``'s layout), (h, w) or (planes, h, w); returns new arrays."""
    spacing, r, sn = notch_arguments(spacing, r, sn, "notch_spectrum")
    return _native.notch_spectrum(f, spacing, r, sn, device=device, ctx=ctx)


def notch_denoise_batch(images, *, spacing=48, r=5, sn=9, equalize=True, out="float64", device=-1, ctx=None):
    """``notch_denoise`` of pictures of one shape, (n, h, w) or (n, h, w, c) uint8 (or a sequence of such pictures), in one
    call; returns an array of that shape.  The transform and the notch of all pictures and channels share their launches;
    the equalisation's tables are one picture's, so its three launches repeat per picture."""
    spacing, r, sn = notch_arguments(spacing, r, sn, "notch_denoise")
    a = np.ascontiguousarray(np.stack([np.asarray(m) for m in images]) if not isinstance(images, np.ndarray) else images)
    if a.dtype != np.uint8 or a.ndim not in (3, 4):
        raise ValueError(f"notch_denoise: uint8 pictures of one shape, (n, h, w) or (n, h, w, c), expected; got {a.dtype} {a.shape}")
    res = _native.notch_denoise(a[..., None] if a.ndim == 3 else a, spacing, r, sn, equalize=equalize, out=out, device=device, ctx=ctx)
    return res[..., 0] if a.ndim == 3 else res


def notch_denoise(img, *, spacing=48, r=5, sn=9, equalize=True, out="float64", device=-1, ctx=None):
    """The denoised (h, w) or (h, w, c) uint8 picture, c <= 4, every channel in one call.  ``out``: "float64" (the reference's
    ``img_new``) or "uint8" (``min(255, floor(x + 0.5))``, what the corner detector reads).  ``spacing`` is the noise
    lattice's period in the spectrum, ``r`` the notch radius, ``sn`` one more than the harmonics treated."""
    a = np.asarray(img)
    if a.dtype != np.uint8 or a.ndim not in (2, 3):
        raise ValueError(f"notch_denoise: an (h, w) or (h, w, c) uint8 picture expected; got {a.dtype} {a.shape}")
    return notch_denoise_batch(a[None], spacing=spacing, r=r, sn=sn, equalize=equalize, out=out, device=device, ctx=ctx)[0]


def spectrum_log(f):
    """``np.log(1 + |f|)`` as the reference spells it (median_filter.py:91-95, :141)."""
    return np.log(1 + np.sqrt(np.power(f.real, 2) + np.power(f.imag, 2)))


def apply_median_filter(img_ori: np.ndarray):
    """The reference's ``apply_median_filter`` of one uint8 plane: ``(img_new, spectrum_log, spectrum_filter_log, img_ori)`` -
    the denoised plane (float64), the log-spectra before and after the notch (computed on the host from the spectra the
    engine returns) and the equalised plane."""
    a = np.asarray(img_ori)
    if a.dtype != np.uint8 or a.ndim != 2:
        raise ValueError(f"apply_median_filter: an (h, w) uint8 plane expected; got {a.dtype} {a.shape}")
    eq = _native.equalize_hist(a)
    fshift = np.fft.fftshift(fft2(eq.astype(np.float64)))
    f1shift = notch_spectrum(fshift)
    img_new = notch_denoise(eq, equalize=False)
    return img_new, spectrum_log(fshift), spectrum_log(f1shift), eq
