"""Inputs of the notch denoising's tests: seeded spectra and pictures made by integer hashing (the same on every numpy), and
the cases of the notch step that tests/golden/denoise_notch_ref.npz pins against the reference's own median_filter."""
import numpy as np

MASK = (1 << 64) - 1


def _mix(x):
    """splitmix64's finaliser on a uint64 array."""
    x = (x + np.uint64(0x9E3779B97F4A7C15))
    x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def _words(count, seed, stream):
    with np.errstate(over="ignore"):
        k = np.arange(count, dtype=np.uint64) * np.uint64(3) + np.uint64(stream)
        return _mix(_mix(k + np.uint64(seed) * np.uint64(0x632BE59BD9B4E019)))


def spectrum(h, w, seed, levels=0):
    """A complex128 (h, w) array.  Parts uniform in (-1000, 1000) on a 2^-32 grid; with ``levels`` the real part takes only
    that many values, so that many elements of a disc tie in it and the imaginary part decides their order."""
    re = (_words(h * w, seed, 0) >> np.uint64(21)).astype(np.float64) * (2000.0 / 2 ** 43) - 1000.0
    im = (_words(h * w, seed, 1) >> np.uint64(21)).astype(np.float64) * (2000.0 / 2 ** 43) - 1000.0
    if levels:
        re = (_words(h * w, seed, 2) % np.uint64(levels)).astype(np.float64) - levels // 2
    return (re + 1j * im).reshape(h, w)


def picture(h, w, seed, channels=0):
    """A uint8 picture of random bytes, (h, w) or (h, w, channels)."""
    c = max(channels, 1)
    a = (_words(h * w * c, seed, 5) >> np.uint64(56)).astype(np.uint8).reshape(h, w, c)
    return a if channels else a[..., 0]


# name: (h, w, spacing, r, sn, seed, levels)
NOTCH_CASES = {
    "boundary_120x144": (120, 144, 9, 1, 9, 11, 0),       # 72 - 8 * 9 = 0: centres exactly on the first column
    "empty_90x100": (90, 100, 14, 2, 9, 12, 16),          # most of the lattice lies off the plane
    "mid_150x160": (150, 160, 14, 2, 9, 13, 16),
    "odd_27x25": (27, 25, 9, 1, 3, 14, 4),
    "odd_75x81": (75, 81, 9, 1, 5, 16, 8),                # odd sides with even counts and live coincident pairs
    "default_768x768": (768, 768, 48, 5, 9, 15, 0),
}
SMALL_CASES = [k for k in NOTCH_CASES if not k.startswith("default")]


def notch_input(name):
    h, w, _, _, _, seed, levels = NOTCH_CASES[name]
    return spectrum(h, w, seed, levels)


def notch_params(name):
    _, _, spacing, r, sn, _, _ = NOTCH_CASES[name]
    return dict(spacing=spacing, r=r, sn=sn)
