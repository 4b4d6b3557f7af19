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


# name: (h, w, spacing, r, sn, seed, levels, how tests/golden/denoise_notch_ref.npz stores the reference's result: "points" -
# the positions it changed and their new values - or "digest" - the SHA-256 of the result and the medians of its discs)
NOTCH_CASES = {
    "boundary_120x144": (120, 144, 9, 1, 9, 11, 0, "points"),      # 72 - 8 * 9 = 0: centres exactly on the first column
    "empty_90x100": (90, 100, 14, 2, 9, 12, 16, "points"),         # most of the lattice lies off the plane
    "mid_150x160": (150, 160, 14, 2, 9, 13, 16, "points"),
    "odd_27x25": (27, 25, 9, 1, 3, 14, 4, "points"),
    "odd_75x81": (75, 81, 9, 1, 5, 16, 8, "points"),               # odd sides with even counts and live coincident pairs
    "default_768x768": (768, 768, 48, 5, 9, 15, 0, "digest"),
    # r = APAP_NOTCH_MAX_R: whole read discs of 2821 points (the kernel's kNotchMaxPts, sorted as 4096) and of 1009 (axis calls)
    "maxr_216x225": (216, 225, 37, 6, 4, 17, 8, "digest"),
    # sn beyond the terms the launch keeps (reach = 47, from the longer side); the notch step alone takes sides that are not 5-smooth
    "beyond_reach_27x400": (27, 400, 9, 1, 64, 18, 4, "points"),
}
SMALL_CASES = [k for k, case in NOTCH_CASES.items() if case[7] == "points"]


# Shapes of the transform at the kernels' edges (tests/test_denoise_spec.py asserts what each is listed for).
# (h, w): the widths of its column strips, min(16, w, 4096 // h) columns a block - none a power of two
FFT_STRIP_SHAPES = {(300, 27): [13, 13, 1], (540, 9): [7, 2], (768, 10): [5, 5]}
# a strip of 16 columns of 128 points: 2048 points a block, from where on a block has 1024 threads
FFT_THRESHOLD_SHAPE = (128, 32)
# (h, w): the radices of its longest side in the order of the stages - the lengths up to 4096 with the most stages of 3 and of 5
FFT_LONG_SHAPES = {(2, 4050): [2, 3, 3, 3, 3, 5, 5], (4050, 2): [2, 3, 3, 3, 3, 5, 5], (4000, 2): [4, 4, 2, 5, 5, 5],
                   (3, 3888): [4, 4, 3, 3, 3, 3, 3], (5, 3750): [2, 3, 5, 5, 5, 5]}

# Whole-chain cases at the notch's edges: h, w, channels, spacing, r, sn, equalize
CHAIN_EDGE_CASES = [(216, 225, 0, 37, 6, 4, True),      # r = 6: the largest disc, through the unshifted plane's index arithmetic
                    (1125, 45, 0, 9, 1, 9, True),       # tall and odd: the notch on the turned copy
                    (30, 32, 4, 9, 1, 3, True),         # four channels, the most a picture has
                    (120, 144, 0, 9, 1, 30, True)]      # sn beyond the 18 terms the launch keeps
TALL_BATCH = dict(count=2, h=1080, w=48, channels=2, spacing=14, r=2, sn=9)


def tie_pictures():
    """name -> a 30 x 32 uint8 picture whose spectrum is zero but for a few points, so that whole discs hold one value and the
    median's sort is all ties: a constant, and stripes two pixels wide (period 4: its only harmonics lie 8 columns from the
    centre, the discs of TIE_PARAMS 18 from it)."""
    return {"constant_30x32": np.full((30, 32), 100, np.uint8),
            "stripes_30x32": np.ascontiguousarray(np.broadcast_to(np.where((np.arange(32) // 2) % 2, 200, 50).astype(np.uint8), (30, 32)))}


TIE_PARAMS = dict(spacing=9, r=1, sn=3)


def notch_input(name):
    h, w, _, _, _, seed, levels, _ = NOTCH_CASES[name]
    return spectrum(h, w, seed, levels)


def notch_params(name):
    _, _, spacing, r, sn, _, _, _ = NOTCH_CASES[name]
    return dict(spacing=spacing, r=r, sn=sn)
