"""tests/denoise_spec.py, the numpy definition the notch-denoising kernels are held to, against what it restates: the
reference's own median_filter (tests/golden/denoise_notch_ref.npz, made by tests/golden/make_denoise_golden.py), a direct DFT
in extended precision, and the chain written with np.fft in complex128.  No GPU."""
import hashlib

import numpy as np
import pytest

import denoise_cases as C
import denoise_spec as S


@pytest.fixture(scope="module")
def traces():
    """name -> (result of notch_spec, its trace), computed once."""
    out = {}
    for name in C.NOTCH_CASES:
        trace = []
        out[name] = (S.notch_spec(C.notch_input(name), trace=trace, **C.notch_params(name)), trace)
    return out


@pytest.mark.parametrize("name", list(C.NOTCH_CASES))
def test_notch_step_equals_the_reference(name, traces, golden, native):
    ref = golden("denoise_notch_ref")
    got, trace = traces[name]
    if name in C.SMALL_CASES:
        want = C.notch_input(name).ravel()
        want[ref[f"{name}_at"]] = ref[f"{name}_values"]
        assert np.array_equal(got.ravel(), want)
    else:
        assert hashlib.sha256(np.ascontiguousarray(got).tobytes()).digest() == ref[f"{name}_sha256"].tobytes()
        assert np.array_equal(np.array([t["median"] for t in trace if t["n"]]), ref[f"{name}_medians"])


@pytest.mark.parametrize("name", list(C.NOTCH_CASES))
def test_notch_cases_reach_what_they_are_for(name, traces):
    """Odd and even counts, clipped discs, coincident pairs; empty discs at 90 x 100.  27 x 25 with sn = 3 cannot hold all of
    them under the engine's rule spacing > max(6 r, 5 r + 3) >= 8: the only harmonic, 2 * spacing >= 18, lies beyond both
    half-sides (13, 12), so its discs are empty or clipped to single points on the border (odd counts; the axis calls'
    coincident pairs are empty).  That case keeps the odd sizes, the clipping and the empty discs."""
    _, trace = traces[name]
    full = [t for t in trace if t["n"]]
    pairs = {}
    for t in trace:
        pairs.setdefault((t["call"], t["centre"]), []).append(t["n"])
    coincident = [v for v in pairs.values() if len(v) == 2]
    assert coincident and all(v[0] == v[1] for v in coincident)
    assert any(t["n"] % 2 == 1 for t in full) and any(0 < t["n"] < t["full"] for t in trace)
    if name == "odd_27x25":
        assert any(t["n"] == 0 for t in trace)
        return
    assert any(t["n"] % 2 == 0 for t in full) and any(v[0] > 0 for v in coincident)
    assert any(t["written"] < t["n"] for t in full)
    if name == "empty_90x100":
        assert sum(t["n"] == 0 for t in trace) > len(trace) // 2
    if name == "boundary_120x144":
        assert any(t["centre"][0] == 0 for t in full) and any(t["centre"][0] == 144 for t in full)
    if name == "default_768x768":
        assert len(trace) == 4 * 77 and max(t["n"] for t in trace) == 1961 and (C.notch_params(name) == dict(spacing=48, r=5, sn=9))
    if name == "maxr_216x225":
        # the largest read disc the kernel is sized for (kNotchMaxPts = 2821, sorted as 4096 = kNotchSortPts), whole; and the
        # axis calls' disc of radius 3 r = 18, whole
        assert C.notch_params(name)["r"] == S.MAX_R == 6 and not any(t["n"] == 0 for t in trace)
        assert {t["full"] for t in trace} == {2821, 1009} and 2048 < 2821 <= 4096
        assert any(t["n"] == t["full"] == 2821 for t in trace) and any(t["n"] == t["full"] == 1009 for t in trace)
    if name == "beyond_reach_27x400":
        # the launch keeps the terms i < min(sn, reach), reach = (max(h, w) + 5 r) / spacing + 2 (csrc/apap_denoise.hip,
        # launch_notch): here reach < sn, no dropped term assigns anything, and the last term that does lies beyond what
        # the shorter side alone would keep - and beyond i = 8, the most any other case decodes a block index into
        h, w, p = *C.notch_input(name).shape, C.notch_params(name)
        reach = (max(h, w) + 5 * p["r"]) // p["spacing"] + 2
        term = [max(uk, vk) // p["spacing"] for uk, vk, _, _ in S.notch_schedule(**p)]
        last = max(term[t["call"]] for t in full)
        assert reach == 47 < p["sn"] == 64 and last == 22 < reach
        assert last > (min(h, w) // 2 + 5 * p["r"]) // p["spacing"] and last > (min(h, w) + 5 * p["r"]) // p["spacing"] + 1 and last > 8
        assert len(trace) == 16368 and len(full) == 256


def test_schedule_counts(golden):
    assert len(S.notch_schedule()) == 77
    # what the reference's own apply_median_filter handed to its median_filter, recorded by the generator
    assert golden("denoise_notch_ref")["schedule_default"].tolist() == [list(c) for c in S.notch_schedule(48, 5, 9)]
    assert len(S.notch_schedule(9, 1, 3)) == 5
    assert S.notch_schedule(48, 5, 9)[:4] == [(96, 96, 5, 25), (48, 96, 5, 25), (96, 48, 5, 25), (0, 96, 3, 15)]


def long_dft2(x, rows=None, cols=None):
    """The direct DFT of ``x`` in np.longdouble: all of it, or the outputs [rows][:, cols] alone."""
    def matrix(n, keep):
        k = np.arange(n, dtype=np.longdouble)
        out = k if keep is None else np.asarray(keep).astype(np.longdouble)
        a = -2 * np.arccos(np.longdouble(-1)) * ((out[:, None] * k[None, :]) % n) / n
        return np.cos(a) + 1j * np.sin(a)
    return matrix(x.shape[0], rows) @ x.astype(np.clongdouble) @ matrix(x.shape[1], cols).T


def sampled_outputs(n, count=64):
    """``count`` distinct output indices of a length ``n``: both ends, the middle and its neighbours, and hashed ones."""
    fixed = [0, 1, 2, n // 2 - 1, n // 2, n // 2 + 1, n - 2, n - 1]
    hashed = [int(v) for v in C._words(4 * count, seed=n, stream=7) % np.uint64(n)]
    return np.array(list(dict.fromkeys(fixed + hashed))[:count])


# the longest lengths with the most radix-3 and radix-5 stages (4050 = 2 3^4 5^2, 4000 = 2^5 5^3, 3888 = 2^4 3^5, 3750 = 2 3 5^4)
# and 4096 = 4^6, as rows and as columns: the lengths at which the kernels are held to fft2_spec and to nothing else
LONG_SHAPES = [(2, 4050), (4050, 2), (4000, 2), (3, 3888), (2, 4096), (5, 3750)]


@pytest.mark.parametrize("shape", [(27, 25), (30, 32), (45, 64)] + LONG_SHAPES)
def test_transform_accuracy(shape, native):
    """fft2_spec's maximum error against a direct DFT in np.longdouble is at most 4 x np.fft.fft2's (complex128 input) at the
    same shape: the margin allows for another factorisation order and the radix-5 constants.  At the long shapes the DFT is
    evaluated at 64 output indices along the long axis (all along the short one) and both errors are taken at those outputs: the
    whole matrix of 4050 points is half a gigabyte.  Measured, fft2_spec / np.fft.fft2 on parts uniform in
    (-1000, 1000): 27 x 25 1.38e-11 / 1.60e-11, 30 x 32 1.27e-11 / 1.35e-11, 45 x 64 3.45e-11 / 3.39e-11; the long shapes'
    figures stand in DESIGN.md."""
    assert np.finfo(np.longdouble).eps < 2e-19
    x = C.spectrum(*shape, seed=31)
    if shape in LONG_SHAPES:
        rows, cols = (sampled_outputs(n) if n > 64 else np.arange(n) for n in shape)
        assert sorted((len(set(rows.tolist())), len(set(cols.tolist())))) == [min(shape), 64]      # distinct outputs
        at = np.ix_(rows, cols)
        truth = long_dft2(x, rows, cols)
    else:
        at = np.ix_(*(np.arange(n) for n in shape))
        truth = long_dft2(x)
    ours = np.abs(S.fft2_spec(x)[at] - truth).max()
    numpys = np.abs(np.fft.fft2(x)[at] - truth).max()
    print(f"{shape}: fft2_spec {float(ours):.3e}, np.fft.fft2 {float(numpys):.3e}")
    assert ours <= 4 * numpys
    back = S.fft2_spec(S.fft2_spec(x), inverse=True)
    assert np.abs(back - x).max() <= 64 * np.finfo(np.float64).eps * np.abs(x).max()


@pytest.mark.parametrize("n", [2, 3, 5, 27, 125, 768, 3840, 4050, 4096])
def test_twiddle_table(n, native):
    t = native.fft_twiddles(n)
    k = np.arange(n, dtype=np.longdouble)
    a = -2 * np.arccos(np.longdouble(-1)) * k / n
    assert np.abs(t[:, 0] - np.cos(a)).max() <= 2.0 ** -52 and np.abs(t[:, 1] - np.sin(a)).max() <= 2.0 ** -52
    assert t[0, 0] == 1.0 and t[0, 1] == 0.0 and not np.signbit(t[0, 1])


def numpy_chain(eq, spacing, r, sn):
    """The chain restated with np.fft in complex128."""
    f = np.fft.fftshift(np.fft.fft2(eq.astype(np.float64)))
    g = S.notch_spec(f, spacing, r, sn)
    return f, g, np.abs(np.fft.ifft2(np.fft.ifftshift(g)))


@pytest.mark.parametrize("h,w,spacing,r,seed", [(120, 144, 9, 1, 42), (768, 768, 48, 5, 42)])
def test_whole_chain_against_numpy_fft(h, w, spacing, r, seed, native):
    """denoise_spec against the same chain on np.fft.  First the input condition: in every disc the gap in real part between
    the median element(s) and their nearest neighbours of another value is at least 1e6 x the largest difference between the
    two transforms - then no disc can select differently.  Then the pixel difference, bounded by 10 x the difference of the two
    inverse transforms on the same filtered spectrum.  The spectrum of a real picture is Hermitian, so a disc that
    straddles the Nyquist column or row holds pairs whose real parts agree to rounding; where such a pair sits at the median the
    condition fails (seeds 41, 43, 44 at 120 x 144; 43 at 768 x 768), hence the seeds.  Measured: 120 x 144
    transforms 1.27e-11 apart, smallest gap 1.09, pixels 2.3e-13 apart against 1.9e-13 of the inverses; 768 x 768 9.0e-11, 0.48,
    2.6e-13 against 2.3e-13."""
    pic = C.picture(h, w, seed)
    st = S.denoise_stages(pic, spacing, r, 9)
    f, g, out = numpy_chain(st["equalized"], spacing, r, 9)
    apart = np.abs(st["spectrum"] - f).max()
    trace = []
    S.notch_spec(st["spectrum"], spacing, r, 9, trace=trace)
    gap = min(t["gap"] for t in trace if t["n"])
    assert gap >= 1e6 * apart, (gap, apart)
    th, tw = S.twiddles(h), S.twiddles(w)
    plain = np.fft.ifftshift(st["filtered"])
    inverses = np.abs(S.fft2_spec(plain, th, tw, inverse=True) - np.fft.ifft2(plain)).max()
    pixels = np.abs(st["out"] - out).max()
    print(f"{h} x {w}: transforms {apart:.3e} apart, smallest gap {gap:.3e}, pixels {pixels:.3e} apart, inverses {inverses:.3e}")
    assert np.array_equal(np.fft.ifftshift(np.fft.fftshift(st["filtered"])), st["filtered"])
    assert pixels <= 10 * inverses
    assert np.array_equal(S.to_uint8(st["out"]), S.denoise_spec(pic, spacing, r, 9, out="uint8"))


def test_transform_shapes_reach_what_they_are_listed_for():
    """The kernels' constants (csrc/apap_denoise.hip), restated: a column strip holds min(kFftMaxStrip = 16, columns,
    kFftLdsPoints = 4096 // rows) columns, a block has 1024 threads from 2048 points on, columns of more than 1024 points take
    the turned path instead."""
    strip = lambda h, w: max(1, min(16, w, 4096 // h))      # noqa: E731
    for (h, w), widths in C.FFT_STRIP_SHAPES.items():
        s = strip(h, w)
        assert h <= 1024 and S.five_smooth(h) and S.five_smooth(w)
        assert [min(s, w - c) for c in range(0, w, s)] == widths and s & (s - 1) != 0 and s == 4096 // h
    assert {w[0] for w in C.FFT_STRIP_SHAPES.values()} == {13, 7, 5}
    h, w = C.FFT_THRESHOLD_SHAPE
    assert strip(h, w) == 16 and strip(h, w) * h == 2048 and w % 16 == 0
    stages = {}
    for shape, radices in C.FFT_LONG_SHAPES.items():
        n, rem, order = max(shape), max(shape), []
        while rem > 1:
            order.append(S.radix(rem))
            rem //= order[-1]
        assert order == radices and 3750 <= n <= S.MAX_LENGTH and S.five_smooth(min(shape)) and shape in LONG_SHAPES
        stages[n] = (order.count(3), order.count(5))
    # stages of radix 3 and of radix 5 behind the even ones: five and none, none and three, four and two, one and four
    assert stages == {3888: (5, 0), 4000: (0, 3), 4050: (4, 2), 3750: (1, 4)}
    # no longer even length has as many stages of 3 and 5 together as 4050, which runs as a row and as a (turned) column
    count = lambda n, p: max(k for k in range(13) if n % p ** k == 0)      # noqa: E731
    assert all(count(n, 3) + count(n, 5) < 6 for n in range(4052, S.MAX_LENGTH + 1, 2) if S.five_smooth(n))
    assert {(4050, 2), (2, 4050)} <= set(C.FFT_LONG_SHAPES)


def chain_trace(h, w, channels, spacing, r, sn, equalize, seed):
    """The notch's trace on the spectrum of the whole chain's first plane."""
    pic = C.picture(h, w, seed=seed, channels=channels)
    st = S.denoise_stages(pic[..., 0] if channels else pic, spacing, r, sn, equalize)
    trace = []
    S.notch_spec(st["spectrum"], spacing, r, sn, trace=trace)
    return trace


def test_chain_cases_reach_what_they_are_for(native):
    """The whole-chain cases of tests/denoise_cases.py (the pictures tests/test_gpu_denoise.py makes: seed 70 + h)."""
    by_r_sn = {(c[4], c[5]): c for c in C.CHAIN_EDGE_CASES}
    case = by_r_sn[(6, 4)]
    trace = chain_trace(*case, seed=70 + case[0])
    assert case[4] == S.MAX_R and any(t["n"] == t["full"] == 2821 for t in trace) and any(t["n"] == t["full"] == 1009 for t in trace)
    assert all(S.five_smooth(n) for n in case[:2])
    case = by_r_sn[(1, 9)]
    h, w = case[:2]
    trace = chain_trace(*case, seed=70 + h)
    assert h > 1024 and h % 2 == 1 and w % 2 == 1 and S.five_smooth(h) and S.five_smooth(w)
    assert any(t["n"] for t in trace) and any(0 < t["n"] < t["full"] for t in trace) and any(t["written"] for t in trace)
    case = by_r_sn[(1, 3)]
    assert case[2] == 4                                      # apap_notch_denoise's most channels
    case = by_r_sn[(1, 30)]
    h, w, _, spacing, r, sn, _ = case
    reach = (max(h, w) + 5 * r) // spacing + 2
    trace = chain_trace(*case, seed=70 + h)
    term = [max(uk, vk) // spacing for uk, vk, _, _ in S.notch_schedule(spacing, r, sn)]
    assert reach == 18 < sn and max(term[t["call"]] for t in trace if t["n"]) < reach <= max(term)
    b = C.TALL_BATCH
    assert b["h"] > 1024 and b["count"] * b["channels"] == 4 and S.five_smooth(b["h"]) and S.five_smooth(b["w"])


@pytest.mark.parametrize("name", list(C.tie_pictures()))
@pytest.mark.parametrize("equalize", [True, False])
def test_tie_pictures_hold_discs_of_one_value(name, equalize, native):
    """Every read disc of the schedule, taken from the spectrum before the notch (no write disc meets another centre's read
    disc), holds one value, and several hold more than one point, an even and an odd count among them: whichever way a sort
    orders equal elements, the median is that value.  The constant comes back unchanged."""
    pic = C.tie_pictures()[name]
    p = C.TIE_PARAMS
    st = S.denoise_stages(pic, equalize=equalize, **p)
    f = st["spectrum"]
    H, W = f.shape
    sizes = set()
    for uk, vk, _, r2 in S.notch_schedule(**p):
        for cx, cy in ((W // 2 + uk, H // 2 + vk), (W // 2 + uk, H // 2 - vk), (W // 2 - uk, H // 2 + vk), (W // 2 - uk, H // 2 - vk)):
            ys, xs = np.mgrid[max(0, cy - r2):max(0, min(H, cy + r2 + 1)), max(0, cx - r2):max(0, min(W, cx + r2 + 1))]
            disc = f[ys, xs][(xs - cx) ** 2 + (ys - cy) ** 2 <= r2 * r2]
            assert (disc == disc[:1]).all()
            sizes.add(len(disc))
    assert any(n > 1 and n % 2 for n in sizes) and any(n > 1 and n % 2 == 0 for n in sizes)
    assert len(np.unique(pic)) == (1 if name.startswith("constant") else 2)
    if name.startswith("constant"):
        assert (st["out"] == 100.0).all() and (pic == 100).all()


def test_shift_is_index_arithmetic():
    for n in (2, 5, 8, 25, 27):
        x = np.arange(n)
        assert np.array_equal(x[S.shift_index(n)], np.fft.fftshift(x))
        back = np.empty(n, int)
        back[S.shift_index(n)] = np.fft.fftshift(x)
        assert np.array_equal(back, x)
        assert np.array_equal((np.arange(n) + n // 2) % n, np.argsort(S.shift_index(n)))
