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


def test_schedule_counts(golden):
    assert len(S.notch_schedule()) == 77
    # what the reference's own apply_median_filter handed to its median_filter, recorded by the generator
    assert golden("denoise_notch_ref")["schedule_default"].tolist() == [list(c) for c in S.notch_schedule(48, 5, 9)]
    assert len(S.notch_schedule(9, 1, 3)) == 5
    assert S.notch_schedule(48, 5, 9)[:4] == [(96, 96, 5, 25), (48, 96, 5, 25), (96, 48, 5, 25), (0, 96, 3, 15)]


def long_dft2(x):
    def matrix(n):
        k = np.arange(n, dtype=np.longdouble)
        a = -2 * np.arccos(np.longdouble(-1)) * ((k[:, None] * k[None, :]) % n) / n
        return np.cos(a) + 1j * np.sin(a)
    return matrix(x.shape[0]) @ x.astype(np.clongdouble) @ matrix(x.shape[1])


@pytest.mark.parametrize("shape", [(27, 25), (30, 32), (45, 64)])
def test_transform_accuracy(shape, native):
    """fft2_spec's maximum error against a direct DFT in np.longdouble is at most 4 x np.fft.fft2's (complex128 input) at the
    same shape: the margin allows for another factorisation order and the radix-5 constants.  Measured, fft2_spec /
    np.fft.fft2 on parts uniform in (-1000, 1000): 27 x 25 1.38e-11 / 1.60e-11, 30 x 32 1.27e-11 / 1.35e-11, 45 x 64
    3.45e-11 / 3.39e-11."""
    assert np.finfo(np.longdouble).eps < 2e-19
    x = C.spectrum(*shape, seed=31)
    truth = long_dft2(x)
    ours = np.abs(S.fft2_spec(x) - truth).max()
    numpys = np.abs(np.fft.fft2(x) - truth).max()
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


def test_shift_is_index_arithmetic():
    for n in (2, 5, 8, 25, 27):
        x = np.arange(n)
        assert np.array_equal(x[S.shift_index(n)], np.fft.fftshift(x))
        back = np.empty(n, int)
        back[S.shift_index(n)] = np.fft.fftshift(x)
        assert np.array_equal(back, x)
        assert np.array_equal((np.arange(n) + n // 2) % n, np.argsort(S.shift_index(n)))
