"""The notch-denoising kernels (csrc/apap_denoise.hip) on the MI355X against tests/denoise_spec.py, byte for byte: the
transform in both directions at every radix mix, at the longest rows and columns, with partial column strips and strips of 13, 7
and 5 columns; the notch step on the spectra that tests/golden/denoise_notch_ref.npz pins against the reference, the largest
disc (r = 6) and a schedule longer than the launch keeps among them; the whole chain in float64 and uint8, tall planes in a
batch, four channels, pictures whose discs are all ties;
and the contracts - guard bytes around every output, a workspace whose prior contents do not matter, pooled buffers reused."""
import numpy as np
import pytest

import denoise_cases as C
import denoise_spec as S

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
GUARD = 256


@pytest.fixture(scope="module")
def native_gpu(native):
    if native.lib().apap_device_count() < 1:
        pytest.skip("no HIP device")
    return native


def device():
    import torch
    return torch.device("cuda:0")


class Guarded:
    """``nbytes`` of device memory between two guards of sentinel bytes, pre-filled with ``fill``."""

    def __init__(self, nbytes, fill=0xFF):
        import torch
        self.n = nbytes
        self.buf = torch.full((nbytes + 2 * GUARD,), SENTINEL, dtype=torch.uint8, device=device())
        self.buf[GUARD:GUARD + nbytes] = fill
        assert self.buf.data_ptr() % 256 == 0
        self.ptr = self.buf.data_ptr() + GUARD

    def read(self, dtype):
        got = self.buf.cpu().numpy()
        assert (got[:GUARD] == SENTINEL).all() and (got[GUARD + self.n:] == SENTINEL).all(), "bytes outside a buffer were written"
        return got[GUARD:GUARD + self.n].copy().view(dtype)


def same(a, b):
    """Equal byte for byte (the sign of a zero included)."""
    return a.shape == b.shape and a.dtype == b.dtype and np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


# every radix alone and mixed; the longest rows and columns; partial strips (27 x 25, 32 x 20: 16 columns a strip; 1024 x 6: 4);
# above 1024 rows the planes are turned through 32 x 32 tiles: whole and partial tiles in both directions
FFT_SHAPES = [(2, 2), (3, 5), (4, 4), (8, 2), (27, 25), (30, 32), (81, 64), (125, 128), (120, 144), (2, 4096), (4096, 2), (4, 3840),
              (2160, 4), (32, 20), (1024, 6), (2048, 3), (2160, 20), (1080, 32), (1125, 45), (1280, 64)]
# column strips of 13, 7 and 5 columns; the column pass's first launch of 1024 threads; the longest lengths with the most
# radix-3 and radix-5 stages (tests/denoise_cases.py; tests/test_denoise_spec.py asserts that they are that)
FFT_SHAPES += list(C.FFT_STRIP_SHAPES) + [C.FFT_THRESHOLD_SHAPE] + list(C.FFT_LONG_SHAPES)


@pytest.mark.parametrize("shape", FFT_SHAPES)
def test_fft2_both_directions(native_gpu, shape):
    x = C.spectrum(*shape, seed=51)
    th, tw = S.twiddles(shape[0]), S.twiddles(shape[1])
    f = native_gpu.fft2(x)
    assert same(f, S.fft2_spec(x, th, tw))
    assert same(native_gpu.fft2(f, inverse=True), S.fft2_spec(f, th, tw, inverse=True))


def test_fft2_planes_and_resident_form(native_gpu):
    import torch
    from cvx_proj_amd import resident
    for shape in ((27, 25), (120, 144), (1024, 6), (1080, 36), (300, 27)):
        x = np.stack([C.spectrum(*shape, seed=60 + k) for k in range(3)])
        f = native_gpu.fft2(x)
        for k in range(3):
            assert same(f[k], native_gpu.fft2(x[k]))
        for inverse in (False, True):
            out = Guarded(x.nbytes)
            need = native_gpu.lib().apap_fft2_workspace_bytes(3, *shape)
            work = Guarded(need)
            d_x = torch.from_numpy(x).to(device())
            native_gpu.check(native_gpu.lib().apap_fft2_device(None, d_x.data_ptr(), out.ptr, 3, shape[0], shape[1], int(inverse), work.ptr, need, None))
            torch.cuda.synchronize()
            work.read(np.uint8)
            assert same(out.read(np.complex128).reshape(x.shape), native_gpu.fft2(x, inverse=inverse))
            assert same(resident.hip_fft2(d_x, inverse=inverse).cpu().numpy(), native_gpu.fft2(x, inverse=inverse))
        d_x = torch.from_numpy(x[0].copy()).to(device())
        assert resident.hip_fft2(d_x, out=d_x) is d_x and same(d_x.cpu().numpy(), f[0])       # in place
        # ... and back in place: by strips of 16, 4 and 13 columns, and (1080 rows) through the turned copy
        assert resident.hip_fft2(d_x, inverse=True, out=d_x) is d_x
        assert same(d_x.cpu().numpy(), S.fft2_spec(f[0], S.twiddles(shape[0]), S.twiddles(shape[1]), inverse=True))


@pytest.mark.parametrize("name", list(C.NOTCH_CASES))
def test_notch_spectrum(native_gpu, name, golden):
    import hashlib
    f0, p = C.notch_input(name), C.notch_params(name)
    got = native_gpu.notch_spectrum(f0, **p)
    assert same(got, S.notch_spec(f0, **p))
    ref = golden("denoise_notch_ref")
    if name in C.SMALL_CASES:
        want = f0.ravel().copy()
        want[ref[f"{name}_at"]] = ref[f"{name}_values"]
        assert same(got.ravel(), want)
    else:
        assert hashlib.sha256(np.ascontiguousarray(got).tobytes()).digest() == ref[f"{name}_sha256"].tobytes()
    two = native_gpu.notch_spectrum(np.stack([f0, f0.conj()]), **p)      # planes of one call are independent
    assert same(two[0], got) and same(two[1], S.notch_spec(f0.conj(), **p))
    import torch
    buf = Guarded(f0.nbytes)                                              # the in-place device form between guard bytes
    buf.buf[GUARD:GUARD + f0.nbytes] = torch.from_numpy(np.ascontiguousarray(f0).view(np.uint8).ravel()).to(device())
    native_gpu.check(native_gpu.lib().apap_notch_spectrum_device(None, buf.ptr, 1, f0.shape[0], f0.shape[1], p["spacing"], p["r"], p["sn"], None))
    torch.cuda.synchronize()
    assert same(buf.read(np.complex128).reshape(f0.shape), got)


# h, w, channels, spacing, r, sn, equalize
DENOISE_CASES = [(120, 144, 0, 9, 1, 9, True), (90, 100, 0, 14, 2, 9, True), (27, 25, 0, 9, 1, 3, True), (150, 160, 3, 14, 2, 9, True),
                 (768, 768, 0, 48, 5, 9, True), (120, 144, 0, 9, 1, 9, False), (90, 100, 2, 14, 2, 9, False), (75, 81, 0, 9, 1, 5, True),
                 (1080, 96, 2, 14, 2, 9, True), (1200, 50, 0, 9, 1, 9, False)] + C.CHAIN_EDGE_CASES


@pytest.mark.parametrize("h,w,channels,spacing,r,sn,equalize", DENOISE_CASES)
def test_notch_denoise(native_gpu, h, w, channels, spacing, r, sn, equalize):
    from cvx_proj_amd import denoise
    pic = C.picture(h, w, seed=70 + h, channels=channels)
    p = dict(spacing=spacing, r=r, sn=sn, equalize=equalize)
    want = S.denoise_spec(pic, **p)
    got = denoise.notch_denoise(pic, **p)
    assert got.dtype == np.float64 and same(got, want)
    got8 = denoise.notch_denoise(pic, out="uint8", **p)
    assert got8.dtype == np.uint8 and same(got8, S.to_uint8(want))
    if channels:        # the channels of one call equal a call each
        for c in range(channels):
            assert same(denoise.notch_denoise(np.ascontiguousarray(pic[..., c]), **p), got[..., c])


def test_batch_and_reference_signature(native_gpu):
    from cvx_proj_amd import denoise
    pics = np.stack([C.picture(90, 100, seed=80 + k, channels=3) for k in range(2)])
    p = dict(spacing=14, r=2, sn=9)
    got = denoise.notch_denoise_batch(pics, **p)
    for k in range(2):
        assert same(got[k], denoise.notch_denoise(pics[k], **p))
    plane = C.picture(768, 768, seed=42)
    new, log0, log1, eq = denoise.apply_median_filter(plane)
    st = S.denoise_stages(plane)
    assert same(eq, st["equalized"]) and same(new, st["out"])
    assert same(log0, np.log(1 + np.sqrt(st["spectrum"].real ** 2 + st["spectrum"].imag ** 2)))
    assert same(log1, np.log(1 + np.sqrt(st["filtered"].real ** 2 + st["filtered"].imag ** 2)))


def test_a_batch_of_tall_pictures(native_gpu):
    """Two pictures of two channels and 1080 rows: four planes through the turned copy and the notch on it in one call."""
    from cvx_proj_amd import denoise
    b = C.TALL_BATCH
    pics = np.stack([C.picture(b["h"], b["w"], seed=84 + k, channels=b["channels"]) for k in range(b["count"])])
    p = dict(spacing=b["spacing"], r=b["r"], sn=b["sn"])
    got = denoise.notch_denoise_batch(pics, **p)
    for k in range(b["count"]):
        assert same(got[k], denoise.notch_denoise(pics[k], **p)) and same(got[k], S.denoise_spec(pics[k], **p))


@pytest.mark.parametrize("name", list(C.tie_pictures()))
@pytest.mark.parametrize("equalize", [True, False])
def test_pictures_whose_discs_are_all_ties(native_gpu, name, equalize):
    from cvx_proj_amd import denoise
    pic = C.tie_pictures()[name]
    want = S.denoise_spec(pic, equalize=equalize, **C.TIE_PARAMS)
    assert same(denoise.notch_denoise(pic, equalize=equalize, **C.TIE_PARAMS), want)
    assert same(denoise.notch_denoise(pic, equalize=equalize, out="uint8", **C.TIE_PARAMS), S.to_uint8(want))
    if name == "constant_30x32":
        assert (want == 100.0).all()


@pytest.mark.parametrize("out", ["float64", "uint8"])
def test_contracts_of_the_resident_form(native_gpu, out):
    """Guard bytes around the output and the workspace; the workspace's prior contents (0xFF, then 0x00, then what the first
    call left) do not matter; hip_notch_denoise gives the same bytes; its uint8 result feeds the corner detector."""
    import torch
    from cvx_proj_amd import denoise, resident
    pic = C.picture(150, 160, seed=90, channels=3)
    p = dict(spacing=14, r=2, sn=9)
    want = denoise.notch_denoise(pic, out=out, **p)
    d_pic = torch.from_numpy(pic).to(device())
    need = native_gpu.lib().apap_notch_denoise_workspace_bytes(1, 150, 160, 3)
    assert need == resident.notch_denoise_workspace_bytes(1, 150, 160, 3)
    results = []
    work = None
    for fill in (0xFF, 0x00, None):
        res = Guarded(want.nbytes)
        work = Guarded(need, fill) if fill is not None else work
        native_gpu.check(native_gpu.lib().apap_notch_denoise_device(None, d_pic.data_ptr(), 1, 150, 160, 3, 1, 14, 2, 9, native_gpu.DENOISE_OUT[out],
                                                                    res.ptr, work.ptr, need, None))
        torch.cuda.synchronize()
        work.read(np.uint8)
        results.append(res.read(want.dtype).reshape(want.shape))
    assert all(same(r, want) for r in results)
    got = resident.hip_notch_denoise(d_pic, out=out, **p)
    assert same(got.cpu().numpy(), want)
    if out == "uint8":
        scratch = torch.empty(need + 512, dtype=torch.uint8, device=device())
        again = resident.hip_notch_denoise(d_pic, out=out, work=scratch, **p)
        assert same(again.cpu().numpy(), want)
        assert again.dtype == torch.uint8 and again.shape == d_pic.shape        # what hip_corner_detect takes


def test_pooled_buffers_are_reused(native_gpu):
    from cvx_proj_amd import denoise
    ctx = native_gpu.Context()
    a, b = C.picture(120, 144, seed=91, channels=3), C.picture(90, 100, seed=92)
    pa, pb = dict(spacing=9, r=1, sn=9), dict(spacing=14, r=2, sn=9)
    first = denoise.notch_denoise(a, ctx=ctx, **pa)
    other = denoise.notch_denoise(b, ctx=ctx, out="uint8", **pb)
    assert same(denoise.notch_denoise(a, ctx=ctx, **pa), first) and same(first, denoise.notch_denoise(a, **pa))
    assert same(other, denoise.notch_denoise(b, out="uint8", **pb))
    f = C.spectrum(30, 32, seed=93)
    assert same(native_gpu.fft2(f, ctx=ctx), native_gpu.fft2(f))
    ctx.close()
