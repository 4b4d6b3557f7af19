"""The notch denoising's host side without a GPU: every argument rule is checked before a device is looked for (so each is
visible here as ERR_INVALID_ARG with a message that names the rule), a valid call without a device is ERR_NO_DEVICE, the
workspace grows with planes and size, and the Python front end (cvx_proj_amd/denoise.py) applies the same rules."""
import numpy as np
import pytest

import denoise_spec as S

OK_NOTCH = dict(spacing=48, r=5, sn=9)


def invalid(native, call, *needles):
    with pytest.raises(native.ApapValueError) as e:
        call()
    assert e.value.code == native.ERR_INVALID_ARG
    for n in needles:
        assert n in str(e.value), str(e.value)


@pytest.mark.parametrize("shape,needle", [((7, 8), "5-smooth"), ((8, 14), "5-smooth"), ((1, 8), "2 .. 4096"), ((8, 4100), "2 .. 4096"),
                                          ((4098, 8), "2 .. 4096"), ((8, 4097), "2 .. 4096")])
def test_lengths(native, shape, needle):
    invalid(native, lambda: native.fft2(np.zeros(shape, np.complex128)), needle)
    invalid(native, lambda: native.notch_denoise(np.zeros((1, *shape, 1), np.uint8)), needle)
    assert native.lib().apap_notch_denoise_workspace_bytes(1, shape[0], shape[1], 1) == 0
    assert native.lib().apap_fft2_workspace_bytes(1, shape[0], shape[1]) == 0


@pytest.mark.parametrize("params,needle", [(dict(r=0), "r=0"), (dict(r=7), "r=7"), (dict(sn=1), "sn=1"), (dict(spacing=30), "max(6 r, 5 r + 3) = 30"),
                                           (dict(spacing=8, r=1), "max(6 r, 5 r + 3) = 8"), (dict(spacing=36, r=6), "= 36")])
def test_notch_parameters(native, params, needle):
    from cvx_proj_amd import denoise
    p = {**OK_NOTCH, **params}
    invalid(native, lambda: native.notch_denoise(np.zeros((1, 8, 8, 1), np.uint8), **p), needle)
    invalid(native, lambda: native.notch_spectrum(np.zeros((8, 8), np.complex128), **p), needle)
    for call in (lambda: denoise.notch_denoise(np.zeros((8, 8), np.uint8), **p), lambda: denoise.notch_spectrum(np.zeros((8, 8), complex), **p),
                 lambda: denoise.notch_schedule(**p)):
        with pytest.raises(ValueError, match="r=|sn=|spacing="):
            call()
    with pytest.raises(ValueError, match="sn="):      # the schedule is a Python list: no plane has 4096 harmonics
        denoise.notch_schedule(sn=10 ** 9)
    with pytest.raises(ValueError):
        S.notch_check(**p)


def test_other_arguments(native):
    invalid(native, lambda: native.notch_denoise(np.zeros((1, 8, 8, 5), np.uint8)), "channels")
    with pytest.raises(ValueError):
        native.notch_denoise(np.zeros((1, 8, 8, 1), np.uint8), out="float32")
    lib = native.lib()
    img, out = np.zeros((8, 8), np.uint8), np.zeros((8, 8))
    assert lib.apap_notch_denoise(None, native._ptr(img, native.C.c_uint8), 1, 8, 8, 1, 1, 48, 5, 9, 7, out.ctypes.data, -1) == native.ERR_INVALID_ARG
    assert "output type" in native.last_error()
    assert lib.apap_notch_denoise(None, None, 1, 8, 8, 1, 1, 48, 5, 9, 0, out.ctypes.data, -1) == native.ERR_INVALID_ARG
    assert lib.apap_fft_twiddles(0, native._ptr(out, native.C.c_double)) == native.ERR_INVALID_ARG
    # the device forms check the same rules before they use a pointer
    assert lib.apap_notch_denoise_device(None, 256, 1, 8, 7, 1, 1, 48, 5, 9, 0, 256, 256, 1 << 30, None) == native.ERR_INVALID_ARG
    assert "5-smooth" in native.last_error()
    assert lib.apap_fft2_device(None, 256, 256, 1, 8, 8, 0, 256, 16, None) == native.ERR_WORKSPACE
    assert lib.apap_notch_spectrum_device(None, 256, 1, 8, 8, 30, 5, 9, None) == native.ERR_INVALID_ARG
    from cvx_proj_amd import denoise
    for bad in (np.zeros((8, 8), np.float32), np.zeros((2, 8, 8, 3, 1), np.uint8)):
        with pytest.raises(ValueError):
            denoise.notch_denoise(bad)
    with pytest.raises(ValueError):
        denoise.apply_median_filter(np.zeros((8, 8, 3), np.uint8))


def test_no_device_is_an_error_not_a_fallback(native):
    if native.lib().apap_device_count() > 0:
        return      # tests/test_gpu_denoise.py runs these calls
    from cvx_proj_amd import denoise
    for call in (lambda: denoise.notch_denoise(np.zeros((8, 8, 3), np.uint8)), lambda: denoise.fft2(np.zeros((8, 8), complex)),
                 lambda: denoise.notch_spectrum(np.zeros((8, 8), complex)), lambda: denoise.apply_median_filter(np.zeros((8, 8), np.uint8))):
        with pytest.raises(native.ApapError) as e:
            call()
        assert e.value.code == native.ERR_NO_DEVICE


def test_workspace_is_monotone(native):
    ws = native.lib().apap_notch_denoise_workspace_bytes
    assert 0 < ws(1, 8, 8, 1) < ws(1, 8, 8, 3) < ws(2, 8, 8, 3) < ws(2, 16, 8, 3) < ws(2, 16, 16, 3) < ws(2, 768, 768, 3)
    assert ws(1, 768, 768, 3) >= 3 * 768 * 768 * 16 + 3 * 768 * 768 + 2 * 768 * 16
    assert ws(1, 4096, 4096, 1) > 1 << 28 and ws(0, 8, 8, 1) == 0 and ws(1, 8, 8, 5) == 0 and ws(65535, 8, 8, 3) == 0
    f = native.lib().apap_fft2_workspace_bytes
    assert 0 < f(1, 2, 2) <= f(1, 8, 8) < f(1, 768, 768) < f(1, 4096, 4096) and f(3, 768, 768) == f(1, 768, 768)
    # above 1024 rows the planes are turned into a second copy
    assert f(1, 1024, 8) == f(1, 1024, 4) and f(2, 1080, 8) >= f(1, 1080, 8) + 1080 * 8 * 16 and f(0, 8, 8) == 0
    assert ws(1, 1080, 8, 1) >= 2 * 1080 * 8 * 16 > ws(1, 1024, 8, 1) - 1024 * 8 * 16


def test_schedule(native):
    from cvx_proj_amd import denoise
    assert len(denoise.notch_schedule()) == 77 and denoise.notch_schedule() == S.notch_schedule()
    assert denoise.notch_schedule(9, 1, 3) == S.notch_schedule(9, 1, 3)
    assert (native.FFT_MIN_LENGTH, native.FFT_MAX_LENGTH, native.NOTCH_MAX_R) == (S.MIN_LENGTH, S.MAX_LENGTH, S.MAX_R)
    import os
    import re
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "apap_hip.h")).read()
    for name, val in (("FFT_MIN_LENGTH", 2), ("FFT_MAX_LENGTH", 4096), ("NOTCH_MAX_R", 6), ("DENOISE_OUT_F64", native.DENOISE_OUT["float64"]),
                      ("DENOISE_OUT_U8", native.DENOISE_OUT["uint8"])):
        assert int(re.search(rf"#define APAP_{name} (\d+)", text).group(1)) == val
