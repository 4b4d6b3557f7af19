"""The dehazing's host side without a GPU: every argument rule is checked before a device is looked for (each visible here as
ERR_INVALID_ARG with a message that names the rule), a valid call without a device is ERR_NO_DEVICE, the workspace is a
positive multiple of 256 bytes, and the Python front end (cvx_proj_amd/dehaze.py) applies the same rules."""
import os
import subprocess
import sys

import numpy as np
import pytest

import dehaze_spec as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PIC = np.zeros((1, 8, 9, 3), np.uint8)
OK = dict(radius=7, omega_q=243, t0_q=410, refine=30, eps=64)


def invalid(native, call, *needles):
    with pytest.raises(native.ApapValueError) as e:
        call()
    assert e.value.code == native.ERR_INVALID_ARG
    for n in needles:
        assert n in str(e.value), str(e.value)


@pytest.mark.parametrize("params,needle", [(dict(radius=-1), "radius=-1"), (dict(radius=33), "radius=33"), (dict(omega_q=-1), "omega_q=-1"),
                                           (dict(omega_q=257), "omega_q=257"), (dict(t0_q=0), "t0_q=0"), (dict(t0_q=4097), "t0_q=4097"),
                                           (dict(refine=-1), "refine=-1"), (dict(refine=33), "refine=33"), (dict(eps=0), "eps=0"),
                                           (dict(eps=65536), "eps=65536")])
def test_parameter_rules_through_the_c_abi(native, params, needle):
    p = {**OK, **params}
    invalid(native, lambda: native.dehaze(PIC, **p), needle)
    invalid(native, lambda: native.transmission(PIC, **p), needle)
    if "radius" in params:
        invalid(native, lambda: native.dark_channel(PIC, params["radius"]), needle)
        invalid(native, lambda: native.atmospheric_light(PIC, params["radius"]), needle)
    # the device forms check the same rules before they use a pointer
    q = tuple(p[k] for k in ("radius", "omega_q", "t0_q", "refine", "eps"))
    lib = native.lib()
    assert lib.apap_dehaze_device(None, 256, 1, 8, 9, 3, *q, 256, None, None, 256, 1 << 30, None) == native.ERR_INVALID_ARG
    assert needle in native.last_error()
    assert lib.apap_transmission_device(None, 256, 1, 8, 9, 3, *q, 256, 256, 1 << 30, None) == native.ERR_INVALID_ARG
    assert needle in native.last_error()


@pytest.mark.parametrize("shape,needle", [((0, 8, 9, 3), "pictures"), ((65536, 1, 1, 3), "pictures"), ((1, 0, 9, 3), "2^31"), ((1, 8, 0, 3), "2^31"),
                                          ((1, 1 << 16, 1 << 15, 3), "2^31"), ((1, 8, 9, 2), "channels"), ((1, 8, 9, 4), "channels")])
def test_picture_rules_through_the_c_abi(native, shape, needle):
    lib = native.lib()
    n, h, w, c = shape
    q = (7, 243, 410, 30, 64)
    assert lib.apap_dehaze_workspace_bytes(n, h, w, c, 30) == 0
    assert lib.apap_dehaze_device(None, 256, n, h, w, c, *q, 256, None, None, 256, 1 << 30, None) == native.ERR_INVALID_ARG
    assert needle in native.last_error(), native.last_error()
    assert lib.apap_dark_channel_device(None, 256, n, h, w, c, 7, 256, 256, 1 << 30, None) == native.ERR_INVALID_ARG
    assert lib.apap_atmospheric_light_device(None, 256, n, h, w, c, 7, 256, 256, 1 << 30, None) == native.ERR_INVALID_ARG
    assert lib.apap_transmission_device(None, 256, n, h, w, c, *q, 256, 256, 1 << 30, None) == native.ERR_INVALID_ARG
    one = np.zeros(4, np.uint8)      # never read: the shape is refused first
    u8 = native._ptr(one, native.C.c_uint8)
    assert lib.apap_dehaze(None, u8, n, h, w, c, *q, u8, None, None, -1) == native.ERR_INVALID_ARG
    assert lib.apap_dark_channel(None, u8, n, h, w, c, 7, u8, -1) == native.ERR_INVALID_ARG
    assert lib.apap_atmospheric_light(None, u8, n, h, w, c, 7, u8, -1) == native.ERR_INVALID_ARG
    assert lib.apap_transmission(None, u8, n, h, w, c, *q, native._ptr(np.zeros(4, np.uint16), native.C.c_uint16), -1) == native.ERR_INVALID_ARG


def test_pointers_and_workspace(native):
    lib = native.lib()
    q = (7, 243, 410, 30, 64)
    u8 = native._ptr(np.zeros(8 * 9 * 3, np.uint8), native.C.c_uint8)
    assert lib.apap_dehaze(None, None, 1, 8, 9, 3, *q, u8, None, None, -1) == native.ERR_INVALID_ARG and "null" in native.last_error()
    assert lib.apap_dehaze(None, u8, 1, 8, 9, 3, *q, None, None, None, -1) == native.ERR_INVALID_ARG and "null" in native.last_error()
    assert lib.apap_dark_channel(None, u8, 1, 8, 9, 3, 7, None, -1) == native.ERR_INVALID_ARG
    assert lib.apap_atmospheric_light(None, u8, 1, 8, 9, 3, 7, None, -1) == native.ERR_INVALID_ARG
    assert lib.apap_transmission(None, u8, 1, 8, 9, 3, *q, None, -1) == native.ERR_INVALID_ARG
    assert lib.apap_dehaze_device(None, None, 1, 8, 9, 3, *q, 256, None, None, 256, 1 << 30, None) == native.ERR_INVALID_ARG
    assert lib.apap_dehaze_device(None, 256, 1, 8, 9, 3, *q, None, None, None, 256, 1 << 30, None) == native.ERR_INVALID_ARG
    assert lib.apap_dehaze_device(None, 256, 1, 8, 9, 3, *q, 256, None, None, None, 1 << 30, None) == native.ERR_INVALID_ARG
    need = lib.apap_dehaze_workspace_bytes(1, 8, 9, 3, 30)
    assert lib.apap_dehaze_device(None, 256, 1, 8, 9, 3, *q, 256, None, None, 256, need - 1, None) == native.ERR_WORKSPACE
    assert lib.apap_dehaze_device(None, 256, 1, 8, 9, 3, *q, 256, None, None, 257, need + 1, None) == native.ERR_INVALID_ARG
    assert "aligned" in native.last_error()
    assert lib.apap_dark_channel_device(None, 256, 1, 8, 9, 3, 7, 256, 256, 16, None) == native.ERR_WORKSPACE


def test_workspace_bytes(native):
    ws = native.lib().apap_dehaze_workspace_bytes
    for args in ((1, 1, 1, 1, 0), (1, 1, 1, 3, 32), (1, 8, 9, 3, 30), (3, 17, 129, 1, 1), (2, 768, 768, 3, 30), (1, 2160, 3840, 3, 0)):
        assert ws(*args) > 0 and ws(*args) % 256 == 0, args
    assert ws(1, 8, 9, 3, 0) < ws(1, 8, 9, 3, 1) == ws(1, 8, 9, 3, 32) < ws(2, 8, 9, 3, 32) < ws(2, 80, 9, 3, 32) < ws(2, 80, 90, 3, 32)
    n = 2160 * 3840
    assert 3 * n <= ws(1, 2160, 3840, 3, 0) < 3 * n + 4096 and 15 * n <= ws(1, 2160, 3840, 3, 30) < 15 * n + 4096
    assert ws(1, 8, 9, 3, 33) == 0 and ws(1, 8, 9, 3, -1) == 0 and ws(0, 8, 9, 3, 0) == 0 and ws(1, 8, 9, 2, 0) == 0


@pytest.mark.parametrize("bad", [dict(radius=-1), dict(radius=33), dict(refine=33), dict(refine=-1), dict(eps=0), dict(eps=65536),
                                 dict(omega=1.01), dict(omega=-0.1), dict(t0=1.5), dict(t0=-0.5), dict(omega=float("nan"))])
def test_parameter_rules_in_python(native, bad):
    from cvx_proj_amd import dehaze
    pic = np.zeros((8, 9, 3), np.uint8)
    with pytest.raises(ValueError, match="radius=|refine=|eps=|omega=|t0="):
        dehaze.dehaze_arguments(**bad)
    with pytest.raises(ValueError):
        S.arguments(**bad)
    for call in (dehaze.dehaze, dehaze.transmission, lambda m, **kw: dehaze.dehaze_batch(m[None], **kw)):
        with pytest.raises(ValueError, match="radius=|refine=|eps=|omega=|t0="):
            call(pic, **bad)
    if "radius" in bad:
        for call in (dehaze.dark_channel, dehaze.atmospheric_light):
            with pytest.raises(ValueError, match="radius="):
                call(pic, **bad)


def test_python_forms(native):
    from cvx_proj_amd import dehaze
    assert dehaze.dehaze_arguments() == (7, 243, 410, 30, 64) == S.arguments()
    for kw in (dict(omega=1.0, t0=0.0), dict(omega=0.0, t0=1.0), dict(omega=0.5, t0=0.25, radius=0, refine=0, eps=1), dict(eps=65535, radius=32, refine=32)):
        assert dehaze.dehaze_arguments(**kw) == S.arguments(**kw)
    for bad in (np.zeros((8, 9), np.float32), np.zeros((8, 9, 2), np.uint8), np.zeros((8, 9, 4), np.uint8), np.zeros((2, 8, 9, 3), np.uint8),
                np.zeros((0, 9, 3), np.uint8)):
        for call in (dehaze.dehaze, dehaze.dark_channel, dehaze.atmospheric_light, dehaze.transmission):
            with pytest.raises(ValueError, match="picture expected"):
                call(bad)
    for bad in (np.zeros((8, 9), np.uint8), np.zeros((2, 8, 9, 2), np.uint8), np.zeros((2, 8, 9), np.int16)):
        with pytest.raises(ValueError, match="pictures of one shape"):
            dehaze.dehaze_batch(bad)
    with pytest.raises(ValueError):
        dehaze.dehaze_batch([np.zeros((8, 9, 3), np.uint8), np.zeros((8, 10, 3), np.uint8)])
    for bad in (np.zeros((8, 9, 3), np.uint8), np.zeros((1, 8, 9, 2), np.uint8)):
        with pytest.raises(ValueError):
            native.dehaze(bad)
    assert (native.DEHAZE_MAX_RADIUS, native.DEHAZE_ONE) == (S.MAX_RADIUS, S.ONE)


def test_no_device_is_an_error_not_a_fallback(native):
    if native.lib().apap_device_count() > 0:
        return      # tests/test_gpu_dehaze.py runs these calls
    from cvx_proj_amd import dehaze
    pic = np.zeros((8, 9, 3), np.uint8)
    for call in (lambda: dehaze.dark_channel(pic), lambda: dehaze.atmospheric_light(pic), lambda: dehaze.transmission(pic),
                 lambda: dehaze.transmission(pic, refine=0), lambda: dehaze.dehaze(pic), lambda: dehaze.dehaze(pic[..., 0], return_parts=True),
                 lambda: dehaze.dehaze_batch(np.stack([pic, pic]))):
        with pytest.raises(native.ApapError) as e:
            call()
        assert e.value.code == native.ERR_NO_DEVICE


def test_the_build_names_the_source_and_the_module_needs_no_torch():
    text = open(os.path.join(ROOT, "cvx_proj_amd", "csrc", "Makefile")).read()
    src = next(line for line in text.splitlines() if line.startswith("SRC"))
    ksrc = next(line for line in text.splitlines() if line.startswith("KSRC"))
    assert "apap_dehaze.hip" in src and "apap_dehaze.hip" in ksrc
    code = ("import sys; import cvx_proj_amd.dehaze as D; from cvx_proj_amd import _native; _native.lib(); D.dehaze_arguments(); "
            "assert 'torch' not in sys.modules, 'torch was imported'; assert 'cv2' not in sys.modules; print('ok')")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stderr[-1500:]
