"""The panorama's two-band blend without a GPU: the numpy specification (tests/panorama_band_spec.py) against a brute-force
blur, against the ramp's specification and against its own identities; the host-only parts of the C ABI (the blur's division,
the argument checks, the workspace rule) against it; and every built input against the edge it is built to reach."""
import numpy as np
import pytest

import panorama_band_cases as BC
import panorama_band_spec as P
import panorama_cases as E
import panorama_ramp_cases as RC
import panorama_ramp_spec as R


@pytest.mark.parametrize("hw", [(1, 1), (1, 5), (4, 1), (2, 2), (5, 7), (9, 4)])
def test_box_blur_is_the_double_loop(hw):
    rng = np.random.default_rng(hw[0] * 100 + hw[1])
    img = rng.integers(0, 256, hw + (3,), dtype=np.uint8)
    for r in (0, 1, 2, 3, 8):
        assert np.array_equal(P.box_blur(img, r), P.box_blur_brute(img, r)), (hw, r)
    assert np.array_equal(P.box_blur(img, 0), img)
    white = np.full(hw + (3,), 255, np.uint8)
    assert (P.box_blur(white, 32) == 255).all(), "the largest sum, 255 x 4225, and its rounding"
    for bad in (-1, 33, 2.0, True):
        with pytest.raises(ValueError):
            P.box_blur(img, bad)


@pytest.mark.parametrize("name", RC.ALL_CASES)
def test_band_0_is_the_ramp(name):
    case = E.get(name)
    center, layers, geos = case["center"], case["layers"], case["geometries"]
    for ramp in (1, 8, 256):
        got = P.compose_band(center, layers, geos, RC.oracle_coords(name), ramp, 0)
        want, wsum, count = R.compose_ramp(center, layers, geos, RC.oracle_coords(name), ramp)
        assert np.array_equal(got.canvas, want) and np.array_equal(got.wsum, wsum) and np.array_equal(got.count, count)


def test_where_one_view_is_present_the_output_is_its_sample():
    """`cross`: the centre and four layers, three of them alone somewhere on the canvas; under gains too."""
    case = E.get("cross")
    center, layers, geos = case["center"], case["layers"], case["geometries"]
    q = BC.gains(5)
    alone_views = set()
    for band in (0, 1, 8, 32):
        for gains in (None, q):
            c, b, D = P.views(center, layers, geos, RC.oracle_coords("cross"), band)
            got = P.blend(c, b, D, 8, gains)
            alone = got.count == 1
            assert alone.sum() > 1000
            sample = c[got.source.clip(0), np.arange(c.shape[1])[:, None], np.arange(c.shape[2])[None, :]]
            want = sample if gains is None else np.stack([P.G.apply(c[v], q[v]) for v in range(5)])[
                got.source.clip(0), np.arange(c.shape[1])[:, None], np.arange(c.shape[2])[None, :]]
            assert np.array_equal(got.canvas[alone], want[alone]), (band, gains)
            assert not got.canvas[got.count == 0].any()
            alone_views |= set(np.unique(got.source[alone]).tolist())
    assert alone_views == {1, 2, 3}, "three of the layers reach beyond every other view"


def test_band_8_differs_from_band_0():
    case = E.get("cross")
    args = (case["center"], case["layers"], case["geometries"], RC.oracle_coords("cross"), 8)
    differ = (P.compose_band(*args, 8).canvas != P.compose_band(*args, 0).canvas).any(axis=-1)
    assert differ.sum() > 500 and not differ[P.compose_band(*args, 8).count <= 1].any()


def test_the_blurs_division_is_exact(native):
    """B = (T + (n^2 >> 1)) // n^2 by ramp_quotient's one float32 division, through its host copy
    apap_panorama_ramp_quotients: every r = 1 .. 32 and every T = 0 .. 255 n^2, about 12 million values."""
    assert native.PANORAMA_MAX_BAND == P.MAX_BAND == 32
    checked = 0
    for r in range(1, 33):
        n2 = (2 * r + 1) ** 2
        T = np.arange(0, 255 * n2 + 1, dtype=np.int64) + (n2 >> 1)
        assert T.max() < 1 << 21 and n2 <= 4225
        got = native.panorama_ramp_quotients(T, np.full_like(T, n2))
        assert np.array_equal(got, T // n2), r
        assert got.max() == 255
        checked += T.size
    assert checked == 255 * sum((2 * r + 1) ** 2 for r in range(1, 33)) + 32 == 12215552


def _c_arguments(native, center, l):
    C = native.C
    i32 = lambda v: np.array([v], dtype=np.int32)      # noqa: E731
    img, H = np.ascontiguousarray(l.img), np.ascontiguousarray(l.local_homography)
    mw, mh = np.ascontiguousarray(l.mesh[0]), np.ascontiguousarray(l.mesh[1])
    out = np.zeros((l.final_size[1], l.final_size[0], 3), np.uint8)
    ints = dict(ih=i32(img.shape[0]), iw=i32(img.shape[1]), mr=i32(H.shape[0]), mc=i32(H.shape[1]), nw=i32(mw.size), nh=i32(mh.size),
                fw=i32(l.final_size[0]), fh=i32(l.final_size[1]), ox=i32(l.offset[0]), oy=i32(l.offset[1]))
    return C, img, H, mw, mh, out, ints


def test_argument_errors_come_before_any_device(native):
    """A band outside 0 .. 32 first, then everything the ramp entry refuses, then the gains: APAP_ERR_INVALID_ARG whether or
    not a GPU is visible; in Python a bad band is a plain ValueError before the library is entered."""
    from cvx_proj_amd import apap
    case = E.get("shared")
    center, layers = case["center"], case["layers"]

    def refused(c, ls, match="", **kw):
        with pytest.raises(native.ApapError, match=match) as e:
            native.panorama(c, ls, blend="band", ramp=8, band=4, **kw)
        assert e.value.code == native.ERR_INVALID_ARG and isinstance(e.value, ValueError)

    fh = layers[1].final_size[1]
    refused(center, [layers[0], layers[1]._replace(final_size=(center.shape[1] - 1, fh))], match="layer 1: centre image")
    refused(center, [layers[0]._replace(img=np.ones((1, 1, 3), np.uint8))], match="layer 0: picture 1 x 1")
    refused(np.ones((1, 1, 3), np.uint8), [layers[0]], match="centre picture 1 x 1")
    refused(center, layers, match=r"gain_q\[1\] = 1023", gain_q=[4096, 1023, 4096])
    refused(center, layers, match=r"gain_q\[2\] = 16384", gain_q=[4096, 4096, 16384])
    with pytest.raises(ValueError, match="gain_q"):
        native.panorama(center, layers, blend="band", gain_q=[4096, 4096])
    for entry in (native.panorama, apap.panorama):
        for bad in (-1, 33, 2.5, "8", None, True):
            with pytest.raises(ValueError, match="band") as e:
                entry(center, layers, blend="band", band=bad)
            assert not isinstance(e.value, native.ApapError), "refused in Python, before the library"
        for bad in (0, 257, "8"):
            with pytest.raises(ValueError, match="ramp") as e:
                entry(center, layers, blend="band", ramp=bad)
            assert not isinstance(e.value, native.ApapError)
    with pytest.raises(ValueError, match="band"):
        apap.panorama(center, layers, blend="band", band=40, gain="auto")
    with pytest.raises(ValueError, match="blend must be"):
        native.panorama(center, layers, blend="bands")
    for bad in (-1, 33, 1.0, True):
        with pytest.raises(ValueError, match="band") as e:
            native.box_blur(center, bad)
        assert not isinstance(e.value, native.ApapError)
    for blend in ("mean", "paste", "ramp"):     # the other blends ignore it: they get as far as the device
        if native.lib().apap_device_count() == 0:
            with pytest.raises(native.ApapError) as e:
                native.panorama(center, layers, blend=blend, band="8")
            assert e.value.code == native.ERR_NO_DEVICE
    assert "band" not in native.PANORAMA_MODES and "ramp" not in native.PANORAMA_MODES

    # straight at the C entry points
    n = 1
    C, img, H, mw, mh, out, ints = _c_arguments(native, center, layers[0])
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))      # noqa: E731
    vpp = lambda p: (C.c_void_p * n)(p)      # noqa: E731

    def call(ramp=8, band=4, gain=None, center_p=center.ctypes.data, img_p=img.ctypes.data, h_p=H.ctypes.data, mw_p=mw.ctypes.data,
             mh_p=mh.ctypes.data, out_p=out.ctypes.data, null_int=None):
        a = {k: (None if k == null_int else ip(v)) for k, v in ints.items()}
        g = None if gain is None else ip(np.array(gain, dtype=np.int32))
        return native.lib().apap_panorama_band(None, C.cast(center_p, C.POINTER(C.c_uint8)), center.shape[0], center.shape[1], vpp(img_p),
                                               a["ih"], a["iw"], vpp(h_p), a["mr"], a["mc"], vpp(mw_p), a["nw"], vpp(mh_p), a["nh"],
                                               a["fw"], a["fh"], a["ox"], a["oy"], n, ramp, band, g, C.cast(out_p, C.POINTER(C.c_uint8)),
                                               None, -1)

    def call_device(ramp=8, band=4, gain=None):
        g = None if gain is None else ip(np.array(gain, dtype=np.int32))
        # host pointers: every call here is refused before one is looked at
        return native.lib().apap_panorama_band_device(
            None, center.ctypes.data, center.shape[0], center.shape[1], vpp(img.ctypes.data), ip(ints["ih"]), ip(ints["iw"]),
            vpp(H.ctypes.data), ip(ints["mr"]), ip(ints["mc"]), vpp(mw.ctypes.data), ip(ints["nw"]), vpp(mh.ctypes.data), ip(ints["nh"]),
            ip(ints["fw"]), ip(ints["fh"]), ip(ints["ox"]), ip(ints["oy"]), n, ramp, band, g, out.ctypes.data, None, 0, None, None)

    for band in (-1, 33, 1 << 20):
        for ramp in (8, 0):     # the band is refused first
            assert call(ramp=ramp, band=band) == native.ERR_INVALID_ARG
            assert native.last_error() == f"apap_panorama_band: band = {band} (0 .. 32)"
            assert call_device(ramp=ramp, band=band) == native.ERR_INVALID_ARG
            assert native.last_error() == f"apap_panorama_band_device: band = {band} (0 .. 32)"
    for ramp in (0, 257, -1):
        assert call(ramp=ramp) == native.ERR_INVALID_ARG and f"apap_panorama_band: ramp = {ramp}" in native.last_error()
        assert call_device(ramp=ramp) == native.ERR_INVALID_ARG and f"apap_panorama_band_device: ramp = {ramp}" in native.last_error()
    for gain in ([4096, 1023], [16384, 4096]):
        assert call(gain=gain) == native.ERR_INVALID_ARG and "gain_q[" in native.last_error()
        assert call_device(gain=gain) == native.ERR_INVALID_ARG and "gain_q[" in native.last_error()
    for kw in [dict(center_p=None), dict(img_p=None), dict(h_p=None), dict(mw_p=None), dict(mh_p=None), dict(out_p=None)] + \
              [dict(null_int=k) for k in ints]:
        assert call(**kw) == native.ERR_INVALID_ARG, kw
        assert "null" in native.last_error()
    # the band is no mode of the entry points that take one: they refuse 3 as they refuse 2 and 7
    code = native.lib().apap_panorama(None, C.cast(center.ctypes.data, C.POINTER(C.c_uint8)), center.shape[0], center.shape[1],
                                      vpp(img.ctypes.data), ip(ints["ih"]), ip(ints["iw"]), vpp(H.ctypes.data), ip(ints["mr"]),
                                      ip(ints["mc"]), vpp(mw.ctypes.data), ip(ints["nw"]), vpp(mh.ctypes.data), ip(ints["nh"]),
                                      ip(ints["fw"]), ip(ints["fh"]), ip(ints["ox"]), ip(ints["oy"]), n, 3,
                                      C.cast(out.ctypes.data, C.POINTER(C.c_uint8)), None, -1)
    assert code == native.ERR_INVALID_ARG and "mode = 3" in native.last_error()

    # apap_box_blur[_device]
    u8 = lambda a: C.cast(a.ctypes.data, C.POINTER(C.c_uint8))      # noqa: E731
    pic, res = np.ones((4, 5, 3), np.uint8), np.zeros((4, 5, 3), np.uint8)
    for radius in (-1, 33):
        assert native.lib().apap_box_blur(None, u8(pic), 4, 5, radius, u8(res), -1) == native.ERR_INVALID_ARG
        assert native.last_error() == f"apap_box_blur: radius = {radius} (0 .. 32)"
        assert native.lib().apap_box_blur_device(None, pic.ctypes.data, 4, 5, radius, res.ctypes.data, None) == native.ERR_INVALID_ARG
        assert native.last_error() == f"apap_box_blur_device: radius = {radius} (0 .. 32)"
    for h, w in ((0, 5), (4, 0), (-1, 5), (1 << 15, 1 << 15)):
        assert native.lib().apap_box_blur(None, u8(pic), h, w, 2, u8(res), -1) == native.ERR_INVALID_ARG
        assert f"picture {h} x {w}" in native.last_error()
        assert native.lib().apap_box_blur_device(None, pic.ctypes.data, h, w, 2, res.ctypes.data, None) == native.ERR_INVALID_ARG
    assert native.lib().apap_box_blur(None, None, 4, 5, 2, u8(res), -1) == native.ERR_INVALID_ARG and "null" in native.last_error()
    assert native.lib().apap_box_blur(None, u8(pic), 4, 5, 2, None, -1) == native.ERR_INVALID_ARG and "null" in native.last_error()
    assert native.lib().apap_box_blur_device(None, None, 4, 5, 2, res.ctypes.data, None) == native.ERR_INVALID_ARG
    assert native.lib().apap_box_blur_device(None, pic.ctypes.data, 4, 5, 2, pic.ctypes.data, None) == native.ERR_INVALID_ARG
    assert "overlaps" in native.last_error()


def test_the_workspace_rule(native):
    """apap_panorama_workspace_bytes plus, for band > 0, a 256-byte aligned slot per view; 0 extra at band 0; 0 for invalid
    arguments."""
    up = lambda v: (v + 255) // 256 * 256      # noqa: E731
    for name in ("cross", "shared", "two_pixels"):
        case = E.get(name)
        center, layers = case["center"], case["layers"]
        ip = native._ip
        i32 = lambda vs: np.array(vs, dtype=np.int32)      # noqa: E731
        ih, iw = i32([l.img.shape[0] for l in layers]), i32([l.img.shape[1] for l in layers])
        mr, mc = i32([l.local_homography.shape[0] for l in layers]), i32([l.local_homography.shape[1] for l in layers])
        fw, fh = i32([l.final_size[0] for l in layers]), i32([l.final_size[1] for l in layers])
        n = len(layers)
        base = native.lib().apap_panorama_workspace_bytes(ip(mr), ip(mc), ip(fw), ip(fh), n)
        f = native.lib().apap_panorama_band_workspace_bytes
        ch, cw = center.shape[:2]
        assert base > 0 and f(ch, cw, ip(ih), ip(iw), ip(mr), ip(mc), ip(fw), ip(fh), n, 0) == base
        slots = up(ch * cw * 3) + sum(up(int(h) * int(w) * 3) for h, w in zip(ih, iw))
        for band in (1, 8, 32):
            got = f(ch, cw, ip(ih), ip(iw), ip(mr), ip(mc), ip(fw), ip(fh), n, band)
            assert got == base + slots and got % 256 == 0
        for band in (-1, 33):
            assert f(ch, cw, ip(ih), ip(iw), ip(mr), ip(mc), ip(fw), ip(fh), n, band) == 0
        assert f(0, cw, ip(ih), ip(iw), ip(mr), ip(mc), ip(fw), ip(fh), n, 8) == 0
        assert f(ch, cw, None, ip(iw), ip(mr), ip(mc), ip(fw), ip(fh), n, 8) == 0
        assert f(ch, cw, ip(ih), ip(iw), None, ip(mc), ip(fw), ip(fh), n, 8) == 0
        assert f(ch, cw, ip(ih), ip(iw), ip(mr), ip(mc), ip(fw), ip(fh), 0, 8) == 0
        assert f(ch, cw, ip(ih), ip(iw), ip(mr), ip(mc), ip(fw), ip(fh), 17, 8) == 0
        zero = i32([0] * n)
        assert f(ch, cw, ip(zero), ip(iw), ip(mr), ip(mc), ip(fw), ip(fh), n, 8) == 0


def test_the_symbols_are_exported_and_bound(native):
    for name in ("apap_box_blur", "apap_box_blur_device", "apap_panorama_band", "apap_panorama_band_device",
                 "apap_panorama_band_workspace_bytes"):
        assert name in native.SIGNATURES
        f = getattr(native.lib(), name)
        restype, argtypes = native.SIGNATURES[name]
        assert f.restype is restype and list(f.argtypes) == list(argtypes), name
    assert native.PANORAMA_BAND == 3
    assert native.lib().apap_abi_version() == 6


def test_no_cpu_fallback(native):
    if native.lib().apap_device_count() > 0:
        pytest.skip("a GPU is visible")
    from cvx_proj_amd import apap
    case = E.get("shared")
    for band, gain_q in ((0, None), (8, None), (32, [4096, 5000, 3000])):
        with pytest.raises(native.ApapError) as e:
            native.panorama(case["center"], case["layers"], blend="band", band=band, gain_q=gain_q)
        assert e.value.code == native.ERR_NO_DEVICE
    for gain in (None, "auto"):
        with pytest.raises(native.ApapError) as e:
            apap.panorama(case["center"], case["layers"], blend="band", gain=gain)
        assert e.value.code == native.ERR_NO_DEVICE
    for radius in (0, 3):
        with pytest.raises(native.ApapError) as e:
            native.box_blur(case["center"], radius)
        assert e.value.code == native.ERR_NO_DEVICE


def test_the_clamp_input_leaves_the_range_on_both_sides():
    case = BC.clamp()
    assert set(np.unique(case["center"]).tolist()) == {1, 255}
    assert (case["layers"][0].img == 255).all() and (case["layers"][1].img == 1).all()
    for band in (1, 8):
        got = P.compose_band(case["center"], case["layers"], case["geometries"], case["coords"], 8, band)
        over, under = int((got.raw > 255).sum()), int((got.raw < 0).sum())
        print(f"clamp, band {band}: {over} channel values above 255, {under} below 0, raw {got.raw.min()} .. {got.raw.max()}")
        assert over > 0 and under > 0 and (got.count == 2).any()
        assert got.canvas.max() == 255 and got.canvas[got.count > 0].min() == 0


def test_the_tie_inputs_tie():
    """All 17 views with one D on the saturation input - the centre must give the detail -, and two layers with one D where
    the centre is absent - the first must."""
    case = RC.saturation()
    got = P.compose_band(case["center"], case["layers"], case["geometries"], case["coords"], 256, 32)
    assert got.tied.max() == 17 and (got.source[got.tied == 17] == 0).all()
    case = BC.layer_ties()
    got = P.compose_band(case["center"], case["layers"], case["geometries"], case["coords"], 8, 8)
    layers_only = (got.tied == 2) & (got.count == 2) & (got.source == 1)
    c, _, _ = P.views(case["center"], case["layers"], case["geometries"], case["coords"], 8)
    assert layers_only.sum() > 50 and not c[0][layers_only].any(), "the centre is absent there"
    assert not (got.source == 2).any()


def test_the_white_saturation_input_fills_the_low_sums():
    case = RC.saturation(white=True)
    got = P.compose_band(case["center"], case["layers"], case["geometries"], case["coords"], 256, 32)
    assert got.wsum.max() == 4352 and got.total.max() == 1109760
    assert (got.canvas[got.count > 0] == 255).all()
