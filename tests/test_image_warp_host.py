"""The global warp and blend without a GPU: the specification (tests/image_warp_spec.py) against the fixture made by the
reference's own image_warping (tests/golden/image_warp_ref.npz), the host-only apap_image_warp_bounds against both, and the
argument checks of every new entry point - refused before any device is touched."""
import ctypes as C

import numpy as np
import pytest

import image_warp_spec as S

NAMES = ("neg_f64", "pos_f32", "persp_f64", "persp_f32")


@pytest.fixture(scope="module")
def ref(golden):
    return golden("image_warp_ref")


def test_fixture_holds_the_cases_the_definition_names(ref):
    assert tuple(ref["names"]) == NAMES
    base, src = ref["base"], ref["src"]
    assert base.shape == (40, 50, 3) and src.shape == (37, 45, 3) and base.dtype == src.dtype == np.uint8
    assert ref["H_neg_f64"].dtype == np.float64 and ref["H_pos_f32"].dtype == np.float32
    assert ref["H_neg_f64"][0, 2] < 0 and ref["H_neg_f64"][1, 2] < 0 and ref["H_pos_f32"][0, 2] > 0 and ref["H_pos_f32"][1, 2] > 0
    assert ref["H_persp_f64"][2, 0] != 0 and ref["H_persp_f64"][2, 1] != 0
    nz = (src != 0).sum(axis=-1)
    assert (nz == 0).sum() >= 80 and (nz == 1).sum() >= 80          # black pixels, pixels with exactly one non-zero channel
    assert ((nz == 1) & (src.max(axis=-1) == 1)).sum() >= 10        # ... some of value 1
    for name in NAMES:
        d, m = ref[f"direct_{name}"], ref[f"mean_{name}"]
        xmin, ymin, xmax, ymax = ref[f"bounds_{name}"]
        assert d.shape == m.shape == (ymax - ymin, xmax - xmin, 3)
        assert np.array_equal(d[-ymin:-ymin + 40, -xmin:-xmin + 50], base)      # the paste
        inside = np.zeros(d.shape[:2], bool)
        inside[-ymin:-ymin + 40, -xmin:-xmin + 50] = True
        assert np.array_equal(d[~inside], m[~inside]) and not np.array_equal(d, m)
        # the black block of the source lies inside the base rectangle somewhere: the mean blend took the base there
        warped = S.warp_perspective(src, ref[f"M_{name}"], (xmax - xmin, ymax - ymin))
        black = inside & ~warped.any(axis=-1)
        assert black.sum() >= 40 and np.array_equal(m[black], d[black])


@pytest.mark.parametrize("name", NAMES)
def test_specification_reproduces_the_fixture(ref, name):
    base, src, H = ref["base"], ref["src"], ref[f"H_{name}"]
    assert S.bounds(40, 50, 37, 45, H) == tuple(int(v) for v in ref[f"bounds_{name}"])
    xmin, ymin = (int(v) for v in ref[f"bounds_{name}"][:2])
    M = S.matrix(H, [-xmin, -ymin])
    assert M.dtype == np.float64 and np.array_equal(M, ref[f"M_{name}"])
    assert np.array_equal(S.image_warping(base, src, H, True), ref[f"direct_{name}"])
    assert np.array_equal(S.image_warping(base, src, H, False), ref[f"mean_{name}"])
    # a float32 H and the same H as float64 are one problem
    assert np.array_equal(S.image_warping(base, src, H.astype(np.float64), False), ref[f"mean_{name}"])


def test_integer_weights_equal_opencvs_15_bit_form():
    """(sum(32 w p) + 2^14) >> 15 == (sum(w p) + 512) >> 10 for every weight pair: OpenCV's table holds w15 = 32 w exactly."""
    rng = np.random.default_rng(5)
    ax, ay = np.meshgrid(np.arange(32, dtype=np.int64), np.arange(32, dtype=np.int64))
    w = np.stack([(32 - ax) * (32 - ay), ax * (32 - ay), (32 - ax) * ay, ax * ay], axis=-1)        # (32, 32, 4)
    assert (w.sum(axis=-1) == 1024).all()
    p = rng.integers(0, 256, (64, 32, 32, 4), dtype=np.int64)
    p[0], p[1] = 255, 0
    p[2] = np.array([255, 0, 0, 255])
    p[3] = np.array([1, 0, 0, 0])
    assert np.array_equal(((32 * w * p).sum(axis=-1) + 16384) >> 15, ((w * p).sum(axis=-1) + 512) >> 10)


def _bounds(native, h1, w1, h2, w2, H):
    H = np.ascontiguousarray(H, dtype=np.float64)
    out = np.full(4, -99, np.int32)
    rc = native.lib().apap_image_warp_bounds(h1, w1, h2, w2, native._ptr(H, C.c_double), native._ptr(out, C.c_int))
    return rc, tuple(int(v) for v in out)


def test_bounds_match_specification_and_fixture(native, ref):
    for name in NAMES:
        H = ref[f"H_{name}"]
        assert native.image_warp_bounds(40, 50, 37, 45, H) == tuple(int(v) for v in ref[f"bounds_{name}"]) == S.bounds(40, 50, 37, 45, H)
    rng = np.random.default_rng(11)
    for k in range(200):
        H = np.eye(3) + rng.normal(0, [[0.2, 0.2, 30.0], [0.2, 0.2, 30.0], [2e-3, 2e-3, 0.0]])
        if k % 2:
            H = H.astype(np.float32)
        h1, w1, h2, w2 = (int(v) for v in rng.integers(1, 90, 4))
        try:
            want = S.bounds(h1, w1, h2, w2, H)
        except (ValueError, OverflowError):
            want = None
        if want is None or not (1 <= want[2] - want[0] <= 32767 and 1 <= want[3] - want[1] <= 32767):
            with pytest.raises(ValueError):
                native.image_warp_bounds(h1, w1, h2, w2, H)
        else:
            assert native.image_warp_bounds(h1, w1, h2, w2, H) == want, (k, H)
            M, cw, ch, tx, ty = native.image_warp_geometry(h1, w1, h2, w2, H)
            assert (cw, ch, tx, ty) == (want[2] - want[0], want[3] - want[1], -want[0], -want[1])
            assert M.dtype == np.float64 and np.array_equal(M, S.matrix(H, [tx, ty]))
            assert tx >= 0 and ty >= 0 and tx + w1 <= cw and ty + h1 <= ch       # the base rectangle lies inside the canvas


def test_bounds_at_float32_halves_negative_w_and_zero_w(native):
    # corners that land exactly on k + 0.5 in float32: min - 0.5 and max + 0.5 are then integers, truncation keeps them
    H = np.array([[1.0, 0.0, -3.5], [0.0, 1.0, -2.5], [0.0, 0.0, 1.0]])
    assert S.perspective_transform(np.float32([[[0, 0]], [[10, 8]]]), H).tolist() == [[[-3.5, -2.5]], [[6.5, 5.5]]]
    assert native.image_warp_bounds(4, 5, 8, 10, H) == S.bounds(4, 5, 8, 10, H) == (-4, -3, 7, 6)
    H = np.array([[1.0, 0.0, 3.5], [0.0, 1.0, 2.5], [0.0, 0.0, 1.0]])
    assert native.image_warp_bounds(4, 5, 8, 10, H) == S.bounds(4, 5, 8, 10, H) == (0, 0, 14, 11)
    # ... and just beside a half: float32(-3.5 -+ 2^-22) - 0.5 rounds in float32 before it is truncated
    for eps in (-2.0 ** -22, 2.0 ** -22, -2.0 ** -30, 2.0 ** -30):
        H = np.array([[1.0, 0.0, -3.5 + eps], [0.0, 1.0, 2.5 + eps], [0.0, 0.0, 1.0]])
        assert native.image_warp_bounds(4, 5, 8, 10, H) == S.bounds(4, 5, 8, 10, H), eps
    # a negative w: the source is mirrored through the origin, 1 / w keeps its sign
    H = np.array([[1.0, 0.0, 2.0], [0.0, 1.0, 1.0], [0.0, 0.0, -1.0]])
    assert native.image_warp_bounds(4, 5, 8, 10, H) == S.bounds(4, 5, 8, 10, H) == (-12, -9, 5, 4)
    # w == 0 exactly at a corner: that corner goes to (0, 0) (w = w ? 1 / w : 0), no division by zero
    H = np.array([[1.0, 0.0, 2.0], [0.0, 1.0, 1.0], [-0.1, 0.0, 1.0]])          # w = 1 - 0.1 x: exactly 0 at x = 10
    w = S._f64_3x3(H)[2, 0] * 10.0 + 1.0
    assert w == 0.0
    assert native.image_warp_bounds(4, 5, 8, 10, H) == S.bounds(4, 5, 8, 10, H) == (0, 0, 5, 9)
    H = np.zeros((3, 3))                                                         # w == 0 everywhere: all four corners at the origin
    assert native.image_warp_bounds(4, 5, 8, 10, H) == S.bounds(4, 5, 8, 10, H) == (0, 0, 5, 4)


def test_bounds_refuses_bad_arguments(native):
    eye = np.eye(3)
    out = np.zeros(4, np.int32)
    lib = native.lib()
    assert lib.apap_image_warp_bounds(4, 5, 8, 10, None, native._ptr(out, C.c_int)) == native.ERR_INVALID_ARG
    assert lib.apap_image_warp_bounds(4, 5, 8, 10, native._ptr(eye, C.c_double), None) == native.ERR_INVALID_ARG
    for shape in ((0, 5, 8, 10), (4, 0, 8, 10), (4, 5, 0, 10), (4, 5, 8, 0), (32768, 5, 8, 10), (4, 32768, 8, 10), (4, 5, 32768, 10),
                  (4, 5, 8, 32768)):
        assert _bounds(native, *shape, eye)[0] == native.ERR_INVALID_ARG, shape
    assert _bounds(native, 32767, 32767, 32767, 32767, eye) == (native.OK, (0, 0, 32767, 32767))
    # a wild H must not be given a canvas: a side beyond 32767, a corner beyond int32, a non-finite corner
    for H in (np.diag([1e3, 1.0, 1.0]), np.diag([1e12, 1.0, 1.0]), np.diag([1e300, 1e300, 1e-300]), np.diag([np.nan, 1.0, 1.0]),
              np.array([[1.0, 0, np.inf], [0, 1.0, 0], [0, 0, 1.0]]), np.array([[1.0, 0, -40000.0], [0, 1.0, 0], [0, 0, 1.0]])):
        rc, _ = _bounds(native, 40, 50, 37, 45, H)
        assert rc == native.ERR_INVALID_ARG, H
        with pytest.raises(ValueError):
            native.image_warp_bounds(40, 50, 37, 45, H)


class Call:
    """One valid problem of the batch entry points as ctypes arguments, with single fields replaced."""

    def __init__(self, native, n=1, **over):
        self.native = native
        self.n = n
        self.base = np.zeros((6, 7, 3), np.uint8)
        self.src = np.zeros((5, 9, 3), np.uint8)
        f = dict(base_h=[6] * n, base_w=[7] * n, src_h=[5] * n, src_w=[9] * n, M=[np.eye(3)] * n, canvas_w=[12] * n, canvas_h=[10] * n,
                 off_x=[2] * n, off_y=[3] * n, direct=[1] * n, out_offset=[k * 360 for k in range(n)],
                 bases=[self.base.ctypes.data] * n, srcs=[self.src.ctypes.data] * n)
        f.update(over)
        self.f = f
        self.out = np.zeros(360 * max(n, 1) + 64, np.uint8)

    def args(self):
        f, nat = self.f, self.native
        self.keep = keep = {}
        for k in ("base_h", "base_w", "src_h", "src_w", "canvas_w", "canvas_h", "off_x", "off_y", "direct"):
            keep[k] = None if f[k] is None else np.ascontiguousarray(f[k], dtype=np.int32)
        keep["M"] = None if f["M"] is None else np.ascontiguousarray(np.stack(f["M"]), dtype=np.float64)
        keep["out_offset"] = None if f["out_offset"] is None else np.ascontiguousarray(f["out_offset"], dtype=np.int64)
        ip = lambda k: nat._ptr(keep[k], C.c_int)      # noqa: E731
        vpp = lambda v: None if v is None else (C.c_void_p * max(len(v), 1))(*v)      # noqa: E731
        return dict(bases=vpp(f["bases"]), base_h=ip("base_h"), base_w=ip("base_w"), srcs=vpp(f["srcs"]), src_h=ip("src_h"),
                    src_w=ip("src_w"), M=nat._ptr(keep["M"], C.c_double), canvas_w=ip("canvas_w"), canvas_h=ip("canvas_h"),
                    off_x=ip("off_x"), off_y=ip("off_y"), direct=ip("direct"), out_offset=nat._ptr(keep["out_offset"], C.c_longlong))

    def host(self, out="self", n=None):
        a = self.args()
        out = self.native._ptr(self.out, C.c_uint8) if out == "self" else out
        return self.native.lib().apap_image_warp_batch(None, a["bases"], a["base_h"], a["base_w"], a["srcs"], a["src_h"], a["src_w"], a["M"],
                                                       a["canvas_w"], a["canvas_h"], a["off_x"], a["off_y"], a["direct"],
                                                       self.n if n is None else n, out, a["out_offset"], -1)

    def device(self, d_out=0x10000, d_work=0x20000, work_bytes=None, n=None):
        """The resident form with made-up device addresses: every check comes before a device is touched, so they are never
        dereferenced."""
        a = self.args()
        n = self.n if n is None else n
        if work_bytes is None:
            work_bytes = self.native.lib().apap_image_warp_workspace_bytes(max(n, 1))
        return self.native.lib().apap_image_warp_batch_device(None, a["bases"], a["base_h"], a["base_w"], a["srcs"], a["src_h"], a["src_w"],
                                                              a["M"], a["canvas_w"], a["canvas_h"], a["off_x"], a["off_y"], a["direct"], n,
                                                              d_out, a["out_offset"], d_work, work_bytes, None, None)


SINGULAR = np.array([[1.0, 2.0, 3.0], [2.0, 4.0, 6.0], [0.0, 1.0, 1.0]])
BAD_FIELDS = [
    ("base_h", [0]), ("base_w", [0]), ("src_h", [0]), ("src_w", [0]), ("canvas_w", [0]), ("canvas_h", [0]),
    ("base_h", [32768]), ("base_w", [32768]), ("src_h", [32768]), ("src_w", [32768]), ("canvas_w", [32768]), ("canvas_h", [32768]),
    ("M", [SINGULAR]), ("M", [np.zeros((3, 3))]), ("M", [np.diag([np.nan, 1.0, 1.0])]), ("M", [np.diag([np.inf, 1.0, 1.0])]),
    ("M", [np.diag([1e-200, 1e-200, 1e-200])]),                 # det underflows to 0
    ("off_x", [6]), ("off_y", [5]), ("off_x", [-1]), ("off_y", [-1]),       # the 6 x 7 base does not fit the 10 x 12 canvas there
    ("canvas_w", [6]), ("canvas_h", [5]),                       # a canvas smaller than the base picture
    ("direct", [2]), ("direct", [-1]), ("out_offset", [-1]),
    ("base_h", None), ("base_w", None), ("src_h", None), ("src_w", None), ("M", None), ("canvas_w", None), ("canvas_h", None),
    ("off_x", None), ("off_y", None), ("direct", None), ("out_offset", None), ("bases", None), ("srcs", None), ("bases", [0]), ("srcs", [0]),
]


@pytest.mark.parametrize("field,value", BAD_FIELDS, ids=[f"{k}-{i}" for i, (k, _) in enumerate(BAD_FIELDS)])
def test_batch_forms_refuse_bad_arguments_before_a_device_is_touched(native, field, value):
    for form in ("host", "device"):
        c = Call(native, **{field: value})
        assert getattr(c, form)() == native.ERR_INVALID_ARG, (form, field)
        assert native.last_error().startswith("apap_image_warp_batch")


def test_batch_forms_refuse_counts_offsets_and_workspaces(native):
    lib = native.lib()
    assert lib.apap_image_warp_workspace_bytes(0) == 0 and lib.apap_image_warp_workspace_bytes(-1) == 0
    assert lib.apap_image_warp_workspace_bytes(65536) == 0
    assert lib.apap_image_warp_workspace_bytes(1) == 256 and lib.apap_image_warp_workspace_bytes(2) == 512
    assert lib.apap_image_warp_workspace_bytes(65535) == (65535 * 144 + 255) // 256 * 256
    for n in (0, -1, 65536):
        assert Call(native).host(n=n) == native.ERR_INVALID_ARG
        assert Call(native).device(n=n) == native.ERR_INVALID_ARG
    assert Call(native).host(out=None) == native.ERR_INVALID_ARG
    assert Call(native).device(d_out=None) == native.ERR_INVALID_ARG
    assert Call(native).device(d_work=None) == native.ERR_INVALID_ARG
    assert Call(native).device(d_work=0x20010) == native.ERR_INVALID_ARG          # misaligned
    assert Call(native).device(work_bytes=255) == native.ERR_WORKSPACE and "workspace" in native.last_error()
    assert Call(native, n=2).device(work_bytes=256) == native.ERR_WORKSPACE
    # two canvases that overlap in the output buffer; the second problem is the one that is wrong
    assert Call(native, n=2, out_offset=[0, 359]).host() == native.ERR_INVALID_ARG and "overlap" in native.last_error()
    assert Call(native, n=2, out_offset=[400, 41]).device() == native.ERR_INVALID_ARG
    assert Call(native, n=2, canvas_w=[12, 0]).host() == native.ERR_INVALID_ARG and "problem 1" in native.last_error()
    assert Call(native, n=2, M=[np.eye(3), SINGULAR]).device() == native.ERR_INVALID_ARG and "problem 1" in native.last_error()


def test_single_forms_refuse_bad_arguments(native):
    lib = native.lib()
    base, src, out = np.zeros((6, 7, 3), np.uint8), np.zeros((5, 9, 3), np.uint8), np.zeros((10, 12, 3), np.uint8)
    M = np.eye(3)
    u8, f64 = (lambda a: native._ptr(a, C.c_uint8)), (lambda a: native._ptr(a, C.c_double))

    def host(b=base, s=src, m=M, o=out, h1=6, w1=7, h2=5, w2=9, cw=12, ch=10, ox=2, oy=3, direct=1):
        return lib.apap_image_warp(None, u8(b), h1, w1, u8(s), h2, w2, f64(m), cw, ch, ox, oy, direct, u8(o), -1)

    def device(b=0x1000, s=0x2000, m=M, o=0x3000, work=0x4000, wb=256, h1=6, w1=7, h2=5, w2=9, cw=12, ch=10, ox=2, oy=3, direct=1):
        return lib.apap_image_warp_device(None, b, h1, w1, s, h2, w2, f64(m), cw, ch, ox, oy, direct, o, work, wb, None, None)

    for call in (host, device):
        for kw in (dict(b=None), dict(s=None), dict(m=None), dict(o=None), dict(h1=0), dict(w1=32768), dict(h2=32768), dict(w2=0),
                   dict(cw=0), dict(ch=32768), dict(ox=6), dict(oy=5), dict(ox=-1), dict(direct=3), dict(m=SINGULAR),
                   dict(m=np.diag([1.0, np.nan, 1.0]))):
            assert call(**kw) == native.ERR_INVALID_ARG, (call.__name__, kw)
    assert device(work=None) == native.ERR_INVALID_ARG and device(wb=128) == native.ERR_WORKSPACE


def test_valid_arguments_need_a_device(native):
    """No CPU fallback: with valid arguments and no GPU the host-buffer forms return APAP_ERR_NO_DEVICE."""
    if native.lib().apap_device_count() > 0:
        pytest.skip("a GPU is visible")
    assert Call(native).host() == native.ERR_NO_DEVICE
    assert Call(native, n=3).host() == native.ERR_NO_DEVICE
    from cvx_proj_amd import utils
    with pytest.raises(native.ApapError) as e:
        utils.image_warping(np.zeros((6, 7, 3), np.uint8), np.zeros((5, 9, 3), np.uint8), np.eye(3))
    assert e.value.code == native.ERR_NO_DEVICE
    with pytest.raises(native.ApapError) as e:
        utils.image_warping_batch([(np.zeros((6, 7, 3), np.uint8), np.zeros((5, 9, 3), np.uint8), np.eye(3, dtype=np.float32), False)] * 2)
    assert e.value.code == native.ERR_NO_DEVICE


def test_python_layer_refuses_wrong_pictures_and_wild_homographies(native):
    from cvx_proj_amd import spectral_method, utils
    ok = np.zeros((6, 7, 3), np.uint8)
    for bad in (np.zeros((6, 7), np.uint8), np.zeros((6, 7, 4), np.uint8), np.zeros((6, 7, 1), np.uint8), np.zeros((6, 7, 3), np.float32),
                np.zeros((6, 7, 3), np.int8), np.zeros((0, 7, 3), np.uint8)):
        for args in ((bad, ok), (ok, bad)):
            with pytest.raises(ValueError):
                utils.image_warping(*args, np.eye(3))
            with pytest.raises(ValueError):
                utils.image_warping_batch([(ok, ok, np.eye(3), True), (*args, np.eye(3), True)])
    for H in (np.eye(4), np.zeros(9), np.diag([1e5, 1.0, 1.0]), np.diag([np.nan, 1.0, 1.0])):
        with pytest.raises(ValueError):
            utils.image_warping(ok, ok, H)
    with pytest.raises(ValueError):
        spectral_method.warp_results(ok, ok, None, np.eye(3))
    with pytest.raises(ValueError):
        native.image_warp_batch([], [], [], [], [], [])


def test_edge_cases_exercise_the_edges_they_are_named_for():
    """tests/test_gpu_image_warp.py cannot pass without meeting these edges: each input of case set E, by the specification."""
    import image_warp_cases as E
    cases = {name: (base, src, H) for name, base, src, H in E.cases()}
    assert len(cases) == len(E.cases())
    geo = {name: E.geometry(*c) for name, c in cases.items()}
    assert all(1 <= g[1] < 200 and 1 <= g[2] < 200 for g in geo.values())
    assert [geo[n][1] % 4 for n in ("width_4k1", "width_4k2", "width_4k3")] == [1, 2, 3] and geo["width_4"][1] == 4
    assert geo["width_base_plus_1"][1] == cases["width_base_plus_1"][0].shape[1] + 1
    assert geo["rows_9"][2] > 8                                                   # three blocks of four rows
    coords = {name: S.fixed_coords(geo[name][0], geo[name][1:3]) for name in cases}
    X, Y = coords["identity"]
    assert not (X & 31).any() and not (Y & 31).any() and ((X >> 5) + 1 == cases["identity"][1].shape[1]).any()
    X, Y = coords["translation_int"]
    assert not (X & 31).any() and not (Y & 31).any() and geo["translation_int"][3:] == (0, 3)
    X, Y = coords["translation_half"]
    assert ((X & 31) == 16).all() and ((Y & 31) == 16).all()
    # half_ties: x / 2 is k + 0.5 in the odd columns, rint takes the even neighbour: X = 0, 0, 1, 2, 2, 3, 4, 4 ...
    M, cw, ch = geo["half_ties"][:3]
    assert np.array_equal(M, np.diag([64.0, 64.0, 1.0])) and (cw, ch) == (192, 128)
    X, _ = coords["half_ties"]
    x = np.arange(cw)
    assert np.array_equal(X[0], np.where(x % 2 == 0, x // 2, (x // 2 + 1) // 2 * 2)) and (X[0, 1], X[0, 3], X[0, 5]) == (0, 2, 2)
    # the W0 = 0 line: exactly zero in canvas column 16, those pixels take src[0, 0]
    M, cw, ch = geo["w0_zero_line"][:3]
    assert np.array_equal(S.invert3(M), [[1, 0, 0], [0, 1, 0], [-0.125, 0, 2]]) and cw > 17 and ch > 20
    X, Y = coords["w0_zero_line"]
    assert not X[:, 16].any() and not Y[:, 16].any() and X[:, 15].all()
    base, src, H = cases["w0_zero_line"]
    assert (S.image_warping(base, src, H, True)[20:, 16] == src[0, 0]).all() and src[0, 0].all()
    # beside the line: the int clamp on both sides, the int16 clamp without the int clamp on both sides
    lo, hi = -2 ** 31, 2 ** 31 - 1
    X = [coords[f"clamp_{k}"][0] for k in range(4)]
    Yc = [coords[f"clamp_{k}"][1] for k in range(4)]
    assert (X[0] == hi).any() and (Yc[0] == hi).any() and (X[1] == lo).any() and (Yc[1] == lo).any()
    assert ((X[2] >> 5 > 32767) & (X[2] < hi)).any() and ((X[3] >> 5 < -32768) & (X[3] > lo)).any()
    assert not (X[2] == hi).any() and not (X[3] == lo).any()
    # blends
    base, src, H = cases["src_black"]
    assert np.array_equal(S.image_warping(base, src, H, False), S.image_warping(base, src, H, True))
    base, src, H = cases["src_one_channel"]
    assert ((src != 0).sum(axis=-1) == 1).all() and src.max() == 1
    d, m = S.image_warping(base, src, H, True), S.image_warping(base, src, H, False)
    tx, ty = geo["src_one_channel"][3:]
    inside = m[ty:ty + base.shape[0], tx:tx + base.shape[1]]
    assert (inside != base).any() and (inside == base >> 1).all(axis=-1).sum() > 20     # where the 1 met an even channel
    base, src, H = cases["base_is_canvas"]
    assert geo["base_is_canvas"][1:] == (base.shape[1], base.shape[0], 0, 0)
    assert np.array_equal(S.image_warping(base, src, H, True), base) and not np.array_equal(S.image_warping(base, src, H, False), base)
    assert cases["H_float32"][2].dtype == np.float32 and cases["H_float64"][2].dtype == np.float64
    assert np.array_equal(geo["H_float32"][0], geo["H_float64"][0])
    for name in ("src_1x1", "src_1x2", "src_2x1"):
        assert S.image_warping(*cases[name], True).any(axis=-1).sum() > cases[name][0].shape[0] * cases[name][0].shape[1] - 40


def test_sweep_reaches_every_residue_of_a_lanes_group():
    """sweep(): what tests/test_gpu_image_warp.py needs of it, by the specification alone."""
    import image_warp_cases as E
    problems = E.sweep()
    assert len(problems) == 80 and len({p[0] for p in problems}) == 80
    pairs = set()
    for direct_p, mean_p in zip(problems[0::2], problems[1::2]):
        _, base, src, M, (cw, ch), (ox, oy), direct = direct_p
        assert direct and not mean_p[6] and all(a is b for a, b in zip(direct_p[1:4], mean_p[1:4])) and direct_p[4:6] == mean_p[4:6]      # one problem, both modes
        assert (cw, ch) == (23, 6) and oy == 2 and base.shape[0] == 3 and src.min() >= 1
        w1 = base.shape[1]
        pairs.add((ox % E.GROUP, (ox + w1) % E.GROUP))
        warped = S.warp_perspective(src, M, (cw, ch))
        # non-zero just left and right of the base rectangle, on its rows: a lane that skipped taps it needs shows black there
        if ox > 0:
            assert warped[oy:oy + 3, ox - 1].any(axis=-1).all()
        assert ox + w1 < cw and warped[oy:oy + 3, ox + w1].any(axis=-1).all()
        assert warped.any(axis=-1).all()
        d, m = E.expected(direct_p), E.expected(mean_p)
        assert np.array_equal(d[oy:oy + 3, ox:ox + w1], base) and not np.array_equal(d, m)
        outside = np.ones((ch, cw), bool)
        outside[oy:oy + 3, ox:ox + w1] = False
        assert np.array_equal(d[outside], warped[outside]) and np.array_equal(m[outside], warped[outside])
    assert pairs == {(a, b) for a in range(4) for b in range(4)}
    # a base picture strictly inside one lane's group of four, and one that straddles a group's boundary at every odd residue
    inside = [(p[5][0], p[1].shape[1]) for p in problems if p[5][0] % 4 >= 1 and p[5][0] % 4 + p[1].shape[1] <= 3]
    assert (1, 1) in inside and (1, 2) in inside and (5, 2) in inside
    assert {p[5][0] % 4 for p in problems if p[5][0] // 4 != (p[5][0] + p[1].shape[1] - 1) // 4} == {0, 1, 2, 3}
    # the fractional translation: no tap weight is zero
    X, Y = S.fixed_coords(problems[0][3], (23, 6))
    assert (X & 31).all() and (Y & 31).all()


def test_tiling_cases_reach_their_edges():
    """tiling_cases(): col_blocks 1 .. 4 in one batch behind first blocks other than 0, widths on both sides of a block's 256
    columns, warped and base pixels on both sides of columns 256 and 512."""
    import image_warp_cases as E
    problems = E.tiling_cases()
    wide = [p for p in problems if p[0].startswith("wide_")]
    assert {p[4] for p in wide} == set(E.WIDE_SHAPES) and len(wide) == 2 * len(E.WIDE_SHAPES)
    assert sorted({p[4][0] for p in wide}) == [255, 256, 257, 511, 512, 513, 769] and {p[4][1] for p in wide} == {3, 4, 5}
    assert {p[4][0] % E.COLS_PER_BLOCK for p in wide} == {255, 0, 1} and {p[4][0] % E.GROUP for p in wide} == {0, 1, 3}
    assert {E.col_blocks(p) for p in wide} == {1, 2, 3, 4} and {p[4][1] % E.ROWS_PER_BLOCK for p in wide} == {0, 1, 3}
    # interleaved: a wide problem never follows a wide one, neighbours differ in col_blocks somewhere, both modes of each
    assert all(a[0].startswith("wide_") != b[0].startswith("wide_") for a, b in zip(problems[:28], problems[1:28]))
    assert [E.col_blocks(p) for p in problems[:28:2]] == [1, 1, 1, 1, 2, 2, 2, 2, 2, 2, 3, 3, 4, 4]
    assert all(E.col_blocks(p) == 1 for p in problems[1::2]) and {p[6] for p in wide} == {True, False}
    assert len({id(p[2]) for p in wide}) == 1 and len({p[3][0, 2] for p in wide}) == len(E.WIDE_SHAPES)     # one source, 7 translations
    for p in wide:
        _, base, src, M, (cw, ch), (ox, oy), direct = p
        assert src.min() >= 1 and oy == 1 and base.shape[0] == 2
        warped = S.warp_perspective(src, M, (cw, ch))
        for col in (255, 256, 257, 511, 512, 513):
            if col < cw:
                assert warped[:, col].any(axis=-1).all(), (p[0], col)
        assert warped[:, cw - 1].any(axis=-1).all() and warped[:, 0].any(axis=-1).all()
        w1 = base.shape[1]
        if cw > 262:
            assert ox == 250 and ox < 256 < ox + w1 - 1                      # the base rectangle straddles column 256
        else:
            assert ox + w1 == cw                                             # ... or ends with the canvas' last column
        if cw == 769:
            assert ox + w1 > 512 + E.GROUP and w1 > E.COLS_PER_BLOCK         # ... and column 512, a whole block's lanes inside it
        got = E.expected(p)
        assert np.array_equal(got[1:3, ox:ox + w1], base) == direct
    # the small problems are set E's, with the specification's geometry; both 1 x 1 pictures close the batch
    by_name = {c[0]: c for c in E.cases()}
    for p in problems[1:28:2]:
        name = p[0].rsplit("_", 1)[0]
        assert name in E.SMALL_IN_WIDE and np.array_equal(E.expected(p), S.image_warping(*by_name[name][1:], p[6]))
    assert [p[0] for p in problems[28:]] == ["both_1x1_direct", "both_1x1_mean"]
    for p in problems[28:]:
        assert p[1].shape == p[2].shape == (1, 1, 3) and np.array_equal(E.expected(p), S.image_warping(*E.tiny_pair(), p[6]))


def test_tiny_pair_shows_both_pictures():
    import image_warp_cases as E
    base, src, H = E.tiny_pair()
    M, cw, ch, ox, oy = E.geometry(base, src, H)
    assert (cw, ch, ox, oy) == (3, 3, 0, 0)
    warped = S.warp_perspective(src, M, (cw, ch))
    assert warped.all() and np.array_equal(warped[0, 0], src[0, 0].astype(np.int64) * 812 + 512 >> 10)
    d, m = S.image_warping(base, src, H, True), S.image_warping(base, src, H, False)
    assert np.array_equal(d[0, 0], base[0, 0]) and np.array_equal(m[0, 0], (base[0, 0].astype(np.int64) + warped[0, 0]) >> 1)
    assert not np.array_equal(d[0, 0], m[0, 0]) and not np.array_equal(m[0, 0], warped[0, 0])


def test_many_problems_differ_from_their_neighbours(native):
    import image_warp_cases as E
    problems = E.many()
    n = len(problems)
    assert n == 521 and all(n % k for k in range(2, 23)) and n > 512
    assert native.lib().apap_image_warp_workspace_bytes(n) == (n * 144 + 255) // 256 * 256 == 75264
    geo = [E.geometry(b, s, H) for b, s, H, _ in problems]
    assert all(5 <= g[1] <= 9 and 5 <= g[2] <= 11 for g in geo)
    assert {g[1] for g in geo} == set(range(5, 10)) and {g[2] for g in geo} == set(range(5, 12))
    assert len({(g[3], g[4]) for g in geo}) >= 9 and len({tuple(H[:2, 2]) for _, _, H, _ in problems}) == n
    assert 200 < sum(d for _, _, _, d in problems) < 321
    want = [S.image_warping(*p) for p in problems]
    assert all(w.any() for w in want)
    for a, b in zip(want, want[1:]):
        assert a.shape != b.shape or not np.array_equal(a, b)
    # the bisection's table: every problem is a handful of blocks, the first blocks all differ
    blocks = [-(-g[1] // E.COLS_PER_BLOCK) * -(-g[2] // E.ROWS_PER_BLOCK) for g in geo]
    assert set(blocks) == {2, 3} and len(set(np.cumsum(blocks))) == n
