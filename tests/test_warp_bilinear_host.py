"""CPU checks of bilinear sampling (DESIGN.md "Bilinear sampling"): the numpy specification against the definitions the
project already holds (the truncating sampler, ``image_warp_spec.sample``), what the built inputs of
tests/warp_bilinear_cases.py reach - conditions on the inputs, from the specification alone -, the context option, and the
``sampling=`` keyword of every Python surface.  tests/test_gpu_warp_bilinear.py holds the kernels to the specification."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import image_warp_spec as I
import warp_bilinear_cases as C
import warp_bilinear_spec as S
import warp_integer_cases as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def random_picture(seed, h, w):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def test_integer_coordinates_give_the_truncating_sampler():
    """Where tx and ty are integers both samplers give the same byte - on a grid of integer coordinates that runs over both
    borders, and on the integer-translation cases of tests/warp_integer_cases.py."""
    src = random_picture(1, 9, 13)
    ty, tx = np.meshgrid(np.arange(-2.0, 12.0), np.arange(-2.0, 16.0), indexing="ij")
    assert np.array_equal(S.sample(src, tx, ty), S.truncate(src, tx, ty))
    assert S.sample(src, tx, ty).any(axis=-1).sum() > 50
    for name in ("integers_a", "integers_b"):
        c = W.get(name)
        tx, ty = c["coords"]
        assert (tx == np.floor(tx)).all() and (ty == np.floor(ty)).all()
        assert np.array_equal(S.sample(c["img"], tx, ty), S.truncate(c["img"], tx, ty)), name


def test_interior_pixels_are_the_cv_definition():
    """On pixels whose four taps lie inside the source the spec is ``image_warp_spec.sample`` at X = rint(32 tx), Y alike."""
    rng = np.random.default_rng(2)
    src = random_picture(3, 21, 17)
    tx, ty = rng.random((40, 50)) * 20.0 - 1.5, rng.random((40, 50)) * 24.0 - 1.5
    tx[::7, ::5] = np.round(tx[::7, ::5] * 64.0) / 64.0 + 1 / 64        # ties of rint among them
    ok = S.present(tx, ty, 17, 21)
    X, Y = S.fixed(tx, ok), S.fixed(ty, ok)
    assert np.array_equal(X[ok], np.rint(32.0 * tx[ok]).astype(np.int64))
    inner = ok & ((X >> 5) + 1 <= 16) & ((Y >> 5) + 1 <= 20)
    assert inner.sum() > 1000 and (ok & ~inner).sum() > 20 and (~ok).sum() > 50
    assert ((32.0 * tx[inner]) % 1.0 == 0.5).sum() > 5
    got, cv = S.sample(src, tx, ty), I.sample(src, X, Y)
    assert np.array_equal(got[inner], cv[inner])
    assert not got[~ok].any()
    rim = ok & ~inner & ((X & 31) != 0) & ((Y & 31) != 0)
    assert (got[rim] != cv[rim]).any(), "the border is replicated here and zero there"


def test_a_constant_picture_stays_constant():
    """The four weights sum to 1024, and the border is replicated: every present pixel of a constant picture has its value."""
    rng = np.random.default_rng(4)
    tx, ty = rng.random((30, 30)) * 9.0 - 1.0, rng.random((30, 30)) * 6.0 - 1.0
    for value in (255, 1, (7, 0, 200)):
        src = np.empty((5, 8, 3), np.uint8)
        src[...] = value
        out = S.sample(src, tx, ty)
        ok = S.present(tx, ty, 8, 5)
        assert ok.sum() > 300 and (out[ok] == src[0, 0]).all() and not out[~ok].any()


def test_the_last_sixty_fourth_lands_on_the_last_column():
    """tx in [w - 1/64, w): X = 32 w, first tap min(w, w - 1) = w - 1 with weight 32 - 0 - the last column's value."""
    src = random_picture(5, 4, 6)
    tx = np.array([[6 - 1 / 64, 6 - 1 / 128, np.nextafter(6.0, 0.0), 6.0, 5.5]])
    ty = np.full_like(tx, 2.0)
    ok = S.present(tx, ty, 6, 4)
    assert ok.tolist() == [[True, True, True, False, True]]
    assert S.fixed(tx, ok).tolist() == [[192, 192, 192, 0, 176]]
    out = S.sample(src, tx, ty)
    assert (out[0, :3] == src[2, 5]).all() and not out[0, 3].any() and (out[0, 4] == src[2, 5]).all()
    assert (S.sample(src, ty, np.full_like(tx, 4 - 1 / 64))[0, 0] == src[3, 2]).all()       # Y = 32 h


def test_built_inputs_reach_their_edges():
    r = {n: C.reaches(C.get(n)) for n in C.BUILT}
    for n in C.BUILT:
        assert r[n]["present"] > 1500 and r[n]["absent"] > 300, n
    t = r["ties"]
    assert min(t["tie_x_down"], t["tie_x_up"], t["tie_y_down"], t["tie_y_up"]) > 500, "exact ties, the even neighbour on both sides"
    assert t["tie_x_down"] + t["tie_x_up"] == t["present"] == t["tie_y_down"] + t["tie_y_up"], "every present pixel is a tie in x and y"
    for n in ("ties_plus", "ties_minus"):
        assert r[n]["tie_x_down"] + r[n]["tie_x_up"] + r[n]["tie_y_down"] + r[n]["tie_y_up"] == 0, n
    # 2^-20 to either side of the tie: the neighbour above, the neighbour below
    ok = S.present(*C.get("ties")["coords"], 60, 34)
    for axis in (0, 1):
        up = S.fixed(C.get("ties_plus")["coords"][axis], ok)
        down = S.fixed(C.get("ties_minus")["coords"][axis], ok)
        assert (up[ok] - down[ok] == 1).all()
    assert r["rim_a"]["x_is_32w"] > 30 and r["rim_a"]["y_last"] > 30
    assert r["rim_b"]["x_is_32w"] > 30 and r["rim_b"]["y_is_32h"] > 30
    assert r["rim_c"]["x_last"] > 30 and r["rim_c"]["clamped"] > 30 and r["rim_c"]["y_is_32h"] > 30
    for n in ("rim_a", "rim_b", "rim_c"):
        assert r[n]["x_first"] > 30 and r[n]["y_first"] > 30, n
    # the tiling: one lane's four pixels (canvas columns 32 .. 35) in three cells, cell-row edges inside a strip of 2 and of 4 rows
    from oracle import apap_oracle as O
    cc, cr = O.cell_lookup(C.FINAL[0], np.asarray(C.MESH_W)), O.cell_lookup(C.FINAL[1], np.asarray(C.MESH_H))
    assert len(set(cc[32:36])) == 3
    assert cr[12] != cr[13] and 12 % C.STRIP_ROWS == 0 and cr[26] != cr[27] and 26 % C.STRIP_ROWS == 0
    # a bilinear canvas that differs from the truncating one on most present pixels (not where both weights round to 0: the
    # cells with k = 0): the tests can tell the samplers apart
    c = C.get("ties")
    differ = (S.sample(c["img"], *c["coords"]) != S.truncate(c["img"], *c["coords"])).any(axis=-1)
    assert differ.sum() > 0.5 * r["ties"]["present"]


def test_the_option(native):
    lib = native.lib()
    v = ctypes.c_int(-1)
    assert lib.apap_ctx_get_option(None, native.OPT_WARP_SAMPLING, ctypes.byref(v)) == native.OK and v.value == 0
    assert native.OPT_WARP_SAMPLING == 14 and (native.SAMPLING_NEAREST, native.SAMPLING_BILINEAR) == (0, 1)
    assert lib.apap_abi_version() == native.ABI_VERSION == 6
    ctx = native.Context()
    try:
        assert ctx.get("warp_sampling") == 0
        assert ctx.set("warp_sampling", 1).get("warp_sampling") == 1
        for bad in (2, -1):
            with pytest.raises(ValueError):
                ctx.set("warp_sampling", bad)
            assert lib.apap_ctx_set_option(native._h(ctx), native.OPT_WARP_SAMPLING, bad) == native.ERR_INVALID_ARG
        assert ctx.get("warp_sampling") == 1
        assert ctx.set("warp_sampling", 0).get("warp_sampling") == 0
        # the last option of the table: the one after it is refused
        assert lib.apap_ctx_get_option(native._h(ctx), native.OPT_WARP_SAMPLING + 1, ctypes.byref(v)) == native.ERR_INVALID_ARG
        assert lib.apap_ctx_set_option(native._h(ctx), native.OPT_WARP_SAMPLING + 1, 0) == native.ERR_INVALID_ARG
    finally:
        ctx.close()
    c = native.Context(warp_sampling=1)         # the constructor's name
    assert c.get("warp_sampling") == 1
    c.close()


def test_a_keyword_leaves_the_context_as_it_found_it(native):
    for start in (0, 1):
        ctx = native.Context(warp_sampling=start)
        try:
            for word, value in (("bilinear", 1), ("nearest", 0)):
                with native.sampling_scope(ctx, word, "test") as inner:
                    assert inner is ctx and ctx.get("warp_sampling") == value
                assert ctx.get("warp_sampling") == start
            with native.sampling_scope(ctx, None, "test") as inner:
                assert inner is ctx and ctx.get("warp_sampling") == start
            with pytest.raises(RuntimeError):
                with native.sampling_scope(ctx, "bilinear", "test"):
                    raise RuntimeError("inside")
            assert ctx.get("warp_sampling") == start
        finally:
            ctx.close()
    with native.sampling_scope(None, "bilinear", "test") as inner:
        assert isinstance(inner, native.Context) and inner.get("warp_sampling") == 1
    assert inner.handle is None, "a context made for the call is closed with it"
    with native.sampling_scope(None, None, "test") as inner:
        assert inner is None


def test_header_and_binding_agree(native):
    text = open(os.path.join(ROOT, "include", "apap_hip.h")).read()
    defs = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define (APAP_(?:OPT|SAMPLING)_[A-Z0-9_]+) (\d+)", text)}
    assert defs["APAP_OPT_WARP_SAMPLING"] == native.OPT_WARP_SAMPLING == 14
    assert defs["APAP_OPT_COUNT"] == 15 == len(native.Context._NAMES) == len(set(native.Context._NAMES.values()))
    assert defs["APAP_SAMPLING_NEAREST"] == native.SAMPLINGS["nearest"] == 0
    assert defs["APAP_SAMPLING_BILINEAR"] == native.SAMPLINGS["bilinear"] == 1
    for name, value in defs.items():
        if name.startswith("APAP_OPT_") and name != "APAP_OPT_COUNT":
            assert getattr(native, name[5:]) == value, name
    assert re.search(r"#define APAP_ABI_VERSION 6\b", text)
    # every default through the NULL context, the new one included
    v = ctypes.c_int(-1)
    for k in range(defs["APAP_OPT_COUNT"]):
        assert native.lib().apap_ctx_get_option(None, k, ctypes.byref(v)) == native.OK


def _surfaces(native):
    """(name, call) of every Python surface with the keyword; each call passes ``sampling`` and otherwise arguments that
    would fail later - the ValueError must come first, before any device (or torch) is touched."""
    from cvx_proj_amd import apap, pipeline
    img = np.zeros((4, 4, 3), np.uint8)
    H = np.tile(np.eye(3, dtype=np.float32), (1, 1, 1, 1))
    mesh = (np.array([0.0, 4.0]), np.array([0.0, 4.0]))
    eng = apap.APAP(0.5, 100.0, [4, 4], [0, 0])
    layer = apap.PanoramaLayer(img, H, mesh, (4, 4), (0, 0))
    out = [
        ("_native.local_warp", lambda s: native.local_warp(img, H, mesh[0], mesh[1], 4, 4, 0, 0, sampling=s)),
        ("_native.local_stitch", lambda s: native.local_stitch(img, img, H, mesh[0], mesh[1], 4, 4, 0, 0, sampling=s)),
        ("_native.panorama", lambda s: native.panorama(img, [layer], sampling=s)),
        ("APAP.local_warp", lambda s: eng.local_warp(img, H, mesh, sampling=s)),
        ("APAP.local_stitch", lambda s: eng.local_stitch(img, img, H, mesh, sampling=s)),
        ("apap.panorama", lambda s: apap.panorama(img, [layer], sampling=s)),
        ("apap.run_pair", lambda s: apap.run_pair(None, None, None, None, None, sampling=s)),
        ("apap.run_pair_by_calls", lambda s: apap.run_pair_by_calls(None, None, None, None, None, sampling=s)),
        ("Pipeline.run_pair", lambda s: pipeline.Pipeline.run_pair(None, None, None, None, None, None, sampling=s)),
    ]
    try:
        import torch  # noqa: F401
        from cvx_proj_amd import resident
    except ImportError:
        return out
    out += [
        ("resident.hip_warp_batch", lambda s: resident.hip_warp_batch(None, None, None, None, 4, 4, 0, 0, (1, 1), sampling=s)),
        ("resident.hip_warp_rows", lambda s: resident.hip_warp_rows(None, None, None, None, 4, 4, 0, 0, 0, 4, None, (1, 1), sampling=s)),
        ("WarpPlan.gather", lambda s: resident.WarpPlan.gather(None, None, sampling=s)),
        ("resident.hip_panorama", lambda s: resident.hip_panorama(None, [layer], sampling=s)),
    ]
    return out


def test_every_surface_refuses_an_unknown_sampling(native):
    surfaces = _surfaces(native)
    assert len(surfaces) >= 9
    for name, call in surfaces:
        for bad in ("cubic", "", 1, True, b"bilinear"):
            with pytest.raises(ValueError, match="sampling"):
                call(bad)
    for name, fn in (("local_warp", native.local_warp), ("local_stitch", native.local_stitch), ("panorama", native.panorama)):
        assert inspect.signature(fn).parameters["sampling"].default is None, name


def test_command_line_has_the_choice():
    from cvx_proj_amd import apap
    with pytest.raises(SystemExit):
        apap.main(["--synth", "C1", "--sampling", "cubic"])
