"""Bilinear sampling on the GPU (APAP_OPT_WARP_SAMPLING, the ``sampling=`` keyword): k_warp_bilinear behind every warp entry
point and k_panorama's bilinear forms, byte for byte the numpy definition (tests/warp_bilinear_spec.py) over the engine's own
coordinates (``_native.warp_coords``) and, on the small cases, over the oracle's.  There is no tolerance and no excepted pixel.
The inputs are tests/warp_bilinear_cases.py's (tests/test_warp_bilinear_host.py shows on the CPU what they reach) and the
panorama's tiling cases."""
import os
import subprocess
import sys

import numpy as np
import pytest

import panorama_cases as E
import panorama_spec as P
import warp_bilinear_cases as C
import warp_bilinear_spec as S
import warp_integer_cases as W
from oracle import apap_oracle as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", autouse=True)
def need_gpu(native):
    assert native.lib().apap_device_count() >= 1, "these tests need a GPU; the library found none"


def same(got, want, what):
    assert got.dtype == np.uint8 and got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere((got != want).any(axis=-1))
    assert len(bad) == 0, f"{what}: {len(bad)} pixels differ, first at (y, x) = {tuple(bad[0])}: {got[tuple(bad[0])]} != {want[tuple(bad[0])]}"


def engine_coords(native, c):
    xy = native.warp_coords(c["H"], c["mesh"][0], c["mesh"][1], *c["final"])
    return np.ascontiguousarray(xy[..., 0]), np.ascontiguousarray(xy[..., 1])


def oracle_coords(c):
    return O.warp_coords_fast(O.invert_cells_f32(c["H"]), c["mesh"], c["final"][:2], c["final"][2:])


def warp(native, c, **kw):
    return native.local_warp(c["img"], c["H"], c["mesh"][0], c["mesh"][1], *c["final"], **kw)[0]


SEEDED = {
    "perspective_5x4": dict(seed=11, final_w=90, final_h=71, rows=4, cols=5),
    "irregular": dict(seed=12, final_w=101, final_h=67, rows=6, cols=7, irregular=True, offset=(4, 3)),
    "width_255": dict(seed=13, final_w=255, final_h=C.STRIP_ROWS + 1, rows=1, cols=9),
    "width_256": dict(seed=14, final_w=256, final_h=C.STRIP_ROWS * C.WAVES_PER_BLOCK + 1, rows=3, cols=8),
    "width_257": dict(seed=15, final_w=257, final_h=5, rows=2, cols=8),
    "width_2": dict(seed=16, final_w=2, final_h=C.STRIP_ROWS * C.WAVES_PER_BLOCK + 1, rows=2, cols=1, src_wh=(3, 9), offset=(1, 0)),
    "source_2x1": dict(seed=17, final_w=9, final_h=5, rows=1, cols=2, src_wh=(2, 1)),
    "source_1x2": dict(seed=18, final_w=6, final_h=11, rows=2, cols=1, src_wh=(1, 2)),
}


@pytest.mark.parametrize("name", sorted(SEEDED))
def test_seeded(native, name):
    """A 37 x 53 source through a 5 x 4 mesh with mild perspective, an irregular mesh with offsets, canvas widths 255, 256, 257
    and 2 (the block's edge, a partial store group), heights one past a strip and one past a block of strips, sources of 2
    pixels: the spec over the engine's coordinates and over the oracle's; the default and an explicit NEAREST give the
    truncating canvas; the inputs are left as they were."""
    c = C.seeded(**SEEDED[name])
    H0, img0 = c["H"].copy(), c["img"].copy()
    tx, ty = engine_coords(native, c)
    want = S.sample(c["img"], tx, ty)
    assert want.any(axis=-1).mean() > 0.3, "most of the canvas gathers a pixel"
    got = warp(native, c, sampling="bilinear")
    same(got, want, f"{name}: bilinear over the engine's coordinates")
    same(got, S.sample(c["img"], *oracle_coords(c)), f"{name}: bilinear over the oracle's coordinates")
    trunc = S.truncate(c["img"], tx, ty)
    assert (want != trunc).any()
    same(warp(native, c), trunc, f"{name}: default")
    ctx = native.Context()
    try:
        same(warp(native, c, ctx=ctx), trunc, f"{name}: a context that never touched the option")
        ctx.set("warp_sampling", native.SAMPLING_NEAREST)
        same(warp(native, c, ctx=ctx), trunc, f"{name}: NEAREST")
        same(warp(native, c, ctx=ctx, sampling="bilinear"), want, f"{name}: the keyword over a NEAREST context")
        assert ctx.get("warp_sampling") == native.SAMPLING_NEAREST
        ctx.set("warp_sampling", native.SAMPLING_BILINEAR)
        same(warp(native, c, ctx=ctx), want, f"{name}: a BILINEAR context")
        same(warp(native, c, ctx=ctx, sampling="nearest"), trunc, f"{name}: the keyword over a BILINEAR context")
        # the two options that do not apply are ignored
        for rows, fast in ((0, 1), (8, 0)):
            ctx.set("warp_rows", rows).set("warp_fast", fast)
            same(warp(native, c, ctx=ctx), want, f"{name}: warp_rows={rows}, warp_fast={fast}")
    finally:
        ctx.close()
    assert np.array_equal(c["H"], H0) and np.array_equal(c["img"], img0)


def test_float64_grid(native):
    """``APAP.local_warp`` with a float64 grid: the spec over the oracle's coordinates on the float64 inverse the engine wrote
    back (as tests/test_gpu_warp_integer.py does for the truncating warp)."""
    from cvx_proj_amd.apap import APAP
    c = C.seeded(seed=21, final_w=83, final_h=59, rows=3, cols=4, dtype=np.float64)
    fw, fh, ox, oy = c["final"]
    eng = APAP(0.5, 100.0, [fw, fh], [ox, oy])
    arg = c["H"].copy()
    got = eng.local_warp(c["img"], arg, c["mesh"], sampling="bilinear")
    assert arg.dtype == np.float64 and np.allclose(arg, np.linalg.inv(c["H"]), rtol=1e-12, atol=1e-15)
    tx, ty = O.warp_coords_fast(arg, c["mesh"], (fw, fh), (ox, oy))
    same(got, S.sample(c["img"], tx, ty), "float64 grid")
    same(eng.local_warp(c["img"], c["H"].copy(), c["mesh"]), S.truncate(c["img"], tx, ty), "float64 grid, default")


@pytest.mark.parametrize("name", C.BUILT)
def test_built_cases(native, name):
    """Exact ties of rint with the even neighbour on either side, the same 2^-20 beside the tie, coordinates in (w - 1, w) and
    (h - 1, h) with [w - 1/64, w) where X = 32 w, coordinates in (0, 1/64), a strip that crosses a cell row, a lane whose four
    pixels sit in three cells: the engine's inverse and coordinates are the designed ones bit for bit, the canvas and the
    stitch (the centre's last pixel on the canvas' last pixel) the spec's."""
    c = C.get(name)
    fw, fh, ox, oy = c["final"]
    out, hinv = native.local_warp(c["img"], c["H"], c["mesh"][0], c["mesh"][1], fw, fh, ox, oy, sampling="bilinear")
    assert hinv.tobytes() == c["hinv"].tobytes(), "the engine's inverse is not the designed one"
    tx, ty = engine_coords(native, c)
    assert tx.tobytes() == c["coords"][0].tobytes() and ty.tobytes() == c["coords"][1].tobytes()
    want = S.sample(c["img"], tx, ty)
    same(out, want, name)
    center = c["center"]
    assert oy + center.shape[0] == fh and ox + center.shape[1] == fw
    got, _ = native.local_stitch(c["img"], center, c["H"], c["mesh"][0], c["mesh"][1], fw, fh, ox, oy, sampling="bilinear")
    same(got, S.stitch(want, center, (ox, oy)), f"{name}: stitch")
    assert (got != want).any()


@pytest.mark.parametrize("name", ["integers_a", "integers_b"])
def test_integer_translations_are_the_truncating_canvas(native, name):
    c = W.get(name)
    trunc = warp(native, c)
    same(trunc, O.local_warp_fast(c["img"], c["hinv"], c["mesh"], c["final"][:2], c["final"][2:]), f"{name}: default against the oracle")
    same(warp(native, c, sampling="bilinear"), trunc, f"{name}: bilinear against truncating")
    assert trunc.any(axis=-1).mean() > 0.3


def test_bands_batch_and_guard_bytes(native):
    """``hip_warp_rows`` bands that start and end inside a strip, ``hip_warp_batch`` of 3 pairs (each its own call's canvas) and
    its fused stitch, all into guarded buffers; ``WarpPlan.gather`` with the keyword."""
    import torch
    from cvx_proj_amd import resident
    dev = torch.device("cuda", 0)
    up = lambda a: torch.from_numpy(np.array(a)).to(dev)      # noqa: E731  (a copy: the cases are read-only)
    names = ("ties", "ties_plus", "ties_minus")
    cases = [C.get(n) for n in names]
    c0 = cases[0]
    fw, fh, ox, oy = c0["final"]
    rows, cols = c0["H"].shape[:2]
    want = [S.sample(c["img"], *c["coords"]) for c in cases]
    img, mw, mh = up(c0["img"]), up(c0["mesh"][0]), up(c0["mesh"][1])
    H = up(np.stack([c["H"].reshape(-1, 9) for c in cases]))
    H0 = H.clone()
    guard = 4096

    def guarded(n):
        buf = torch.full((guard + n + guard,), 0x5C, dtype=torch.uint8, device=dev)
        return buf, buf[guard:guard + n]

    def intact(buf, n):
        torch.cuda.synchronize(dev)
        return bool((buf[:guard] == 0x5C).all()) and bool((buf[guard + n:] == 0x5C).all())

    # bands of the first pair: inside a strip of 2 rows at both ends, a single row, the last rows
    for begin, count in ((1, 4), (3, 1), (5, 30), (fh - 3, 3)):
        n = count * fw * 3
        buf, flat = guarded(n)
        st = resident.hip_warp_rows(img, H[0], mw, mh, fw, fh, ox, oy, begin, count, flat.view(1, count, fw, 3), (rows, cols),
                                    sampling="bilinear")
        assert intact(buf, n) and int(st.cpu()[0]) == 0
        same(flat.view(count, fw, 3).cpu().numpy(), want[0][begin:begin + count], f"band [{begin}, {begin + count})")
    # the batch
    n = 3 * fh * fw * 3
    buf, flat = guarded(n)
    out, st = resident.hip_warp_batch(img, H, mw, mh, fw, fh, ox, oy, (rows, cols), out=flat.view(3, fh, fw, 3), sampling="bilinear")
    assert intact(buf, n) and int(st.cpu()[0]) == 0 and torch.equal(H, H0)
    for k, name in enumerate(names):
        same(out[k].cpu().numpy(), want[k], f"batch, pair {k} ({name})")
        same(out[k].cpu().numpy(), warp(native, cases[k], sampling="bilinear"), f"batch, pair {k} against its own call")
    # the batch's stitch, one centre for all
    buf, flat = guarded(n)
    out, _ = resident.hip_warp_batch(img, H, mw, mh, fw, fh, ox, oy, (rows, cols), out=flat.view(3, fh, fw, 3), centers=up(c0["center"]),
                                     sampling="bilinear")
    assert intact(buf, n)
    for k, name in enumerate(names):
        same(out[k].cpu().numpy(), S.stitch(want[k], c0["center"], (ox, oy)), f"batched stitch, pair {k}")
    # default unchanged in the same launch shape
    out, _ = resident.hip_warp_batch(img, H, mw, mh, fw, fh, ox, oy, (rows, cols))
    for k, c in enumerate(cases):
        same(out[k].cpu().numpy(), S.truncate(c["img"], *c["coords"]), f"batch, default, pair {k}")
    # a plan: the set-up phases once, the gather with either sampler
    plan = resident.WarpPlan((c0["mesh"][0].copy(), c0["mesh"][1].copy()), (rows, cols), fw, fh, ox, oy, dev, batch=3)
    plan.begin()
    plan.cells(H)
    same(plan.gather(img, sampling="bilinear")[1].cpu().numpy(), want[1], "plan, bilinear")
    same(plan.gather(img)[1].cpu().numpy(), S.truncate(cases[1]["img"], *cases[1]["coords"]), "plan, default")
    same(plan.gather(img, rows=(13, 2), sampling="bilinear")[2].cpu().numpy(), want[2][13:15], "plan, a band")
    assert plan.status_word() == 0


PANORAMAS = ("cross", "strip259", "two_pixels", "black_outside", "white17")


@pytest.mark.parametrize("name", PANORAMAS)
def test_panorama(native, name):
    """``_native.panorama(..., sampling="bilinear")`` for mean, paste and ramp (ramp = 8): the composition of
    tests/panorama_spec.py / the ramp's over the bilinear single-pair warps of its layers - the engine's, which are the spec's
    over the engine's coordinates -; ``hip_panorama`` gives the host-buffer form's bytes; the default stays the truncating
    composition."""
    import torch
    from cvx_proj_amd import apap, resident
    case = E.get(name)
    center, layers, geos = case["center"], case["layers"], case["geometries"]
    coords, warps = [], []
    for l in layers:
        c = dict(img=l.img, H=l.local_homography, mesh=l.mesh, final=tuple(l.final_size) + tuple(l.offset))
        coords.append(engine_coords(native, c))
        warps.append(warp(native, c, sampling="bilinear", want_inverse=False))
        same(warps[-1], S.sample(l.img, *coords[-1]), f"{name}: a layer's bilinear warp")
    want = {mode: P.compose(center, warps, geos, mode) for mode in ("mean", "paste")}
    want["ramp"] = S.compose_ramp(center, layers, geos, coords, 8)
    dev = torch.device("cuda", 0)
    up = lambda a: torch.from_numpy(np.array(a)).to(dev)      # noqa: E731  (a copy: the cases are read-only)
    d_layers = [apap.PanoramaLayer(up(l.img), up(l.local_homography), (up(l.mesh[0]), up(l.mesh[1])), l.final_size, l.offset)
                for l in layers]
    differs = False
    for mode in ("mean", "paste", "ramp"):
        got, bounds = native.panorama(center, layers, blend=mode, ramp=8, sampling="bilinear")
        assert bounds == P.panorama_size(center.shape, geos)
        same(got, want[mode], f"{name}, {mode}")
        dgot, dbounds, status = resident.hip_panorama(up(center), d_layers, blend=mode, ramp=8, sampling="bilinear")
        assert dbounds == bounds and not status.cpu().numpy().any()
        same(dgot.cpu().numpy(), got, f"{name}, {mode}: device form")
        default, _ = native.panorama(center, layers, blend=mode, ramp=8)
        nearest, _ = apap.panorama(center, layers, blend=mode, ramp=8, sampling="nearest")
        assert default.tobytes() == nearest.tobytes()
        if mode != "ramp":
            same(default, P.compose(center, case["oracle"], geos, mode), f"{name}, {mode}: default")
        differs = differs or (default != got).any()
    assert differs or name == "white17", "the two samplers give different canvases"


def test_pipeline_and_command_line(native, tmp_path):
    """One synthetic pair: ``Pipeline.run_pair`` (the solve-then-warp plan) and ``run_pair_by_calls`` with the keyword give the
    same canvas, which differs from the default's; ``python -m cvx_proj_amd.apap --pair ... --warp ... --sampling bilinear``
    writes it."""
    from cvx_proj_amd import apap
    from cvx_proj_amd.synth import synth_pair
    p = synth_pair(320, 240, 96, 12, seed=7)
    args = (p.src, p.dst, p.Hg, p.shape, p.shape, 12, 0.5, 100.0)
    flat, want = apap.run_pair_by_calls(*args, other_img=p.img, sampling="bilinear")
    flat0, default = apap.run_pair_by_calls(*args, other_img=p.img)
    assert np.array_equal(flat, flat0) and want.shape == default.shape and (want != default).any()
    _, got = apap.run_pair(*args, other_img=p.img, sampling="bilinear")
    same(got, want, "Pipeline.run_pair against the calls")
    _, got = apap.run_pair(*args, other_img=p.img)
    same(got, default, "Pipeline.run_pair, default")
    pair, out = tmp_path / "pair.npz", tmp_path / "warp.npy"
    np.savez(pair, src=p.src, dst=p.dst, H=p.Hg, other_shape=np.array(p.shape), center_shape=np.array(p.shape), other_img=p.img)
    r = subprocess.run([sys.executable, "-m", "cvx_proj_amd.apap", "--pair", str(pair), "--mesh-size", "12", "--warp", str(out),
                        "--sampling", "bilinear", "--out-prefix", str(tmp_path) + "/"], cwd=ROOT, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    same(np.load(out), want, "command line")
