"""The panorama's two-band blend on the GPU (apap_panorama_band*, apap.panorama and resident.hip_panorama with
``blend="band"``): byte for byte the composition of tests/panorama_band_spec.py over the engine's own coordinates
(``_native.warp_coords``) of every layer and over the oracle's, on the cases of tests/panorama_cases.py, on the inputs that
fill the accumulators (tests/panorama_ramp_cases.py) and on those of tests/panorama_band_cases.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

import panorama_band_cases as BC
import panorama_band_spec as P
import panorama_cases as E
import panorama_ramp_cases as RC
import panorama_spec as S

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RAMP_BAND = ((8, 0), (8, 1), (3, 8), (256, 32))


@pytest.fixture(scope="module")
def native_gpu(native):
    if native.lib().apap_device_count() < 1:
        pytest.skip("no HIP device")
    return native


def same(got, want, what):
    assert got.dtype == np.uint8 and got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere((got != want).any(axis=-1))
    assert len(bad) == 0, f"{what}: {len(bad)} pixels differ, first at (y, x) = {tuple(bad[0])}: {got[tuple(bad[0])]} != {want[tuple(bad[0])]}"


@pytest.mark.parametrize("name", RC.ALL_CASES)
def test_cases(native_gpu, name):
    """All ten cases at (ramp, band) = (8, 0), (8, 1), (3, 8), (256, 32): the specification over the engine's coordinates and
    over the oracle's, the bounds, unmodified grids, and at band 0 the engine's own ramp blend."""
    from cvx_proj_amd import apap
    case = E.get(name)
    center, layers, geos = case["center"], case["layers"], case["geometries"]
    grids = [np.array(l.local_homography) for l in layers]
    own = RC.engine_coords(native_gpu, layers)
    for ramp, band in RAMP_BAND:
        got, bounds = apap.panorama(center, layers, blend="band", ramp=ramp, band=band)
        assert bounds == S.panorama_size(center.shape, geos)
        what = f"{name}, ramp {ramp}, band {band}"
        same(got, P.compose_band(center, layers, geos, own, ramp, band).canvas, what + ", against the engine's coordinates")
        same(got, P.compose_band(center, layers, geos, RC.oracle_coords(name), ramp, band).canvas, what + ", against the oracle's")
        if band == 0:
            same(got, apap.panorama(center, layers, blend="ramp", ramp=ramp)[0], what + ", against the engine's ramp")
    assert all(np.array_equal(g, l.local_homography) for g, l in zip(grids, layers)), "the grids are not modified"


def test_band_8_differs_from_band_0(native_gpu):
    from cvx_proj_amd import apap
    case = E.get("cross")
    a = apap.panorama(case["center"], case["layers"], blend="band", ramp=8, band=8)[0]
    b = apap.panorama(case["center"], case["layers"], blend="band", ramp=8, band=0)[0]
    assert (a != b).any(), "the radius reaches the kernel"
    same(apap.panorama(case["center"], case["layers"], blend="band", ramp=8)[0], a, "band = 8 is the default")


@pytest.mark.parametrize("name", ["clamp", "layer_ties"])
def test_band_cases(native_gpu, name):
    """The clip at both ends, and ties of D among layers where the centre is absent."""
    from cvx_proj_amd import apap
    case = getattr(BC, name)()
    center, layers, geos = case["center"], case["layers"], case["geometries"]
    own = RC.engine_coords(native_gpu, layers)
    for ramp, band in ((8, 1), (8, 8), (3, 32)):
        got, _ = apap.panorama(center, layers, blend="band", ramp=ramp, band=band)
        want = P.compose_band(center, layers, geos, own, ramp, band)
        if name == "clamp" and band < 32:
            assert (want.raw > 255).any() and (want.raw < 0).any()
        same(got, want.canvas, f"{name}, ramp {ramp}, band {band}, against the engine's coordinates")
        same(got, P.compose_band(center, layers, geos, case["coords"], ramp, band).canvas, f"{name}, ramp {ramp}, band {band}, against the oracle's")


@pytest.mark.parametrize("white", [False, True], ids=["random", "white"])
def test_saturation(native_gpu, white):
    """17 samples of weight 256 and of one D on a pixel: the weight sums hold 4352, the low sums (all pictures 255) 1 109 760,
    and the centre wins the tie.  Over the engine's own coordinates (see test_gpu_panorama_ramp.py)."""
    from cvx_proj_amd import apap
    case = RC.saturation(white)
    got, bounds = apap.panorama(case["center"], case["layers"], blend="band", ramp=256, band=32)
    assert bounds == (512, 512, 0, 0)
    own = RC.engine_coords(native_gpu, case["layers"][:1]) * 16
    want = P.compose_band(case["center"], case["layers"], case["geometries"], own, 256, 32)
    assert want.wsum.max() == 4352 and want.count.max() == 17 and want.tied.max() == 17
    same(got, want.canvas, "saturation against the engine's coordinates")
    if white:
        assert want.total.max() == 1109760 and (got == 255).all()


def test_one_layer_at_c1(native_gpu):
    """768 x 768 pictures on a 20 x 20 mesh at ramp 64, band 8: 4 x 3 strips of blocks, every cell row and column."""
    from cvx_proj_amd import apap
    case = E.single_c1()
    (l,), center = case["layers"], case["center"]
    got, bounds = apap.panorama(center, [l], blend="band", ramp=64, band=8)
    assert bounds == tuple(l.final_size) + tuple(l.offset)
    want = P.compose_band(center, [l], case["geometries"], RC.engine_coords(native_gpu, [l]), 64, 8)
    assert want.wsum.max() == 128 and want.count.max() == 2
    same(got, want.canvas, "C1, ramp 64, band 8, against the engine's coordinates")


@pytest.mark.parametrize("name", ["cross", "wide"])
def test_bilinear(native_gpu, name):
    from cvx_proj_amd import apap
    case = E.get(name)
    center, layers, geos = case["center"], case["layers"], case["geometries"]
    own = RC.engine_coords(native_gpu, layers)
    for ramp, band in ((8, 0), (8, 2), (256, 32)):
        got, _ = apap.panorama(center, layers, blend="band", ramp=ramp, band=band, sampling="bilinear")
        same(got, P.compose_band(center, layers, geos, own, ramp, band, sampling="bilinear").canvas, f"{name}, bilinear, ramp {ramp}, band {band}")
        if band == 0:
            same(got, apap.panorama(center, layers, blend="ramp", ramp=ramp, sampling="bilinear")[0], f"{name}, bilinear, against the engine's ramp")
    nearest = apap.panorama(center, layers, blend="band", ramp=8, band=2)[0]
    assert (nearest != apap.panorama(center, layers, blend="band", ramp=8, band=2, sampling="bilinear")[0]).any()


@pytest.mark.parametrize("name", ["cross", "strip259"])
def test_gains(native_gpu, name):
    """A q per view; q = 4096 everywhere is the ungained canvas; under both samplings; and gain="auto"."""
    from cvx_proj_amd import apap
    case = E.get(name)
    center, layers, geos = case["center"], case["layers"], case["geometries"]
    own = RC.engine_coords(native_gpu, layers)
    q = BC.gains(len(layers) + 1)
    assert len(set(q)) == len(q)
    for sampling in ("nearest", "bilinear"):
        got, _ = apap.panorama(center, layers, blend="band", ramp=8, band=4, gain=q, sampling=sampling)
        same(got, P.compose_band(center, layers, geos, own, 8, 4, sampling=sampling, q=q).canvas, f"{name}, {sampling}, gains {q}")
        plain = apap.panorama(center, layers, blend="band", ramp=8, band=4, sampling=sampling)[0]
        same(apap.panorama(center, layers, blend="band", ramp=8, band=4, gain=[4096] * len(q), sampling=sampling)[0], plain,
             f"{name}, {sampling}, q = 4096 everywhere")
        assert (got != plain).any()
    auto = apap.panorama_gains(center, layers, step=1)
    same(apap.panorama(center, layers, blend="band", ramp=8, band=4, gain="auto", gain_step=1)[0],
         P.compose_band(center, layers, geos, own, 8, 4, q=[int(v) for v in auto.q]).canvas, f"{name}, gain='auto'")


@pytest.mark.parametrize("name", ["cross", "wide"])
def test_device_form_and_its_buffers(native_gpu, name):
    """resident.hip_panorama(blend="band", ramp=8, band=4) on device tensors: the host-buffer form's bytes, and again into a
    guarded ``out`` with a workspace of 0xA5; nothing written outside ``out`` or past the workspace; the grids unchanged."""
    import torch
    from cvx_proj_amd import apap, resident
    case = E.get(name)
    dev = torch.device("cuda", 0)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)      # noqa: E731
    center = up(case["center"])
    layers = [apap.PanoramaLayer(up(l.img), up(l.local_homography), (up(l.mesh[0]), up(l.mesh[1])), l.final_size, l.offset)
              for l in case["layers"]]
    n = len(layers)
    grids = [l.local_homography.clone() for l in layers]
    W, H, OX, OY = S.panorama_size(case["center"].shape, case["geometries"])
    need = resident.panorama_band_workspace_bytes(center, layers, 4)
    assert need > resident.panorama_workspace_bytes(layers) == resident.panorama_band_workspace_bytes(center, layers, 0) and need % 256 == 0
    want, _ = apap.panorama(case["center"], case["layers"], blend="band", ramp=8, band=4)
    same(want, P.compose_band(case["center"], case["layers"], case["geometries"], RC.oracle_coords(name), 8, 4).canvas, f"{name}, host-buffer form")
    got, bounds, status = resident.hip_panorama(center, layers, blend="band", ramp=8, band=4)
    assert bounds == (W, H, OX, OY) and status.tolist() == [0] * n
    same(got.cpu().numpy(), want, f"{name}, device form")
    guard = 4096
    buf = torch.full((guard + H * W * 3 + guard,), 0x5C, dtype=torch.uint8, device=dev)
    out = buf[guard:guard + H * W * 3].view(H, W, 3)
    work = torch.full((need + 512,), 0xA5, dtype=torch.uint8, device=dev)
    status = torch.zeros(n + 2, dtype=torch.int32, device=dev)
    got2, _, status2 = resident.hip_panorama(center, layers, blend="band", ramp=8, band=4, out=out, status=status, work=work)
    torch.cuda.synchronize(dev)
    assert got2.data_ptr() == out.data_ptr() and status2.data_ptr() == status.data_ptr()
    same(got2.cpu().numpy(), want, f"{name}, device form into out, 0xA5 workspace")
    assert bool((buf[:guard] == 0x5C).all()) and bool((buf[guard + H * W * 3:] == 0x5C).all()), "guard bytes around out"
    assert bool((work[need:] == 0xA5).all()), "bytes past the workspace the call asked for"
    assert status.tolist() == [0] * (n + 2)
    assert all(torch.equal(g, l.local_homography) for g, l in zip(grids, layers)), "the grids are not modified"
    q = BC.gains(n + 1)
    same(resident.hip_panorama(center, layers, blend="band", ramp=8, band=4, gain=q)[0].cpu().numpy(),
         apap.panorama(case["center"], case["layers"], blend="band", ramp=8, band=4, gain=q)[0], f"{name}, device form under gains")
    same(resident.hip_panorama(center, layers, blend="band", ramp=8, band=4, gain="auto")[0].cpu().numpy(),
         apap.panorama(case["center"], case["layers"], blend="band", ramp=8, band=4, gain="auto")[0], f"{name}, device form, gain='auto'")
    for bad in (-1, 33, 2.5, "8"):
        with pytest.raises(ValueError, match="band"):
            resident.hip_panorama(center, layers, blend="band", band=bad)
    with pytest.raises(ValueError, match="ramp"):
        resident.hip_panorama(center, layers, blend="band", ramp=0)


def test_command_line(native_gpu, tmp_path):
    """``--synth C1 --cases 1 --imgs 1,2,4,5 --panorama out.npy --panorama-blend band --panorama-ramp 16 --panorama-band 4``:
    apap.panorama of the same four pairs; no torch."""
    from cvx_proj_amd import apap
    from cvx_proj_amd.synth import CONFIGS, synth_pair
    out = tmp_path / "pano.npy"
    code = ("import sys; from cvx_proj_amd import apap; rc = apap.main(sys.argv[1:]); "
            "assert 'torch' not in sys.modules, 'torch was imported'; sys.exit(rc)")
    r = subprocess.run([sys.executable, "-c", code, "--synth", "C1", "--cases", "1", "--imgs", "1,2,4,5", "--panorama", str(out),
                        "--panorama-blend", "band", "--panorama-ramp", "16", "--panorama-band", "4", "--out-prefix", str(tmp_path) + "/"],
                       cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    got = np.load(out)
    w, h, n, m, seed = CONFIGS["C1"]
    layers, center = [], None
    for img_idx in (1, 2, 4, 5):
        s = seed + (img_idx - 1)
        p = synth_pair(w, h, n, m, s)
        if center is None:
            center = np.random.default_rng(s + 1).integers(0, 256, p.shape, dtype=np.uint8)
        layers.append(apap.panorama_layer(p.src, p.dst, p.Hg, p.img, p.shape, m, 0.5, 100.0))
    want, bounds = apap.panorama(center, layers, blend="band", ramp=16, band=4)
    assert got.shape == (bounds[1], bounds[0], 3)
    same(got, want, "command line against apap.panorama")
    assert (want != apap.panorama(center, layers, blend="band", ramp=16, band=0)[0]).any(), "the radius reaches the kernel"
