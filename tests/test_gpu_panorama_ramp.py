"""The panorama's edge-ramp blend on the GPU (apap_panorama_ramp*, apap.panorama and resident.hip_panorama with
``blend="ramp"``): byte for byte the composition of tests/panorama_ramp_spec.py over the engine's own coordinates
(``_native.warp_coords``) of every layer and over the oracle's, on the cases of tests/panorama_cases.py and on the input that
fills the accumulators (tests/panorama_ramp_cases.py)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import panorama_cases as E
import panorama_ramp_cases as RC
import panorama_ramp_spec as R
import panorama_spec as S

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RAMPS = (1, 3, 8, 256)


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
    """All ten cases at ramps 1, 3, 8 and 256: the specification over the engine's coordinates and over the oracle's, the
    bounds, unmodified grids, and at ramp 1 the engine's own mean."""
    from cvx_proj_amd import apap
    case = E.get(name)
    center, layers, geos = case["center"], case["layers"], case["geometries"]
    grids = [np.array(l.local_homography) for l in layers]
    own = RC.engine_coords(native_gpu, layers)
    for ramp in RAMPS:
        got, bounds = apap.panorama(center, layers, blend="ramp", ramp=ramp)
        assert bounds == S.panorama_size(center.shape, geos)
        same(got, R.compose_ramp(center, layers, geos, own, ramp)[0], f"{name}, ramp {ramp}, against the engine's coordinates")
        same(got, R.compose_ramp(center, layers, geos, RC.oracle_coords(name), ramp)[0], f"{name}, ramp {ramp}, against the oracle's")
        if ramp == 1:
            same(got, apap.panorama(center, layers, blend="mean")[0], f"{name}, ramp 1 against the engine's mean")
    assert all(np.array_equal(g, l.local_homography) for g, l in zip(grids, layers)), "the grids are not modified"


@pytest.mark.parametrize("white", [False, True], ids=["random", "white"])
def test_saturation(native_gpu, white):
    """17 samples of weight 256 on one pixel: the packed weight sums hold 4352 and, all pictures 255, the sums 1 109 760
    (tests/test_panorama_ramp_host.py shows that the input reaches both).  Over the engine's own coordinates: on 262 144
    pixels of one cell the oracle's float32 inverse, which may differ from the engine's in the last place, can truncate a
    coordinate to the neighbouring source pixel; the small cases of test_cases are held to both."""
    from cvx_proj_amd import apap
    case = RC.saturation(white)
    got, bounds = apap.panorama(case["center"], case["layers"], blend="ramp", ramp=256)
    assert bounds == (512, 512, 0, 0)
    own = RC.engine_coords(native_gpu, case["layers"][:1]) * 16      # 16 times the same layer
    want, wsum, count = R.compose_ramp(case["center"], case["layers"], case["geometries"], own, 256)
    assert wsum.max() == 4352 and count.max() == 17
    same(got, want, "saturation against the engine's coordinates")
    if white:       # whichever source pixel a sample truncates to: the oracle's coordinates give the same canvas
        same(got, R.compose_ramp(case["center"], case["layers"], case["geometries"], case["coords"], 256)[0], "saturation against the oracle's")
        assert (got == 255).all()


def test_one_layer_at_c1(native_gpu):
    """768 x 768 pictures on a 20 x 20 mesh at ramp 64: 4 x 3 strips of blocks, every cell row and column."""
    from cvx_proj_amd import apap
    case = E.single_c1()
    (l,), center = case["layers"], case["center"]
    assert l.img.shape == center.shape == (768, 768, 3) and l.local_homography.shape[:2] == (20, 20)
    got, bounds = apap.panorama(center, [l], blend="ramp", ramp=64)
    assert bounds == tuple(l.final_size) + tuple(l.offset)
    want, wsum, count = R.compose_ramp(center, [l], case["geometries"], RC.engine_coords(native_gpu, [l]), 64)
    assert wsum.max() == 128 and count.max() == 2
    same(got, want, "C1, ramp 64, against the engine's coordinates")


@pytest.mark.parametrize("name", ["cross", "wide"])
def test_device_form_and_its_buffers(native_gpu, name):
    """resident.hip_panorama(blend="ramp", ramp=8) on device tensors: the host-buffer form's bytes, and again into a guarded
    ``out`` with a workspace of 0xA5; nothing written outside ``out`` or past the workspace; the grids unchanged."""
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
    need = resident.panorama_workspace_bytes(layers)
    assert need > 0 and need % 256 == 0
    want, _ = apap.panorama(case["center"], case["layers"], blend="ramp", ramp=8)
    same(want, R.compose_ramp(case["center"], case["layers"], case["geometries"], RC.oracle_coords(name), 8)[0], f"{name}, host-buffer form")
    got, bounds, status = resident.hip_panorama(center, layers, blend="ramp", ramp=8)
    assert bounds == (W, H, OX, OY) and status.tolist() == [0] * n
    same(got.cpu().numpy(), want, f"{name}, device form")
    guard = 4096
    buf = torch.full((guard + H * W * 3 + guard,), 0x5C, dtype=torch.uint8, device=dev)
    out = buf[guard:guard + H * W * 3].view(H, W, 3)
    work = torch.full((need + 512,), 0xA5, dtype=torch.uint8, device=dev)
    status = torch.zeros(n + 2, dtype=torch.int32, device=dev)
    got2, _, status2 = resident.hip_panorama(center, layers, blend="ramp", ramp=8, out=out, status=status, work=work)
    torch.cuda.synchronize(dev)
    assert got2.data_ptr() == out.data_ptr() and status2.data_ptr() == status.data_ptr()
    same(got2.cpu().numpy(), want, f"{name}, device form into out, 0xA5 workspace")
    assert bool((buf[:guard] == 0x5C).all()) and bool((buf[guard + H * W * 3:] == 0x5C).all()), "guard bytes around out"
    assert bool((work[need:] == 0xA5).all()), "bytes past the workspace the call asked for"
    assert status.tolist() == [0] * (n + 2)
    assert all(torch.equal(g, l.local_homography) for g, l in zip(grids, layers)), "the grids are not modified"
    for bad in (0, 257, 2.5, "8"):
        with pytest.raises(ValueError, match="ramp"):
            resident.hip_panorama(center, layers, blend="ramp", ramp=bad)


def test_command_line(native_gpu, tmp_path):
    """``--synth C1 --cases 1 --imgs 1,2,4,5 --panorama out.npy --panorama-blend ramp --panorama-ramp 16``: apap.panorama of
    the same four pairs; no torch."""
    from cvx_proj_amd import apap
    from cvx_proj_amd.synth import CONFIGS, synth_pair
    out = tmp_path / "pano.npy"
    code = ("import sys; from cvx_proj_amd import apap; rc = apap.main(sys.argv[1:]); "
            "assert 'torch' not in sys.modules, 'torch was imported'; sys.exit(rc)")
    r = subprocess.run([sys.executable, "-c", code, "--synth", "C1", "--cases", "1", "--imgs", "1,2,4,5", "--panorama", str(out),
                        "--panorama-blend", "ramp", "--panorama-ramp", "16", "--out-prefix", str(tmp_path) + "/"],
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
    want, bounds = apap.panorama(center, layers, blend="ramp", ramp=16)
    assert got.shape == (bounds[1], bounds[0], 3)
    same(got, want, "command line against apap.panorama")
    assert (want != apap.panorama(center, layers, blend="ramp", ramp=1)[0]).any(), "the ramp width reaches the kernel"
