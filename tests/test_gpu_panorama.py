"""The panorama on the GPU (apap_panorama*, apap.panorama, resident.hip_panorama): byte for byte the composition of
tests/panorama_spec.py over the engine's own single-pair ``local_warp`` of every layer - and, on the small cases, over the
oracle's - at the kernel's edges (tests/panorama_cases.py)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import panorama_cases as E
import panorama_spec as S

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = ("mean", "paste")


@pytest.fixture(scope="module")
def native_gpu(native):
    if native.lib().apap_device_count() < 1:
        pytest.skip("no HIP device")
    return native


def warps(native, case):
    """Every layer's canvas by the engine's single-pair local_warp (cached on the case)."""
    if "warps" not in case:
        case["warps"] = [native.local_warp(l.img, l.local_homography, l.mesh[0], l.mesh[1], l.final_size[0], l.final_size[1],
                                           l.offset[0], l.offset[1], want_inverse=False)[0] for l in case["layers"]]
    return case["warps"]


def same(got, want, what):
    assert got.dtype == np.uint8 and got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere((got != want).any(axis=-1))
    assert len(bad) == 0, f"{what}: {len(bad)} pixels differ, first at (y, x) = {tuple(bad[0])}: {got[tuple(bad[0])]} != {want[tuple(bad[0])]}"


def check_case(native, case, what, oracle=True):
    from cvx_proj_amd import apap
    center, layers, geos = case["center"], case["layers"], case["geometries"]
    grids = [np.array(l.local_homography) for l in layers]
    for mode in MODES:
        got, bounds = apap.panorama(center, layers, blend=mode)
        assert bounds == S.panorama_size(center.shape, geos)
        same(got, S.compose(center, warps(native, case), geos, mode), f"{what} {mode} against local_warp")
        if oracle:
            same(got, S.compose(center, case["oracle"], geos, mode), f"{what} {mode} against the oracle")
    assert all(np.array_equal(g, l.local_homography) for g, l in zip(grids, layers)), "the grids are not modified"


@pytest.mark.parametrize("name", sorted(E.HOST_CASES))
def test_small_cases(native_gpu, name):
    """The cross (four directions, every alignment of a pair canvas against the lanes' groups of 4, an irregular mesh), the
    canvases 259 and 517 wide and 16 n + 1 high, 16 layers, two layers on one source buffer: both modes."""
    check_case(native_gpu, E.get(name), name)


@pytest.mark.parametrize("name", sorted(E.TILING_CASES))
def test_tiling_cases(native_gpu, name):
    """Pair canvases that begin and end at the 256-column strip boundaries of a 530-wide canvas, a canvas of exactly one
    block, a black block of the first layer over a present second one outside the centre picture, 17 white pictures on one
    pixel, pictures of two pixels: both modes (tests/test_panorama_host.py shows that each case reaches its edge)."""
    check_case(native_gpu, E.get(name), name)


def test_one_layer_at_c1_is_local_stitch(native_gpu):
    from cvx_proj_amd import apap
    case = E.single_c1()
    (l,), center = case["layers"], case["center"]
    assert l.img.shape == center.shape == (768, 768, 3) and l.local_homography.shape[:2] == (20, 20)
    got, bounds = apap.panorama(center, [l], blend="mean")
    want, _ = native_gpu.local_stitch(l.img, center, l.local_homography, l.mesh[0], l.mesh[1], l.final_size[0], l.final_size[1],
                                      l.offset[0], l.offset[1])
    assert bounds == tuple(l.final_size) + tuple(l.offset)
    same(got, want, "K = 1 mean against local_stitch")
    check_case(native_gpu, case, "C1", oracle=False)


def test_sixteen_layers_and_not_seventeen(native_gpu):
    from cvx_proj_amd import apap
    case = E.sixteen()
    assert len(case["layers"]) == 16 and all(l.img.shape == (8, 8, 3) for l in case["layers"])
    with pytest.raises(ValueError):
        apap.panorama(case["center"], case["layers"] + case["layers"][:1])


def test_linear_scan_set_up(native_gpu):
    """More than 4096 mesh edges: the set-up takes its linear-scan kernels and leaves the same tables."""
    case = E.linear_scan()
    assert case["layers"][0].mesh[0].size == 4101 and case["geometries"] == [(4200, 6, 0, 0)]
    check_case(native_gpu, case, "1 x 4100 mesh", oracle=False)


def test_paste_shows_the_centre_and_keeps_its_black_pixels(native_gpu):
    from cvx_proj_amd import apap
    case = E.get("cross")
    center = case["center"].copy()
    center[5:9, 7:30] = 0                   # black pixels of the centre, under present layers
    center[20, 3] = 0
    geos = case["geometries"]
    W, H, OX, OY = S.panorama_size(center.shape, geos)
    got, _ = apap.panorama(center, case["layers"], blend="paste")
    rect = got[OY:OY + center.shape[0], OX:OX + center.shape[1]]
    assert np.array_equal(rect, center) and not rect[5:9, 7:30].any()
    stack = S.placed(center, warps(native_gpu, case), geos)
    hidden = stack[1:, OY + 5:OY + 9, OX + 7:OX + 30].any(axis=-1).any(axis=0)
    assert hidden.all(), "a layer is present under every one of those black pixels and does not show"
    same(got, S.compose(center, warps(native_gpu, case), geos, "paste"), "paste, black centre pixels")
    mean, _ = apap.panorama(center, case["layers"], blend="mean")
    same(mean, S.compose(center, warps(native_gpu, case), geos, "mean"), "mean, black centre pixels")
    assert mean[OY + 5:OY + 9, OX + 7:OX + 30].any(axis=-1).all()      # there the mean is the layers' alone


def test_shared_source_is_one_buffer(native_gpu):
    case = E.get("shared")
    a, b = case["layers"]
    assert a.img is b.img and a.img.ctypes.data == b.img.ctypes.data
    check_case(native_gpu, case, "shared source")


def test_status_names_the_layer(native_gpu):
    from cvx_proj_amd import apap
    case = E.get("cross")
    layers = list(case["layers"])
    H = layers[2].local_homography.copy()
    H[4, 5] = 0.0
    layers[2] = layers[2]._replace(local_homography=H)
    with pytest.raises(np.linalg.LinAlgError, match="layer 2") as e:
        apap.panorama(case["center"], layers)
    assert isinstance(e.value, native_gpu.ApapSingularError) and "Singular matrix" in str(e.value)
    _, _, status = native_gpu.panorama(case["center"], layers, return_status=True)
    assert status.tolist() == [0, 0, native_gpu.STATUS_SINGULAR, 0]
    # row edges that stop 5 short of the pair canvas: local_warp's IndexError
    layers = list(case["layers"])
    mesh_w, mesh_h = layers[1].mesh
    short = mesh_h.copy()
    short[-1] -= 5.0
    layers[1] = layers[1]._replace(mesh=(mesh_w, short))
    with pytest.raises(IndexError, match="layer 1") as e:
        apap.panorama(case["center"], layers, blend="paste")
    assert isinstance(e.value, native_gpu.ApapIndexError)
    _, _, status = native_gpu.panorama(case["center"], layers, return_status=True)
    assert status.tolist() == [0, native_gpu.STATUS_INDEX, 0, 0]


def test_device_form_and_its_buffers(native_gpu):
    """resident.hip_panorama on device tensors: the host-buffer form's bytes; the grids unchanged; nothing written outside
    ``out``; a workspace full of 0xA5 makes no difference; a status word per layer."""
    import torch
    from cvx_proj_amd import apap, resident
    case = E.get("cross")
    dev = torch.device("cuda", 0)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)      # noqa: E731
    center = up(case["center"])
    layers = [apap.PanoramaLayer(up(l.img), up(l.local_homography), (up(l.mesh[0]), up(l.mesh[1])), l.final_size, l.offset)
              for l in case["layers"]]
    grids = [l.local_homography.clone() for l in layers]
    W, H, OX, OY = S.panorama_size(case["center"].shape, case["geometries"])
    need = resident.panorama_workspace_bytes(layers)
    assert need > 0 and need % 256 == 0
    guard = 4096
    for mode in MODES:
        want, _ = apap.panorama(case["center"], case["layers"], blend=mode)
        got, bounds, status = resident.hip_panorama(center, layers, blend=mode)
        assert bounds == (W, H, OX, OY) and status.tolist() == [0, 0, 0, 0]
        same(got.cpu().numpy(), want, f"device form, {mode}")
        buf = torch.full((guard + H * W * 3 + guard,), 0x5C, dtype=torch.uint8, device=dev)
        out = buf[guard:guard + H * W * 3].view(H, W, 3)
        work = torch.full((need + 512,), 0xA5, dtype=torch.uint8, device=dev)
        status = torch.zeros(6, dtype=torch.int32, device=dev)
        got2, _, status2 = resident.hip_panorama(center, layers, blend=mode, out=out, status=status, work=work)
        torch.cuda.synchronize(dev)
        assert got2.data_ptr() == out.data_ptr() and status2.data_ptr() == status.data_ptr()
        same(got2.cpu().numpy(), want, f"device form into out, 0xA5 workspace, {mode}")
        assert bool((buf[:guard] == 0x5C).all()) and bool((buf[guard + H * W * 3:] == 0x5C).all()), "guard bytes around out"
        assert bool((work[need:] == 0xA5).all()), "bytes past the workspace the call asked for"
        assert status.tolist() == [0] * 6
    assert all(torch.equal(g, l.local_homography) for g, l in zip(grids, layers)), "the grids are not modified"
    # a zeroed cell: its layer's word, nobody else's
    bad = layers[3].local_homography.clone()
    bad[0, 0] = 0
    _, _, status = resident.hip_panorama(center, layers[:3] + [layers[3]._replace(local_homography=bad)])
    assert status.tolist() == [0, 0, 0, native_gpu.STATUS_SINGULAR]


@pytest.mark.parametrize("name", ["wide", "black_outside"])
def test_device_form_on_tiling_cases(native_gpu, name):
    """resident.hip_panorama into a guarded ``out`` with a workspace of 0xA5: the specification's bytes over the oracle's
    layers, nothing written outside ``out``."""
    import torch
    from cvx_proj_amd import apap, resident
    case = E.get(name)
    dev = torch.device("cuda", 0)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)      # noqa: E731
    center = up(case["center"])
    layers = [apap.PanoramaLayer(up(l.img), up(l.local_homography), (up(l.mesh[0]), up(l.mesh[1])), l.final_size, l.offset)
              for l in case["layers"]]
    n = len(layers)
    W, H, OX, OY = S.panorama_size(case["center"].shape, case["geometries"])
    need = resident.panorama_workspace_bytes(layers)
    assert need > 0 and need % 256 == 0
    guard = 4096
    for mode in MODES:
        buf = torch.full((guard + H * W * 3 + guard,), 0x5C, dtype=torch.uint8, device=dev)
        out = buf[guard:guard + H * W * 3].view(H, W, 3)
        work = torch.full((need + 512,), 0xA5, dtype=torch.uint8, device=dev)
        status = torch.zeros(n + 2, dtype=torch.int32, device=dev)
        got, bounds, _ = resident.hip_panorama(center, layers, blend=mode, out=out, status=status, work=work)
        torch.cuda.synchronize(dev)
        assert got.data_ptr() == out.data_ptr() and bounds == (W, H, OX, OY)
        same(got.cpu().numpy(), S.compose(case["center"], case["oracle"], case["geometries"], mode), f"{name}, device form, {mode}")
        assert bool((buf[:guard] == 0x5C).all()) and bool((buf[guard + H * W * 3:] == 0x5C).all()), "guard bytes around out"
        assert bool((work[need:] == 0xA5).all()), "bytes past the workspace the call asked for"
        assert status.tolist() == [0] * (n + 2)


def test_command_line(native_gpu, tmp_path):
    """``--synth C1 --cases 1 --imgs 1,2,4,5 --panorama``: one canvas, apap.panorama of the same four pairs; no torch."""
    from cvx_proj_amd import apap
    from cvx_proj_amd.synth import CONFIGS, synth_pair
    out = tmp_path / "pano.npy"
    code = ("import sys; from cvx_proj_amd import apap; rc = apap.main(sys.argv[1:]); "
            "assert 'torch' not in sys.modules, 'torch was imported'; sys.exit(rc)")
    r = subprocess.run([sys.executable, "-c", code, "--synth", "C1", "--cases", "1", "--imgs", "1,2,4,5", "--panorama", str(out),
                        "--out-prefix", str(tmp_path) + "/"], cwd=ROOT, capture_output=True, text=True, timeout=300)
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
    want, bounds = apap.panorama(center, layers)
    assert got.shape == (bounds[1], bounds[0], 3)
    same(got, want, "command line against apap.panorama")
    geos = [tuple(l.final_size) + tuple(l.offset) for l in layers]
    canvases = [native_gpu.local_warp(l.img, l.local_homography, l.mesh[0], l.mesh[1], *l.final_size, *l.offset, want_inverse=False)[0]
                for l in layers]
    same(got, S.compose(center, canvases, geos, "mean"), "command line against the composition of local_warp")
    assert all((tmp_path / "case1" / f"H3{i}_apap.mat").exists() for i in (1, 2, 4, 5))
