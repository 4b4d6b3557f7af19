"""Exposure gain compensation of the panorama on the GPU (apap_panorama_gain*, apap_panorama_auto_gain*, apap.panorama /
apap.panorama_gains / resident.hip_panorama with ``gain``): the overlap statistics and the gained canvases are those of
tests/panorama_gain_spec.py, exactly, over the engine's own coordinates (``_native.warp_coords``) and over the oracle's, on the
cases of tests/panorama_cases.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

import panorama_cases as E
import panorama_gain_spec as G
import panorama_ramp_cases as RC
import panorama_spec as S

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAMPLINGS = ("nearest", "bilinear")
STEPS = (1, 2, 3, 64)
BLENDS = (("mean", 1), ("paste", 1), ("ramp", 1), ("ramp", 8), ("ramp", 256))
NAMED = ("cross", "wide", "sixteen", "shared", "black_outside", "two_pixels")
CASES = NAMED + ("strip255", "strip256", "strip257")

_cases = {}


def strip_case(width):
    """``panorama_cases.strip_case``: canvases 255, 256 and 257 wide here."""
    case = E.strip_case(width)
    assert S.panorama_size(case["center"].shape, case["geometries"])[0] == width
    return case


def get(name):
    """center, layers, geometries and the oracle's coordinates of a case; built once, read-only."""
    if name not in _cases:
        if name in NAMED:
            case = E.get(name)
            coords = RC.oracle_coords(name)
        else:
            case = strip_case(int(name[5:]))
            coords = [RC.layer_coords(l) for l in case["layers"]]
        _cases[name] = (case["center"], case["layers"], case["geometries"], coords)
    return _cases[name]


@pytest.fixture(scope="module")
def native_gpu(native):
    if native.lib().apap_device_count() < 1:
        pytest.skip("no HIP device")
    return native


def same(got, want, what):
    assert got.dtype == np.uint8 and got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere((got != want).any(axis=-1))
    assert len(bad) == 0, f"{what}: {len(bad)} pixels differ, first at (y, x) = {tuple(bad[0])}: {got[tuple(bad[0])]} != {want[tuple(bad[0])]}"


def center_rect(center, geos):
    _, _, OX, OY = S.panorama_size(center.shape, geos)
    return OX, OY, center.shape[1], center.shape[0]


@pytest.mark.parametrize("name", CASES)
def test_statistics(native_gpu, name):
    """N and S at steps 1, 2, 3 and 64 for both samplings: the specification over the engine's coordinates, and for the
    truncating sampler over the oracle's as well."""
    center, layers, geos, oracle = get(name)
    W, H, _, _ = S.panorama_size(center.shape, geos)
    own = RC.engine_coords(native_gpu, layers)
    for sampling in SAMPLINGS:
        values, _ = G.samples(center, layers, geos, own, sampling)
        by_oracle = G.samples(center, layers, geos, oracle, sampling)[0] if sampling == "nearest" else None
        for step in STEPS:
            N, Sm = native_gpu.panorama_gain_stats(center, layers, step=step, sampling=sampling)
            want_N, want_S = G.stats(values, step)
            assert N.dtype == Sm.dtype == np.uint64 and N.shape == Sm.shape == (len(layers) + 1,) * 2
            assert np.array_equal(N, want_N) and np.array_equal(Sm, want_S), (name, sampling, step, N, want_N, Sm, want_S)
            assert np.array_equal(N, N.T)
            if by_oracle is not None:
                o_N, o_S = G.stats(by_oracle, step)
                assert np.array_equal(N, o_N) and np.array_equal(Sm, o_S), (name, step, "the oracle's coordinates")
            if step == 64:
                assert N.max() <= ((W + 63) // 64) * ((H + 63) // 64)
                if name == "two_pixels":
                    assert N.max() <= 1     # the lattice is canvas pixel (0, 0) alone


def test_statistics_carry_past_32_bits(native_gpu):
    """A 2400 x 2400 all-255 centre and one identity layer on a 1 x 1 mesh, step 1: the strict test 0 < t drops the layer's
    row 0 and column 0, so N_01 = 2399^2 = 5 755 201 and S_01 = 765 N_01 = 4 402 728 765 > 2^32."""
    white = np.full((2400, 2400, 3), 255, np.uint8)
    layer = E.PanoramaLayer(white, np.eye(3, dtype=np.float32).reshape(1, 1, 3, 3), (np.array([0.0, 2400.0]), np.array([0.0, 2400.0])),
                            (2400, 2400), (0, 0))
    N, Sm = native_gpu.panorama_gain_stats(white, [layer], step=1)
    full, part = 2400 * 2400, 2399 * 2399
    assert 765 * part == 4_402_728_765 > 2 ** 32
    assert N.tolist() == [[full, part], [part, part]]
    assert Sm.tolist() == [[765 * full, 765 * part], [765 * part, 765 * part]]


@pytest.mark.parametrize("name", CASES)
def test_gained_canvases(native_gpu, name):
    """mean, paste and ramp (1, 8, 256) for both samplings under seeded random gains: the specification over the engine's
    coordinates, byte for byte; under q = 4096 everywhere: the engine's own ungained canvas."""
    from cvx_proj_amd import apap
    center, layers, geos, _ = get(name)
    rect = center_rect(center, geos)
    own = RC.engine_coords(native_gpu, layers)
    rng = np.random.default_rng(len(name) * 1000 + len(layers))
    v = len(layers) + 1
    q = rng.integers(G.MIN_Q, G.MAX_Q + 1, v).tolist()
    q[rng.integers(v)] = G.MAX_Q
    unit = [G.UNIT] * v
    grids = [np.array(l.local_homography) for l in layers]
    for sampling in SAMPLINGS:
        values, weight_of = G.samples(center, layers, geos, own, sampling)
        for blend, ramp in BLENDS:
            what = f"{name}, {sampling}, {blend} {ramp}"
            got, bounds = apap.panorama(center, layers, blend=blend, ramp=ramp, sampling=sampling, gain=q)
            assert bounds == S.panorama_size(center.shape, geos)
            same(got, G.compose(values, weight_of, rect, q, blend, ramp), what + ", random gains")
            plain, _ = apap.panorama(center, layers, blend=blend, ramp=ramp, sampling=sampling)
            same(apap.panorama(center, layers, blend=blend, ramp=ramp, sampling=sampling, gain=unit)[0], plain, what + ", q = 4096")
            same(plain, G.compose(values, weight_of, rect, unit, blend, ramp), what + ", the ungained specification")
    assert all(np.array_equal(g, l.local_homography) for g, l in zip(grids, layers)), "the grids are not modified"


def test_the_clamp_at_255(native_gpu):
    """The largest gain on near-white pictures (bytes 200 .. 255): every channel clamps."""
    from cvx_proj_amd import apap
    case = E.sixteen()
    rng = np.random.default_rng(255)
    center = rng.integers(200, 256, case["center"].shape, dtype=np.uint8)
    layers = [l._replace(img=rng.integers(200, 256, l.img.shape, dtype=np.uint8)) for l in case["layers"]]
    geos, rect = case["geometries"], center_rect(center, case["geometries"])
    own = RC.engine_coords(native_gpu, layers)
    q = [G.MAX_Q] * 17
    for sampling in SAMPLINGS:
        values, weight_of = G.samples(center, layers, geos, own, sampling)
        for blend, ramp in BLENDS:
            got, _ = apap.panorama(center, layers, blend=blend, ramp=ramp, sampling=sampling, gain=q)
            same(got, G.compose(values, weight_of, rect, q, blend, ramp), f"white, {sampling}, {blend} {ramp}")
            assert set(np.unique(got)) <= {0, 255} and (got == 255).any()


def test_a_sample_gained_to_black_is_still_present(native_gpu):
    """black_outside with its first layer all (1, 0, 0) under the smallest gain: the layer's samples become (0, 0, 0) and are
    still counted by mean and ramp and still win paste over the second layer."""
    from cvx_proj_amd import apap
    case = E.black_outside()
    center, geos = case["center"], case["geometries"]
    dim = np.zeros_like(case["layers"][0].img)
    dim[..., 0] = 1
    layers = [case["layers"][0]._replace(img=dim), case["layers"][1]]
    rect = center_rect(center, geos)
    own = RC.engine_coords(native_gpu, layers)
    q = [G.UNIT, G.MIN_Q, G.UNIT]
    for sampling in SAMPLINGS:
        values, weight_of = G.samples(center, layers, geos, own, sampling)
        both = values[1].any(axis=-1) & values[2].any(axis=-1) & ~values[0].any(axis=-1)
        assert both.sum() > 20, "the two layers overlap outside the centre"
        for blend, ramp in BLENDS:
            got, _ = apap.panorama(center, layers, blend=blend, ramp=ramp, sampling=sampling, gain=q)
            same(got, G.compose(values, weight_of, rect, q, blend, ramp), f"dim layer, {sampling}, {blend} {ramp}")
            if blend == "paste":
                assert not got[both].any(), "the black sample of the first layer is the paste winner"
            elif blend == "mean":
                assert np.array_equal(got[both], values[2][both] // 2), "the black sample is counted"


def test_auto(native_gpu):
    """gain="auto" is panorama_gains followed by the gained call; the resident chain's device solve gives the host solve's
    bits for the tables it read, and the same canvas."""
    import torch
    from cvx_proj_amd import apap, resident
    center, layers, geos, _ = get("cross")
    dev = torch.device("cuda", 0)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)      # noqa: E731
    d_center = up(center)
    d_layers = [apap.PanoramaLayer(up(l.img), up(l.local_homography), (up(l.mesh[0]), up(l.mesh[1])), l.final_size, l.offset) for l in layers]
    for sampling in SAMPLINGS:
        for (blend, ramp), step in zip(BLENDS, (1, 2, 3, 4, 1)):
            gains = apap.panorama_gains(center, layers, step=step, sampling=sampling)
            assert isinstance(gains, apap.PanoramaGains) and gains.q.tolist() == [G.quantise(g) for g in gains.gains]
            assert len(set(gains.q.tolist())) > 1, "random pictures: the gains differ"
            want, _ = apap.panorama(center, layers, blend=blend, ramp=ramp, sampling=sampling, gain=gains.q)
            got, _ = apap.panorama(center, layers, blend=blend, ramp=ramp, sampling=sampling, gain="auto", gain_step=step)
            same(got, want, f"auto, {sampling}, {blend} {ramp}")
            d_got, _, status, d_gains = resident.hip_panorama(d_center, d_layers, blend=blend, ramp=ramp, sampling=sampling, gain="auto",
                                                              gain_step=step, return_gains=True)
            N, Sm = d_gains.N.cpu().numpy().view(np.uint64), d_gains.S.cpu().numpy().view(np.uint64)
            assert np.array_equal(N, gains.N) and np.array_equal(Sm, gains.S) and not status.cpu().numpy().any()
            g, q, flag = native_gpu.panorama_gain_solve(N, Sm)
            assert flag == 0 and d_gains.gains.cpu().numpy().tobytes() == g.tobytes(), "the device solve's bits"
            assert d_gains.q.cpu().numpy().tolist() == q.tolist() == gains.q.tolist()
            same(d_got.cpu().numpy(), want, f"resident auto, {sampling}, {blend} {ramp}")
            d_q, _, _ = resident.hip_panorama(d_center, d_layers, blend=blend, ramp=ramp, sampling=sampling, gain=gains.q.tolist())
            same(d_q.cpu().numpy(), want, f"resident with q, {sampling}, {blend} {ramp}")


@pytest.mark.parametrize("name", ["cross", "wide"])
def test_device_forms_and_their_buffers(native_gpu, name):
    """The statistics into tables pre-filled with garbage, the auto chain into a guarded ``out``, both with a workspace of
    0xA5: the host-buffer forms' results, nothing written outside, the grids unchanged."""
    import torch
    from cvx_proj_amd import apap, resident
    center, layers, geos, _ = get(name)
    dev = torch.device("cuda", 0)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)      # noqa: E731
    d_center = up(center)
    d_layers = [apap.PanoramaLayer(up(l.img), up(l.local_homography), (up(l.mesh[0]), up(l.mesh[1])), l.final_size, l.offset) for l in layers]
    n = len(layers)
    grids = [l.local_homography.clone() for l in d_layers]
    W, H, _, _ = S.panorama_size(center.shape, geos)
    need = resident.panorama_workspace_bytes(d_layers)
    gains = apap.panorama_gains(center, layers, step=2)
    want, _ = apap.panorama(center, layers, blend="ramp", ramp=8, gain=gains.q)
    tables = torch.full((3, n + 1, n + 1), -0x0123456789ABCDF, dtype=torch.int64, device=dev)
    work = torch.full((need + 512,), 0xA5, dtype=torch.uint8, device=dev)
    status = torch.zeros(n + 2, dtype=torch.int32, device=dev)
    N, Sm, _ = resident.hip_panorama_gain_stats(d_center, d_layers, step=2, N=tables[0], S=tables[1], status=status, work=work)
    torch.cuda.synchronize(dev)
    assert N.data_ptr() == tables[0].data_ptr() and Sm.data_ptr() == tables[1].data_ptr()
    assert np.array_equal(N.cpu().numpy().view(np.uint64), gains.N) and np.array_equal(Sm.cpu().numpy().view(np.uint64), gains.S)
    assert bool((tables[2] == -0x0123456789ABCDF).all()), "the words behind the tables"
    assert bool((work[need:] == 0xA5).all()), "bytes past the workspace the call asked for"
    guard = 4096
    buf = torch.full((guard + H * W * 3 + guard,), 0x5C, dtype=torch.uint8, device=dev)
    out = buf[guard:guard + H * W * 3].view(H, W, 3)
    work.fill_(0xA5)
    got, _, status2, d_gains = resident.hip_panorama(d_center, d_layers, blend="ramp", ramp=8, out=out, status=status, work=work,
                                                     gain="auto", gain_step=2, return_gains=True)
    torch.cuda.synchronize(dev)
    assert got.data_ptr() == out.data_ptr() and status2.data_ptr() == status.data_ptr()
    same(got.cpu().numpy(), want, f"{name}, auto into out, 0xA5 workspace")
    assert d_gains.q.cpu().numpy().tolist() == gains.q.tolist()
    assert bool((buf[:guard] == 0x5C).all()) and bool((buf[guard + H * W * 3:] == 0x5C).all()), "guard bytes around out"
    assert bool((work[need:] == 0xA5).all()), "bytes past the workspace the call asked for"
    assert status.tolist() == [0] * (n + 2)
    assert all(torch.equal(g, l.local_homography) for g, l in zip(grids, d_layers)), "the grids are not modified"
    with pytest.raises(ValueError, match="gain"):
        resident.hip_panorama(d_center, d_layers, gain="manual")
    with pytest.raises(ValueError, match="step"):
        resident.hip_panorama_gain_stats(d_center, d_layers, step=2.5)


def test_command_line(native_gpu, tmp_path):
    """``--synth C1 --cases 1 --imgs 1,2,4,5 --panorama out.npy --panorama-gain auto --panorama-gain-step 8``:
    apap.panorama(gain="auto", gain_step=8) of the same four pairs; no torch."""
    from cvx_proj_amd import apap
    from cvx_proj_amd.synth import CONFIGS, synth_pair
    out = tmp_path / "pano.npy"
    code = ("import sys; from cvx_proj_amd import apap; rc = apap.main(sys.argv[1:]); "
            "assert 'torch' not in sys.modules, 'torch was imported'; sys.exit(rc)")
    r = subprocess.run([sys.executable, "-c", code, "--synth", "C1", "--cases", "1", "--imgs", "1,2,4,5", "--panorama", str(out),
                        "--panorama-gain", "auto", "--panorama-gain-step", "8", "--out-prefix", str(tmp_path) + "/"],
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
    want, bounds = apap.panorama(center, layers, gain="auto", gain_step=8)
    assert got.shape == (bounds[1], bounds[0], 3)
    same(got, want, "command line against apap.panorama")
    assert (want != apap.panorama(center, layers)[0]).any(), "the gains reach the kernel"
