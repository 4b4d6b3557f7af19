"""The low-pass slots of a two-band call, the overlap statistics of a block with two strips, the lattice widths around a wave,
and the device gain solve on every kind of table (k_box_blur's multi-picture launch, k_panorama_stats, k_panorama_gain_solve):
bytes and integers against tests/panorama_band_spec.py, tests/panorama_gain_spec.py and the host solve, on the inputs of
tests/panorama_edge_cases.py (tests/test_panorama_edge_inputs.py shows that each reaches its edge)."""
import numpy as np
import pytest

import panorama_band_spec as P
import panorama_edge_cases as X
import panorama_gain_spec as G
import panorama_ramp_cases as RC
import panorama_spec as S

pytestmark = pytest.mark.gpu

SAMPLINGS = ("nearest", "bilinear")
FILL = 0xA5


@pytest.fixture(scope="module")
def native_gpu(native):
    if native.lib().apap_device_count() < 1:
        pytest.skip("no HIP device")
    return native


def same(got, want, what):
    assert got.dtype == np.uint8 and got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere(got != want)
    assert len(bad) == 0, f"{what}: {len(bad)} bytes differ, first at {tuple(bad[0])}: {got[tuple(bad[0])]} != {want[tuple(bad[0])]}"


def upload(center, layers, share=True):
    """The case on device 0.  ``share``: one tensor per picture OBJECT, so a layer that is the centre's picture gets the
    centre's tensor and two layers of one picture one tensor; else a tensor of its own for every view."""
    import torch
    from cvx_proj_amd import apap
    dev = torch.device("cuda", 0)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)      # noqa: E731
    d_center = up(center)
    tensors = {id(center): d_center}
    d_layers = []
    for l in layers:
        if not share:
            img = up(l.img)
        else:
            if id(l.img) not in tensors:
                tensors[id(l.img)] = up(l.img)
            img = tensors[id(l.img)]
        d_layers.append(apap.PanoramaLayer(img, up(l.local_homography), (up(l.mesh[0]), up(l.mesh[1])), l.final_size, l.offset))
    return d_center, d_layers


def check_slots(native, name, ramp, band, sampling):
    """One ``hip_panorama(blend="band")`` into a workspace of 0xA5: every slot of a view that is blurred holds its low-pass
    picture, every other byte behind the warp slices is untouched, and the canvas is the spec's - and that of the same call
    on separate tensors."""
    import torch
    from cvx_proj_amd import resident
    center, layers, geos, _ = X.get(name)
    pictures = [center] + [l.img for l in layers]
    first = X.first_view_of(center, layers)
    d_center, d_layers = upload(center, layers)
    ptrs = [d_center.data_ptr()] + [l.img.data_ptr() for l in d_layers]
    assert [ptrs.index(p) for p in ptrs] == first, "a duplicate view is its first view's tensor"
    base = resident.panorama_workspace_bytes(d_layers)
    need = resident.panorama_band_workspace_bytes(d_center, d_layers, band)
    assert base > 0 and base % 256 == 0 and need == base + sum(X.up256(p.size) for p in pictures)
    work = torch.full((need + 512,), FILL, dtype=torch.uint8, device=d_center.device)
    assert work.data_ptr() % 256 == 0
    got, bounds, status = resident.hip_panorama(d_center, d_layers, blend="band", ramp=ramp, band=band, sampling=sampling, work=work)
    torch.cuda.synchronize(d_center.device)
    what = f"{name}, ramp {ramp}, band {band}, {sampling}"
    assert bounds == S.panorama_size(center.shape, geos) and status.tolist() == [0] * len(layers), what
    w = work.cpu().numpy()
    at = base
    for v, (picture, f) in enumerate(zip(pictures, first)):
        slot = w[at:at + X.up256(picture.size)]
        if f == v:
            same(slot[:picture.size].reshape(picture.shape), P.box_blur(picture, band), f"{what}: the slot of view {v}")
            assert (slot[picture.size:] == FILL).all(), f"{what}: the padding behind the slot of view {v}"
        else:
            assert (slot == FILL).all(), f"{what}: the slot of view {v}, which shares view {f}'s picture, is not used"
        at += len(slot)
    assert at == need and (w[need:] == FILL).all(), f"{what}: bytes past the workspace the call asked for"
    own = RC.engine_coords(native, layers)
    same(got.cpu().numpy(), P.compose_band(center, layers, geos, own, ramp, band, sampling=sampling).canvas, what + ", against the engine's coordinates")
    s_center, s_layers = upload(center, layers, share=False)
    apart, _, _ = resident.hip_panorama(s_center, s_layers, blend="band", ramp=ramp, band=band, sampling=sampling)
    same(got.cpu().numpy(), apart.cpu().numpy(), what + ", against the call on separate tensors")
    same(d_center.cpu().numpy(), center, "the centre is not modified")


@pytest.mark.parametrize("ramp,band,sampling", [(8, 16, "nearest"), (8, 17, "nearest"), (256, 32, "nearest"), (8, 17, "bilinear")],
                         ids=lambda v: str(v))
def test_low_pass_slots_of_shared_pictures(native_gpu, ramp, band, sampling):
    """blur_views: four blurred pictures of 9, 4, 1 and 5 tiles (15, 6, 1 and 10 above r = 16) in one launch; the centre's own
    tensor as a layer and a layer's tensor as a later layer sit between them and are not blurred again."""
    check_slots(native_gpu, "blur_views", ramp, band, sampling)


def test_low_pass_slots_of_17_views(native_gpu):
    """sixteen at band 17: 17 descriptors, a tile each."""
    check_slots(native_gpu, "sixteen", 8, 17, "nearest")


def check_statistics(native, name, steps):
    """N and S of the host-buffer and the device form at ``steps`` for both samplings: the spec over the engine's coordinates
    and, for the truncating sampler, over the oracle's."""
    import torch
    from cvx_proj_amd import resident
    center, layers, geos, oracle = X.get(name)
    own = RC.engine_coords(native, layers)
    d_center, d_layers = upload(center, layers)
    for sampling in SAMPLINGS:
        values, _ = G.samples(center, layers, geos, own, sampling)
        by_oracle = G.samples(center, layers, geos, oracle, sampling)[0] if sampling == "nearest" else None
        for step in steps:
            want_N, want_S = G.stats(values, step)
            N, Sm = native.panorama_gain_stats(center, layers, step=step, sampling=sampling)
            d_N, d_S, status = resident.hip_panorama_gain_stats(d_center, d_layers, step=step, sampling=sampling)
            torch.cuda.synchronize(d_center.device)
            d_N, d_S = d_N.cpu().numpy().view(np.uint64), d_S.cpu().numpy().view(np.uint64)
            what = (name, sampling, step)
            assert N.dtype == Sm.dtype == np.uint64 and N.shape == Sm.shape == want_N.shape and status.tolist() == [0] * len(layers), what
            assert np.array_equal(N, want_N) and np.array_equal(Sm, want_S), (what, "host buffers", N, want_N, Sm, want_S)
            assert np.array_equal(d_N, want_N) and np.array_equal(d_S, want_S), (what, "device form", d_N, want_N, d_S, want_S)
            if by_oracle is not None:
                o_N, o_S = G.stats(by_oracle, step)
                assert np.array_equal(N, o_N) and np.array_equal(Sm, o_S), (what, "the oracle's coordinates")


def test_statistics_of_a_block_with_two_unlike_strips(native_gpu):
    """tall: 4108 strips at step 1; the blocks 0 .. 11 see the centre with views 1 and 4 in their first strip and with views 2
    and 3 in their second."""
    W, H, _, _ = X.canvas("tall")
    assert X.stat_strips(W, H, 1)[2] > X.STAT_BLOCKS
    check_statistics(native_gpu, "tall", (1, 2, 3))


@pytest.mark.parametrize("step", sorted(X.STRIP_WIDTHS))
def test_statistics_at_lattices_of_a_wave_and_a_column_more(native_gpu, step):
    """Lattices of 256, 256 and 257 columns at steps 2 and 3."""
    for width in X.STRIP_WIDTHS[step]:
        W, H, _, _ = X.canvas(f"strip{width}")
        assert W == width and X.stat_strips(W, H, step)[0] == (257 if width % 256 == 1 else 256)
        check_statistics(native_gpu, f"strip{width}", (step,))


SOLVES = [(name, 10.0, 0.1) for name in X.SOLVE_CASES] + [("dim", 5.0, 1.0)]


@pytest.mark.parametrize("name,sigma_n,sigma_g", SOLVES, ids=[f"{n}-{a:g}-{b:g}" for n, a, b in SOLVES])
def test_device_solve(native_gpu, name, sigma_n, sigma_g):
    """The resident auto chain at step 1 under ``ramp`` 8: its tables are ``panorama_gains``', its gains the host solve's bits
    - and the spec's -, its q equal, the flag 0, its canvas the host-buffer call's under that q.  The chain does not return the
    device's flag: a raised one would have set every gain to 1.0, which the bits exclude wherever a gain differs from 1."""
    import torch
    from cvx_proj_amd import apap, resident
    center, layers, geos, _ = X.get(name)
    d_center, d_layers = upload(center, layers)
    gains = apap.panorama_gains(center, layers, step=1, sigma_n=sigma_n, sigma_g=sigma_g)
    got, bounds, status, d_gains = resident.hip_panorama(d_center, d_layers, blend="ramp", ramp=8, gain="auto", gain_step=1, sigma_n=sigma_n,
                                                         sigma_g=sigma_g, return_gains=True)
    torch.cuda.synchronize(d_center.device)
    assert bounds == S.panorama_size(center.shape, geos) and status.tolist() == [0] * len(layers)
    N, Sm = d_gains.N.cpu().numpy().view(np.uint64), d_gains.S.cpu().numpy().view(np.uint64)
    assert np.array_equal(N, gains.N) and np.array_equal(Sm, gains.S), (name, N, gains.N, Sm, gains.S)
    g, q, flag = native_gpu.panorama_gain_solve(N, Sm, sigma_n, sigma_g)
    d_g, d_q = d_gains.gains.cpu().numpy(), d_gains.q.cpu().numpy()
    assert flag == 0
    assert d_g.dtype == np.float64 and d_g.tobytes() == g.tobytes(), (name, "the device solve's bits", d_g, g)
    spec_g, spec_q, spec_flag = G.solve(N, Sm, sigma_n, sigma_g)
    assert spec_flag == 0 and d_g.tobytes() == np.array(spec_g, np.float64).tobytes(), (name, "the spec's bits", d_g, spec_g)
    assert d_q.dtype == np.int32 and d_q.tolist() == q.tolist() == gains.q.tolist() == spec_q, (name, d_q, q, gains.q, spec_q)
    assert (d_g != 1.0).any(), "a raised flag would have set every gain to 1.0"
    want, _ = apap.panorama(center, layers, blend="ramp", ramp=8, gain=q)
    same(got.cpu().numpy(), want, f"{name}: the auto chain's canvas against gain=q")
    values, weight_of = G.samples(center, layers, geos, RC.engine_coords(native_gpu, layers))
    _, _, OX, OY = bounds
    same(want, G.compose(values, weight_of, (OX, OY, center.shape[1], center.shape[0]), spec_q, "ramp", 8), f"{name}: gain=q against the spec")
    if name == "dim":
        assert d_q[0] == G.MIN_Q and 4096.0 * d_g[0] < G.MIN_Q, "the lower clamp"
    if name == "wide":
        alone = [v for v in range(len(N)) if all(N[v, u] == 0 for u in range(len(N)) if u != v)]
        assert alone and all(d_g[v] == 1.0 for v in alone), "the identity rows"
