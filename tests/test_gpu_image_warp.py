"""The global warp and blend on the GPU (apap_image_warp*, utils.image_warping, resident.hip_image_warp*) against the numpy
specification of tests/image_warp_spec.py: the same bytes, at the kernel's edges (case set E of tests/image_warp_cases.py),
in batches of any order, on device tensors, and on pooled buffers shared with other host-buffer calls."""
import os

import numpy as np
import pytest

import image_warp_cases as E
import image_warp_spec as S

pytestmark = pytest.mark.gpu

CASES = E.cases()
NAMES = [c[0] for c in CASES]


@pytest.fixture(scope="module")
def native_gpu(native):
    if native.lib().apap_device_count() < 1:
        pytest.skip("no HIP device")
    return native


@pytest.fixture(scope="module")
def want():
    """The specification's canvas of every case of E in both modes, computed once: {(name, direct): canvas}."""
    out = {}
    for name, base, src, H in CASES:
        for direct in (True, False):
            out[name, direct] = S.image_warping(base, src, H, direct)
            out[name, direct].setflags(write=False)
    return out


def problems_of(order):
    by_name = {c[0]: c for c in CASES}
    return [(by_name[n][1], by_name[n][2], by_name[n][3], d) for n, d in order]


def same(got, want_, what):
    assert got.dtype == np.uint8 and got.shape == want_.shape, (what, got.shape, want_.shape)
    bad = np.argwhere((got != want_).any(axis=-1))
    assert len(bad) == 0, f"{what}: {len(bad)} pixels differ, first at (y, x) = {tuple(bad[0])}: {got[tuple(bad[0])]} != {want_[tuple(bad[0])]}"


@pytest.mark.parametrize("name", NAMES)
def test_image_warping_matches_the_specification(native_gpu, want, name):
    from cvx_proj_amd import utils
    _, base, src, H = next(c for c in CASES if c[0] == name)
    for direct in (True, False):
        same(utils.image_warping(base, src, H, direct), want[name, direct], f"{name} direct={direct}")
    same(utils.image_warping(base, src, H), want[name, True], f"{name}: direct_blend defaults to True")


def test_float32_and_float64_H_are_one_problem(native_gpu, want):
    from cvx_proj_amd import utils
    _, base, src, H32 = next(c for c in CASES if c[0] == "H_float32")
    for direct in (True, False):
        a, b = utils.image_warping(base, src, H32, direct), utils.image_warping(base, src, H32.astype(np.float64), direct)
        assert np.array_equal(a, b) and np.array_equal(want["H_float32", direct], want["H_float64", direct])


def test_batch_in_any_order_equals_the_single_calls(native_gpu, want):
    from cvx_proj_amd import utils
    everything = [(n, d) for n in NAMES for d in (True, False)]
    size = {k: want[k].size for k in everything}
    smallest = min(everything, key=size.get)
    rest = [k for k in everything if k != smallest]
    rng = np.random.default_rng(3)
    shuffled = [everything[i] for i in rng.permutation(len(everything))]
    single = {}
    for order in (everything, shuffled, everything[::-1], [smallest] + rest, rest + [smallest]):
        got = utils.image_warping_batch(problems_of(order))
        assert len(got) == len(order)
        for k, canvas in zip(order, got):
            same(canvas, want[k], f"batch of {len(order)}, problem {k}")
    for k in shuffled[:6]:
        (p,) = problems_of([k])
        single[k] = utils.image_warping(*p)
        same(utils.image_warping_batch([p])[0], single[k], f"batch of one, {k}")


def test_warp_results_shares_one_pair(native_gpu, want):
    """spectral_method.warp_results: two problems on one image pair with different H, in one call."""
    from cvx_proj_amd import spectral_method
    ref = np.load(os.path.join(E.GOLDEN, "image_warp_ref.npz"))
    base, src = ref["base"], ref["src"]
    baseline, result = spectral_method.warp_results(base, src, ref["H_neg_f64"], ref["H_persp_f32"])
    same(baseline, want["fixture_neg_f64", False], "warp_results baseline")
    same(result, want["fixture_persp_f32", False], "warp_results result")
    assert np.array_equal(baseline, ref["mean_neg_f64"]) and np.array_equal(result, ref["mean_persp_f32"])
    d0, d1 = spectral_method.warp_results(base, src, ref["H_pos_f32"], ref["H_persp_f64"], direct_blend=True)
    assert np.array_equal(d0, ref["direct_pos_f32"]) and np.array_equal(d1, ref["direct_persp_f64"])


def test_batch_writes_at_the_given_offsets_only(native_gpu, want):
    """Nonzero first offset, gaps of odd lengths between the canvases (so they start at any byte address), canvases placed in
    another order than the problems: every byte outside a canvas keeps its value."""
    order = [("width_4k1", False), ("width_4", True), ("src_1x1", False), ("width_4k3", False), ("half_ties", True), ("width_4k2", False)]
    probs = problems_of(order)
    geo = [native_gpu.image_warp_geometry(b.shape[0], b.shape[1], s.shape[0], s.shape[1], H) for b, s, H, _ in probs]
    sizes = [g[1] * g[2] * 3 for g in geo]
    place = [3, 0, 5, 1, 4, 2]                       # the position of each problem's canvas in the buffer
    offsets, at = [0] * len(order), 13
    for p in np.argsort(place):
        offsets[p] = at
        at += sizes[p] + (1, 7, 2, 5, 3, 11)[p]
    out = np.full(at + 29, 0xA5, np.uint8)
    got = native_gpu.image_warp_batch([p[0] for p in probs], [p[1] for p in probs], [g[0] for g in geo], [(g[1], g[2]) for g in geo],
                                      [(g[3], g[4]) for g in geo], [p[3] for p in probs], out=out, out_offsets=offsets)
    untouched = np.ones(out.size, bool)
    for k, canvas, o, n in zip(order, got, offsets, sizes):
        same(canvas, want[k], f"offset {o}, {k}")
        assert np.array_equal(out[o:o + n], want[k].ravel())
        untouched[o:o + n] = False
    assert (out[untouched] == 0xA5).all() and untouched.sum() == 13 + 29 + 29


def test_resident_forms_on_a_side_stream_with_a_poisoned_workspace(native_gpu, want):
    import torch
    from cvx_proj_amd import resident
    dev = torch.device("cuda")
    order = [(n, d) for n in ("fixture_persp_f64", "width_4k1", "width_4k2", "width_4k3", "width_4", "src_1x1", "w0_zero_line", "clamp_0",
                              "clamp_3", "half_ties", "src_one_channel", "rows_9") for d in (False, True)]
    probs = problems_of(order)
    tensors = {}

    def up(a):
        if id(a) not in tensors:
            tensors[id(a)] = torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        return tensors[id(a)]

    dprobs = [(up(b), up(s), H, d) for b, s, H, d in probs]
    sizes = [want[k].size for k in order]
    offsets, at = [], 5
    for n in sizes:
        offsets.append(at)
        at += n + 3                                   # the canvases start at any byte address, 3 poisoned bytes between them
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    out = torch.full((at + 16,), 0x5A, dtype=torch.uint8, device=dev)
    work = torch.full((resident.image_warp_workspace_bytes(len(order)),), 0xFF, dtype=torch.uint8, device=dev)
    work1 = torch.full((resident.image_warp_workspace_bytes(1),), 0xFF, dtype=torch.uint8, device=dev)
    assert work.numel() == (len(order) * 144 + 255) // 256 * 256 and work1.numel() == 256
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        got = resident.hip_image_warp_batch(dprobs, out=out, out_offsets=offsets, status=status, work=work)
        singles = [resident.hip_image_warp(b, s, H, d, status=status, work=work1) for b, s, H, d in dprobs[:8]]
        packed = resident.hip_image_warp_batch(dprobs[:3])
    side.synchronize()
    assert int(status.item()) == 0
    host = out.cpu().numpy()
    untouched = np.ones(host.size, bool)
    for k, canvas, o, n in zip(order, got, offsets, sizes):
        assert canvas.data_ptr() == out.data_ptr() + o
        same(canvas.cpu().numpy(), want[k], f"resident batch, {k}")
        untouched[o:o + n] = False
    # the bytes before each canvas (so before each first row) and after each last row
    assert (host[untouched] == 0x5A).all() and untouched.sum() == 5 + 3 * len(order) + 16
    for k, canvas in zip(order[:8], singles):
        same(canvas.cpu().numpy(), want[k], f"resident single, {k}")
    for k, canvas in zip(order[:3], packed):
        same(canvas.cpu().numpy(), want[k], f"resident batch packed back to back, {k}")
    with pytest.raises(native_gpu.ApapError):
        resident.hip_image_warp(torch.zeros((4, 4, 3), dtype=torch.uint8), dprobs[0][1], np.eye(3))       # a host tensor


def test_host_buffer_form_shares_the_pool_with_other_calls(native_gpu, want):
    """Twice on one context, another host-buffer call (apap_equalize_hist: S_IMG, S_OUT, S_WORK as well) in between and after."""
    from cvx_proj_amd import utils
    ctx = native_gpu.Context()
    img = np.random.default_rng(7).integers(0, 200, (33, 17, 3), dtype=np.uint8)
    eq0 = native_gpu.equalize_hist(img)
    big, small = next(c for c in CASES if c[0] == "w0_zero_line"), next(c for c in CASES if c[0] == "width_4")
    same(utils.image_warping(*big[1:], False, ctx=ctx), want["w0_zero_line", False], "first call")
    assert np.array_equal(native_gpu.equalize_hist(img, ctx=ctx), eq0)
    same(utils.image_warping(*small[1:], True, ctx=ctx), want["width_4", True], "second call, smaller buffers")
    got = utils.image_warping_batch(problems_of([("half_ties", False), ("width_4k3", True)]), ctx=ctx)
    same(got[0], want["half_ties", False], "batch on the context")
    same(got[1], want["width_4k3", True], "batch on the context")
    assert np.array_equal(native_gpu.equalize_hist(img, ctx=ctx), eq0)
    same(utils.image_warping(*big[1:], True, ctx=ctx), want["w0_zero_line", True], "third call")
    ctx.close()
    same(utils.image_warping(*big[1:], False), want["w0_zero_line", False], "the shared pool")


@pytest.mark.parametrize("direct", [True, False])
def test_medium_pair(native_gpu, direct):
    """A 512 x 384 pair on a canvas of about 700 x 500: several blocks along x as well."""
    from cvx_proj_amd import utils
    rng = np.random.default_rng(21)
    base, src = rng.integers(0, 256, (384, 512, 3), dtype=np.uint8), rng.integers(0, 256, (384, 512, 3), dtype=np.uint8)
    src[100:140, 200:300] = 0
    c, s = np.cos(0.05), np.sin(0.05)
    H = np.array([[1.02 * c, -1.02 * s, 171.3], [1.02 * s, 1.02 * c, -88.6], [4e-5, -3e-5, 1.0]], np.float32)
    spec = S.image_warping(base, src, H, direct)
    assert 650 <= spec.shape[1] <= 750 and 450 <= spec.shape[0] <= 560, spec.shape
    same(utils.image_warping(base, src, H, direct), spec, f"medium direct={direct}")
