"""The global warp and blend on the GPU (apap_image_warp*, utils.image_warping, resident.hip_image_warp*) against the numpy
specification of tests/image_warp_spec.py: the same bytes, at the kernel's edges (case set E of tests/image_warp_cases.py),
in batches of any order, on device tensors, and on pooled buffers shared with other host-buffer calls; and at the tiling's
edges (the sets sweep, tiling_cases and many of the same file): the base rectangle at every residue of a lane's group of 4,
canvases of several blocks along a row inside a batch, 521 problems in one launch, both pictures 1 x 1."""
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


# ---------------------------------------------------------------- the tiling sets (caller-chosen geometry)
def run_batch(native, problems, out=None, out_offsets=None):
    return native.image_warp_batch([p[1] for p in problems], [p[2] for p in problems], [p[3] for p in problems], [p[4] for p in problems],
                                   [p[5] for p in problems], [p[6] for p in problems], out=out, out_offsets=out_offsets)


def run_single(native, p):
    return native.image_warp(p[1], p[2], p[3], p[4][0], p[4][1], p[5][0], p[5][1], p[6])


def frozen(canvases):
    for c in canvases:
        c.setflags(write=False)
    return canvases


@pytest.fixture(scope="module")
def tiling():
    """tiling_cases() and the specification's canvas of each, computed once."""
    problems = E.tiling_cases()
    return problems, frozen([E.expected(p) for p in problems])


@pytest.fixture(scope="module")
def many():
    problems = E.many()
    return problems, frozen([S.image_warping(*p) for p in problems])


def test_base_rectangle_at_every_residue_of_a_lanes_group(native_gpu):
    """sweep(): 80 problems in one launch, the base rectangle's two vertical edges at all 16 pairs of residues mod 4, base
    pictures narrower than a lane's group strictly inside one, both modes; every eleventh also as its own single call."""
    problems = E.sweep()
    want_ = [E.expected(p) for p in problems]
    got = run_batch(native_gpu, problems)
    assert len(got) == len(problems) == 80
    for p, canvas, w in zip(problems, got, want_):
        same(canvas, w, f"sweep batch, {p[0]}")
    for k in range(0, len(problems), 11):
        same(run_single(native_gpu, problems[k]), want_[k], f"sweep single, {problems[k][0]}")


def test_wide_canvases_inside_a_batch(native_gpu, tiling):
    """tiling_cases(): 1, 2, 3 and 4 blocks along a row within one launch, behind problems that move the first block off 0, in
    three orders; the canvases at odd gaps in a poisoned buffer, placed in another order than the problems."""
    problems, want_ = tiling
    n = len(problems)
    rng = np.random.default_rng(9)
    sizes = [w.size for w in want_]
    for order in (list(range(n)), list(range(n))[::-1], [int(i) for i in rng.permutation(n)]):
        place = rng.permutation(n)                       # the position of each problem's canvas in the buffer
        offsets, at = [0] * n, 7
        for j in np.argsort(place):
            offsets[j] = at
            at += sizes[order[j]] + (1, 3, 5, 7, 11)[j % 5]
        out = np.full(at + 32, 0xA5, np.uint8)
        got = run_batch(native_gpu, [problems[i] for i in order], out=out, out_offsets=offsets)
        untouched = np.ones(out.size, bool)
        for i, canvas, o in zip(order, got, offsets):
            same(canvas, want_[i], f"order {order[:3]}..., {problems[i][0]} at offset {o}")
            assert np.array_equal(out[o:o + sizes[i]], want_[i].ravel())
            untouched[o:o + sizes[i]] = False
        assert (out[untouched] == 0xA5).all() and untouched.sum() == out.size - sum(sizes)


def test_each_wide_problem_equals_its_own_single_call(native_gpu, tiling):
    for p, w in zip(*tiling):
        same(run_single(native_gpu, p), w, f"single call, {p[0]}")


def test_521_problems_in_one_launch(native_gpu, many):
    """The host-buffer form and the resident form (a poisoned workspace of exactly the size asked for, canvases one poisoned
    byte apart) on many(): the descriptor table is 75 KB, the bisection ten levels deep, every neighbour another problem."""
    import torch
    from cvx_proj_amd import resident, utils
    problems, want_ = many
    n = len(problems)
    assert n == E.MANY == 521
    got = utils.image_warping_batch(problems)
    assert len(got) == n
    for k, (canvas, w) in enumerate(zip(got, want_)):
        same(canvas, w, f"host-buffer batch of {n}, problem {k}")
    dev = torch.device("cuda")
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)      # noqa: E731
    dprobs = [(up(b), up(s), H, d) for b, s, H, d in problems]
    sizes = [w.size for w in want_]
    offsets = [int(v) for v in np.cumsum([3] + [s + 1 for s in sizes])[:-1]]
    need = resident.image_warp_workspace_bytes(n)
    assert need == (n * 144 + 255) // 256 * 256
    work = torch.full((need,), 0xFF, dtype=torch.uint8, device=dev)
    out = torch.full((offsets[-1] + sizes[-1] + 9,), 0x5A, dtype=torch.uint8, device=dev)
    views = resident.hip_image_warp_batch(dprobs, out=out, out_offsets=offsets, work=work)
    torch.cuda.synchronize()
    host = out.cpu().numpy()
    untouched = np.ones(host.size, bool)
    for k, (v, w, o, size) in enumerate(zip(views, want_, offsets, sizes)):
        assert v.data_ptr() == out.data_ptr() + o
        same(host[o:o + size].reshape(w.shape), w, f"resident batch of {n}, problem {k}")
        untouched[o:o + size] = False
    assert (host[untouched] == 0x5A).all() and untouched.sum() == 3 + (n - 1) + 9


def test_both_pictures_1x1(native_gpu):
    """Alone, in both modes, through the host-buffer and the resident single calls (in a batch: tiling_cases())."""
    import torch
    from cvx_proj_amd import resident, utils
    base, src, H = E.tiny_pair()
    assert base.shape == src.shape == (1, 1, 3)
    dev = torch.device("cuda")
    dbase, dsrc = torch.from_numpy(base).to(dev), torch.from_numpy(src).to(dev)
    for direct in (True, False):
        w = S.image_warping(base, src, H, direct)
        same(utils.image_warping(base, src, H, direct), w, f"1 x 1 pair, direct={direct}")
        same(resident.hip_image_warp(dbase, dsrc, H, direct).cpu().numpy(), w, f"1 x 1 pair, resident, direct={direct}")
