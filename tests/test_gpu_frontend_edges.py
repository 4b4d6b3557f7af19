"""Histogram equalisation and the RANSAC seed homography on the MI355X at the edges of their kernels (csrc/apap_frontend.hip)
that seeded random shapes leave out; tests/test_frontend_edge_inputs.py asserts on the CPU that the inputs of
tests/frontend_edge_cases.py reach them.  Equalisation: every head offset with every channel count, 0 / 1 / 2 chunks in the
body, the shortest and longest tails, aligned and unaligned stores, images that end inside the head, first bins on the table
builder's wave boundaries, the grid-stride loop, the workspace's zero-on-return contract, error codes.  RANSAC: the last
partial block of hypotheses, the scoring stride at 255 / 256 / 257 points, the tie rule of the selection, all-NaN and partly
NaN tables, a wrapping counter, thresholds whose squares are 0 and inf, a best count of 3 and of 4, argument checks.  The
yardstick is oracle/frontend_oracle.py everywhere, byte for byte.  Last, the sampler that the seed homography shares with the
fundamental matrix (csrc/apap_ransac_dev.h) at its smallest pools, n = K and K + 1 for K = 4 and 8 draws: the fundamental
cases against tests/fundamental_spec.py."""
import ctypes

import numpy as np
import pytest

import frontend_edge_cases as E
import test_frontend as TF
from oracle import frontend_oracle as F

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5          # what the output buffer holds before a call, and must still hold wherever the call may not write
NULL = ctypes.c_void_p(0)


@pytest.fixture(scope="module")
def native_gpu(native):
    if native.lib().apap_device_count() < 1:
        pytest.skip("no HIP device")
    return native


def device():
    import torch
    return torch.device("cuda:0")


# ---------------------------------------------------------------- equalisation through apap_equalize_hist_device
def eq_workspace(native, C):
    import torch
    return torch.zeros(native.lib().apap_equalize_workspace_bytes(C), dtype=torch.uint8, device=device())


def counters_are_zero(work, C):
    """The REPLICAS x C x 256 uint32 counters at the start of the workspace: zero on entry, zero on return."""
    return not bool(work[:E.REPLICAS * C * 256 * 4].any())


def eq_device(native, img, off_in, off_out, work=None):
    """One device-entry call on byte buffers with 32 bytes of slack: the image ``off_in`` bytes after a 16-byte boundary, the
    output ``off_out`` bytes after one.  Asserts that nothing outside the output's bytes was written and that the workspace's
    counters are zero again; returns the output."""
    import torch
    dev = device()
    img = np.ascontiguousarray(img)
    h, w, C = img.shape
    nbytes = img.size
    work = eq_workspace(native, C) if work is None else work
    buf_in = torch.full((nbytes + 32,), 0x3C, dtype=torch.uint8, device=dev)     # a byte read from outside the image shows in the histogram
    buf_out = torch.full((nbytes + 32,), SENTINEL, dtype=torch.uint8, device=dev)
    assert buf_in.data_ptr() % 16 == 0 and buf_out.data_ptr() % 16 == 0 and 0 <= off_in < 16 and 0 <= off_out < 16
    buf_in[off_in:off_in + nbytes] = torch.from_numpy(img.ravel()).to(dev)
    native.check(native.lib().apap_equalize_hist_device(None, buf_in.data_ptr() + off_in, h, w, C, buf_out.data_ptr() + off_out,
                                                        work.data_ptr(), work.numel(), NULL))
    torch.cuda.synchronize()
    assert bool((buf_out[:off_out] == SENTINEL).all()) and bool((buf_out[off_out + nbytes:] == SENTINEL).all()), \
        f"{img.shape} in +{off_in} out +{off_out}: bytes outside the output were written"
    assert counters_are_zero(work, C), f"{img.shape} in +{off_in} out +{off_out}: the workspace's counters are not zero on return"
    return buf_out[off_out:off_out + nbytes].cpu().numpy().reshape(img.shape)


def same_image(got, want, what):
    bad = np.flatnonzero(got.ravel() != want.ravel())
    assert bad.size == 0, f"{what}: {bad.size} of {got.size} bytes differ, the first at byte {int(bad[0])}"


@pytest.mark.parametrize("off_in", E.HEAD_OFFSETS)
@pytest.mark.parametrize("C", [1, 2, 3, 4])
def test_equalize_every_head_with_0_1_2_chunks_and_every_tail(native_gpu, C, off_in):
    """The per-lane channel phase (head + 16 lane) % C with every head, the body of 0, 1 and 2 chunks, the tail at its
    shortest and longest; stores with the input's alignment and with another."""
    work = eq_workspace(native_gpu, C)                                  # one workspace for all: zero on return, never cleared
    for shape in E.eq_sizes(C, off_in):
        img = E.eq_image(shape)
        want = F.equalize_hist_image(img)
        for off_out in (off_in, E.other_offset(off_in)):
            same_image(eq_device(native_gpu, img, off_in, off_out, work), want, f"{shape} in +{off_in} out +{off_out}")


def test_equalize_images_that_end_inside_the_head(native_gpu):
    for shape, off_in in E.eq_tiny():
        img = E.eq_image(shape, seed=1)
        want = F.equalize_hist_image(img)
        for off_out in (off_in, E.other_offset(off_in), 0):
            same_image(eq_device(native_gpu, img, off_in, off_out), want, f"{shape} in +{off_in} out +{off_out}")


@pytest.mark.parametrize("kind", ["above", "two", "all"])
def test_equalize_first_bin_on_the_table_builders_wave_boundaries(native_gpu, kind):
    """eq_build_luts finds the first occupied bin through per-wave ballots and scans the bins after it: first bins 63 | 64,
    127 | 128, 191 | 192, 0 and 254, through the host-buffer form and the device entry."""
    for i0, plane in E.eq_bins(kind).items():
        want = F.equalize_hist_channel(plane)
        same_image(native_gpu.equalize_hist(plane), want, f"{kind}, first bin {i0}, host buffers")
        same_image(eq_device(native_gpu, plane[..., None], 0, 0)[..., 0], want, f"{kind}, first bin {i0}, device entry")
        same_image(eq_device(native_gpu, plane[..., None], 3, 6)[..., 0], want, f"{kind}, first bin {i0}, device entry +3")


def test_equalize_four_channels_do_not_leak_into_each_other(native_gpu):
    img = E.eq_four_channels()
    want = F.equalize_hist_image(img)
    got = native_gpu.equalize_hist(img)
    assert np.array_equal(got[..., 0], img[..., 0])                     # the constant channel is returned as it is
    same_image(got, want, "host buffers")
    for off_in, off_out in ((0, 0), (5, 5), (2, 9)):
        same_image(eq_device(native_gpu, img, off_in, off_out), want, f"device entry in +{off_in} out +{off_out}")
    for order in ((3, 2, 1, 0), (1, 0, 3, 2)):                          # the same planes in other channels
        same_image(native_gpu.equalize_hist(np.ascontiguousarray(img[..., order])), want[..., order], f"channels {order}")


def test_equalize_known_answers_ties_to_even(native_gpu):
    for plane, answer in E.eq_known_answers():
        assert native_gpu.equalize_hist(plane).tolist() == answer.tolist()
        assert eq_device(native_gpu, plane[..., None], 1, 2)[..., 0].tolist() == answer.tolist()
        for C in (2, 3, 4):                                             # the same plane in every channel of an interleaved image
            img = np.ascontiguousarray(np.stack([plane] * C, -1))
            assert native_gpu.equalize_hist(img).tolist() == np.stack([answer] * C, -1).tolist()


_strided = {}


def strided(C):
    """(image, oracle's answer) of the 18.9 MB image, built once."""
    if C not in _strided:
        img = E.eq_strided(C)
        _strided[C] = (img, F.equalize_hist_image(img))
    return _strided[C]


@pytest.mark.parametrize("off_in,off_out", [(0, 0), (5, 3)])
@pytest.mark.parametrize("C", [1, 2, 4])
def test_equalize_grid_stride_loop(native_gpu, C, off_in, off_out):
    """6144 chunks on the capped grid of 4096 waves: half of them carry a second chunk through the register double buffer,
    half do not."""
    img, want = strided(C)
    same_image(eq_device(native_gpu, img, off_in, off_out), want, f"{img.shape} in +{off_in} out +{off_out}")


def test_equalize_workspace_is_zero_on_return_and_reusable_without_a_memset(native_gpu):
    for C in (1, 2, 3, 4):
        work = eq_workspace(native_gpu, C)
        first = E.eq_image((37, 53, C), seed=2)
        second = np.ascontiguousarray(255 - E.eq_image((61, 47, C), seed=3))
        third = E.eq_image((1, 2 * E.CHUNK // C + 5, C), seed=4)
        for k, (img, offs) in enumerate(((first, (0, 0)), (second, (5, 3)), (third, (15, 15)), (first, (1, 1)))):
            got = eq_device(native_gpu, img, *offs, work)               # asserts the counters read zero after every call
            same_image(got, F.equalize_hist_image(img), f"C = {C}, call {k} on one workspace")


def test_equalize_error_codes_leave_the_output_untouched(native_gpu):
    import torch
    dev = device()
    lib = native_gpu.lib()
    h, w, C = 9, 11, 3
    img = torch.from_numpy(E.eq_image((h, w, C)).ravel()).to(dev)
    out = torch.full((h * w * 4 + 32,), SENTINEL, dtype=torch.uint8, device=dev)
    work = eq_workspace(native_gpu, 4)
    need = lib.apap_equalize_workspace_bytes(C)
    assert need == E.REPLICAS * C * 256 * 4 + 16 + C * 256 and lib.apap_equalize_workspace_bytes(0) == 0 == lib.apap_equalize_workspace_bytes(5)
    i, o, k = img.data_ptr(), out.data_ptr(), work.data_ptr()
    calls = {"0 channels": ((i, h, w, 0, o, k, work.numel()), native_gpu.ERR_INVALID_ARG),
             "5 channels": ((i, h, w, 5, o, k, work.numel()), native_gpu.ERR_INVALID_ARG),
             "h = 0": ((i, 0, w, C, o, k, work.numel()), native_gpu.ERR_INVALID_ARG),
             "w = 0": ((i, h, 0, C, o, k, work.numel()), native_gpu.ERR_INVALID_ARG),
             "null image": ((None, h, w, C, o, k, work.numel()), native_gpu.ERR_INVALID_ARG),
             "null output": ((i, h, w, C, None, k, work.numel()), native_gpu.ERR_INVALID_ARG),
             "null workspace": ((i, h, w, C, o, None, work.numel()), native_gpu.ERR_INVALID_ARG),
             "workspace at an odd address": ((i, h, w, C, o, k + 1, need), native_gpu.ERR_INVALID_ARG),
             "workspace one byte short": ((i, h, w, C, o, k, need - 1), native_gpu.ERR_WORKSPACE)}
    for what, (args, code) in calls.items():
        assert lib.apap_equalize_hist_device(None, *args, NULL) == code, what
        torch.cuda.synchronize()
        assert bool((out == SENTINEL).all()), f"{what}: the output was written"
        assert not bool(work.any()), f"{what}: the workspace was written"
    # the exact size is enough
    assert lib.apap_equalize_hist_device(None, i, h, w, C, o, k, need, NULL) == native_gpu.OK
    torch.cuda.synchronize()
    assert np.array_equal(out[:h * w * C].cpu().numpy(), F.equalize_hist_image(img.cpu().numpy().reshape(h, w, C)).ravel())


# ---------------------------------------------------------------- RANSAC through apap_ransac_device
def ransac_got(native, name, **kw):
    return TF.ransac_device(native, *E.ransac_cases()[name], **kw)


@pytest.mark.parametrize("name", list(E.ransac_cases()))
def test_ransac_device_edge_cases_are_bit_identical_to_the_oracle(native_gpu, name):
    """All K hypotheses (NaN pattern and values), all K counts, the winner and its count, the mask and the winner's matrix."""
    TF.assert_ransac_equals_core(ransac_got(native_gpu, name), E.ransac_core(name))


def test_ransac_tie_goes_to_the_first_hypothesis_with_the_most_inliers(native_gpu):
    """Hundreds of hypotheses share the maximum; the first is index 3, while tied indices 258 and 512 sit in selection threads
    2 and 0: a tie broken on the thread number, on the larger index or by '>=' inside a thread's scan picks another."""
    core = E.ransac_core("ties")
    got = ransac_got(native_gpu, "ties")
    assert np.array_equal(got["counts"], core["counts"])
    facts = E.tie_facts(got["counts"])
    assert got["result"][0] == facts["first"], \
        f"the selection took hypothesis {got['result'][0]}; the first of the {len(facts['tied'])} with the most inliers is {facts['first']}"
    assert got["result"][0] == 3 and got["result"][1] == 217


def outputs(got, K):
    """Every byte a call produced."""
    return (got["work"][:K * 76].cpu().numpy().tobytes(), got["H_best"].tobytes(), got["mask"].tobytes(), tuple(got["result"]))


@pytest.mark.parametrize("name", ["ties", "default"])
def test_ransac_does_not_depend_on_the_workspace_on_entry(native_gpu, name):
    case = E.ransac_cases()["ties"] if name == "ties" else TF.ransac_case(600, 0.3, seed=0)[:2] + (5.0, 512, F.RANSAC_SEED)
    K = case[3]
    first = TF.ransac_device(native_gpu, *case)
    TF.assert_ransac_equals_core(first, F.ransac_core(*case))
    want = outputs(first, K)
    again = TF.ransac_device(native_gpu, *case, work=first["work"])    # the workspace as the first call left it
    assert outputs(again, K) == want
    assert outputs(TF.ransac_device(native_gpu, *case, fill=0xFF), K) == want


def test_ransac_argument_checks_leave_the_outputs_untouched(native_gpu):
    import torch
    dev = device()
    lib = native_gpu.lib()
    n, K = 57, 65
    src, dst = E.ransac_cases()["n=57 K=65"][:2]
    d_src = torch.zeros(2 * n + 2, dtype=torch.float32, device=dev)
    d_src[1:2 * n + 1] = torch.from_numpy(src.ravel()).to(dev)          # the points start at a 4-byte, not 8-byte, address
    a_src, d_dst = torch.from_numpy(src).to(dev), torch.from_numpy(dst).to(dev)
    wb = lib.apap_ransac_workspace_bytes(n, K)
    assert wb == K * 76 and lib.apap_ransac_workspace_bytes(3, K) == 0 == lib.apap_ransac_workspace_bytes(n, 0)
    work = torch.full((wb + 8,), SENTINEL, dtype=torch.uint8, device=dev)
    Hb = torch.full((9,), -7.0, dtype=torch.float64, device=dev)
    mask = torch.full((n,), SENTINEL, dtype=torch.uint8, device=dev)
    res = torch.full((2,), -7, dtype=torch.int32, device=dev)
    assert a_src.data_ptr() % 8 == 0 and d_src.data_ptr() % 8 == 0 and work.data_ptr() % 8 == 0

    def call(src_ptr=a_src.data_ptr(), n=n, thresh=5.0, K=K, work_ptr=work.data_ptr(), work_bytes=wb, H_ptr=Hb.data_ptr()):
        return lib.apap_ransac_device(None, src_ptr, d_dst.data_ptr(), n, thresh, K, ctypes.c_ulonglong(F.RANSAC_SEED), H_ptr,
                                      mask.data_ptr(), res.data_ptr(), work_ptr, work_bytes, NULL)

    bad, short = native_gpu.ERR_INVALID_ARG, native_gpu.ERR_WORKSPACE
    calls = {"n = 3": (dict(n=3), bad), "0 iterations": (dict(K=0), bad), "2^24 + 1 iterations": (dict(K=(1 << 24) + 1, work_bytes=1 << 40), bad),
             "negative threshold": (dict(thresh=-1.0), bad), "NaN threshold": (dict(thresh=float("nan")), bad),
             "points at a 4-byte address": (dict(src_ptr=d_src.data_ptr() + 4), bad),
             "workspace at a 4-byte address": (dict(work_ptr=work.data_ptr() + 4), bad),
             "null output": (dict(H_ptr=None), bad), "workspace one byte short": (dict(work_bytes=wb - 1), short)}
    for what, (kw, code) in calls.items():
        assert call(**kw) == code, what
        torch.cuda.synchronize()
        assert bool((work == SENTINEL).all()) and bool((mask == SENTINEL).all()), f"{what}: workspace or mask written"
        assert Hb.cpu().tolist() == [-7.0] * 9 and res.cpu().tolist() == [-7, -7], f"{what}: outputs written"
    # the exact size is enough, and the bytes after it stay
    assert call() == native_gpu.OK
    torch.cuda.synchronize()
    assert res.cpu().tolist() == [E.ransac_core("n=57 K=65")["best"], E.ransac_core("n=57 K=65")["count"]]
    assert bool((work[wb:] == SENTINEL).all())


# ---------------------------------------------------------------- RANSAC through _native.find_homography_ransac
def test_find_homography_with_3_agreeing_points_returns_no_model(native_gpu):
    src, dst, thresh, K, seed = E.ransac_cases()["count 3"]
    assert E.ransac_core("count 3")["count"] == 3
    H, mask = native_gpu.find_homography_ransac(src, dst, thresh, iterations=K, seed=seed)
    assert H is None and mask.shape == (len(src), 1) and not mask.any()
    H_ref, mask_ref = F.ransac_homography(src, dst, thresh, iterations=K, seed=seed)
    assert H_ref is None and np.array_equal(mask, mask_ref)


def test_find_homography_with_4_agreeing_points_refits_those_4(native_gpu):
    src, dst, thresh, K, seed = E.ransac_cases()["count 4"]
    core = E.ransac_core("count 4")
    H, mask = native_gpu.find_homography_ransac(src, dst, thresh, iterations=K, seed=seed)
    assert H is not None and H.shape == (3, 3) and H.dtype == np.float64
    assert int(mask.sum()) == 4 and np.array_equal(mask.ravel(), core["mask"])
    keep = core["mask"].astype(bool)
    one_cell, _ = native_gpu.local_homography(src[keep], dst[keep], np.zeros((1, 1, 2)), 1.0, 1.0, want_weights=False)
    assert np.array_equal(H, one_cell[0, 0].astype(np.float64))         # the wrapper is that composition
    H_ref, mask_ref = F.ransac_homography(src, dst, thresh, iterations=K, seed=seed)
    assert np.array_equal(mask, mask_ref)
    print("4-point re-fit against the oracle's: largest difference", np.abs(H - H_ref).max())
    assert np.allclose(H, H_ref, rtol=1e-5, atol=1e-7), np.abs(H - H_ref).max()


@pytest.mark.parametrize("name", ["all NaN", "duplicates", f"seed {E.SEEDS[1]:#x}"])
def test_find_homography_on_nan_tables_and_a_wrapping_seed(native_gpu, name):
    src, dst, thresh, K, seed = E.ransac_cases()[name]
    H, mask = native_gpu.find_homography_ransac(src, dst, thresh, iterations=K, seed=seed)
    H_ref, mask_ref = F.ransac_homography(src, dst, thresh, iterations=K, seed=seed)
    assert mask.dtype == np.uint8 and np.array_equal(mask, mask_ref)
    assert (H is None) == (H_ref is None) == (name == "all NaN")
    if H is not None:
        assert np.array_equal(H, H_ref), np.abs(H - H_ref).max()        # the re-fit is the hot path: bit-exact float32


# ---------------------------------------------------------------- the shared sampler at its smallest pools, both estimators
@pytest.mark.parametrize("seed_name", list(E.POOL_SEEDS))
@pytest.mark.parametrize("model,n", E.SMALL_POOLS)
def test_sampler_smallest_pools_are_bit_identical_to_both_specifications(native_gpu, model, n, seed_name):
    """n = 4 / 5 through apap_ransac_device and n = 8 / 9 through apap_fundamental_batch_device at 65 iterations: the last
    draw modulo 1 and modulo 2, one live lane in the second block of hypotheses, a wrapping counter.  Every hypothesis, count,
    the winner, the mask (and F) against the estimator's own specification."""
    case, core = E.small_pool_case(model, n, seed_name), E.small_pool_core(model, n, seed_name)
    if model == "homography":
        TF.assert_ransac_equals_core(TF.ransac_device(native_gpu, *case), core)
    else:
        import test_gpu_fundamental as TG
        got = TG.run_resident(native_gpu, case.src, case.dst, [0, n], case.thresh, case.iterations, case.seed)
        TG.check_pair(got, 0, slice(0, n), core, case.name)
