"""Corner detection, descriptor extraction and matching on the MI355X at the edges that the byte-level suites of the three
kernels leave out (tests/test_feature_edge_inputs.py asserts on the CPU that the inputs reach them): the block's corner list
exactly full, the radix select's top digit, every combination of select and sort path, the radii next to the dispatch between
the two kernel instances; exact zero, equal and axis-aligned gradients in the descriptor's atan2, saturated and noise-only
descriptors, batches with a block's four waves in four images, non-finite coordinates on the resident form; infinite and
overflowing distances; first offsets above 0 in both batches.  Every comparison is byte for byte against the numpy
specifications (tests/corner_spec.py, tests/sift_spec.py, tests/match_spec.py)."""
import ctypes as C

import numpy as np
import pytest

import corner_spec as CS
import feature_edge_cases as E
import match_spec as MS
import sift_spec as SS
import test_gpu_corner as TC
import test_gpu_match as TM
import test_gpu_sift as TS

pytestmark = pytest.mark.gpu

SMALL_RADIUS = 5     # kSmallRadius of csrc/apap_corner.hip: k_corner_tile<5> serves radius <= 5, k_corner_tile<16> radius 6 .. 16


@pytest.fixture(scope="module")
def native_gpu(native):
    if native.lib().apap_device_count() < 1:
        pytest.skip("no HIP device")
    return native


@pytest.fixture(scope="module")
def spec(native_gpu):
    """The float32 descriptor specification with the constants the kernel uses."""
    taps, window = native_gpu.sift_taps(), native_gpu.sift_window()
    return lambda img, pts: SS.describe(img, np.asarray(pts, np.float32), taps, window)


def ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int))


def fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


# ---------------------------------------------------------------- corner detection
def corner_case(native, img, max_corners, quality, what, radius=1):
    TC.same(native.corner_detect(img, max_corners, radius, quality, full=True), CS.detect_full(img, max_corners, radius, quality), what)


def test_dense_image_full_block_lists(native_gpu):
    """Two tiles hold 512 corners, the whole of the block's list; 2790 corners share one response (rows 126 .. 2915 of the
    order), so 200, 2048 and 2049 cut inside it, the radix select keeps all 2916 at or above it and they sort in the workspace
    by index; 100 cuts a group of 62."""
    img = E.dense_image()
    cap = CS.bound(96, 128, 1)
    assert cap == 3072
    corner_case(native_gpu, img, cap, 0, "all corners")
    for k in (100, 200, 2048, 2049):
        corner_case(native_gpu, img, k, 0, f"max_corners {k}")
    pts, resp, n = native_gpu.corner_detect(img, cap, 1, 1000, full=True)
    assert n == 62 and len(set(resp[:62].tolist())) == 1
    corner_case(native_gpu, img, cap, 1000, "quality 1000")
    corner_case(native_gpu, img, cap, 500, "quality 500")
    corner_case(native_gpu, img, 2049, 500, "quality 500, max_corners 2049")


def test_binary_image_top_radix_digit(native_gpu):
    """Responses up to 2^48.35: 17 corners with the top digit 1, so a cut at 10 ends the select's first pass inside that digit
    and one at 100 below it; 5399 corners sort as 8192; 4096 and 4097 cut through equal responses."""
    img = E.binary_image()
    cap = CS.bound(256, 320, 1)
    want = CS.detect_full(img, cap, 1, 0)
    assert want[2] == 5399 and int(want[1][0]) >> 48 == 1
    TC.same(native_gpu.corner_detect(img, cap, 1, 0, full=True), want, "all corners")
    for k in (10, 100, 4096, 4097):
        corner_case(native_gpu, img, k, 0, f"max_corners {k}")


@pytest.mark.parametrize("k", [2048, 2049])
def test_prototype_scene_either_side_of_the_lds_sort(native_gpu, k):
    """2324 corners with distinct responses around row 2048: the select keeps exactly k, sorted in LDS at 2048 and in the
    workspace (padded to 4096) at 2049."""
    corner_case(native_gpu, CS.prototype_scene(), k, 0, f"max_corners {k}")


def radius_images():
    return [TC.image((33, 65), 3), TC.image((37, 53, 3), 4), np.tile(TC.image((16, 16), 5), (5, 7))]


@pytest.mark.parametrize("radius", [2, 4, SMALL_RADIUS + 1, 15])
@pytest.mark.parametrize("which", [0, 1, 2], ids=["(33, 65)", "(37, 53, 3)", "(80, 112) periodic"])
def test_radii_between_the_extremes(native_gpu, which, radius):
    assert 4 <= SMALL_RADIUS < 6
    img = radius_images()[which]
    assert img.shape == [(33, 65), (37, 53, 3), (80, 112)][which]
    cap = CS.bound(img.shape[0], img.shape[1], radius)
    want = CS.detect_full(img, cap, radius, 0)
    assert want[2] >= 1
    TC.same(native_gpu.corner_detect(img, cap, radius, 0, full=True), want, "all corners")
    corner_case(native_gpu, img, max(1, want[2] // 2), 0, "half", radius)


def test_corner_batch_of_extremes(native_gpu):
    imgs = [E.dense_image(), TC.image((7, 7), 1), E.binary_image()]
    singles = [native_gpu.corner_detect(im, 3000, 1, 0) for im in imgs]
    out = native_gpu.corner_detect_batch(imgs, 3000, 1, 0)
    assert len(out) == 3
    for m, ((pts, resp), (sp, sr)) in enumerate(zip(out, singles)):
        assert pts.shape == sp.shape and pts.tobytes() == sp.tobytes() and resp.tobytes() == sr.tobytes(), m
    assert [len(s[0]) for s in singles][::2] == [3000, 3000] and 0 < len(singles[1][0]) <= CS.bound(7, 7, 1)
    for m in (0, 1, 2):
        want = CS.detect(imgs[m], 3000, 1, 0)
        assert singles[m][0].tobytes() == want[0].tobytes() and singles[m][1].tobytes() == want[1].tobytes(), m


# ---------------------------------------------------------------- descriptor extraction
@pytest.mark.parametrize("name", ["vertical step", "horizontal step", "ramp", "diagonal step", "bright pixel"])
def test_structured_images(native_gpu, spec, name):
    """A keypoint on every pixel and on the two rings outside: gradients that are exactly 0 in one axis, in both, or equal in
    both (with the kernel's own taps), saturated rows next to the step, and rows made of the blur's last taps, scaled to full size."""
    img = E.structured_images()[name]
    classes = E.gradient_classes(img, native_gpu.sift_taps())
    if name != "bright pixel":
        assert sum(classes.values()) > 0 and max(classes["dx0"], classes["dy0"], classes["diag"]) > 300, classes
    else:
        assert min(classes.values()) > 0, classes
    pts = E.every_pixel_and_a_ring(*img.shape)
    want = spec(img, pts)
    assert int((want == 255).any(axis=1).sum()) > 100 and want.any(axis=1).sum() > 400
    TS.same_bytes(native_gpu.sift_describe(img, pts), want, "grey")
    TS.same_bytes(native_gpu.sift_describe(E.bgr(img), pts), spec(E.bgr(img), pts), "BGR")


def batch_case(n):
    imgs = E.batch_images(n)
    lengths = [1, 1, 1, 1, 1, 2, 3, 1, 6] if n == 9 else [1] * n
    rng = np.random.default_rng(n)
    pts = [rng.uniform(-2, [im.shape[1] + 2, im.shape[0] + 2], (k, 2)).astype(np.float32) for im, k in zip(imgs, lengths)]
    return imgs, lengths, pts


@pytest.mark.parametrize("n", [9, 65])
def test_descriptor_batches_of_single_keypoints(native_gpu, spec, n):
    """Most images hold one keypoint: the four waves of a block look up four different images, in tables of 9 and 65."""
    imgs, lengths, pts = batch_case(n)
    assert len(lengths) == n and lengths[:4] == [1, 1, 1, 1]
    out = native_gpu.sift_describe_batch(imgs, np.concatenate(pts), lengths)
    assert out.shape == (sum(lengths), 128)
    rows = TS.split_like(out, lengths)
    for m in range(n):
        TS.same_bytes(rows[m], native_gpu.sift_describe(imgs[m], pts[m]), f"image {m}")
        if n == 9:
            TS.same_bytes(rows[m], spec(imgs[m], pts[m]), f"image {m} against the specification")
    assert np.count_nonzero(out.any(axis=1)) > n // 2


def test_resident_form_non_finite_coordinates(native_gpu, spec):
    import torch
    from cvx_proj_amd import resident
    img = TS.scene(40, 50, seed=1)
    nan, inf = np.nan, np.inf
    pts = np.float32([[10, 12], [nan, 12], [20.5, 7], [inf, 7], [-inf, 9], [30, 30], [12, nan], [12, inf], [12, -inf], [nan, nan],
                      [45, 36], [-inf, inf], [3, 3]])
    bad = ~np.isfinite(pts).all(axis=1)
    assert bad[:4].tolist() == [False, True, False, True] and bad.sum() == 8     # valid and non-finite rows in one block
    dev = torch.device("cuda", 0)
    got = resident.hip_sift_describe(torch.from_numpy(img).to(dev), torch.from_numpy(pts).to(dev)).cpu().numpy()
    assert not got[bad].any() and got[~bad].any(axis=1).all()
    TS.same_bytes(got, spec(img, pts))
    with pytest.raises(ValueError):              # the host-buffer form refuses them
        native_gpu.sift_describe(img, pts)


# ---------------------------------------------------------------- matching
def never_chosen_case(native, q_row, q_value, t_row, t_value):
    """Query row 5 gets ``q_value`` in one entry and train row 7 ``t_value`` in another: every d2 of either is +inf."""
    rng = np.random.default_rng(6)
    q, t = TM.ints(rng, 70), TM.ints(rng, 200)
    clean = MS.match_int(np.delete(q, q_row, axis=0), np.delete(t, t_row, axis=0))
    q[q_row, 17] = q_value
    t[t_row, 100] = t_value
    idx, dist, idx2, dist2 = native.match_descriptors(q, t)
    assert (idx[q_row], idx2[q_row], dist[q_row], dist2[q_row]) == (-1, -1, np.inf, np.inf)
    assert not np.any(idx == t_row) and not np.any(idx2 == t_row)
    others = np.arange(len(q)) != q_row
    lift = lambda i: i + (i >= t_row)     # noqa: E731   indices of the train set without the row -> with it
    TM.same_bytes((idx[others], dist[others], idx2[others], dist2[others]), (lift(clean[0]), clean[1], lift(clean[2]), clean[3]))
    return q, t


def test_infinite_entries_are_never_selected(native_gpu):
    q, t = never_chosen_case(native_gpu, 5, np.inf, 7, -np.inf)
    never_chosen_case(native_gpu, 69, -np.inf, 199, np.inf)          # the last rows: the other signs
    # a train set of infinite rows only: nothing to select, whatever the signs (inf - inf is NaN)
    r = native_gpu.match_descriptors(q[:6], np.stack([np.full(MS.DIM, np.inf, np.float32), np.full(MS.DIM, -np.inf, np.float32)]))
    assert r[0].tolist() == [-1] * 6 and r[2].tolist() == [-1] * 6 and np.all(np.isposinf(r[1])) and np.all(np.isposinf(r[3]))


def test_overflowing_distances_are_never_selected(native_gpu):
    """Finite entries of 1e20 and -1e20: the squared difference is 1e40, +inf in float32."""
    assert np.isfinite(np.float32(1e20)) and float(np.float32(1e20)) ** 2 > float(np.finfo(np.float32).max)
    never_chosen_case(native_gpu, 5, 1e20, 7, -1e20)
    never_chosen_case(native_gpu, 64, -1e20, 128, 1e20)


# ---------------------------------------------------------------- first offsets above 0
Q_OFFSET, T_OFFSET = [3, 70, 200], [5, 133, 400]
MATCH_SENTINEL = (-7, -7.0, -7, -7.0)


@pytest.fixture(scope="module")
def offset_pairs(native_gpu):
    """Concatenated descriptors whose first pair starts at rows 3 and 5 (the rows before them are NaN: never to be read), and
    every pair's own single call."""
    rng = np.random.default_rng(9)
    q, t = TM.ints(rng, Q_OFFSET[-1]), TM.ints(rng, T_OFFSET[-1])
    q[:Q_OFFSET[0]] = np.nan
    t[:T_OFFSET[0]] = np.nan
    singles = [native_gpu.match_descriptors(q[Q_OFFSET[p]:Q_OFFSET[p + 1]], t[T_OFFSET[p]:T_OFFSET[p + 1]]) for p in range(2)]
    TM.same_bytes(singles[1], MS.match_int(q[Q_OFFSET[1]:], t[T_OFFSET[1]:]))
    return q, t, singles


def check_match_offsets(got, singles, what):
    for name, g, s in zip(TM.NAMES, got, MATCH_SENTINEL):
        assert np.all(g[:Q_OFFSET[0]] == s), (what, name, "rows before the first offset were written")
    for p in range(2):
        TM.same_bytes([g[Q_OFFSET[p]:Q_OFFSET[p + 1]] for g in got], singles[p], f"{what}, pair {p}")


def test_match_batch_with_a_first_offset_host_buffers(native_gpu, offset_pairs):
    q, t, singles = offset_pairs
    qo, to = np.array(Q_OFFSET, np.int32), np.array(T_OFFSET, np.int32)
    n = len(q)
    out = [np.full(n, s, dt) for s, dt in zip(MATCH_SENTINEL, (np.int32, np.float32, np.int32, np.float32))]
    native_gpu.check(native_gpu.lib().apap_match_descriptors_batch(None, fp(q), fp(t), ip(qo), ip(to), 2, ip(out[0]), fp(out[1]), ip(out[2]),
                                                                   fp(out[3]), -1))
    check_match_offsets(out, singles, "host buffers")


def test_match_batch_with_a_first_offset_device(native_gpu, offset_pairs):
    import torch
    q, t, singles = offset_pairs
    qo, to = np.array(Q_OFFSET, np.int32), np.array(T_OFFSET, np.int32)
    dev = torch.device("cuda", 0)
    n = len(q)
    need = native_gpu.lib().apap_match_batch_workspace_bytes(ip(qo), ip(to), 2)
    rel = native_gpu.lib().apap_match_batch_workspace_bytes(ip(qo - qo[0]), ip(to - to[0]), 2)
    assert need == rel > 0                      # the workspace depends on the pairs' sizes, not on where they start
    dq, dt = torch.from_numpy(q).to(dev), torch.from_numpy(t).to(dev)
    out = [torch.full((n,), s, dtype=d, device=dev) for s, d in zip(MATCH_SENTINEL, (torch.int32, torch.float32, torch.int32, torch.float32))]
    work = torch.empty(need, dtype=torch.uint8, device=dev)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    native_gpu.check(native_gpu.lib().apap_match_descriptors_batch_device(None, dq.data_ptr(), dt.data_ptr(), ip(qo), ip(to), 2,
                                                                          out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(),
                                                                          out[3].data_ptr(), work.data_ptr(), need, stream))
    torch.cuda.synchronize(dev)
    check_match_offsets([x.cpu().numpy() for x in out], singles, "device")


PT_OFFSET = [2, 7, 137]
SIFT_SENTINEL = -7.0


@pytest.fixture(scope="module")
def offset_keypoints(native_gpu, spec):
    """Two images, grey and BGR, whose keypoints start at row 2 of the concatenated array (the rows before are NaN, which the
    host-buffer form refuses where it reads them), and every image's own single call."""
    imgs = [SS.grey(TS.scene(23, 31, seed=4)).copy(), TS.scene(40, 50, seed=5)]
    rng = np.random.default_rng(10)
    pts = np.full((PT_OFFSET[-1], 2), np.nan, np.float32)
    for m, im in enumerate(imgs):
        pts[PT_OFFSET[m]:PT_OFFSET[m + 1]] = rng.uniform(-2, [im.shape[1] + 2, im.shape[0] + 2], (PT_OFFSET[m + 1] - PT_OFFSET[m], 2))
    singles = [native_gpu.sift_describe(im, pts[PT_OFFSET[m]:PT_OFFSET[m + 1]]) for m, im in enumerate(imgs)]
    TS.same_bytes(singles[1], spec(imgs[1], pts[PT_OFFSET[1]:]))
    assert singles[0].any() and singles[1].any()
    return imgs, pts, singles


def check_sift_offsets(out, singles, what):
    assert np.all(out[:PT_OFFSET[0]] == SIFT_SENTINEL), (what, "rows before the first offset were written")
    for m in range(2):
        TS.same_bytes(out[PT_OFFSET[m]:PT_OFFSET[m + 1]], singles[m], f"{what}, image {m}")


def sift_tables(imgs):
    i32 = lambda v: np.array(v, np.int32)     # noqa: E731
    return i32([im.shape[0] for im in imgs]), i32([im.shape[1] for im in imgs]), i32([1 if im.ndim == 2 else 3 for im in imgs]), i32(PT_OFFSET)


def test_sift_batch_with_a_first_offset_host_buffers(native_gpu, offset_keypoints):
    imgs, pts, singles = offset_keypoints
    hs, ws, cs, off = sift_tables(imgs)
    ptrs = (C.c_void_p * 2)(*[im.ctypes.data for im in imgs])
    out = np.full((len(pts), 128), SIFT_SENTINEL, np.float32)
    native_gpu.check(native_gpu.lib().apap_sift_describe_batch(None, ptrs, ip(hs), ip(ws), ip(cs), 2, fp(pts), ip(off), fp(out), -1))
    check_sift_offsets(out, singles, "host buffers")


def test_sift_batch_with_a_first_offset_device(native_gpu, offset_keypoints):
    import torch
    imgs, pts, singles = offset_keypoints
    hs, ws, cs, off = sift_tables(imgs)
    dev = torch.device("cuda", 0)
    d_imgs = [torch.from_numpy(im).to(dev) for im in imgs]
    ptrs = (C.c_void_p * 2)(*[im.data_ptr() for im in d_imgs])
    d_pts = torch.from_numpy(pts).to(dev)
    out = torch.full((len(pts), 128), SIFT_SENTINEL, dtype=torch.float32, device=dev)
    need = native_gpu.lib().apap_sift_workspace_bytes(2)
    work = torch.empty(need, dtype=torch.uint8, device=dev)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    native_gpu.check(native_gpu.lib().apap_sift_describe_batch_device(None, ptrs, ip(hs), ip(ws), ip(cs), 2, d_pts.data_ptr(), ip(off),
                                                                      out.data_ptr(), work.data_ptr(), need, stream))
    torch.cuda.synchronize(dev)
    check_sift_offsets(out.cpu().numpy(), singles, "device")
