"""SIFT descriptor extraction on the MI355X (apap_sift_describe and its batch, resident and Python forms) against the numpy
specification of tests/sift_spec.py: the same bytes, the specification evaluated with the library's own constants."""
import numpy as np
import pytest

import sift_spec as S
from test_sift_host import scene

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def native_gpu(native):
    if native.lib().apap_device_count() < 1:
        pytest.skip("no HIP device")
    return native


@pytest.fixture(scope="module")
def spec(native_gpu):
    """The float32 specification with the constants the kernel uses."""
    taps, window = native_gpu.sift_taps(), native_gpu.sift_window()
    return lambda img, pts: S.describe(img, np.asarray(pts, np.float32), taps, window)


def same_bytes(got, want, what=""):
    assert got.dtype == want.dtype == np.float32 and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    bad = np.flatnonzero((got.view(np.int32) != want.view(np.int32)).any(axis=1))
    assert got.tobytes() == want.tobytes(), (what, len(bad), "rows differ; first", int(bad[0]), got[bad[0]][:16], want[bad[0]][:16])


def test_7x7_every_pixel_and_outside(native_gpu, spec):
    rng = np.random.default_rng(7)
    img = rng.integers(0, 256, (7, 7)).astype(np.uint8)
    yy, xx = (a.ravel() for a in np.mgrid[:7, :7])
    pts = np.concatenate([np.stack([xx, yy], -1), [[-0.4, -0.6], [-3, 2], [6.5, 2.5], [3.5, 100]]]).astype(np.float32)
    got = native_gpu.sift_describe(img, pts)
    same_bytes(got, spec(img, pts))
    assert got[24].any() and not got[52].any()           # the centre has a descriptor, (3.5, 100) is far outside


@pytest.mark.parametrize("shape", [(9, 64), (64, 9), (37, 53, 3)], ids=str)
def test_small_and_narrow_images(native_gpu, spec, shape):
    rng = np.random.default_rng(sum(shape))
    img = rng.integers(0, 256, shape).astype(np.uint8)
    h, w = shape[:2]
    pts = np.concatenate([rng.uniform(-3, [w + 3, h + 3], (300, 2)), [[0, 0], [w - 1, h - 1], [1, 1], [w - 2, h - 2], [0.5, 1.5], [1.5, 2.5]]])
    got = native_gpu.sift_describe(img, pts)             # float64 coordinates: cast to float32 first
    same_bytes(got, spec(img, pts.astype(np.float32)))
    assert np.count_nonzero(got.any(axis=1)) > 100


@pytest.fixture(scope="module")
def big(native_gpu, spec):
    """128 x 96 BGR with 5000 keypoints, and the specification's descriptors, computed once."""
    img = scene()
    pts = np.random.default_rng(11).uniform(-2, [130, 98], (5000, 2)).astype(np.float32)
    return img, pts, spec(img, pts)


def block_edges(native):
    """Counts at the edges of the launch: one keypoint, one block, one more, many blocks plus one, from the binding's constant."""
    per = native.SIFT_BLOCK_KEYPOINTS
    assert per == 4
    return [1, per, per + 1, 16 * per + 1, 64 * per + 1, 5000]


@pytest.mark.parametrize("n", [1, 4, 5, 65, 257, 5000])
def test_bytes_equal_the_specification(native_gpu, big, n):
    assert n in block_edges(native_gpu)
    img, pts, want = big
    same_bytes(native_gpu.sift_describe(img, pts[:n]), want[:n], f"n = {n}")
    if n == 257:         # the tail of the list, so that other keypoints sit at the block's edge; and the grey plane alone
        same_bytes(native_gpu.sift_describe(img, pts[-n:]), want[-n:], "tail")
        same_bytes(native_gpu.sift_describe(S.grey(img), pts[:n]), want[:n], "grey")


@pytest.mark.parametrize("shape", [(7, 7, 3), (37, 53, 3)], ids=str)
def test_bgr_equals_its_grey(native_gpu, spec, shape):
    """test_gpu_corner.py::test_bgr_equals_its_grey for the descriptor: the kernels of both read an image through the same
    apap::grey_at.  Keypoints on the four corners, the four edge midpoints and the centre; at 7 x 7, the smallest image, every
    one of them reads reflected indices on all four sides."""
    import torch
    from cvx_proj_amd import resident
    h, w = shape[:2]
    img = np.random.default_rng(h * w).integers(0, 256, shape).astype(np.uint8)
    g = S.grey(img)
    assert g.shape == (h, w) and g.dtype == np.uint8
    pts = np.float32([[x, y] for y in (0, h // 2, h - 1) for x in (0, w // 2, w - 1)])
    a, b = native_gpu.sift_describe(img, pts), native_gpu.sift_describe(g, pts)
    same_bytes(a, b, "BGR against grey")
    same_bytes(b, spec(g, pts), "against the specification")
    assert a.shape == (9, 128) and a.any(axis=1).all()
    dev = torch.device("cuda", 0)
    d_pts = torch.from_numpy(pts).to(dev)
    da, db = (resident.hip_sift_describe(torch.from_numpy(x).to(dev), d_pts).cpu().numpy() for x in (img, g))
    same_bytes(da, db, "resident: BGR against grey")
    same_bytes(da, a, "resident against host buffers")


def test_zero_descriptors(native_gpu):
    img = scene(40, 50)
    far = np.float32([[-3, 5], [5, -3], [52, 5], [5, 42], [1e6, 1e6], [-1e30, 3], [3, 3e38], [-3.4, 5]])
    got = native_gpu.sift_describe(img, far)
    assert got.shape == (8, 128) and not got.any() and not np.isnan(got).any()
    for const in (np.zeros((40, 50), np.uint8), np.full((40, 50, 3), 255, np.uint8), np.full((7, 7), 9, np.uint8)):
        h, w = const.shape[:2]
        pts = np.random.default_rng(0).uniform(0, [w, h], (64, 2))
        got = native_gpu.sift_describe(const, pts)
        assert not got.any() and not np.isnan(got).any()


def translated_pair():
    """A centre image and the other image: the same scene shifted by (dx, dy) = (5, 3), with keypoints shifted alike."""
    world = scene(110, 140, seed=3)
    dx, dy = 5, 3
    c_img, o_img = world[:96, :128], world[dy:dy + 96, dx:dx + 128]         # o(y, x) = c(y + dy, x + dx)
    rng = np.random.default_rng(4)
    cells = rng.permutation(15 * 20)[:200]                                   # distinct pixels, 6 apart: distinct descriptors
    pts_c = np.stack([10 + 6 * (cells % 20), 8 + 6 * (cells // 20)], -1).astype(np.float64)
    pts_o = pts_c - [dx, dy]
    inner = np.all((pts_c >= 11) & (pts_c <= [128 - 12, 96 - 12]) & (pts_o >= 11) & (pts_o <= [128 - 12, 96 - 12]), axis=1)
    return np.ascontiguousarray(c_img), np.ascontiguousarray(o_img), pts_c, pts_o, inner


def test_translation(native_gpu):
    from cvx_proj_amd import features
    c_img, o_img, pts_c, pts_o, inner = translated_pair()
    assert inner.sum() > 100
    kc, fc = features.compute(c_img, pts_c)
    ko, fo = features.compute(o_img, pts_o)
    assert kc[0].pt == tuple(pts_c[0]) and kc[0].size == 1.0 and fc.dtype == np.float32 and fc.shape == (200, 128)
    same_bytes(fc[inner], fo[inner], "keypoints at least 11 px from every border")
    assert fc[inner].any(axis=1).all()
    # only the inner keypoints: the identity matching at distance 0
    k1, f1, k2, f2, matches = features.coarse_matching(c_img, o_img, pts_c[inner], pts_o[inner])
    assert len(k1) == len(k2) == len(matches) == inner.sum()
    same_bytes(f1, fc[inner])
    same_bytes(f2, fo[inner])
    assert [(m.queryIdx, m.trainIdx, m.distance) for m in matches] == [(i, i, 0.0) for i in range(int(inner.sum()))]
    src, dst, cf, of = features.matched_arrays(c_img, o_img, pts_c[inner], pts_o[inner])
    assert src.dtype == np.float32 and np.array_equal(src, pts_c[inner].astype(np.float32)) and np.array_equal(dst, pts_o[inner].astype(np.float32))
    same_bytes(cf, fc[inner])
    same_bytes(of, fo[inner])


@pytest.fixture(scope="module")
def ragged(native_gpu):
    """Three images of different shapes and channel counts, their keypoints, and every image's own single call."""
    rng = np.random.default_rng(5)
    imgs = [scene(40, 50, seed=1), S.grey(scene(9, 64, seed=2)), scene(96, 128, seed=3)]
    pts = [rng.uniform(-2, [im.shape[1] + 2, im.shape[0] + 2], (n, 2)).astype(np.float32) for im, n in zip(imgs, (5, 130, 259))]
    return imgs, pts, [native_gpu.sift_describe(im, p) for im, p in zip(imgs, pts)]


def split_like(a, lengths):
    at = np.cumsum([0] + list(lengths))
    return [a[at[m]:at[m + 1]] for m in range(len(lengths))]


@pytest.mark.parametrize("order", [(0, 1, 2), (2, 0, 1)], ids=["in order", "permuted"])
def test_batch_equals_the_single_calls(native_gpu, spec, ragged, order):
    imgs, pts, singles = ragged
    lengths = [len(pts[m]) for m in order]
    out = native_gpu.sift_describe_batch([imgs[m] for m in order], np.concatenate([pts[m] for m in order]), lengths)
    for m, got in zip(order, split_like(out, lengths)):
        same_bytes(got, singles[m], f"image {m}")
    same_bytes(singles[1], spec(imgs[1], pts[1]))         # so that the chain ends in numpy
    same_bytes(native_gpu.sift_describe(imgs[2], pts[2]), singles[2], "a second call")


def test_resident_and_features_forms_equal_the_host_buffer_forms(native_gpu, ragged):
    import torch
    from cvx_proj_amd import features, resident
    imgs, pts, singles = ragged
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    lengths = [len(p) for p in pts]
    with torch.cuda.stream(stream):
        d_imgs = [torch.from_numpy(im).to(dev) for im in imgs]
        d_pts = [torch.from_numpy(p).to(dev) for p in pts]
        assert resident.sift_workspace_bytes(3) == 256 and resident.sift_workspace_bytes(0) == 0
        work = torch.empty(256, dtype=torch.uint8, device=dev)
        one = [resident.hip_sift_describe(im, p, work=work) for im, p in zip(d_imgs, d_pts)]
        many = resident.hip_sift_describe_batch(d_imgs, torch.cat(d_pts), lengths, work=work)
    stream.synchronize()
    assert many.dtype == torch.float32 and tuple(many.shape) == (sum(lengths), 128)
    for m, got in enumerate(split_like(many.cpu().numpy(), lengths)):
        same_bytes(got, singles[m], f"batch, image {m}")
        same_bytes(one[m].cpu().numpy(), singles[m], f"single, image {m}")
    a, b = features.describe_pair(imgs[0], imgs[2], pts[0], pts[2])
    same_bytes(a, singles[0])
    same_bytes(b, singles[2])
    same_bytes(features.compute(imgs[1], pts[1])[1], singles[1])
    with pytest.raises(native_gpu.ApapError):     # a short workspace is refused, not replaced
        native_gpu.check(native_gpu.lib().apap_sift_describe_device(None, d_imgs[0].data_ptr(), 40, 50, 3, d_pts[0].data_ptr(), 5,
                                                                    one[0].data_ptr(), work.data_ptr(), 128, None))
    with pytest.raises(ValueError):
        resident.hip_sift_describe(d_imgs[0].float(), d_pts[0])
    with pytest.raises(native_gpu.ApapError):
        resident.hip_sift_describe(d_imgs[0], d_pts[0].cpu())


def test_describe_and_match_chain(native_gpu):
    import torch
    from cvx_proj_amd import features, resident
    c_img, o_img, pts_c, pts_o, inner = translated_pair()
    dev = torch.device("cuda", 0)
    ci, oi = torch.from_numpy(c_img).to(dev), torch.from_numpy(o_img).to(dev)
    pc, po = torch.from_numpy(pts_c.astype(np.float32)).to(dev), torch.from_numpy(pts_o.astype(np.float32)).to(dev)
    for second in (True, False):
        idx, dist, idx2, dist2, fc, fo = resident.hip_describe_and_match(ci, oi, pc, po, second=second)
        sc, so = resident.hip_sift_describe(ci, pc), resident.hip_sift_describe(oi, po)
        want = resident.hip_match_descriptors(sc, so, second=second)
        torch.cuda.synchronize(dev)
        assert torch.equal(fc, sc) and torch.equal(fo, so)
        for g, w in zip((idx, dist, idx2, dist2), want):
            assert (g is None and w is None and not second) or torch.equal(g, w)
    matches = features.coarse_matching(c_img, o_img, pts_c, pts_o)[4]
    assert [m.trainIdx for m in matches] == idx.cpu().tolist() and [m.distance for m in matches] == dist.cpu().tolist()
    assert np.array_equal(idx.cpu().numpy()[inner], np.flatnonzero(inner))
