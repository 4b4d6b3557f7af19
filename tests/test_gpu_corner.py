"""Corner detection on the MI355X (apap_corner_detect and its batch, resident and Python forms) against the numpy int64
specification of tests/corner_spec.py: the same bytes; then the chain from two images to matches and to a homography."""
import numpy as np
import pytest

import corner_spec as S
from test_corner_host import edge, rectangle, shifted_crops
from test_sift_host import scene

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def native_gpu(native):
    if native.lib().apap_device_count() < 1:
        pytest.skip("no HIP device")
    return native


def same(got, want, what=""):
    """(pts, response, count) of the library against the specification's, byte for byte; rows from count on are zero."""
    (gp, gr, gn), (wp, wr, wn) = got, want
    assert gp.dtype == np.float32 and gr.dtype == np.int64 and gp.shape == wp.shape and gr.shape == wr.shape, (what, gp.shape, wp.shape)
    assert int(gn) == wn, (what, "count", int(gn), wn)
    bad = np.flatnonzero((gp != wp).any(axis=1) | (gr != wr))
    assert gp.tobytes() == wp.tobytes() and gr.tobytes() == wr.tobytes(), \
        (what, len(bad), "rows differ; first", int(bad[0]), gp[bad[0]], gr[bad[0]], wp[bad[0]], wr[bad[0]])
    assert not gp[wn:].any() and not gr[wn:].any()


def image(shape, seed):
    """Seeded noise, lightly smoothed along x so that responses vary in strength; BGR when the shape says so."""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 256, shape[:2] + (shape[2] if len(shape) == 3 else 1,)).astype(np.int64)
    a = (a + np.roll(a, 1, axis=1)) // 2
    return a.astype(np.uint8).reshape(shape)


TILE_H, TILE_W = 32, 64
SHAPES = [(7, 7), (9, 130), (130, 9), (37, 53, 3), (TILE_H, TILE_W), (TILE_H + 1, TILE_W + 1), (200, 260)]


@pytest.mark.parametrize("radius", [1, 5, 16])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_bytes_equal_the_specification(native_gpu, shape, radius):
    """Every corner of the image (max_corners at the bound, quality 0); a short list at the default quality; the stronger half;
    a strict quality with more rows than the image can have corners."""
    assert (native_gpu.CORNER_TILE_H, native_gpu.CORNER_TILE_W) == (TILE_H, TILE_W)
    img = S.prototype_scene() if shape == (200, 260) else image(shape, sum(shape) + radius)
    cap = S.bound(shape[0], shape[1], radius)
    want = S.detect_full(img, cap, radius, 0)
    same(native_gpu.corner_detect(img, cap, radius, 0, full=True), want, "all corners")
    assert want[2] >= 1
    k = max(1, want[2] // 3)
    same(native_gpu.corner_detect(img, k, radius, 10, full=True), S.detect_full(img, k, radius, 10), "quality 10, a third")
    half = max(1, want[2] // 2)
    same(native_gpu.corner_detect(img, half, radius, 0, full=True), S.detect_full(img, half, radius, 0), "quality 0, half")
    same(native_gpu.corner_detect(img, cap + 7, radius, 500, full=True), S.detect_full(img, cap + 7, radius, 500), "quality 500, beyond the bound")


@pytest.mark.parametrize("radius", [1, 5, 16])
def test_ties(native_gpu, radius):
    """A periodic image: equal responses across periods, and at radius 16 inside one window.  The plateau rule and the index
    order against the specification, also with max_corners cutting through a group of equal responses."""
    img = np.tile(image((16, 16), 5), (5, 7))                # 80 x 112: several tiles, the period no divisor of the tile's height
    h, w = img.shape
    cap = S.bound(h, w, radius)
    want = S.detect_full(img, cap, radius, 0)
    R = S.response(img)
    assert np.array_equal(R[16:32, 16:32], R[32:48, 48:64])  # equal responses at distance 16 and 32: inside the window at radius 16
    same(native_gpu.corner_detect(img, cap, radius, 0, full=True), want, "all")
    resp = want[1][:want[2]]
    if radius < 16:
        start = np.flatnonzero(np.diff(resp) == 0)
        assert len(start) > 3
        for k in (int(start[0]) + 1, int(start[len(start) // 2]) + 1, int(start[-1]) + 1):   # row k - 1 and row k hold equal responses
            assert resp[k - 1] == resp[k]
            same(native_gpu.corner_detect(img, k, radius, 0, full=True), S.detect_full(img, k, radius, 0), f"cut at {k}")
    else:
        assert want[2] >= 1
    flat = np.full((40, 70), 17, np.uint8)
    flat[10:30, 20:50] = 99                                  # R = 0 on the plateaux: not corners; the four rectangle corners are
    same(native_gpu.corner_detect(flat, 50, radius, 0, full=True), S.detect_full(flat, 50, radius, 0), "plateaux")


def test_empty_results_and_rectangle(native_gpu):
    for img in (np.zeros((30, 40), np.uint8), np.full((7, 7, 3), 255, np.uint8), edge(), edge().T.copy(), np.stack([edge()] * 3, -1)):
        pts, resp, n = native_gpu.corner_detect(img, 50, 5, 0, full=True)
        assert n == 0 and pts.shape == (50, 2) and not pts.any() and not resp.any()
        pts, resp = native_gpu.corner_detect(img, 50)
        assert pts.shape == (0, 2) and resp.shape == (0,) and pts.dtype == np.float32 and resp.dtype == np.int64
    pts, resp = native_gpu.corner_detect(rectangle(), 100)
    assert sorted(map(tuple, pts.tolist())) == [(24.0, 20.0), (24.0, 43.0), (49.0, 20.0), (49.0, 43.0)]
    same(native_gpu.corner_detect(rectangle(), 100, full=True), S.detect_full(rectangle(), 100), "rectangle")


@pytest.fixture(scope="module")
def crops(native_gpu):
    """The translated pair, every corner of both crops (quality 0, max_corners at the bound) and the common inner corners for
    a margin: rows of (x, y) in the centre crop's frame, with both crops' row numbers."""
    radius = 5
    c_img, o_img, inner, (dx, dy) = shifted_crops(radius)
    h, w = c_img.shape
    cap = S.bound(h, w, radius)
    (pc, rc), (po, ro) = native_gpu.corner_detect(c_img, cap, radius, 0), native_gpu.corner_detect(o_img, cap, radius, 0)

    def common(margin):
        ok = lambda q: np.all((q >= margin) & (q <= [w - 1 - margin, h - 1 - margin]), axis=1)     # noqa: E731
        at_o = {(x + dx, y + dy): j for j, (x, y) in enumerate(po.tolist())}
        rows = [(i, at_o[tuple(q)]) for i, q in enumerate(pc.tolist()) if tuple(q) in at_o]
        rows = [(i, j) for i, j in rows if ok(pc[i:i + 1])[0] and ok(po[j:j + 1])[0]]
        return np.array(rows)
    return c_img, o_img, (pc, rc), (po, ro), common, inner, (dx, dy), cap


def test_translation(native_gpu, crops):
    c_img, o_img, (pc, rc), (po, ro), common, inner, (dx, dy), cap = crops
    a = {(x, y, r) for (x, y), r in zip(pc[inner(pc)].tolist(), rc[inner(pc)].tolist())}
    b = {(x + dx, y + dy, r) for (x, y), r in zip(po.tolist(), ro.tolist()) if inner(np.array([[x + dx, y + dy]]))[0]}
    assert a == b and len(a) > 50
    same(native_gpu.corner_detect(c_img, cap, 5, 0, full=True), S.detect_full(c_img, cap, 5, 0))


def test_bgr_equals_its_grey(native_gpu):
    img = scene(70, 90, seed=2)
    g = S.grey(img).astype(np.uint8)
    for radius in (1, 5):
        cap = S.bound(70, 90, radius)
        a, b = native_gpu.corner_detect(img, cap, radius, 0, full=True), native_gpu.corner_detect(g, cap, radius, 0, full=True)
        same(a, b, "BGR against grey")
        same(b, S.detect_full(img, cap, radius, 0), "against the specification")
        assert a[2] > 10


@pytest.fixture(scope="module")
def ragged(native_gpu):
    """Five images of different shapes and channel counts, one without corners, and every image's own single call."""
    imgs = [scene(40, 50, seed=1), image((9, 130), 2), S.prototype_scene(100, 140, seed=3), edge(), image((33, 65, 3), 4)]
    return imgs, [native_gpu.corner_detect(im, 20, 5, 10) for im in imgs]


@pytest.mark.parametrize("order", [(0, 1, 2, 3, 4), (3, 2, 4, 0, 1)], ids=["in order", "permuted"])
def test_batch_equals_the_single_calls(native_gpu, ragged, order):
    imgs, singles = ragged
    out = native_gpu.corner_detect_batch([imgs[m] for m in order], 20, 5, 10)
    assert len(out) == len(order)
    for m, (pts, resp) in zip(order, out):
        assert pts.tobytes() == singles[m][0].tobytes() and resp.tobytes() == singles[m][1].tobytes() and pts.shape == singles[m][0].shape, m
    assert len(singles[3][0]) == 0 and len(singles[2][0]) == 20 and 0 < len(singles[1][0]) < 20
    want = S.detect(imgs[2], 20, 5, 10)                       # so that the chain ends in numpy
    assert singles[2][0].tobytes() == want[0].tobytes() and singles[2][1].tobytes() == want[1].tobytes()


def test_resident_and_features_forms_equal_the_host_buffer_forms(native_gpu, ragged):
    import torch
    from cvx_proj_amd import features, resident
    imgs, singles = ragged
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    with torch.cuda.stream(stream):
        d_imgs = [torch.from_numpy(im).to(dev) for im in imgs]
        need = resident.corner_workspace_bytes([im.shape for im in imgs], 5)
        assert need > 0 and need % 256 == 0 and resident.corner_workspace_bytes([(5, 5)], 5) == 0
        work = torch.empty(need, dtype=torch.uint8, device=dev)
        one = [resident.hip_corner_detect(im, 20, 5, 10, work=work) for im in d_imgs]
        many = resident.hip_corner_detect_batch(d_imgs, 20, 5, 10, work=work)
    stream.synchronize()
    pts, resp, count = (x.cpu().numpy() for x in many)
    assert pts.shape == (5, 20, 2) and resp.shape == (5, 20) and count.shape == (5,) and count.dtype == np.int32
    for m, (sp, sr) in enumerate(singles):
        n = len(sp)
        want = (np.zeros((20, 2), np.float32), np.zeros(20, np.int64), n)
        want[0][:n], want[1][:n] = sp, sr
        same((pts[m], resp[m], count[m]), want, f"batch, image {m}")
        same(tuple(x.cpu().numpy() for x in one[m]), want, f"single, image {m}")
    assert features.detect(imgs[0], 20).tobytes() == singles[0][0].tobytes()
    a, b = features.detect_pair(imgs[2], imgs[4], 20)
    assert a.tobytes() == singles[2][0].tobytes() and b.tobytes() == singles[4][0].tobytes()
    assert features.detect(imgs[3]).shape == (0, 2)
    with pytest.raises(native_gpu.ApapError):     # a short workspace is refused, not replaced
        native_gpu.check(native_gpu.lib().apap_corner_detect_device(None, d_imgs[0].data_ptr(), 40, 50, 3, 20, 5, 10, one[0][0].data_ptr(),
                                                                    one[0][1].data_ptr(), many[2].data_ptr(), work.data_ptr(), 256, None))
    with pytest.raises(ValueError):
        resident.hip_corner_detect(d_imgs[0].float(), 60)
    with pytest.raises(native_gpu.ApapError):
        resident.hip_corner_detect(d_imgs[0].cpu(), 60)


def test_detect_describe_match_chain(native_gpu, crops):
    """Every corner common to both crops and at least 16 px from all borders in both frames (beyond the descriptor's 12 px
    footprint and the detector's radius + 2) has the same descriptor in both: its nearest neighbour is at distance exactly 0,
    and it is the corner's translate wherever only one train descriptor is at distance 0."""
    import torch
    from cvx_proj_amd import features, resident
    c_img, o_img, (pc, rc), (po, ro), common, inner, (dx, dy), cap = crops
    rows = common(16)
    assert len(rows) > 40
    dev = torch.device("cuda", 0)
    out = resident.hip_detect_describe_match(torch.from_numpy(c_img).to(dev), torch.from_numpy(o_img).to(dev), cap, 5, 0)
    idx, dist, idx2, dist2, fc, fo, kc, ko = (x.cpu().numpy() for x in out)
    assert kc.tobytes() == pc.tobytes() and ko.tobytes() == po.tobytes() and fc.shape == (len(pc), 128) and fo.shape == (len(po), 128)
    assert np.all(dist[rows[:, 0]] == 0)
    zeros = (np.abs(fc[rows[:, 0], None, :] - fo[None, :, :]).max(axis=2) == 0).sum(axis=1)       # train descriptors at distance 0
    assert np.all(zeros >= 1) and (zeros == 1).sum() > 40
    single = zeros == 1
    assert np.array_equal(idx[rows[single, 0]], rows[single, 1])
    # the host-buffer chain gives the same matches
    k1, f1, k2, f2, matches = features.detect_and_match(c_img, o_img, cap, 5, 0.0)
    assert [k.pt for k in k1] == [tuple(q) for q in pc.tolist()] and f1.tobytes() == fc.tobytes() and f2.tobytes() == fo.tobytes()
    assert [m.trainIdx for m in matches] == idx.tolist() and [m.distance for m in matches] == dist.tolist()
    with pytest.raises(ValueError):
        resident.hip_detect_describe_match(torch.from_numpy(edge()).to(dev), torch.from_numpy(c_img).to(dev), 50)
    # defaults: from two uint8 images to matches with no other input
    assert len(features.detect_and_match(c_img, o_img)[4]) > 40


def test_end_to_end_homography(native_gpu, crops):
    """From the two images alone to the spectral EM loop's homography: the exact matches (distance 0 passes any ratio test)
    put every inlier on the translation, so least squares recovers it to rounding: the common corners map to their translates
    within 1e-3 px."""
    from cvx_proj_amd import features
    from cvx_proj_amd import spectral_method as SM
    c_img, o_img, (pc, rc), (po, ro), common, inner, (dx, dy), cap = crops
    arrays = features.matched_arrays_from_images(c_img, o_img, cap, 5, 0.0, ratio=0.5)
    src, dst = arrays[:2]
    assert len(src) > 40 and np.all(src - dst == [dx, dy], axis=1).mean() > 0.9
    em = SM.spectral_em(*arrays, F=np.zeros((3, 3)), epi_weight=0, lms=True)
    rows = common(16)
    p, q = pc[rows[:, 0]].astype(np.float64), po[rows[:, 1]].astype(np.float64)

    def worst(H, a, b):
        m = np.hstack([a, np.ones((len(a), 1))]) @ np.asarray(H, np.float64).T
        return float(np.abs(m[:, :2] / m[:, 2:] - b).max())
    errs = {"H_pred c->o": worst(em.rounds[-1].H_pred, p, q), "H_pred o->c": worst(em.rounds[-1].H_pred, q, p),
            "H_save c->o": worst(em.H_save, p, q), "H_save o->c": worst(em.H_save, q, p)}
    print("end to end:", len(src), "matches,", len(rows), "common corners, worst error in px:", errs)
    # the M-step inverts its solution (swap): H_pred maps the other image's corners to the centre's, H_save is its inverse
    assert errs["H_pred o->c"] <= 1e-3 and errs["H_save c->o"] <= 1e-3
