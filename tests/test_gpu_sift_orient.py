"""Keypoint orientation and oriented descriptors on the MI355X (apap_sift_orient, apap_sift_describe_oriented and their batch,
_device, resident and Python forms) against the numpy specification of tests/sift_orient_spec.py: the same bytes - angles
as float32 bits, descriptors as bytes - with the specification evaluated with the library's own constants."""
import ctypes as C

import numpy as np
import pytest

import sift_orient_cases as K
import sift_orient_spec as O

pytestmark = pytest.mark.gpu
GUARD, SENTINEL = 64, np.float32(-777.25)


@pytest.fixture(scope="module")
def native_gpu(native):
    if native.lib().apap_device_count() < 1:
        pytest.skip("no HIP device")
    return native


@pytest.fixture(scope="module")
def spec(native_gpu):
    """(orient, describe) of the float32 specification with the constants the kernel uses."""
    kw = dict(taps=native_gpu.sift_taps(), orient_window=native_gpu.sift_orient_window())
    return (lambda img, pts: O.orient(img, pts, **kw),
            lambda img, pts, angles=None: O.describe(img, pts, angles, descr_window=native_gpu.sift_descr_window(), **kw))


def same_bits(got, want, what=""):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype == np.float32 and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    bad = np.flatnonzero((got.view(np.int32) != want.view(np.int32)).reshape(len(got), -1).any(axis=1))
    assert got.tobytes() == want.tobytes(), (what, len(bad), "rows differ; first", int(bad[0]), got[bad[0]], want[bad[0]])


class DeviceForms:
    """The _device entry points called through ctypes on torch tensors: guard floats around every output, a dirty workspace."""

    def __init__(self, native):
        import torch
        self.torch, self.native, self.lib = torch, native, native.lib()
        self.dev = torch.device("cuda", 0)

    def guarded(self, n):
        return self.torch.full((n + 2 * GUARD,), float(SENTINEL), dtype=self.torch.float32, device=self.dev)

    def inner(self, buf, shape):
        a = buf.cpu().numpy()
        assert np.all(a[:GUARD] == SENTINEL) and np.all(a[-GUARD:] == SENTINEL), "an output's guard was written"
        return a[GUARD:-GUARD].reshape(shape).copy()

    def run(self, imgs, pts, offsets, mode, angles=None, rows=None):
        """mode: "orient", "given", "fused".  ``rows``: the length of the keypoint arrays (offsets may start above 0)."""
        t = self.torch
        rows = len(pts) if rows is None else rows
        d_imgs = [t.from_numpy(np.ascontiguousarray(im)).to(self.dev) for im in imgs]
        ptrs = (C.c_void_p * len(imgs))(*[d.data_ptr() for d in d_imgs])
        hs, ws = np.array([im.shape[0] for im in imgs], np.int32), np.array([im.shape[1] for im in imgs], np.int32)
        cs = np.array([1 if im.ndim == 2 else im.shape[2] for im in imgs], np.int32)
        off = np.asarray(offsets, np.int32)
        ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))      # noqa: E731
        d_pts = t.from_numpy(np.ascontiguousarray(pts, np.float32)).to(self.dev)
        need = self.lib.apap_sift_orient_workspace_bytes(len(imgs))
        work = t.randint(0, 256, (need,), dtype=t.uint8, device=self.dev)
        ang_buf, out_buf = self.guarded(rows), self.guarded(rows * 128)
        p_ang, p_out = ang_buf.data_ptr() + 4 * GUARD, out_buf.data_ptr() + 4 * GUARD
        common = (None, ptrs, ip(hs), ip(ws), ip(cs), len(imgs), d_pts.data_ptr(), ip(off))
        tail = (work.data_ptr(), need, None)
        if mode == "orient":
            rc = self.lib.apap_sift_orient_batch_device(*common, p_ang, *tail)
        elif mode == "fused":
            rc = self.lib.apap_sift_describe_oriented_batch_device(*common, None, p_ang, p_out, *tail)
        else:
            d_ang = t.from_numpy(np.ascontiguousarray(angles, np.float32)).to(self.dev)
            rc = self.lib.apap_sift_describe_oriented_batch_device(*common, d_ang.data_ptr(), None, p_out, *tail)
        self.native.check(rc)
        t.cuda.synchronize(self.dev)
        return self.inner(ang_buf, (rows,)), self.inner(out_buf, (rows, 128))


@pytest.fixture(scope="module")
def forms(native_gpu):
    return DeviceForms(native_gpu)


def every_form(native, forms, spec, img, pts, given, what):
    """Orientation only, given angles and fused through the host-buffer, _device and resident forms, against the specification."""
    import torch
    from cvx_proj_amd import resident
    want_a = spec[0](img, pts)
    want_given, want_fused = spec[1](img, pts, given), spec[1](img, pts, want_a)
    n = len(pts)
    # host buffers
    same_bits(native.sift_orient(img, pts), want_a, what + ": host orient")
    same_bits(native.sift_describe_oriented(img, pts, given), want_given, what + ": host given")
    f, a = native.sift_describe_oriented(img, pts)
    same_bits(a, want_a, what + ": host fused angles")
    same_bits(f, want_fused, what + ": host fused")
    # _device
    a, untouched = forms.run([img], pts, [0, n], "orient")
    same_bits(a, want_a, what + ": device orient")
    assert np.all(untouched == SENTINEL)
    untouched, f = forms.run([img], pts, [0, n], "given", given)
    same_bits(f, want_given, what + ": device given")
    assert np.all(untouched == SENTINEL)
    a, f = forms.run([img], pts, [0, n], "fused")
    same_bits(a, want_a, what + ": device fused angles")
    same_bits(f, want_fused, what + ": device fused")
    # resident
    dev = forms.dev
    d_img, d_pts = torch.from_numpy(img).to(dev), torch.from_numpy(pts).to(dev)
    ra = resident.hip_sift_orient(d_img, d_pts)
    rg = resident.hip_sift_describe_oriented(d_img, d_pts, torch.from_numpy(given).to(dev))
    rf, rfa = resident.hip_sift_describe_oriented(d_img, d_pts)
    rt = resident.hip_sift_describe_oriented(d_img, d_pts, ra)          # orient followed by given-angle: the fused bytes
    torch.cuda.synchronize(dev)
    same_bits(ra.cpu().numpy(), want_a, what + ": resident orient")
    same_bits(rg.cpu().numpy(), want_given, what + ": resident given")
    same_bits(rfa.cpu().numpy(), want_a, what + ": resident fused angles")
    same_bits(rf.cpu().numpy(), want_fused, what + ": resident fused")
    same_bits(rt.cpu().numpy(), want_fused, what + ": orient, then given")
    return want_a, want_fused


@pytest.mark.parametrize("name", sorted(K.cases()))
def test_edge_cases_equal_the_specification(native_gpu, forms, spec, name):
    img, pts, given = K.cases()[name]
    want_a, want_f = every_form(native_gpu, forms, spec, img, pts, given, name)
    assert np.all((want_a >= 0) & (want_a < 360))
    if "flat" in name:
        assert not want_a.any() and not want_f.any()


def test_bgr_every_pixel(native_gpu, forms, spec):
    img = K.seeded(48, 64, 3, 9)
    yy, xx = (a.ravel() for a in np.mgrid[:48, :64])
    pts = np.stack([xx, yy], -1).astype(np.float32)
    want_a, want_f = every_form(native_gpu, forms, spec, img, pts, K.given_angles(len(pts), 9), "64 x 48 BGR")
    assert len(np.unique(want_a)) > 1000 and np.count_nonzero(want_f.any(axis=1)) > 2500


def small_batch(n, seed):
    """n images from 13 x 13 to 40 x 50, grey and BGR in turn, mostly one keypoint each: the four waves of a block bisect the
    image table to different images."""
    shapes = [(13, 13), (40, 50), (13, 31), (23, 14), (16, 16), (13, 50), (40, 13), (19, 19), (33, 20)]
    rng = np.random.default_rng(seed)
    imgs, pts, lengths = [], [], []
    for m in range(n):
        h, w = shapes[m % len(shapes)]
        imgs.append(K.seeded(h, w, 3 if m % 2 else 1, 100 + m))
        k = 3 if m % 7 == 3 else 1
        pts.append(rng.uniform(-1, [w, h], (k, 2)).astype(np.float32))
        lengths.append(k)
    return imgs, pts, lengths


@pytest.mark.parametrize("n_images", [9, 65])
def test_batches_of_small_images(native_gpu, forms, spec, n_images):
    import torch
    from cvx_proj_amd import resident
    imgs, pts, lengths = small_batch(n_images, n_images)
    all_pts = np.concatenate(pts)
    given = K.given_angles(len(all_pts), n_images)
    at = np.cumsum([0] + lengths)
    want_a = np.concatenate([spec[0](im, p) for im, p in zip(imgs, pts)])
    want_g = np.concatenate([spec[1](im, p, given[at[m]:at[m + 1]]) for m, (im, p) in enumerate(zip(imgs, pts))])
    want_f = np.concatenate([spec[1](im, p) for im, p in zip(imgs, pts)])
    same_bits(native_gpu.sift_orient_batch(imgs, all_pts, lengths), want_a, "host orient")
    same_bits(native_gpu.sift_describe_oriented_batch(imgs, all_pts, lengths, given), want_g, "host given")
    f, a = native_gpu.sift_describe_oriented_batch(imgs, all_pts, lengths)
    same_bits(a, want_a, "host fused angles")
    same_bits(f, want_f, "host fused")
    a, _ = forms.run(imgs, all_pts, at, "orient")
    same_bits(a, want_a, "device orient")
    _, f = forms.run(imgs, all_pts, at, "given", given)
    same_bits(f, want_g, "device given")
    a, f = forms.run(imgs, all_pts, at, "fused")
    same_bits(a, want_a, "device fused angles")
    same_bits(f, want_f, "device fused")
    d_imgs = [torch.from_numpy(im).to(forms.dev) for im in imgs]
    d_pts = torch.from_numpy(all_pts).to(forms.dev)
    rf, ra = resident.hip_sift_describe_oriented_batch(d_imgs, d_pts, lengths)
    ro = resident.hip_sift_orient_batch(d_imgs, d_pts, lengths)
    rg = resident.hip_sift_describe_oriented_batch(d_imgs, d_pts, lengths, torch.from_numpy(given).to(forms.dev))
    torch.cuda.synchronize(forms.dev)
    same_bits(ra.cpu().numpy(), want_a, "resident fused angles")
    same_bits(ro.cpu().numpy(), want_a, "resident orient")
    same_bits(rf.cpu().numpy(), want_f, "resident fused")
    same_bits(rg.cpu().numpy(), want_g, "resident given")


def test_offsets_that_start_above_zero(native_gpu, forms, spec):
    """pt_offset = [2, 7, 137]: rows 0 and 1 of every array belong to nobody and keep their sentinel."""
    imgs = [K.seeded(13, 40, 3, 21), K.seeded(40, 50, 1, 22)]
    rng = np.random.default_rng(23)
    rows, off = 137, np.array([2, 7, 137], np.int32)
    pts = np.full((rows, 2), SENTINEL, np.float32)
    pts[2:7] = rng.uniform(-1, [40, 13], (5, 2))
    pts[7:] = rng.uniform(-1, [50, 40], (130, 2))
    given = np.full(rows, SENTINEL, np.float32)
    given[2:] = K.given_angles(135, 24)
    want_a = np.concatenate([spec[0](imgs[0], pts[2:7]), spec[0](imgs[1], pts[7:])])
    want_g = np.concatenate([spec[1](imgs[0], pts[2:7], given[2:7]), spec[1](imgs[1], pts[7:], given[7:])])
    want_f = np.concatenate([spec[1](imgs[0], pts[2:7]), spec[1](imgs[1], pts[7:])])
    for mode, ang in (("orient", None), ("given", given), ("fused", None)):
        a, f = forms.run(imgs, pts, off, mode, ang, rows=rows)
        if mode != "given":
            same_bits(a[2:], want_a, "device " + mode)
            assert np.all(a[:2] == SENTINEL)
        if mode != "orient":
            same_bits(f[2:], want_g if mode == "given" else want_f, "device " + mode)
            assert np.all(f[:2] == SENTINEL)
    # the host-buffer batch forms address their host arrays by the same offsets
    lib, f32 = native_gpu.lib(), C.POINTER(C.c_float)
    ptrs = (C.c_void_p * 2)(*[im.ctypes.data for im in imgs])
    hs, ws, cs = np.array([13, 40], np.int32), np.array([40, 50], np.int32), np.array([3, 1], np.int32)
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))      # noqa: E731
    angles, out = np.full(rows, SENTINEL, np.float32), np.full((rows, 128), SENTINEL, np.float32)
    common = (None, ptrs, ip(hs), ip(ws), ip(cs), 2, pts.ctypes.data_as(f32), ip(off))
    native_gpu.check(lib.apap_sift_orient_batch(*common, angles.ctypes.data_as(f32), -1))
    same_bits(angles[2:], want_a, "host orient")
    assert np.all(angles[:2] == SENTINEL)
    native_gpu.check(lib.apap_sift_describe_oriented_batch(*common, given.ctypes.data_as(f32), None, out.ctypes.data_as(f32), -1))
    same_bits(out[2:], want_g, "host given")
    assert np.all(out[:2] == SENTINEL)
    angles[:], out[:] = SENTINEL, SENTINEL
    native_gpu.check(lib.apap_sift_describe_oriented_batch(*common, None, angles.ctypes.data_as(f32), out.ctypes.data_as(f32), -1))
    same_bits(angles[2:], want_a, "host fused angles")
    same_bits(out[2:], want_f, "host fused")
    assert np.all(angles[:2] == SENTINEL) and np.all(out[:2] == SENTINEL)


def test_bad_keypoints_and_angles_among_valid_ones(native_gpu, forms, spec):
    """NaN and +-inf coordinates and angles beside valid keypoints of one block (_device forms): zero rows and angle 0, and the
    neighbours keep the specification's bytes."""
    img = K.seeded(40, 50, 3, 31)
    pts = np.float32([[20, 20], [np.nan, 20], [21, 19], [np.inf, 5], [22, 18], [5, -np.inf], [23, 17], [np.nan, np.nan],
                      [24, 16], [25, 15], [26, 14], [27, 13]])
    bad_pt = ~np.isfinite(pts).all(axis=1)
    a, f = forms.run([img], pts, [0, len(pts)], "fused")
    assert not a[bad_pt].any() and not f[bad_pt].any()
    same_bits(a[~bad_pt], spec[0](img, pts[~bad_pt]), "fused angles of the valid")
    same_bits(f[~bad_pt], spec[1](img, pts[~bad_pt]), "fused rows of the valid")
    same_bits(a, spec[0](img, pts), "the specification treats them alike")
    a, _ = forms.run([img], pts, [0, len(pts)], "orient")
    assert not a[bad_pt].any()
    same_bits(a, spec[0](img, pts), "orient")
    ok_pts = pts[~bad_pt]
    given = np.float32([10, np.nan, 200, np.inf, 359, -np.inf, -1, 360.0001][:len(ok_pts)])
    bad_angle = ~((given >= 0) & (given <= 360))
    assert bad_angle.sum() == 5
    _, f = forms.run([img], ok_pts, [0, len(ok_pts)], "given", given)
    assert not f[bad_angle].any() and f[~bad_angle].any(axis=1).all()
    same_bits(f[~bad_angle], spec[1](img, ok_pts[~bad_angle], given[~bad_angle]), "given rows of the valid")
    same_bits(f, spec[1](img, ok_pts, given), "the specification treats them alike")
    with pytest.raises(ValueError):                     # the host-buffer forms refuse both
        native_gpu.sift_describe_oriented(img, ok_pts, given)
    with pytest.raises(ValueError):
        native_gpu.sift_orient(img, pts)


def test_detect_and_match_on_the_quarter_turn(native_gpu, spec):
    """features.detect_and_match(..., oriented=True) equals the chain over the specifications: corners, fused descriptors,
    nearest neighbours; and the oriented descriptors find the turned picture's partners where the unoriented ones cannot."""
    import corner_spec
    import match_spec
    from cvx_proj_amd import features
    img, turned, _, _ = K.quarter_turn_pair()
    cap, radius = 400, 3
    k1, f1, k2, f2, matches = features.detect_and_match(img, turned, cap, radius, 0.001, oriented=True)
    pc, po = (corner_spec.detect(x, cap, radius, 1)[0].astype(np.float32) for x in (img, turned))
    assert [k.pt for k in k1] == [tuple(q) for q in pc.tolist()] and [k.pt for k in k2] == [tuple(q) for q in po.tolist()]
    same_bits(f1, spec[1](img, pc), "centre image")
    same_bits(f2, spec[1](turned, po), "turned image")
    idx, dist, _, _ = match_spec.match_int(f1, f2)
    assert [m.trainIdx for m in matches] == idx.tolist() and [m.distance for m in matches] == dist.tolist()
    # the same corners are found in both pictures (the detector is exact and symmetric): most matches are the true partners
    w = img.shape[1]
    partner = {(float(y), float(w - 1 - x)) for x, y in pc.tolist()}
    assert sum(tuple(q) in partner for q in po.tolist()) >= 0.9 * len(pc)
    good = sum(tuple(po[m.trainIdx]) == (pc[m.queryIdx][1], w - 1 - pc[m.queryIdx][0]) for m in matches)
    plain = features.detect_and_match(img, turned, cap, radius, 0.001)[4]
    good_plain = sum(tuple(po[m.trainIdx]) == (pc[m.queryIdx][1], w - 1 - pc[m.queryIdx][0]) for m in plain)
    print("true partners among", len(pc), "corners: oriented", good, "unoriented", good_plain)
    assert good > good_plain and good >= 0.8 * len(pc)
