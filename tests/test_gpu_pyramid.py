"""The image pyramid on the MI355X (apap_pyramid_build, apap_pyramid_keypoints and their batch, resident and Python forms)
against the numpy specification of tests/pyramid_spec.py: the same bytes; then the chain from two pictures of unlike scale to
matches against the composition of the specifications."""
import ctypes as C

import numpy as np
import pytest

import corner_spec
import match_spec
import pyramid_cases as cases_mod
import pyramid_spec as P
import sift_orient_spec
import sift_spec

pytestmark = pytest.mark.gpu

CASES = cases_mod.cases()
GUARD, SENTINEL = 256, 0xA5


@pytest.fixture(scope="module")
def native_gpu(native):
    if native.lib().apap_device_count() < 1:
        pytest.skip("no HIP device")
    return native


@pytest.fixture(scope="module")
def want():
    """The specification's levels of every case, computed once: (name, half_steps) -> list of levels at n_levels = 16."""
    return {(name, half): P.levels(img, 16, half) for name, img in CASES.items() for half in (False, True)}


@pytest.fixture(scope="module")
def describe(native_gpu):
    """(plain, oriented) float32 specifications of the descriptor with the constants the kernels use."""
    taps = native_gpu.sift_taps()
    window, ow, dw = native_gpu.sift_window(), native_gpu.sift_orient_window(), native_gpu.sift_descr_window()
    return (lambda img, pts: sift_spec.describe(img, np.asarray(pts, np.float32), taps, window),
            lambda img, pts: sift_orient_spec.describe(img, np.asarray(pts, np.float32), None, taps=taps, orient_window=ow, descr_window=dw))


def same_levels(got, wanted, what):
    assert len(got) == len(wanted), (what, "levels", len(got), len(wanted))
    for k, (g, w) in enumerate(zip(got, wanted)):
        g = np.asarray(g)
        assert g.dtype == np.uint8 and g.shape == w.shape, (what, k, g.shape, w.shape)
        bad = np.argwhere(g != w)
        assert g.tobytes() == w.tobytes(), (what, "level", k, len(bad), "pixels differ; first", bad[0].tolist(), int(g[tuple(bad[0])]), int(w[tuple(bad[0])]))


@pytest.mark.parametrize("name", sorted(CASES))
def test_host_buffer_levels_equal_the_specification(native_gpu, want, name):
    """Every level of the case, with and without half steps; n_levels 1, 2, 3 and 16 (which the layout clamps)."""
    img = CASES[name]
    for half in (False, True):
        full = want[name, half]
        for n_levels in (1, 2, 3, 16):
            same_levels(native_gpu.pyramid(img, n_levels, half), full[:n_levels], (name, half, n_levels))
    if name in ("white", "black"):
        assert all((a == (255 if name == "white" else 0)).all() for a in native_gpu.pyramid(img, 16))


class DeviceForm:
    """apap_pyramid_build_batch_device through ctypes on torch tensors: guard bytes around the level buffer, a sentinel in the
    gaps between levels, a workspace filled as asked."""

    def __init__(self, native):
        import torch
        self.torch, self.native, self.lib, self.dev = torch, native, native.lib(), torch.device("cuda", 0)

    def run(self, imgs, n_levels, half, work_fill):
        t = self.torch
        d_imgs = [t.from_numpy(np.ascontiguousarray(im)).to(self.dev) for im in imgs]
        ptrs = (C.c_void_p * len(imgs))(*[d.data_ptr() for d in d_imgs])
        hs, ws = np.array([im.shape[0] for im in imgs], np.int32), np.array([im.shape[1] for im in imgs], np.int32)
        cs = np.array([1 if im.ndim == 2 else im.shape[2] for im in imgs], np.int32)
        lays = [self.native.pyramid_layout(im.shape[0], im.shape[1], n_levels, half) for im in imgs]
        total = sum(int(lay[2][-1]) for lay in lays)
        buf = t.full((total + 2 * GUARD,), SENTINEL, dtype=t.uint8, device=self.dev)
        need = self.lib.apap_pyramid_workspace_bytes(len(imgs), n_levels)
        work = t.full((need,), work_fill, dtype=t.uint8, device=self.dev)
        ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))      # noqa: E731
        assert buf.data_ptr() % 256 == 0
        self.native.check(self.lib.apap_pyramid_build_batch_device(None, ptrs, ip(hs), ip(ws), ip(cs), len(imgs), n_levels, int(half),
                                                                   buf.data_ptr() + GUARD, total, work.data_ptr(), need, None))
        t.cuda.synchronize()
        raw = buf.cpu().numpy()
        written = np.zeros(len(raw), bool)
        out, at = [], GUARD
        for lh, lw, off, _, _ in lays:
            levels = []
            for k in range(len(lh)):
                a, n = at + int(off[k]), int(lh[k]) * int(lw[k])
                levels.append(raw[a:a + n].reshape(lh[k], lw[k]).copy())
                written[a:a + n] = True
            out.append(levels)
            at += int(off[-1])
        assert at == GUARD + total
        assert np.all(raw[~written] == SENTINEL), "a byte outside the levels (a guard, or a gap up to the 256-byte alignment) was written"
        return out


@pytest.mark.parametrize("name", ["side33", "side45", "side65", "past_tile_w", "past_tile_h", "framed", "bgr", "bgr_wide", "scene"])
def test_device_form_guards_and_dirty_workspace(native_gpu, want, name):
    form = DeviceForm(native_gpu)
    img = CASES[name]
    for half in (False, True):
        for n_levels in (2, 16):
            clean = form.run([img], n_levels, half, 0)[0]
            dirty = form.run([img], n_levels, half, 0xFF)[0]
            same_levels(clean, want[name, half][:n_levels], (name, half, n_levels, "device form"))
            same_levels(dirty, clean, (name, half, n_levels, "0xFF workspace"))


def test_batch_equals_every_pictures_own_call(native_gpu):
    """Six pictures of unlike shapes and channel counts, the first with level 0 alone: host-buffer batch, device batch with guards
    and resident batch against the specification, which is what each picture's own call gives."""
    import torch
    from cvx_proj_amd import features, resident
    batch = cases_mod.batch()
    form = DeviceForm(native_gpu)
    dev = torch.device("cuda", 0)
    d_imgs = [torch.from_numpy(np.ascontiguousarray(im)).to(dev) for im in batch]
    for half in (False, True):
        for n_levels in (3, 6):
            spec = [P.levels(im, n_levels, half) for im in batch]
            host = native_gpu.pyramid_batch(batch, n_levels, half)
            device = form.run(batch, n_levels, half, 0xFF)
            res = resident.hip_pyramid_batch(d_imgs, n_levels, half)
            for m in range(len(batch)):
                same_levels(host[m], spec[m], ("host batch", m, half, n_levels))
                same_levels(device[m], spec[m], ("device batch", m, half, n_levels))
                same_levels([a.cpu().numpy() for a in res[m]], spec[m], ("resident batch", m, half, n_levels))
                same_levels(native_gpu.pyramid(batch[m], n_levels, half), spec[m], ("single", m, half, n_levels))
    assert len(spec[0]) == 1 and len(spec[5]) == 6
    one = resident.hip_pyramid(d_imgs[1], 6, True, work=torch.empty(resident.pyramid_workspace_bytes(1, 6), dtype=torch.uint8, device=dev))
    same_levels([a.cpu().numpy() for a in one], spec[1], "resident single")
    assert all(a.data_ptr() % 256 == 0 for a in one)
    same_levels(features.pyramid(batch[4], levels=6), spec[4], "features.pyramid")
    with pytest.raises(native_gpu.ApapError):
        resident.hip_pyramid(d_imgs[1].cpu())
    with pytest.raises(ValueError):
        resident.hip_pyramid(d_imgs[1].float())


def test_the_pack_equals_the_specification(native_gpu):
    """The scene (the cap binds on its fine levels and not on its coarse ones) and the white picture (no corner on any level)
    in one pack: all four arrays and level_offset, host-buffer and resident forms."""
    import torch
    from cvx_proj_amd import resident
    max_corners, rows = 100, 128
    pics = [CASES["scene"], CASES["white"], CASES["side46"]]
    spts, sresp, counts, num, shift, index, wanted = [], [], [], [], [], [], []
    caps = P.level_caps(max_corners, 6)
    for pic in pics:
        lv = P.levels(pic, 6)
        lay = P.layout(lv[0].shape[0], lv[0].shape[1], 6)
        wanted.append(P.keypoints(pic, max_corners, lv=lv))
        for m, a in enumerate(lv):
            pts, resp, n = corner_spec.detect_full(a, rows, 5, 10)       # the detector's slab at more rows than the cap
            spts.append(pts)
            sresp.append(resp)
            counts.append(min(n, caps[m]))
            num.append(lay[3][m])
            shift.append(lay[4][m])
            index.append(m)
    found = [corner_spec.detect_full(a, rows, 5, 10)[2] for a in P.levels(pics[0], 6)]
    assert any(f > c for f, c in zip(found, caps)) and any(0 < f < c for f, c in zip(found, caps)) and counts[6:9] == [0, 0, 0] and len(counts) == 11
    spts, sresp = np.stack(spts), np.stack(sresp)
    w_pts, w_lpts, w_level, w_resp = (np.concatenate([w[k] for w in wanted]) for k in range(4))
    w_off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    dev = torch.device("cuda", 0)
    host = native_gpu.pyramid_keypoints(spts, sresp, counts, num, shift, index)
    res = resident.hip_pyramid_keypoints(torch.from_numpy(spts).to(dev), torch.from_numpy(sresp).to(dev), counts, num, shift, index)
    res = tuple(x.cpu().numpy() for x in res[:4]) + (res[4],)
    for what, got in (("host", host), ("resident", res)):
        for k, (g, w) in enumerate(zip(got, (w_pts, w_lpts, w_level, w_resp, w_off))):
            assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes(), (what, k)
    assert w_level.max() == 5 and (w_pts != w_lpts).any() and not np.array_equal(w_pts, np.rint(w_pts))     # 3/4 levels: thirds
    # a pack of empty levels alone: nothing to launch, the offsets all 0
    empty = native_gpu.pyramid_keypoints(spts[6:8], sresp[6:8], [0, 0], [1, 3], [0, 2], [0, 1])
    assert empty[0].shape == (0, 2) and empty[4].tolist() == [0, 0, 0]
    e2 = resident.hip_pyramid_keypoints(torch.from_numpy(spts[6:8]).to(dev), torch.from_numpy(sresp[6:8]).to(dev), [0, 0], [1, 3], [0, 2], [0, 1])
    assert e2[0].shape == (0, 2) and e2[4].tolist() == [0, 0, 0]


def spec_chain(pair, max_corners, levels, describe_fn, ratio, cross_check):
    """(pts_c, feats_c, pts_o, feats_o, kept query rows, their train rows, their distances) from the specifications alone."""
    (pc, fc, lc, rc), (po, fo, lo, ro) = (P.detect_and_describe(im, max_corners, n_levels=levels, describe=describe_fn) for im in pair)
    idx, dist, _, dist2 = match_spec.match_int(fc, fo)
    back = match_spec.match_int(fo, fc)[0]
    keep = match_spec.filters(idx, dist, dist2, back, ratio=ratio, cross_check=cross_check)
    return (pc, fc, lc, rc), (po, fo, lo, ro), keep, idx, dist


@pytest.fixture(scope="module")
def pairs():
    big, small = cases_mod.scaled_pair((2, 4))
    return {"scaled": (big, small, 300), "tiny": (CASES["side65"], CASES["side46"], 40)}


@pytest.mark.parametrize("oriented", [False, True], ids=["plain", "oriented"])
@pytest.mark.parametrize("which", ["scaled", "tiny"])
def test_the_chain_equals_the_composition_of_the_specifications(native_gpu, describe, pairs, which, oriented):
    """features.detect_and_match(levels=6) and resident.hip_pyramid_detect_describe_match on the 360 / 180 px pair and a tiny
    pair: keypoints, descriptors and match indices byte for byte."""
    import torch
    from cvx_proj_amd import features, resident
    c_img, o_img, max_corners = pairs[which]
    (pc, fc, lc, rc), (po, fo, lo, ro), keep, idx, dist = spec_chain((c_img, o_img), max_corners, 6, describe[int(oriented)], 0.8, True)
    assert len(pc) > 30 and len(po) > 16 and lc.max() >= 1

    k1, f1, k2, f2, matches = features.detect_and_match(c_img, o_img, max_corners, levels=6, oriented=oriented, ratio=0.8, cross_check=True)
    assert np.array([k.pt for k in k1], np.float32).tobytes() == pc.tobytes() and np.array([k.pt for k in k2], np.float32).tobytes() == po.tobytes()
    assert f1.tobytes() == fc.tobytes() and f2.tobytes() == fo.tobytes()
    assert [m.queryIdx for m in matches] == keep.tolist() and [m.trainIdx for m in matches] == idx[keep].tolist()
    assert [m.distance for m in matches] == dist[keep].tolist()
    if which == "scaled":
        assert len(matches) > 50

    got = features.detect_and_describe(c_img, max_corners, oriented=oriented)
    for g, w in zip(got, (pc, fc, lc, rc)):
        assert g.dtype == w.dtype and g.tobytes() == w.tobytes()
    assert features.detect(o_img, max_corners, levels=6).tobytes() == po.tobytes()
    a, b = features.detect_pair(c_img, o_img, max_corners, levels=6)
    assert a.tobytes() == pc.tobytes() and b.tobytes() == po.tobytes()

    dev = torch.device("cuda", 0)
    out = resident.hip_pyramid_detect_describe_match(torch.from_numpy(c_img).to(dev), torch.from_numpy(o_img).to(dev), max_corners, levels=6,
                                                     oriented=oriented)
    ridx, rdist, ridx2, rdist2, rfc, rfo, rpc, rpo = (x.cpu().numpy() for x in out)
    assert rpc.tobytes() == pc.tobytes() and rpo.tobytes() == po.tobytes() and rfc.tobytes() == fc.tobytes() and rfo.tobytes() == fo.tobytes()
    assert ridx.tolist() == idx.tolist() and rdist.tobytes() == dist.tobytes()
    arrays = features.matched_arrays_from_images(c_img, o_img, max_corners, levels=6, oriented=oriented, ratio=0.8, cross_check=True)
    assert arrays[0].tobytes() == pc[keep].tobytes() and arrays[1].tobytes() == po[idx[keep]].tobytes()


def test_level_0_and_levels_none_are_todays_outputs(native_gpu, describe, pairs):
    """Level 0's slice of the pyramid chain equals features.detect + features.compute; levels=None equals the single-scale
    composition of the specifications - the parent's outputs - and a BGR picture's level 0 equals its grey picture's."""
    from cvx_proj_amd import features
    c_img, o_img, max_corners = pairs["scaled"]
    pts, feats, level, resp = features.detect_and_describe(c_img, max_corners)
    n0 = int((level == 0).sum())
    base = features.detect(c_img, max_corners)
    assert n0 == len(base) > 100 and pts[:n0].tobytes() == base.tobytes()
    assert feats[:n0].tobytes() == features.compute(c_img, base)[1].tobytes()
    assert resp[:n0].tobytes() == corner_spec.detect(c_img, max_corners)[1].tobytes()

    pc, po = corner_spec.detect(c_img, max_corners)[0], corner_spec.detect(o_img, max_corners)[0]
    fc, fo = describe[0](c_img, pc), describe[0](o_img, po)
    idx, dist, _, dist2 = match_spec.match_int(fc, fo)
    keep = match_spec.filters(idx, dist, dist2, match_spec.match_int(fo, fc)[0], ratio=0.8, cross_check=True)
    for kw in ({}, {"levels": None}):
        k1, f1, k2, f2, matches = features.detect_and_match(c_img, o_img, max_corners, ratio=0.8, cross_check=True, **kw)
        assert np.array([k.pt for k in k1], np.float32).tobytes() == pc.tobytes() and f1.tobytes() == fc.tobytes() and f2.tobytes() == fo.tobytes()
        assert [m.queryIdx for m in matches] == keep.tolist() and [m.trainIdx for m in matches] == idx[keep].tolist()
    single = features.detect_and_describe(c_img, max_corners, levels=None)
    assert single[0].tobytes() == pc.tobytes() and single[1].tobytes() == fc.tobytes() and not single[2].any()

    bgr = CASES["bgr"]
    got = features.detect_and_describe(bgr, 60, levels=3)
    n0 = int((got[2] == 0).sum())
    want_pts = features.detect(bgr, 60)
    assert n0 == len(want_pts) > 0 and got[0][:n0].tobytes() == want_pts.tobytes()
    assert got[1][:n0].tobytes() == features.compute(bgr, want_pts)[1].tobytes()
