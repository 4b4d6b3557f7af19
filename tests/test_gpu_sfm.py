"""The co-visibility and triangulation kernels (csrc/apap_sfm.hip) on the MI355X against tests/sfm_spec.py, bit for bit: the
tracks (table, track_pts, point_track, T) on every case of tests/sfm_cases.py and on seeded inputs at the scan's tile and
block edges, with eight views, with every point identical, with a chain longer than a block, with chains that give a thread of
the resolver several links and make its walk go on behind a joiner, and on 12 000 observations; the positions (X, lam_min,
n_rays) at the launch's block edges, for every ray count 2 .. 9, where the clamp fires, below min_views and with a NaN
pixel; and the contracts - guard bytes around every output, a workspace whose prior contents do not matter, rows behind T
untouched, resident forms that give the host forms' bytes."""
import numpy as np
import pytest

import sfm_cases as C
import sfm_spec as S

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
GUARD = 256
FILL = 0xFF


@pytest.fixture(scope="module")
def native_gpu(native):
    if native.lib().apap_device_count() < 1:
        pytest.skip("no HIP device")
    return native


def device():
    import torch
    return torch.device("cuda:0")


class Guarded:
    """``nbytes`` of device memory between two guards of sentinel bytes, pre-filled with ``fill``."""

    def __init__(self, nbytes, fill=FILL):
        import torch
        self.n = nbytes
        self.buf = torch.full((nbytes + 2 * GUARD,), SENTINEL, dtype=torch.uint8, device=device())
        self.buf[GUARD:GUARD + nbytes] = fill
        assert self.buf.data_ptr() % 256 == 0
        self.ptr = self.buf.data_ptr() + GUARD

    def read(self, dtype):
        got = self.buf.cpu().numpy()
        assert (got[:GUARD] == SENTINEL).all() and (got[GUARD + self.n:] == SENTINEL).all(), "bytes outside a buffer were written"
        return got[GUARD:GUARD + self.n].copy().view(dtype)


def same(a, b):
    """Equal byte for byte (the sign of a zero and the bits of a NaN included)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def tracks_on_device(native, views, eps=S.EPS):
    """apap_covis_tracks_device on guarded outputs and a 0xFF workspace; checks that nothing behind T was written."""
    import torch
    pts, idx, off = S.flatten(views)
    N, V = len(pts), len(views)
    rows = max(N, 1)
    d_pts = torch.from_numpy(pts if N else np.zeros((1, 2), np.float32)).to(device())
    d_idx = torch.from_numpy(idx if N else np.zeros(1, np.int32)).to(device())
    table, tpts, ptrack, count = Guarded(rows * V * 4), Guarded(rows * 8), Guarded(rows * 4), Guarded(4)
    status = Guarded(4, fill=0)
    need = native.lib().apap_covis_workspace_bytes(N, V)
    assert need == native.covis_workspace_layout(N, V)["total"]
    work = Guarded(need)
    native.check(native.lib().apap_covis_tracks_device(None, d_pts.data_ptr(), d_idx.data_ptr(), native._ip(off), V,
                                                       native.C.c_float(float(eps)), table.ptr, tpts.ptr, ptrack.ptr, count.ptr,
                                                       status.ptr, work.ptr, need, None))
    torch.cuda.synchronize()
    work.read(np.uint8)
    assert status.read(np.int32)[0] == 0
    T = int(count.read(np.int32)[0])
    assert 0 <= T <= N
    tb, tp = table.read(np.int32).reshape(rows, V), tpts.read(np.float32).reshape(rows, 2)
    assert (tb[T:].view(np.uint8) == FILL).all() and (tp[T:].view(np.uint8) == FILL).all(), "rows behind T were written"
    return tb[:T], tp[:T], ptrack.read(np.int32)[:N]


def check_tracks(native, views, eps=S.EPS):
    want = S.covis_tracks(views, eps)
    got = native.covis_tracks(views, eps)
    for g, w in zip(got, want):
        assert same(g, w)
    for g, w in zip(tracks_on_device(native, views, eps), want):
        assert same(g, w)
    return want


@pytest.mark.parametrize("name", list(C.track_cases()))
def test_tracks_on_the_cases(native_gpu, name):
    check_tracks(native_gpu, C.track_cases()[name])


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2049])
def test_tracks_at_the_scan_edges(native_gpu, n):
    """Observation counts around the wave, the 256-query block and tile, the 512-entry chunk and the resolver's 1024 threads."""
    table, _, _ = check_tracks(native_gpu, C.random_views(n, 4, seed=100 + n))
    assert n < 64 or 0 < ((table >= 0).sum(1) > 1).sum() < len(table)


def test_tracks_with_eight_views_and_other_eps(native_gpu):
    views = C.random_views(700, 8, seed=8)
    check_tracks(native_gpu, views)
    check_tracks(native_gpu, views, eps=np.float32(0.0))           # nothing matches: every observation a track
    check_tracks(native_gpu, views, eps=np.float32(1e30))          # everything matches the first point


@pytest.mark.parametrize("empty_view0", [False, True])
def test_tracks_of_identical_points(native_gpu, empty_view0):
    views = [(np.full((n, 2), 12.5, np.float32), np.arange(n, dtype=np.int32) + 1000 * v)
             for v, n in enumerate([0 if empty_view0 else 90, 110, 100])]
    table, _, point_track = check_tracks(native_gpu, views)
    assert len(table) == (1 if empty_view0 else 90) and (point_track[views[0][0].shape[0]:] == 0).all()


def test_no_observations_at_all(native_gpu):
    empty = (np.zeros((0, 2), np.float32), np.zeros(0, np.int32))
    table, track_pts, point_track = check_tracks(native_gpu, [empty, empty, empty])
    assert table.shape == (0, 3) and track_pts.shape == (0, 2) and point_track.shape == (0,)


def test_tracks_of_a_chain_longer_than_a_block(native_gpu):
    views = C.chain_views(300)
    table, _, _ = check_tracks(native_gpu, views)
    assert len(table) == 1 + 150          # every second point of the chain opens a track


def test_tracks_of_a_chain_with_three_links_per_resolver_thread(native_gpu):
    table, _, _ = check_tracks(native_gpu, C.chain_views(C.LONG_CHAIN))
    assert len(table) == 1101


@pytest.mark.parametrize("spaced", [False, True])
def test_tracks_of_interlocked_chains(native_gpu, spaced):
    """Chains longer than the resolver's workgroup in two views, the second's points between the first's: every second walk
    passes an observation that joined another track and goes on behind it (tests/test_sfm_inputs.py asserts that).  With
    ``spaced`` the position behind the joiner holds a far-away founder, not the next in-box observation."""
    table, _, _ = check_tracks(native_gpu, C.interlocked_views(spaced=spaced))
    assert len(table) == (3151 if spaced else 2051)


def test_tracks_of_twelve_thousand_observations(native_gpu):
    table, _, _ = check_tracks(native_gpu, C.random_views(**C.LARGE_RANDOM))
    assert len(table) == 4806 and int(((table >= 0).sum(1) > 1).sum()) == 3445


# ------------------------------------------------------------------ triangulation
def check_rays(native, origins, dirs, off):
    want = S.triangulate_rays(origins, dirs, off)
    got = native.triangulate_rays(origins, dirs, off)
    for g, w in zip(got, want):
        assert same(g, w)
    return want


@pytest.mark.parametrize("tracks", [1, 63, 64, 65, 257])
def test_rays_at_the_block_edges(native_gpu, tracks):
    X, lam, n = check_rays(native_gpu, *C.ray_case(tracks, seed=40 + tracks))
    assert np.isfinite(X).all() and (n >= 2).all() and (tracks < 63 or ((lam < 1e-3).any() and (lam > 1e-3).any()))


def test_rays_of_the_golden_case_and_degenerate_tracks(native_gpu):
    origins, dirs, off = C.ray_case(**C.RAY_CASE)
    check_rays(native_gpu, origins, dirs, off)
    # a track without rays, one ray, two parallel rays (two eigenvalues clamped), a NaN direction, a zero direction
    o = np.array([[1.0, 2.0, 3.0], [0.0, 0.0, 60.0], [5.0, 0.0, 60.0], [0.0, 0.0, 1.0], [1.0, 1.0, 1.0], [2.0, 2.0, 2.0]])
    d = np.array([[0.0, 0.6, 0.8], [0.0, 0.0, -1.0], [0.0, 0.0, -1.0], [np.nan, 0.0, 1.0], [0.0, 1.0, 0.0], [0.0, 0.0, 0.0]])
    X, lam, n = check_rays(native_gpu, o, d, np.array([0, 0, 1, 3, 5, 6], np.int32))
    assert n.tolist() == [0, 1, 2, 2, 1] and np.isnan(X[0]).all() and np.isnan(X[3]).all() and np.isfinite(X[[1, 2, 4]]).all()
    assert same(X[0], np.full(3, np.nan)) and same(lam[[0, 3]], np.full(2, np.nan))


def dst_lists(cam):
    off = cam["dst_offset"]
    return [cam["dst_pts"][off[v]:off[v + 1]] for v in range(len(off) - 1)]


def check_tracks_triangulation(native, cam, min_views):
    args = (cam["table"], cam["track_pts"], cam["dst_pts"], cam["dst_offset"], cam["Kinv"], cam["R"], cam["origins"], cam["center_cam"],
            cam["view_cam"], min_views)
    want = S.triangulate_tracks(*args)
    got = native.triangulate_tracks(cam["table"], cam["track_pts"], dst_lists(cam), cam["Kinv"], cam["R"], cam["origins"],
                                    cam["center_cam"], cam["view_cam"], min_views=min_views)
    for g, w in zip(got, want):
        assert same(g, w)
    # the same rays, handed over as rays
    for g, w in zip(native.triangulate_rays(*S.track_rays(*args)), want):
        assert same(g, w)
    return want


def test_triangulate_tracks_of_every_ray_count(native_gpu):
    cam = C.camera_case(8, 257, seed=31)
    cam["track_pts"][7, 0] = np.nan                 # a NaN pixel in the centre picture
    cam["dst_pts"][cam["dst_offset"][2] + 5] = np.nan   # and in a view
    cam["table"][9, 0] = 37                         # an index behind the view's points: not seen there
    cam["table"][10, 1] = -5
    cam["table"][7, 0] = 1
    cam["table"][11] = [3, -1, -1, -1, -1, -1, -1, -1]      # two rays
    cam["table"][12] = np.arange(8)                         # nine
    X, lam, n = check_tracks_triangulation(native_gpu, cam, min_views=1)
    assert set(range(2, 10)) <= set(n.tolist()) and np.isnan(X[7]).all() and n[7] > 0
    X, lam, n = check_tracks_triangulation(native_gpu, cam, min_views=2)
    below = ((cam["table"] >= 0) & (cam["table"] < 37)).sum(1) < 2
    assert below.any() and (n[below] == 0).all() and (n[~below] >= 3).all()
    assert same(X[below], np.full((int(below.sum()), 3), np.nan)) and same(lam[below], np.full(int(below.sum()), np.nan))
    check_tracks_triangulation(native_gpu, cam, min_views=9)            # nothing is seen that often


@pytest.mark.parametrize("tracks", [1, 63, 64, 65])
def test_triangulate_tracks_where_the_clamp_fires(native_gpu, tracks):
    cam = C.camera_case(4, tracks, seed=50 + tracks, nearly_coincident=True)
    X, lam, n = check_tracks_triangulation(native_gpu, cam, min_views=1)
    assert (lam < 1e-3).all() and np.isfinite(X).all()


def test_triangulation_device_forms_write_only_their_rows(native_gpu):
    """Guard bytes around X, lam_min and n_rays; with a track count on the device below the rows given, the rest is untouched."""
    import torch
    lib = native_gpu.lib()
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device())      # noqa: E731
    cam = C.camera_case(4, 65, seed=95)
    rows, live = 65, 40
    want = S.triangulate_tracks(cam["table"][:live], cam["track_pts"][:live], cam["dst_pts"], cam["dst_offset"], cam["Kinv"], cam["R"],
                                cam["origins"], cam["center_cam"], cam["view_cam"], 2)
    X, lam, n = Guarded(rows * 24), Guarded(rows * 8), Guarded(rows * 4)
    d = [to(cam[k]) for k in ("table", "track_pts", "dst_pts", "Kinv", "R", "origins")]
    count = to(np.array([live], np.int32))
    native_gpu.check(lib.apap_triangulate_tracks_device(None, d[0].data_ptr(), d[1].data_ptr(), count.data_ptr(), rows, 4, d[2].data_ptr(),
                                                        native_gpu._ip(cam["dst_offset"]), d[3].data_ptr(), d[4].data_ptr(), d[5].data_ptr(), 5,
                                                        cam["center_cam"], native_gpu._ip(np.array(cam["view_cam"], np.int32)), 2, X.ptr,
                                                        lam.ptr, n.ptr, None))
    torch.cuda.synchronize()
    got = X.read(np.float64).reshape(rows, 3), lam.read(np.float64), n.read(np.int32)
    for g, w in zip(got, want):
        assert same(g[:live], w) and (g[live:].view(np.uint8) == FILL).all()
    o, dr, off = C.ray_case(65, seed=96)
    bad = off.copy()
    bad[10], bad[21] = off[11] + 1, 10 ** 6            # a reversed range (tracks 9 and 10) and one that leaves the rays (20, 21)
    X, lam, n = Guarded(65 * 24), Guarded(65 * 8), Guarded(65 * 4)
    d_o, d_d, d_off = to(o), to(dr), to(bad)
    native_gpu.check(lib.apap_triangulate_rays_device(None, d_o.data_ptr(), d_d.data_ptr(), d_off.data_ptr(), len(o), 65, X.ptr, lam.ptr,
                                                      n.ptr, None))
    torch.cuda.synchronize()
    wX, wlam, wn = S.triangulate_rays(o, dr, off)
    gX, glam, gn = X.read(np.float64).reshape(65, 3), lam.read(np.float64), n.read(np.int32)
    odd = [10, 20, 21]                                 # empty on the device; 9 runs on to the moved offset and differs too
    keep = np.setdiff1d(np.arange(65), odd + [9])
    assert same(gX[keep], wX[keep]) and same(glam[keep], wlam[keep]) and same(gn[keep], wn[keep])
    assert (gn[odd] == 0).all() and np.isnan(gX[odd]).all() and gn[9] == wn[9] + wn[10] + 1


def test_resident_forms_give_the_host_forms_bytes(native_gpu):
    """hip_covis_tracks feeds hip_triangulate_tracks on the stream, with no host synchronisation between them."""
    import torch
    from cvx_proj_amd import resident
    views = C.random_views(900, 4, seed=77)
    pts, idx, off = S.flatten(views)
    cam = C.camera_case(4, 1, seed=78)
    dst_lengths = [6000] * 4                        # the tracks' indices are below 5000
    dst = (C.uniform(2 * 24000, 79, 0) * 768.0).astype(np.float32).reshape(-1, 2)
    dev = device()
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)      # noqa: E731
    work = torch.full((resident.covis_workspace_bytes(len(pts), 4),), 0xFF, dtype=torch.uint8, device=dev)
    table, tpts, ptrack, count = resident.hip_covis_tracks(to(pts), to(idx), [len(p) for p, _ in views], work=work)
    X, lam, n = resident.hip_triangulate_tracks(table, tpts, count, to(dst), dst_lengths, to(cam["Kinv"]), to(cam["R"]), to(cam["origins"]),
                                                cam["center_cam"], cam["view_cam"])
    T = int(count.cpu()[0])
    h_table, h_tpts, h_ptrack = native_gpu.covis_tracks(views)
    assert T == len(h_table) and same(table[:T].cpu().numpy(), h_table) and same(tpts[:T].cpu().numpy(), h_tpts)
    assert same(ptrack.cpu().numpy(), h_ptrack)
    hX, hlam, hn = native_gpu.triangulate_tracks(h_table, h_tpts, [dst[6000 * v:6000 * (v + 1)] for v in range(4)], cam["Kinv"], cam["R"],
                                                 cam["origins"], cam["center_cam"], cam["view_cam"])
    assert (hn >= 3).any() and (hn == 0).any()
    assert same(X[:T].cpu().numpy(), hX) and same(lam[:T].cpu().numpy(), hlam) and same(n[:T].cpu().numpy(), hn)
    o, d, roff = C.ray_case(130, seed=80)
    rX, rlam, rn = resident.hip_triangulate_rays(to(o), to(d), to(roff))
    for g, w in zip((rX, rlam, rn), native_gpu.triangulate_rays(o, d, roff)):
        assert same(g.cpu().numpy(), w)


def test_drop_in_module(native_gpu, golden):
    """cvx_proj_amd.sfm_test with the reference's lists in and out, against what the reference itself returned."""
    from cvx_proj_amd import sfm_test
    from cvx_proj_amd.matching import DMatch
    ref = golden("sfm_ref")
    views = C.track_cases()["chain_4x120"]
    src = [[p.reshape(1, 2).copy() for p in pts] for pts, _ in views]
    matches = [[DMatch(0, int(t), 0.0) for t in idx] for _, idx in views]
    res, covid = sfm_test.get_covid(src, matches)
    assert np.array_equal(np.array(covid), ref["tracks_chain_4x120_table"]) and all(len(r) == 4 and type(r[0]) is int for r in covid)
    assert res[0].shape == (1, 2) and same(np.array(res, np.float32).reshape(-1, 2), ref["tracks_chain_4x120_pts"])
    o, d, off = C.ray_case(**C.RAY_CASE)
    for k in (0, 1, 2, 3):
        a, b = off[k], off[k + 1]
        got = sfm_test.solve_3d_position(o[a:b, :, None], d[a:b, :, None])
        assert got.shape == (3, 1) and same(got.ravel(), S.solve_rays(o[a:b], d[a:b])[0])
    cam = C.camera_case(4, 40, seed=90)
    poses = dict(Rs=cam["R"], ts=cam["origins"], K=cam["K"])
    X = sfm_test.covid_3d_optimize(cam["table"].tolist(), list(cam["track_pts"]), dst_lists(cam), **poses)
    want, _, n = S.triangulate_tracks(cam["table"], cam["track_pts"], cam["dst_pts"], cam["dst_offset"], np.linalg.inv(cam["K"]), cam["R"],
                                      cam["origins"], 2, [0, 1, 3, 4], 2)
    assert X.shape == (40, 3) and same(X, want) and (n == 0).any() and (n >= 3).any()
