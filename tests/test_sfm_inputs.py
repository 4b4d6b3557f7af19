"""The inputs of the co-visibility and triangulation tests reach the edges they are meant for; asserted from the
specification (tests/sfm_spec.py) and from what the reference recorded (tests/golden/sfm_ref.npz), without a GPU."""
import numpy as np
import pytest

import sfm_cases as C
import sfm_spec as S

CASES = C.track_cases()


def tracks(name):
    return S.covis_tracks(CASES[name])


def test_the_prototype_cases_have_their_sizes():
    for name, per_view in (("jitter_4x40", 40), ("chain_4x120", 120), ("repeats_4x200", 200)):
        assert [len(p) for p, _ in CASES[name]] == [per_view] * 4
        table, _, _ = tracks(name)
        assert 0 < ((table >= 0).sum(1) > 1).sum() < len(table)       # tracks seen in several views, and tracks seen in one


def test_the_chain_needs_at_least_50_rounds():
    assert S.covis_tracks_fixed_point(CASES["chain_4x120"])[3] >= 50
    assert S.covis_tracks_fixed_point(C.chain_views(300))[3] >= 256     # the GPU test's: longer than a wave and a 256-block
    assert S.covis_tracks_fixed_point(CASES["jitter_4x40"])[3] in (2, 3)


def test_the_chain_makes_the_walk_pass_a_decided_observation_that_opened_nothing():
    """What the resolver's on-demand continuation is for: an in-box earlier observation that joined another track."""
    views = C.chain_views(300)
    pts, _, off = S.flatten(views)
    _, _, point_track = S.covis_tracks(views)
    g = off[1] + 2                                                      # the chain's third point
    assert S.in_box(pts[g - 1], pts[g], S.EPS) and not S.in_box(pts[g - 2], pts[g], S.EPS)
    assert point_track[g - 1] == point_track[g - 2] and point_track[g] != point_track[g - 1]


def first_in_box_before(pts, g):
    """The first position e < g inside g's box, or -1: what the scan hands to the resolver."""
    with np.errstate(invalid="ignore"):
        hit = (np.abs(pts[:g, 0] - pts[g, 0]) < S.EPS) & (np.abs(pts[:g, 1] - pts[g, 1]) < S.EPS)
    return int(hit.argmax()) if hit.any() else -1


def founders(point_track):
    """founder[g]: g opened its track (it is the first observation of it)."""
    out = np.zeros(len(point_track), bool)
    out[np.unique(point_track, return_index=True)[1]] = True
    return out


def test_the_resolver_is_one_workgroup_of_1024_threads():
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "cvx_proj_amd", "csrc", "apap_sfm.hip")).read()
    assert int(re.search(r"constexpr int kResolveThreads = (\d+);", text).group(1)) == C.RESOLVE_THREADS
    assert "for (int g = n0 + t; g < N; g += kResolveThreads)" in text        # the ownership the cases below are built on


def test_the_long_chain_gives_a_resolver_thread_three_links():
    views = C.chain_views(C.LONG_CHAIN)
    pts, _, off = S.flatten(views)
    table, _, point_track = S.covis_tracks(views)
    n0 = int(off[1])
    assert len(table) == 1101 and C.LONG_CHAIN > 2 * C.RESOLVE_THREADS
    chain = np.arange(n0, len(pts))
    assert np.bincount((chain - n0) % C.RESOLVE_THREADS).max() == 3
    # one chain: every point but the first has its predecessor, and nothing else, as its first earlier in-box observation
    assert all(first_in_box_before(pts, g) == g - 1 for g in chain[1:]) and first_in_box_before(pts, n0) == -1
    assert np.array_equal(founders(point_track)[n0:], np.arange(C.LONG_CHAIN) % 2 == 0)       # decided one after the other


@pytest.mark.parametrize("spaced", [False, True])
def test_the_interlocked_chains_make_the_walk_go_on_behind_a_joiner(spaced):
    """Without ``spaced`` the next in-box observation behind a joiner is, but for the last point, the next position; with it,
    the next position is never in the box and has founded a track: a walk that stepped there would join it."""
    views = C.interlocked_views(spaced=spaced)
    pts, _, off = S.flatten(views)
    table, _, point_track = S.covis_tracks(views)
    n0, n1 = int(off[1]), int(off[2])
    length, step = len(pts) - n1, 2 if spaced else 1
    # view 0, every second point of view 1's chain, the last point of view 2; with ``spaced`` the points between as well
    assert len(table) == 1500 + 550 + 1 + (length if spaced else 0) and n0 == 1500 and n0 % 64 != 0 and n0 % C.RESOLVE_THREADS != 0
    assert length == 1100 > C.RESOLVE_THREADS and n1 - n0 == step * length         # both chains are longer than the workgroup
    found = founders(point_track)
    assert np.array_equal(found[n0:n1:step], np.arange(length) % 2 == 0) and (point_track[n0:] >= n0).all()
    assert not spaced or found[n0 + 1:n1:2].all()
    rescans, to_the_end, neighbours = 0, 0, 0
    for g in range(n1, len(pts)):
        c = first_in_box_before(pts, g)
        assert c >= n0                                          # an observation, not a point of view 0: the resolver's to decide
        if not found[c]:                                        # c joined another track: the walk goes on behind it
            rescans += 1
            nxt = c + 1 + np.flatnonzero((np.abs(pts[c + 1:g, 0] - pts[g, 0]) < S.EPS) & (np.abs(pts[c + 1:g, 1] - pts[g, 1]) < S.EPS))
            assert len(nxt) and (point_track[g] == point_track[nxt[0]] or not found[nxt[0]])
            to_the_end += not any(found[e] for e in nxt)
            neighbours += nxt[0] == c + 1
            assert not spaced or (found[c + 1] and not S.in_box(pts[c + 1], pts[g], S.EPS))
    assert rescans == length // 2 and to_the_end == 1 and found[-1]                # the last point walks past all and opens a track
    assert neighbours == (0 if spaced else rescans - 1)
    # every point of the second chain has the first chain's points k and k + 1 in its box: a dependency across the views
    k = 501
    assert first_in_box_before(pts, n1 + k) == n0 + step * k and S.in_box(pts[n0 + step * (k + 1)], pts[n1 + k], S.EPS)
    assert S.in_box(pts[n1 + k - 1], pts[n1 + k], S.EPS)


def test_the_large_random_case():
    views = C.random_views(**C.LARGE_RANDOM)
    pts, _, off = S.flatten(views)
    table, _, point_track = S.covis_tracks(views)
    n0 = int(off[1])
    assert len(pts) == 12000 and len(views) == 8 and all(len(p) for p, _ in views)
    assert len(table) == 4806 and int(((table >= 0).sum(1) > 1).sum()) == 3445
    # the scan's grid: blocks of 256 queries by chunks of 512 entries; the resolver's threads own eleven observations and more
    assert (len(pts) - n0 + 255) // 256 >= 40 and (len(pts) + 511) // 512 == 24 and (len(pts) - n0) // C.RESOLVE_THREADS >= 10
    found = founders(point_track)
    sample = range(n0, len(pts), 7)
    firsts = [first_in_box_before(pts, g) for g in sample]
    assert sum(1 for c in firsts if c >= n0 and not found[c]) > 20       # the walk goes on behind a joiner here too


def test_the_box_is_strict_and_needs_both_axes():
    (p0, _), (p1, _) = CASES["exactly_eps_apart"]
    assert np.float32(p1[0, 0] - p0[0, 0]) == np.float32(0.1) and len(tracks("exactly_eps_apart")[0]) == 2
    (p0, _), (p1, _) = CASES["just_below_eps"]
    assert np.float32(p1[0, 0] - p0[0, 0]) == np.nextafter(np.float32(0.1), np.float32(0)) and len(tracks("just_below_eps")[0]) == 1
    assert len(tracks("inside_in_x_only")[0]) == 2


def test_identical_points_in_view0_both_open_and_the_first_collects():
    table, pts, point_track = tracks("identical_in_view0")
    assert table.tolist() == [[10, 20, 30], [11, -1, -1]] and point_track.tolist() == [0, 1, 0, 0]
    assert pts.tolist() == [[7.0, 7.0], [7.0, 7.0]]


def test_the_last_observation_of_a_view_wins():
    table, _, point_track = tracks("last_of_a_view_wins")
    assert point_track.tolist() == [0, 0, 1, 0] and table.tolist() == [[10, 22], [-1, 21]]


def test_empty_views_and_a_single_view():
    table, _, _ = tracks("empty_view_in_the_middle")
    assert (table[:, 1] == -1).all() and table.tolist() == [[10, -1, 30, -1], [11, -1, -1, 41], [-1, -1, 31, 40]]
    table, _, point_track = tracks("empty_view0")
    assert (table[:, 0] == -1).all() and table.tolist() == [[-1, 21, 31], [-1, 22, 30]] and point_track.tolist() == [0, 0, 1, 1, 0]
    table, _, point_track = tracks("single_view")
    assert table.tolist() == [[10], [11], [12]] and point_track.tolist() == [0, 1, 2]


def test_nan_points_match_nothing():
    table, pts, point_track = tracks("nan_point")
    assert point_track.tolist() == [0, 1, 0, 2] and table.tolist() == [[10, 21], [-1, 20], [-1, 22]] and np.isnan(pts[1:, 0]).all()


def test_the_ray_case_clamps_a_quarter_and_leaves_the_threshold_band_empty(golden):
    smin = golden("sfm_ref")["tri_smin"]
    origins, dirs, off = C.ray_case(**C.RAY_CASE)
    assert len(smin) == len(off) - 1 == 240 and sorted(set(np.diff(off).tolist())) == [2, 3, 4, 5]
    assert not ((smin > 5e-4) & (smin < 2e-3)).any()
    assert (smin < 1e-3).sum() == 60 and (smin[::4] < 1e-3).all()
    _, lam, _ = S.triangulate_rays(origins, dirs, off)
    assert ((lam < 1e-3) == (smin < 1e-3)).all()                        # the specification clamps exactly those
    sweeps = []
    for k in range(len(off) - 1):
        info = {}
        S.solve_rays(origins[off[k]:off[k + 1]], dirs[off[k]:off[k + 1]], info)
        sweeps.append(info["sweeps"])
    assert max(sweeps) <= 5 < S.MAX_SWEEPS                              # the cap is never what ends the iteration


def test_the_camera_cases_hold_every_ray_count_and_parallel_rays():
    cam = C.camera_case(8, 257, seed=31)
    seen = (cam["table"] >= 0).sum(1)
    assert set(range(2, 9)) <= set(seen.tolist()) and (seen < 2).any()
    for R in cam["R"]:
        assert np.abs(R @ R.T - np.eye(3)).max() < 1e-15
    assert np.abs(cam["K"] @ cam["Kinv"] - np.eye(3)).max() == 0
    cam = C.camera_case(4, 65, seed=115, nearly_coincident=True)
    args = (cam["table"], cam["track_pts"], cam["dst_pts"], cam["dst_offset"], cam["Kinv"], cam["R"], cam["origins"], cam["center_cam"],
            cam["view_cam"], 1)
    _, lam, n = S.triangulate_tracks(*args)
    assert (lam < 1e-3).all() and (n >= 2).all()


def test_the_random_views_split_unevenly_and_mix_matches_with_new_tracks():
    for n in (63, 257, 2049):
        views = C.random_views(n, 4, seed=100 + n)
        assert sum(len(p) for p, _ in views) == n and len(set(len(p) for p, _ in views)) > 1
    views = C.random_views(700, 8, seed=8)
    assert len(views) == 8 and all(len(p) for p, _ in views)
