"""tests/sfm_spec.py against the reference: its tracks equal what the reference's own get_covid returned (tests/golden/
sfm_ref.npz, written by tests/golden/make_sfm_golden.py) exactly; its rays and positions agree with the reference's
world_frame_ray_dir and solve_3d_position within four times the largest difference measured; and the fixed-point form that
the kernels take equals the sequential one."""
import numpy as np
import pytest

import sfm_cases as C
import sfm_spec as S

# measured against the recorded reference outputs (numpy's matmul and SVD on the fixture's machine), relative to
# max(1, |value|); the assertions allow four times these
MEASURED_RAY = 5.551e-17
MEASURED_X_UNCLAMPED = 8.553e-14
MEASURED_X_CLAMPED = 2.100e-12


@pytest.mark.parametrize("name", C.REFERENCE_TRACK_CASES)
def test_tracks_equal_the_reference(golden, name):
    ref = golden("sfm_ref")
    views = C.track_cases()[name]
    table, pts, _ = S.covis_tracks(views)
    want = ref[f"tracks_{name}_table"]
    assert want.shape[1] == 4 and (want[:, len(views):] == -1).all()           # the reference's rows are 4 long
    assert np.array_equal(table, want[:, :len(views)]) and table.dtype == np.int32
    assert pts.dtype == np.float32 and pts.tobytes() == ref[f"tracks_{name}_pts"].tobytes()


@pytest.mark.parametrize("name", [k for k, v in C.track_cases().items() if sum(len(p) for p, _ in v) <= 160])
def test_the_array_search_is_the_plain_loop(name):
    views = C.track_cases()[name]
    for a, b in zip(S.covis_tracks(views), S.covis_tracks(views, plain=True)):
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes()


def fixed_point_equals_sequence(views, eps=S.EPS):
    table, pts, point_track = S.covis_tracks(views, eps)
    f_table, f_pts, f_point_track, rounds = S.covis_tracks_fixed_point(views, eps)
    assert np.array_equal(table, f_table) and pts.tobytes() == f_pts.tobytes() and np.array_equal(point_track, f_point_track)
    return rounds


@pytest.mark.parametrize("name", list(C.track_cases()))
def test_the_fixed_point_equals_the_sequence_on_the_cases(name):
    fixed_point_equals_sequence(C.track_cases()[name])


def test_the_fixed_point_equals_the_sequence_on_seeded_inputs():
    """What the kernels' correctness argument rests on, also where boxes overlap without being transitive."""
    for n, v, seed in ((63, 4, 163), (257, 4, 357), (700, 8, 8), (400, 3, 5)):
        fixed_point_equals_sequence(C.random_views(n, v, seed=seed))
    dense = C.random_views(500, 5, seed=9, base_frac=0.05, jitter=0.3)          # many overlapping boxes
    assert fixed_point_equals_sequence(dense) >= 2
    fixed_point_equals_sequence(dense, eps=np.float32(0.25))
    assert fixed_point_equals_sequence(C.chain_views(300)) >= 256


def test_rays_agree_with_the_reference(golden):
    ref = golden("sfm_ref")["rays_dirs"]
    cam = C.camera_case(4, 16, seed=21)
    pix = np.concatenate([cam["track_pts"], cam["dst_pts"][:16]]).astype(np.float32).reshape(-1, 2, 1)
    Rs = np.stack([cam["R"][k % len(cam["R"])] for k in range(len(pix))])
    got = S.world_frame_ray_dir(np.linalg.inv(cam["K"]), pix, Rs)
    worst = np.abs(got - ref).max()
    print(f"world_frame_ray_dir: largest difference {worst:.3e}")
    assert got.shape == ref.shape == (32, 3, 1) and worst <= 4 * MEASURED_RAY
    assert np.abs(np.sqrt((got ** 2).sum(1)) - 1).max() < 1e-15
    from cvx_proj_amd import utils
    assert utils.world_frame_ray_dir(np.linalg.inv(cam["K"]), pix, Rs).tobytes() == got.tobytes()      # the module's numpy form


def test_positions_agree_with_the_reference(golden):
    ref = golden("sfm_ref")
    origins, dirs, off = C.ray_case(**C.RAY_CASE)
    X, lam, n = S.triangulate_rays(origins, dirs, off)
    rel = np.abs(X - ref["tri_X"]).max(1) / np.maximum(1.0, np.abs(ref["tri_X"]).max(1))
    clamped = ref["tri_smin"] < 1e-3
    print(f"solve_3d_position: largest relative difference {rel[~clamped].max():.3e} unclamped, {rel[clamped].max():.3e} clamped")
    assert rel[~clamped].max() <= 4 * MEASURED_X_UNCLAMPED and rel[clamped].max() <= 4 * MEASURED_X_CLAMPED
    assert np.abs(lam - ref["tri_smin"]).max() < 1e-14 and (n == np.diff(off)).all()


def test_noise_free_rays_recover_their_point():
    for seed in range(5):
        u = C.uniform(3 * 6, seed, 0).reshape(6, 3)
        origins = np.stack([u[:, 0] * 50.0, u[:, 1] * 50.0, 60.0 + u[:, 2] * 20.0], axis=1)
        point = np.array([20.0 + seed, 30.0 - seed, -3.0])
        d = point - origins
        dirs = d / np.sqrt((d * d).sum(1))[:, None]
        for count in (2, 3, 6):
            X, lam, n = S.solve_rays(origins[:count], dirs[:count])
            assert n == count and lam > 1e-3 and np.abs(X - point).max() < 1e-11


def test_degenerate_tracks():
    X, lam, n = S.solve_rays(np.zeros((0, 3)), np.zeros((0, 3)))
    assert n == 0 and np.isnan(X).all() and np.isnan(lam)
    X, lam, n = S.solve_rays(np.array([[1.0, 2.0, 3.0]]), np.array([[0.0, 0.6, 0.8]]))      # one ray: finite, its origin's foot
    assert n == 1 and lam < 1e-3 and np.isfinite(X).all()
    X, lam, n = S.solve_rays(np.array([[0.0, 0.0, 1.0], [1.0, 1.0, 1.0]]), np.array([[np.nan, 0.0, 1.0], [0.0, 1.0, 0.0]]))
    assert n == 2 and np.isnan(lam) and X.tobytes() == np.full(3, np.nan).tobytes()          # the canonical NaN
