"""The fundamental-matrix estimator as its specification (tests/fundamental_spec.py) defines it, on the CPU: it recovers the F
of two known poses, keeps the clean matches of contaminated scenes and drops the others, and its F has the scale, the sign
and the rank that include/apap_hip.h promises.  The kernels are pinned to this specification bit for bit by
tests/test_gpu_fundamental.py, so these are the estimator's accuracy tests."""
import numpy as np
import pytest

import fundamental_cases as C
import fundamental_spec as S
from cvx_proj_amd.spectral_method import fundamental

EPS = np.finfo(np.float64).eps
# Largest entry difference at unit Frobenius norm between the specification's F and fundamental(Rc, Ro, tc, to, K) on
# noise-free float32 points, measured over n = 8, 9, 64, 500 and scene seeds 1, 2, 3: 3.3e-8 at worst (n = 8; 9e-11 .. 3e-9
# from n = 64 on; the float64 prototype with eigh gave 2e-9 .. 8e-7).  The float32 rounding of the points (1e-4 px at 4K) and of
# the reference's own float32 skew matrix set it, not the solver.  Four times that for other seeds:
NOISE_FREE_TOL = 4 * 3.3e-8


@pytest.mark.parametrize("n", [8, 9, 64, 500])
def test_noise_free_scenes_recover_the_poses_f(n):
    for seed in (1, 2, 3):
        sc = C.two_pose_scene(n, seed)
        F, mask = S.find_fundamental(sc.src, sc.dst, 3.0, 256)
        assert F is not None and mask.all()
        err = np.abs(C.unit(F) - C.unit(fundamental(sc.Rc, sc.Ro, sc.tc, sc.to, sc.K))).max()
        print(f"n={n} seed={seed}: {err:.3e}")
        assert err < NOISE_FREE_TOL, (n, seed, err)


SCENES = [(200, 0.3, 1), (200, 0.5, 2), (2000, 0.3, 1), (2000, 0.5, 2)]      # n, contaminated share, seed (scene and call)
_FITS = {}


def fit(n, share, seed):
    if (n, share, seed) not in _FITS:
        sc = C.two_pose_scene(n, seed, noise=0.5, contaminated=share)
        _FITS[n, share, seed] = (sc,) + S.find_fundamental(sc.src, sc.dst, 3.0, S.ITERATIONS, seed)
    return _FITS[n, share, seed]


@pytest.mark.parametrize("n,share,seed", SCENES)
def test_contaminated_scenes_keep_the_clean_matches(n, share, seed):
    sc, F, mask = fit(n, share, seed)
    m = mask.ravel().astype(bool)
    kept, wrong = int((m & sc.clean).sum()), int((m & ~sc.clean).sum())
    print(f"n={n} share={share}: {kept} of {int(sc.clean.sum())} clean, {wrong} contaminated in the mask")
    assert kept >= 0.99 * sc.clean.sum() and wrong <= 0.01 * n
    r = np.abs(np.einsum("ni,ij,nj->n", np.c_[sc.dst, np.ones(n)].astype(np.float64), F, np.c_[sc.src, np.ones(n)].astype(np.float64)))
    assert np.median(r[sc.clean]) < 1.0 and np.median(r[~sc.clean]) > 100.0


@pytest.mark.parametrize("n,share,seed", SCENES)
def test_scale_sign_and_rank(n, share, seed):
    sc, F, _ = fit(n, share, seed)
    s = np.c_[sc.src.astype(np.float64), np.ones(n)]
    d = np.c_[sc.dst.astype(np.float64), np.ones(n)]
    a = s @ F.T
    g = np.sqrt(a[:, 0] ** 2 + a[:, 1] ** 2).max()
    assert abs(g - 1.0) <= 4 * EPS                        # measured: at most 1 ulp (one division and the re-evaluation)
    r = np.abs(np.sum(a * d, axis=1))
    dist = C.point_line_distance(F, sc.src, sc.dst)
    assert (r <= dist * (1 + 4 * EPS)).all()              # measured: at most 0.9 ulp above
    assert np.median(r / dist) > 0.5                      # "close to it": the lines' norms vary little across a picture
    k = np.argmax(np.abs(F))
    assert F.ravel()[k] > 0
    sv = np.linalg.svd(F, compute_uv=False)
    # measured 1.6e-19 .. 8.1e-19; numpy's own SVD resolves the smallest singular value to about eps sv[0], which is the bound
    assert sv[2] <= EPS * sv[0] and sv[1] > 1e-9 * sv[0]


@pytest.mark.parametrize("n", [8, 9])
@pytest.mark.parametrize("seed", [S.SEED, C.WRAP_SEED, 0])
def test_sampler_draws_eight_distinct_indices(n, seed):
    picks = S.sample(n, 500, seed)
    assert picks.shape == (500, 8) and picks.min() >= 0 and picks.max() < n
    assert all(len(set(p)) == 8 for p in picks.tolist())
    if n == 9:
        assert len(set(np.setdiff1d(np.arange(9), p)[0] for p in picks)) == 9      # every index is left out sometimes


def test_moments_tree_is_the_sum():
    """The re-fit's summation tree adds every inlier once: against a plain float64 sum, to rounding."""
    rng = np.random.default_rng(0)
    n = 700
    x, y, u, v = rng.uniform(-1, 1, (4, n))
    mask = (rng.random(n) < 0.6).astype(np.uint8)
    r = S.rows9(x, y, u, v)[mask.astype(bool)]
    want = (r.T @ r)[np.triu_indices(9)]
    assert np.allclose(S.moments(x, y, u, v, mask), want, rtol=1e-12, atol=1e-12)


def test_jacobi_and_rank2_against_lapack():
    rng = np.random.default_rng(1)
    r = S.rows9(*rng.uniform(-1, 1, (4, 40)))
    M = r.T @ r
    A, V = S.jacobi_eigen(M[np.triu_indices(9)])
    w = np.linalg.eigvalsh(M)
    assert np.allclose(np.sort(np.diag(A)), w, rtol=1e-10, atol=1e-13 * w[-1]) and np.allclose(V.T @ V, np.eye(9), atol=1e-14)
    f = rng.normal(size=9)
    U, s, Vt = np.linalg.svd(f.reshape(3, 3))
    want = (U[:, :2] * s[:2]) @ Vt[:2]
    assert np.allclose(S.rank2(f).reshape(3, 3), want, atol=1e-14)
