"""The numpy specification of the Huber M-step (tests/huber_spec.py) against checks that do not share its method: the
duality gap as a bound, scipy's quasi-Newton minimiser on f, and what the loss is for (outliers count for less)."""
import numpy as np
import pytest

import huber_cases as HC
import huber_spec as HS
import model_spec as S

CASES = HC.cases()


def solved(name):
    c = CASES[name]
    return HS.solve_points(c["pc"], c["po"], c["w"], c["M"], c["cap"] or HS.DEFAULT_CAP, c["floor"])


def test_phi_is_cvxpys_huber():
    r = np.array([-3.0, -0.5, -0.25, 0.0, 0.25, 0.5, 2.0])
    np.testing.assert_array_equal(HS.phi(r, 0.5), [2.75, 0.25, 0.0625, 0.0, 0.0625, 0.25, 1.75])
    # continuous with a continuous derivative at |r| = M
    M, e = 0.7, 1e-7
    assert abs(HS.phi(np.array([M + e]), M)[0] - HS.phi(np.array([M - e]), M)[0] - 2 * M * 2 * e) < 1e-12


def test_the_dual_value_is_a_lower_bound_for_any_h():
    """gap >= 0 (to rounding) at arbitrary points, and f(h) (1 - gap(h)) never exceeds the optimum."""
    A, rhs, r = solved("moderate_500_M2")
    M = CASES["moderate_500_M2"]["M"]
    best = float(HS.objective(A, rhs, r.h, M))
    rng = np.random.default_rng(0)
    for scale in (1e-9, 1e-6, 1e-3, 0.1):
        h = r.h * (1 + scale * rng.normal(size=8))
        g = HS.gap(A, rhs, h, M)
        f = float(HS.objective(A, rhs, h, M))
        assert g >= -1e-13 and f >= best * (1 - 1e-13)
        assert f * (1 - g) <= best * (1 + 1e-12), (scale, f, g, best)


def test_the_gap_tells_converged_from_perturbed():
    A, rhs, r = solved("clean_500")
    M = CASES["clean_500"]["M"]
    assert HS.gap(A, rhs, r.h, M) <= 1e-10
    rng = np.random.default_rng(1)
    g = HS.gap(A, rhs, r.h * (1 + 1e-5 * rng.normal(size=8)), M)
    assert g > 1e-9


@pytest.mark.parametrize("name", HC.CONVERGING)
def test_scipy_finds_no_lower_point(name):
    optimize = pytest.importorskip("scipy.optimize")
    c = CASES[name]
    A, rhs, r = solved(name)
    M = c["M"]
    s = 1.0 / np.sqrt((A * A).sum(axis=0))
    As = A * s

    def fun(x):
        res = As @ x - rhs
        y = 2 * np.clip(res, -M, M)
        return HS.phi(res, M).sum(), As.T @ y

    pc, po, w = S.select(c["pc"], c["po"], c["w"], c["floor"])
    h0 = S.solve(pc, po, w, "lms")[0]
    out = optimize.minimize(fun, h0 / s, jac=True, method="L-BFGS-B", options=dict(maxiter=5000, ftol=1e-15, gtol=1e-10, maxcor=30))
    f_spec = float(HS.objective(A, rhs, r.h, M))
    f_ref = float(HS.objective(A, rhs, out.x * s, M))
    print(f"{name}: f {f_spec:.12g}, scipy {f_ref:.12g} after {out.nit} iterations")
    assert f_spec <= f_ref * (1 + 1e-12)
    assert f_ref - f_spec <= 1e-6 * f_spec


def test_huber_beats_least_squares_on_moderate_outliers():
    """5 % of the matches displaced by 5 .. 30 px: the inliers' reprojection error under the Huber fit is below the
    least-squares fit's."""
    c = CASES["moderate_2000"]
    A, rhs, r = solved("moderate_2000")
    h_lms = S.solve(c["pc"], c["po"], c["w"], "lms")[0]

    def rmse(h):
        H = np.append(h, 1.0).reshape(3, 3)
        q = np.hstack([c["pc"].astype(np.float64), np.ones((len(c["pc"]), 1))]) @ H.T
        d = q[:, :2] / q[:, 2:] - c["po"]
        return float(np.sqrt((d[c["inlier"]] ** 2).sum(axis=1).mean()))
    a, b = rmse(r.h), rmse(h_lms)
    print(f"inlier RMSE: Huber {a:.4f} px, least squares {b:.4f} px")
    assert a < b
