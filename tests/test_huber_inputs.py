"""The inputs of the Huber M-step's tests reach the edges they are named for, judged by the numpy specification alone
(tests/huber_spec.py): a GPU test on a case that misses its edge would prove nothing."""
import hashlib

import numpy as np
import pytest

import huber_cases as HC
import huber_spec as HS
import model_spec as S

CASES = HC.cases()


@pytest.fixture(scope="module")
def solved():
    out = {}
    for name, c in CASES.items():
        if c["expect"] != "degenerate":
            out[name] = HS.solve_points(c["pc"], c["po"], c["w"], c["M"], c["cap"] or HS.DEFAULT_CAP, c["floor"])
    return out


def test_inputs_are_reproducible():
    """Integer hashing and + - * / only: the same bytes on every numpy."""
    a, b = HC.cases(), HC.cases()
    for name in a:
        for k in ("pc", "po", "w"):
            assert a[name][k].tobytes() == b[name][k].tobytes() and a[name][k].dtype == np.float32
    c = a["clean_500"]
    digest = hashlib.sha256(c["pc"].tobytes() + c["po"].tobytes() + c["w"].tobytes()).hexdigest()
    assert digest == HC.CLEAN_500_SHA256


def test_case_sizes():
    T = HC.T
    sizes = {k: len(c["pc"]) for k, c in CASES.items()}
    assert sizes["n4"] == 4 and sizes["n5"] == 5 and sizes["n3"] == 3
    assert (sizes["n24"], sizes["n25"], sizes["n240"], sizes["n241"]) == (24, 25, 240, 241)
    assert [2 * sizes[k] for k in ("rows_T_minus_2", "rows_T", "rows_T_plus_2")] == [T - 2, T, T + 2]
    assert [sizes[k] for k in ("matches_T_minus_1", "matches_T", "matches_T_plus_1")] == [T - 1, T, T + 1]
    assert max(sizes.values()) <= 2000
    for k in ("clean_2000", "moderate_2000", "gross_2000"):
        assert sizes[k] > 4 * T                 # every thread sums several matches
    c = CASES["empty_fold"]
    keep = c["w"].astype(np.float64) > c["floor"]
    assert not keep[24:48].any() and keep[:24].all() and keep[48:].all()
    w = CASES["subnormal_weights"]["w"]
    assert (w[::5] > 0).all() and (w[::5] < np.finfo(np.float32).tiny).all()
    assert abs(CASES["moderate_2000"]["inlier"].mean() - 0.95) < 0.02 and abs(CASES["gross_2000"]["inlier"].mean() - 0.8) < 0.03


@pytest.mark.parametrize("name", HC.CONVERGING)
def test_converging_cases_close_the_gap(solved, name):
    """A condition on the inputs: the specification's own gap, recomputed in extended precision, is below 1e-10, and no
    residual of its optimum lies within 1e-6 of M (a clipped set that rounding could flip)."""
    c = CASES[name]
    A, rhs, r = solved[name]
    g = HS.gap(A, rhs, r.h, c["M"])
    near = np.abs(np.abs(A @ r.h - rhs) - c["M"]).min()
    print(f"{name}: rows {len(rhs)} steps {r.iterations} fallbacks {r.fallbacks} clipped {r.clipped:.3f} gap {r.gap:.2e} "
          f"(extended {g:.2e}) nearest |r| - M {near:.1e}")
    assert r.converged and r.gap <= HS.GAP_TOL and -1e-12 <= g <= 1e-10
    assert near > 1e-6
    assert 2 * r.iterations <= HS.DEFAULT_CAP <= 200       # the default cap: at least twice every count here
    assert r.f <= r.f0


def test_clipped_shares(solved):
    assert solved["M_1e6"][2].clipped == 0 and solved["M_1e6"][2].iterations == 0
    assert solved["n4"][2].clipped == 0 and solved["n4"][2].iterations == 0        # an exact fit: nothing to clip
    assert solved["n5"][2].clipped == 0
    assert solved["M_0p011_clean"][2].clipped > 0.95                               # a near-L1 problem
    assert 0.3 < solved["clean_2000"][2].clipped < 0.6
    assert solved["gross_2000"][2].clipped > 0.8
    assert 0.02 < solved["moderate_500_M2"][2].clipped < 0.1
    for name in HC.CONVERGING:
        if name not in ("n5",):
            assert solved[name][2].clipped > 0 and solved[name][2].iterations >= 1, name


def test_fallback_and_cap_cases(solved):
    assert solved["gross_2000"][2].fallbacks >= 1 and solved["gross_2000"][2].converged
    hard = solved["M_0p011_gross"][2]
    assert hard.iterations == HS.DEFAULT_CAP and hard.fallbacks >= 1 and not hard.converged
    cap = solved["cap_1"][2]
    assert cap.iterations == 1 and not cap.converged and cap.gap > 1e-6 and cap.f < cap.f0


def test_M_sits_on_a_residual():
    c = CASES["M_at_a_residual"]
    A, rhs = HS.problem(c["pc"], c["po"], c["w"])
    h0 = S.solve(c["pc"], c["po"], c["w"], "lms")[0]
    r = np.abs(A @ h0 - rhs)
    assert (r == c["M"]).sum() == 1 and 0.1 < (r > c["M"]).mean() < 0.3


def test_degenerate_cases():
    c = CASES["collinear"]
    A, _ = HS.problem(c["pc"], c["po"], c["w"])
    assert np.linalg.matrix_rank(A) < 8
    assert len(CASES["n3"]["pc"]) < 4
