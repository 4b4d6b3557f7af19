"""The numpy specification of the spectral weighting (tests/spectral_spec.py), without a GPU: first against the reference's
own calculate_M (tests/golden/spectral_*.npz) at the tolerances tests/test_gpu_spectral.py holds the engine to, then the
conditions every generated case of tests/test_gpu_spectral_edges.py must meet, here for n <= 4100 (the two larger ones are
checked in that module, where their references are computed anyway)."""
import functools
import glob
import os

import numpy as np
import pytest

import spectral_spec as S
from conftest import GOLDEN, ulp_diff_f32

FIXTURES = sorted(glob.glob(os.path.join(GOLDEN, "spectral_*.npz")))
SMALL = [c for c in S.cases() if c.n <= 4100]


def load(path):
    g = dict(np.load(path))
    if "codebook" in g:     # the largest case stores its descriptors as rows of a codebook
        g["c_feats"], g["o_feats"] = g["codebook"][g["c_index"]], g["codebook"][g["o_index"]]
    g["c"] = g["c_feats"].astype(np.float32)
    g["o"] = g["o_feats"].astype(np.float32)
    return g


def test_the_fixtures_are_all_here():
    assert len(FIXTURES) == 11
    assert sorted(len(np.load(p)["src"]) for p in FIXTURES) == [1, 2, 7, 40, 48, 64, 300, 500, 500, 2000, 5000]


@pytest.mark.parametrize("path", FIXTURES, ids=os.path.basename)
def test_specification_matches_the_reference(path):
    g = load(path)
    opts = S.Opts(*(float(x) for x in g["opts"]))
    diag, off = S.affinity(g["src"], g["dst"], g["c"], g["o"], g["F"], opts)
    if "M_off" in g:
        assert off.view(np.uint32).tobytes() == g["M_off"].view(np.uint32).tobytes()
        assert (np.abs(diag - g["M_diag"]) <= 4 * np.spacing(np.abs(g["M_diag"]))).all()
    lam, v, delta, gap, r_ref = S.principal(diag, off)
    assert abs(lam - float(g["lam"])) <= 1e-12 * abs(float(g["lam"]))
    ms = S.match_score(g["c"], g["o"])
    mask = S.initial_mask(g["src"], g["dst"], ms, g["Hg"], opts) if "Hg" in g else g["mask"]
    seg, rm, om = S.finish(v, mask, opts)
    assert np.abs(seg - g["segment"]).max() <= 1e-9
    assert np.array_equal(seg > opts.aff_thresh, g["segment"] > opts.aff_thresh)
    assert np.array_equal(om, g["original_mask"])
    assert ulp_diff_f32(rm, g["ransac_mask"]).max() <= 1
    if len(diag) > 1:
        assert abs(gap - float(g["gap"])) <= 1e-9
        assert S.tolerance(lam, v, delta, r_ref) <= 1e-9      # the derived bound is no wider than the fixtures' fixed one


def test_group_sizes():
    assert S.group_sizes(300, 1) == [300]
    for n, g in ((300, 2), (301, 3), (257, 5)):
        sizes = S.group_sizes(n, g)
        assert sum(sizes) == n and len(set(sizes)) == g and all(b - a >= 1 for a, b in zip(sizes, sizes[1:])), sizes


def test_case_list():
    names = [c.name for c in S.cases()]
    assert len(names) == len(set(names)) == 14 + 3 + 2 + 4 + 7 + 3
    assert [c.n for c in S.cases() if c.name.startswith("translation_")] == list(S.TRANSLATION_N)
    assert sorted(c.n for c in S.cases() if c.n > 4100) == [8192, 8193, 8193]


@functools.lru_cache(maxsize=None)
def built(name):
    return S.build(next(c for c in SMALL if c.name == name))


@pytest.mark.parametrize("case", SMALL, ids=repr)
def test_case_meets_its_conditions(case):
    b = built(case.name)
    assert b is not None, "no seed met the conditions"
    n = case.n
    steps, cycles, how = b.emulated
    raw = S.raw_segment(b.v)
    print(f"{case.name}: seed {b.seed} lam {b.lam:.6g} gap {b.gap:.3g} delta {b.delta:.3g} r_ref {b.r_ref:.2e} tol {b.tol:.2e} "
          f"emulated steps {steps} cycles {cycles} {how}")
    assert b.gap >= 1e-3
    assert b.tol == S.tolerance(b.lam, b.v, b.delta, b.r_ref) and b.tol <= 1e-7
    assert np.abs(raw - case.opts.aff_thresh).min() > 10 * b.tol and np.abs(raw - 1e-6).min() > 10 * b.tol
    if case.family in ("scale", "disjoint"):
        assert cycles >= 2 and how == "converged" and b.residuals[1] >= S.SEVERAL_MARGIN * S.TOL
    if case.family == "groups":
        assert (steps == 1 and cycles == 0 and how == "converged") if case.groups == 1 else how == "breakdown"
    if case.name.startswith("translation_") and n >= 63:
        assert cycles == 1 and how == "converged"
    assert S.conditions(case, b) == []
    # the inputs are what the families promise
    assert b.src.dtype == b.dst.dtype == b.c.dtype == b.o.dtype == np.float32 and b.src.shape == (n, 2) and b.c.shape == (n, 128)
    assert np.array_equal(b.c, np.rint(b.c)) and np.array_equal(b.o, np.rint(b.o))
    assert set(np.unique(b.mask)) <= {0.0, 1.0}
    if case.family == "disjoint":
        assert not S.off_diagonal_f32(b.src, b.dst, case.opts.affinity_eps).any()
        assert np.count_nonzero(b.segment) == 1 and b.segment.max() == 1.0
    if case.zero_k2:
        i = n // 2
        Hg = b.Hg
        assert (Hg[2, 0] * b.dst[i, 0] + Hg[2, 1] * b.dst[i, 1]) + Hg[2, 2] == 0 and b.initial[i] == 0
    if case.use_hg:
        assert 0 < b.initial.sum() < n


def test_build_is_deterministic():
    case = next(c for c in SMALL if c.name == "translation_257")
    a, b = S.build(case), built(case.name)
    assert a.seed == b.seed
    for x, y in ((a.src, b.src), (a.c, b.c), (a.mask, b.mask), (a.segment, b.segment)):
        assert x.tobytes() == y.tobytes()


def test_emulation_on_a_matrix_with_a_known_answer():
    """diag(3, 2, 1) + a rank-one link: the whole space at n = 3, so one cycle of 3 steps and one more step to notice."""
    diag = np.array([3.0, 2.0, 1.0])
    off = np.float32([[0, 0.5, 0], [0.5, 0, 0.25], [0, 0.25, 0]])
    assert S.lanczos_cycles(diag, off) == (4, 1, "converged")
    # ones is an eigenvector: convergence at step 1, no tridiagonal solve
    assert S.lanczos_cycles(np.full(5, 2.0), np.float32(np.ones((5, 5)) - np.eye(5))) == (1, 0, "converged")
    # two invariant blocks of unequal size: a Krylov space of dimension 2
    off = np.zeros((7, 7), np.float32)
    off[:4, :4] = 1
    off[4:, 4:] = 1
    np.fill_diagonal(off, 0)
    steps, cycles, how = S.lanczos_cycles(np.full(7, 1.0), off)
    assert how == "breakdown" and cycles == 1
