"""The inputs of tests/fundamental_cases.py reach the edges they are named after: asserted from the specification
(tests/fundamental_spec.py) on the CPU, so that tests/test_gpu_fundamental.py compares the kernels where it matters."""
import numpy as np

import fundamental_cases as C
import fundamental_spec as S

EDGE = {c.name: c for c in C.edge_cases()}
SHAPE = {c.name: c for c in C.shape_cases()}


def nan_rows(H):
    return np.isnan(H).all(axis=1)


def test_every_matrix_is_whole_or_all_nan():
    for c in list(EDGE.values()) + list(SHAPE.values()):
        e = C.expected(c)
        for M in (e["H"], e["F"][None], e["winner"][None]):
            assert np.array_equal(np.isnan(M).any(axis=1), nan_rows(M)), c.name
            assert np.isfinite(M[~nan_rows(M)]).all(), c.name
            assert (M[nan_rows(M)].view(np.uint64) == 0x7FF8000000000000).all(), c.name


def test_n8_every_hypothesis_is_the_same_eight_matches():
    c = EDGE["n8_permutations"]
    picks = C.expected(c)["picks"]
    assert len(c.src) == 8 and (np.sort(picks, axis=1) == np.arange(8)).all()
    assert len({tuple(p) for p in picks}) > 32               # in many orders
    assert not nan_rows(C.expected(c)["H"]).any() and C.expected(c)["count"] == 8


def test_integer_grid_some_hypotheses_meet_a_zero_pivot():
    c = EDGE["integer_grid"]
    e = C.expected(c)
    assert e["box"][2] == 0.5 and e["box"][6] == 0.5          # exact normalised coordinates
    bad = int(nan_rows(e["H"]).sum())
    assert 16 <= bad <= c.iterations - 16


def test_no_model_cases():
    one = C.expected(EDGE["one_match_eight_times"])
    assert one["box"][3] == 0 and one["box"][7] == 0 and np.isinf(one["box"][2])
    assert nan_rows(one["H"]).all() and one["count"] == 0 and one["best"] == 0 and np.isnan(one["F"]).all()
    c = EDGE["thresh0_unrelated"]
    e = C.expected(c)
    assert c.thresh == 0 and not nan_rows(e["H"]).any() and 0 < e["count"] < 8 and np.isnan(e["F"]).all()
    assert e["mask"].sum() == e["count"]                     # the device form's mask is the winner's also then
    F, mask = S.find_fundamental(c.src, c.dst, c.thresh, c.iterations, c.seed)
    assert F is None and not mask.any()


def test_collinear_equal_planar_and_wrapping_inputs():
    c = EDGE["collinear"]
    for pts in (c.src, c.dst):
        d = pts.astype(np.float64) - pts[0]
        assert np.abs(d[:, 0] * d[-1, 1] - d[:, 1] * d[-1, 0]).max() < 1e-3 * np.abs(d[-1]).max()
    assert nan_rows(C.expected(c)["H"]).any() and not nan_rows(C.expected(c)["H"]).all()
    c = EDGE["src_equals_dst"]
    assert np.array_equal(c.src, c.dst) and C.expected(c)["count"] == len(c.src)
    c = EDGE["planar"]
    e = C.expected(c)
    sv = np.linalg.svd(e["F"].reshape(3, 3), compute_uv=False)
    assert e["count"] >= 0.99 * len(c.src) and np.isfinite(e["F"]).all() and sv[2] < 1e-12 * sv[0] and sv[1] > 1e-9 * sv[0]
    c = EDGE["wrapping_seed"]
    assert c.seed + 8 * c.iterations > 1 << 64 and c.seed + 7 >= 1 << 64 and len(c.src) == 9
    assert np.array_equal(S.sample(9, 4, c.seed)[1:], S.sample(9, 3, (c.seed + 8) % (1 << 64)))


def test_shape_cases_cover_the_strides():
    assert tuple(len(SHAPE[f"n{n}"].src) for n in C.N_VALUES) == C.N_VALUES
    assert {c.iterations for c in SHAPE.values()} == set(C.ITERATION_VALUES)
    assert {c.thresh for c in SHAPE.values()} == set(C.THRESH_VALUES)
    for n in C.N_VALUES:
        e = C.expected(SHAPE[f"n{n}"])
        assert e["count"] >= 8 and np.isfinite(e["F"]).all(), n
        assert len(set(e["counts"].tolist())) > 1 or n <= 9, n         # the scores tell hypotheses apart
    inf = C.expected(SHAPE["threshinf"])
    assert inf["best"] == 0 and inf["count"] == 257 and (inf["counts"] == 257).all()
    zero = C.expected(SHAPE["thresh0.0"])
    assert zero["count"] <= 8
    # the re-fit's lanes: more inliers than one pass of the block at n = 1000, fewer than a wave at n = 63
    assert C.expected(SHAPE["n1000"])["count"] > 256 and C.expected(SHAPE["n63"])["count"] < 64


def test_batch_case_starts_above_zero():
    src, dst, off = C.batch_case()
    assert off[0] == 13 and np.diff(off).tolist() == [8, 257, 64, 1000] and len(src) == off[-1] == len(dst)
