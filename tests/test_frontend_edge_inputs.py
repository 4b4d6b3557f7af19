"""The inputs of tests/frontend_edge_cases.py reach the edges they were built for: asserted from oracle/frontend_oracle.py and
plain arithmetic alone, so that tests/test_gpu_frontend_edges.py cannot pass without exercising them.  The oracle's
equalisation is also held to the statement-by-statement transcription of test_frontend.py on the planes built around the
table builder's wave boundaries, so that the kernels are compared with something that was itself checked there."""
import numpy as np
import pytest

import frontend_edge_cases as E
import test_frontend as TF
from oracle import frontend_oracle as F


# ---------------------------------------------------------------- equalisation
@pytest.mark.parametrize("C", [1, 2, 3, 4])
def test_eq_sizes_put_0_1_2_chunks_behind_every_head(C):
    assert E.HEAD_OFFSETS == (0, 1, 2, 3, 5, 15) and E.CHUNK == 3072 and E.CHUNK % C == 0
    phases = set()
    for off in E.HEAD_OFFSETS:
        head = (16 - off) % 16
        tails = E.eq_tails(C, off)
        assert 0 <= tails[0] < C and tails[1] == tails[0] + C and tails[2] < E.CHUNK <= tails[2] + C
        if head % C == 0:
            assert tails == (0, C, E.CHUNK - C)                        # empty, one pixel, one pixel short of a chunk
        want = [(head, k, t) for k in (0, 1, 2) for t in tails if head + k * E.CHUNK + t]
        sizes = E.eq_sizes(C, off)
        assert len(sizes) == len(want) >= 8
        for (h, w, c), split in zip(sizes, want):
            assert (h, c) == (1, C) and w >= 1
            assert E.eq_split(off, w * C) == split
        assert (E.other_offset(off) - off) % 16 != 0                   # the body of the output is not 16-byte aligned
        phases.add(head % C)
    assert phases == set(range(C))                                     # every channel phase of lane 0 occurs


def test_eq_tiny_images_end_inside_the_head():
    tiny = E.eq_tiny()
    assert ((1, 1, 3), 1) in tiny
    for (h, w, C), off in tiny:
        nbytes = h * w * C
        assert nbytes <= (16 - off) % 16
        assert E.eq_split(off, nbytes) == (nbytes, 0, 0)
    assert any(h * w * C == (16 - off) % 16 for (h, w, C), off in tiny)     # the head exactly
    assert {C for (_, _, C), _ in tiny} == {1, 2, 3, 4}


def test_eq_image_has_another_table_per_channel():
    img = E.eq_image((1, 1029, 4))
    luts = [F.equalize_lut(np.bincount(img[..., c].ravel(), minlength=256), img[..., c].size) for c in range(4)]
    for a in range(4):
        for b in range(a + 1, 4):
            assert not np.array_equal(luts[a], luts[b])


@pytest.mark.parametrize("kind,occupied", [("above", lambda i0: 256 - i0), ("two", lambda i0: 2), ("all", lambda i0: 256)])
def test_eq_bins_first_bin_and_occupancy(kind, occupied):
    planes = E.eq_bins(kind)
    assert tuple(planes) == ((0,) if kind == "all" else (0, 63, 64, 127, 128, 191, 192, 254))
    for i0, plane in planes.items():
        hist = np.bincount(plane.ravel(), minlength=256)
        assert int(np.flatnonzero(hist)[0]) == i0 and int(np.count_nonzero(hist)) == occupied(i0)
        assert hist.max() > hist[hist > 0].min()                       # unequal bins
        out = F.equalize_hist_channel(plane)
        assert np.array_equal(out, TF.scalar_equalize(plane))          # the oracle is right at these bins
        assert out.min() == 0 and out.max() == 255
        assert np.array_equal(out, plane) == (kind == "two" and i0 == 0)   # only {0, 255} is its own equalisation


def test_eq_four_channels_differ_and_only_the_constant_one_is_returned_unchanged():
    img = E.eq_four_channels()
    assert img.shape[2] == 4 and (img[..., 0] == 255).all()
    assert sorted(np.unique(img[..., 1]).tolist()) == [100, 200]
    assert int(img[..., 2].min()) == 64 and int(img[..., 3].min()) == 191
    out = F.equalize_hist_image(img)
    assert np.array_equal(out[..., 0], img[..., 0])
    for c in (1, 2, 3):
        assert not np.array_equal(out[..., c], img[..., c])
        assert np.array_equal(out[..., c], TF.scalar_equalize(img[..., c]))


def test_eq_known_answers_hold_both_ties_to_even():
    (plane, answer), (two, two_answer) = E.eq_known_answers()
    assert F.equalize_hist_channel(plane).tolist() == answer.tolist() == [[0, 42, 128, 128, 170, 255, 255]]
    assert F.equalize_hist_channel(two).tolist() == two_answer.tolist() == [[0, 0, 0, 255]]
    hist = np.bincount(plane.ravel(), minlength=256)
    scale = np.float32(255.0) / np.float32(plane.size - hist[0])
    products = (np.cumsum(hist[1:5]).astype(np.float32) * scale).tolist()
    assert 42.5 in products and 127.5 in products                      # exact ties: one rounds down, one up
    assert answer[0, 1] == 42 and answer[0, 2] == 128


@pytest.mark.parametrize("C", [1, 2, 4])
def test_eq_strided_gives_half_the_waves_a_second_chunk(C):
    h, w, c = E.STRIDED_SHAPES[C]
    assert c == C
    waves = E.MAX_BLOCKS * E.WAVES
    for off in (0, 5):
        head, chunks, tail = E.eq_split(off, h * w * c)
        assert waves == 4096 < chunks < 2 * waves                      # some waves take a second chunk, none a third
        assert (h * w * c // E.CHUNK + 1 + E.WAVES - 1) // E.WAVES > E.MAX_BLOCKS    # the grid is capped at MAX_BLOCKS blocks
        assert 0 < chunks - waves < waves
    img = E.eq_strided(C)
    assert img.shape == (h, w, c) and img.dtype == np.uint8
    for ch in range(C):
        levels = np.unique(img[::16, :, ch])
        assert len(levels) == 32 and int(levels[0]) == 40 + 37 * ch    # narrow band: bins of about 600 000


# ---------------------------------------------------------------- RANSAC
def test_ransac_tie_case_decides_the_tie_rule():
    src, dst, thresh, K, seed = E.ransac_ties()
    assert len(src) == 257 and K == 600 and np.array_equal(src, np.rint(src)) and np.array_equal(dst, np.rint(dst))
    core = E.ransac_core("ties")
    facts = E.tie_facts(core["counts"])
    print({k: (len(v) if hasattr(v, "__len__") else v) for k, v in facts.items()})
    assert len(facts["tied"]) >= 2                                     # a tie at the maximum
    assert facts["first"] != 0 and core["best"] == facts["first"]      # "any tied one" or "index 0" is not the answer
    assert facts["earlier_thread"]                                     # a tie broken on the thread number picks one of these
    assert facts["same_thread"]                                        # ">=" inside a thread's scan picks i + 256
    assert core["count"] == int((core["mask"] != 0).sum()) == 217


def test_ransac_all_nan_and_duplicates():
    core = E.ransac_core("all NaN")
    assert len(E.ransac_all_nan()[0]) == 9
    assert np.isnan(core["H"]).all() and core["count"] == 0 and core["best"] == 0 and not core["mask"].any()
    assert not core["counts"].any()
    src, dst, thresh, K, seed = E.ransac_duplicates()
    assert len(src) == 60 and np.array_equal(src[0::2], src[1::2]) and np.array_equal(dst[0::2], dst[1::2])
    core = E.ransac_core("duplicates")
    bad = np.isnan(core["H"]).any(axis=1)
    assert 0 < int(bad.sum()) < K and np.array_equal(bad, np.isnan(core["H"]).all(axis=1))
    pairs = np.sort(core["picks"] // 2, axis=1)
    assert np.array_equal(bad, (pairs[:, 1:] == pairs[:, :-1]).any(axis=1))      # exactly the samples with both copies of a point
    assert not core["counts"][bad].any() and core["count"] >= 4


@pytest.mark.parametrize("k", [3, 4])
def test_ransac_count_cases_have_a_best_count_of_exactly(k):
    core = E.ransac_core(f"count {k}")
    assert core["count"] == k == int(core["counts"].max()) == int(core["mask"].sum())
    assert set(np.flatnonzero(core["mask"]).tolist()) <= set(core["picks"][core["best"]].tolist())    # only its own sample


def test_ransac_grids_and_seeds():
    assert E.GRID_K == (1, 63, 64, 65, 255, 256, 257, 2049) and E.GRID_N == (5, 6, 7, 255, 256, 257, 513)
    cases = E.ransac_cases()
    for K in E.GRID_K:
        assert cases[f"n=57 K={K}"][3] == K and len(cases[f"n=57 K={K}"][0]) == 57
    for n in E.GRID_N:
        assert len(cases[f"n={n} K=65"][0]) == n and cases[f"n={n} K=65"][3] == 65
        assert E.ransac_core(f"n={n} K=65")["count"] >= 4
    assert E.SEEDS == (0, 2 ** 64 - 5, 2 ** 63)
    wrap = E.SEEDS[1]
    src, dst, thresh, K, seed = cases[f"seed {wrap:#x}"]
    assert seed == wrap and seed + 4 * 1 + 0 < 2 ** 64 <= seed + 4 * 1 + 1 and seed + 4 * K > 2 ** 64   # wraps inside hypothesis 1
    picks = {s: E.ransac_core(f"seed {s:#x}")["picks"] for s in E.SEEDS}
    for p in picks.values():
        assert p.shape == (K, 4) and p.min() >= 0 and p.max() < len(src)
        s = np.sort(p, axis=1)
        assert (s[:, 1:] != s[:, :-1]).all()
    # the wrapped counter continues at 0: hypothesis h >= 2 of the wrap seed draws what seed 0 draws 5 counters earlier
    flat = lambda s: F.splitmix64((np.uint64(s) + np.arange(4 * K, dtype=np.uint64)))     # noqa: E731
    with np.errstate(over="ignore"):
        assert np.array_equal(flat(wrap)[5:], flat(0)[:4 * K - 5])
    assert not np.array_equal(picks[wrap], picks[0]) and not np.array_equal(picks[1 << 63], picks[0])


def test_ransac_thresholds_whose_squares_are_zero_and_infinite():
    assert E.THRESHOLDS == (0.0, 1e-200, 1e200) and 1e-200 * 1e-200 == 0.0 and 1e200 * 1e200 == np.inf
    for prefix in ("", "duplicates, "):
        zero, tiny, huge = (E.ransac_core(f"{prefix}thresh {t:g}") for t in E.THRESHOLDS)
        assert np.array_equal(zero["counts"], tiny["counts"]) and zero["best"] == tiny["best"]
        assert zero["count"] == (8 if prefix else 3)       # what a hypothesis reproduces without any rounding error
        src, dst = E.ransac_cases()[f"{prefix}thresh 1e+200"][:2]
        err = F.ransac_errors(huge["H"], src, dst)
        assert np.array_equal(huge["counts"], (~np.isnan(err)).sum(axis=1))          # everything but NaN passes
        assert huge["count"] == len(src)
    nan_rows = np.isnan(E.ransac_core("duplicates, thresh 1e+200")["H"]).any(axis=1)
    assert nan_rows.any() and not E.ransac_core("duplicates, thresh 1e+200")["counts"][nan_rows].any()


@pytest.mark.parametrize("seed_name", list(E.POOL_SEEDS))
@pytest.mark.parametrize("model,n", E.SMALL_POOLS)
def test_small_pools_force_the_last_picks_and_still_give_a_model(model, n, seed_name):
    """n = K: every hypothesis draws a permutation of all n matches; n = K + 1: all but one.  The winner keeps at least K
    inliers, so neither wrapper's "no model" branch hides the comparison."""
    K = {"homography": 4, "fundamental": 8}[model]
    assert n in (K, K + 1) and E.POOL_ITERATIONS == E.HYP_LANES + 1
    case, core = E.small_pool_case(model, n, seed_name), E.small_pool_core(model, n, seed_name)
    if model == "homography":
        picks, seed = core["picks"], case[4]
    else:
        import fundamental_spec as S
        picks, seed = S.sample(n, E.POOL_ITERATIONS, case.seed), case.seed
        assert np.isfinite(core["F"]).all()
    assert picks.shape == (E.POOL_ITERATIONS, K)
    assert all(len(set(p.tolist())) == K and 0 <= p.min() and p.max() < n for p in picks)
    assert len({tuple(p.tolist()) for p in picks}) > 1                                      # not one sample 65 times
    assert core["count"] >= K and not np.isnan(core["H"][core["best"]]).any()
    if seed_name == "wrap":
        assert seed + K * 2 > 2 ** 64 > seed         # the counter wraps inside hypothesis 0 (K = 8) or 1 (K = 4)
