"""The spectral solver on the MI355X where the reference's fixtures do not reach: the R = 8 and R = 32 forms of the product,
sizes one past a tile, restart cycles that converge, the breakdown exit, convergence at step 1, options other than the
default, and batches that mix all of these.  The yardstick is the numpy specification (tests/spectral_spec.py, held to the
reference in tests/test_spectral_spec.py); the bound on ``segment`` is its ``tolerance``: derived from the contract
|M v - lambda v| <= 1e-13 |lambda| and the specification's own residual, nothing from the engine's output."""
import sys
import warnings

import numpy as np
import pytest

import spectral_spec as S
from conftest import ROOT, ulp_diff_f32

sys.path.insert(0, ROOT)
from test_gpu_em_batch import assert_same, batch, single  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = S.cases()
AFFINITY_MAX = 600
RESIDENT = ("translation_257", "scale_2049", "scale_4097", "scale_8193")
BATCH = ("translation_65", "translation_257", "scale_2049", "translation_4097", "translation_8193", "disjoint_1000")
_BUILT, _RESULT = {}, {}
_WORST = {"ratio": 0.0, "case": None}


def rows_per_block(n):
    return 4 if n <= 2048 else 8 if n <= 4096 else 16 if n <= 8192 else 32


def built(name):
    """The case's inputs and the specification's answer, computed once per module."""
    if name not in _BUILT:
        case = next(c for c in CASES if c.name == name)
        _BUILT[name] = S.build(case, keep_matrix=case.n <= AFFINITY_MAX)
    b = _BUILT[name]
    assert b is not None, f"{name}: no seed met the conditions"
    return b


@pytest.fixture(scope="module")
def spectral(native):
    from cvx_proj_amd import spectral_method
    if native.lib().apap_device_count() < 1:
        pytest.skip("no HIP device")
    return spectral_method


def run(spectral, name):
    """spectral_weights (the host-buffer form) on the case, once per module; any warning is an error."""
    if name not in _RESULT:
        b = built(name)
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            _RESULT[name] = spectral.spectral_weights(b.src, b.dst, b.c, b.o, b.F, Hg=b.Hg, mask=None if b.case.use_hg else b.mask,
                                                      **b.opts.kw())
    return _RESULT[name]


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_against_the_specification(spectral, case):
    b = built(case.name)
    n, aff = case.n, case.opts.aff_thresh
    if n > 4100:        # the conditions of the larger cases (the smaller ones: tests/test_spectral_spec.py)
        assert S.conditions(case, b) == [] and b.gap >= 1e-3 and b.tol <= 1e-7
    r = run(spectral, case.name)
    err = float(np.abs(r.segment - b.segment).max())
    ratio = err / b.tol
    if ratio > _WORST["ratio"]:
        _WORST.update(ratio=ratio, case=case.name)
    e_steps, e_cycles, e_how = b.emulated
    print(f"{case.name}: n={n} R={rows_per_block(n)} seed={b.seed} steps={r.steps} restarts={r.restarts} (emulated: steps={e_steps} "
          f"cycles={e_cycles} {e_how}) residual={r.residual:.2e} gap={r.gap:.3g} (spec {b.gap:.3g}) |dlam|/|lam|="
          f"{abs(r.lam - b.lam) / abs(b.lam):.2e} segment err={err:.2e} tol={b.tol:.2e} ratio={ratio:.3g}; largest ratio so far "
          f"{_WORST['ratio']:.3g} ({_WORST['case']})")
    assert r.converged and r.residual <= 1e-13
    assert abs(r.lam - b.lam) <= 1e-12 * abs(b.lam)
    assert err <= b.tol
    assert np.array_equal(r.segment > aff, b.segment > aff)
    assert r.original_mask.dtype == np.float32 and r.original_mask.tobytes() == b.initial.tobytes()
    assert ulp_diff_f32(r.ransac_mask, b.ransac_mask).max() <= 1
    if case.family in ("scale", "disjoint"):
        assert r.restarts >= 2
    if case.family == "groups" and case.groups == 1:
        assert r.steps == 1


@pytest.mark.parametrize("case", [c for c in CASES if c.n <= AFFINITY_MAX], ids=repr)
def test_affinity_against_the_specification(spectral, native, case):
    b = built(case.name)
    M = native.spectral_affinity(b.src, b.dst, b.c, b.o, b.F, native.spectral_params(*b.opts.values()))
    d = np.diag(M).copy()
    off = M.copy()
    np.fill_diagonal(off, 0)
    differ = int(np.count_nonzero(d != b.diag))
    print(f"{case.name}: n={case.n} diagonal entries not bit-identical: {differ}, largest |difference| "
          f"{float((np.abs(d - b.diag) / np.spacing(np.abs(b.diag))).max()):.2f} ulp")
    assert np.array_equal(off.astype(np.float32).astype(np.float64), off)
    assert off.astype(np.float32).view(np.uint32).tobytes() == b.off.view(np.uint32).tobytes()
    assert (np.abs(d - b.diag) <= 4 * np.spacing(np.abs(b.diag))).all()


@pytest.mark.parametrize("name", RESIDENT)
def test_resident_form_gives_the_same_bytes(spectral, native, name):
    """The resident form enqueues all 30 cycles: after a convergence in a later cycle every remaining launch must return at
    once on the `done` word."""
    import torch
    from cvx_proj_amd import resident
    b = built(name)
    r = run(spectral, name)
    dev = torch.device("cuda", 0)

    def t(a, dt):
        return torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)

    status = torch.zeros(1, dtype=torch.int32, device=dev)
    seg, rm, om, info = resident.hip_spectral(
        t(b.src, np.float32), t(b.dst, np.float32), t(b.c, np.float32), t(b.o, np.float32), t(b.F, np.float64),
        native.spectral_params(*b.opts.values()), Hg=None, mask=t(b.mask, np.float32), status=status)
    torch.cuda.synchronize()
    info = info.cpu().numpy()
    print(f"{name}: resident steps={int(info[2])} restarts={int(info[4])}; host-buffer steps={r.steps} restarts={r.restarts}")
    assert int(status.cpu()[0]) == 0 and info[3] == 0
    assert seg.cpu().numpy().tobytes() == r.segment.tobytes()
    assert rm.cpu().numpy().tobytes() == r.ransac_mask.tobytes()
    assert om.cpu().numpy().tobytes() == r.original_mask.tobytes()
    assert np.float64(info[0]).tobytes() == np.float64(r.lam).tobytes()
    assert (int(info[2]), int(info[4])) == (r.steps, r.restarts)


def test_the_largest_case_twice_gives_the_same_bytes(spectral, native):
    b = built("scale_8193")
    params = native.spectral_params(*b.opts.values())
    first = native.spectral_weights(b.src, b.dst, b.c, b.o, b.F, params, mask=b.mask)
    second = native.spectral_weights(b.src, b.dst, b.c, b.o, b.F, params, mask=b.mask)
    for x, y in zip(first, second):
        assert x.dtype == y.dtype and x.tobytes() == y.tobytes()
    assert first[0].tobytes() == run(spectral, "scale_8193").segment.tobytes()


@pytest.fixture(scope="module")
def mixed(spectral, native):
    """Pairs of all four rows-per-block classes that need one, two and three cycles, each with the default options and the
    least-squares M-step; per problem its own single call."""
    pairs = []
    for name in BATCH:
        b = built(name)
        assert not b.case.use_hg and b.opts.values() == S.Opts().values()
        pairs.append((b.src, b.dst, b.c, b.o, b.F, b.mask))
    blocks = (native.spectral_params(), native.model_params(native.MODEL_LMS))
    want = [single(native, p, blocks[0], blocks[1], 1) for p in pairs]
    return pairs, blocks, want


def test_batch_of_every_class_and_cycle_count_equals_the_single_calls(spectral, native, mixed):
    pairs, blocks, want = mixed
    assert sorted({rows_per_block(len(p[0])) for p in pairs}) == [4, 8, 16, 32]
    problems = [(i, blocks) for i in range(len(pairs))]
    got, status = batch(native, pairs, problems, 1)
    cycles = []
    for i, name in enumerate(BATCH):
        out, word, raised = want[i]
        sinfo = got[i][5][0]
        cycles.append(int(sinfo[4]))
        print(f"batch of {len(BATCH)}: {name} n={len(pairs[i][0])} R={rows_per_block(len(pairs[i][0]))} steps={int(sinfo[2])} "
              f"restarts={int(sinfo[4])} status={int(status[i])} single={word} raised={raised}")
        assert_same(got[i], out, name)
        assert int(status[i]) == word, name
        # the round's calculate_M is the call the specification was held against
        assert got[i][2][0].tobytes() == run(spectral, name).segment.tobytes(), name
        assert (int(sinfo[2]), int(sinfo[4])) == (run(spectral, name).steps, run(spectral, name).restarts), name
    assert min(cycles) == 1 and 2 in cycles and max(cycles) >= 3, cycles
    perm = [4, 0, 5, 2, 1, 3]
    got_p, status_p = batch(native, [pairs[i] for i in perm], problems, 1)
    for at, i in enumerate(perm):
        assert_same(got_p[at], want[i][0], BATCH[i])
        assert int(status_p[at]) == want[i][1]


def test_batch_without_a_class_0_problem(spectral, native, mixed):
    pairs, blocks, want = mixed
    keep = [BATCH.index("scale_2049"), BATCH.index("translation_8193")]
    assert [rows_per_block(len(pairs[i][0])) for i in keep] == [8, 32]
    got, status = batch(native, [pairs[i] for i in keep], [(0, blocks), (1, blocks)], 1)
    for at, i in enumerate(keep):
        print(f"batch of 2: {BATCH[i]} steps={int(got[at][5][0][2])} restarts={int(got[at][5][0][4])}")
        assert_same(got[at], want[i][0], BATCH[i])
        assert int(status[at]) == want[i][1]
