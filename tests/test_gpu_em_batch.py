"""The batched EM loop on the MI355X.  The yardstick in every case is the single-problem path (``_native.spectral_em``, one
call per problem): every output of every problem of a batch equals it byte for byte, whatever else is in the batch."""
import glob
import itertools
import os
import sys
import warnings

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

sys.path.insert(0, ROOT)
from tools.spectral_rate import synth  # noqa: E402

pytestmark = pytest.mark.gpu

NAMES = ("H", "model info", "segment", "ransac_mask", "original_mask", "spectral info")
# n = 1, 2, 7, 40, 48, 300, 500, 2000, 5000
RAGGED = ("spectral_n1", "spectral_n2", "spectral_n7", "spectral_disjoint", "spectral_negative", "spectral_clusters", "spectral_n500",
          "spectral_n2000", "spectral_n5000")


@pytest.fixture(scope="module")
def native_gpu(native):
    if native.lib().apap_device_count() < 1:
        pytest.skip("no HIP device")
    return native


def load(name):
    g = dict(np.load(os.path.join(GOLDEN, name + ".npz")))
    if "codebook" in g:     # the largest case stores its descriptors as rows of a codebook
        g["c_feats"], g["o_feats"] = g["codebook"][g["c_index"]], g["codebook"][g["o_index"]]
    mask = g["mask"] if "mask" in g else g["original_mask"]
    e, a, t, r, s = (float(x) for x in g["opts"])
    opts = dict(epi_weight=e, affinity_eps=a, aff_thresh=t, em_radius=r, score_thresh=s)
    if name == "spectral_negative":
        # this fixture's descriptors are anti-correlated by construction (make_golden_spectral.py: o = -c + noise), so every
        # match_score is near -1 and the later rounds' recompute_matching (`feat_score > score_thresh`) would keep no match
        # under any threshold a cosine can reach.  A threshold below -1 leaves the distance test alone to select: the pair's
        # geometry (dst = 3 src) is an exact homography, so the EM rounds then have matches to work on.
        opts["score_thresh"] = -2.0
    return (g["src"], g["dst"], g["c_feats"].astype(np.float32), g["o_feats"].astype(np.float32), g["F"], mask.astype(np.float32)), opts


def blocks(native, opts):
    """(spectral params, model params) of one option dict, as spectral_method builds them."""
    o = dict(opts)
    lms, fluc = o.pop("lms", False), o.pop("fluc", 0.5)
    mp = native.model_params(native.MODEL_LMS) if lms else native.model_params(native.MODEL_SDP, fluc, fluc)
    return native.spectral_params(**o), mp


def single(native, pair, sp, mp, em_steps):
    """The single call's six outputs and its status word (the bits of every round's two info blocks); `raised` when the
    host-buffer call turned the status into an exception (its .info then holds the outputs)."""
    raised = False
    try:
        out = native.spectral_em(*pair[:5], sp, mp, em_steps, pair[5])
    except native.ApapValueError as e:
        out, raised = e.info, True
    word = 0
    for k in range(em_steps):
        word |= int(out[5][k][3]) | int(out[1][k][native.MODEL_INFO_STATUS])
    return out, word, raised


def batch(native, pairs, problems, em_steps):
    """_native.spectral_em_batch on (pair index, (sp, mp)) problems: per problem the six outputs, and the status words."""
    H, info, seg, rm, om, sinfo, status = native.spectral_em_batch(
        np.concatenate([p[0] for p in pairs]), np.concatenate([p[1] for p in pairs]), np.concatenate([p[2] for p in pairs]),
        np.concatenate([p[3] for p in pairs]), np.stack([p[4] for p in pairs]), np.concatenate([p[5] for p in pairs]),
        [len(p[0]) for p in pairs], [i for i, _ in problems], np.stack([b[0] for _, b in problems]),
        np.stack([b[1] for _, b in problems]), em_steps)
    return [(H[b], info[b], seg[b], rm[b], om[b], sinfo[b]) for b in range(len(problems))], status


def assert_same(got, want, what):
    for name, a, b in zip(NAMES, got, want):
        assert a.shape == b.shape and a.dtype == b.dtype, (what, name, a.shape, b.shape)
        assert a.tobytes() == b.tobytes(), (what, name)


@pytest.fixture(scope="module")
def ragged(native_gpu):
    native = native_gpu
    pairs, problems, labels = [], [], []
    for name in RAGGED:
        pair, opts = load(name)
        pairs.append(pair)
        for extra in (dict(fluc=0.5), dict(lms=True)):
            problems.append((len(pairs) - 1, blocks(native, {**opts, **extra})))
            labels.append(f"{name} {'lms' if 'lms' in extra else 'sdp'}")
    pairs.append(synth(3000, seed=7))      # rows-per-block class 8, between the fixtures' 4 and 16
    for extra in (dict(fluc=0.5), dict(lms=True)):
        problems.append((len(pairs) - 1, blocks(native, extra)))
        labels.append(f"synthetic n3000 {'lms' if 'lms' in extra else 'sdp'}")
    return pairs, problems, labels


def test_ragged_batch_equals_the_single_calls(native_gpu, ragged):
    native = native_gpu
    pairs, problems, labels = ragged
    assert sorted(len(p[0]) for p in pairs) == [1, 2, 7, 40, 48, 300, 500, 2000, 3000, 5000]
    inputs = [[a.copy() for a in p] for p in pairs]
    got, status = batch(native, pairs, problems, 3)
    assert status.shape == (len(problems),) and status.dtype == np.int32
    for b, (idx, (sp, mp)) in enumerate(problems):
        want, word, raised = single(native, pairs[idx], sp, mp, 3)
        n = len(pairs[idx][0])
        print(f"{labels[b]}: n={n} status batch={int(status[b])} single={word} raised={raised} "
              f"selected={[int(want[1][k][native.MODEL_INFO_COUNT]) for k in range(3)]}")
        assert_same(got[b], want, labels[b])
        assert int(status[b]) == word, labels[b]
        if n <= 2:
            assert raised and word & native.STATUS_MODEL_DEGENERATE, labels[b]
            assert np.isnan(got[b][0]).all(), labels[b]
        else:
            assert not raised and not int(status[b]) & native.STATUS_MODEL_DEGENERATE, labels[b]
    for p, q in zip(pairs, inputs):
        for a, c in zip(p, q):
            assert a.tobytes() == c.tobytes()


def test_permuting_the_problems_permutes_the_outputs(native_gpu, ragged):
    native = native_gpu
    pairs, problems, labels = ragged
    got, status = batch(native, pairs, problems, 2)
    perm = np.random.default_rng(3).permutation(len(problems))
    got_p, status_p = batch(native, pairs, [problems[i] for i in perm], 2)
    for at, i in enumerate(perm):
        assert_same(got_p[at], got[i], labels[i])
        assert status_p[at] == status[i]
    # the pairs permuted as well: the concatenation order is no input of a problem
    order = list(reversed(range(len(pairs))))
    got_r, status_r = batch(native, [pairs[i] for i in order], [(order.index(idx), blk) for idx, blk in problems], 2)
    for b in range(len(problems)):
        assert_same(got_r[b], got[b], labels[b])
    assert status_r.tobytes() == status.tobytes()


def test_the_same_batch_twice_gives_the_same_bytes(native_gpu, ragged):
    native = native_gpu
    pairs, problems, labels = ragged
    a, sa = batch(native, pairs, problems, 2)
    b, sb = batch(native, pairs, problems, 2)
    for x, y, label in zip(a, b, labels):
        assert_same(x, y, label)
    assert sa.tobytes() == sb.tobytes()


@pytest.mark.parametrize("name", ["spectral_n500", "spectral_n2", "spectral_n5000"])
def test_batch_of_one_equals_the_single_call(native_gpu, name):
    native = native_gpu
    pair, opts = load(name)
    sp, mp = blocks(native, {**opts, "fluc": 0.5})
    got, status = batch(native, [pair], [(0, (sp, mp))], 2)
    want, word, _ = single(native, pair, sp, mp, 2)
    assert_same(got[0], want, name)
    assert int(status[0]) == word


def test_unequal_fluctuations_in_one_batch(native_gpu):
    """du != dv and its exchange next to du = dv on one pair (blocks() passes one value for both): each problem equals its
    own single call."""
    native = native_gpu
    pair, opts = load("spectral_n500")
    sp = native.spectral_params(**opts)
    sets = [(0.5, 0.5), (0.2, 1.25), (1.25, 0.2)]
    problems = [(0, (sp, native.model_params(native.MODEL_SDP, du, dv))) for du, dv in sets]
    got, status = batch(native, [pair], problems, 2)
    for b, (du, dv) in enumerate(sets):
        want, word, raised = single(native, pair, sp, problems[b][1][1], 2)
        assert not raised
        assert_same(got[b], want, (du, dv))
        assert int(status[b]) == word, (du, dv)
    assert got[1][0].tobytes() != got[2][0].tobytes()       # the exchange is another problem, and is routed as one


GRID = {"affinity_eps": [20, 22.5, 25, 27.5], "aff_thresh": [0.6, 0.7, 0.8], "epi_weight": [0.25, 0.5, 0.75], "fluc": [0.8, 1.0, 1.25]}


def test_the_reference_grid_equals_108_single_calls(native_gpu):
    """grid_search.sh's 4 x 3 x 3 x 3 parameter sets (em_radius 5, score_thresh 0.5, em_steps 1) on one pair, through
    spectral_em_grid, against 108 spectral_em calls in the script's order."""
    from cvx_proj_amd import spectral_method as SM
    pair, _ = load("spectral_n500")
    before = [a.copy() for a in pair]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        options, results = SM.spectral_em_grid(pair, GRID, em_radius=5, score_thresh=0.5, em_steps=1)
        assert len(options) == len(results) == 108
        order = list(itertools.product(GRID["affinity_eps"], GRID["aff_thresh"], GRID["epi_weight"], GRID["fluc"]))
        for i, (a, t, e, f) in enumerate(order):
            assert options[i] == dict(em_radius=5, score_thresh=0.5, affinity_eps=a, aff_thresh=t, epi_weight=e, fluc=f)
            want = SM.spectral_em(*pair[:5], em_steps=1, mask=pair[5], em_radius=5, score_thresh=0.5, affinity_eps=a, aff_thresh=t,
                                  epi_weight=e, fluc=f)
            got = results[i]
            assert len(got.rounds) == 1
            g, w = got.rounds[0], want.rounds[0]
            assert g.H_pred.tobytes() == w.H_pred.tobytes(), i
            assert got.H_save.tobytes() == want.H_save.tobytes(), i
            for field in ("segment", "ransac_mask", "original_mask"):
                assert getattr(g.spectral, field).tobytes() == getattr(w.spectral, field).tobytes(), (i, field)
            # lam, gap, steps, restarts, residual, converged
            assert np.array(g.spectral[4:], np.float64).tobytes() == np.array(w.spectral[4:], np.float64).tobytes(), i
            assert g.spectral.H is None and w.spectral.H is None
            for x, y in zip(g.model, w.model):
                assert np.asarray(x).tobytes() == np.asarray(y).tobytes(), i
    for a, b in zip(pair, before):
        assert a.tobytes() == b.tobytes()


def test_resident_form_equals_the_host_buffer_form(native_gpu, ragged):
    import torch
    from cvx_proj_amd import resident
    native = native_gpu
    pairs, problems, labels = ragged
    got, status = batch(native, pairs, problems, 2)
    dev = torch.device("cuda", 0)
    cat = lambda i, dt: torch.from_numpy(np.ascontiguousarray(np.concatenate([p[i] for p in pairs]), dtype=dt)).to(dev)  # noqa: E731
    lengths = [len(p[0]) for p in pairs]
    out = resident.hip_spectral_em_batch(cat(0, np.float32), cat(1, np.float32), cat(2, np.float32), cat(3, np.float32),
                                         torch.from_numpy(np.stack([p[4] for p in pairs])).to(dev), cat(5, np.float32), lengths,
                                         [i for i, _ in problems], np.stack([b[0] for _, b in problems]),
                                         np.stack([b[1] for _, b in problems]), 2)
    torch.cuda.synchronize()
    H, info, seg, rm, om, sinfo, st = (t.cpu().numpy() for t in out)
    assert st.shape == (len(problems),) and st.dtype == np.int32     # one word per problem
    assert st.tobytes() == status.tobytes()
    per = [lengths[i] for i, _ in problems]
    seg, rm, om = (native.em_batch_split(x, per, 2) for x in (seg, rm, om))
    for b, label in enumerate(labels):
        assert_same((H[b], info[b], seg[b], rm[b], om[b], sinfo[b]), got[b], label)


def test_launch_count_does_not_depend_on_the_batch_size(native_gpu):
    """Timing-free: the context's profiling scope brackets each round's spectral launches once, whatever B; that no launch
    sits in a loop over problems is checked on the source (tests/test_em_batch_host.py), and profiles/em_batch_kernel_stats.txt
    records the dispatch counts of a B = 108 call."""
    native = native_gpu
    pair, opts = load("spectral_n500")
    counts = []
    for B in (1, 8, 27):
        ctx = native.Context(profile=1)
        problems = [(0, blocks(native, {**opts, "fluc": 0.5 + 0.01 * b})) for b in range(B)]
        H, info, seg, rm, om, sinfo, status = native.spectral_em_batch(
            pair[0], pair[1], pair[2], pair[3], pair[4][None], pair[5], [len(pair[0])], [0] * B, np.stack([b[0] for _, b in problems]),
            np.stack([b[1] for _, b in problems]), 2, ctx=ctx)
        counts.append(ctx.profile_read()["spectral"][1])
        ctx.close()
    assert counts == [2, 2, 2], counts
