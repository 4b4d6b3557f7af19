"""The M-step family's outputs, pinned across commits.

The other byte tests of the M-step compare the entry forms of one build with each other; this file compares a build with
tests/golden/model_digests.json, the SHA-256 digests recorded on an MI355X by tests/golden/make_model_digests_golden.py from
the build of the commit before the M-step kernels' shared steps (the Huber row walk, the selection rule, the float32 tail,
the serial Cholesky solve, phi_M) were given one definition each.  A digest covers H, all 24 info doubles and the status
word of one solve.  The shapes are the smallest that reach every line of those steps: one fold and many folds of M1, one
wave and several waves of the Huber walk (matches_T +- 1), the floor (empty_fold), degenerate input (n3, collinear) and the
iteration cap (cap_1), all from tests/huber_cases.py.
"""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN
import huber_cases

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(GOLDEN, "model_digests.json")
SDP_SETS = ((1.0, 1.0), (0.5, 2.0))          # (du, dv)
SIGMA, SMALL_GAMMA = 12.0, 1e-4              # tests/test_gpu_local_model.py's
EM_FIXTURE = "spectral_n500"                 # tests/test_gpu_model.py's EM fixture
EM_STEPS = 2


@pytest.fixture(scope="module")
def native_gpu(native):
    if native.lib().apap_device_count() < 1:
        pytest.skip("no HIP device")
    return native


def sha(*parts):
    h = hashlib.sha256()
    for p in parts:
        h.update(np.ascontiguousarray(p).tobytes())
    return h.hexdigest()


def model_digests(native, mode):
    """apap_model_solve on every case of huber_cases.cases(), swap 0 and 1: the raw entry point, so that a degenerate case
    hands back its outputs and its return code instead of an exception."""
    out = {}
    for name, c in huber_cases.cases().items():
        pc, po, w = (np.ascontiguousarray(c[k], np.float32) for k in ("pc", "po", "w"))
        if mode == "huber":
            sets = [("", native.MODEL_HUBER, c["M"], 1.0, c["cap"])]
        elif mode == "lms":
            sets = [("", native.MODEL_LMS, 1.0, 1.0, 0)]
        else:
            sets = [(f" du={du} dv={dv}", native.MODEL_SDP, du, dv, 0) for du, dv in SDP_SETS]
        for label, m, du, dv, cap in sets:
            for swap in (False, True):
                params = native.model_params(m, du, dv, floor=c["floor"], swap=swap, max_iter=cap)
                H = np.full((3, 3), np.nan, np.float32)
                info = np.full(native.MODEL_INFO, np.nan)
                code = native.lib().apap_model_solve(None, native._ptr(pc, C.c_float), native._ptr(po, C.c_float),
                                                     native._ptr(w, C.c_float), len(pc), native._ptr(params, C.c_double),
                                                     native._ptr(H, C.c_float), native._ptr(info, C.c_double), -1)
                out[f"model {mode} {name}{label} swap={int(swap)}"] = sha(H, info, np.int32(code))
    return out


def local_digests(native, mode):
    """apap_local_model_solve on clean_500 over a 3 x 2 grid of vertices of its 4K frame, with and without match weights."""
    c = huber_cases.cases()["clean_500"]
    v = np.stack(np.meshgrid(np.float64([640.37, 1920.37, 3200.37]), np.float64([539.79, 1619.79])), axis=-1)      # (2, 3, 2)
    params = native.model_params(native.MODEL_LMS) if mode == "lms" else native.model_params(native.MODEL_SDP, 0.5, 0.5)
    out = {}
    for label, mw in (("weights", c["w"]), ("no weights", None)):
        H, info, status = native.local_model_solve(c["pc"], c["po"], v, SMALL_GAMMA, SIGMA, params, match_weights=mw)
        for k in range(6):
            i, j = divmod(k, 3)
            out[f"local {mode} {label} cell {k}"] = sha(H[i, j], info[i, j], status[i, j])
    return out


def em_pair():
    g = dict(np.load(os.path.join(GOLDEN, EM_FIXTURE + ".npz")))
    e, a, t, r, s = (float(x) for x in g["opts"])
    opts = dict(epi_weight=e, affinity_eps=a, aff_thresh=t, em_radius=r, score_thresh=s)
    return (g["src"], g["dst"], g["c_feats"].astype(np.float32), g["o_feats"].astype(np.float32), g["F"], g["mask"]), opts


def em_model_params(native, mode):
    if mode == "huber":
        return native.model_params(native.MODEL_HUBER, 0.5)
    return native.model_params(native.MODEL_LMS) if mode == "lms" else native.model_params(native.MODEL_SDP, 0.5, 0.5)


def em_digests(native, mode):
    pair, opts = em_pair()
    try:
        out = native.spectral_em(*pair[:5], native.spectral_params(**opts), em_model_params(native, mode), EM_STEPS, pair[5])
    except native.ApapError as e:      # a status bit turned into an exception: the outputs are on it
        out = e.info
    return {f"em {mode} round {k}": sha(out[0][k], out[1][k], np.int32(out[1][k][native.MODEL_INFO_STATUS])) for k in range(EM_STEPS)}


def batch_digests(native, mode):
    """One apap_spectral_em_batch of three problems of the EM fixture: SDP, LMS, SDP with du != dv."""
    pair, opts = em_pair()
    sp = native.spectral_params(**opts)
    mps = [native.model_params(native.MODEL_SDP, 0.5, 0.5), native.model_params(native.MODEL_LMS),
           native.model_params(native.MODEL_SDP, 0.5, 2.0)]
    H, info, _, _, _, _, status = native.spectral_em_batch(pair[0], pair[1], pair[2], pair[3], pair[4][None], pair[5], [len(pair[0])],
                                                           [0, 0, 0], np.stack([sp] * 3), np.stack(mps), EM_STEPS)
    return {f"batch problem {b} round {k}": sha(H[b, k], info[b, k], status[b]) for b in range(3) for k in range(EM_STEPS)}


GROUPS = [(model_digests, "huber"), (model_digests, "lms"), (model_digests, "sdp"), (local_digests, "lms"), (local_digests, "sdp"),
          (em_digests, "huber"), (em_digests, "lms"), (em_digests, "sdp"), (batch_digests, "lms+sdp")]


@pytest.mark.parametrize("fn,mode", GROUPS, ids=[f"{fn.__name__}-{mode}" for fn, mode in GROUPS])
def test_outputs_equal_the_recorded_digests(native_gpu, fn, mode):
    with open(FIXTURE) as f:
        want = json.load(f)
    got = fn(native_gpu, mode)
    assert got and set(got) <= set(want), sorted(set(got) - set(want))
    differ = sorted(k for k in got if got[k] != want[k])
    assert not differ, f"{len(differ)} of {len(got)} digests differ: {differ}"


def test_the_fixture_holds_no_other_entry():
    """Every recorded digest belongs to one of the groups above (counted without a solve: 27 cases x 2 swaps x (1 + 1 + 2)
    modes, 2 x 2 x 6 cells, 3 x 2 and 3 x 2 rounds)."""
    with open(FIXTURE) as f:
        want = json.load(f)
    assert len(huber_cases.cases()) == 27
    assert len(want) == 27 * 2 * 4 + 24 + 6 + 6, len(want)
