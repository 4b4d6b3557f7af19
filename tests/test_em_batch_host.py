"""The batched EM loop without a GPU: the C ABI's three symbols, the workspace size, every argument refusal (before any
device is touched), the Python wrappers' checks and the order of the grid."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT

SYMBOLS = ("apap_spectral_em_batch_workspace_bytes", "apap_spectral_em_batch_device", "apap_spectral_em_batch")


def i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def ip(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_int))


def ws(native, lengths, pair_of):
    off = i32(np.concatenate([[0], np.cumsum(lengths)]))
    po = i32(pair_of)
    return native.lib().apap_spectral_em_batch_workspace_bytes(ip(off), len(lengths), ip(po), len(po))


def test_symbols_are_exported_and_bound(native):
    for sym in SYMBOLS:
        assert sym in native.SIGNATURES and hasattr(native.lib(), sym)
    assert native.lib().apap_abi_version() == native.ABI_VERSION == 6     # additive: the ABI generation stays


def test_workspace_size(native):
    lib = native.lib()
    off, po = i32([0, 5]), i32([0])
    assert lib.apap_spectral_em_batch_workspace_bytes(None, 1, ip(po), 1) == 0
    assert lib.apap_spectral_em_batch_workspace_bytes(ip(off), 1, None, 1) == 0
    assert lib.apap_spectral_em_batch_workspace_bytes(ip(off), 0, ip(po), 1) == 0
    assert lib.apap_spectral_em_batch_workspace_bytes(ip(off), 1, ip(po), 0) == 0
    assert lib.apap_spectral_em_batch_workspace_bytes(ip(i32([0, 0])), 1, ip(po), 1) == 0     # an empty pair
    assert lib.apap_spectral_em_batch_workspace_bytes(ip(off), 1, ip(i32([1])), 1) == 0       # pair out of range
    lengths = [1, 7, 300, 2000, 5000]
    one = [ws(native, lengths, [p]) for p in range(len(lengths))]
    for n, b in zip(lengths, one):
        assert b > 0 and b % 256 == 0
        # a problem's slice: the single-problem spectral and model layouts plus a fixed header (descriptor, list entry, state)
        fixed = b - lib.apap_spectral_workspace_bytes(n) - lib.apap_model_workspace_bytes(n)
        assert fixed == one[0] - lib.apap_spectral_workspace_bytes(1) - lib.apap_model_workspace_bytes(1)
        assert 0 < fixed <= 2048 and fixed % 256 == 0
    # additive over problems, whatever the order and however often a pair is used
    assert ws(native, lengths, [0, 1, 2, 3, 4]) == sum(one)
    assert ws(native, lengths, [4, 4, 0, 2]) == 2 * one[4] + one[0] + one[2]
    # linear in n: 512 n bytes of basis plus well under 200 n bytes of the rest
    big = [ws(native, [n], [0]) for n in (1 << 16, 1 << 17, 1 << 18)]
    # up to the 256-byte rounding of the parts and the M-step's block factors, which are bounded (at most 1024 of them)
    model_cap = 1024 * 15 * 15 * 8 + 8192
    assert abs((big[2] - big[1]) - 2 * (big[1] - big[0])) <= 3 * model_cap + 64 * 256
    assert 556 * (1 << 16) <= big[1] - big[0] <= 700 * (1 << 16)     # 556 = basis 512 + diag, W, Y 24 + points 16 + mask 4


def call_device(native, off, n_pairs, pair_of, sp, mp, n_problems, em_steps, data=None, work=None, work_bytes=0):
    """apap_spectral_em_batch_device with fake (never dereferenced) or null data pointers."""
    d = ctypes.c_void_p(data)
    f64 = native._f64p
    return native.lib().apap_spectral_em_batch_device(
        None, d, d, d, d, d, d, None if off is None else ip(off), n_pairs, None if pair_of is None else ip(pair_of),
        None if sp is None else sp.ctypes.data_as(f64), None if mp is None else mp.ctypes.data_as(f64), n_problems, em_steps, d, d,
        d, d, d, d, None, ctypes.c_void_p(work), work_bytes, None)


def good(native, problems=2):
    off, po = i32([0, 5, 12]), i32([0, 1][:problems] if problems <= 2 else [0, 1] * (problems // 2))
    sp = np.stack([native.spectral_params()] * len(po))
    mp = np.stack([native.model_params(native.MODEL_SDP, 0.5, 0.5)] * len(po))
    return off, po, sp, mp


def test_argument_errors_before_any_device(native):
    """Every refusal comes from host checks: the data pointers here are null or fake, so a call that went further would
    fault.  The order: shape of the batch, em_steps, per-problem parameters, null data pointers, workspace."""
    E, W = native.ERR_INVALID_ARG, native.ERR_WORKSPACE
    off, po, sp, mp = good(native)
    fake, work = 4096, 1 << 20
    assert call_device(native, None, 2, po, sp, mp, 2, 2, fake, work, 1 << 30) == E
    assert call_device(native, off, 2, None, sp, mp, 2, 2, fake, work, 1 << 30) == E
    assert call_device(native, off, 2, po, None, mp, 2, 2, fake, work, 1 << 30) == E
    assert call_device(native, off, 2, po, sp, None, 2, 2, fake, work, 1 << 30) == E
    assert call_device(native, off, 0, po, sp, mp, 2, 2, fake, work, 1 << 30) == E
    assert call_device(native, off, 2, po, sp, mp, 0, 2, fake, work, 1 << 30) == E
    assert call_device(native, off, 2, i32([0, 2]), sp, mp, 2, 2, fake, work, 1 << 30) == E
    assert b"problem 1: pair 2 out of range" in native.lib().apap_last_error()
    assert call_device(native, off, 2, i32([-1, 0]), sp, mp, 2, 2, fake, work, 1 << 30) == E
    for bad_off in ([0, 5, 5], [0, 5, 3], [-1, 5, 12]):
        assert call_device(native, i32(bad_off), 2, po, sp, mp, 2, 2, fake, work, 1 << 30) == E
    for steps in (0, -1, 65):
        assert call_device(native, off, 2, po, sp, mp, 2, steps, fake, work, 1 << 30) == E
        assert b"em_steps" in native.lib().apap_last_error()
    bad = mp.copy()
    bad[1, 0] = 3           # neither LMS nor SDP
    assert call_device(native, off, 2, po, sp, bad, 2, 2) == E
    assert b"problem 1" in native.lib().apap_last_error()
    bad = sp.copy()
    bad[1, 5] = -1          # max_restarts
    assert call_device(native, off, 2, po, bad, mp, 2, 2) == E
    assert b"problem 1" in native.lib().apap_last_error()
    mixed = sp.copy()
    mixed[1, 5] = 7         # 30 (the default) against 7
    assert call_device(native, off, 2, po, mixed, mp, 2, 2) == E
    assert b"max_restarts" in native.lib().apap_last_error()
    mixed[0, 5] = 7         # equal again
    assert call_device(native, off, 2, po, mixed, mp, 2, 2) == E      # now only the null data pointers are wrong
    assert b"null device pointer" in native.lib().apap_last_error()
    need = ws(native, [5, 7], [0, 1])
    assert call_device(native, off, 2, po, sp, mp, 2, 2, fake, work, need - 1) == W
    assert call_device(native, off, 2, po, sp, mp, 2, 2, fake, 0, need) == E             # null workspace
    assert call_device(native, off, 2, po, sp, mp, 2, 2, fake, work + 128, need) == E    # misaligned workspace
    assert b"256-byte" in native.lib().apap_last_error()


def pair(n, seed=0):
    rng = np.random.default_rng(seed)
    src = (rng.random((n, 2)) * 900).astype(np.float32)
    return src, src + np.float32(3), rng.random((n, 128), dtype=np.float32), rng.random((n, 128), dtype=np.float32), np.eye(3), \
        np.ones(n, np.float32)


def test_refuses_without_a_device_after_the_argument_checks(native):
    src, dst, c, o, F, mask = pair(6)
    sp = native.spectral_params()[None]
    mp = native.model_params(native.MODEL_SDP, 0.5, 0.5)[None]
    bad = mp.copy()
    bad[0, 0] = 3
    with pytest.raises(native.ApapValueError, match="problem 0"):      # with or without a GPU: the checks come first
        native.spectral_em_batch(src, dst, c, o, F[None], mask, [6], [0], sp, bad, 2)
    with pytest.raises(native.ApapValueError, match="null argument"):
        native.check(native.lib().apap_spectral_em_batch(None, None, None, None, None, None, None, None, 1, None, None, None, 1, 1,
                                                         None, None, None, None, None, None, None, -1))
    if native.lib().apap_device_count() > 0:
        return      # the rest needs a machine without a GPU
    with pytest.raises(native.ApapError) as e:
        native.spectral_em_batch(src, dst, c, o, F[None], mask, [6], [0], sp, mp, 2)
    assert e.value.code == native.ERR_NO_DEVICE
    from cvx_proj_amd import spectral_method
    with pytest.raises(native.ApapError) as e:
        spectral_method.spectral_em_batch([(src, dst, c, o, F, mask)], [(0, {})])
    assert e.value.code == native.ERR_NO_DEVICE


def test_python_wrappers_reject_bad_input(native):
    from cvx_proj_amd import spectral_method as sm
    src, dst, c, o, F, mask = pair(6)
    sp = native.spectral_params()[None]
    mp = native.model_params(native.MODEL_LMS)[None]
    with pytest.raises(ValueError):     # points of the wrong shape
        native.spectral_em_batch(src[:5], dst, c, o, F[None], mask, [6], [0], sp, mp, 2)
    with pytest.raises(ValueError):     # descriptors
        native.spectral_em_batch(src, dst, c[:, :64], o, F[None], mask, [6], [0], sp, mp, 2)
    with pytest.raises(ValueError):     # one F per pair
        native.spectral_em_batch(src, dst, c, o, F, mask, [6], [0], sp, mp, 2)
    with pytest.raises(ValueError):     # mask
        native.spectral_em_batch(src, dst, c, o, F[None], mask[:3], [6], [0], sp, mp, 2)
    with pytest.raises(ValueError):     # parameter blocks per problem
        native.spectral_em_batch(src, dst, c, o, F[None], mask, [6], [0, 0], sp, mp, 2)
    with pytest.raises(ValueError):     # pair index
        native.spectral_em_batch(src, dst, c, o, F[None], mask, [6], [1], sp, mp, 2)
    with pytest.raises(ValueError):     # a float is no pair index
        native.spectral_em_batch(src, dst, c, o, F[None], mask, [6], [0.0], sp, mp, 2)
    with pytest.raises(ValueError):     # em_steps
        native.spectral_em_batch(src, dst, c, o, F[None], mask, [6], [0], sp, mp, 65)
    with pytest.raises(ValueError, match="max_restarts"):
        native.spectral_em_batch(src, dst, c, o, F[None], mask, [6], [0, 0], np.stack([native.spectral_params(max_restarts=3),
                                 native.spectral_params(max_restarts=4)]), np.stack([mp[0], mp[0]]), 2)
    p = (src, dst, c, o, F, mask)
    with pytest.raises(ValueError, match="pair_index"):
        sm.spectral_em_batch([p], [(1, {})])
    with pytest.raises(ValueError, match="pair_index"):
        sm.spectral_em_batch([p], [(-1, {})])
    with pytest.raises(ValueError, match="max_restarts"):
        sm.spectral_em_batch([p], [(0, {"max_restarts": 3}), (0, {"max_restarts": 4})])
    with pytest.raises(TypeError, match="unknown"):
        sm.spectral_em_batch([p], [(0, {"aff_tresh": 0.5})])
    with pytest.raises(ValueError):
        sm.spectral_em_batch([p], [])
    with pytest.raises(ValueError):
        sm.spectral_em_batch([(src, dst, c, o, F, mask[:2])], [(0, {})])
    with pytest.raises(ValueError):
        sm.spectral_em_batch([(src.astype(np.float64)[:, :1], dst, c, o, F, mask)], [(0, {})])
    with pytest.raises(NotImplementedError, match="Huber"):
        sm.spectral_em_batch([p], [(0, {"lms": True, "huber_param": 0.5})])


def test_grid_is_the_cartesian_product_in_the_scripts_order(native, monkeypatch):
    """grid_search.sh nests affinity_eps, aff_thresh, epi_weight, fluc (outermost first); the grid mapping's own order does
    not matter."""
    from cvx_proj_amd import spectral_method as sm
    seen = {}

    def fake(pairs, problems, **kw):
        seen["pairs"], seen["problems"], seen["kw"] = pairs, problems, kw
        return [("result", i) for i in range(len(problems))]
    monkeypatch.setattr(sm, "spectral_em_batch", fake)
    grid = {"fluc": [0.8, 1.0, 1.25], "epi_weight": [0.25, 0.5, 0.75], "aff_thresh": [0.6, 0.7, 0.8],
            "affinity_eps": [20, 22.5, 25, 27.5]}
    p = pair(6)
    options, results = sm.spectral_em_grid(p, grid, em_radius=5, score_thresh=0.5, em_steps=1, device=0)
    want = [dict(em_radius=5, score_thresh=0.5, affinity_eps=a, aff_thresh=t, epi_weight=e, fluc=f)
            for a in grid["affinity_eps"] for t in grid["aff_thresh"] for e in grid["epi_weight"] for f in grid["fluc"]]
    assert len(options) == 108 and options == want
    assert results == [("result", i) for i in range(108)]
    assert seen["kw"] == {"em_steps": 1, "device": 0}
    assert len(seen["pairs"]) == 1 and seen["pairs"][0] is p
    assert seen["problems"] == [(0, o) for o in want]
    with pytest.raises(TypeError):
        sm.spectral_em_grid(p, grid, fluc=0.5)
    with pytest.raises(ValueError):
        sm.spectral_em_grid(p, {"fluc": []})


def test_the_new_source_follows_the_library_conventions():
    """No environment variable, no mutable global (tests/test_capi_symbols.py scans csrc/ too), and none of the constructs
    the file header rules out: floating-point atomics, grid-wide barriers, spin-waits."""
    csrc = os.path.join(ROOT, "cvx_proj_amd", "csrc")
    assert "apap_em_batch.hip" in open(os.path.join(csrc, "Makefile")).read()
    for f in ("apap_em_batch.hip", "apap_spectral_dev.h", "apap_model_dev.h"):
        text = open(os.path.join(csrc, f)).read()
        assert "getenv" not in text, f
        assert not re.search(r"^\s*(static\s+)?(int|bool)\s+g_\w+\s*=", text, flags=re.M), f
        assert not re.search(r"atomicAdd|cooperative_groups|grid\.sync|while\s*\(\s*!?\s*\*?\s*\(?volatile", text), f


def test_no_launch_sits_in_a_loop_over_problems():
    """The launch count cannot grow with B: in the batch run every launch comes after the descriptor upload, in loops over
    rounds, restart cycles, Lanczos steps and (unrolled) the four rows-per-block classes; the only loop over problems there
    reads the `done` words the host-buffer form has copied back."""
    text = open(os.path.join(ROOT, "cvx_proj_amd", "csrc", "apap_em_batch.hip")).read()
    run = text[text.index("int spectral_em_batch_run("):text.index("}  // namespace apap")]
    head, tail = run.split("hipStream_t s = (hipStream_t)stream;")
    assert "hipLaunchKernelGGL" not in head and "launch_matvec" not in head
    assert tail.count("hipLaunchKernelGGL") == 8 and tail.count("launch_matvec<") == 4
    over_problems = [line for line in tail.splitlines() if re.search(r"for \(int b\b", line)]
    assert len(over_problems) == 1 and "states[b].done" in over_problems[0]
    assert set(re.findall(r"for \(int (\w+) = 0; \1 < (\w+)", tail)) == {("k", "em_steps"), ("c", "restarts"), ("j", "max_m"), ("b", "B")}
