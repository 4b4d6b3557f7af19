"""The moment slab as k_assemble_mfma leaves it: every sum in its place, every bit as before, nothing else touched.

K1's MFMA kernel turns a wave's D registers round in LDS and writes the slab ([split][column][cells_pad] float64) in whole
128-byte lines.  The paired-against-plain test compares two launches of one build and would not see a mistake both share, so
the references here come from outside the build:

(a) position: every sum of every cell below `cells` against a numpy evaluation from the table, the vertices, gamma and sigma:
    sum over the split's keypoints of w^2 table[k, column], w^2 = max(exp(-2 d / sigma^2), gamma^2).  A sum in the wrong column,
    cell, split or pair is off by its whole size; the bar is REL = 1e-10 of sum_k w^2 |table[k, column]|, the size of the terms
    (the only scale the rounding of a float64 sum knows: a column whose terms cancel has no digits relative to its own value).
    The float32 weight chain reads float32 coordinates (the table's column 29) and rounds its weights to float32: its reference
    is evaluated from those coordinates, and its bar is REL + max_k (6 |x_k| + 4) 2^-24, x = 2 log2(e) d / sigma^2, the bound
    that include/apap_hip.h states for a normal float32 w^2 (oracle/weight_spec.py, rel_bound_f32, without the coordinates'
    rounding, which the reference shares).
(b) bits: the SHA-256 of the whole workspace, and of the grid, equals tests/golden/k1_slab_stores_sha.npz, recorded by
    tests/golden/make_k1_slab_stores_golden.py from the library of the commit BEFORE the whole-line epilogue.
(c) sentinels: the workspace is allocated 4096 bytes longer than apap_solve_batch_workspace_bytes says, filled with a byte
    pattern and passed with its exact size: the tail is untouched, no sum is left as the pattern, every sum is finite.

Shapes: cells 1 .. 197 around the 16-cell group and the 64-cell tile (197: a last tile of 5 cells), keypoints 5, 64, 65 and 150
(150: a partial last chunk, no barrier behind it) in one and in two splits, two paired launches (an odd tile left over; pairs in
both splits), a batch of 2, at both weightings of tests/test_gpu_k1_paired.py, for the 30-sum form, the 24-sum form and the
24-sum form with float32 weights; a case on K2's careful path and a 24-sum table given to a 30-sum context (a NaN grid).
The MFMA variant is forced: small meshes otherwise take the fused launch, which has no slab.
"""
import ctypes
import functools
import hashlib

import numpy as np
import pytest

from cvx_proj_amd.synth import synth_pair

pytestmark = pytest.mark.gpu

REL = 1e-10
WEIGHTINGS = [(0.5, 100.0), (0.01, 8.0)]
NO_PAIRS = 1 << 30
FILL = 0xA5
TAIL = 4096
FORMS = {"m30": {}, "m24": {"moments": 24}, "m24-w32": {"moments": 24, "weights_f32": 1}}

CELLS = [1, 15, 16, 17, 63, 64, 65, 129, 197]
KEYPOINTS = [5, 64, 65, 150]
# (cells, n, batch, plan_slots, want_waves): want_waves = 1 keeps the 150 keypoints in ONE split (two chunks and 22 keypoints),
# 0 leaves the plan alone (150: two splits of 128 and 22; fewer than 128: one split)
CASES = ([(c, n, 1, NO_PAIRS, 0) for c in CELLS for n in KEYPOINTS] +
         [(c, 150, 1, NO_PAIRS, 1) for c in CELLS] +
         [(320, 64, 1, 3, 0),          # 5 tiles, one split: pairs (0, 1) and (2, 3), tile 4 single and levelled
          (197, 150, 1, 5, 0),         # 4 tiles x 2 splits: two pairs in split 0, one in split 1; the second of a pair holds 5 cells
          (129, 150, 2, NO_PAIRS, 0)])  # a batch of 2 (the 3-D grid)
CAREFUL = (65, 65, 1, NO_PAIRS, 0)      # gamma = 0, sigma = 3, 30 sums: K2 re-solves cells from float64 weights
WRONG_TABLE = (65, 65, 1, NO_PAIRS, 0)  # a 24-sum table given to a 30-sum context: K2 refuses it, the grid is NaN


def case_id(case):
    cells, n, batch, slots, waves = case
    return f"{cells}-{n}-b{batch}" + ("" if slots == NO_PAIRS else f"-s{slots}") + ("-1split" if waves else "")


def key(case, form, gamma, sigma, table=None):
    return f"{case_id(case)}_{form}_{gamma}_{sigma}" + (f"_table{table}" if table else "")


def sha(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def inputs(cells, n, batch):
    """Host and device tables (30 and 24 sums), denormalisations and vertices of `batch` pairs, built once per shape and
    never written."""
    import torch
    from cvx_proj_amd import _native as native
    dev = torch.device("cuda:0")
    tabs, dens = {24: [], 30: []}, []
    for b in range(batch):
        p = synth_pair(640, 480, n, 4, seed=7300 + b + n)
        q = native.host_prepare(p.src, p.dst)
        for m in (24, 30):
            tabs[m].append(native.host_build_table(p.src, q["cf1"], q["cf2"], moments=m))
        dens.append(native.host_build_denorm(q["iC2"], q["C1"], q["iN2"], q["N1"]))
    verts = np.random.default_rng(cells * 13 + n).random((cells, 2)) * [640, 480]
    h_tab = {m: np.stack(t) for m, t in tabs.items()}
    return (h_tab, verts, {m: torch.from_numpy(t).to(dev) for m, t in h_tab.items()}, torch.from_numpy(np.stack(dens)).to(dev),
            torch.from_numpy(verts).to(dev))


@functools.lru_cache(maxsize=None)
def solve(case, form, gamma, sigma, table=None):
    """(the workspace's bytes and the TAIL behind them, H, workspace bytes) of one solve; the buffer starts as FILL.  `table`:
    the moments of the table passed, where it is not the form's own."""
    import torch
    from cvx_proj_amd import _native as native
    cells, n, batch, slots, waves = case
    options = dict(FORMS[form])
    _, _, d_tab, d_den, d_vert = inputs(cells, n, batch)
    ctx = native.Context(variant=native.VARIANT_MFMA, plan_slots=slots, **options)
    if waves:
        ctx.set("want_waves", waves)
    nbytes = native.lib().apap_solve_batch_workspace_bytes(native._h(ctx), n, cells, batch)
    work = torch.full((nbytes + TAIL,), FILL, dtype=torch.uint8, device="cuda:0")
    assert work.data_ptr() % 256 == 0
    H = torch.full((batch, cells, 9), float("nan"), dtype=torch.float32, device="cuda:0")
    native.check(native.lib().apap_solve_batch_device(native._h(ctx), d_tab[table or options.get("moments", 30)].data_ptr(), n,
                                                      d_vert.data_ptr(), 0, cells, gamma, sigma, d_den.data_ptr(), H.data_ptr(),
                                                      batch, work.data_ptr(), nbytes, ctypes.c_void_p(0)))
    torch.cuda.synchronize()
    ctx.close()
    return work.cpu().numpy(), H.cpu().numpy(), nbytes


def layout(case, form, nbytes):
    """(sums per split, cells_pad, splits, keypoints per split) of the case's slab, from its size and the plan's rule (a
    split is a whole number of 64-keypoint chunks, none is empty)."""
    cells, n, batch, _, waves = case
    sums = 24 if "moments" in FORMS[form] else 30
    cells_pad = (cells + 63) // 64 * 64
    splits, rest = divmod(nbytes, batch * sums * cells_pad * 8)
    assert rest == 0 and splits in (1, 2), f"workspace of {nbytes} bytes: {splits} splits?"
    per_split = ((n + splits - 1) // splits + 63) // 64 * 64
    assert (n + per_split - 1) // per_split == splits
    return sums, cells_pad, splits, per_split


def reference(table, verts, gamma, sigma, f32):
    """(sum_k w^2 table[k, c], sum_k w^2 |table[k, c]|, the chain's relative bound) per (column, cell), keypoints = the rows
    of `table`."""
    if f32:
        xy = np.ascontiguousarray(table[:, 29]).view(np.float32).reshape(-1, 2).astype(np.float64)
        v = verts.astype(np.float32).astype(np.float64)
        g2 = float(np.float32(gamma * gamma))
    else:
        xy, v, g2 = table[:, 30:32], verts, gamma * gamma
    d = np.sqrt((v[:, None, 0] - xy[None, :, 0]) ** 2 + (v[:, None, 1] - xy[None, :, 1]) ** 2)      # cells x keypoints
    u = 2.0 * d / (sigma * sigma)
    w2 = np.maximum(np.exp(-u), g2)
    bound = REL + ((6.0 * u.max() * 1.4426950408889634 + 4.0) * 2.0 ** -24 if f32 else 0.0)
    return table.T @ w2.T, np.abs(table).T @ w2.T, bound


def check_positions(case, form, gamma, sigma):
    cells, n, batch, _, _ = case
    work, _, nbytes = solve(case, form, gamma, sigma)
    sums, cells_pad, splits, per_split = layout(case, form, nbytes)
    slab = work[:nbytes].view(np.float64).reshape(batch, splits, sums, cells_pad)
    h_tab, verts, _, _, _ = inputs(cells, n, batch)
    worst = 0.0
    for b in range(batch):
        for s in range(splits):
            rows = h_tab[sums][b, s * per_split:min(n, (s + 1) * per_split)]
            ref, scale, bound = reference(rows, verts, gamma, sigma, "weights_f32" in FORMS[form])
            err, bar = np.abs(slab[b, s, :, :cells] - ref[:sums]), bound * scale[:sums]
            worst = max(worst, float((err[bar > 0] / bar[bar > 0]).max()))
            bad = np.argwhere(~(err <= bar))
            assert bad.size == 0, (f"{key(case, form, gamma, sigma)} pair {b} split {s}: {len(bad)} sums off, the first at column "
                                   f"{bad[0][0]} cell {bad[0][1]}: {slab[b, s, bad[0][0], bad[0][1]]!r} against {ref[bad[0][0], bad[0][1]]!r}")
    return worst


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_every_sum_is_in_its_place(native, case):
    for form in FORMS:
        for gamma, sigma in WEIGHTINGS:
            worst = check_positions(case, form, gamma, sigma)
            print(f"{key(case, form, gamma, sigma)}: largest error {worst:.2e} of the bar")


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_the_slab_has_the_bits_of_the_earlier_epilogue(native, golden, case):
    g = golden("k1_slab_stores_sha")
    wrong = []
    for form in FORMS:
        for gamma, sigma in WEIGHTINGS:
            work, H, nbytes = solve(case, form, gamma, sigma)
            k = key(case, form, gamma, sigma)
            if not np.array_equal(sha(work[:nbytes]), g[k + "_work"]):
                wrong.append(f"{k}: the workspace's SHA-256 differs from the recorded one")
            if not np.array_equal(sha(H), g[k + "_H"]):
                wrong.append(f"{k}: the grid's SHA-256 differs from the recorded one")
    assert not wrong, "; ".join(wrong)


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_nothing_but_the_sums_is_written(native, case):
    for form in FORMS:
        for gamma, sigma in WEIGHTINGS:
            work, H, nbytes = solve(case, form, gamma, sigma)
            k = key(case, form, gamma, sigma)
            assert work.size == nbytes + TAIL and (work[nbytes:] == FILL).all(), f"{k}: the bytes behind the workspace were written"
            sums = work[:nbytes].view(np.float64)
            # every column of every split belongs to the form, padded cells included: no sum may be left as the pattern
            left = np.flatnonzero(work[:nbytes].view(np.uint64) == np.uint64(0xA5A5A5A5A5A5A5A5))
            assert left.size == 0, f"{k}: {left.size} of {sums.size} sums were never written, the first at index {left[0]}"
            assert np.isfinite(sums).all(), f"{k}: {int((~np.isfinite(sums)).sum())} sums are not finite"
            assert np.isfinite(H).all(), f"{k}: the grid is not finite"


def test_a_case_on_the_careful_path(native, golden):
    """gamma = 0, sigma = 3: weights down to e^-177, K2 re-solves the cells whose trace is below its floor."""
    g = golden("k1_slab_stores_sha")
    gamma, sigma = 0.0, 3.0
    work, H, nbytes = solve(CAREFUL, "m30", gamma, sigma)
    k = key(CAREFUL, "m30", gamma, sigma)
    print(f"{k}: largest error {check_positions(CAREFUL, 'm30', gamma, sigma):.2e} of the bar")
    assert (work[nbytes:] == FILL).all() and np.isfinite(work[:nbytes].view(np.float64)).all() and np.isfinite(H).all()
    assert np.array_equal(sha(work[:nbytes]), g[k + "_work"]), "the workspace's SHA-256 differs from the recorded one"
    assert np.array_equal(sha(H), g[k + "_H"]), "the grid's SHA-256 differs from the recorded one"


def test_a_24_sum_table_given_to_a_30_sum_context(native, golden):
    """K1 sums whatever the table holds (its marker column is NaN) and K2 refuses the layout: a NaN grid, the same bits."""
    g = golden("k1_slab_stores_sha")
    gamma, sigma = WEIGHTINGS[0]
    work, H, nbytes = solve(WRONG_TABLE, "m30", gamma, sigma, 24)
    k = key(WRONG_TABLE, "m30", gamma, sigma, 24)
    assert (work[nbytes:] == FILL).all() and np.isnan(H).all()
    assert not (work[:nbytes].view(np.uint64) == np.uint64(0xA5A5A5A5A5A5A5A5)).any()
    assert np.array_equal(sha(work[:nbytes]), g[k + "_work"]), "the workspace's SHA-256 differs from the recorded one"
    assert np.array_equal(sha(H), g[k + "_H"]), "the grid's SHA-256 differs from the recorded one"
