"""K1's chunk staging through a range-checked buffer window (k_assemble_mfma): the rows behind a split's end must read as zero.

k_assemble_mfma stages every 64-keypoint chunk of its split through a raw buffer resource that covers the chunk's rows below the
split's end; the hardware's range check, and no compare in the kernel, makes the rows from there on zero.  Right behind a
split's end lie the next split's rows, or the next pair's table: a window one row too long, or a part of the offset that the
range check does not see, adds foreign rows to every sum.  Here those rows are made impossible to overlook: every table row
whose index is a multiple of 64 - the first row of every chunk, so of every split, and of every pair's table - holds sums 1e3
times the others'.

(a) bits: the SHA-256 of the whole moment workspace equals tests/golden/k1_staging_sha.npz, recorded by
    tests/golden/make_k1_staging_golden.py from the library of the commit BEFORE the buffer window, whose loader compared
    every row's index with the split's end.
(b) position: every sum of every cell against a numpy evaluation from the table rows of its own split, at the bar of
    tests/test_gpu_k1_slab_stores.py: REL = 1e-10 of sum_k w^2 |table[k, column]|, and for the float32 weight chain
    REL + max_k (6 |x_k| + 4) 2^-24, x = 2 log2(e) d / sigma^2 (include/apap_hip.h's bound for a normal float32 w^2).
(c) the 4096 bytes behind the workspace keep their pattern, and no sum is left as the pattern.

Shapes, the MFMA variant forced so that these sizes reach the kernel:
  rows per split   1, 3, 4, 63, 64, 65, 127, 128, 129, 250 keypoints in ONE split (want_waves = 1): a split shorter than one
                   4-keypoint step, a partial first and last chunk, a chunk boundary exactly at the split's end (64, 128: the
                   last whole chunk stages a window of no rows)
  splits           129 = 128 + 1, 150 = 128 + 22, 250 = 128 + 122 (two splits), 257 = 128 + 128 + 1, 320 = 128 + 128 + 64 (three):
                   the last split shorter than the others.  The plan makes every split a whole number of 64-keypoint chunks,
                   so no option places a split's first row off a chunk boundary: a window's base is always 16 KiB-aligned
                   relative to the table, and a base that is not cannot be reached through the library.
  batch            3 pairs with their own tables, two splits each (the 3-D grid)
  launches         the plain grid, and paired, levelled launches (plan_slots as in tests/test_gpu_k1_paired.py: 5 tiles x 1
                   split on 3 slots, 4 tiles x 2 splits on 5 slots, 4 tiles x 3 splits on 10 slots)
  blocks           vertices on a mesh 96 cells wide (every block shares the row term: threads 0 .. 127 fetch column 31 through
                   the same window) and arbitrary vertices (no whole tile shares); asserted on the host for every case
  cells            70, 129, 197, 320: no multiple of 64
for the 30-sum form, the 24-sum form and the 24-sum form with float32 weights, at both weightings of the other K1 tests.
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
BIG = 1e3
MESH_WIDTH = 96     # one and a half tiles: any tile, and any pair of tiles (2 j, 2 j + 1), lies on one or two rows
FORMS = {"m30": {}, "m24": {"moments": 24}, "m24-w32": {"moments": 24, "weights_f32": 1}}

# (cells, n, batch, plan_slots, want_waves, splits expected)
ROWS = [(70, n, 1, NO_PAIRS, 1, 1) for n in (1, 3, 4, 63, 64, 65, 127, 128, 129, 250)]
SPLITS = [(70, 129, 1, NO_PAIRS, 0, 2), (70, 150, 1, NO_PAIRS, 0, 2), (70, 250, 1, NO_PAIRS, 0, 2),
          (70, 257, 1, NO_PAIRS, 0, 3), (70, 320, 1, NO_PAIRS, 0, 3)]
BATCH = [(129, 150, 3, NO_PAIRS, 0, 2)]
PAIRED = [(320, 64, 1, 3, 0, 1),       # 5 tiles, one split: pairs (0, 1) and (2, 3), tile 4 single and levelled
          (197, 150, 1, 5, 0, 2),      # 4 tiles x 2 splits: two pairs in split 0, one in split 1
          (197, 257, 1, 10, 0, 3)]     # 4 tiles x 3 splits (128 + 128 + 1) on 10 slots: two pairs
CASES = ROWS + SPLITS + BATCH + PAIRED
VERTICES = ["mesh", "any"]


def case_id(case):
    cells, n, batch, slots, waves, _ = case
    return f"{cells}-{n}-b{batch}" + ("" if slots == NO_PAIRS else f"-s{slots}") + ("-1split" if waves else "")


def key(case, verts, form, gamma, sigma):
    return f"{case_id(case)}_{verts}_{form}_{gamma}_{sigma}"


def sha(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), dtype=np.uint8)


def vertices(cells, kind):
    """Mesh: rows of MESH_WIDTH cells, one y per row (a 64-cell tile, or a pair of tiles, then lies on few rows); any: random."""
    if kind == "mesh":
        k = np.arange(cells)
        return np.stack([(k % MESH_WIDTH) * 12.5 + 3.0, (k // MESH_WIDTH) * 37.0 + 11.0], axis=1).astype(np.float64)
    return np.random.default_rng(cells * 17 + 5).random((cells, 2)) * [640, 480]


def blocks_share(verts, cells_per_block):
    """The kernel's rule (apap_row_term.h), on bit patterns through cell_vertex's clamp: every cell's vy is the first cell's or
    the first other one's."""
    out = []
    for first in range(0, len(verts), cells_per_block):
        vy = verts[np.minimum(np.arange(first, first + cells_per_block), len(verts) - 1), 1].view(np.int64)
        other = vy[vy != vy[0]]
        out.append(bool(np.all((vy == vy[0]) | (vy == (other[0] if other.size else vy[0])))))
    return out


@functools.lru_cache(maxsize=None)
def inputs(cells, n, batch, kind):
    """Host and device tables (30 and 24 sums) of `batch` pairs with the sums of every 64th row BIG times as large, the
    denormalisations and the vertices; built once per shape and never written.  A table is its first n rows of a problem of
    at least 16 keypoints: the normalisation wants more than the 1, 3 or 4 rows that K1 is given here, and K1 sums whatever
    rows the table holds."""
    import torch
    from cvx_proj_amd import _native as native
    dev = torch.device("cuda:0")
    tabs, dens = {24: [], 30: []}, []
    for b in range(batch):
        p = synth_pair(640, 480, max(n, 16), 4, seed=9100 + 7 * b + n)
        q = native.host_prepare(p.src, p.dst)
        for m in (24, 30):
            t = np.array(native.host_build_table(p.src, q["cf1"], q["cf2"], moments=m))[:n]
            t[::64, :m] *= BIG      # the sums' columns; the coordinates (29 .. 31) and the 24-sum marker (28) stay
            tabs[m].append(t)
        dens.append(native.host_build_denorm(q["iC2"], q["C1"], q["iN2"], q["N1"]))
    verts = vertices(cells, kind)
    h_tab = {m: np.stack(t) for m, t in tabs.items()}
    return (h_tab, verts, {m: torch.from_numpy(t).to(dev) for m, t in h_tab.items()}, torch.from_numpy(np.stack(dens)).to(dev),
            torch.from_numpy(verts).to(dev))


@functools.lru_cache(maxsize=None)
def solve(case, kind, form, gamma, sigma):
    """(the workspace's bytes and the TAIL behind them, workspace bytes) of one solve; the buffer starts as FILL."""
    import torch
    from cvx_proj_amd import _native as native
    cells, n, batch, slots, waves, _ = case
    options = dict(FORMS[form])
    _, _, d_tab, d_den, d_vert = inputs(cells, n, batch, kind)
    ctx = native.Context(variant=native.VARIANT_MFMA, plan_slots=slots, **options)
    if waves:
        ctx.set("want_waves", waves)
    nbytes = native.lib().apap_solve_batch_workspace_bytes(native._h(ctx), n, cells, batch)
    work = torch.full((nbytes + TAIL,), FILL, dtype=torch.uint8, device="cuda:0")
    assert work.data_ptr() % 256 == 0
    H = torch.full((batch, cells, 9), float("nan"), dtype=torch.float32, device="cuda:0")
    native.check(native.lib().apap_solve_batch_device(native._h(ctx), d_tab[options.get("moments", 30)].data_ptr(), n,
                                                      d_vert.data_ptr(), 0, cells, gamma, sigma, d_den.data_ptr(), H.data_ptr(),
                                                      batch, work.data_ptr(), nbytes, ctypes.c_void_p(0)))
    torch.cuda.synchronize()
    ctx.close()
    return work.cpu().numpy(), nbytes


def layout(case, form, nbytes):
    """(sums per split, cells_pad, splits, keypoints per split) of the case's slab, from its size and the plan's rule (a
    split is a whole number of 64-keypoint chunks, none is empty)."""
    cells, n, batch, _, _, want = case
    sums = 24 if "moments" in FORMS[form] else 30
    cells_pad = (cells + 63) // 64 * 64
    splits, rest = divmod(nbytes, batch * sums * cells_pad * 8)
    assert rest == 0 and splits == want, f"workspace of {nbytes} bytes: {splits} splits, the case is meant to have {want}"
    parts = 1
    while not case[4] and parts < 32 and n // (parts * 2) >= 64:    # (these sizes never reach the rule's limit on waves)
        parts *= 2
    per_split = ((n + parts - 1) // parts + 63) // 64 * 64
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


def check_positions(case, kind, form, gamma, sigma):
    cells, n, batch, _, _, _ = case
    work, nbytes = solve(case, kind, form, gamma, sigma)
    sums, cells_pad, splits, per_split = layout(case, form, nbytes)
    slab = work[:nbytes].view(np.float64).reshape(batch, splits, sums, cells_pad)
    h_tab, verts, _, _, _ = inputs(cells, n, batch, kind)
    worst = 0.0
    for b in range(batch):
        for s in range(splits):
            rows = h_tab[sums][b, s * per_split:min(n, (s + 1) * per_split)]
            ref, scale, bound = reference(rows, verts, gamma, sigma, "weights_f32" in FORMS[form])
            err, bar = np.abs(slab[b, s, :, :cells] - ref[:sums]), bound * scale[:sums]
            worst = max(worst, float((err[bar > 0] / bar[bar > 0]).max()))
            bad = np.argwhere(~(err <= bar))
            assert bad.size == 0, (f"{key(case, kind, form, gamma, sigma)} pair {b} split {s}: {len(bad)} sums off, the first at "
                                   f"column {bad[0][0]} cell {bad[0][1]}: {slab[b, s, bad[0][0], bad[0][1]]!r} against "
                                   f"{ref[bad[0][0], bad[0][1]]!r}")
    return worst


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_the_blocks_take_the_paths_the_cases_are_meant_for(case):
    """Mesh vertices: every tile, and every pair of tiles a paired launch forms, shares the row term; arbitrary ones: no whole
    tile or pair (a last tile of one cell has one vy and shares)."""
    cells = case[0]
    for width in (64, 128):
        assert all(blocks_share(vertices(cells, "mesh"), width)), (cells, width)
        assert not any(blocks_share(vertices(cells, "any"), width)[:cells // width]), (cells, width)


@pytest.mark.parametrize("kind", VERTICES)
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_the_workspace_has_the_bits_of_the_compared_loader(native, golden, case, kind):
    g = golden("k1_staging_sha")
    wrong = []
    for form in FORMS:
        for gamma, sigma in WEIGHTINGS:
            work, nbytes = solve(case, kind, form, gamma, sigma)
            k = key(case, kind, form, gamma, sigma)
            if not np.array_equal(sha(work[:nbytes]), g[k]):
                wrong.append(f"{k}: the workspace's SHA-256 differs from the recorded one")
    assert not wrong, "; ".join(wrong)


@pytest.mark.parametrize("kind", VERTICES)
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_every_sum_holds_its_own_split_and_nothing_behind_it(native, case, kind):
    for form in FORMS:
        for gamma, sigma in WEIGHTINGS:
            worst = check_positions(case, kind, form, gamma, sigma)
            print(f"{key(case, kind, form, gamma, sigma)}: largest error {worst:.2e} of the bar")


@pytest.mark.parametrize("kind", VERTICES)
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_nothing_but_the_sums_is_written(native, case, kind):
    for form in FORMS:
        for gamma, sigma in WEIGHTINGS:
            work, nbytes = solve(case, kind, form, gamma, sigma)
            k = key(case, kind, form, gamma, sigma)
            assert work.size == nbytes + TAIL and (work[nbytes:] == FILL).all(), f"{k}: the bytes behind the workspace were written"
            left = np.flatnonzero(work[:nbytes].view(np.uint64) == np.uint64(0xA5A5A5A5A5A5A5A5))
            assert left.size == 0, f"{k}: {left.size} sums were never written, the first at index {left[0]}"
            assert np.isfinite(work[:nbytes].view(np.float64)).all(), f"{k}: a sum is not finite"
