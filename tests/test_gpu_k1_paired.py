"""K1's paired launch against its plain launch, bit for bit.

A single pair whose J = tiles x splits blocks are more than the S blocks the device keeps resident, and fewer than 2 S, is
launched as S blocks of which J - S carry two 64-cell tiles of one keypoint split (k_assemble_mfma, plan_pairs).  Cells are
independent and every accumulator receives the same MFMAs in the same order, so the pairing may not move one bit.
APAP_OPT_PLAN_SLOTS sets S: every case here is solved once with the S that forces the pairing under test and once with an S so
large that nothing pairs, through apap_solve_batch_device with the MFMA variant forced (no fused small-mesh launch), and

(a) the WHOLE moment slab - the workspace bytes: every float64 sum of every split, the padded cells included - is equal byte
    for byte (the float32 grid alone would hide a reordered sum);
(b) the grid H is equal byte for byte;

at the benchmark's weighting (gamma = 0.5, sigma = 100) and at gamma = 0.01, sigma = 8, where the weights span many orders of
magnitude and any reordering of a sum shows.  The workspace is pre-filled with a pattern, so a block that wrote to the wrong
place, or not at all, shows too.
"""
import ctypes
import functools

import numpy as np
import pytest

from cvx_proj_amd.synth import synth_pair

pytestmark = pytest.mark.gpu

WEIGHTINGS = [(0.5, 100.0), (0.01, 8.0)]
NO_PAIRS = 1 << 30
FILL = 0xA5

# (cells, n, slots): what the pairing does there
CASES = [
    (165, 150, 4),      # 3 tiles (the last of 37 cells) x 2 splits of 128 and 22 keypoints (6 steps, zero rows): one pair per split
    (197, 150, 5),      # 4 tiles (the last of 5 cells: second of a pair) x 2 splits: three pairs, two in split 0 and one in split 1
    (130, 40, 2),       # 3 tiles (the last of 2 cells), one split without a full chunk: one pair
    (165, 64, 2),       # exactly one chunk
    (165, 65, 2),       # one chunk and one keypoint
    (320, 64, 3),       # 5 tiles, one split: pairs (0, 1) and (2, 3), tile 4 single (J = 2 S - 1: all but one block paired)
]
# the edges of the rule, batch = 1: J = 8 blocks (197 cells, 150 keypoints) or J = 5 (320 cells, 64 keypoints)
EDGES = [
    (197, 150, 8),      # J = S: no pair
    (197, 150, 4),      # J = 2 S: no pair
    (197, 150, 7),      # J = S + 1: one pair
    (320, 64, 4),       # J = S + 1, odd tile count
    (320, 64, 5),       # J = S
]


@functools.lru_cache(maxsize=None)
def inputs(cells, n, batch):
    """Device tables (30 and 24 sums), denormalisations and vertices of `batch` pairs, built once per shape and never written."""
    import torch
    from cvx_proj_amd import _native as native
    dev = torch.device("cuda:0")
    tabs, dens = {24: [], 30: []}, []
    for b in range(batch):
        p = synth_pair(640, 480, n, 4, seed=4100 + b + n)
        q = native.host_prepare(p.src, p.dst)
        for m in (24, 30):
            tabs[m].append(native.host_build_table(p.src, q["cf1"], q["cf2"], moments=m))
        dens.append(native.host_build_denorm(q["iC2"], q["C1"], q["iN2"], q["N1"]))
    verts = np.random.default_rng(cells * 11 + n).random((cells, 2)) * [640, 480]
    return ({m: torch.from_numpy(np.stack(t)).to(dev) for m, t in tabs.items()}, torch.from_numpy(np.stack(dens)).to(dev),
            torch.from_numpy(verts).to(dev))


def solve(native, cells, n, batch, slots, gamma, sigma, **options):
    """(workspace bytes after the solve, H) with APAP_OPT_PLAN_SLOTS = slots; the workspace starts as FILL."""
    import torch
    d_tab, d_den, d_vert = inputs(cells, n, batch)
    ctx = native.Context(variant=native.VARIANT_MFMA, plan_slots=slots, **options)
    nbytes = native.lib().apap_solve_batch_workspace_bytes(native._h(ctx), n, cells, batch)
    work = torch.full((nbytes,), FILL, dtype=torch.uint8, device="cuda:0")
    H = torch.full((batch, cells, 9), float("nan"), dtype=torch.float32, device="cuda:0")
    native.check(native.lib().apap_solve_batch_device(native._h(ctx), d_tab[options.get("moments", 30)].data_ptr(), n, d_vert.data_ptr(),
                                                      0, cells, gamma, sigma, d_den.data_ptr(), H.data_ptr(), batch, work.data_ptr(),
                                                      nbytes, ctypes.c_void_p(0)))
    torch.cuda.synchronize()
    ctx.close()
    return work.cpu().numpy(), H.cpu().numpy()


def same_bits(native, cells, n, slots, batch=1, **options):
    for gamma, sigma in WEIGHTINGS:
        slab_p, H_p = solve(native, cells, n, batch, slots, gamma, sigma, **options)
        slab_1, H_1 = solve(native, cells, n, batch, NO_PAIRS, gamma, sigma, **options)
        where = f"cells={cells} n={n} batch={batch} slots={slots} gamma={gamma} sigma={sigma} {options}"
        assert slab_p.size == slab_1.size and slab_p.size % 8 == 0
        sums = slab_1.view(np.float64)
        assert np.isfinite(sums).all() and not (slab_1 == FILL).all(), f"{where}: the plain launch left no sums"
        diff = np.flatnonzero(slab_p.view(np.uint64) != slab_1.view(np.uint64))
        assert diff.size == 0, f"{where}: {diff.size} of {sums.size} float64 sums differ, the first at index {diff[0]}"
        assert np.array_equal(H_p.view(np.uint32), H_1.view(np.uint32)), f"{where}: the grids differ"


@pytest.mark.parametrize("cells,n,slots", CASES)
def test_paired_tiles_leave_every_sum_as_it_was(native, cells, n, slots):
    same_bits(native, cells, n, slots)


@pytest.mark.parametrize("options", [{"moments": 24}, {"moments": 24, "weights_f32": 1}], ids=["m24", "m24-w32"])
def test_paired_tiles_in_the_24_sum_forms(native, options):
    same_bits(native, 165, 150, 4, **options)


@pytest.mark.parametrize("cells,n,slots", EDGES)
def test_edges_of_the_pairing_rule(native, cells, n, slots):
    same_bits(native, cells, n, slots)


def test_a_batch_is_never_paired(native):
    """batch = 2 with few slots: the 3-D grid (a 1-D paired grid would leave the second pair's slabs and grid unwritten)."""
    same_bits(native, 197, 150, 2, batch=2)
    same_bits(native, 197, 150, 5, batch=2)


def test_plan_slots_moves_neither_workspace_nor_splits(native):
    lib = native.lib()
    ctx = native.Context(variant=native.VARIANT_MFMA)
    shapes = [(150, 165, 1), (150, 197, 2), (2000, 40000, 1), (64, 320, 1), (5000, 20000, 1)]
    before = [lib.apap_solve_batch_workspace_bytes(native._h(ctx), n, cells, batch) for n, cells, batch in shapes]
    assert before[0] == 2 * 30 * 192 * 8 and before[2] == 2 * 30 * 40000 * 8       # two keypoint splits each
    for slots in (1, 2, 5, 1024, NO_PAIRS):
        ctx.set("plan_slots", slots)
        assert ctx.get("plan_slots") == slots
        assert [lib.apap_solve_batch_workspace_bytes(native._h(ctx), n, cells, batch) for n, cells, batch in shapes] == before
    ctx.set("plan_slots", 0)
    assert ctx.get("plan_slots") == 0
    with pytest.raises(native.ApapError):
        ctx.set("plan_slots", -1)
    assert ctx.get("plan_slots") == 0
    ctx.close()
