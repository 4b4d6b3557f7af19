"""K1's shared row term against the loop that forms it in every lane, bit for bit.

A block of k_assemble_mfma (float64 weights) whose cells hold at most two distinct vy - A, its first cell's, and B, the first
other one in cell order - computes fma(dy, dy, 1e-300), dy = vy - sy, once per keypoint and value into a side table in LDS and
its lanes read it there; every other block runs the loop as it has always been (cvx_proj_amd/csrc/apap_row_term.h).  A cell's
sums do not depend on the block that computed them, and that is the lever: every problem here is solved once with its cells in
MESH order, where the blocks share the term, and once with the same cells PERMUTED so that every block holds three or more
distinct vy and takes the old loop.  After undoing the permutation every real cell's 30 (or 24) sums in every split of the
workspace, and its H, must be byte-equal (numpy.array_equal on the raw bytes: the special values include NaN).

Which path a block takes is decided on the host by `shares`, the rule of the kernel, and asserted for every case before
anything is launched: the expectations below are part of the test, not commentary.

ROWS, 677 cells = 10 tiles of 64 and one of 37 (values a .. k stand for 11 different vy):
  tile  0  a x 64            no change (A == B)                        shares
  tile  1  a x 64            no change                                 shares; pair (0, 1): no change, shares
  tile  2  b x 40, c x 24    change inside a 16-cell group             shares
  tile  3  c x 64                                                      shares; pair (2, 3): b, c: shares
  tile  4  d x 32, e x 32    change exactly at a wave's boundary       shares
  tile  5  e x 64                                                      shares; pair (4, 5): d, e: shares
  tile  6  f x 64
  tile  7  g x 64            pair (6, 7): change exactly at the tile boundary of the paired block: shares
  tile  8  h x 30, i x 34    rows {h, i}                               shares
  tile  9  i x 20, j x 44    rows {i, j}                               shares; pair (8, 9) touches THREE rows: the old loop
  tile 10  j x 10, k x 27    the last tile, an overhang of 27 lanes that repeat the last cell (k)   shares
  permuted (cells dealt out in proportion over the 11 values): every tile and every pair holds >= 3 values: the old loop
Launch forms, through plan_slots as tests/test_gpu_k1_paired.py does it (11 tiles x 2 splits of 128 + 22 keypoints = 22 units):
  slots = 12: ten pairs, tiles (0, 1) .. (8, 9) of both splits in the paired body, tile 10 in the levelled single body
  slots = 21: one pair, (0, 1) of split 0; every other unit in the levelled single body
  slots = 2^30: nothing paired, the plain 3-D grid; so is batch = 3 (a batch is never paired)
Keypoint counts on the plain grid: n = 5 (2 steps, the second with three zero rows whose y is taken as 0), 63, 64 (exactly one
chunk), 65, 150 in ONE split (want_waves = 1: two chunks and 22 keypoints, 6 steps, two zero rows) and 150 over two splits.
24 sums with float64 weights take the same two paths; 24 sums with float32 weights never share (the unchanged control: both
orders run the one float32 loop).

NONMONO, 197 cells: tile 0 = a x 20, b x 20, a x 24 (A, B, A: shares); tile 1 = a x 20, c x 20, b x 24 (A, C, B: the old
loop); tile 2 = d x 30, e x 34 (shares); tile 3 = 5 cells of e (shares); permuted: the old loop in tiles 0 .. 2, and tile 3's
five cells hold three values too.
SPECIAL, 256 cells: tile 0 = +0.0 x 32, -0.0 x 32 (two values by their bits, one by their size: shares, A = +0.0, B = -0.0);
tile 1 = v x 32, nextafter(v) x 32 (one ulp apart: shares); tile 2 = NaN x 32, inf x 32 (shares); tile 3 = +0.0 x 20,
-0.0 x 20, 1.0 x 24 (three values by their bits: the old loop, although a float compare would see two); permuted: the old loop.

The H of the ROWS problem in mesh order (every block shares) is also compared with the VALU kernel's, which never shares.
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

V = 37.25
ROW_VALUES = {c: 20.0 + 43.0 * i for i, c in enumerate("abcdefghijk")}
SPECIAL_VALUES = {"p": 0.0, "m": -0.0, "v": V, "w": float(np.nextafter(V, 1e9)), "N": float("nan"), "I": float("inf"), "1": 1.0}
LAYOUTS = {
    # name: (runs of (value, cells) in mesh order, values, which tiles share, which pairs (2 j, 2 j + 1) share)
    "rows": ([("a", 128), ("b", 40), ("c", 88), ("d", 32), ("e", 96), ("f", 64), ("g", 64), ("h", 30), ("i", 54), ("j", 54), ("k", 27)],
             ROW_VALUES, [True] * 11, [True, True, True, True, False]),
    "nonmono": ([("a", 20), ("b", 20), ("a", 24), ("a", 20), ("c", 20), ("b", 24), ("d", 30), ("e", 39)],
                ROW_VALUES, [True, False, True, True], [False, True]),
    "special": ([("p", 32), ("m", 32), ("v", 32), ("w", 32), ("N", 32), ("I", 32), ("p", 20), ("m", 20), ("1", 24)],
                SPECIAL_VALUES, [True, True, True, False], [False, False]),
}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def shares(vy_block, width):
    """The kernel's rule for a block of `width` lanes over these cells' vy (the lanes past the last cell repeat it)."""
    b = bits(vy_block)
    b = np.concatenate([b, np.repeat(b[-1:], width - b.size)])
    other = b[b != b[0]]
    second = other[0] if other.size else b[0]
    return bool(((b == b[0]) | (b == second)).all())


def block_paths(vy, width):
    return [shares(vy[i:i + width], width) for i in range(0, vy.size, width)]


@functools.lru_cache(maxsize=None)
def layout(name):
    """(vertices in mesh order, permutation P: position k of the permuted problem holds mesh cell P[k]); never written."""
    runs, values, tiles_share, pairs_share = LAYOUTS[name]
    vy = np.concatenate([np.full(count, values[v]) for v, count in runs])
    cells = vy.size
    vx = np.random.default_rng(cells).random(cells) * 640.0
    verts = np.stack([vx, vy], axis=1)
    # deal the cells out in proportion over the distinct values (by their bits)
    _, group = np.unique(bits(vy), return_inverse=True)
    key = np.empty(cells)
    for g in range(group.max() + 1):
        idx = np.flatnonzero(group == g)
        key[idx] = (np.arange(idx.size) + 0.5) / idx.size
    P = np.lexsort((group, key))
    assert sorted(P.tolist()) == list(range(cells))
    # the paths, by construction
    tiles = (cells + 63) // 64
    paired = tiles // 2 * 128           # the cells of the tile pairs (2 j, 2 j + 1); an odd last tile is never paired
    assert block_paths(vy, 64) == tiles_share, (name, block_paths(vy, 64))
    assert block_paths(vy[:paired], 128) == pairs_share, (name, block_paths(vy[:paired], 128))
    assert not any(block_paths(vy[P], 64)) and not any(block_paths(vy[P][:paired], 128)), name
    verts.setflags(write=False)
    P.setflags(write=False)
    return verts, P


@functools.lru_cache(maxsize=None)
def tables(n, batch):
    """Device tables (30 and 24 sums) and denormalisations of `batch` pairs, built once per shape and never written."""
    import torch
    from cvx_proj_amd import _native as native
    tabs, dens = {24: [], 30: []}, []
    for b in range(batch):
        p = synth_pair(640, 480, n, 4, seed=5200 + b + n)
        q = native.host_prepare(p.src, p.dst)
        for m in (24, 30):
            tabs[m].append(native.host_build_table(p.src, q["cf1"], q["cf2"], moments=m))
        dens.append(native.host_build_denorm(q["iC2"], q["C1"], q["iN2"], q["N1"]))
    dev = torch.device("cuda:0")
    return {m: torch.from_numpy(np.stack(t)).to(dev) for m, t in tabs.items()}, torch.from_numpy(np.stack(dens)).to(dev)


def solve(native, verts, n, batch, gamma, sigma, **options):
    """(slabs [batch][splits][sums][cells_pad] as uint64, H [batch][cells][9] as uint32); the workspace starts as FILL."""
    import torch
    d_tab, d_den = tables(n, batch)
    d_vert = torch.from_numpy(np.array(verts)).to("cuda:0")       # (a copy: the layouts are read-only)
    cells = verts.shape[0]
    options.setdefault("variant", native.VARIANT_MFMA)
    ctx = native.Context(**options)
    nbytes = native.lib().apap_solve_batch_workspace_bytes(native._h(ctx), n, cells, batch)
    work = torch.full((nbytes,), FILL, dtype=torch.uint8, device="cuda:0")
    H = torch.full((batch, cells, 9), float("nan"), dtype=torch.float32, device="cuda:0")
    sums = options.get("moments", 30)
    native.check(native.lib().apap_solve_batch_device(native._h(ctx), d_tab[sums].data_ptr(), n, d_vert.data_ptr(), 0, cells, gamma,
                                                      sigma, d_den.data_ptr(), H.data_ptr(), batch, work.data_ptr(), nbytes,
                                                      ctypes.c_void_p(0)))
    torch.cuda.synchronize()
    ctx.close()
    cells_pad = (cells + 63) // 64 * 64
    per_split = sums * cells_pad * 8
    assert nbytes % (batch * per_split) == 0, (nbytes, batch, per_split)
    slabs = work.cpu().numpy().view(np.uint64).reshape(batch, nbytes // (batch * per_split), sums, cells_pad)
    return slabs, H.cpu().numpy().view(np.uint32)


def same_bits(native, name, n, batch=1, splits=None, weightings=WEIGHTINGS, **options):
    verts, P = layout(name)
    cells = verts.shape[0]
    for gamma, sigma in weightings:
        slab_m, H_m = solve(native, verts, n, batch, gamma, sigma, **options)
        slab_p, H_p = solve(native, verts[P], n, batch, gamma, sigma, **options)
        where = f"{name} n={n} batch={batch} gamma={gamma} sigma={sigma} {options}"
        assert slab_m.shape == slab_p.shape and (splits is None or slab_m.shape[1] == splits), f"{where}: {slab_m.shape}"
        fill = np.frombuffer(bytes([FILL]) * 8, dtype=np.uint64)[0]
        assert not (slab_m[..., :cells] == fill).any() and not (slab_p[..., :cells] == fill).any(), f"{where}: sums never written"
        diff = np.flatnonzero(slab_p[..., :cells] != slab_m[..., P])
        print(f"{where}: {diff.size} of {slab_m[..., :cells].size} float64 sums differ, "
              f"{int((H_p != H_m[:, P]).sum())} of {H_m.size} float32 entries of H")
        assert np.array_equal(slab_p[..., :cells], slab_m[..., P]), f"{where}: {diff.size} sums differ, the first at {diff[0]}"
        assert np.array_equal(H_p, H_m[:, P]), f"{where}: the grids differ"


@pytest.mark.parametrize("n,splits,options", [(5, 1, {}), (63, 1, {}), (64, 1, {}), (65, 1, {}), (150, 1, {"want_waves": 1}), (150, 2, {})],
                         ids=["n5", "n63", "n64", "n65", "n150-one-split", "n150-two-splits"])
def test_row_changes_and_keypoint_counts_on_the_plain_grid(native, n, splits, options):
    same_bits(native, "rows", n, splits=splits, plan_slots=NO_PAIRS, **options)


@pytest.mark.parametrize("slots", [12, 21], ids=["ten-pairs", "one-pair"])
def test_paired_and_levelled_bodies(native, slots):
    """slots = 12: pairs (0, 1) .. (6, 7) share, pair (8, 9) touches three rows and runs the old paired loop, tile 10 (the
    overhang) is a levelled single block; slots = 21: one pair, the levelled single body for every other tile."""
    same_bits(native, "rows", 150, splits=2, plan_slots=slots)


def test_batch_of_three_on_the_plain_grid(native):
    same_bits(native, "rows", 150, batch=3, splits=2, plan_slots=12)


@pytest.mark.parametrize("options", [{"moments": 24}, {"moments": 24, "weights_f32": 1}], ids=["m24", "m24-w32-control"])
@pytest.mark.parametrize("slots", [12, NO_PAIRS], ids=["ten-pairs", "plain"])
def test_24_sums(native, options, slots):
    same_bits(native, "rows", 150, splits=2, plan_slots=slots, **options)


@pytest.mark.parametrize("slots", [NO_PAIRS, 5], ids=["plain", "paired"])
def test_non_monotone_blocks(native, slots):
    """A, B, A shares; A, C, B does not.  slots = 5 (4 tiles x 2 splits): three pairs, (0, 1) twice and (2, 3) once."""
    same_bits(native, "nonmono", 150, splits=2, plan_slots=slots)


@pytest.mark.parametrize("slots", [NO_PAIRS, 5], ids=["plain", "paired"])
def test_special_row_values(native, slots):
    """+0.0 / -0.0, one ulp apart, NaN and inf as vy: compared on the raw bytes."""
    same_bits(native, "special", 150, splits=2, plan_slots=slots)
    same_bits(native, "special", 65, plan_slots=NO_PAIRS, weightings=WEIGHTINGS[:1])


def test_sharing_blocks_against_the_valu_kernel(native):
    """Every block of ROWS in mesh order shares the term; the VALU kernel forms it in every lane."""
    verts, _ = layout("rows")
    gamma, sigma = WEIGHTINGS[0]
    _, H_mfma = solve(native, verts, 150, 1, gamma, sigma, plan_slots=NO_PAIRS)
    _, H_valu = solve(native, verts, 150, 1, gamma, sigma, variant=native.VARIANT_VALU)
    print(f"float32 entries of H that differ from the VALU kernel's: {int((H_mfma != H_valu).sum())} of {H_mfma.size}")
    assert np.array_equal(H_mfma, H_valu)
