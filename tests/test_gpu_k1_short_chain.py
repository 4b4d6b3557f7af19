"""K1's short weight chain against the full one, bit for bit.

k_assemble_mfma with float64 weights runs a 64-keypoint chunk on a shorter chain - the exp table's entry already scaled, no
clamp at gamma^2 - where it has proved, from the chunk's keypoints and the bounding box of the block's cells, that every scaled
distance yu stays below ylim = (1 - 2^-20) min(768, -512 log2(gamma^2)) (cvx_proj_amd/csrc/apap_exp_long.h).  Either chain
gives the same bits, and apap_ctx_set_short_chain(ctx, 0) sends every chunk through the full one: every problem here is solved
with the switch at 1 and at 0, and the WHOLE moment workspace (every float64 sum of every split, padded cells included; it starts
as a fill pattern) and the grid H must be byte-equal - on the raw bytes, the problems include NaN and infinity.

The problems: 197 cells (tiles of 64, 64, 64 and 5 cells) in three vertex layouts, keypoints inside a 640 x 480 picture, so
distances up to ~800 px and yu = d * 1477 / sigma^2.
  wide     vy = 150 * (cell // 64): every tile and every pair of tiles holds at most two vy - the blocks SHARE the row term
  scatter  random vertices: no block shares
  line     vy = 240 everywhere, vx from exactly 0 to 640: for the keypoint placed on the limit (below)
Launch forms through plan_slots as tests/test_gpu_k1_paired.py reaches them (4 tiles x 2 splits = 8 units; x 1 split = 4):
  plain (nothing paired, the 3-D grid), slots = 5 (three pairs: the paired body, and levelled single blocks), slots = 7 (one
  pair), and slots = 3 with one split (one pair, two levelled singles).
Verdicts, at gamma = 0.5 (ylim = 768 less the margin):
  sigma = 100  yu <= 133: every chunk qualifies          sigma = 8  yu ~ 23 d: none does (yu far above the table)
  sigma = 30   yu = 1.64 d: chunks qualify or not by where their keypoints lie
  sigma = 100 with ONE keypoint moved to (1e4, 1e4) - in the table's columns 30, 31, which is where K1 reads it - in the first
  chunk (row 3: the block switches to the full chain at once and stays there) or in the second only (row 70)
gamma in {0, 0.5, 0.9, 1, 2}: ylim = 768, 768, 155.6 (sigma = 100: yu <= 133 still qualifies; sigma = 60 does not), 0, 0.
Not finite: a NaN and an infinite keypoint coordinate (the full chain gives such a keypoint the weight gamma^2, the short one
would give NaN: the chunk must not qualify), a NaN vertex (the same for a cell: the block must not qualify), and a vertex
equal to a keypoint (d = 0: yu = 1e-150 scale, the table's entry of 0).
On the limit: layout `line`, a keypoint at (x, 240), so that the bound the kernel checks is fma(x, x, 1e-300) s^2 < ylim^2 with
no other rounding; x is the largest double for which it holds (found by bisection with exact rational arithmetic) and, in a
second problem, the next double, for which it does not.  yu is then within 2^-20 of 768: the table's last entry.

The body test.  That the short body runs where a chunk qualifies cannot be seen from the results (that is the point of it), and
a comparison of the two settings passes as well when both run the full body.  So every solve here is profiled
(APAP_OPT_PROFILE), under which the kernel counts per block the chunks it ran and how many of them on the short chain
(apap_ctx_profile_k1_chunks): with the switch at 0 the count of short chunks must be 0, and with it at 1 it must be what the
problem says - every chunk where all qualify, none where none can (sigma = 8, gamma >= 1, float32 weights), and exact numbers,
worked out below from the launch's blocks, for the far keypoint, the values that are not finite and the keypoint on the limit.
(tests/test_exp_long_host.py asserts from the compiled code what the short loops hold.)
Blocks and chunks at n = 200, two splits of 128 + 72 keypoints (2 chunks each: 64 + 64, 64 + 8): the plain grid has 4 tiles x 2
splits = 8 blocks, 16 chunks; slots = 5 has 5 blocks - split 0: pairs (0, 1) and (2, 3); split 1: pair (0, 1), tiles 2 and 3
single - 10 chunks (a paired block counts a chunk once).  At n = 150: 128 + 22 keypoints, 2 + 1 chunks, 12 on the plain grid.
"""
import ctypes
import functools
import math
from fractions import Fraction

import numpy as np
import pytest

from cvx_proj_amd.synth import synth_pair

pytestmark = pytest.mark.gpu

NO_PAIRS = 1 << 30
FILL = 0xA5
CELLS = 197
K_EXP_LONG = 768
MARGIN = 1.0 - 2.0 ** -20
K_EXP_SCALE = 512.0 * float.fromhex("0x1.71547652b82fep+0")


@functools.lru_cache(maxsize=None)
def vertices(layout):
    rng = np.random.default_rng(1970 + len(layout))
    cell = np.arange(CELLS)
    if layout == "wide":
        v = np.stack([rng.random(CELLS) * 640.0, 150.0 * (cell // 64)], axis=1)
    elif layout == "scatter":
        v = rng.random((CELLS, 2)) * [640.0, 480.0]
    else:
        v = np.stack([np.linspace(0.0, 640.0, CELLS), np.full(CELLS, 240.0)], axis=1)
        assert v[0, 0] == 0.0 and v[:, 0].min() == 0.0
    v.setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def problem(n):
    """(tables {30, 24} as numpy [n][32], denormalisation) of one synthetic pair; never written.  (n = 1: the first row of a
    pair of two keypoints - the host set-up wants two, the solve takes one.)"""
    from cvx_proj_amd import _native as native
    p = synth_pair(640, 480, max(n, 2), 4, seed=6100 + n)
    q = native.host_prepare(p.src, p.dst)
    tabs = {m: np.ascontiguousarray(native.host_build_table(p.src, q["cf1"], q["cf2"], moments=m)[:n]) for m in (30, 24)}
    for t in tabs.values():
        assert t.shape == (n, 32) and np.array_equal(t[:, 30:32], p.src[:n].astype(np.float64))
        t.setflags(write=False)
    return tabs, native.host_build_denorm(q["iC2"], q["C1"], q["iN2"], q["N1"])


def solve(native, table, verts, den, gamma, sigma, **options):
    """(workspace bytes, H bytes, splits) of one solve with the MFMA variant forced."""
    import torch
    n, cells = table.shape[0], verts.shape[0]
    sums = options.get("moments", 30)
    d_tab = torch.from_numpy(np.array(table)).to("cuda:0")
    d_vert = torch.from_numpy(np.array(verts)).to("cuda:0")
    d_den = torch.from_numpy(np.array(den)).to("cuda:0")
    ctx = native.Context(variant=native.VARIANT_MFMA, profile=1, **options)
    nbytes = native.lib().apap_solve_batch_workspace_bytes(native._h(ctx), n, cells, 1)
    work = torch.full((nbytes,), FILL, dtype=torch.uint8, device="cuda:0")
    H = torch.full((1, cells, 9), float("nan"), dtype=torch.float32, device="cuda:0")
    native.check(native.lib().apap_solve_batch_device(native._h(ctx), d_tab.data_ptr(), n, d_vert.data_ptr(), 0, cells, gamma, sigma,
                                                      d_den.data_ptr(), H.data_ptr(), 1, work.data_ptr(), nbytes, ctypes.c_void_p(0)))
    torch.cuda.synchronize()
    counts = ctx.profile_k1_chunks()
    assert ctx.profile_k1_chunks() == (0, 0), "a read clears the counts"
    ctx.close()
    per_split = sums * ((cells + 63) // 64 * 64) * 8
    assert nbytes % per_split == 0
    return work.cpu().numpy(), H.cpu().numpy().view(np.uint32), nbytes // per_split, counts


def same_bits(native, n, layout, gamma, sigma, splits=None, table=None, verts=None, expect=None, **options):
    """`expect`: "all", "none", or (short chunks, chunks) of the solve with the switch at 1; None where the problem does not say."""
    tabs, den = problem(n)
    table = tabs[options.get("moments", 30)] if table is None else table
    verts = vertices(layout) if verts is None else verts
    short = solve(native, table, verts, den, gamma, sigma, short_chain=1, **options)
    full = solve(native, table, verts, den, gamma, sigma, short_chain=0, **options)
    where = f"n={n} {layout} gamma={gamma} sigma={sigma} {options}"
    assert short[2] == full[2] and (splits is None or short[2] == splits), f"{where}: {short[2]} splits"
    a, b = short[0].view(np.uint64), full[0].view(np.uint64)
    fill = np.frombuffer(bytes([FILL]) * 8, dtype=np.uint64)[0]
    assert not (b == fill).any(), f"{where}: sums never written"
    diff = np.flatnonzero(a != b)
    print(f"{where}: {diff.size} of {a.size} float64 sums differ, {int((short[1] != full[1]).sum())} of {full[1].size} entries of H")
    assert diff.size == 0, f"{where}: {diff.size} sums differ, the first at index {diff[0]}"
    assert np.array_equal(short[1], full[1]), f"{where}: the grids differ"
    (ran_short, ran), (off_short, off_ran) = short[3], full[3]
    print(f"{where}: {ran_short} of {ran} chunks on the short chain")
    assert off_short == 0 and off_ran == ran > 0 and ran_short <= ran, f"{where}: {short[3]} with the switch at 1, {full[3]} at 0"
    if expect == "all":
        assert ran_short == ran, f"{where}: {ran_short} of {ran} chunks ran the short body, all of them qualify"
    elif expect == "none":
        assert ran_short == 0, f"{where}: {ran_short} of {ran} chunks ran the short body, none may"
    elif expect is not None:
        assert (ran_short, ran) == expect, f"{where}: {(ran_short, ran)} chunks (short, all), the launch has {expect}"


def moved(n, row, x, y, sums=30):
    """The table of problem(n) with keypoint `row` moved to (x, y): columns 30 and 31."""
    t = np.array(problem(n)[0][sums])
    t[row, 30], t[row, 31] = x, y
    return t


# (plan_slots, other options, splits): the launch forms; one split needs n < 128 or want_waves = 1
FORMS = {"plain": (NO_PAIRS, {}), "three-pairs": (5, {}), "one-pair": (7, {}), "one-split-paired": (3, {"want_waves": 1})}


def test_the_switch_and_its_default(native):
    """A switch of the context beside the option table (apap_ctx_set_short_chain): default 1, 0 or 1, NULL = the default."""
    lib = native.lib()
    ctx = native.Context()
    assert ctx.get("short_chain") == 1
    assert ctx.set("short_chain", 0).get("short_chain") == 0
    for bad in (2, -1):
        with pytest.raises(ValueError):
            ctx.set("short_chain", bad)
    assert ctx.get("short_chain") == 0 and ctx.set("short_chain", 1).get("short_chain") == 1
    ctx.close()
    c = native.Context(short_chain=0, moments=24)       # the constructor's name, beside a numbered option
    assert (c.get("short_chain"), c.get("moments")) == (0, 24)
    c.close()
    v = ctypes.c_int(-1)
    assert lib.apap_ctx_get_short_chain(None, ctypes.byref(v)) == native.OK and v.value == 1
    assert lib.apap_ctx_set_short_chain(None, 0) == native.ERR_INVALID_ARG      # NULL cannot be changed
    assert lib.apap_ctx_get_short_chain(None, None) == native.ERR_INVALID_ARG


@pytest.mark.parametrize("n", [1, 63, 64, 65, 130, 200])
@pytest.mark.parametrize("layout", ["wide", "scatter"])
def test_keypoint_counts_and_split_counts(native, n, layout):
    """A partial chunk alone, whole chunks, one more than a chunk; 130 and 200 in two splits (128 + 2: a split that ends on a
    chunk's edge, 128 + 72) and in one (two and three whole chunks and a partial one).  Every chunk qualifies (sigma = 100)
    and none does (sigma = 8)."""
    for sigma, expect in ((100.0, "all"), (8.0, "none")):
        same_bits(native, n, layout, 0.5, sigma, splits=2 if n >= 128 else 1, plan_slots=NO_PAIRS, expect=expect)
        if n >= 128:
            same_bits(native, n, layout, 0.5, sigma, splits=1, plan_slots=NO_PAIRS, want_waves=1, expect=expect)


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("layout", ["wide", "scatter"])
@pytest.mark.parametrize("sigma", [100.0, 30.0, 8.0], ids=["all-qualify", "some-qualify", "none-qualifies"])
def test_kernel_bodies_and_verdicts(native, form, layout, sigma):
    """The plain grid, the levelled and the paired body, each in a block that shares the row term (wide) and one that does not."""
    slots, options = FORMS[form]
    expect = {100.0: "all", 30.0: None, 8.0: "none"}[sigma]
    same_bits(native, 200, layout, 0.5, sigma, splits=1 if options else 2, plan_slots=slots, expect=expect, **options)


@pytest.mark.parametrize("form", ["plain", "three-pairs"])
@pytest.mark.parametrize("layout", ["wide", "scatter"])
@pytest.mark.parametrize("row", [3, 70], ids=["far-keypoint-in-the-first-chunk", "far-keypoint-in-the-second-chunk-only"])
def test_one_far_keypoint(native, form, layout, row):
    """sigma = 100: every chunk qualifies but the one that holds the moved keypoint (yu ~ 2000); in the first chunk the block
    never runs the short body, in the second it runs it once and then never again; the other split is untouched by it."""
    slots, options = FORMS[form]
    # split 0's blocks (4 on the plain grid, 2 with three pairs) run 0 or 1 of their 2 chunks short, split 1's both
    expect = {("plain", 3): (8, 16), ("plain", 70): (12, 16), ("three-pairs", 3): (6, 10), ("three-pairs", 70): (8, 10)}[form, row]
    for sums in (30, 24):
        same_bits(native, 200, layout, 0.5, 100.0, splits=2, table=moved(200, row, 1e4, 1e4, sums), plan_slots=slots, expect=expect,
                  **({"moments": 24} if sums == 24 else {}), **options)


@pytest.mark.parametrize("gamma", [0.0, 0.5, 0.9, 1.0, 2.0])
@pytest.mark.parametrize("layout", ["wide", "scatter"])
def test_gammas(native, gamma, layout):
    """ylim = 768, 768, 155.6, 0, 0 (less the margin): sigma = 100 keeps yu below 133, sigma = 60 takes it to 370 - above the
    limit of gamma = 0.9, where the clamp would bite - and sigma = 30 past the table."""
    for sigma in (100.0, 60.0, 30.0):
        for slots in (NO_PAIRS, 5):
            expect = "none" if gamma >= 1.0 else "all" if sigma == 100.0 else None
            same_bits(native, 150, layout, gamma, sigma, splits=2, plan_slots=slots, expect=expect)


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("layout", ["wide", "scatter"])
def test_24_sums_with_float64_weights(native, form, layout):
    slots, options = FORMS[form]
    for sigma, expect in ((100.0, "all"), (30.0, None)):
        same_bits(native, 200, layout, 0.5, sigma, moments=24, plan_slots=slots, expect=expect, **options)
    # the float32-weight form has no short chain: the unchanged control
    same_bits(native, 200, layout, 0.5, 100.0, moments=24, weights_f32=1, plan_slots=slots, expect="none", **options)


@pytest.mark.parametrize("slots", [NO_PAIRS, 5], ids=["plain", "three-pairs"])
@pytest.mark.parametrize("layout", ["wide", "scatter"])
def test_values_that_are_not_finite(native, slots, layout):
    nan, inf = float("nan"), float("inf")
    src = problem(150)[0][30][:, 30:32]
    plain = slots == NO_PAIRS
    # n = 150 on the plain grid: 4 blocks of split 0 with 2 chunks, 4 of split 1 with one.  A keypoint that is no number stops
    # its split's blocks at its chunk: row 5 -> 0 of 2, row 70 -> 1 of 2 (split 0), row 140 -> 0 of 1 (split 1)
    for row, x, y in [(5, nan, 100.0), (70, 100.0, nan), (5, inf, 100.0), (140, 100.0, -inf), (70, nan, inf)]:
        expect = {5: (4, 12), 70: (8, 12), 140: (8, 12)}[row] if plain else None
        same_bits(native, 150, layout, 0.5, 100.0, splits=2, table=moved(150, row, x, y), plan_slots=slots, expect=expect)
    # a vertex that is no number stops its tile's two blocks altogether: 3 chunks of 12
    for cell, vx, vy in [(10, nan, None), (70, None, nan), (196, nan, nan), (130, inf, None)]:
        v = np.array(vertices(layout))
        v[cell, 0] = v[cell, 0] if vx is None else vx
        v[cell, 1] = v[cell, 1] if vy is None else vy
        same_bits(native, 150, layout, 0.5, 100.0, splits=2, verts=v, plan_slots=slots, expect=(9, 12) if plain else None)
    v = np.array(vertices(layout))      # d = 0: vertices that ARE keypoints, in the first and in the last tile
    v[7], v[195] = src[3], src[149]
    same_bits(native, 150, layout, 0.5, 100.0, splits=2, verts=v, plan_slots=slots, expect="all")
    same_bits(native, 150, layout, 0.0, 100.0, splits=2, verts=v, plan_slots=slots, expect="all")


def bound_holds(x, sigma, ylim):
    """The kernel's compare for a keypoint (x, 240) against the box [0, 640] x [240, 240] of layout `line`, x >= 640: every
    operation as the device performs it - the fused step exactly, by rational arithmetic."""
    inv_sigma2 = 2.0 * (1.0 / (sigma * sigma))
    s = inv_sigma2 * K_EXP_SCALE
    ax = max(abs(x - 0.0), abs(x - 640.0))
    ay = max(abs(240.0 - 240.0), abs(240.0 - 240.0))
    inner = float(Fraction(ay) * Fraction(ay) + Fraction(1e-300))
    d2 = float(Fraction(ax) * Fraction(ax) + Fraction(inner))
    return d2 * (s * s) < ylim * ylim


@pytest.mark.parametrize("slots", [NO_PAIRS, 5], ids=["plain", "three-pairs"])
def test_a_keypoint_on_the_limit(native, slots):
    sigma, gamma = 100.0, 0.5
    ylim = MARGIN * min(float(K_EXP_LONG), -512.0 * math.log2(gamma * gamma))
    assert ylim == MARGIN * K_EXP_LONG
    lo, hi = 640.0, 1e5     # the bound holds at lo and not at hi
    assert bound_holds(lo, sigma, ylim) and not bound_holds(hi, sigma, ylim)
    while np.nextafter(lo, hi) < hi:
        mid = lo + (hi - lo) / 2
        if not lo < mid < hi:
            mid = float(np.nextafter(lo, hi))
        lo, hi = (mid, hi) if bound_holds(mid, sigma, ylim) else (lo, mid)
    assert hi == np.nextafter(lo, 1e9) and bound_holds(lo, sigma, ylim) and not bound_holds(hi, sigma, ylim)
    yu = lo * (2.0 * (1.0 / (sigma * sigma)) * K_EXP_SCALE)
    assert K_EXP_LONG - 1 < yu < K_EXP_LONG, yu     # the table's last entry
    print(f"the last keypoint below the limit: x = {lo!r} ({lo.hex()}), yu = {yu!r}")
    # Only tile 0's box reaches down to x = 0, so only its block of the keypoint's split can fail, and at `hi` it must, from
    # the keypoint's chunk on: row 3 -> 0 of split 0's 2 chunks, row 70 -> 1 of 2, row 149 -> 0 of split 1's one.
    for x in (lo, hi):
        for row in (3, 70, 149):
            expect = None if slots != NO_PAIRS else (12, 12) if x == lo else {3: (10, 12), 70: (11, 12), 149: (11, 12)}[row]
            same_bits(native, 150, "line", gamma, sigma, splits=2, table=moved(150, row, x, 240.0), plan_slots=slots, expect=expect)
