"""The inputs of tests/panorama_edge_cases.py without a GPU: each reaches the edge that tests/test_gpu_panorama_edges.py and
tests/test_gpu_box_blur.py run it for.  Presence and statistics are the numpy specs' over the oracle's coordinates."""
import numpy as np
import pytest

import panorama_edge_cases as X
import panorama_gain_spec as G
import panorama_spec as S


def presence(name, sampling="nearest"):
    center, layers, geos, coords = X.get(name)
    return G.samples(center, layers, geos, coords, sampling)[0].any(axis=-1)


def tables(name, step=1):
    center, layers, geos, coords = X.get(name)
    return G.stats(G.samples(center, layers, geos, coords)[0], step)


def spec_status(layer):
    """The set-up's status word in the spec's terms: 1 where a cell has no float32 inverse, 2 where the edges do not cover
    the pair canvas (the oracle's LinAlgError and IndexError)."""
    from oracle import apap_oracle as O
    status = 0
    try:
        O.invert_cells_f32(np.array(layer.local_homography))
    except np.linalg.LinAlgError:
        status |= 1
    for count, edges in zip(layer.final_size, layer.mesh):
        try:
            O.cell_lookup(count, edges)
        except IndexError:
            status |= 2
    return status


def test_blur_lds_by_radius():
    """DESIGN.md's layout: th + 2 r rows of ((64 + 2 r) 3 + 3) & ~3 bytes and as many rows of 192 16-bit sums, th = 32 up to
    r = 16 and 16 above.  No radius needs more than 60 KB; the largest radius fills it under the 16-row tile."""
    need = {r: X.blur_lds_bytes(r) for r in range(1, 33)}
    assert max(need.values()) <= 61440 and need[32] == 61440
    assert need[16] == 43008 and need[17] == 34000
    assert [X.blur_tile_rows(r) for r in (1, 16, 17, 32)] == [32, 32, 16, 16]
    assert all(((64 + 2 * r) * 3) % 4 == (2 if r % 2 else 0) for r in range(1, 33)), "only an odd radius pads the row"
    # the 32-row tile with the halo of the largest radius would not fit
    assert (32 + 64) * (((64 + 64) * 3 + 3) & ~3) + (32 + 64) * 192 * 2 > 61440


def test_blur_views_reaches_its_edges():
    center, layers, geos, _ = X.get("blur_views")
    assert [(l.img.shape[1], l.img.shape[0]) for l in layers] == [(65, 33), (130, 67), (2, 1), (65, 33), (257, 17)]
    assert center.shape == (67, 130, 3)
    assert X.first_view_of(center, layers) == [0, 1, 0, 3, 1, 5], "D is the centre's picture, E is A's: a skipped view between blurred ones, twice"
    blurred = [center, layers[0].img, layers[2].img, layers[4].img]
    assert [X.blur_tiles(*p.shape[:2], 16) for p in blurred] == [9, 4, 1, 5]
    assert [X.blur_tiles(*p.shape[:2], 17) for p in blurred] == [15, 6, 1, 10]
    assert [spec_status(l) for l in layers] == [0] * 5
    for sampling in ("nearest", "bilinear"):
        p = presence("blur_views", sampling)
        for v, what in ((1, "A"), (5, "C"), (2, "D")):
            assert (p[v] & p[0]).sum() >= 100, (what, sampling)
        assert (p[4] & p[1] & ~p[0]).sum() >= 100, ("E and A outside the centre", sampling)
    # the low-pass pictures differ from the pictures at every radius the GPU test uses: a slot is not a copy
    import panorama_band_spec as P
    for r in (16, 17, 32):
        for img in blurred:
            assert (P.box_blur(img, r) != img).any()


def test_sixteen_has_17_views_of_one_tile():
    center, layers, _, _ = X.get("sixteen")
    assert len(layers) + 1 == 17 and X.first_view_of(center, layers) == list(range(17))
    assert all(X.blur_tiles(*p.shape[:2], 17) == 1 for p in [center] + [l.img for l in layers])
    assert [spec_status(l) for l in layers] == [0] * 16


def test_tall_gives_a_block_two_strips_of_unlike_views():
    center, layers, geos, _ = X.get("tall")
    W, H, _, _ = S.panorama_size(center.shape, geos)
    assert H % 4 != 0, "the last row block is partial"
    LW, LH, strips = X.stat_strips(W, H, 1)
    assert (LW, LH) == (W, H) and X.STAT_BLOCKS < strips == 4108 <= 2 * X.STAT_BLOCKS
    second = (X.STAT_BLOCKS * X.STAT_ROWS) // ((LW + X.STAT_COLS - 1) // X.STAT_COLS)     # the first lattice row of a second strip
    assert second == 16384
    assert [spec_status(l) for l in layers] == [0] * 4
    for sampling in ("nearest", "bilinear"):
        p = presence("tall", sampling)
        for (a, b), (top, bottom) in (((1, 4), (True, False)), ((2, 3), (False, True))):
            for pair in ((0, a), (0, b), (a, b)):
                both = p[pair[0]] & p[pair[1]]
                n_top, n_bottom = int(both[:64].sum()), int(both[second:].sum())
                assert (n_top >= 100 and n_bottom == 0) if top else (n_bottom >= 100 and n_top == 0), (pair, sampling, n_top, n_bottom)
        for a in (1, 4):
            for b in (2, 3):
                assert not (p[a] & p[b]).any()
    N, _ = tables("tall")
    assert [int(N[0, 1]), int(N[0, 4]), int(N[1, 4])] == [240, 288, 315] and [int(N[0, 2]), int(N[2, 3])] == [219, 171]
    # the first strips of the blocks 0 .. 11 hold rows 0 .. 47, their second strips rows 16384 .. 16431: both regions
    p = presence("tall")
    assert p[1][:48].any() and p[4][:48].any() and p[2][second:second + 48].any() and p[3][second:second + 48].any()
    # at steps 2 and 3 every block has one strip: the unlike strips are step 1's
    assert X.stat_strips(W, H, 2)[2] <= X.STAT_BLOCKS and X.stat_strips(W, H, 3)[2] <= X.STAT_BLOCKS


@pytest.mark.parametrize("step", sorted(X.STRIP_WIDTHS))
def test_lattice_widths_of_a_wave_and_a_column_more(step):
    got = []
    for width in X.STRIP_WIDTHS[step]:
        center, layers, geos, _ = X.get(f"strip{width}")
        W, H, _, _ = S.panorama_size(center.shape, geos)
        assert W == width
        LW, _, strips = X.stat_strips(W, H, step)
        got.append(LW)
        assert strips == ((LW + 255) // 256) * ((((H - 1) // step + 1) + 3) // 4)
        N, _ = tables(f"strip{width}", step)
        assert N[1, 2] > 0, "the layers that reach the last lattice columns overlap"
        p = presence(f"strip{width}")[:, ::step, ::step]
        assert p[1][:, LW - 1].any(), "a view is present in the last lattice column"
    assert got == [256, 256, 257]


def test_the_solve_inputs_reach_the_solves_paths():
    # an identity row: a view that overlaps no other
    N, _ = tables("wide")
    alone = [v for v in range(len(N)) if all(N[v, u] == 0 for u in range(len(N)) if u != v)]
    assert alone and all(N[v, v] > 0 for v in alone)
    g, q, flag = G.solve(*tables("wide"))
    assert flag == 0 and all(g[v] == 1.0 and q[v] == G.UNIT for v in alone) and len(set(q)) > 2
    # the full row stride of the factor
    assert len(tables("sixteen")[0]) == 17
    # the lower clamp
    center, layers, _, _ = X.get("dim")
    assert 230 <= center.min() and center.max() <= 250 and 8 <= layers[0].img.min() and layers[0].img.max() <= 22
    assert spec_status(layers[0]) == 0
    N, Sm = tables("dim")
    g, q, flag = G.solve(N, Sm)
    assert flag == 0 and q[0] == G.MIN_Q and 0.13 < g[0] < 0.15 and 4096.0 * g[0] < G.MIN_Q
    g, q, flag = G.solve(N, Sm, 5.0, 1.0)
    assert flag == 0 and q[0] == G.MIN_Q and G.MIN_Q < q[1] < G.MAX_Q
    for name in X.SOLVE_CASES:
        g, q, flag = G.solve(*tables(name))
        assert flag == 0 and all(v < G.MAX_Q for v in q), name     # the upper clamp and the flag stay with the host tests
