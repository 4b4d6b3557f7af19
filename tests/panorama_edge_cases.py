"""Inputs of the edge tests of the box blur, the two-band blend's low-pass slots, the overlap statistics and the device gain
solve (tests/test_gpu_panorama_edges.py); tests/test_panorama_edge_inputs.py shows without a GPU that each reaches its edge.

A case is a dict as in tests/panorama_cases.py.  Built once per session and shared: read-only."""
import numpy as np

import panorama_cases as E
import panorama_ramp_cases as RC
import panorama_spec as S

# k_box_blur (DESIGN.md "Panorama, two-band blend"): a tile of 64 columns and 32 rows up to r = 16, 16 rows above
BLUR_COLS, BLUR_SWITCH = 64, 16
STAT_COLS, STAT_ROWS, STAT_BLOCKS = 256, 4, 4096     # k_panorama_stats: a strip, and the blocks that share the strips


def blur_tile_rows(r):
    return 32 if r <= BLUR_SWITCH else 16


def blur_tiles(h, w, r):
    """Blocks of k_box_blur for an h x w picture."""
    th = blur_tile_rows(r)
    return ((w + BLUR_COLS - 1) // BLUR_COLS) * ((h + th - 1) // th)


def blur_lds_bytes(r):
    """The tile with its halo as bytes, rows padded to a dword, and the 16-bit row sums of its 192 output bytes a row."""
    rows_in = blur_tile_rows(r) + 2 * r
    return rows_in * (((BLUR_COLS + 2 * r) * 3 + 3) & ~3) + rows_in * (BLUR_COLS * 3) * 2


def up256(n):
    return (n + 255) & ~255


def stat_strips(W, H, step):
    """(lattice width, lattice height, strips) of k_panorama_stats, by the launcher's formula."""
    LW, LH = (W - 1) // step + 1, (H - 1) // step + 1
    return LW, LH, ((LW + STAT_COLS - 1) // STAT_COLS) * ((LH + STAT_ROWS - 1) // STAT_ROWS)


def blur_views():
    """A centre of 130 x 67 and the layers A (65 x 33), D (the centre's own picture object), B (2 x 1, magnified four times),
    E (A's picture object under another placement) and C (257 x 17): 9, 4, 1 and 5 tiles under the 32-row tile, 15, 6, 1 and 10
    under the 16-row tile, a view that is not blurred again between blurred ones twice.  A, C and D overlap the centre; E
    overlaps A left of the centre."""
    rng = np.random.default_rng(13067)
    center = E.picture(rng, 130, 67)
    a = E.picture(rng, 65, 33)
    layers = [E.make_layer(rng, center.shape, 65, 33, E.placement(-40.0, 20.0, 0.01), 2, 2, img=a),
              E.make_layer(rng, center.shape, 130, 67, E.placement(100.0, -40.0, -0.01), 3, 2, img=center),
              E.make_layer(rng, center.shape, 2, 1, np.array([[4.0, 0.0, 50.5], [0.0, 4.0, 10.5], [0.0, 0.0, 1.0]]), 1, 2),
              E.make_layer(rng, center.shape, 65, 33, E.placement(-60.0, 30.0, -0.02), 1, 3, img=a),
              E.make_layer(rng, center.shape, 257, 17, E.placement(-100.0, 60.0, 0.005), 2, 5)]
    assert layers[1].img is center and layers[3].img is layers[0].img
    return dict(center=center, layers=layers, geometries=[tuple(l.final_size) + tuple(l.offset) for l in layers], planted=[None] * 5)


def first_view_of(center, layers):
    """Per view (the centre, then every layer) the first view with the same picture object: itself unless it is a duplicate."""
    pictures = [center] + [l.img for l in layers]
    return [next(u for u in range(v + 1) if pictures[u] is pictures[v]) for v in range(len(pictures))]


def tall():
    """A canvas of 16 x 16430: 4108 strips at step 1, so the blocks 0 .. 11 of the 4096 take a second strip, 4096 strips and
    16384 canvas rows further down; the last row block is partial.  Views 1 and 4 overlap the centre and each other in canvas
    rows below 64 only, views 2 and 3 in rows from 16384 on only: a block's two strips see unlike sets of views."""
    specs = [(12, 40, E.placement(2.0, 3.0, 0.01), 2, 2),
             (10, 30, E.placement(-3.0, 16392.0, -0.01), 3, 1),
             (9, 50, E.placement(1.0, 16380.0), 1, 2),
             (14, 36, E.placement(-2.0, 8.0, 0.02), 2, 1)]
    return E.build(4097, (8, 16420), specs)


def dim():
    """A centre of bytes 230 .. 250 under one layer of bytes 8 .. 22, placed on it by a translation of whole pixels: the
    centre's gain falls to 0.14 and q[0] clamps at 1024."""
    rng = np.random.default_rng(1024)
    center = rng.integers(230, 251, (40, 48, 3), dtype=np.uint8)
    img = rng.integers(8, 23, (30, 36, 3), dtype=np.uint8)
    layers = [E.make_layer(rng, center.shape, 36, 30, E.placement(5.0, 4.0), 2, 2, img=img)]
    return dict(center=center, layers=layers, geometries=[tuple(l.final_size) + tuple(l.offset) for l in layers], planted=[None])


STRIP_WIDTHS = {2: (511, 512, 513), 3: (766, 768, 769)}     # step: canvas widths with lattices of 256, 256 and 257 columns

CASES = {"blur_views": blur_views, "tall": tall, "dim": dim}
SOLVE_CASES = ("cross", "wide", "sixteen", "black_outside", "two_pixels", "tall", "dim")

_cache = {}


def get(name):
    """(center, layers, geometries, the oracle's coordinates) of a case of CASES, of tests/panorama_cases.py or of
    ``strip<width>``."""
    if name not in _cache:
        if name in CASES:
            case = CASES[name]()
            coords = [RC.layer_coords(l) for l in case["layers"]]
        elif name.startswith("strip"):
            case = E.strip_case(int(name[5:]))
            coords = [RC.layer_coords(l) for l in case["layers"]]
        else:
            case, coords = E.get(name), RC.oracle_coords(name)
        _cache[name] = (case["center"], case["layers"], case["geometries"], coords)
    return _cache[name]


def canvas(name):
    center, _, geos, _ = get(name)
    return S.panorama_size(center.shape, geos)
