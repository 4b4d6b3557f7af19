"""Seeded inputs of the panorama tests: a centre picture and layers that need no solver.

Layer k's forward grid is ``Hg_k (I + 1e-3 S(cell))`` cast to float32, ``S`` a smooth function of the cell's row and column:
cells that differ as a moving-DLT grid's do, around a global homography ``Hg_k`` that places the layer.  The geometry is the
reference's own: ``geometry.final_size`` for the pair canvas and the offsets, ``geometry.get_mesh`` for the edges.

A case is a dict: ``center`` (h, w, 3) uint8, ``layers`` (a list of ``_native.PanoramaLayer``), ``geometries`` (a list of
(fw, fh, ox, oy)), ``planted`` (per layer, the source pixels planted black and with one non-zero channel, as (x, y))."""
import numpy as np

from cvx_proj_amd import geometry
from cvx_proj_amd._native import PanoramaLayer

STRIP_ROWS, WAVES_PER_BLOCK, STRIP_COLS, GROUP = 4, 4, 256, 4       # k_panorama's tiling (csrc/apap_panorama.hip)


class _Shape:
    def __init__(self, shape):
        self.shape = shape


def placement(tx, ty, angle=0.0, px=0.0, py=0.0):
    """other -> centre: a rotation by ``angle`` about the origin, the translation (tx, ty), perspective terms (px, py)."""
    c, s = np.cos(angle), np.sin(angle)
    return np.array([[c, -s, tx], [s, c, ty], [px, py, 1.0]])


def picture(rng, w, h):
    """Bytes 1 .. 255: no pixel is black unless a test plants it."""
    return rng.integers(1, 256, (h, w, 3), dtype=np.uint8)


def make_layer(rng, center_shape, w, h, Hg, rows, cols, irregular=False, img=None):
    img = picture(rng, w, h) if img is None else img
    fw, fh, ox, oy = (int(v) for v in geometry.final_size(_Shape(img.shape), _Shape(center_shape), Hg))
    mesh_w, mesh_h = geometry.get_mesh((fw, fh), cols + 1)[0], geometry.get_mesh((fw, fh), rows + 1)[1]
    if irregular:       # interior edges moved by up to a third of a cell, still increasing
        for e in (mesh_w, mesh_h):
            if e.size > 2:
                e[1:-1] += (rng.random(e.size - 2) - 0.5) * (e[1] - e[0]) * 0.66
    r, c = np.meshgrid(np.arange(rows) / max(rows, 1), np.arange(cols) / max(cols, 1), indexing="ij")
    S = np.zeros((rows, cols, 3, 3))
    S[..., 0, 0], S[..., 0, 1], S[..., 0, 2] = np.sin(2.0 * r + c), np.cos(r - 3.0 * c), 300.0 * np.sin(3.0 * r) * np.cos(2.0 * c)
    S[..., 1, 0], S[..., 1, 1], S[..., 1, 2] = np.cos(r + 2.0 * c), np.sin(3.0 * r - c), 300.0 * np.cos(2.0 * r + c)
    S[..., 2, 0], S[..., 2, 1] = 1e-2 * np.sin(r + c), 1e-2 * np.cos(r - c)
    H = (Hg @ (np.eye(3) + 1e-3 * S)).astype(np.float32)
    return PanoramaLayer(img, H, (mesh_w, mesh_h), (fw, fh), (ox, oy))


def plant(layer, center_shape, Hg, at=(0.5, 0.5)):
    """A black pixel and, two pixels to its right, one with a single non-zero channel, each as a 3 x 3 block (the warp is close
    to a translation: some canvas pixel samples a block's middle) around the source point that lands at ``at`` (fractions of
    the centre picture).  Returns the two source pixels (x, y)."""
    h, w = layer.img.shape[:2]
    p = np.linalg.inv(Hg) @ np.array([at[0] * center_shape[1], at[1] * center_shape[0], 1.0])
    x, y = int(np.clip(p[0] / p[2], 2, w - 7)), int(np.clip(p[1] / p[2], 2, h - 3))
    layer.img[y - 1:y + 2, x - 1:x + 2] = 0
    layer.img[y - 1:y + 2, x + 3:x + 6] = (0, 0, 7)
    return (x, y), (x + 4, y)


def build(seed, center_wh, specs, plant_at=None):
    """specs: (w, h, Hg, rows, cols[, irregular]) per layer."""
    rng = np.random.default_rng(seed)
    center = picture(rng, *center_wh)
    layers, planted = [], []
    for k, spec in enumerate(specs):
        w, h, Hg, rows, cols = spec[:5]
        layer = make_layer(rng, center.shape, w, h, Hg, rows, cols, irregular=len(spec) > 5 and spec[5])
        planted.append(plant(layer, center.shape, Hg, plant_at[k]) if plant_at and plant_at[k] else None)
        layers.append(layer)
    return dict(center=center, layers=layers, geometries=[tuple(l.final_size) + tuple(l.offset) for l in layers], planted=planted)


def cross():
    """Centre 61 x 47 and four layers to its left, right, top and bottom; sources 64 x 48, 50 x 70, 33 x 33, 90 x 40, meshes
    1 x 1, 3 x 5, 9 x 9 (irregular) and 20 x 7.  All four and the centre overlap in a small rectangle; each layer's planted
    pixels land inside the centre's rectangle."""
    specs = [(64, 48, placement(-29.0, 3.0, 0.02, 1e-5, -2e-5), 1, 1),
             (50, 70, placement(26.0, -10.0, -0.03, -2e-5, 1e-5), 3, 5),
             (33, 33, placement(-2.0, -19.0, 0.01), 9, 9, True),
             (90, 40, placement(-15.0, 10.0, -0.015, 1e-5, 1e-5), 20, 7)]
    return build(101, (61, 47), specs, plant_at=[(0.3, 0.5), (0.7, 0.5), (0.4, 0.15), (0.5, 0.7)])


def strip_edges(width):
    """Canvases 259 and 517 pixels wide (a wave covers 256) and one row higher than a multiple of the block's 16 rows: pure
    translations by whole pixels place the layers, so the canvas is known in advance."""
    if width == 259:
        specs = [(100, 33, placement(159.0, 0.0), 2, 3), (70, 20, placement(140.0, 6.0, 0.01), 4, 4)]
        return build(259, (200, 30), specs)
    assert width == 517
    specs = [(227, 17, placement(290.0, 0.0), 1, 6), (140, 12, placement(200.0, 2.0, -0.01), 3, 2), (90, 17, placement(255.0, 0.0), 2, 2)]
    return build(517, (300, 17), specs)


def strip_case(width):
    """``strip_edges`` at a canvas one column short of a wave's 256, exactly that wide and one column wider; 33 rows: one more
    than two blocks of 16."""
    specs = [(100, 33, placement(width - 100.0, 0.0), 2, 3), (70, 20, placement(width - 119.0, 6.0, 0.01), 4, 4)]
    case = build(width, (200, 30), specs)
    assert geometry.panorama_size(case["center"].shape, case["layers"])[0] == width
    return case


def single_c1():
    """K = 1 at C1's size: 768 x 768 pictures, a 20 x 20 mesh."""
    return build(768, (768, 768), [(768, 768, np.array([[1.02, 0.01, 12.3], [-0.015, 0.99, 8.4], [2.5e-5, -5e-5, 1.0]]), 20, 20)])


def sixteen(n=16):
    """n layers of 8 x 8 pictures around an 8 x 8 centre."""
    specs = [(8, 8, placement(3.0 * np.cos(k * 2.0 * np.pi / 16), 3.0 * np.sin(k * 2.0 * np.pi / 16), 0.01 * k), 1 + k % 3, 1 + k % 2)
             for k in range(n)]
    return build(16, (8, 8), specs)


def linear_scan():
    """One layer with a 1 x 4100 mesh on a 4200 x 6 pair canvas: more than 4096 edges take the set-up's linear-scan kernels."""
    case = build(4100, (100, 6), [(4100, 6, placement(100.0, 0.0), 1, 4100)])
    assert case["geometries"] == [(4200, 6, 0, 0)]
    return case


def shared_source():
    """Two layers that are the same picture object, placed left and right of the centre."""
    rng = np.random.default_rng(77)
    center = picture(rng, 40, 30)
    img = picture(rng, 36, 28)
    layers = [make_layer(rng, center.shape, 36, 28, placement(-14.0, 3.0, 0.02), 2, 2, img=img),
              make_layer(rng, center.shape, 36, 28, placement(19.0, -3.0, -0.02), 3, 3, img=img)]
    assert layers[0].img is layers[1].img
    return dict(center=center, layers=layers, geometries=[tuple(l.final_size) + tuple(l.offset) for l in layers], planted=[None, None])


def plant_at(layer, Hg, point):
    """``plant`` with the target given as a point (x, y) relative to the centre picture's first pixel - a canvas pixel less
    (OX, OY) - which may lie outside the centre picture.  Returns the two source pixels (x, y)."""
    h, w = layer.img.shape[:2]
    p = np.linalg.inv(Hg) @ np.array([point[0], point[1], 1.0])
    x, y = int(np.clip(p[0] / p[2], 2, w - 7)), int(np.clip(p[1] / p[2], 2, h - 3))
    layer.img[y - 1:y + 2, x - 1:x + 2] = 0
    layer.img[y - 1:y + 2, x + 3:x + 6] = (0, 0, 7)
    return (x, y), (x + 4, y)


def wide():
    """Pair canvases against the 256-column strips of a 530 x 18 canvas: one begins in a strip's last column (dx = 255), one in
    the next strip's first (256), one ends with a strip (right = 512), one a column later (513); one ends a row below a strip
    of 4 rows (below = 17).  The placements are translations, by a fraction that keeps the pair canvases' first and last
    columns inside the sources although every cell moves by a few tenths of a pixel."""
    specs = [(30, 9, placement(-300.0, 0.0), 1, 2),
             (20, 9, placement(-45.6, 0.0), 2, 2),
             (20, 12, placement(-44.6, 2.0), 1, 3),
             (30, 9, placement(182.4, 0.0), 2, 1),
             (30, 9, placement(183.4, -3.0), 1, 1),
             (30, 14, placement(200.4, 1.0), 3, 2)]
    return build(530, (40, 9), specs)


def exact():
    """A canvas of exactly 256 x 16: one block, no partial strip, no row tail."""
    return build(256, (200, 10), [(56, 16, placement(200.0, 0.0), 2, 2), (60, 9, placement(100.0, 1.0), 1, 3)])


def black_outside():
    """Two layers that overlap right of the centre picture; the FIRST has a black block and a block with one non-zero channel
    in that overlap: paste falls through to the second layer on a value there, not on an absence."""
    Hg0 = placement(25.0, 5.0, 0.02, 1e-5, -1e-5)
    case = build(77, (30, 20), [(40, 30, Hg0, 2, 3), (40, 30, placement(35.0, -2.0, -0.01), 3, 2)])
    case["planted"][0] = plant_at(case["layers"][0], Hg0, (45.0, 15.0))
    return case


def white17():
    """sixteen() with every picture entirely 255: the packed sums hold 17 x 255 = 4335 where all are present."""
    case = sixteen()
    case["center"] = np.full_like(case["center"], 255)
    case["layers"] = [l._replace(img=np.full_like(l.img, 255)) for l in case["layers"]]
    return case


def two_pixels():
    """The smallest pictures: a centre of 2 x 1 pixels, sources of 2 x 1 and 1 x 2 pixels (width x height) magnified four
    times, through meshes of 1 x 2 and 2 x 1 cells."""
    specs = [(2, 1, np.array([[4.0, 0.0, 1.5], [0.0, 4.0, 0.5], [0.0, 0.0, 1.0]]), 1, 2),
             (1, 2, np.array([[4.0, 0.0, -2.5], [0.0, 4.0, -3.5], [0.0, 0.0, 1.0]]), 2, 1)]
    return build(2, (2, 1), specs)


HOST_CASES = {"cross": cross, "strip259": lambda: strip_edges(259), "strip517": lambda: strip_edges(517), "sixteen": sixteen,
              "shared": shared_source}

# the tiling's edges that HOST_CASES do not reach; tests/test_panorama_host.py shows that each reaches its own
TILING_CASES = {"wide": wide, "exact": exact, "black_outside": black_outside, "white17": white17, "two_pixels": two_pixels}

_cache = {}


def get(name):
    """The case ``name`` of HOST_CASES or TILING_CASES with ``oracle``: every layer's canvas by the oracle's ``local_warp`` (float32 inverses
    of the cells, then the vectorised pixel loop).  Built once per session and shared: treat it as read-only."""
    if name not in _cache:
        from oracle import apap_oracle as O
        case = (HOST_CASES.get(name) or TILING_CASES[name])()
        case["oracle"] = [O.local_warp_fast(l.img, O.invert_cells_f32(l.local_homography), l.mesh, l.final_size, l.offset)
                          for l in case["layers"]]
        _cache[name] = case
    return _cache[name]
