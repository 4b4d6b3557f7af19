"""The seeded pictures and named edges of the image pyramid's tests (tests/test_pyramid_inputs.py asserts, from the
specification alone, that each reaches its edge; tests/test_gpu_pyramid.py runs them on the GPU).

The kernel's source tile is 64 x 32 (w x h).  A level exists from 32 pixels a side, so a picture of 32 .. 35 has level 0
alone (the grey plane), and 43 .. 46 are the smallest sides whose 3/4 level exists: they give that level's source every
residue mod 4."""
import numpy as np

import corner_spec

TILE_W, TILE_H = 64, 32


def noise(shape, seed):
    """Seeded noise, lightly smoothed so that the levels keep corners; BGR when the shape says so."""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 256, tuple(shape[:2]) + (shape[2] if len(shape) == 3 else 1,)).astype(np.int64)
    a = (a + np.roll(a, 1, axis=1) + np.roll(a, 1, axis=0)) // 3
    return a.astype(np.uint8).reshape(shape)


def framed(h, w):
    """The two outermost rows and columns 255 on 0: a reflected tap reads 255 where a replicated border would not."""
    a = np.zeros((h, w), np.uint8)
    a[:2], a[-2:], a[:, :2], a[:, -2:] = 255, 255, 255, 255
    return a


def unequal_bgr(h, w, seed):
    """Three planes of unlike content, so that a swapped channel or weight changes the grey plane."""
    a = noise((h, w, 3), seed)
    a[:, :, 0] //= 3
    a[:, :, 2] = 255 - a[:, :, 2] // 2
    return a


def cases():
    """name -> picture.  Every picture is at least 32 a side."""
    out = {}
    for s in (32, 33, 34, 35):                      # level 0 alone: the grey copy at every alignment of the rows
        out[f"side{s}"] = noise((s, s), s)
    for s in (43, 44, 45, 46):                      # Q's source at every residue mod 4; H of odd and even sides
        out[f"side{s}"] = noise((s, s + 4), s)
    for s in (63, 64, 65):                          # one pixel either side of the tile's width, twice its height
        out[f"side{s}"] = noise((s, s), s)
    out["past_tile_w"] = noise((40, 2 * TILE_W + 1), 1)       # a third tile column of one pixel
    out["past_tile_h"] = noise((3 * TILE_H + 1, 50), 2)       # a fourth tile row of one pixel
    out["strip"] = noise((32, 300), 3)
    out["white"] = np.full((70, 90), 255, np.uint8)
    out["black"] = np.zeros((70, 90), np.uint8)
    out["framed"] = framed(66, 71)
    out["bgr"] = unequal_bgr(67, 91, 4)
    out["bgr_wide"] = unequal_bgr(45, 2 * TILE_W + 3, 5)      # BGR rows that start at every byte alignment
    out["scene"] = corner_spec.prototype_scene()              # 200 x 260: six levels, corners on all of them
    return out


def batch():
    """Five pictures of unequal shapes and channel counts behind a first picture that stops at level 0 + 1 = one level."""
    c = cases()
    return [noise((40, 41), 6), c["bgr"], c["side64"], c["strip"], unequal_bgr(50, 86, 7), c["scene"]]


def scaled_pair(reductions=(2, 4), side=720, seed=11):
    """One seeded scene of `side` pixels area-reduced by the two factors: a pair of relative scale reductions[1] /
    reductions[0], the second picture the coarser.  Box-blurred noise with flat rectangles at several sizes, so that there
    are corners at every scale."""
    rng = np.random.default_rng(seed)
    g = rng.integers(0, 256, (side + 8, side + 8)).astype(np.int64)
    g = sum(g[dy:dy + side, dx:dx + side] for dy in range(9) for dx in range(9)) // 81
    g = (g - g.min()) * 255 // max(1, g.max() - g.min())
    for _ in range(side // 4):
        y, x = int(rng.integers(0, side - 12)), int(rng.integers(0, side - 12))
        hh, ww = int(rng.integers(8, side // 6)), int(rng.integers(8, side // 6))
        g[y:y + hh, x:x + ww] = int(rng.integers(0, 256))
    out = []
    for r in reductions:
        n = side // r
        out.append((g[:n * r, :n * r].reshape(n, r, n, r).sum(axis=(1, 3)) // (r * r)).astype(np.uint8))
    return out
