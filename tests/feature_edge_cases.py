"""Inputs that reach the edges of the feature front end's kernels (csrc/apap_corner.hip, apap_sift.hip) which the byte-level
suites do not: test infrastructure shared by tests/test_feature_edge_inputs.py, which asserts from the numpy specifications
alone that every input reaches its edge, and tests/test_gpu_feature_edges.py, which runs them on the GPU."""
import numpy as np

import sift_spec

DENSE_PATTERN = [[0, 0, 0, 255], [255, 0, 255, 255], [255, 255, 255, 0], [0, 255, 0, 0]]


def dense_image():
    """96 x 128, a 4 x 4 pattern tiled: at radius 1 two 32 x 64 tiles hold 512 corners each, the tile's bound
    ceil(32 / 2) ceil(64 / 2) and the length of the block's corner list, and most corners share one response."""
    return np.tile(np.array(DENSE_PATTERN, np.uint8), (24, 32))


def binary_image(h=256, w=320, seed=0):
    """0 / 255 noise: responses above 2^48 (the radix select's top digit is not 0) and more than 4096 corners at radius 1."""
    return (np.random.default_rng(seed).integers(0, 2, (h, w)) * 255).astype(np.uint8)


STRUCTURED_SHAPE = (40, 50)


def structured_images():
    """Name -> 40 x 50 grey image whose blurred gradients are exactly zero in one axis, equal in both, or zero in both over
    large regions, next to saturated descriptor rows: the octant branches of the kernel's atan2 with exact values."""
    h, w = STRUCTURED_SHAPE
    yy, xx = np.mgrid[:h, :w]
    out = {}
    g = np.full((h, w), 20, np.uint8)
    g[:, 25:] = 230
    out["vertical step"] = g
    g = np.full((h, w), 20, np.uint8)
    g[20:, :] = 230
    out["horizontal step"] = g
    out["ramp"] = np.clip(5 * xx, 0, 255).astype(np.uint8)
    out["diagonal step"] = np.where(xx - 5 > yy, 230, 20).astype(np.uint8)
    g = np.zeros((h, w), np.uint8)
    g[20, 25] = 255
    out["bright pixel"] = g
    return out


STEP_IMAGES = ("vertical step", "horizontal step", "diagonal step")


def every_pixel_and_a_ring(h, w):
    """(x, y) float32 keypoints at every pixel, then the points 1 and 2 px outside the image, rings included at their corners."""
    yy, xx = (a.ravel() for a in np.mgrid[-2:h + 2, -2:w + 2])
    inside = (yy >= 0) & (yy < h) & (xx >= 0) & (xx < w)
    pts = np.stack([xx, yy], -1).astype(np.float32)
    return np.concatenate([pts[inside], pts[~inside]])


def gradient_classes(img, taps=None):
    """The numbers of interior pixels with dx == 0 != dy, dy == 0 != dx, |dx| == |dy| != 0 and dx == dy == 0, from the base
    image's central differences as sift_spec.describe takes them (float32, the taps the specification defaults to)."""
    taps = sift_spec.taps_f64().astype(np.float32) if taps is None else np.asarray(taps, np.float32)
    base = sift_spec.blur_full(sift_spec.grey(img), taps)
    dx = base[1:-1, 2:] - base[1:-1, :-2]
    dy = base[:-2, 1:-1] - base[2:, 1:-1]
    return {"dx0": int(np.count_nonzero((dx == 0) & (dy != 0))), "dy0": int(np.count_nonzero((dy == 0) & (dx != 0))),
            "diag": int(np.count_nonzero((np.abs(dx) == np.abs(dy)) & (dx != 0))), "both0": int(np.count_nonzero((dx == 0) & (dy == 0)))}


def bgr(g):
    """A grey image as BGR with three equal planes: the integer grey conversion gives the plane back."""
    return np.ascontiguousarray(np.stack([g] * 3, -1))


def batch_images(n, seed=0):
    """n small images of mixed shapes, 7 x 7 up to 40 x 50, grey and BGR in turn, seeded noise smoothed along x."""
    rng = np.random.default_rng(seed)
    shapes = [(7, 7), (40, 50), (9, 31), (23, 8), (16, 16), (7, 50), (40, 7), (12, 19), (33, 20)]
    imgs = []
    for m in range(n):
        h, w = shapes[m % len(shapes)]
        shape = (h, w, 3) if m % 2 else (h, w)
        a = rng.integers(0, 256, shape).astype(np.int64)
        imgs.append(((a + np.roll(a, 1, axis=1)) // 2).astype(np.uint8))
    return imgs
