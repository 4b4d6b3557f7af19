"""Inputs that reach the edges of the orientation kernel (csrc/apap_sift_orient.hip): test infrastructure shared by
tests/test_sift_orient_inputs.py, which asserts from the numpy specification alone that every input reaches its edge, and
tests/test_gpu_sift_orient.py, which runs them on the GPU.  ``cases()`` is hashed there, so that neither file can drift."""
import hashlib

import numpy as np

import feature_edge_cases as E

F32 = np.float32


def beside(values, ulps=(-1, 0, 1)):
    """Every value and its float32 neighbours at the given distances in ulps, those inside [0, 360] only."""
    out = []
    for v in values:
        for u in ulps:
            x = F32(v)
            for _ in range(abs(u)):
                x = np.nextafter(x, F32(np.inf if u > 0 else -np.inf), dtype=F32)
            if 0 <= x <= 360:
                out.append(x)
    return np.array(out, F32)


# cos(ori) = 3 / 4: (j cos) / 1.5 + 1.5 is -1, 0, 3 and 4 at j = -5, -3, 3, 5 - exactly or within an ulp, as the float32 cos falls
ORI_34 = float(np.degrees(np.arccos(0.75)))
# angles (found by a seeded search over the specification) at which a bin coordinate lies one ulp of the rotated coordinate,
# 2^-22, below and above -1 (the sum r_rot + 1.5 is exact there, so nothing closer exists) and one float32 beside 4
NEAR_ANGLES = [6.45019388, 9.06110954, 30.4196644, 36.0340958, 79.4737549, 69.6359024, 159.635895, 339.635895]
SPECIAL_ANGLES = np.concatenate([beside([0, 90, 180, 270, 360, 45]), beside(NEAR_ANGLES, (0,)),
                                 beside([360 - ORI_34, ORI_34, 90 - ORI_34, 270 + ORI_34, 180 - ORI_34], range(-2, 3))])


def tie_image():
    """13 x 13, one bright column: the base image is exactly symmetric about it and the same in every row, so dy = 0 and
    dx(6 + d) = -dx(6 - d) bit for bit.  A keypoint one row above or below the image on that column has one row of valid samples:
    bins 0 and 18 hold the same two terms added in either order - exactly equal, and the first must win."""
    g = np.zeros((13, 13), np.uint8)
    g[:, 6] = 200
    return g


def seeded(h, w, channels, seed):
    rng = np.random.default_rng(seed)
    shape = (h, w, 3) if channels == 3 else (h, w)
    a = rng.integers(0, 256, shape).astype(np.int64)
    return ((a + np.roll(a, 1, axis=1) + np.roll(a, 1, axis=0)) // 3).astype(np.uint8)


def given_angles(n, seed=0):
    """n angles for the given-angle form: the special ones in turn, then seeded ones in [0, 360)."""
    rng = np.random.default_rng(seed)
    a = rng.uniform(0, 360, n).astype(F32)
    a[a >= 360] = 0
    k = min(n, len(SPECIAL_ANGLES))
    a[:k] = SPECIAL_ANGLES[:k]
    return a


def cases():
    """name -> (img, pts (n, 2) float32, angles (n,) float32 for the given-angle form)."""
    out = {}
    h, w = E.STRUCTURED_SHAPE
    pts = E.every_pixel_and_a_ring(h, w)
    for name, g in E.structured_images().items():
        out[name] = (g, pts, given_angles(len(pts), len(out)))
    for name, g in (("flat 13 x 13", np.full((13, 13), 77, np.uint8)), ("bright column 13 x 13", tie_image()),
                    ("seeded 13 x 13", seeded(13, 13, 1, 1)), ("seeded 13 x 40 BGR", seeded(13, 40, 3, 2)),
                    ("seeded 40 x 13", seeded(40, 13, 1, 3))):
        p = E.every_pixel_and_a_ring(*g.shape[:2])
        out[name] = (g, p, given_angles(len(p), len(out)))
    # every special angle at keypoints well inside a textured image, where all 121 samples are valid
    g = seeded(40, 50, 1, 4)
    n = len(SPECIAL_ANGLES)
    p = np.stack([10 + np.arange(n) % 30, 8 + np.arange(n) % 23], -1).astype(F32)
    out["special angles inside"] = (g, p, SPECIAL_ANGLES.copy())
    return out


def digest(cs):
    m = hashlib.sha256()
    for name in sorted(cs):
        m.update(name.encode())
        for a in cs[name]:
            m.update(str(a.shape).encode() + str(a.dtype).encode() + np.ascontiguousarray(a).tobytes())
    return m.hexdigest()


def quarter_turn_pair(h=120, w=150, seed=11, max_corners=400, radius=3, quality_permille=1):
    """A seeded scene of flat rectangles on blurred noise, its quarter turn (``np.rot90``), the first picture's corners
    (``corner_spec.detect``) at least 12 px inside, and the same points in the second picture: pixel (y, x) of an (h, w) image
    lies at (w - 1 - x, y) after the turn.  Returns (img, turned, pts, turned_pts), keypoints (x, y) float32.  The seed is one
    at which no orientation sample has ang / 10 exactly on a half (rint to even is not equivariant under the turn: 4.5 -> 4,
    13.5 -> 14); tests/test_sift_orient_spec.py asserts that."""
    import corner_spec
    img = corner_spec.prototype_scene(h, w, seed)
    pts = corner_spec.detect(img, max_corners, radius, quality_permille)[0].astype(F32)
    x, y = pts[:, 0], pts[:, 1]
    pts = pts[(x >= 12) & (x <= w - 13) & (y >= 12) & (y <= h - 13)]
    turned = np.ascontiguousarray(np.rot90(img))
    turned_pts = np.stack([pts[:, 1], w - 1 - pts[:, 0]], -1).astype(F32)
    assert all(turned[int(q[1]), int(q[0])] == img[int(p[1]), int(p[0])] for p, q in zip(pts, turned_pts))
    return img, turned, pts, turned_pts


def partner_share(feats_a, feats_b):
    """The share of rows of ``feats_a`` whose nearest row of ``feats_b`` (squared distance, the first among equals) is their own."""
    a, b = feats_a.astype(np.float64), feats_b.astype(np.float64)
    d = (a * a).sum(1)[:, None] - 2 * a @ b.T + (b * b).sum(1)[None, :]
    return float(np.mean(np.argmin(d, axis=1) == np.arange(len(a))))
