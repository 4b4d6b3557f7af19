#!/usr/bin/env python3
"""Generate tests/golden/image_warp_ref.npz FROM THE REFERENCE'S OWN image_warping (pyviz/utils.py:93-127).

Run in the build container only (``/root/reference`` must be mounted):

    python tests/golden/make_image_warp_golden.py

It imports the reference's ``utils.py`` in place (nothing is copied), runs its ``image_warping`` on small seeded inputs in
both blend modes, and stores the inputs, ``H``, the canvases and the bounds.  The committed ``.npz`` is data; this script
is how it was made.

What the fixture pins and what it does not.  OpenCV is not installed here, so an in-memory module named ``cv2`` is
registered whose ``perspectiveTransform`` and ``warpPerspective`` are those of ``tests/image_warp_spec.py`` (the
specification of this repository's definition: OpenCV 4.x's fixed-point bilinear warp, restated).  The fixture therefore
pins the parts that are the REFERENCE'S OWN code - the bounds arithmetic (``np.int32(pts.min(...) - 0.5)``), ``Ht.dot(H)``,
the paste, and the blend loop with its ``any(...)`` rule and truncating float32 mean - around a ``warpPerspective`` that is
the specification's.  It is not a pin against OpenCV itself (DESIGN.md "Global warp and blend").
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference/pyviz"
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.join(REPO, "tests"))

import image_warp_spec as S  # noqa: E402


seen = []      # (M, size) of every warpPerspective call the reference made


def import_reference():
    cv2 = types.ModuleType("cv2")
    cv2.perspectiveTransform = S.perspective_transform

    def warpPerspective(src, M, size):
        seen.append((M, size))
        return S.warp_perspective(src, M, size)

    cv2.warpPerspective = warpPerspective
    cv2.DMatch = type("DMatch", (), {})        # utils.py:153 names them in an annotation at import time
    cv2.KeyPoint = type("KeyPoint", (), {})
    sys.modules["cv2"] = cv2
    sys.path.insert(0, REF)
    cwd = os.getcwd()
    os.chdir(REF)
    try:
        import utils as ref_utils  # noqa: E402
    finally:
        os.chdir(cwd)
    return ref_utils


def pictures(rng):
    """A 40 x 50 base and a 37 x 45 source: random bytes, the source with a black block (inside every footprint: the blend
    takes the base there), a block whose pixels have exactly one non-zero channel (the ``any(...)`` rule), some of value 1
    (odd sums for the truncating mean), and single black and single-channel pixels scattered among the random ones."""
    base = rng.integers(0, 256, (40, 50, 3), dtype=np.uint8)
    src = rng.integers(1, 256, (37, 45, 3), dtype=np.uint8)
    src[10:18, 12:22] = 0
    one = np.zeros((8, 10, 3), np.uint8)
    ch = rng.integers(0, 3, (8, 10))
    val = rng.integers(1, 256, (8, 10)).astype(np.uint8)
    val[::2, ::3] = 1
    np.put_along_axis(one, ch[..., None], val[..., None], axis=-1)
    src[22:30, 20:30] = one
    for _ in range(40):
        y, x = rng.integers(0, 37), rng.integers(0, 45)
        src[y, x] = 0
        y, x = rng.integers(0, 37), rng.integers(0, 45)
        src[y, x] = 0
        src[y, x, rng.integers(0, 3)] = 1
    return base, src


def homographies():
    c, s = np.cos(0.07), np.sin(0.07)
    return {
        # a negative translation: the canvas grows to the left and up, the base picture sits at a positive offset
        "neg_f64": np.array([[1.04 * c, -1.04 * s, -7.3], [1.04 * s, 1.04 * c, -5.6], [0.0, 0.0, 1.0]], np.float64),
        # a positive translation, float32 as cv.findHomography's result becomes after model.py's tail
        "pos_f32": np.array([[0.97 * c, 0.97 * s, 11.25], [-0.97 * s, 0.97 * c, 6.5], [0.0, 0.0, 1.0]], np.float32),
        # a perspective row
        "persp_f64": np.array([[1.02, 0.03, -4.2], [-0.02, 0.98, 3.7], [6.0e-4, -9.0e-4, 1.0]], np.float64),
        # a perspective row and both signs of translation, float32
        "persp_f32": np.array([[0.95, -0.06, 9.6], [0.05, 1.07, -8.9], [-1.1e-3, 7.0e-4, 1.0]], np.float32),
    }


def main():
    ref = import_reference()
    if not hasattr(np, "int"):
        np.int = int
    rng = np.random.default_rng(20240611)
    base, src = pictures(rng)
    out = {"base": base, "src": src, "names": np.array(list(homographies()))}
    for name, H in homographies().items():
        out[f"H_{name}"] = H
        seen.clear()
        ref.image_warping(base, src, H, True)
        # the bounds the reference computed (utils.py:101-107), read back from what it handed to warpPerspective: the size
        # is (xmax - xmin, ymax - ymin), and with H[2, 2] = 1 the last column of Ht.dot(H) is H's plus t = (-xmin, -ymin)
        M, size = seen[-1]
        assert H[2, 2] == 1
        t = np.rint(np.asarray(M, np.float64)[:2, 2] - np.asarray(H, np.float64)[:2, 2]).astype(np.int64)
        out[f"bounds_{name}"] = np.array([-t[0], -t[1], size[0] - t[0], size[1] - t[1]], np.int32)
        out[f"M_{name}"] = np.asarray(M)
        for mode, direct in (("direct", True), ("mean", False)):
            canvas = ref.image_warping(base, src, H, direct)
            assert canvas.dtype == np.uint8 and canvas.shape == (size[1], size[0], 3)
            out[f"{mode}_{name}"] = canvas
            print(name, mode, canvas.shape, "non-black pixels:", int(canvas.any(axis=-1).sum()))
    path = os.path.join(HERE, "image_warp_ref.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
