#!/usr/bin/env python3
"""Matching a picture against a copy of itself turned by 30 degrees, without and with keypoint orientation (an illustration,
not a test).

The scene is random rectangles on blurred noise.  The second picture is the first one turned about its centre with the
project's own global warp (``utils.image_warping``, onto a one-pixel base picture, so that the canvas is the turned picture's
bounding box).  Both runs detect the same corners; the unoriented descriptors are taken in the pictures' own axes and find
next to nothing to agree on, the oriented ones (``oriented=True``) are taken in each keypoint's dominant gradient direction.
Printed for both: corners, matches under the ratio test, RANSAC inliers (3 px), and how many matches lie within 3 px of where
the turn really puts them.

    python examples/rotated_pair_match.py [seed] [degrees]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from cvx_proj_amd import _native, features, utils  # noqa: E402
from cvx_proj_amd.baseline_stitch_test import find_homography  # noqa: E402
from cvx_proj_amd.spectral_method import cv_to_array  # noqa: E402


def scene(seed, h=360, w=480, rects=60):
    rng = np.random.default_rng(seed)
    g = rng.integers(0, 256, (h + 4, w + 4)).astype(np.int64)
    g = sum(g[dy:dy + h, dx:dx + w] for dy in range(5) for dx in range(5)) // 25
    for _ in range(rects):
        y, x = int(rng.integers(0, h - 8)), int(rng.integers(0, w - 8))
        g[y:y + int(rng.integers(6, 50)), x:x + int(rng.integers(6, 50))] = int(rng.integers(0, 256))
    return np.ascontiguousarray(np.stack([g.astype(np.uint8)] * 3, -1))


def turned(img, degrees):
    """(the picture turned about its centre, the 3 x 3 map from its own pixels to the turned picture's)."""
    h, w = img.shape[:2]
    a = np.radians(degrees)
    cx, cy = (w - 1) / 2, (h - 1) / 2
    R = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1.0]])
    H = np.array([[1, 0, cx], [0, 1, cy], [0, 0, 1.0]]) @ R @ np.array([[1, 0, -cx], [0, 1, -cy], [0, 0, 1.0]])
    base = np.zeros((1, 1, 3), np.uint8)
    M = _native.image_warp_geometry(1, 1, h, w, H)[0]           # H, then the shift onto the canvas
    return utils.image_warping(base, img, H), M


def report(name, kc, ko, matches, M):
    line = f"{name}: {len(kc)} and {len(ko)} corners, {len(matches)} matches"
    if len(matches) >= 4:
        pts_c, pts_o = cv_to_array(kc, ko, matches)
        _, mask = find_homography(pts_c, pts_o, 3.0)
        at = np.c_[pts_c, np.ones(len(pts_c))] @ M.T
        true = int(np.count_nonzero(np.linalg.norm(at[:, :2] / at[:, 2:] - pts_o, axis=1) <= 3.0))
        line += f", {0 if mask is None else int(mask.sum())} RANSAC inliers, {true} within 3 px of the true turn"
    print(line)


def main(seed=0, degrees=30.0):
    c_img = scene(seed)
    o_img, M = turned(c_img, degrees)
    print(f"{c_img.shape[1]} x {c_img.shape[0]} turned by {degrees} degrees onto {o_img.shape[1]} x {o_img.shape[0]}")
    for name, oriented in (("unoriented", False), ("oriented", True)):
        kc, _, ko, _, matches = features.detect_and_match(c_img, o_img, max_corners=1500, oriented=oriented, ratio=0.8)
        report(name, kc, ko, matches, M)


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 0, float(sys.argv[2]) if len(sys.argv) > 2 else 30.0)
