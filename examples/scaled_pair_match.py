#!/usr/bin/env python3
"""Matching a picture against a smaller copy of itself, without and with the image pyramid (an illustration, not a test).

The scene is random rectangles on blurred noise, 1440 pixels a side.  It is area-reduced by 2 to make the first picture and
by 4 (relative scale s = 2) or by 3 (s = 1.5) to make the second.  The single-scale run (``levels=None``, the default)
detects corners on the pictures as they are and describes each from its 21 x 21 patch: the same scene point looks unlike
itself at another scale.  The run over the pyramid (``levels=6``) detects and describes on every level of both pictures, so
that a level of the one meets a level of the other at nearly the same scale; its keypoints come back in the pictures' own
frames.  Printed for both: corners, matches under the ratio test, RANSAC inliers (3 px), and how many matches lie within 3 px
of where the reduction really puts them.

    python examples/scaled_pair_match.py [seed]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from cvx_proj_amd import features  # noqa: E402
from cvx_proj_amd.baseline_stitch_test import find_homography  # noqa: E402
from cvx_proj_amd.spectral_method import cv_to_array  # noqa: E402


def scene(seed, side=1440, rects=360):
    rng = np.random.default_rng(seed)
    g = rng.integers(0, 256, (side + 8, side + 8)).astype(np.int64)
    g = sum(g[dy:dy + side, dx:dx + side] for dy in range(9) for dx in range(9)) // 81
    g = (g - g.min()) * 255 // max(1, g.max() - g.min())
    for _ in range(rects):
        y, x = int(rng.integers(0, side - 12)), int(rng.integers(0, side - 12))
        g[y:y + int(rng.integers(8, side // 6)), x:x + int(rng.integers(8, side // 6))] = int(rng.integers(0, 256))
    return g


def reduced(g, r):
    """The scene area-reduced by r: pixel x has its centre at scene coordinate r x + (r - 1) / 2."""
    n = g.shape[0] // r
    return (g[:n * r, :n * r].reshape(n, r, n, r).sum(axis=(1, 3)) // (r * r)).astype(np.uint8)


def report(name, kc, ko, matches, ra, rb):
    line = f"  {name}: {len(kc)} and {len(ko)} keypoints, {len(matches)} matches"
    inliers = 0
    if len(matches) >= 4:
        pts_c, pts_o = cv_to_array(kc, ko, matches)
        _, mask = find_homography(pts_c, pts_o, 3.0)
        inliers = 0 if mask is None else int(mask.sum())
        at = (ra * pts_c.astype(np.float64) + (ra - 1) / 2 - (rb - 1) / 2) / rb
        true = int(np.count_nonzero(np.linalg.norm(at - pts_o, axis=1) <= 3.0))
        line += f", {inliers} RANSAC inliers, {true} within 3 px of the true reduction"
    print(line)
    return inliers


def main(seed=0):
    g = scene(seed)
    c_img = reduced(g, 2)
    for rb in (4, 3):
        o_img = reduced(g, rb)
        print(f"{c_img.shape[1]} x {c_img.shape[0]} against {o_img.shape[1]} x {o_img.shape[0]}: relative scale {rb / 2}")
        got = {}
        for name, levels in (("single scale", None), ("pyramid, 6 levels", 6)):
            kc, _, ko, _, matches = features.detect_and_match(c_img, o_img, max_corners=600, levels=levels, ratio=0.8, cross_check=True)
            got[name] = report(name, kc, ko, matches, 2, rb)
        print(f"  inliers: {got['single scale']} -> {got['pyramid, 6 levels']}")


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 0)
