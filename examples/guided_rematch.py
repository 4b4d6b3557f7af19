#!/usr/bin/env python3
"""Re-matching under the global homography, on a synthetic pair of pictures full of look-alikes (an illustration, not a test).

The centre picture is one 64 x 64 tile of random rectangles repeated over 480 x 640 ("roofs") under a little noise of its own;
the other picture is the same scene shifted by (13, 7) pixels under fresh noise.  Unguided nearest-neighbour matching pairs a
corner with the same corner of ANY tile; after ``find_homography`` on those matches, ``guided.rematch`` searches each centre
corner's partner only within ``em_radius`` of where the homography puts it - what the reference's ``recompute_matching``
docstring asks for.  Printed: matches and RANSAC inliers (5 px) before and after.

    python examples/guided_rematch.py [seed]
"""
import os
import sys
from types import SimpleNamespace

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from cvx_proj_amd import features, guided  # noqa: E402
from cvx_proj_amd.baseline_stitch_test import find_homography  # noqa: E402
from cvx_proj_amd.spectral_method import cv_to_array  # noqa: E402


def pictures(seed, h=480, w=640, shift=(13, 7)):
    rng = np.random.default_rng(seed)
    tile = np.full((64, 64), 90.0)
    for _ in range(6):
        y, x, a, b = rng.integers(0, 48, 2).tolist() + rng.integers(8, 16, 2).tolist()
        tile[y:y + a, x:x + b] = rng.integers(30, 230)
    scene = np.tile(tile, ((h + shift[1]) // 64 + 1, (w + shift[0]) // 64 + 1))[:h + shift[1], :w + shift[0]]
    scene = scene + rng.normal(0, 2.0, scene.shape)      # what tells one tile from the next: not much
    centre = scene[:h, :w] + rng.normal(0, 1.0, (h, w))
    other = scene[shift[1]:, shift[0]:] + rng.normal(0, 1.0, (h, w))
    as_u8 = lambda a: np.clip(np.rint(a), 0, 255).astype(np.uint8)      # noqa: E731
    return as_u8(centre), as_u8(other)


def inliers(kpts_cp, kpts_op, matches):
    """(H other -> centre or None, RANSAC inliers at 5 px) of the matches."""
    if len(matches) < 4:
        return None, 0
    pts_c, pts_o = cv_to_array(kpts_cp, kpts_op, matches)
    H, mask = find_homography(pts_o, pts_c, 5.0)
    return H, int(mask.sum())


def main(seed=0):
    c_img, o_img = pictures(seed)
    kc, fc, ko, fo, matches = features.detect_and_match(c_img, o_img, max_corners=1500)
    H, n_in = inliers(kc, ko, matches)
    print(f"unguided: {len(matches)} matches, {n_in} RANSAC inliers")
    if H is None:
        raise SystemExit("no homography from the unguided matches")
    opts = SimpleNamespace(em_radius=6.0, score_thresh=0.4)
    kc, fc, ko, fo, again = guided.rematch(kc, fc, ko, fo, H, opts)
    _, n_again = inliers(kc, ko, again)
    print(f"rematch under H at {opts.em_radius} px: {len(again)} matches, {n_again} RANSAC inliers")
    print("H (other -> centre):\n", H)


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 0)
