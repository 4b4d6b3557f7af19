#!/usr/bin/env python3
"""Dehaze two hazy pictures, then match them: ``dehaze.dehaze_batch`` (dark channel prior, guided refinement) in front of
``features.detect_and_match``, beside the reference's own answer to haze, the per-channel equalisation, and no answer at all.

    python examples/dehaze_then_match.py [width height [shift]]

The pair is synthetic: ``cvx_proj_amd/synth.py``'s seeded picture, laid out in blocks so that it has corners, seen twice ``shift``
pixels apart; each view is hazed on its own by ``I = J t + A (1 - t)`` with a depth ramp across the view, so the same point of the
scene carries different haze in the two views.  For each of the three treatments the script prints the corners found in each
view, the matches that pass the ratio test, and how many of them agree with one homography (RANSAC at 3 pixels).  An
illustration, not a test: the counts depend on the scene.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from cvx_proj_amd import _native, dehaze, features  # noqa: E402
from cvx_proj_amd.synth import synth_pair  # noqa: E402

AIRLIGHT = np.array([225.0, 232.0, 240.0])


def hazy_pair(width=640, height=480, shift=24, block=8, seed=7):
    """``(centre, other)`` hazy uint8 views and the haze-free ones."""
    small = synth_pair((width + shift + block - 1) // block, (height + shift + block - 1) // block, 4, 2, seed).img
    scene = np.repeat(np.repeat(small, block, axis=0), block, axis=1)
    clear = [np.ascontiguousarray(scene[shift:shift + height, shift:shift + width]), np.ascontiguousarray(scene[:height, :width])]
    t = np.linspace(0.85, 0.15, width)[None, :, None]
    hazy = [np.floor(v * t + AIRLIGHT * (1.0 - t) + 0.5).astype(np.uint8) for v in clear]
    return hazy, clear


def report(name, c_img, o_img):
    kc, _, ko, _, matches = features.detect_and_match(c_img, o_img, ratio=0.8)
    inliers = 0
    if len(matches) >= 4:
        src = np.array([ko[m.trainIdx].pt for m in matches], dtype=np.float32)
        dst = np.array([kc[m.queryIdx].pt for m in matches], dtype=np.float32)
        inliers = int(np.count_nonzero(_native.find_homography_ransac(src, dst, 3.0)[1]))
    print(f"{name:10s} corners {len(kc):5d} / {len(ko):5d}   matches {len(matches):5d}   RANSAC inliers {inliers:5d}")
    return len(kc), len(ko), len(matches), inliers


def main(width=640, height=480, shift=24):
    (c_hazy, o_hazy), _ = hazy_pair(width, height, shift)
    report("hazy", c_hazy, o_hazy)
    report("equalised", _native.equalize_hist(c_hazy), _native.equalize_hist(o_hazy))
    c_clear, o_clear = dehaze.dehaze_batch(np.stack([c_hazy, o_hazy]))      # one call for both views
    report("dehazed", c_clear, o_clear)


if __name__ == "__main__":
    if len(sys.argv) not in (1, 3, 4):
        raise SystemExit(__doc__)
    main(*(int(v) for v in sys.argv[1:]))
