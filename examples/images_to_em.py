#!/usr/bin/env python3
"""From two uint8 pictures to the robust global homography, with nothing but the pictures: corners, SIFT descriptors and exact
matches (``features``), the fundamental matrix of the matches (``estimate_fundamental``: no calibration spreadsheet), then the
spectral EM loop, whose epipolar score needs that F.

    python examples/images_to_em.py centre.npy other.npy        # two (h, w, 3) or (h, w) uint8 arrays
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from cvx_proj_amd import features, spectral_method as SM  # noqa: E402


def main(centre_path, other_path):
    c_img, o_img = np.load(centre_path), np.load(other_path)
    src, dst, c_feats, o_feats = features.matched_arrays_from_images(c_img, o_img, ratio=0.8)
    F, f_mask = SM.estimate_fundamental(src, dst, thresh=3.0)      # dst_h^T F src_h = 0, |dst^T F src| in pixels
    if F is None:
        raise SystemExit(f"fewer than 8 of the {len(src)} matches agree on an epipolar geometry")
    print(f"{len(src)} matches, {int(f_mask.sum())} within 3 px of their epipolar lines")
    em = SM.spectral_em(src, dst, c_feats, o_feats, F, em_steps=2)
    print("H_save (spectral_method.py:235-236):\n", em.H_save)


if __name__ == "__main__":
    if len(sys.argv) != 3:
        raise SystemExit(__doc__)
    main(sys.argv[1], sys.argv[2])
