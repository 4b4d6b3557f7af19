#!/usr/bin/env python3
"""Denoise two pictures that carry periodic noise, then match them: ``denoise.notch_denoise`` (equalise, transform, notch the
noise lattice's harmonics, invert) in front of ``features.matched_arrays_from_images``, whose Harris detector would otherwise
find a field of corners in the noise pattern.

    python examples/denoise_then_match.py centre.npy other.npy [spacing]     # two (h, w, 3) or (h, w) uint8 arrays of one shape

Both sides of the pictures must be 5-smooth lengths (2 .. 4096); ``spacing`` is the lattice's period in the spectrum
(default 48, the reference's: 1 / 8 of its 384-pixel half side).
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from cvx_proj_amd import denoise, features  # noqa: E402


def main(centre_path, other_path, spacing=48):
    c_img, o_img = np.load(centre_path), np.load(other_path)
    before = features.matched_arrays_from_images(c_img, o_img, ratio=0.8)
    if c_img.shape == o_img.shape:      # one call for both pictures
        c_den, o_den = denoise.notch_denoise_batch(np.stack([c_img, o_img]), spacing=spacing, out="uint8")
    else:
        c_den, o_den = (denoise.notch_denoise(m, spacing=spacing, out="uint8") for m in (c_img, o_img))
    # the pictures are equalised already: the detector reads them as they are
    after = features.matched_arrays_from_images(c_den, o_den, ratio=0.8)
    print(f"{len(before[0])} matches on the pictures as they came, {len(after[0])} after notch denoising")
    return after


if __name__ == "__main__":
    if len(sys.argv) not in (3, 4):
        raise SystemExit(__doc__)
    main(sys.argv[1], sys.argv[2], *(int(v) for v in sys.argv[3:]))
