// How the feature front end reads a uint8 image on the device: the one definition of the index reflection and of the grey
// conversion that the corner detector (apap_corner.hip) and the descriptor extraction (apap_sift.hip) share.  The detector
// and the descriptor must see the same grey image, bit for bit: tests/corner_spec.py and tests/sift_spec.py restate both
// steps in numpy.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace apap {

// reflect-101, once, then clamped.  One reflection is all that either caller needs, for images of 7 pixels a side or more:
//   k_sift_describe: a valid sample reads indices -6 .. n + 5 only, which reflect once into 0 .. n - 1 for n >= 7; the clamp
//     keeps what an invalid sample would read (and never uses) inside the image;
//   k_sift_orient (apap_sift_orient.hip): its 25 x 25 patch reads -12 .. n + 11, one reflection for n >= 13, its smallest side;
//   k_corner_tile: positions more than one pixel outside the image are staged but never used (a gradient outside the image
//     is taken at its reflection, whose Sobel window reaches one pixel outside at most).
__device__ __forceinline__ int reflect(int i, int n) {
    if (i < 0) i = -i;
    if (i > n - 1) i = 2 * (n - 1) - i;
    return min(max(i, 0), n - 1);
}

// The grey value of pixel (y, x) of an image w pixels wide with c = 1 (grey) or 3 (BGR) interleaved channels: the uint8 as it
// is, or (3735 B + 19235 G + 9798 R + 16384) >> 15 in integers.
__device__ __forceinline__ int grey_at(const uint8_t *img, int y, int x, int w, int c) {
    const uint8_t *p = img + ((size_t)y * w + x) * c;
    int g = p[0];
    if (c == 3) g = (3735 * g + 19235 * (int)p[1] + 9798 * (int)p[2] + 16384) >> 15;
    return g;
}

}  // namespace apap
