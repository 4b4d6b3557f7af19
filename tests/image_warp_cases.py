"""Case set E of the global warp and blend: the inputs at the kernel's edges, shared by tests/test_gpu_image_warp.py (which
runs them on the GPU) and tests/test_image_warp_host.py (which checks, without a GPU, that each input does exercise the
edge it is named for).  A case is (name, img_base, img2warp, H); every canvas is under 200 x 200."""
import os

import numpy as np

import image_warp_spec as S

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _pic(rng, h, w, lo=0):
    return rng.integers(lo, 256, (h, w, 3), dtype=np.uint8)


def translation(tx, ty, dtype=np.float64):
    return np.array([[1, 0, tx], [0, 1, ty], [0, 0, 1]], dtype)


def w0_line(delta):
    """H whose inverse has the third row (-1/8, 0, 2 + delta): W0 = 0 on the canvas column x = 16 for delta = 0 (every entry a
    power of two: the cofactor inverse is exact); a small delta puts the zero just beside that column, where 32 / W0 is huge."""
    c = 2.0 + delta
    return np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.125 / c, 0.0, 1.0 / c]])


def cases():
    rng = np.random.default_rng(77)
    ref = np.load(os.path.join(GOLDEN, "image_warp_ref.npz"))
    out = [(f"fixture_{n}", ref["base"], ref["src"], ref[f"H_{n}"]) for n in ref["names"]]
    frac = translation(0.3, 0.4)
    # canvas widths around the 4-pixel store: 4k + 1, 4k + 2, 4k + 3, exactly 4, and a canvas 1 px wider than the base
    for w2, w1, name in ((13, 9, "width_4k1"), (14, 9, "width_4k2"), (15, 9, "width_4k3"), (4, 3, "width_4"), (17, 16, "width_base_plus_1")):
        out.append((name, _pic(rng, 5, w1), _pic(rng, 7, w2, 1), frac))
    # more than one block along x (256 pixels a block would be past the 200-pixel limit: several rows of blocks instead)
    out.append(("rows_9", _pic(rng, 9, 30), _pic(rng, 8, 31, 1), frac))
    # tiny sources, spread over a few canvas pixels
    spread = np.array([[3.0, 0.0, 2.5], [0.0, 3.0, 1.25], [0.0, 0.0, 1.0]])
    out.append(("src_1x1", _pic(rng, 6, 5), _pic(rng, 1, 1, 1), spread))
    out.append(("src_1x2", _pic(rng, 6, 5), _pic(rng, 1, 2, 1), spread))
    out.append(("src_2x1", _pic(rng, 6, 5), _pic(rng, 2, 1, 1), spread))
    out.append(("base_1x1", _pic(rng, 1, 1), _pic(rng, 9, 11, 1), spread))
    # identity: every ax = ay = 0 and the tap at sx + 1 = w2 has weight 0
    out.append(("identity", _pic(rng, 17, 21), _pic(rng, 20, 33, 1), np.eye(3)))
    out.append(("translation_int", _pic(rng, 17, 21), _pic(rng, 20, 33, 1), translation(5, -3)))
    out.append(("translation_half", _pic(rng, 17, 21), _pic(rng, 20, 33, 1), translation(0.5, 0.5)))
    # M = diag(64, 64, 1): X = x / 2, k + 0.5 exactly in the odd canvas columns - round half to even
    out.append(("half_ties", _pic(rng, 5, 7), _pic(rng, 2, 3, 1), np.diag([64.0, 64.0, 1.0])))
    # the line W0 = 0 crosses the canvas; just beside it the coordinates pass the int and the int16 clamp, on both sides
    out.append(("w0_zero_line", _pic(rng, 20, 30), _pic(rng, 20, 40, 1), w0_line(0.0)))
    for k, delta in enumerate((2.0 ** -40, -2.0 ** -40, 2.0 ** -17, -2.0 ** -17)):
        out.append((f"clamp_{k}", _pic(rng, 20, 30), _pic(rng, 20, 40, 1), w0_line(delta)))
    # an all-black source: the mean blend takes the base everywhere
    out.append(("src_black", _pic(rng, 12, 14), np.zeros((15, 18, 3), np.uint8), translation(-2.25, 1.5)))
    # every source pixel has one non-zero channel, of value 1: odd sums for the truncating mean, any(...) on a single channel
    one = np.zeros((15, 18, 3), np.uint8)
    np.put_along_axis(one, rng.integers(0, 3, (15, 18, 1)), 1, axis=-1)
    out.append(("src_one_channel", _pic(rng, 12, 14), one, translation(2, 1)))
    # the base picture is the whole canvas: nothing of the source shows in direct mode
    out.append(("base_is_canvas", _pic(rng, 22, 26), _pic(rng, 9, 11, 1), translation(6.5, 7.25)))
    # one H as float32 and as float64
    H32 = np.array([[0.9, 0.1, 3.3], [-0.1, 1.1, -2.7], [1e-3, -2e-3, 1.0]], np.float32)
    b, s = _pic(rng, 19, 23), _pic(rng, 21, 18, 1)
    out.append(("H_float32", b, s, H32))
    out.append(("H_float64", b, s, H32.astype(np.float64)))
    return out


def geometry(base, src, H):
    """(M, canvas_w, canvas_h, off_x, off_y) by the specification."""
    xmin, ymin, xmax, ymax = S.bounds(base.shape[0], base.shape[1], src.shape[0], src.shape[1], H)
    return S.matrix(np.asarray(H), [-xmin, -ymin]), xmax - xmin, ymax - ymin, -xmin, -ymin
