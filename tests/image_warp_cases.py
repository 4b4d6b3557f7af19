"""Case set E of the global warp and blend: the inputs at the kernel's edges, shared by tests/test_gpu_image_warp.py (which
runs them on the GPU) and tests/test_image_warp_host.py (which checks, without a GPU, that each input does exercise the
edge it is named for).  A case is (name, img_base, img2warp, H); every canvas is under 200 x 200.  Below it the sets at the
tiling's edges, which set E does not reach: sweep(), tiling_cases(), many() and tiny_pair()."""
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


# ---------------------------------------------------------------- the tiling sets: caller-chosen geometry, wide canvases, many problems
# k_image_warp's tiling (csrc/apap_image_warp.hip): a lane owns GROUP consecutive pixels of a row, a block COLS_PER_BLOCK
# columns of ROWS_PER_BLOCK rows; a problem takes col_blocks x row_tiles consecutive blocks of the launch.
GROUP, COLS_PER_BLOCK, ROWS_PER_BLOCK = 4, 256, 4

# A problem with caller-chosen geometry is (name, img_base, img2warp, M, (canvas_w, canvas_h), (off_x, off_y), direct): what
# _native.image_warp_batch takes per problem.  Set E above never sets the geometry itself: its offsets are multiples of 4 but
# for two cases, and its canvases one block wide.


def expected(problem):
    """The specification's canvas of a problem with caller-chosen geometry."""
    _, base, src, M, canvas, off, direct = problem
    return S.blend(S.warp_perspective(src, M, canvas), base, off, direct)


def col_blocks(problem):
    return (problem[4][0] + COLS_PER_BLOCK - 1) // COLS_PER_BLOCK


def explicit(name, base, src, H, direct):
    """A case of set E's form as a problem with the geometry the specification derives for it."""
    M, cw, ch, ox, oy = geometry(base, src, H)
    return (name, base, src, M, (cw, ch), (ox, oy), direct)


SWEEP_CANVAS, SWEEP_OFF_Y, SWEEP_BASE_H = (23, 6), 2, 3


def sweep():
    """The base rectangle's left edge at every residue of a lane's group against its right edge at every residue: off_x in
    0 .. 7, base_w in 1 .. 5, on one 23 x 6 canvas, each geometry in both blend modes with one base picture - 80 problems.  The
    source (bytes 1 .. 255) covers the whole canvas through a fractional translation, so every warped pixel is non-zero: a lane
    that skips taps it needs shows black."""
    rng = np.random.default_rng(401)
    src = _pic(rng, 9, 25, 1)
    M = translation(-0.3, -0.4)
    out = []
    for off_x in range(8):
        for base_w in range(1, 6):
            base = _pic(rng, SWEEP_BASE_H, base_w)
            for direct in (True, False):
                out.append((f"sweep_x{off_x}_w{base_w}_{'direct' if direct else 'mean'}", base, src, M, SWEEP_CANVAS,
                            (off_x, SWEEP_OFF_Y), direct))
    return out


def tiny_pair():
    """Both pictures 1 x 1, (img_base, img2warp, H): the source is spread over a 3 x 3 canvas whose pixel (0, 0), where the
    base lies, takes 812 / 1024 of it."""
    rng = np.random.default_rng(11)
    return _pic(rng, 1, 1, 1), _pic(rng, 1, 1, 64), np.array([[3.0, 0.0, 0.4], [0.0, 3.0, 0.3], [0.0, 0.0, 1.0]])


WIDE_SHAPES = ((255, 3), (256, 4), (257, 5), (511, 4), (512, 3), (513, 5), (769, 4))
SMALL_IN_WIDE = ("width_4k1", "src_1x1", "half_ties", "width_4", "rows_9", "base_1x1", "width_4k3")


def tiling_cases():
    """Canvases 255, 256, 257, 511, 512, 513 and 769 wide (1, 1, 2, 2, 2, 3, 4 blocks along a row) and 3, 4, 5 high, in both
    modes, each followed by a small problem of set E, and the pair of 1 x 1 pictures in both modes: a block's index minus its
    problem's first block has to be split by that problem's own col_blocks.  One source 7 x 780 of bytes 1 .. 255 serves the wide
    problems, each through its own fractional translation; the 2-row base straddles column 256 (columns 250 .. 261; 243 ..
    254 where the canvas ends before that), and on the 769 canvas columns 250 .. 519, so whole lanes and a whole block's
    middle lie inside it."""
    rng = np.random.default_rng(402)
    src = _pic(rng, 7, 780, 1)
    by_name = {c[0]: c for c in cases()}
    out = []
    for k, (cw, ch) in enumerate(WIDE_SHAPES):
        base_w = 270 if cw == 769 else 12
        off_x = min(250, cw - base_w)
        base = _pic(rng, 2, base_w)
        small = by_name[SMALL_IN_WIDE[k]]
        for direct in (True, False):
            out.append((f"wide_{cw}x{ch}_{'direct' if direct else 'mean'}", base, src, translation(-0.3 - k, -0.4), (cw, ch), (off_x, 1),
                        direct))
            out.append(explicit(f"{small[0]}_{'direct' if direct else 'mean'}", small[1], small[2], small[3], not direct))
    base, tiny, H = tiny_pair()
    for direct in (True, False):
        out.append(explicit(f"both_1x1_{'direct' if direct else 'mean'}", base, tiny, H, direct))
    return out


MANY = 521


def many():
    """521 (a prime above 512) problems of set E's form, (img_base, img2warp, H, direct_blend), on canvases between 5 x 5 and
    9 x 11: every problem has its own pictures, its own translation (drawn until the canvas has such a size) and its own mode,
    so a block routed to a neighbouring problem writes other bytes.  The descriptor table is 75 KB and the bisection over the
    first blocks ten levels deep."""
    rng = np.random.default_rng(403)
    out = []
    while len(out) < MANY:
        h1, w1, h2, w2 = (int(v) for v in rng.integers(1, 9, 4))
        H = translation(*np.round(rng.uniform(-3.0, 3.0, 2), 3))
        base, src, direct = _pic(rng, h1, w1), _pic(rng, h2, w2, 1), bool(rng.integers(0, 2))
        _, cw, ch, _, _ = geometry(base, src, H)
        if 5 <= cw <= 9 and 5 <= ch <= 11:
            out.append((base, src, H, direct))
    return out
