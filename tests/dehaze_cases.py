"""Inputs of the dehazing's tests: hashed pictures (the same on every numpy, as denoise_cases.picture makes them), four synthetic
hazy scenes ``I = J t + A (1 - t)`` with a depth ramp, and the named edge cases.  tests/test_dehaze_inputs.py asserts from the
specification alone that each named case reaches the edge it is named after; tests/test_gpu_dehaze.py runs the kernels on all."""
import numpy as np

from denoise_cases import picture

from cvx_proj_amd import _native      # its constants need neither the library nor a device

# the kernels' tile sides and the pixels a block of the selection scans at a time (include/apap_hip.h): the cases follow them
TILES = dict(_native.DEHAZE_TILES)
AIR_CHUNK = _native.DEHAZE_AIR_CHUNK
AIR_MAX_BLOCKS = _native.DEHAZE_AIR_MAX_BLOCKS
AIR_PASS = AIR_MAX_BLOCKS * AIR_CHUNK         # pixels the selection's whole grid scans at a time: a larger picture takes passes
AIR_PASSES_SHAPE = (1027, 1025)               # 1 052 675 pixels: a second pass of five chunks, the last one of three pixels

DEFAULTS = dict(radius=7, omega_q=243, t0_q=410, refine=30, eps=64)


def blocks(h, w, seed, side, channels=3):
    """A hashed picture of ``side`` x ``side`` blocks of one colour: structure for the guide to follow."""
    small = picture((h + side - 1) // side, (w + side - 1) // side, seed, channels)
    return np.ascontiguousarray(np.repeat(np.repeat(small, side, axis=0), side, axis=1)[:h, :w])


# ---- synthetic hazy scenes: name -> (h, w, radius, refine, seed, block side)
SCENES = {
    "scene_96x128": (96, 128, 7, 30, 101, 6),
    "scene_60x50": (60, 50, 3, 8, 102, 4),
    "scene_40x200": (40, 200, 15, 32, 103, 5),
    "scene_33x33": (33, 33, 1, 1, 104, 3),
}
SCENE_A = np.array([225, 232, 240], dtype=np.float64)       # BGR: a slightly blue haze


def scene(name):
    """``(J, I, t, params)``: the haze-free picture, the hazy picture, the true transmission (float64 (h, w)), and the integer
    parameters.  The transmission falls along the columns from 0.9 to 0.08 (the far end is all haze: where A is found)."""
    h, w, radius, refine, seed, side = SCENES[name]
    J = blocks(h, w, seed, side)
    t = np.broadcast_to(np.linspace(0.9, 0.08, w)[None, :], (h, w))
    I = np.floor(J * t[..., None] + SCENE_A * (1.0 - t[..., None]) + 0.5).astype(np.uint8)
    return J, I, t, dict(DEFAULTS, radius=radius, refine=refine)


# ---- named edge cases: name -> (picture, parameters)
def _levels(h, w, levels, base=10, spread=100, seed=7):
    """A grey-free BGR picture for radius 0 whose dark channel is exactly ``levels`` at the first pixels of rows 1, 3, 5, ...
    and below ``spread + base`` elsewhere: the histogram's upper end is the test's to place."""
    img = (picture(h, w, seed, 3) % spread + base).astype(np.uint8)
    for k, v in enumerate(levels):
        img[2 * k + 1, 3 * k] = (v, min(v + 3, 255), min(v + 5, 255))
    return img


def _noise(h, w, seed, channels=0):
    """0 / 255 noise."""
    return ((picture(h, w, seed, channels) >> 7) * 255).astype(np.uint8)


def _step(h, w, channels=0):
    """0 | 255, the edge in the middle column."""
    img = np.zeros((h, w, channels) if channels else (h, w), dtype=np.uint8)
    img[:, w // 2:] = 255
    return img


def _two_best(h, w):
    img = (picture(h, w, 9, 3) % 100).astype(np.uint8)
    img[0, 0] = (250, 240, 230)
    img[-1, -1] = (230, 240, 250)
    return img


def air_place(i, n_pixels):
    """(block, pass, pixels of its chunk) of pixel ``i`` in the selection's scan of ``n_pixels`` pixels: block b takes the
    chunks b, b + grid, b + 2 grid, ... of AIR_CHUNK consecutive pixels, grid = min(chunks, AIR_MAX_BLOCKS)."""
    chunks = (n_pixels + AIR_CHUNK - 1) // AIR_CHUNK
    grid = min(chunks, AIR_MAX_BLOCKS)
    chunk = i // AIR_CHUNK
    return chunk % grid, chunk // grid, min(AIR_CHUNK, n_pixels - chunk * AIR_CHUNK)


AIR_TIES_AT = (7, AIR_PASS + 7, AIR_PASS + AIR_CHUNK + 3)      # block 0's first pass, block 0's second, block 1's second


def _marked(h, w, seed, marks):
    """A dim background (channels 10 .. 109) with the pixels of ``marks`` (flat index -> colour) far brighter."""
    img = (picture(h, w, seed, 3) % 100 + 10).astype(np.uint8)
    flat = img.reshape(-1, 3)
    for at, colour in marks.items():
        flat[at] = colour
    return img


def _floor_clips(h, w):
    """A bright plain with single pixels darker and (in two channels) brighter than A: the refinement, close to a box mean under
    the largest eps, holds t on the floor at them, and the recovery leaves 0 .. 255 on both sides."""
    img = np.full((h, w, 3), 250, dtype=np.uint8)
    img[5, 7] = (255, 250, 250)                     # A: the largest sum among the candidates
    for k in range(4):
        img[12 + 9 * k, 10 + 11 * k] = (0, 3, 90)
        img[14 + 9 * k, 40 - 6 * k] = (240, 255, 253)
    return img


def _constant(h, w, colour):
    return np.ascontiguousarray(np.broadcast_to(np.array(colour, dtype=np.uint8), (h, w, len(colour))))


def cases():
    """name -> (picture, integer parameters)."""
    P = lambda **kw: dict(DEFAULTS, **kw)      # noqa: E731
    out = {
        # shapes
        "one_pixel": (picture(1, 1, 1, 3), P()),
        "row_1x40": (picture(1, 40, 2, 3), P()),
        "col_40x1": (picture(40, 1, 3), P()),
        "all_clamped_5x7": (picture(5, 7, 4, 3), P(radius=7, refine=32)),
        # windows
        "radius0_refine0": (picture(40, 50, 5, 3), P(radius=0, refine=0)),
        "radius1_refine1": (blocks(40, 50, 6, 4), P(radius=1, refine=1)),
        "defaults_40x50": (blocks(40, 50, 7, 5), P()),
        "radius32_refine32": (blocks(40, 50, 8, 5), P(radius=32, refine=32)),
        "grey_refine0": (blocks(37, 41, 10, 3, channels=0), P(radius=1, refine=0)),
        # atmospheric light
        "air_k1": (picture(20, 30, 11, 3), P(radius=2, refine=3)),
        "air_exact": (_levels(50, 60, (250, 220, 200)), P(radius=0, refine=2)),
        "air_jump": (_levels(50, 60, (250, 250, 200, 200, 200, 200, 200)), P(radius=0, refine=2)),
        "air_constant": (_constant(70, 70, (100, 150, 200)), P(radius=3, refine=4)),
        "air_two_best": (_two_best(40, 40), P(radius=0, refine=0)),
        "air_black": (np.zeros((33, 35, 3), np.uint8), P(radius=2, refine=2)),
        # more pixels than the selection's grid scans at once: the only bright pixel is the last one, in the second pass's
        # partial chunk; and three equally bright ones in different passes and blocks, the first of which must win
        "air_second_pass": (_marked(*AIR_PASSES_SHAPE, 19, {AIR_PASSES_SHAPE[0] * AIR_PASSES_SHAPE[1] - 1: (250, 252, 255)}),
                            P(radius=0, refine=1)),
        "air_ties_across_passes": (_marked(*AIR_PASSES_SHAPE, 20, dict(zip(AIR_TIES_AT, ((250, 240, 230), (230, 240, 250), (240, 240, 240))))),
                                   P(radius=0, refine=0)),
        # transmission
        "cap_grey": (picture(45, 47, 12), P(radius=1, refine=2)),
        "cap_bgr": (picture(45, 47, 13, 3), P(radius=3, refine=2)),
        "omega0": (blocks(30, 34, 14, 4), P(omega_q=0, refine=3)),
        "omega256": (blocks(30, 34, 15, 4), P(radius=0, omega_q=256, refine=3)),
        "t0_one": (blocks(30, 34, 16, 4), P(t0_q=4096, refine=3)),
        # the guide
        "noise_eps1_rho32": (_noise(70, 75, 17), P(radius=0, refine=32, eps=1)),
        "noise_eps1_rho1": (_noise(40, 45, 18, 3), P(radius=0, refine=1, eps=1)),
        "step_eps1_rho32": (_step(40, 70), P(radius=0, refine=32, eps=1)),
        "step_eps1_rho2": (_step(40, 70, 3), P(radius=1, refine=2, eps=1)),
        # recovery
        "floor_clips": (_floor_clips(50, 60), P(radius=0, omega_q=256, refine=2, eps=65535)),
    }
    # sides one less than, equal to and one more than each kernel's tile side, in both directions
    for k, (name, (rows, cols)) in enumerate(sorted(TILES.items())):
        for d in (-1, 0, 1):
            out[f"tile_{name}_{rows + d}x{cols + d}"] = (blocks(rows + d, cols + d, 30 + 3 * k + d, 4, channels=3 if d else 0),
                                                         P(radius=2 + k, refine=3 + k))
    return out


def pack(params):
    """The parameters in the C ABI's order."""
    return tuple(params[k] for k in ("radius", "omega_q", "t0_q", "refine", "eps"))
