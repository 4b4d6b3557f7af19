"""Inputs of the bilinear warp's tests (tests/warp_bilinear_spec.py is the definition).  Built once per session and shared:
read-only.  tests/test_warp_bilinear_host.py asserts on the CPU, from the spec alone, that every built input reaches its edge;
tests/test_gpu_warp_bilinear.py holds the kernels to the spec on them, byte for byte.

Built cases.  Every cell is an exact translation: its float32 forward matrix is ``[[1, 0, -A], [0, 1, -B], [0, 0, 1]]``, its
inverse ``[[1, 0, A], [0, 1, B], [0, 0, 1]]`` with no rounding (asserted), and a canvas pixel's coordinate ``(x + A, y + B)``
is exact in float64 - the division is by 1.  |A|, |B| < 16 so that ``m + (2 k + 1) / 64 +- 2^-20`` is a float32.  Canvas 70 x
40 with the offsets (3, 2) over a 60 x 34 source; mesh columns [0, 16, 33, 35, 52, 70] - the 2 px column puts canvas pixels
32 .. 35, one lane's group of four, in three cells - and rows [0, 13, 27, 40]: the edges at 13 and 27 fall inside a strip
of two rows (12, 13 and 26, 27) and of four (12 .. 15, 24 .. 27).

  ties        A = m + (2 k + 1) / 64: 32 tx is an integer and a half, an exact tie of rint; k of both parities, so the even
              neighbour lies below (k even) and above (k odd).  B alike per cell row.
  ties_plus   the same moved by + 2^-20, ties_minus by - 2^-20: no tie, and the nearer neighbour on either side
  rim_a       the last column's A = -7 + 63/64: tx = w - 1/64 at the canvas' last column, a tie that goes to the even X = 32 w,
              which must land on column w - 1; the last row's B = -4 + 1/2: ty in (h - 1, h) with Y < 32 h
  rim_b       A = -7 + 63/64 + 2^-10: tx inside (w - 1/64, w), X = 32 w without a tie; B = -4 + 63/64: Y = 32 h by the tie
  rim_c       A = -7 + 1/2: tx in (w - 1, w) with X < 32 w; B = -4 + 63/64 + 2^-10
              In all three column 0 has A = -1 + 2^-8 and row 0 B = -2 + 2^-9: tx in (0, 1/64) at x = 1, ty at y = 2.

Seeded cases: a source, a grid around a mild perspective, a mesh (regular or irregular) - ``seeded``.
"""
import numpy as np

from oracle import apap_oracle as O
import warp_bilinear_spec as S
from warp_integer_cases import picture

SRC_HW = (34, 60)
FINAL = (70, 40, 3, 2)
MESH_W = [0.0, 16, 33, 35, 52, 70]
MESH_H = [0.0, 13, 27, 40]
STRIP_ROWS, WAVES_PER_BLOCK = 2, 4      # k_warp_bilinear's tiling (csrc/apap_warp_bilinear.hip)

_cases = {}


def tie(m, k):
    return m + (2 * k + 1) / 64.0


def _translations(name, A, B, shift=0.0):
    """One case from per-column A and per-row B (+ shift)."""
    rows, cols = len(B), len(A)
    H = np.zeros((rows, cols, 3, 3), np.float32)
    hinv = np.zeros_like(H)
    for r in range(rows):
        for c in range(cols):
            a, b = A[c] + shift, B[r] + shift
            assert np.float32(a) == a and np.float32(b) == b and abs(a) < 16 and abs(b) < 16
            H[r, c] = [[1, 0, -a], [0, 1, -b], [0, 0, 1]]
            hinv[r, c] = [[1, 0, a], [0, 1, b], [0, 0, 1]]
    assert np.array_equal(O.invert_cells_f32(H), hinv), "numpy's float32 inverse is not the designed translation"
    mesh = (np.asarray(MESH_W, np.float64), np.asarray(MESH_H, np.float64))
    tx, ty = O.warp_coords_fast(hinv, mesh, FINAL[:2], FINAL[2:])
    img = picture(*SRC_HW)
    center = np.random.default_rng(len(name)).integers(0, 256, (FINAL[1] - FINAL[3], FINAL[0] - FINAL[2], 3), dtype=np.uint8)
    for a in (H, hinv, tx, ty, img, center) + mesh:
        a.setflags(write=False)
    return dict(name=name, img=img, H=H, hinv=hinv, mesh=mesh, final=FINAL, coords=(tx, ty), center=center)


TIE_A = [tie(-2, 0), tie(1, 1), tie(0, 30), tie(-1, 15), tie(2, 2)]
TIE_B = [tie(1, 3), tie(-1, 0), tie(0, 16)]
RIM_A = [-1 + 2.0 ** -8, tie(0, 5), 0.25, -0.75]         # + the last column's
RIM_B = [-2 + 2.0 ** -9, 0.5]                            # + the last row's
RIM_LAST = dict(rim_a=(-7 + 63 / 64, -4 + 0.5), rim_b=(-7 + 63 / 64 + 2.0 ** -10, -4 + 63 / 64),
                rim_c=(-7 + 0.5, -4 + 63 / 64 + 2.0 ** -10))

_BUILDERS = dict(ties=lambda: _translations("ties", TIE_A, TIE_B),
                 ties_plus=lambda: _translations("ties_plus", TIE_A, TIE_B, 2.0 ** -20),
                 ties_minus=lambda: _translations("ties_minus", TIE_A, TIE_B, -2.0 ** -20),
                 **{n: (lambda n=n, a=a, b=b: _translations(n, RIM_A + [a], RIM_B + [b])) for n, (a, b) in RIM_LAST.items()})
BUILT = tuple(_BUILDERS)


def get(name):
    if name not in _cases:
        _cases[name] = _BUILDERS[name]()
    return _cases[name]


def seeded(seed, final_w, final_h, rows, cols, src_wh=(37, 53), irregular=False, dtype=np.float32, offset=(0, 0)):
    """A source picture (random bytes 1 .. 255), a (rows, cols) grid of forward matrices around a mild perspective that maps
    the source onto most of the canvas, and mesh edges that cover the canvas - interior edges moved by up to a third of a cell
    when ``irregular``."""
    rng = np.random.default_rng(seed)
    w, h = src_wh
    img = rng.integers(1, 256, (h, w, 3), dtype=np.uint8)
    Hg = np.array([[0.93 * final_w / w, 0.03, 0.6 - offset[0]], [-0.02, 0.9 * final_h / h, 0.4 - offset[1]], [2e-4 / w, -3e-4 / h, 1.0]])
    r, c = np.meshgrid(np.arange(rows) / rows, np.arange(cols) / cols, indexing="ij")
    P = np.zeros((rows, cols, 3, 3))
    P[..., 0, 0], P[..., 0, 1], P[..., 0, 2] = np.sin(2.0 * r + c), np.cos(r - 3.0 * c), 3.0 * np.sin(3.0 * r) * np.cos(2.0 * c)
    P[..., 1, 0], P[..., 1, 1], P[..., 1, 2] = np.cos(r + 2.0 * c), np.sin(3.0 * r - c), 3.0 * np.cos(2.0 * r + c)
    P[..., 2, 0], P[..., 2, 1] = 1e-3 * np.sin(r + c), 1e-3 * np.cos(r - c)
    H = np.ascontiguousarray(Hg @ (np.eye(3) + 1e-2 * P)).astype(dtype)
    mesh = [np.linspace(0.0, final_w, cols + 1), np.linspace(0.0, final_h, rows + 1)]
    if irregular:
        for e in mesh:
            if e.size > 2:
                e[1:-1] += (rng.random(e.size - 2) - 0.5) * (e[1] - e[0]) * 0.66
    return dict(img=img, H=H, mesh=tuple(mesh), final=(final_w, final_h, offset[0], offset[1]))


def reaches(case):
    """What a built case's coordinates reach, from the spec: a dict of pixel counts."""
    h, w = case["img"].shape[:2]
    tx, ty = case["coords"]
    ok = S.present(tx, ty, w, h)
    X, Y = S.fixed(tx, ok), S.fixed(ty, ok)
    fx, fy = 32.0 * tx, 32.0 * ty
    tie_x = ok & (fx - np.floor(fx) == 0.5)
    tie_y = ok & (fy - np.floor(fy) == 0.5)
    return dict(present=int(ok.sum()), absent=int((~ok).sum()),
                tie_x_down=int((tie_x & (X < fx)).sum()), tie_x_up=int((tie_x & (X > fx)).sum()),
                tie_y_down=int((tie_y & (Y < fy)).sum()), tie_y_up=int((tie_y & (Y > fy)).sum()),
                x_is_32w=int((ok & (X == 32 * w)).sum()), y_is_32h=int((ok & (Y == 32 * h)).sum()),
                x_last=int((ok & (tx > w - 1) & (X < 32 * w)).sum()), y_last=int((ok & (ty > h - 1) & (Y < 32 * h)).sum()),
                x_first=int((ok & (tx < 1 / 64)).sum()), y_first=int((ok & (ty < 1 / 64)).sum()),
                clamped=int((ok & ((X >> 5) + 1 > w - 1) & ((X & 31) != 0)).sum()))
