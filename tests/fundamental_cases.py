"""Inputs of the fundamental-matrix tests (tests/test_fundamental_*.py, tests/test_gpu_fundamental.py): synthetic two-pose
scenes and the named edge cases.  Every case is ``(src, dst)`` float32 (n, 2) plus the call's settings; what each case is
meant to reach is asserted from the specification in tests/test_fundamental_inputs.py."""
from __future__ import annotations

from typing import NamedTuple

import numpy as np

W4K, H4K = 3840, 2160
K4K = np.array([[3000.0, 0.0, W4K / 2], [0.0, 3000.0, H4K / 2], [0.0, 0.0, 1.0]])
WRAP_SEED = (1 << 64) - 5          # seed + 8 h + j passes 2^64 within the first hypothesis


def _rot(rx, ry, rz):
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


class Scene(NamedTuple):
    src: np.ndarray        # (n, 2) float32, centre picture
    dst: np.ndarray        # (n, 2) float32, other picture
    clean: np.ndarray      # (n,) bool: a true correspondence
    Rc: np.ndarray
    Ro: np.ndarray
    tc: np.ndarray
    to: np.ndarray
    K: np.ndarray


def two_pose_scene(n, seed, noise=0.0, contaminated=0.0, planar=False):
    """``n`` matches between two 4K views.  Camera-to-world rotations Rc, Ro and positions tc, to as
    ``spectral_method.fundamental`` takes them; points 40 .. 120 units in front of the cameras (``planar``: on one tilted
    plane), kept when both projections fall inside the pictures.  ``noise``: Gaussian, pixels, on both pictures;
    ``contaminated``: that share of the matches gets a uniformly random ``dst``."""
    rng = np.random.default_rng(seed)
    Rc, tc = np.eye(3), np.zeros(3)
    Ro, to = _rot(0.03, -0.05, 0.02), np.array([6.0, 1.5, 0.5])
    src, dst = np.zeros((0, 2)), np.zeros((0, 2))
    while len(src) < n:
        m = 4 * n + 64
        xy = rng.uniform(-1.0, 1.0, (m, 2)) * np.array([50.0, 30.0])
        z = 80.0 + 0.3 * xy[:, 0] - 0.2 * xy[:, 1] if planar else rng.uniform(40.0, 120.0, m)
        P = np.column_stack([xy, z])
        Xc = (P - tc) @ Rc          # rows of Rc^-1 (P - tc): Rc is orthogonal
        Xo = (P - to) @ Ro
        s = (Xc / Xc[:, 2:3]) @ K4K.T
        d = (Xo / Xo[:, 2:3]) @ K4K.T
        ok = (Xc[:, 2] > 1) & (Xo[:, 2] > 1)
        for q in (s, d):
            ok &= (q[:, 0] >= 0) & (q[:, 0] <= W4K - 1) & (q[:, 1] >= 0) & (q[:, 1] <= H4K - 1)
        src, dst = np.vstack([src, s[ok, :2]]), np.vstack([dst, d[ok, :2]])
    src, dst = src[:n], dst[:n]
    if noise:
        src = src + rng.normal(0.0, noise, src.shape)
        dst = dst + rng.normal(0.0, noise, dst.shape)
    clean = np.ones(n, dtype=bool)
    bad = rng.permutation(n)[:int(round(contaminated * n))]
    clean[bad] = False
    dst[bad] = rng.uniform(0.0, 1.0, (len(bad), 2)) * np.array([W4K - 1, H4K - 1])
    return Scene(src.astype(np.float32), dst.astype(np.float32), clean, Rc, Ro, tc, to, K4K)


def unit(F):
    """F at unit Frobenius norm with its first entry of largest magnitude positive."""
    F = np.asarray(F, dtype=np.float64) / np.linalg.norm(F)
    return -F if F.ravel()[np.argmax(np.abs(F))] < 0 else F


def point_line_distance(F, src, dst):
    """Distance in pixels of every ``dst`` from the epipolar line ``F src`` (plain numpy, for the property tests)."""
    s = np.column_stack([src.astype(np.float64), np.ones(len(src))])
    d = np.column_stack([dst.astype(np.float64), np.ones(len(dst))])
    line = s @ F.T
    return np.abs(np.sum(line * d, axis=1)) / np.sqrt(line[:, 0] ** 2 + line[:, 1] ** 2)


class Case(NamedTuple):
    name: str
    src: np.ndarray
    dst: np.ndarray
    thresh: float = 3.0
    iterations: int = 64
    seed: int = 0x5EEDC0DE5EEDC0DE


def _scene_case(name, n, seed, **kw):
    settings = {k: kw.pop(k) for k in ("thresh", "iterations", "call_seed") if k in kw}
    if "call_seed" in settings:
        settings["seed"] = settings.pop("call_seed")
    s = two_pose_scene(n, seed, **kw)
    return Case(name, s.src, s.dst, **settings)


def integer_grid_case():
    """Points of a 5 x 5 integer grid (bounding box 0 .. 4: the normalised coordinates are multiples of 1/2, every operation of
    the elimination is exact for a while), many of them repeated: hypotheses that draw a repeated match meet an exactly zero
    pivot, the others do not."""
    rng = np.random.default_rng(11)
    g = np.array([(i, j) for i in range(5) for j in range(5)], dtype=np.float32)
    src = g[rng.integers(0, 25, 40)]
    dst = g[rng.integers(0, 25, 40)]
    src[:4], dst[:4] = g[[0, 4, 20, 24]], g[[0, 4, 20, 24]]      # the corners: the boxes are the whole grid
    src[20:], dst[20:] = src[:20], dst[:20]                      # every match twice
    return Case("integer_grid", src, dst, 3.0, 256)


def edge_cases():
    rng = np.random.default_rng(5)
    one = np.tile(np.float32([[123.5, 77.25]]), (8, 1))
    unrelated = (rng.uniform(0, 1, (64, 2)) * [W4K, H4K]).astype(np.float32), (rng.uniform(0, 1, (64, 2)) * [W4K, H4K]).astype(np.float32)
    tline = np.sort(rng.uniform(0.0, 1.0, 40))
    line_s = np.column_stack([100 + 3000 * tline, 200 + 1500 * tline]).astype(np.float32)
    line_d = np.column_stack([300 + 2800 * tline, 1900 - 1200 * tline]).astype(np.float32)
    same = two_pose_scene(100, 3).src
    return [
        _scene_case("n8_permutations", 8, 21, iterations=64),
        integer_grid_case(),
        Case("one_match_eight_times", one, one + np.float32(5.0), 3.0, 64),
        Case("thresh0_unrelated", unrelated[0], unrelated[1], 0.0, 64),
        Case("collinear", line_s, line_d, 3.0, 64),
        Case("src_equals_dst", same, same.copy(), 3.0, 64),
        _scene_case("planar", 300, 9, planar=True, noise=0.3, iterations=128),
        _scene_case("wrapping_seed", 9, 22, iterations=64, call_seed=WRAP_SEED),
    ]


N_VALUES = (8, 9, 63, 64, 65, 255, 256, 257, 1000)      # wave and block strides of the score and re-fit loops
ITERATION_VALUES = (1, 63, 64, 65, 2048)
THRESH_VALUES = (0.0, 3.0, float("inf"))


def shape_cases():
    """One contaminated scene per n (64 iterations, 3 px), then the iteration counts and the thresholds at n = 257."""
    out = [_scene_case(f"n{n}", n, 100 + n, noise=0.5, contaminated=0.0 if n < 16 else 0.3, iterations=64) for n in N_VALUES]
    out += [_scene_case(f"it{k}", 257, 357, noise=0.5, contaminated=0.3, iterations=k) for k in ITERATION_VALUES if k != 64]
    out += [_scene_case(f"thresh{t}", 257, 357, noise=0.5, contaminated=0.3, iterations=64, thresh=t) for t in THRESH_VALUES if t != 3.0]
    return out


_EXPECTED = {}


def expected(case):
    """The specification's ``core`` of a case, computed once per process and shared (callers do not change it)."""
    if case.name not in _EXPECTED:
        import fundamental_spec as S
        _EXPECTED[case.name] = S.core(case.src, case.dst, case.thresh, case.iterations, case.seed)
    return _EXPECTED[case.name]


def batch_case():
    """Pairs of 8, 257, 64 and 1000 matches behind 13 unused rows (a first offset above 0)."""
    scenes = [two_pose_scene(n, 200 + n, noise=0.5, contaminated=0.0 if n < 16 else 0.3) for n in (8, 257, 64, 1000)]
    pad = np.full((13, 2), 7.0, dtype=np.float32)
    src = np.concatenate([pad] + [s.src for s in scenes])
    dst = np.concatenate([pad] + [s.dst for s in scenes])
    offsets = np.cumsum([13] + [len(s.src) for s in scenes]).astype(np.int32)
    return src, dst, offsets
