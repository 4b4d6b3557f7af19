"""Inputs of the Huber M-step's tests: seeded by integer hashing and built with + - * / only, so they are the same on every
numpy.  Synthetic 4K pairs that share one true homography; every case names the edge it reaches."""
import numpy as np

from sfm_cases import integers, uniform

F32 = np.float32
T = 256                      # APAP_MODEL_HUBER_THREADS: the workgroup's width
H_TRUE = np.array([[0.97, 0.04, 35.0], [-0.03, 1.01, -12.0], [2e-6, -1e-6, 1.0]])
SIZE = np.array([3840.0, 2160.0])


def pair(n, seed, kind="clean", noise=1.0):
    """(pts_c, pts_o, weights, inlier mask): ``n`` matches of the 4K pair, weights 0.3 .. 1, ``noise`` px of noise (a sum of
    four uniforms, variance one).  kind: 'clean'; 'moderate' (5 % displaced by 5 .. 30 px); 'gross' (20 % anywhere)."""
    pc = (uniform(2 * n, seed, 0).reshape(n, 2) * SIZE).astype(F32)
    x, y = pc[:, 0].astype(np.float64), pc[:, 1].astype(np.float64)
    q = [x * H_TRUE[k, 0] + y * H_TRUE[k, 1] + H_TRUE[k, 2] for k in range(3)]      # no matrix product: no fused multiply-add
    po = np.stack([q[0] / q[2], q[1] / q[2]], axis=1)
    u = uniform(8 * n, seed, 1).reshape(n, 2, 4)
    g = (u[:, :, 0] + u[:, :, 1] + u[:, :, 2] + u[:, :, 3] - 2.0) * 1.7320508075688772
    po = po + noise * g
    inlier = np.ones(n, bool)
    if kind == "moderate":
        bad = integers(n, seed, 2, 100) < 5
        mag = 5.0 + 25.0 * uniform(n, seed, 3)
        t = uniform(n, seed, 4)
        sx = 2.0 * integers(n, seed, 5, 2) - 1.0
        sy = 2.0 * integers(n, seed, 6, 2) - 1.0
        po[bad] += np.stack([sx * mag * t, sy * mag * (1.0 - t)], axis=1)[bad]
        inlier = ~bad
    elif kind == "gross":
        bad = integers(n, seed, 2, 100) < 20
        po[bad] = (uniform(2 * n, seed, 3).reshape(n, 2) * SIZE)[bad]
        inlier = ~bad
    elif kind != "clean":
        raise ValueError(kind)
    w = (0.3 + 0.7 * uniform(n, seed, 7)).astype(F32)
    return pc, po.astype(F32), w, inlier


def _case(n, seed, kind="clean", M=0.5, floor=None, cap=0, expect="converge", edit=None):
    pc, po, w, inl = pair(n, seed, kind)
    c = dict(pc=pc, po=po, w=w, inlier=inl, M=M, floor=floor, cap=cap, expect=expect)
    if edit:
        edit(c)
    return c


def _empty_fold(c):
    c["w"][24:48] = F32(5e-4)            # the second fold of 24 matches lies wholly below the floor


def _subnormal(c):
    c["w"][::5] = F32(1e-40)             # subnormal float32 weights: kept (no floor), rows of subnormal products


def _collinear(c):
    x = np.arange(len(c["pc"]), dtype=F32) * 16
    c["pc"] = np.stack([x, 2 * x + 8], axis=1).astype(F32)
    c["po"] = c["pc"] + F32([5, 3])
    c["w"][:] = 1


def cases():
    """name -> case.  expect: 'converge' (the gap must close), 'unclipped' (M so large that the least-squares solution is
    returned), 'hard' (only the status rules hold), 'exact' (four matches: the fit is exact, f(h) is rounding noise and so is
    its relative gap), 'degenerate'."""
    out = {
        "clean_500": _case(500, 1),
        "clean_2000": _case(2000, 2),
        "moderate_2000": _case(2000, 3, "moderate"),
        "moderate_500_M2": _case(500, 4, "moderate", M=2.0),
        "gross_2000": _case(2000, 5, "gross"),
        "gross_500_M5": _case(500, 6, "gross", M=5.0),
        "n4": _case(4, 7, expect="exact"),
        "n5": _case(5, 8),
        "n24": _case(24, 9),
        "n25": _case(25, 10),
        "n240": _case(240, 11),
        "n241": _case(241, 12),
        "rows_T_minus_2": _case(T // 2 - 1, 13),
        "rows_T": _case(T // 2, 14),
        "rows_T_plus_2": _case(T // 2 + 1, 15),
        "matches_T_minus_1": _case(T - 1, 16),
        "matches_T": _case(T, 17),
        "matches_T_plus_1": _case(T + 1, 18),
        "empty_fold": _case(300, 19, floor=1e-3, edit=_empty_fold),
        "subnormal_weights": _case(300, 20, edit=_subnormal),
        "M_1e6": _case(500, 1, M=1e6, expect="unclipped"),
        "M_0p011_clean": _case(500, 1, M=0.011),
        "M_0p011_gross": _case(500, 6, "gross", M=0.011, expect="hard"),
        "cap_1": _case(500, 3, "moderate", cap=1, expect="hard"),
        "collinear": _case(12, 21, expect="degenerate", edit=_collinear),
        "n3": _case(3, 22, expect="degenerate"),
    }
    out["M_at_a_residual"] = m_at_a_residual()
    return out


def m_at_a_residual():
    """M set to the magnitude of one residual of the specification's least-squares solution, exactly: that row is not clipped
    (|r| <= M).  The engine's least-squares solution differs from numpy's in the last bits, so there the row sits within
    rounding of M on either side at the start."""
    import model_spec as S
    c = _case(300, 23)
    A, rhs, _, _ = S.rows(c["pc"], c["po"], c["w"])
    h0 = S.solve(c["pc"], c["po"], c["w"], "lms")[0]
    r = np.abs(A.astype(np.float64) @ h0 - rhs.astype(np.float64).ravel())
    c["M"] = float(np.sort(r)[int(0.8 * len(r))])
    c["expect"] = "converge"
    return c


CLEAN_500_SHA256 = "cf46890089dcb00db3a8a9a5f980985f802891cd11076bb80be02c670d787d6d"     # of clean_500's pc, po, w: the generator is the same everywhere
CONVERGING = [k for k, c in cases().items() if c["expect"] == "converge"]
HARD = [k for k, c in cases().items() if c["expect"] == "hard"]
DEGENERATE = [k for k, c in cases().items() if c["expect"] == "degenerate"]
