"""TEST INFRASTRUCTURE - never imported by the product.

Specification, in numpy, of the squared weights K1 sums and of the test K2 routes a cell to the careful path with
(``cvx_proj_amd/csrc/apap_kernels.hip``).  The reference forms ``w = max(exp(-d / sigma^2), gamma)`` in float64 and takes the
SVD of ``w * aa`` (apap.py:150-159); K1 forms ``w^2 = max(exp(-2 d / sigma^2), gamma^2)`` directly, which halves the usable
exponent range.  Restated here:

* ``cell_weight_sq_tab`` (float64, the default): the 512-entry table of 2^(j/512), the degree-4 polynomial and the
  ``ldexp``, operation by operation.  Its rsq-seeded square root (< 1 ulp) is modelled as correctly rounded, and its FMAs
  as exact products rounded once (evaluated in extended precision).
* ``cell_weight_sq_f32`` (float32, APAP_OPT_WEIGHTS_F32): float32 arithmetic throughout.  ``v_sqrt_f32`` and ``v_exp_f32``
  are accurate to 1 ulp on the hardware; they are modelled as correctly rounded, and the bound below allows the ulp.
  ``v_exp_f32`` on gfx950 flushes subnormal results to 0 (observed for every x in [-155.5, -126.5]), and so does the
  model; the bound (2^-126 absolute below x = -126) would hold without the flush too.
* ``k1_gamma2``: the gamma^2 each chain clamps at.
* K2's routing: trace, ``underflowed`` (the trace floor of the chain), the eigen-gap test, n < 5.

``cell()`` returns, for one (vertex, keypoints, gamma, sigma, chain), the w^2 vector, the region of each weight and of the
cell, and ``eps_cell``: a bound on the relative perturbation of the cell's normal matrix M = sum_k w_k^2 (r1 r1^T + r2 r2^T)
that the chain's weights cause, ||M_chain - M|| <= eps_cell * trace(M) (M from the exact weights).  Singular-vector
perturbation theory turns that into ``bar()`` = BAR_C (eps_cell + EPS64) cond scale + FLOOR_ULPS EPS32 scale px of
reprojection error, with ``cond = trace(M) / (lambda_8 - lambda_9)`` (``normal_cond``), ``scale`` the size of the projected
coordinates and the last term the float32 rounding of both grids.  BAR_C and FLOOR_ULPS are calibrated on the CPU by
tests/test_weight_spec.py from this emulation, not from GPU runs.
"""
import numpy as np

EPS64 = 2.0 ** -53
EPS32 = 2.0 ** -24
LOG2E = float.fromhex("0x1.71547652b82fep+0")
EXP_BITS = 9
EXP_N = 1 << EXP_BITS
EXP_SCALE = EXP_N * LOG2E                  # kExpScale
TRACE_FLOOR_F64 = 1e-280                   # kTraceFloorF64
TRACE_FLOOR_W32 = 2.0 ** -40               # kTraceFloorW32
GAMMA_CUT_F64 = 2.0 ** 128                 # kGammaCutF64
GAP_TOL = 1e-3                             # kGapTol
F32_NORMAL_MIN = 2.0 ** -126
F64_NORMAL_MIN = 2.0 ** -1022
BAR_C = 16.0                               # reprojection bar constants (calibrated in tests/test_weight_spec.py)
FLOOR_ULPS = 4.0


def _exp2_table():
    """The 512 correctly rounded values of 2^(j / 512) (kExp2Tab)."""
    import mpmath as mp
    with mp.workprec(200):
        return np.array([float(mp.power(2, mp.mpf(j) / EXP_N)) for j in range(EXP_N)])


EXP2_TAB = _exp2_table()


def _fma(a, b, c):
    """a * b + c rounded once (float64 operands; the exact product fits the 64-bit extended mantissa only approximately,
    which is the model's one liberty)."""
    return (np.longdouble(a) * np.longdouble(b) + np.longdouble(c)).astype(np.float64)


def k1_gamma2(gamma, chain):
    """What the host (and k_solve_small) passes K1 as gamma^2 (k1_gamma2 in the kernels): from gamma = 1 (float32 chain) or
    2^128 (float64) on every weight is gamma, and the chain clamps at 1 instead of an overflowing gamma^2."""
    if gamma >= (1.0 if chain == "f32" else GAMMA_CUT_F64):
        return 1.0
    return gamma * gamma if gamma > 0.0 else 0.0


def w2_f64(vertex, src, gamma, sigma):
    """cell_weight_sq_tab for every keypoint of ``src`` (n x 2, widened to float64) at ``vertex``."""
    vx, vy = (float(v) for v in vertex)
    s = np.asarray(src, np.float64)
    inv_sigma = 1.0 / (sigma * sigma)
    scaled = (2.0 * inv_sigma) * EXP_SCALE
    dx, dy = vx - s[:, 0], vy - s[:, 1]
    x = _fma(dx, dx, _fma(dy, dy, 1e-300))
    g = np.sqrt(x)                                          # rsq + cubic correction: modelled as correctly rounded
    with np.errstate(all="ignore"):
        yu = g * scaled
        nk = np.where(-yu <= -2.0 ** 31, -2 ** 31, np.trunc(-np.nan_to_num(yu, nan=0.0, posinf=2.0 ** 31))).astype(np.int64)
        f = yu - np.floor(yu)                               # v_fract_f64 (inf -> NaN)
        t = EXP2_TAB[nk & (EXP_N - 1)]
        L = float.fromhex("0x1.62e42fefa39efp-1") / EXP_N
        p = _fma(f, L * L * L * L / 24, -(L * L * L / 6))
        p = _fma(f, p, L * L / 2)
        p = _fma(f, p, -L)
        p = _fma(f, p, 1.0)
        r = np.ldexp(t * p, (nk >> EXP_BITS).astype(np.int32))
    return np.fmax(r, k1_gamma2(gamma, "f64"))              # fmax drops a NaN


def w2_f32(vertex, src, gamma, sigma):
    """cell_weight_sq_f32 for every keypoint: float32 vertex and keypoint (the 24-sum table's column 29), float32
    arithmetic, ``v_sqrt_f32`` / ``v_exp_f32`` modelled as correctly rounded."""
    f = np.float32
    vxf, vyf = f(vertex[0]), f(vertex[1])
    s = np.asarray(src, np.float64).astype(f)
    inv_sigma2 = 2.0 * (1.0 / (sigma * sigma))
    neg_scale = f(inv_sigma2 * -LOG2E)
    g2 = f(k1_gamma2(gamma, "f32"))
    with np.errstate(all="ignore"):
        dx = vxf - s[:, 0]
        dy = vyf - s[:, 1]
        q = (dx.astype(np.float64) * dx + (dy * dy).astype(np.float64)).astype(f)    # v_fma_f32(dx, dx, dy * dy)
        d = np.sqrt(q)
        x = d * neg_scale
        w = np.exp2(x.astype(np.float64)).astype(f)        # rounded once
    w = np.where(w < F32_NORMAL_MIN, f(0.0), w)             # v_exp_f32 flushes subnormal results (observed on gfx950)
    return np.fmax(w, g2).astype(np.float64), x.astype(np.float64)


def w2_exact(vertex, src, gamma, sigma):
    """max(exp(-2 d / sigma^2), gamma^2) in extended precision (no underflow down to 1e-4900): the weights the reference
    squares, the yardstick of both chains."""
    s = np.asarray(src, np.float64).astype(np.longdouble)
    v = np.asarray(vertex, np.float64).astype(np.longdouble)
    d = np.sqrt((v[0] - s[:, 0]) ** 2 + (v[1] - s[:, 1]) ** 2)
    sig = np.longdouble(sigma)
    return np.maximum(np.exp(-2 * d / (sig * sig)), np.longdouble(gamma) ** 2)


def rel_bound_f32(vertex, src, sigma, x):
    """Per keypoint, the relative error bound of a NORMAL float32 w^2 that include/apap_hip.h states:
    (6 |x| + 4) 2^-24 + 2 c / sigma^2.  6 |x| 2^-24 covers the roundings of x = d * neg_scale (neg_scale, the product, and
    d's own: dx, dy, dy * dy, the FMA, the square root's ulp), times ln 2 < 1; 4 2^-24 the exp2's ulp and the clamp's
    rounding; c = |float32(v) - v|_1 + |float32(s) - s|_1 is what the coordinates' rounding moves d by, and
    2 log2(e) ln(2) = 2 turns it into relative error of w^2."""
    s = np.asarray(src, np.float64)
    v = np.asarray(vertex, np.float64)
    c = (abs(float(np.float32(v[0])) - v[0]) + abs(float(np.float32(v[1])) - v[1])
         + np.abs(s.astype(np.float32).astype(np.float64) - s).sum(axis=1))
    return (6.0 * np.abs(x) + 4.0) * EPS32 + 2.0 * c / (sigma * sigma)


def rel_bound_f64(u):
    """Per keypoint, the relative error bound of a normal float64 w^2 = e^-u, u = 2 d / sigma^2: the table exp's 1.5 ulp (1 + u)
    (the kernel's comment) plus the square root's ulp, rounded up: (4 + 4 u) 2^-53."""
    return (4.0 + 4.0 * np.abs(u)) * EPS64


def regions(w2, chain):
    """Per keypoint: 'normal', 'subnormal' or 'zero' (of the chain's format)."""
    lo = F32_NORMAL_MIN if chain == "f32" else F64_NORMAL_MIN
    return np.where(w2 == 0, "zero", np.where(w2 < lo, "subnormal", "normal"))


def row_norms2(aa):
    """t_k = |r1|^2 + |r2|^2 of each keypoint's two DLT rows (``aa``: 2n x 9 float32)."""
    a = np.asarray(aa, np.float64)
    return (a[0::2] ** 2).sum(axis=1) + (a[1::2] ** 2).sum(axis=1)


def normal_matrix(w2, aa):
    """M = sum_k w_k^2 (r1 r1^T + r2 r2^T), float64."""
    a = np.asarray(aa, np.float64)
    return (a * np.repeat(np.asarray(w2, np.float64), 2)[:, None]).T @ a


def route(M, n, chain, careful=True):
    """K2's test (eigen_denorm_cell): the careful path when n < 5, when the trace is below the chain's floor or not finite
    (``underflowed``), or when a second eigenvalue lies within 1e-3 of the trace of the smallest (``gap``; the kernel counts
    eigenvalues below rho + gap_tol, modelled here on the exact spectrum)."""
    trace = float(np.trace(M))
    floor = TRACE_FLOOR_W32 if chain == "f32" else TRACE_FLOOR_F64
    underflowed = not (trace >= floor) or not (trace < 1.797e308)
    gap_small = False
    if not underflowed:
        lam = np.linalg.eigvalsh(M)
        gap_small = not (lam[1] - lam[0] >= GAP_TOL * trace)
    return dict(trace=trace, underflowed=underflowed, gap_small=gap_small,
                careful=bool(careful and (n < 5 or underflowed or gap_small)))


def normal_cond(M):
    """trace(M) / (lambda_8 - lambda_9) of a normal matrix: what a relative perturbation of M is amplified by in the
    singular vector taken (inf for a double smallest eigenvalue)."""
    lam = np.linalg.eigvalsh(np.asarray(M, np.float64))
    gap = lam[1] - lam[0]
    return float(np.trace(M) / gap) if gap > 0 else np.inf


def cell(vertex, src, gamma, sigma, chain, aa=None, careful=True):
    """One cell on chain "f64" or "f32".  ``aa`` (the reference's 2n x 9 float32 rows) weighs each keypoint's error by its
    rows' size t_k = |r1|^2 + |r2|^2 and gives K2's full routing; without it t_k = 1 and only the trace test is modelled.
    Returns a dict:
      w2          the chain's w^2 (float64 array)
      exact       the yardstick: max(exp(-2 d / sigma^2), gamma^2) in extended precision, times the constant the chain
                  rescales by where gamma^2 would overflow it (every weight is gamma there)
      x           the exponent argument in powers of two (float32 chain: that of the exp2; float64: -u / ln 2)
      region      per keypoint 'normal' / 'subnormal' / 'zero' (of the chain's format)
      route       K2's routing on the chain's normal matrix (``route``)
      cell_region 'careful' when routed, else the region of the largest w^2
      eps_chain   bound on ||M_chain - M|| / trace(M): sum_k A_k t_k / sum_k exact_k t_k with A_k = rel_k exact_k for a
                  normal weight (rel_bound_*; 4 ulp for a clamped one) and the format's smallest normal number for a
                  subnormal or zero one, flushed or not
      eps_cell    what the ENGINE solves with: 0 on the careful path (float64 weights, QR of the rows), else eps_chain
      eps_actual  sum_k |w2_k - exact_k| t_k / sum_k exact_k t_k, measured"""
    if chain not in ("f32", "f64"):
        raise ValueError(chain)
    exact = w2_exact(vertex, src, gamma, sigma)
    if gamma >= (1.0 if chain == "f32" else GAMMA_CUT_F64):
        exact = exact * (np.longdouble(k1_gamma2(gamma, chain)) / (np.longdouble(gamma) ** 2))
    n = exact.shape[0]
    t = row_norms2(aa) if aa is not None else np.ones(n)
    s = np.asarray(src, np.float64)
    d = np.hypot(float(vertex[0]) - s[:, 0], float(vertex[1]) - s[:, 1])
    u = 2.0 * d / (sigma * sigma)
    with np.errstate(over="ignore"):
        clamped = np.exp(-np.longdouble(u)) <= np.longdouble(gamma) ** 2
    if chain == "f32":
        w2, x = w2_f32(vertex, src, gamma, sigma)
        rel = np.where(clamped, 4.0 * EPS32, rel_bound_f32(vertex, src, sigma, x))
        lo = F32_NORMAL_MIN
    else:
        w2 = w2_f64(vertex, src, gamma, sigma)
        x = -u / np.log(2.0)
        rel = np.where(clamped, 4.0 * EPS64, rel_bound_f64(u))
        lo = F64_NORMAL_MIN
    ex = exact.astype(np.float64)                          # 0 below the float64 range: only used for "is it tiny"
    tiny = (w2 < lo) | (ex < lo * (1 + 1e-6))
    A = np.where(tiny, lo, rel * ex)
    reg = regions(w2, chain)
    r = dict(w2=w2, exact=exact, x=x, region=reg)
    den = (exact * t).sum()
    with np.errstate(all="ignore"):
        r["eps_actual"] = float((np.abs(w2.astype(np.longdouble) - exact) * t).sum() / den) if den > 0 else np.inf
        r["eps_chain"] = float((np.longdouble(1) * A * t).sum() / den) if den > 0 else np.inf
    if aa is not None:
        rt = route(normal_matrix(w2, aa), n, chain, careful)
    else:
        trace = float((w2 * t).sum())
        floor = TRACE_FLOOR_W32 if chain == "f32" else TRACE_FLOOR_F64
        rt = dict(trace=trace, underflowed=not (trace >= floor) or not (trace < 1.797e308), gap_small=False)
        rt["careful"] = bool(careful and (n < 5 or rt["underflowed"]))
    r["route"] = rt
    r["eps_cell"] = 0.0 if rt["careful"] else r["eps_chain"]
    r["cell_region"] = "careful" if rt["careful"] else str(reg[int(np.argmax(w2))])
    return r


def bar(eps_cell, cond, scale):
    """The reprojection bar (px) of a cell solved from the normal matrix of weights within eps_cell (see the module text)."""
    return BAR_C * (eps_cell + EPS64) * cond * scale + FLOOR_ULPS * EPS32 * scale


def solve_normal(M, p):
    """The eigenvector of M's smallest eigenvalue, de-normalised as apap.py:163-167 does (``p``: oracle.prepare) -
    what K2 computes from the sums, in float64 LAPACK (test emulation only)."""
    from oracle.apap_oracle import _denormalise
    _, V = np.linalg.eigh(M)
    return _denormalise(V[:, 0], p).astype(np.float32)


def solve_rows(w2, p):
    """The careful path's answer: the last right singular vector of sqrt(w2) * aa in float64 (test emulation only)."""
    from oracle.apap_oracle import _denormalise
    A = np.repeat(np.sqrt(np.asarray(w2, np.float64)), 2)[:, None] * p["aa"]
    _, _, vt = np.linalg.svd(A, full_matrices=False)
    return _denormalise(vt[-1], p).astype(np.float32)
