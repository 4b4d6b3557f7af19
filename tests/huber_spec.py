"""numpy specification of the Huber M-step (model.py's LMSSolver with huber_param > 1e-2) as the engine computes it
(cvx_proj_amd/csrc/apap_model_dev.h: model_huber_body, DESIGN.md "Huber M-step").  Test infrastructure only: the product
never imports it.

    minimise over h in R^8   f(h) = sum_j phi_M(r_j),   r = A h - rhs
    phi_M(r) = r^2 if |r| <= M, 2 M |r| - M^2 otherwise            (cvxpy's huber(x, M))

* ``problem``: A (2c x 8) and rhs (2c) of the selected matches through ``model_spec.rows``, as float64.
* ``objective`` / ``gap``: f(h) and the relative duality gap of h in ``np.longdouble``, from the rows alone.
* ``solve``: the kernel's method with the kernel's guards (Newton steps on the active quadratic piece with a halving line
  search, a majorise-minimise step as the fallback), in float64.
"""
from __future__ import annotations

from typing import NamedTuple

import numpy as np

import model_spec as S

GAP_TOL = 1e-10
DEFAULT_CAP = 100     # APAP_MODEL_MAX_ITER = 0 (DESIGN.md "Huber M-step": twice the largest count of a converging case, rounded up)
HALVINGS = 11         # alpha = 1, 1/2, .., 2^-10
LD = np.longdouble


def problem(pts_c, pts_o, weights):
    """(A float64 (2c, 8), rhs float64 (2c,)) of the matches GIVEN (select them first with model_spec.select)."""
    A, rhs, _, _ = S.rows(pts_c, pts_o, weights)
    return A.astype(np.float64), rhs.astype(np.float64).ravel()


def phi(r, M):
    a = np.abs(r)
    return np.where(a <= M, r * r, 2 * M * a - M * M)


def objective(A, rhs, h, M):
    """f(h) in extended precision."""
    r = A.astype(LD) @ np.asarray(h, LD) - rhs.astype(LD)
    return LD(phi(r, LD(M)).sum())


def _chol_solve_ld(G, b):
    """Solve G x = b (G symmetric positive definite, 8 x 8) in extended precision."""
    n = len(b)
    L = np.zeros((n, n), LD)
    for k in range(n):
        p = G[k, k] - (L[k, :k] * L[k, :k]).sum()
        if not p > 0:
            raise np.linalg.LinAlgError("not positive definite")
        L[k, k] = np.sqrt(p)
        for i in range(k + 1, n):
            L[i, k] = (G[i, k] - (L[i, :k] * L[k, :k]).sum()) / L[k, k]
    y = np.zeros(n, LD)
    for i in range(n):
        y[i] = (b[i] - (L[i, :i] * y[:i]).sum()) / L[i, i]
    x = np.zeros(n, LD)
    for i in range(n - 1, -1, -1):
        x[i] = (y[i] - (L[i + 1:, i] * x[i + 1:]).sum()) / L[i, i]
    return x


def gap(A, rhs, h, M):
    """The relative duality gap of h, in extended precision:
        y  = 2 clip(r, -M, M)
        y' = theta (y - A (A^T A)^-1 A^T y),  theta = min(1, 2 M / max|.|)
        D  = -sum y'^2 / 4 - rhs^T y'
        gap = (f(h) - D) / f(h), 0 when f(h) = 0
    D bounds the optimum from below for any h (Fenchel dual: phi*(y) = y^2 / 4 on |y| <= 2 M, subject to A^T y = 0)."""
    Al, bl, Ml = A.astype(LD), rhs.astype(LD), LD(M)
    r = Al @ np.asarray(h, LD) - bl
    f = phi(r, Ml).sum()
    if f == 0:
        return 0.0
    y = 2 * np.clip(r, -Ml, Ml)
    # columns scaled by exact powers of two, so that the Gram matrix is well scaled
    s = np.array([1.0 / S.pow2_near(float(c)) for c in np.sqrt((A * A).sum(axis=0))]).astype(LD)
    As = Al * s
    z = _chol_solve_ld(As.T @ As, As.T @ y)
    yp = y - As @ z
    m = np.abs(yp).max()
    theta = min(LD(1), 2 * Ml / m) if m > 0 else LD(1)
    yp = theta * yp
    D = -(yp * yp).sum() / 4 - bl @ yp
    return float((f - D) / f)


class Result(NamedTuple):
    h: np.ndarray        # (8,) float64
    f: float             # f(h), float64 arithmetic
    gap: float           # the gap of h in float64 arithmetic (what the kernel reports)
    iterations: int      # accepted steps
    converged: bool      # gap <= GAP_TOL
    fallbacks: int       # majorise-minimise steps among them
    clipped: float       # share of the rows with |r| > M at the returned h
    f0: float            # f(h0)


def _chol_solve(G, b):
    try:
        L = np.linalg.cholesky(G)
    except np.linalg.LinAlgError:
        return None
    return np.linalg.solve(L.T, np.linalg.solve(L, b))


def _gap64(As, rhs, hs, M):
    r = As @ hs - rhs
    f = phi(r, M).sum()
    if f == 0:
        return 0.0
    y = 2 * np.clip(r, -M, M)
    z = _chol_solve(As.T @ As, As.T @ y)
    if z is None:
        return np.inf
    yp = y - As @ z
    m = np.abs(yp).max()
    theta = min(1.0, 2 * M / m) if m > 0 else 1.0
    D = -theta * theta * (yp * yp).sum() / 4 - theta * (rhs @ yp)
    return float((f - D) / f)


def solve(A, rhs, M, h0, cap=DEFAULT_CAP):
    """The kernel's iteration from h0 (the least-squares solution), in the equilibrated variables h'' = h / s."""
    s = np.array([1.0 / S.pow2_near(c) for c in np.sqrt((A * A).sum(axis=0))])
    As = A * s
    h = np.asarray(h0, np.float64) / s
    alphas = 0.5 ** np.arange(HALVINGS)
    it = fallbacks = 0
    f0 = None

    def line(h, d, f):
        """(best alpha or None, f there, clipped set at alpha = 1)."""
        r = As @ h - rhs
        ad = As @ d
        fa = np.array([phi(r + a * ad, M).sum() for a in alphas])
        r1 = r + ad
        s1 = np.where(np.abs(r1) <= M, 0.0, np.sign(r1))
        k = int(np.argmin(fa))            # the first of equal minima: the largest step
        return (alphas[k], fa[k], s1, fa[0]) if fa[k] < f else (None, f, s1, fa[0])

    while True:
        r = As @ h - rhs
        clip = np.abs(r) > M
        sg = np.where(clip, np.sign(r), 0.0)
        f = float(phi(r, M).sum())
        if f0 is None:
            f0 = f
            if not clip.any():
                break
        if it == cap:
            break
        # Newton point of the active quadratic piece, as a correction: G0 d = -g
        U = As[~clip]
        g = U.T @ r[~clip] + M * (As[clip].T @ sg[clip])
        d = _chol_solve(U.T @ U, -g) if len(U) else None
        moved = False
        if d is not None:
            a, fa, s1, f1 = line(h, d, f)
            if np.array_equal(s1, sg) and f1 <= f:
                h = h + d
                it += 1
                break
            if a is not None:
                h = h + a * d
                it += 1
                moved = True
        if not moved:
            om = np.minimum(1.0, M / np.maximum(np.abs(r), 1e-300))
            d = _chol_solve((As * om[:, None]).T @ As, -(As.T @ (om * r)))
            if d is None:
                break
            a, fa, _, _ = line(h, d, f)
            if a is None:
                break
            h = h + a * d
            it += 1
            fallbacks += 1
    r = As @ h - rhs
    gp = _gap64(As, rhs, h, M)
    return Result(h * s, float(phi(r, M).sum()), gp, it, gp <= GAP_TOL, fallbacks, float((np.abs(r) > M).mean()), f0)


def solve_points(pts_c, pts_o, weights, M, cap=DEFAULT_CAP, floor=1e-3):
    """select -> rows -> least squares -> solve: (A, rhs, Result)."""
    pc, po, w = S.select(pts_c, pts_o, weights, floor)
    A, rhs = problem(pc, po, w)
    h0 = S.solve(pc, po, w, "lms")[0]
    return A, rhs, solve(A, rhs, M, h0, cap)
