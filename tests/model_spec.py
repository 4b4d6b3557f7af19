"""numpy specification of the spectral method's M-step (model.py's LMSSolver / SDPSolver) as the engine computes it
(cvx_proj_amd/csrc/apap_model.hip, DESIGN.md "M-step and EM loop").  Test infrastructure only: the product never imports it.

* ``rows``: A, rhs, A1, A2 in the reference's dtypes and rounding (model.py:29-35, :77-93).
* ``reduced``: K = [A | -rhs | A1[:, 0 3 6] | A2[:, 1 4 7]] (2n x 15), its R factor, and the equilibration the engine uses.
* ``phi``: the SDP's objective at h, max over the unit disc of ||q + [u v] delta||^2, from the 2n original rows.
* ``psi``: the lower bound min_h tr(Z G(h)) of a dual 3 x 3 block Z, after scaling Z onto the feasible set.
* ``tail``: model.py:50-56 / :117-123, the float32 solution (and its inverse when swap).
* ``ipm``: the primal-dual interior-point method of the solve kernel, on the 18 x 18 LMI, in numpy.
"""
from __future__ import annotations

import numpy as np

GAP_TOL = 1e-10
MAX_IT = 80
STEP = 0.98          # fraction of the step to the boundary of the cone
BISECT = 14          # bisection steps of the step-length search


def select(pts_c, pts_o, w, floor=1e-3):
    """spectral_method.py:165-180: the matches with w > floor, in order, as float32."""
    w = np.asarray(w, np.float32).ravel()
    keep = w.astype(np.float64) > floor if floor is not None else np.ones(len(w), bool)   # numpy 1.x compares in float64
    return (np.float32(np.asarray(pts_c)[keep]).reshape(-1, 2), np.float32(np.asarray(pts_o)[keep]).reshape(-1, 2),
            np.float32(w[keep]))


def get_shifted(pts, num_points, x=1.0):
    padded = np.concatenate([pts, np.repeat(np.float32([[x, 0, 0, 0]]), num_points, axis=0)], axis=-1)
    rolled = np.roll(padded, shift=3, axis=-1)
    return np.concatenate([np.expand_dims(padded, axis=-2), np.expand_dims(rolled, axis=-2)], axis=-2)


def rows(pts_c, pts_o, weights, du=1.0, dv=1.0):
    """(A float32 (2n, 8), rhs float32 (2n, 1), A1 float64 (2n, 8), A2 float64 (2n, 8)) exactly as SDPSolver.solve builds them."""
    pts_c = np.asarray(pts_c, np.float32)
    pts_o = np.asarray(pts_o, np.float32)
    n = pts_c.shape[0]
    rare = -pts_o[..., None] @ pts_c[:, None, :]
    front = get_shifted(pts_c, n)
    w = np.repeat(np.asarray(weights, np.float32)[..., None], repeats=2, axis=-1).reshape(-1, 1)
    A = np.concatenate([front, rare], axis=-1).reshape(-1, 8) * w
    rhs = pts_o.reshape(-1, 1) * w
    u_p = np.repeat(np.float32([[du, 0]]), repeats=n, axis=0)
    u_rare = np.hstack((-pts_o.reshape(-1, 1), np.zeros((n << 1, 1)))) * du
    A1 = np.concatenate([get_shifted(u_p, n, 0.0).reshape(-1, 6), u_rare], axis=-1) * w
    v_p = np.repeat(np.float32([[0, dv]]), repeats=n, axis=0)
    v_rare = np.hstack((np.zeros((n << 1, 1)), -pts_o.reshape(-1, 1))) * dv
    A2 = np.concatenate([get_shifted(v_p, n, 0.0).reshape(-1, 6), v_rare], axis=-1) * w
    return A, rhs, A1, A2


def K_of(A, rhs, A1, A2):
    return np.hstack([A.astype(np.float64), -rhs.astype(np.float64), A1[:, [0, 3, 6]], A2[:, [1, 4, 7]]])


def pow2_near(x):
    """The power of two nearest x on a log scale (1 for 0 / non-finite): x = m 2^e, m in [1/2, 1) -> 2^e if m >= sqrt(1/2),
    else 2^(e - 1).  An exact scale."""
    if not (np.isfinite(x) and x > 0):
        return 1.0
    m, e = np.frexp(x)
    return float(np.ldexp(1.0, int(e) if m >= np.sqrt(0.5) else int(e) - 1))


def equilibrate(R):
    """(R'', s (8,), sigma): R'' = R D with D = diag(s for h's columns, 1 / sigma for the rhs column, s of the matching h for the
    A1 / A2 columns); every entry a power of two.  h = sigma * s * h'', r = sigma^2 r'', t = sigma^2 t''."""
    cn = np.sqrt((R * R).sum(axis=0))
    s = np.array([1.0 / pow2_near(c) for c in cn[:8]])
    sigma = pow2_near(cn[8])
    d = np.concatenate([s, [1.0 / sigma], s[[0, 3, 6]], s[[1, 4, 7]]])
    return R * d[None, :], s, sigma


def reduced(pts_c, pts_o, weights, du=1.0, dv=1.0):
    """R (15 x 15, upper, diagonal >= 0) of K from numpy's QR."""
    K = K_of(*rows(pts_c, pts_o, weights, du, dv))
    R = np.zeros((15, 15))
    r = np.linalg.qr(K, mode="r")
    R[:r.shape[0]] = r
    R = R * np.where(np.diag(R) < 0, -1.0, 1.0)[:, None]
    return K, R


# ---------------------------------------------------------------- the 18 x 18 LMI in (h'', r'', t'')
def lmi_basis(R):
    """F0 and F_1..F_10 of S(x) = F0 + sum x_i F_i = [[I_15, R X(h)], [(R X(h))^T, diag(r, r, t)]], P = [u v q]."""
    F = np.zeros((11, 18, 18))
    F[0, :15, :15] = np.eye(15)

    def off(k, col, vec):
        F[k, :15, 15 + col] += vec
        F[k, 15 + col, :15] += vec
    off(0, 2, R[:, 8])
    for j in range(8):
        off(j + 1, 2, R[:, j])
        if j % 3 == 0:
            off(j + 1, 0, R[:, 9 + j // 3])
        if j % 3 == 1:
            off(j + 1, 1, R[:, 12 + j // 3])
    F[9, 15, 15] = F[9, 16, 16] = 1.0
    F[10, 17, 17] = 1.0
    return F


def gram(R, h):
    """G = (R X(h))^T (R X(h)), 3 x 3, order (u, v, q)."""
    X = np.zeros((15, 3))
    X[:8, 2] = h
    X[8, 2] = 1.0
    X[9:12, 0] = h[[0, 3, 6]]
    X[12:15, 1] = h[[1, 4, 7]]
    RX = R @ X
    return RX.T @ RX


def _chol_ok(A):
    try:
        np.linalg.cholesky(A)
        return True
    except np.linalg.LinAlgError:
        return False


def max_step(A, dA):
    """The step length of the kernel: 1 when A + dA / STEP stays positive definite, else STEP x the largest feasible
    point of a BISECT-step bisection of [0, 1 / STEP]."""
    hi = 1.0 / STEP
    if _chol_ok(A + hi * dA):
        return 1.0
    lo = 0.0
    for _ in range(BISECT):
        mid = 0.5 * (lo + hi)
        if _chol_ok(A + mid * dA):
            lo = mid
        else:
            hi = mid
    return STEP * lo


def ipm(R, h0):
    """Primal-dual path following (HKM direction, Mehrotra predictor-corrector) from the strictly feasible pair
    x = (h0, tau, tau), Z = diag(zeta I_15, 1/2, 1/2, 1).  R: the equilibrated factor.  Returns (x (10,), Z (18, 18), gap,
    iterations, converged); gap = tr(S Z) / (r + t).  The kernel's guards: when rounding pushes S out of the cone, or the
    Schur matrix is no longer positive definite (near-collinear points, at gaps just above GAP_TOL), the loop ends there and
    the best iterate is returned with converged False."""
    F = lmi_basis(R)
    c = np.zeros(10)
    c[8:] = 1.0
    G = gram(R, h0)
    tau = 2.0 * np.trace(G) + 1e-12
    x = np.concatenate([h0, [tau, tau]])
    Z = np.diag(np.concatenate([np.full(15, 0.5 * tau), [0.5, 0.5, 1.0]]))

    def S_of(x):
        return F[0] + np.tensordot(x, F[1:], axes=1)

    best = None
    for it in range(MAX_IT + 1):
        S = S_of(x)
        gap_abs = float(np.sum(S * Z))
        rel = gap_abs / max(x[8] + x[9], 1e-300)
        if best is None or rel < best[2]:
            best = (x.copy(), Z.copy(), rel, it)
        if rel <= GAP_TOL or it == MAX_IT:
            break
        mu = gap_abs / 18.0
        if not _chol_ok(S):
            break
        Si = np.linalg.inv(S)
        B = [F[1 + i] @ Si for i in range(10)]           # F_i S^-1
        FZ = [F[1 + j] @ Z for j in range(10)]           # F_j Z
        Mx = np.array([[np.sum(B[i] * FZ[j].T) for j in range(10)] for i in range(10)])   # tr(F_i S^-1 F_j Z)
        g = np.array([np.trace(Si @ F[1 + i]) for i in range(10)])
        try:
            L = np.linalg.cholesky(Mx)
        except np.linalg.LinAlgError:
            break

        def solve(rhs):
            return np.linalg.solve(L.T, np.linalg.solve(L, rhs))

        def dirs(dx, extra):
            dS = np.tensordot(dx, F[1:], axes=1)
            dZ = extra - Z - Si @ dS @ Z
            return dS, 0.5 * (dZ + dZ.T)
        # predictor
        dx = solve(-c)
        dSa, dZa = dirs(dx, 0.0)
        ap, ad = max_step(S, dSa), max_step(Z, dZa)
        mu_aff = float(np.sum((S + ap * dSa) * (Z + ad * dZa))) / 18.0
        sig = min(1.0, (mu_aff / mu) ** 3)
        # corrector
        C = Si @ dSa @ dZa
        rhs = sig * mu * g - c - np.array([np.sum(F[1 + i] * C.T) for i in range(10)])
        dx = solve(rhs)
        dS, dZ = dirs(dx, sig * mu * Si - C)
        ap, ad = max_step(S, dS), max_step(Z, dZ)
        x = x + ap * dx
        Z = Z + ad * dZ
    x, Z, rel, it_best = best
    return x, Z, rel, it, rel <= GAP_TOL


def lms(R):
    """h'' of min ||A h - rhs||^2 by back-substitution on the leading 9 x 9 block of the equilibrated R."""
    return np.linalg.solve(np.triu(R[:8, :8]), -R[:8, 8])


def solve(pts_c, pts_o, weights, mode, du=1.0, dv=1.0):
    """(h float64 (8,), r, t, Z 3 x 3, gap, iterations) as the engine defines them; mode 'lms' or 'sdp'."""
    _, R = reduced(pts_c, pts_o, weights, du, dv)
    Re, s, sigma = equilibrate(R)
    h0 = lms(Re)
    if mode == "lms":
        return sigma * s * h0, None, None, None, 0.0, 0
    x, Z, gap, it, _ = ipm(Re, h0)
    return sigma * s * x[:8], sigma ** 2 * x[8], sigma ** 2 * x[9], Z[15:, 15:], gap, it


# ---------------------------------------------------------------- certificates
def uvq(pts_c, pts_o, weights, h, du=1.0, dv=1.0):
    """u = A1 h, v = A2 h, q = A h - rhs from the original rows, in extended precision."""
    A, rhs, A1, A2 = rows(pts_c, pts_o, weights, du, dv)
    hl = np.asarray(h, np.longdouble)
    return (A1.astype(np.longdouble) @ hl, A2.astype(np.longdouble) @ hl,
            A.astype(np.longdouble) @ hl - rhs.astype(np.longdouble).ravel())


def phi(pts_c, pts_o, weights, h, du=1.0, dv=1.0):
    """max_{|delta| <= 1} ||q + [u v] delta||^2: convex in delta, so the maximum lies on the unit circle; dense sampling,
    then Newton on the derivative of the trigonometric quadratic."""
    u, v, q = uvq(pts_c, pts_o, weights, h, du, dv)
    uu, vv, qq, uv, qu, qv = (float(np.dot(a, b)) for a, b in ((u, u), (v, v), (q, q), (u, v), (q, u), (q, v)))

    def f(th):
        c, s = np.cos(th), np.sin(th)
        return qq + uu * c * c + vv * s * s + 2 * qu * c + 2 * qv * s + 2 * uv * c * s
    th = np.linspace(0, 2 * np.pi, 4097)[:-1]
    vals = f(th)
    best = float(vals.max())
    for t0 in th[np.argsort(vals)[-4:]]:
        t = float(t0)
        for _ in range(60):
            c, s = np.cos(t), np.sin(t)
            d1 = 2 * (vv - uu) * s * c - 2 * qu * s + 2 * qv * c + 2 * uv * (c * c - s * s)
            d2 = 2 * (vv - uu) * (c * c - s * s) - 2 * qu * c - 2 * qv * s - 8 * uv * s * c
            if d2 >= 0:
                break
            t -= d1 / d2
        best = max(best, float(f(t)))
    return best


def feasible_Z(Z):
    """Z >= 0 with Z11 + Z22 = 1 and Z33 = 1: symmetrise, clip negative eigenvalues, rescale by diag(a, a, b) (a congruence:
    positive semidefiniteness is kept)."""
    Z = 0.5 * (np.asarray(Z, np.float64) + np.asarray(Z, np.float64).T)
    w, V = np.linalg.eigh(Z)
    Z = (V * np.clip(w, 0, None)) @ V.T
    d = np.array([1 / np.sqrt(Z[0, 0] + Z[1, 1]), 1 / np.sqrt(Z[0, 0] + Z[1, 1]), 1 / np.sqrt(Z[2, 2])])
    return Z * d[:, None] * d[None, :]


def psi(pts_c, pts_o, weights, Z, du=1.0, dv=1.0):
    """min_h tr(Z G(h)) = min_h ||[u v q] L||_F^2 (Z = L L^T) for the feasible Z: a float64 least-squares problem in h."""
    Z = feasible_Z(Z)
    w, V = np.linalg.eigh(Z)
    L = V * np.sqrt(np.clip(w, 0, None))
    A, rhs, A1, A2 = rows(pts_c, pts_o, weights, du, dv)
    A = A.astype(np.float64)
    rhs = rhs.astype(np.float64).ravel()
    # column k of P L = L[0,k] A1 h + L[1,k] A2 h + L[2,k] (A h - rhs)
    M = np.vstack([L[0, k] * A1 + L[1, k] * A2 + L[2, k] * A for k in range(3)])
    b = np.concatenate([L[2, k] * rhs for k in range(3)])
    cn = np.sqrt((M * M).sum(axis=0))
    cn[cn == 0] = 1
    h = np.linalg.lstsq(M / cn, b, rcond=None)[0] / cn
    res = M.astype(np.longdouble) @ h.astype(np.longdouble) - b.astype(np.longdouble)
    return float(np.dot(res, res))


def tail(h, swap=True):
    """model.py:50-56: the float32 solution with [2, 2] = 1, inverted and normalised in float32 when swap."""
    sol = np.ones(9, dtype=np.float32)
    sol[:-1] = np.asarray(h, np.float64).ravel()
    sol = sol.reshape(3, 3)
    if swap:
        sol = np.linalg.inv(sol)
        sol /= sol[-1, -1]
    return sol
