"""Numpy specification of this repository's fundamental-matrix estimator (TEST INFRASTRUCTURE, not product): the contract of
``cv.findFundamentalMat(src, dst, cv.FM_RANSAC, thresh)``, NOT a restatement of OpenCV's code (sampler, adaptive stopping and
polish differ).  It pins csrc/apap_fundamental.hip bit for bit: everything below is float64, every product, sum and quotient
is rounded on its own (numpy's elementwise operations never fuse), and only ``+ - * / sqrt`` and comparisons are used.

Convention: ``src`` holds the centre picture's points, ``dst`` the other picture's; ``dst_h^T F src_h = 0`` (calculate_M's
``epi_vectors = F @ homo_src.T`` dotted with ``homo_dst``).  F is 3 x 3 float64, row-major.

A matrix that is "no model" is nine copies of ``np.nan`` (the positive quiet NaN, 0x7ff8000000000000): every place where a
NaN could reach an output replaces the whole matrix by that value, so that no platform's NaN sign or payload shows.
"""
from __future__ import annotations

import numpy as np

ITERATIONS = 2048
SEED = 0x5EEDC0DE5EEDC0DE
MIN_POINTS = 8
LANES = 256            # the re-fit's block: lane t sums inliers t, t + 256, ...
SWEEP_CAP = 30         # of both Jacobi iterations
_UPPER = [(i, j) for i in range(9) for j in range(i, 9)]      # the 45 distinct entries of A^T A, row-major


def splitmix64(x):
    x = np.asarray(x, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = x + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def sample(n, iterations=ITERATIONS, seed=SEED):
    """(iterations, 8) distinct indices below ``n``: draw j of hypothesis h is the high 32 bits of
    ``splitmix64(seed + 8 h + j)`` (mod 2^64) modulo ``n - j``, stepped over the earlier picks in ascending order."""
    assert n >= MIN_POINTS
    h = np.arange(iterations, dtype=np.uint64)
    picks = np.zeros((iterations, 8), dtype=np.int64)
    with np.errstate(over="ignore"):
        for j in range(8):
            r = (splitmix64(np.uint64(seed) + h * np.uint64(8) + np.uint64(j)) >> np.uint64(32)).astype(np.int64)
            p = r % (n - j)
            prev = np.sort(picks[:, :j], axis=1)
            for k in range(j):
                p = p + (p >= prev[:, k])
            picks[:, j] = p
    return picks


def box(pts):
    """(cx, cy, s, extent) of the bounding box of float32 points: c = (lo + hi) / 2, s = 2 / max extent."""
    pts = np.ascontiguousarray(pts, dtype=np.float32)
    lo = pts.min(axis=0).astype(np.float64)
    hi = pts.max(axis=0).astype(np.float64)
    c = (lo + hi) / 2.0
    ex, ey = hi[0] - lo[0], hi[1] - lo[1]
    ext = ex if ex > ey else ey
    with np.errstate(all="ignore"):
        s = np.float64(2.0) / ext
    return np.array([c[0], c[1], s, ext])


def normalise(pts, b):
    p = np.ascontiguousarray(pts, dtype=np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        return (p[..., 0] - b[0]) * b[2], (p[..., 1] - b[1]) * b[2]


def rows9(x, y, u, v):
    """The epipolar constraint's row of one match, stacked on the last axis."""
    return np.stack([u * x, u * y, u, v * x, v * y, v, x, y, np.ones_like(x)], axis=-1)


def minimal_solve(x, y, u, v):
    """Null vectors of K systems of 8 rows: ``x y u v`` (K, 8) normalised.  Gaussian elimination with complete pivoting (the
    largest |a| of the remaining block, the first in row-major order; NaN never wins), the column never chosen gets 1, back
    substitution from row 7 up with the terms subtracted in ascending column order.  (K, 9); NaN rows where a pivot was zero
    or not finite."""
    K = x.shape[0]
    a = rows9(x, y, u, v)
    perm = np.tile(np.arange(9), (K, 1))
    ok = np.ones(K, dtype=bool)
    rows = np.arange(K)
    with np.errstate(all="ignore"):
        for c in range(8):
            blk = np.abs(a[:, c:, c:])
            key = np.where(np.isnan(blk), -1.0, blk).reshape(K, -1)
            idx = np.argmax(key, axis=1)
            pr, pc = c + idx // (9 - c), c + idx % (9 - c)
            tmp = a[rows, pr].copy()
            a[rows, pr] = a[:, c]
            a[:, c] = tmp
            tmp = a[rows, :, pc].copy()
            a[rows, :, pc] = a[:, :, c]
            a[:, :, c] = tmp
            tmp = perm[rows, pc].copy()
            perm[rows, pc] = perm[:, c]
            perm[:, c] = tmp
            piv = a[:, c, c]
            ok &= (piv != 0) & np.isfinite(piv)
            for r in range(c + 1, 8):
                f = a[:, r, c] / piv
                a[:, r, c + 1:] = a[:, r, c + 1:] - f[:, None] * a[:, c, c + 1:]
        sol = np.zeros((K, 9))
        sol[:, 8] = 1.0
        for i in range(7, -1, -1):
            s = -a[:, i, 8]
            for j in range(i + 1, 8):
                s = s - a[:, i, j] * sol[:, j]
            sol[:, i] = s / a[:, i, i]
    f = np.empty((K, 9))
    f[rows[:, None], perm] = sol
    f[~ok] = np.nan
    return f


def denormalise(Fn, bs, bd):
    """``T_d^T F_n T_s`` for (K, 9) matrices: G = F_n T_s column by column, then T_d^T G row by row."""
    F = Fn.reshape(-1, 3, 3)
    ss, csx, csy = bs[0:3][[2, 0, 1]]
    sd, cdx, cdy = bd[0:3][[2, 0, 1]]
    with np.errstate(all="ignore"):
        g0 = F[:, :, 0] * ss
        g1 = F[:, :, 1] * ss
        g2 = (F[:, :, 2] - g0 * csx) - g1 * csy
        G = np.stack([g0, g1, g2], axis=-1)
        r0 = G[:, 0] * sd
        r1 = G[:, 1] * sd
        r2 = (G[:, 2] - r0 * cdx) - r1 * cdy
    return np.stack([r0, r1, r2], axis=1).reshape(-1, 9)


def canonical(F9):
    """Rows with a non-finite entry become all ``np.nan``."""
    F9 = F9.copy()
    F9[~np.isfinite(F9).all(axis=1)] = np.nan
    return F9


def sampson_inliers(F9, src, dst, thr2):
    """(K, n) bool: r^2 / (a1^2 + a2^2 + b1^2 + b2^2) <= thr2 with r = d^T F s, a = F s, b = F^T d; NaN compares false."""
    x, y = src[:, 0].astype(np.float64), src[:, 1].astype(np.float64)
    u, v = dst[:, 0].astype(np.float64), dst[:, 1].astype(np.float64)
    f = F9[:, :, None]
    with np.errstate(all="ignore"):
        a1 = (f[:, 0] * x + f[:, 1] * y) + f[:, 2]
        a2 = (f[:, 3] * x + f[:, 4] * y) + f[:, 5]
        a3 = (f[:, 6] * x + f[:, 7] * y) + f[:, 8]
        r = (u * a1 + v * a2) + a3
        b1 = (f[:, 0] * u + f[:, 3] * v) + f[:, 6]
        b2 = (f[:, 1] * u + f[:, 4] * v) + f[:, 7]
        den = ((a1 * a1 + a2 * a2) + b1 * b1) + b2 * b2
        return (r * r) / den <= thr2


def moments(x, y, u, v, mask):
    """The 45 distinct entries of A^T A over the inliers, in the re-fit kernel's tree: lane t of 256 adds the products of
    inliers t, t + 256, ... in ascending order to a sum that starts at 0 (non-inliers are skipped); per wave of 64 lanes
    ``v[l] += v[l + d]`` for d = 32, 16, .. 1; the four waves are added in ascending order."""
    n = len(x)
    acc = np.zeros((LANES, 45))
    iu = np.array([i for i, _ in _UPPER])
    ju = np.array([j for _, j in _UPPER])
    for k0 in range(0, n, LANES):
        k = np.arange(k0, min(k0 + LANES, n))
        keep = mask[k].astype(bool)
        k = k[keep]
        r = rows9(x[k], y[k], u[k], v[k])
        lanes = k - k0
        acc[lanes] = acc[lanes] + r[:, iu] * r[:, ju]
    w = acc.reshape(4, 64, 45).copy()
    d = 32
    while d:
        w[:, :d] = w[:, :d] + w[:, d:2 * d]
        d //= 2
    return ((w[0, 0] + w[1, 0]) + w[2, 0]) + w[3, 0]


def _angle(diff, off):
    """t, c, s of the rotation that annihilates ``off`` given the difference of the two diagonal terms."""
    with np.errstate(all="ignore"):
        theta = diff / (off + off)
        t = 1.0 / (abs(theta) + np.sqrt(theta * theta + 1.0))
        if theta < 0:
            t = -t
        c = 1.0 / np.sqrt(t * t + 1.0)
        return t, c, t * c


# The round-robin order of the Jacobi sweep: round r turns the four disjoint pairs {(r + k) % 9, (r - k) % 9}, k = 1 .. 4, at
# once (index r rests); the nine rounds hold each of the 36 pairs once.
_ABOVE = np.triu_indices(9, 1)
ROUNDS = [[(min((r + k) % 9, (r - k) % 9), max((r + k) % 9, (r - k) % 9)) for k in (1, 2, 3, 4)] for r in range(9)]


def jacobi_eigen(m45):
    """Cyclic Jacobi on the symmetric 9 x 9 matrix of the 45 sums, in the order ROUNDS.  A pair (p, q) whose a_pq is exactly
    zero is passed over; one with |a_pp| + 100 |a_pq| == |a_pp| and the same for a_qq has a_pq set to zero without a rotation;
    the others are rotated, all from the round's incoming matrix: the columns first (p' = c p - s q, q' = s p + c q), then the
    rows of that, the entries on and above the diagonal kept and mirrored; a rotated pair's own entries are a_pp - t a_pq,
    a_qq + t a_pq and 0.  The iteration stops after the first sweep without a rotation, or after SWEEP_CAP sweeps.
    Returns (A, V)."""
    A = np.zeros((9, 9))
    for k, (i, j) in enumerate(_UPPER):
        A[i, j] = A[j, i] = m45[k]
    V = np.eye(9)
    with np.errstate(all="ignore"):
        for _ in range(SWEEP_CAP):
            rotated = False
            for pairs in ROUNDS:
                turns, zeroed = [], []
                for p, q in pairs:
                    apq, app, aqq = A[p, q], A[p, p], A[q, q]
                    if apq == 0.0:
                        continue
                    g = 100.0 * abs(apq)
                    if abs(app) + g == abs(app) and abs(aqq) + g == abs(aqq):
                        zeroed.append((p, q))
                        continue
                    rotated = True
                    turns.append((p, q) + _angle(aqq - app, apq) + (apq, app, aqq))
                B, Vn = A.copy(), V.copy()
                for p, q, t, c, s, *_ in turns:
                    B[:, p], B[:, q] = c * A[:, p] - s * A[:, q], s * A[:, p] + c * A[:, q]
                    Vn[:, p], Vn[:, q] = c * V[:, p] - s * V[:, q], s * V[:, p] + c * V[:, q]
                Cm = B.copy()
                for p, q, t, c, s, *_ in turns:
                    Cm[p, :], Cm[q, :] = c * B[p, :] - s * B[q, :], s * B[p, :] + c * B[q, :]
                Cm[_ABOVE[1], _ABOVE[0]] = Cm[_ABOVE]
                for p, q, t, c, s, apq, app, aqq in turns:
                    Cm[p, p], Cm[q, q] = app - t * apq, aqq + t * apq
                    Cm[p, q] = Cm[q, p] = 0.0
                for p, q in zeroed:
                    Cm[p, q] = Cm[q, p] = 0.0
                A, V = Cm, Vn
            if not rotated:
                break
    return A, V


def smallest_eigenvector(m45):
    A, V = jacobi_eigen(m45)
    d = np.diag(A)
    k = 0
    for i in range(1, 9):
        if d[i] < d[k]:
            k = i
    return V[:, k].copy()


def rank2(f9):
    """One-sided (Hestenes) Jacobi on the columns of the 3 x 3: pairs (0, 1), (0, 2), (1, 2); a pair whose inner product gamma
    is zero, or has sqrt(alpha beta) + |gamma| == sqrt(alpha beta), is passed over.  The column of smallest squared norm (the
    first such) is then zeroed and the matrix rebuilt as G W^T."""
    G = f9.reshape(3, 3).copy()
    W = np.eye(3)
    dot = lambda a, b: (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]      # noqa: E731
    with np.errstate(all="ignore"):
        for _ in range(SWEEP_CAP):
            rotated = False
            for p, q in ((0, 1), (0, 2), (1, 2)):
                alpha, beta, gamma = dot(G[:, p], G[:, p]), dot(G[:, q], G[:, q]), dot(G[:, p], G[:, q])
                if gamma == 0.0:
                    continue
                lim = np.sqrt(alpha * beta)
                if lim + abs(gamma) == lim:
                    continue
                rotated = True
                _, c, s = _angle(beta - alpha, gamma)
                for M in (G, W):
                    mp, mq = M[:, p].copy(), M[:, q].copy()
                    M[:, p], M[:, q] = c * mp - s * mq, s * mp + c * mq
            if not rotated:
                break
        norms = [dot(G[:, k], G[:, k]) for k in range(3)]
        k = 0
        for i in (1, 2):
            if norms[i] < norms[k]:
                k = i
        G[:, k] = 0.0
        out = np.empty((3, 3))
        for i in range(3):
            for j in range(3):
                out[i, j] = (G[i, 0] * W[j, 0] + G[i, 1] * W[j, 1]) + G[i, 2] * W[j, 2]
    return out.reshape(9)


def scale_and_sign(Fp9, src):
    """F / g with g = max_k sqrt(a1^2 + a2^2), a = F s_k (NaN terms are passed over, the maximum starts at 0), then the first
    entry of largest magnitude made positive.  All NaN when g is zero or not finite, or an entry of the result is not."""
    x, y = src[:, 0].astype(np.float64), src[:, 1].astype(np.float64)
    f = Fp9
    with np.errstate(all="ignore"):
        a1 = (f[0] * x + f[1] * y) + f[2]
        a2 = (f[3] * x + f[4] * y) + f[5]
        v = np.sqrt(a1 * a1 + a2 * a2)
        g = 0.0
        for t in v[~np.isnan(v)]:
            if t > g:
                g = t
        if not (g > 0.0) or not np.isfinite(g):
            return np.full(9, np.nan)
        out = f / g
    if not np.isfinite(out).all():
        return np.full(9, np.nan)
    k = 0
    for i in range(1, 9):
        if abs(out[i]) > abs(out[k]):
            k = i
    return -out if out[k] < 0 else out


def refit(src, dst, mask, bs, bd):
    """Steps 7 and 8 on the inliers ``mask``: (9,) float64, all NaN for fewer than 8 inliers or a degenerate scale."""
    if int(np.count_nonzero(mask)) < MIN_POINTS:
        return np.full(9, np.nan)
    x, y = normalise(src, bs)
    u, v = normalise(dst, bd)
    f = smallest_eigenvector(moments(x, y, u, v, mask))
    Fp = denormalise(rank2(f)[None], bs, bd)[0]
    return scale_and_sign(Fp, np.ascontiguousarray(src, dtype=np.float32))


def hypotheses(src, dst, picks, bs, bd):
    """(K, 9) denormalised hypotheses, all NaN where the minimal solve failed or an entry is not finite."""
    xs, ys = normalise(src[picks], bs)
    us, vs = normalise(dst[picks], bd)
    return canonical(denormalise(minimal_solve(xs, ys, us, vs), bs, bd))


def core(src, dst, thresh=3.0, iterations=ITERATIONS, seed=SEED):
    """Everything the kernels leave behind: ``dict(box (8,), picks, H (K, 9), counts, best, count, mask, winner (9,), F (9,))``.
    ``mask`` is the winner's inliers also when there are fewer than 8 (the device form's mask)."""
    src = np.ascontiguousarray(src, dtype=np.float32).reshape(-1, 2)
    dst = np.ascontiguousarray(dst, dtype=np.float32).reshape(-1, 2)
    bs, bd = box(src), box(dst)
    picks = sample(len(src), iterations, seed)
    H = hypotheses(src, dst, picks, bs, bd)
    thr2 = np.float64(thresh) * np.float64(thresh)
    counts = np.empty(iterations, dtype=np.int64)
    inl_best = None
    for k0 in range(0, iterations, 256):      # in slabs: (K, n) temporaries stay small
        inl = sampson_inliers(H[k0:k0 + 256], src, dst, thr2)
        counts[k0:k0 + 256] = inl.sum(axis=1)
    best = int(np.argmax(counts))
    inl_best = sampson_inliers(H[best:best + 1], src, dst, thr2)[0]
    mask = inl_best.astype(np.uint8)
    F = refit(src, dst, mask, bs, bd)
    return dict(box=np.concatenate([bs, bd]), picks=picks, H=H, counts=counts, best=best, count=int(counts[best]), mask=mask,
                winner=H[best].copy(), F=F)


def find_fundamental(src, dst, thresh=3.0, iterations=ITERATIONS, seed=SEED):
    """``(F (3, 3) float64 or None, mask (n, 1) uint8)``: what ``_native.find_fundamental_ransac`` returns."""
    c = core(src, dst, thresh, iterations, seed)
    if c["count"] < MIN_POINTS or not np.isfinite(c["F"]).all():
        return None, np.zeros((len(c["mask"]), 1), dtype=np.uint8)
    return c["F"].reshape(3, 3), c["mask"].reshape(-1, 1)
