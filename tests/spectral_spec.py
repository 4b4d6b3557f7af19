"""Specification of the spectral match weighting in numpy / scipy (test infrastructure; the product never imports it).

It restates the contract of DESIGN.md "Spectral match weighting": the float32 affinity and its fp64 diagonal in the set-up
kernel's stated order, ``recompute_matching`` in float32, the eigenpair of largest |lambda| from LAPACK / ARPACK, the
finishing step, and the bound within which an engine that honours ``|M v - lambda v| <= 1e-13 |lambda|`` must meet it.
``lanczos_cycles`` emulates the restarted iteration in float64 - only to classify an input (one cycle, several, breakdown),
never to be compared number for number.  ``cases()`` lists the seeded inputs of tests/test_spectral_spec.py and
tests/test_gpu_spectral_edges.py; ``build(case)`` makes one, moving to the next seed until its conditions hold.
"""
import numpy as np

DIM = 128
BASIS = 64            # Krylov basis of the engine
TOL = 1e-13           # kSpecTol: converged means |M v - lambda v| <= TOL |lambda|
BREAKDOWN = 1e-15     # kSpecBreakdown: beta <= BREAKDOWN |T| ends a cycle early
MAX_CYCLES = 30
EIGH_MAX = 2100       # up to here the whole spectrum (LAPACK); above, four eigenpairs of largest magnitude (ARPACK)
LONGDOUBLE_MAX = 4100
MAX_SEEDS = 20
SEVERAL_MARGIN = 100.0   # a case meant to need >= 2 cycles: the emulated residual after the first is >= this x TOL


class Opts:
    """The options of calculate_M (defaults: the reference's options.py)."""

    def __init__(self, epi_weight=0.5, affinity_eps=30.0, aff_thresh=0.5, em_radius=6.0, score_thresh=0.4):
        self.epi_weight, self.affinity_eps, self.aff_thresh = float(epi_weight), float(affinity_eps), float(aff_thresh)
        self.em_radius, self.score_thresh = float(em_radius), float(score_thresh)

    def kw(self):
        return dict(epi_weight=self.epi_weight, affinity_eps=self.affinity_eps, aff_thresh=self.aff_thresh,
                    em_radius=self.em_radius, score_thresh=self.score_thresh)

    def values(self):
        return (self.epi_weight, self.affinity_eps, self.aff_thresh, self.em_radius, self.score_thresh)


# ------------------------------------------------------------------ the affinity
def pairwise128(a):
    """numpy's float32 pairwise sum of 128 terms (8 accumulators) along the last axis, as the set-up kernel sums."""
    r = a[..., :8].copy()
    for i in range(8, 128, 8):
        r = r + a[..., i:i + 8]
    return ((r[..., 0] + r[..., 1]) + (r[..., 2] + r[..., 3])) + ((r[..., 4] + r[..., 5]) + (r[..., 6] + r[..., 7]))


def off_diagonal_f32(src, dst, affinity_eps, rows=512):
    """spectral_method.py:116-123 restated: every step float32, rounded separately, the diagonal set to 0.  Built ``rows``
    rows at a time: the (n, n, 2) temporaries of the one-shot form are 0.5 GB each at n = 8193."""
    src = np.asarray(src, np.float32)
    dst = np.asarray(dst, np.float32)
    n = len(src)
    rcp = np.float32(1 / 2 / (affinity_eps ** 2))
    off = np.empty((n, n), np.float32)
    for a in range(0, n, rows):
        ds = src[a:a + rows, None, :] - src[None, :, :]
        dd = dst[a:a + rows, None, :] - dst[None, :, :]
        s = ds[..., 0] * ds[..., 0] + ds[..., 1] * ds[..., 1]
        d = dd[..., 0] * dd[..., 0] + dd[..., 1] * dd[..., 1]
        t = s - d
        off[a:a + rows] = np.maximum(np.float32(4.5) - (t * t) * rcp, np.float32(0))
    np.fill_diagonal(off, 0)
    assert off.dtype == np.float32
    return off


def match_score(c, o):
    """sum(c / |c| * o / |o|) in float32, norms and sum in the 8-accumulator order."""
    c = np.asarray(c, np.float32)
    o = np.asarray(o, np.float32)
    nc = np.sqrt(pairwise128(c * c))[:, None]
    no = np.sqrt(pairwise128(o * o))[:, None]
    ms = pairwise128((c / nc) * (o / no))
    assert ms.dtype == np.float32
    return ms


def diagonal(src, dst, ms, F, epi_weight):
    """M_ii = float64(match_score) + epi_weight / (1 + epi), epi = |(u e0 + v e1) + e2|, e_r = (F[r,0] x + F[r,1] y) + F[r,2]."""
    F = np.asarray(F, np.float64)
    src = np.asarray(src, np.float32)
    dst = np.asarray(dst, np.float32)
    x, y = src[:, 0].astype(np.float64), src[:, 1].astype(np.float64)
    u, v = dst[:, 0].astype(np.float64), dst[:, 1].astype(np.float64)
    e = [(F[r, 0] * x + F[r, 1] * y) + F[r, 2] for r in range(3)]
    epi = np.abs((u * e[0] + v * e[1]) + e[2])
    return ms.astype(np.float64) + epi_weight / (1.0 + epi)


def affinity(src, dst, c, o, F, opts):
    """(diag float64 (n,), off float32 (n, n)) of the symmetric M."""
    return diagonal(src, dst, match_score(c, o), F, opts.epi_weight), off_diagonal_f32(src, dst, opts.affinity_eps)


def dense(diag, off):
    """M in float64 (every float32 entry is exact in it)."""
    M = off.astype(np.float64)
    np.fill_diagonal(M, diag)
    return M


def initial_mask(src, dst, ms, Hg, opts):
    """recompute_matching in float32, in the set-up kernel's order: k_r = (Hg[r,0] u + Hg[r,1] v) + Hg[r,2], the two
    divisions, sqrt(ex*ex + ey*ey), each step rounded separately; the two comparisons in float64.  k2 = 0 gives an infinite
    or NaN distance: mask 0."""
    Hg = np.asarray(Hg, np.float32)
    src = np.asarray(src, np.float32)
    dst = np.asarray(dst, np.float32)
    u, v = dst[:, 0], dst[:, 1]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        k = [(Hg[r, 0] * u + Hg[r, 1] * v) + Hg[r, 2] for r in range(3)]
        ex = k[0] / k[2] - src[:, 0]
        ey = k[1] / k[2] - src[:, 1]
        dist = np.sqrt(ex * ex + ey * ey)
        assert dist.dtype == np.float32
        keep = (dist.astype(np.float64) < opts.em_radius) & (np.asarray(ms, np.float32).astype(np.float64) > opts.score_thresh)
    return keep.astype(np.float32)


# ------------------------------------------------------------------ the eigenpair and the finish
def principal(diag, off, M=None):
    """(lam, v, delta, gap, r_ref): the eigenpair of largest |lambda| of M (v of unit length), the distance from lam to the
    nearest other eigenvalue returned, the relative gap (|l1| - |l2|) / |l1|, and the specification's own residual
    |M v - lam v|_2 (np.longdouble up to n = 4100, float64 above)."""
    n = len(diag)
    if M is None:
        M = dense(diag, off)
    if n <= EIGH_MAX:
        w, V = np.linalg.eigh(M)
    else:
        from scipy.sparse.linalg import eigsh
        w, V = eigsh(M, k=4, which="LM", tol=1e-14, ncv=96, v0=np.full(n, 1.0 / np.sqrt(n)))
    order = np.argsort(-np.abs(w), kind="stable")
    lam = float(w[order[0]])
    v = V[:, order[0]].copy()
    v /= np.linalg.norm(v)
    if len(w) == 1:
        delta, gap = np.inf, 1.0
    else:
        rest = np.delete(w, order[0])
        delta = float(np.abs(rest - lam).min())
        gap = float((abs(lam) - abs(w[order[1]])) / abs(lam))
    if n <= LONGDOUBLE_MAX:
        vl = v.astype(np.longdouble)
        r = M.astype(np.longdouble) @ vl - np.longdouble(lam) * vl
        r_ref = float(np.sqrt((r * r).sum()))
    else:
        r_ref = float(np.linalg.norm(M @ v - lam * v))
    return lam, v, delta, gap, r_ref


def raw_segment(v):
    a = np.abs(np.asarray(v, np.float64))
    return a / a.max()


def finish(v, mask, opts):
    """(segment float64, ransac_mask float32, original_mask float32): segment = |v| / max|v| zeroed below 1e-6;
    ransac_mask = mask * float32(aff_thresh), replaced by float32(segment) where segment > aff_thresh."""
    seg = raw_segment(v)
    seg[seg < 1e-6] = 0.0
    original = np.asarray(mask, np.float32).copy()
    ransac = original * np.float32(opts.aff_thresh)
    sel = seg > opts.aff_thresh
    ransac[sel] = seg[sel].astype(np.float32)
    return seg, ransac, original


def tolerance(lam, v, delta, r_ref):
    """The bound on |segment_engine - segment_spec|, from the contract and the specification alone.

    The engine stops at |M v - lam v| <= TOL |lam|; by Davis-Kahan its unit vector is within sin(theta) <= TOL |lam| / delta
    of the true one, and the specification's own within r_ref / delta.  Two unit vectors at angle theta differ by at most
    2 sin(theta / 2) <= sqrt(2) sin(theta) in every entry; dividing by max|v| moves numerator and denominator by that much
    each, and segment <= 1, so the quotient moves by at most 2 sqrt(2) <= 4 times (sum of the two angles) / max|v| to first
    order.  The last term is the rounding of the abs, the maximum and the division themselves."""
    return 4.0 * (TOL * abs(lam) + r_ref) / (delta * float(np.abs(v).max())) + 4 * 2.3e-16


# ------------------------------------------------------------------ the iteration, emulated
def lanczos_cycles(diag, off, m=BASIS, M=None, trace=None):
    """(steps, cycles, how) of a float64 emulation of the engine's restarted Lanczos iteration: start from ones, classical
    Gram-Schmidt twice against the whole basis, at most ``m`` vectors per cycle, restart from the Ritz vector of largest
    |theta|, convergence tested at the first step after a (re)start, a cycle ended early when beta <= 1e-15 |T|.
    ``steps`` counts matrix-vector products, ``cycles`` tridiagonal solves; ``how`` is "converged", "breakdown" (converged,
    and some cycle ended early) or "cap".  ``trace`` (a list) receives the relative residual of every convergence test."""
    n = len(diag)
    if M is None:
        M = dense(diag, off)
    m = min(m, n)
    w = np.ones(n)
    steps = cycles = 0
    broke = False
    for _ in range(MAX_CYCLES):
        V = np.zeros((n, m))
        alpha, beta = np.zeros(m), np.zeros(m + 1)
        m_eff = m
        for j in range(m):
            b = np.sqrt(w @ w)
            if j >= 1:
                tnorm = max(abs(alpha[k]) + (beta[k] if k else 0.0) for k in range(j))
                beta[j] = b
                if j == 1 and trace is not None:
                    trace.append(b / abs(alpha[0]))
                if j == 1 and b <= TOL * abs(alpha[0]):
                    return steps, cycles, "breakdown" if broke else "converged"
                if b <= BREAKDOWN * tnorm:
                    m_eff, broke = j, True
                    break
            x = w / b
            V[:, j] = x
            y = M @ x
            h = V[:, :j + 1].T @ y
            y = y - V[:, :j + 1] @ h
            h2 = V[:, :j + 1].T @ y
            w = y - V[:, :j + 1] @ h2
            alpha[j] = h[j] + h2[j]
            steps += 1
        T = np.diag(alpha[:m_eff]) + np.diag(beta[1:m_eff], 1) + np.diag(beta[1:m_eff], -1)
        th, S = np.linalg.eigh(T)
        k = int(np.argmax(np.abs(th)))
        cycles += 1
        if m_eff == 1 and trace is not None:
            trace.append(np.sqrt(w @ w) / abs(alpha[0]))
        if m_eff == 1 and np.sqrt(w @ w) <= TOL * abs(alpha[0]):
            return steps, cycles, "breakdown" if broke else "converged"
        w = V[:, :m_eff] @ S[:, k]
    return steps, cycles, "cap"


# ------------------------------------------------------------------ seeded inputs
def fundamental(Rc, Ro, tc, to, K):
    """utils.py:171-178 (the skew-symmetric matrix float32, as there)."""
    Ro_inv = np.linalg.inv(Ro)
    Rr = Ro_inv @ Rc
    x, y, z = Ro_inv @ (tc - to)
    ss_t = np.float32([[0, -z, y], [z, 0, -x], [-y, x, 0]])
    K_inv = np.linalg.inv(K)
    return K_inv.T @ ss_t @ Rr @ K_inv


def camera_F(rng):
    from scipy.spatial.transform import Rotation as Rot
    K = np.float32([[1000, 0, 640], [0, 1000, 480], [0, 0, 1]])
    Rc = Rot.from_euler("xyz", rng.normal(0, 2, 3), degrees=True).as_matrix()
    Ro = Rot.from_euler("xyz", rng.normal(0, 2, 3), degrees=True).as_matrix()
    tc = np.float32(rng.normal(0, 1, 3))
    to = np.float32(rng.normal(0, 1, 3) + [3, 0, 0])
    return np.asarray(fundamental(Rc, Ro, tc, to, K), dtype=np.float64)


H_TRUE = np.array([[1.01, 0.02, 12.0], [-0.015, 0.99, -7.0], [2e-6, -1e-6, 1.0]])


def model_Hg():
    """The homography family's model: the other image's keypoint (dst) back onto the centre one (src), float32."""
    Hinv = np.linalg.inv(H_TRUE)
    return np.float32(Hinv / Hinv[2, 2])


def descriptors(rng, n, out):
    """Small integers as float32: the other image's descriptor a perturbed copy, unrelated for the outliers."""
    c = rng.integers(0, 120, (n, DIM))
    o = np.clip(c + rng.integers(-25, 25, (n, DIM)), 0, 255)
    o[out] = rng.integers(0, 120, (int(out.sum()), DIM))
    return c.astype(np.float32), o.astype(np.float32)


def group_sizes(n, g):
    """g sizes that sum to n, each one more than the one before, the last taking the remainder."""
    q = (n - g * (g - 1) // 2) // g
    sizes = [q + k for k in range(g)]
    sizes[-1] += n - sum(sizes)
    return sizes


def make_inputs(family, n, rng, groups=0):
    """(src, dst, c, o) float32 of one family (module docstring of tests/golden/make_golden_spectral.py for the first
    three; `scale` and `groups` are this file's)."""
    out = np.zeros(n, bool)
    if family == "groups":
        sizes = group_sizes(n, groups)
        centre = rng.uniform(0, 1000, (groups, 2))
        motion = rng.uniform(-60, 60, (groups, 2))
        feats = rng.integers(1, 120, (groups, DIM))
        of = np.repeat(np.arange(groups), sizes)
        src, dst = centre[of], (centre + motion)[of]
        c = o = feats[of].astype(np.float32)
        return src.astype(np.float32), dst.astype(np.float32), c, o.copy()
    if family == "disjoint":        # spacing 10 px, dst = 3 src: |s - d| >= 800 for every pair, so M is diagonal
        side = int(np.ceil(np.sqrt(n)))
        g = np.stack(np.meshgrid(np.arange(side), np.arange(side)), -1).reshape(-1, 2)[:n] * 10.0 + 5
        src = g + rng.uniform(-1, 1, (n, 2))
        dst = 3 * src
    elif family == "scale":
        src = rng.uniform(0, 1000, (n, 2))
        dst = 1.03 * src + rng.normal(0, 0.3, (n, 2))
    else:
        src = rng.uniform(0, 1000, (n, 2))
        if family == "homography":
            q = np.c_[src, np.ones(n)] @ H_TRUE.T
            dst = q[:, :2] / q[:, 2:]
        else:
            assert family == "translation", family
            dst = src + [35.0, -18.0]
        dst = dst + rng.normal(0, 0.5, (n, 2))
        out = rng.random(n) < 0.2
        dst[out] = rng.uniform(0, 1000, (int(out.sum()), 2))
    c, o = descriptors(rng, n, out)
    return src.astype(np.float32), dst.astype(np.float32), c, o


def zero_denominator_point(Hg):
    """A float32 (u, 0) whose third homogeneous coordinate (Hg[2,0] u + Hg[2,1] 0) + Hg[2,2] is exactly 0 in float32."""
    h6, h8 = Hg[2, 0], Hg[2, 2]
    u = np.float32(-h8 / h6)
    for _ in range(64):
        for cand in (u, np.nextafter(u, np.float32(np.inf)), np.nextafter(u, np.float32(-np.inf))):
            if (h6 * cand + Hg[2, 1] * np.float32(0)) + h8 == 0:
                return cand
        u = np.nextafter(np.nextafter(u, np.float32(np.inf)), np.float32(np.inf))
    raise AssertionError("no float32 u with a zero denominator")


class Case:
    """One input of the edge tests.  ``expect``: "one" (a single cycle), "several" (>= 2 cycles), "breakdown", "step1",
    or None (no condition on the iteration)."""

    def __init__(self, name, family, n, opts=None, groups=0, use_hg=False, zero_k2=False, expect=None, seed=0):
        self.name, self.family, self.n, self.opts = name, family, n, opts or Opts()
        self.groups, self.use_hg, self.zero_k2, self.expect, self.seed0 = groups, use_hg, zero_k2, expect, seed

    def __repr__(self):
        return self.name


TRANSLATION_N = (3, 63, 64, 65, 255, 256, 257, 513, 2048, 2049, 4096, 4097, 8192, 8193)
OPTION_SETS = [("affinity_eps", 5.0), ("affinity_eps", 22.5), ("affinity_eps", 100.0), ("aff_thresh", 0.3), ("aff_thresh", 0.8),
               ("epi_weight", 0.0), ("epi_weight", 0.75)]


# Where the seed search of these cases starts instead: the first seed at which a search from the default start ended when the
# cases were written (about one `scale` seed in six needs a second cycle).  build() checks every condition all the same.
SEED_START = {"scale_2049": 4547, "scale_4097": 4573, "scale_8193": 4611, "disjoint_1000": 4669}


def cases():
    """Every case, in a fixed order; the seed search of ``build`` starts at 4000 + 37 x its position, or at SEED_START."""
    out = [Case(f"translation_{n}", "translation", n, expect="one" if n >= 63 else None) for n in TRANSLATION_N]
    out += [Case(f"scale_{n}", "scale", n, expect="several") for n in (2049, 4097, 8193)]
    out += [Case(f"disjoint_{n}", "disjoint", n, expect="several") for n in (300, 1000)]
    out += [Case(f"groups_{n}_{g}", "groups", n, Opts(epi_weight=0.0), groups=g, expect="step1" if g == 1 else "breakdown")
            for n, g in ((300, 1), (300, 2), (301, 3), (257, 5))]
    out += [Case(f"opt_{key}_{value:g}", "translation", 257, Opts(**{key: value})) for key, value in OPTION_SETS]
    out += [Case("hg_257", "homography", 257, use_hg=True), Case("hg_2049", "homography", 2049, use_hg=True),
            Case("hg_65_zero_k2", "homography", 65, use_hg=True, zero_k2=True)]
    for k, c in enumerate(out):
        c.seed0 = SEED_START.get(c.name, 4000 + 37 * k)
    return out


class Built:
    """A case's inputs, the specification's answer, and what ``conditions`` measured."""


def conditions(case, b):
    """The reasons (empty when none) why the built case ``b`` may not be used: the requirements of the edge tests."""
    why = []
    if len(b.diag) > 1 and not b.gap >= 1e-3:
        why.append(f"relative gap {b.gap:.3g} < 1e-3")
    if not b.tol <= 1e-7:
        why.append(f"tolerance {b.tol:.3g} > 1e-7")
    raw = raw_segment(b.v)
    near = min(np.abs(raw - case.opts.aff_thresh).min(), np.abs(raw - 1e-6).min())
    if not near > 10 * b.tol:
        why.append(f"a segment value {near:.3g} from a threshold (10 tol = {10 * b.tol:.3g})")
    steps, cycles, how = b.emulated
    if case.expect == "one" and not (cycles == 1 and how == "converged"):
        why.append(f"emulation: {b.emulated}, wanted one cycle")
    if case.expect == "several" and not (cycles >= 2 and how != "cap"):
        why.append(f"emulation: {b.emulated}, wanted >= 2 cycles")
    elif case.expect == "several" and not b.residuals[1] >= SEVERAL_MARGIN * TOL:
        # the engine's sums have another order: a first cycle that misses TOL by a hair here may meet it there
        why.append(f"emulation: residual {b.residuals[1]:.3g} after the first cycle, within {SEVERAL_MARGIN:g} x of 1e-13")
    if case.expect == "breakdown" and how != "breakdown":
        why.append(f"emulation: {b.emulated}, wanted a breakdown")
    if case.expect == "step1" and not (steps == 1 and how == "converged"):
        why.append(f"emulation: {b.emulated}, wanted convergence at step 1")
    return why


def build_seed(case, seed, keep_matrix=False):
    rng = np.random.default_rng(seed)
    b = Built()
    b.case, b.seed, b.opts = case, seed, case.opts
    b.src, b.dst, b.c, b.o = make_inputs(case.family, case.n, rng, case.groups)
    b.F = camera_F(rng)
    b.mask = (rng.random(case.n) < 0.5).astype(np.float32)
    b.Hg = model_Hg() if case.use_hg else None
    if case.zero_k2:
        b.dst[case.n // 2] = (zero_denominator_point(b.Hg), 0.0)
    b.ms = match_score(b.c, b.o)
    b.diag = diagonal(b.src, b.dst, b.ms, b.F, case.opts.epi_weight)
    off = off_diagonal_f32(b.src, b.dst, case.opts.affinity_eps)
    M = dense(b.diag, off)
    b.off = off if keep_matrix else None
    del off
    b.lam, b.v, b.delta, b.gap, b.r_ref = principal(b.diag, None, M=M)
    b.tol = tolerance(b.lam, b.v, b.delta, b.r_ref)
    b.residuals = []
    b.emulated = lanczos_cycles(b.diag, None, M=M, trace=b.residuals)
    del M
    b.initial = initial_mask(b.src, b.dst, b.ms, b.Hg, case.opts) if case.use_hg else b.mask.copy()
    b.segment, b.ransac_mask, b.original_mask = finish(b.v, b.initial, case.opts)
    return b


def build(case, keep_matrix=False):
    """The first of MAX_SEEDS seeds from the case's own whose build meets every condition; None (with the reasons printed)
    when none does.  The search is deterministic, so every caller gets the same inputs; the seed kept is ``.seed``."""
    for seed in range(case.seed0, case.seed0 + MAX_SEEDS):
        b = build_seed(case, seed, keep_matrix)
        why = conditions(case, b)
        if not why:
            return b
        print(f"  {case.name} seed {seed}: {'; '.join(why)}; next seed")
    return None
