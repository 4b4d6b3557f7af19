"""The panorama's exposure gain compensation in numpy and plain Python (DESIGN.md "Panorama, gain compensation"): exact.

Like ``panorama_ramp_spec`` it starts from the target coordinates of every pair canvas - the oracle's ``warp_coords_fast`` or
the engine's ``_native.warp_coords`` - and derives every sample from them.  View 0 is the centre, view k layer k - 1.

1. statistics   over the canvas pixels with ``X % step == 0 and Y % step == 0``: ``N[a][b]`` the number at which a and b are
                both present, ``S[a][b]`` the sum of ``I_a = r + g + b`` of a's sample over them (uint64).
2. gains        Brown & Lowe (IJCV 2007, section 6): the normal equations of
                ``1/2 sum_{a != b} N_ab [(g_a m_ab - g_b m_ba)^2 / sigma_n^2 + (1 - g_a)^2 / sigma_g^2]``, ``m_ab = S_ab / (3 N_ab)``,
                solved by Cholesky in ONE written-out order of ``+ - * / sqrt`` on Python floats (IEEE float64, nothing
                fused); ``q = clamp(rint(4096 g), 1024, 16383)``.
3. application  a channel ``c`` of a sample of view v becomes ``min(255, (c q_v + 2048) >> 12)``; presence, the ramp's
                weight and paste's first present layer are decided on the ungained sample.
"""
import math

import numpy as np

import panorama_ramp_spec as R
import warp_bilinear_spec as B
from panorama_spec import panorama_size

MIN_Q, MAX_Q, UNIT = 1024, 16383, 4096
MAX_STEP = 64


def samples(center, layers, geometries, coords, sampling="nearest"):
    """The K + 1 views on the union canvas: ``values`` (K + 1, H, W, 3) uint8, black where a view has no sample, and ``weight_of``
    (ramp) -> (K + 1, H, W) int64, the ramp weights of the samples' source pixels (any value where the sample is black)."""
    W, H, OX, OY = panorama_size(center.shape, geometries)
    values = np.zeros((len(layers) + 1, H, W, 3), np.uint8)
    src = []                        # per view: (rows, cols, picture shape, ix, iy) of its rectangle
    ch, cw = center.shape[:2]
    values[0, OY:OY + ch, OX:OX + cw] = center
    yy, xx = np.meshgrid(np.arange(ch), np.arange(cw), indexing="ij")
    src.append((slice(OY, OY + ch), slice(OX, OX + cw), (ch, cw), xx, yy))
    for k, (layer, (fw, fh, ox, oy), (tx, ty)) in enumerate(zip(layers, geometries, coords)):
        img = np.asarray(layer.img)
        assert tx.shape == ty.shape == (fh, fw)
        inside, ix, iy = R.gathered(img, tx, ty)
        rows, cols = slice(OY - oy, OY - oy + fh), slice(OX - ox, OX - ox + fw)
        if sampling == "bilinear":
            values[k + 1, rows, cols] = B.sample(img, tx, ty)
        else:
            assert sampling == "nearest"
            values[k + 1, rows, cols] = np.where(inside[..., None], img[iy, ix], 0)
        src.append((rows, cols, img.shape[:2], ix, iy))

    def weight_of(ramp):
        w = np.zeros(values.shape[:3], np.int64)
        for v, (rows, cols, (h, wd), ix, iy) in enumerate(src):
            w[v, rows, cols] = R.weight_map(h, wd, ramp)[iy, ix]
        return w

    return values, weight_of


def stats(values, step):
    """Step 1 on the views of ``samples``: (N, S), (K + 1, K + 1) uint64."""
    assert isinstance(step, (int, np.integer)) and 1 <= step <= MAX_STEP
    lattice = values[:, ::step, ::step]
    present = lattice.any(axis=-1)
    inten = lattice.astype(np.int64).sum(axis=-1)
    V = len(values)
    N, S = np.zeros((V, V), np.uint64), np.zeros((V, V), np.uint64)
    for a in range(V):
        for b in range(V):
            both = present[a] & present[b]
            N[a, b] = int(both.sum())
            S[a, b] = int(inten[a][both].sum())
    return N, S


def solve(N, S, sigma_n=10.0, sigma_g=0.1):
    """Step 2: (g, q, flag); g a list of Python floats, q a list of ints."""
    n = len(N)
    N = [[int(N[a][b]) for b in range(n)] for a in range(n)]
    S = [[int(S[a][b]) for b in range(n)] for a in range(n)]
    inv_n2, inv_g2 = 1.0 / (sigma_n * sigma_n), 1.0 / (sigma_g * sigma_g)
    L = [[0.0] * n for _ in range(n)]
    g = [0.0] * n
    for c in range(n):
        acc, rhs = 0.0, 0.0
        for b in range(n):
            if b == c or N[c][b] == 0:
                continue
            nf = float(N[c][b])
            d3 = 3.0 * nf
            mcb, mbc = float(S[c][b]) / d3, float(S[b][c]) / d3
            acc = acc + nf * ((2.0 * (mcb * mcb)) * inv_n2 + inv_g2)
            rhs = rhs + nf * inv_g2
            L[c][b] = -((((2.0 * nf) * mcb) * mbc) * inv_n2)
        L[c][c], g[c] = (acc, rhs) if acc > 0.0 else (1.0, 1.0)
    bad = False
    for j in range(n):
        for k in range(j):
            s = L[j][k]
            for p in range(k):
                s = s - L[j][p] * L[k][p]
            L[j][k] = s / L[k][k]
        d = L[j][j]
        for p in range(j):
            d = d - L[j][p] * L[j][p]
        if not (d > 0.0) or math.isinf(d):
            bad = True
            break
        L[j][j] = math.sqrt(d)
    if not bad:
        for j in range(n):
            s = g[j]
            for p in range(j):
                s = s - L[j][p] * g[p]
            g[j] = s / L[j][j]
        for j in range(n - 1, -1, -1):
            s = g[j]
            for p in range(j + 1, n):
                s = s - L[p][j] * g[p]
            g[j] = s / L[j][j]
        bad = not all(math.isfinite(v) for v in g)
    if bad:
        g = [1.0] * n
    return g, [quantise(v) for v in g], int(bad)


def quantise(g):
    return int(min(max(round(4096.0 * g), MIN_Q), MAX_Q))     # round(): half to even


def normal_equations(N, S, sigma_n=10.0, sigma_g=0.1):
    """The system of step 2 in exact fractions: (A, rhs) as lists of ``fractions.Fraction``."""
    from fractions import Fraction as F
    n = len(N)
    sn2, sg2 = F(sigma_n) ** 2, F(sigma_g) ** 2
    A = [[F(0)] * n for _ in range(n)]
    rhs = [F(0)] * n
    for c in range(n):
        for b in range(n):
            if b == c or int(N[c][b]) == 0:
                continue
            nn = F(int(N[c][b]))
            mcb, mbc = F(int(S[c][b])) / (3 * nn), F(int(S[b][c])) / (3 * nn)
            A[c][c] += nn * (2 * mcb * mcb / sn2 + 1 / sg2)
            A[c][b] = -2 * nn * mcb * mbc / sn2
            rhs[c] += nn / sg2
        if A[c][c] == 0:
            A[c][c], rhs[c] = F(1), F(1)
    return A, rhs


def apply(values, q):
    """Step 3 on uint8 values of one view."""
    assert MIN_Q <= q <= MAX_Q
    return np.minimum((values.astype(np.int64) * q + 2048) >> 12, 255).astype(np.uint8)


def compose(values, weight_of, center_rect, q, blend, ramp=1):
    """The canvas of ``blend`` ('mean', 'paste', 'ramp') under the gains ``q`` (K + 1 ints) from the views of ``samples``;
    ``center_rect`` = (OX, OY, cw, ch)."""
    present = values.any(axis=-1)
    gained = np.stack([apply(v, int(qv)) for v, qv in zip(values, q)])
    if blend == "paste":
        out = np.zeros(values.shape[1:], np.uint8)
        open_ = np.ones(values.shape[1:3], bool)
        for v in range(1, len(values)):
            take = open_ & present[v]
            out[take] = gained[v][take]
            open_ &= ~take
        OX, OY, cw, ch = center_rect
        out[OY:OY + ch, OX:OX + cw] = gained[0, OY:OY + ch, OX:OX + cw]
        return out
    wt = present.astype(np.int64) if blend == "mean" else np.where(present, weight_of(ramp), 0)
    assert blend in ("mean", "ramp")
    total = (wt[..., None] * gained.astype(np.int64)).sum(axis=0)
    return (total // np.maximum(wt.sum(axis=0), 1)[..., None]).astype(np.uint8)
