"""Brute-force specification of descriptor matching in numpy (test infrastructure; the product never imports it).

* Integer-valued descriptors: d2 in int64 - exact - a stable arg-sort for the nearest and the runner-up (ties to the lowest
  index), and ``np.sqrt(np.float32(d2))``, numpy's correctly rounded float32 square root.
* Float descriptors: d2 in float64 from the float32 inputs, against which the float32 kernel is held to a derived bound;
  and ``match_f32``, the kernel's own float32 sum restated step by step (``fmaf`` rounds once), which pins its bytes.
"""
import numpy as np

DIM = 128
U = 2.0 ** -24                     # unit roundoff of float32
# relative error bound of the float32 d2 in the difference form: two roundings from the squared difference, one from the
# product, at most 128 from the sum; every term is >= 0, so it holds in any summation order
GAMMA = 132 * U / (1 - 132 * U)
EPS = (1 + GAMMA) / (1 - GAMMA) - 1   # so d64(chosen) <= (1 + EPS) min d64: ~1.574e-5


def d2_int(q, t):
    """Exact squared distances (nq, nt) int64 of integer-valued descriptors (any dtype): the sum of squared differences,
    expanded.  Every quantity below is an integer under 2^53, so the float64 products and sums (BLAS) are exact."""
    q64, t64 = np.asarray(q, dtype=np.float64), np.asarray(t, dtype=np.float64)
    assert np.array_equal(q64, np.rint(q64)) and np.array_equal(t64, np.rint(t64)) and np.abs(q64).max(initial=0) < 2 ** 20 \
        and np.abs(t64).max(initial=0) < 2 ** 20
    d = q64 @ t64.T
    d *= -2.0
    d += (q64 * q64).sum(1)[:, None]
    d += (t64 * t64).sum(1)[None, :]
    return d.astype(np.int64)


def d2_f64(q, t, block=64):
    """Squared distances (nq, nt) in float64, difference form, of float32 descriptors."""
    q64, t64 = np.asarray(q, dtype=np.float64), np.asarray(t, dtype=np.float64)
    out = np.empty((len(q64), len(t64)))
    for a in range(0, len(q64), block):
        diff = q64[a:a + block, None, :] - t64[None, :, :]
        out[a:a + block] = np.einsum("ijk,ijk->ij", diff, diff)
    return out


def two_smallest(d):
    """(idx, idx2) int32 of the smallest and second-smallest entry of every row of ``d``, ties to the lowest index; idx2 = -1
    with a single column: the first two columns of a stable arg-sort.  Rows of more than 4096 entries take the first minimum,
    strike it out and take the first minimum again - the same two indices at a fraction of the sorting time
    (test_match_host.py holds the two against each other)."""
    if d.shape[1] <= 4096:
        order = np.argsort(d, axis=1, kind="stable")
        idx = order[:, 0].astype(np.int32)
        idx2 = order[:, 1].astype(np.int32) if d.shape[1] > 1 else np.full(len(d), -1, np.int32)
        return idx, idx2
    return two_smallest_by_argmin(d)


def two_smallest_by_argmin(d):
    rows = np.arange(len(d))
    idx = np.argmin(d, axis=1)
    if d.shape[1] == 1:
        return idx.astype(np.int32), np.full(len(d), -1, np.int32)
    rest = d.copy()
    rest[rows, idx] = np.iinfo(np.int64).max if d.dtype.kind == "i" else np.inf
    return idx.astype(np.int32), np.argmin(rest, axis=1).astype(np.int32)


def match_int(q, t):
    """(idx, dist, idx2, dist2) of integer-valued descriptors: int32 indices, float32 distances (+inf where the index is -1)."""
    out = []
    for a in range(0, len(q), 1024):    # in blocks of queries: (block, nt) int64 at a time
        d = d2_int(q[a:a + 1024], t)
        idx, idx2 = two_smallest(d)
        rows = np.arange(len(d))
        dist = np.sqrt(np.float32(d[rows, idx]))
        dist2 = np.where(idx2 >= 0, np.sqrt(np.float32(d[rows, np.maximum(idx2, 0)])), np.float32(np.inf)).astype(np.float32)
        out.append((idx, dist, idx2, dist2))
    return tuple(np.concatenate(x) for x in zip(*out))


def fmaf(a, b, c):
    """float32(a * b + c) with one rounding, of float32 arrays: C's fmaf, restated in float64.

    The product of two float32 is exact in float64 (48 bits).  The float64 sum p + c is not: s = fl(p + c) and its error e
    (Knuth's TwoSum, exact) are.  Where e != 0 the true sum lies strictly between s and its neighbour on e's side, and the one
    of the two whose last mantissa bit is odd is the sum rounded to odd; rounding that to float32 is rounding the true sum
    (53 >= 24 + 2 bits: Boldo and Melquiond, "Emulation of a FMA and correctly rounded sums", 2008).  A plain float64 add
    fails where p + c lies just off the middle of two float32: it rounds onto the middle, and the cast then goes to even."""
    a, b, c = (np.asarray(x, dtype=np.float32).astype(np.float64) for x in (a, b, c))
    with np.errstate(invalid="ignore", over="ignore"):
        p = a * b
        s = p + c
        bb = s - p
        e = (p - (s - bb)) + (c - bb)
        inexact = np.isfinite(s) & (e != 0)      # e is NaN where s is not finite
        even = (s.view(np.int64) & 1) == 0
        odd = np.where(inexact & even, np.nextafter(s, np.where(e > 0, np.inf, -np.inf)), s)
        return odd.astype(np.float32)


def d2_f32(q, t):
    """The matcher's squared distances (nq, nt) of float32 descriptors, bit for bit: float32 from acc = 0, then for k
    ascending d = q[i, k] - t[j, k] and acc = fmaf(d, d, acc)."""
    q, t = np.asarray(q, dtype=np.float32), np.asarray(t, dtype=np.float32)
    acc = np.zeros((len(q), len(t)), np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(DIM):
            d = q[:, None, k] - t[None, :, k]
            acc = fmaf(d, d, acc)
    return acc


def match_f32(q, t):
    """(idx, dist, idx2, dist2) of float32 descriptors as the matcher defines them: d2_f32, the candidates - the finite d2 -
    in the order (d2, train index), and float32(sqrt(float64(d2))), the correctly rounded float32 root; -1 and +inf where
    there is no candidate."""
    d = d2_f32(q, t)
    d[~np.isfinite(d)] = np.inf
    rows = np.arange(len(d))
    order = np.argsort(d, axis=1, kind="stable")      # stable: equal d2 stay in the order of the index
    out = []
    for col in (0, 1):
        if col < d.shape[1]:
            i = order[:, col]
            v = d[rows, i]
            out += [np.where(np.isinf(v), -1, i).astype(np.int32), np.sqrt(v.astype(np.float64)).astype(np.float32)]
        else:
            out += [np.full(len(d), -1, np.int32), np.full(len(d), np.inf, np.float32)]
    return tuple(out)


def filters(idx, dist, dist2, back_idx, ratio=None, cross_check=False):
    """The queries that ``matching.match`` keeps, from the specification's arrays (``back_idx``: the nearest query of every
    train row)."""
    keep = idx >= 0
    if ratio is not None:
        keep = keep & (dist < np.float32(ratio) * dist2)
    if cross_check:
        keep = keep & (back_idx[idx] == np.arange(len(idx)))
    return np.flatnonzero(keep)
