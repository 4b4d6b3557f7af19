#!/usr/bin/env python3
"""Generate the spectral-weighting fixtures tests/golden/spectral_*.npz FROM THE REFERENCE ITSELF.

Run in the build container only (the reference's ``pyviz`` must be mounted where REF points):

    python tests/golden/make_golden_spectral.py

It imports the reference's ``spectral_method.py`` (and through it ``utils.py``) in place - nothing is copied - and calls
its real ``calculate_M`` on seeded synthetic matches (the dataset is not distributed).  Stored per case: the inputs
(points float32, descriptors as the small integers they are made of - for the largest case as indices into a 512-row
codebook, which keeps the file small - F, Hg or the RANSAC mask), the reference's
``segment``, ``ransac_mask``, ``original_mask``, the eigenvalue of largest |lambda| and the relative gap from
``np.linalg.eigvalsh`` of the reference's own M, and for n <= 500 that M (diagonal float64, off-diagonal float32).

Stubs, in memory only, for what the import needs and this image lacks or the path does not use:
* ``cv2``: ``DMatch`` / ``KeyPoint`` (annotations), ``RANSAC``, and ``findHomography`` returning the mask the case stores
  (the test hands that mask in through ``mask=``);
* ``matplotlib.pyplot``, ``cvxpy``, ``configargparse`` (model.py / options.py import them), ``pandas`` (utils.py).

Each case is checked before it is written, so that the GPU test can demand exact mask equality:
* relative gap (|l1| - |l2|) / |l1| >= 1e-3;
* no segment value within 1e-7 of aff_thresh or of 1e-6;
* with Hg: every match's float32 distance at least 1e-3 px from em_radius and its score 1e-5 from score_thresh
  (the reference's 1-D norms there go through BLAS).
A seed that fails is replaced by the next one.
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference/pyviz"
sys.dont_write_bytecode = True

_RANSAC_MASK = {}


def import_reference():
    cv2 = types.ModuleType("cv2")
    cv2.DMatch = type("DMatch", (), {})
    cv2.KeyPoint = type("KeyPoint", (), {})
    cv2.RANSAC = 8

    def findHomography(src, dst, method, thresh):
        return np.eye(3), _RANSAC_MASK["mask"].reshape(-1, 1).astype(np.uint8)

    cv2.findHomography = findHomography
    sys.modules["cv2"] = cv2
    for name in ("matplotlib", "matplotlib.pyplot", "cvxpy", "configargparse", "pandas"):
        sys.modules[name] = types.ModuleType(name)
    sys.modules["matplotlib"].pyplot = sys.modules["matplotlib.pyplot"]
    sys.path.insert(0, REF)
    cwd = os.getcwd()
    os.chdir(REF)
    try:
        import spectral_method as ref      # noqa: E402
        import utils as ref_utils          # noqa: E402
    finally:
        os.chdir(cwd)
    return ref, ref_utils


class KP:
    def __init__(self, x, y):
        self.pt = (float(x), float(y))


class DM:
    def __init__(self, q, t):
        self.queryIdx, self.trainIdx = q, t


class Opts:
    epi_weight, affinity_eps, aff_thresh, em_radius, score_thresh = 0.5, 30.0, 0.5, 6.0, 0.4


def camera_F(ref_utils, rng):
    K = np.float32([[1000, 0, 640], [0, 1000, 480], [0, 0, 1]])
    from scipy.spatial.transform import Rotation as Rot
    Rc = Rot.from_euler("xyz", rng.normal(0, 2, 3), degrees=True).as_matrix()
    Ro = Rot.from_euler("xyz", rng.normal(0, 2, 3), degrees=True).as_matrix()
    tc = np.float32(rng.normal(0, 1, 3))
    to = np.float32(rng.normal(0, 1, 3) + [3, 0, 0])
    return np.asarray(ref_utils.fundamental(Rc, Ro, tc, to, K), dtype=np.float64)


def make_case(kind, n, rng, book=False):
    """(src, dst, c int, o int, inlier mask, Hg float32 or None, codebook or None).  With ``book`` the descriptors are rows
    of a 512-row codebook (256 rows and a perturbed copy of each): a large case then stores indices, not n x 256 values."""
    out = np.zeros(n, bool)
    if kind in ("disjoint", "negative"):   # no consistent pair: spacing 10 px, dst = 3 src -> |s - d| >= 800 for every pair
        side = int(np.ceil(np.sqrt(n)))
        g = np.stack(np.meshgrid(np.arange(side), np.arange(side)), -1).reshape(-1, 2)[:n] * 10.0 + 5
        src = g + rng.uniform(-1, 1, (n, 2))
        dst = 3 * src
    else:
        src = rng.uniform(0, 1000, (n, 2))
        if kind == "clusters":      # two compact groups, different motions: no consistency across, distinct Perron roots
            k = int(n * 0.6)
            src[:k] = rng.uniform(100, 130, (k, 2))
            src[k:] = rng.uniform(600, 640, (n - k, 2))
            dst = src.copy()
            dst[:k] += [40, -25]
            dst[k:] += [-20, 60]
        elif kind == "homography":
            H = np.array([[1.01, 0.02, 12.0], [-0.015, 0.99, -7.0], [2e-6, -1e-6, 1.0]])
            q = np.c_[src, np.ones(n)] @ H.T
            dst = q[:, :2] / q[:, 2:]
        else:                       # translation
            dst = src + [35.0, -18.0]
        dst = dst + rng.normal(0, 0.5, (n, 2))
        out = rng.random(n) < 0.2
        dst[out] = rng.uniform(0, 1000, (out.sum(), 2))
    codes = None
    if book:
        base = rng.integers(0, 120, (256, 128))
        codes = np.concatenate([base, np.clip(base + rng.integers(-25, 25, (256, 128)), 0, 255)])
        ci = rng.integers(0, 256, n)
        oi = ci + 256
        oi[out] = rng.integers(0, 256, out.sum())
        c, o = codes[ci], codes[oi]
        codes = (codes.astype(np.int16), ci.astype(np.int16), oi.astype(np.int16))
    elif kind == "negative":
        c = rng.integers(-60, 60, (n, 128))
        o = -c + rng.integers(-8, 8, (n, 128))
    else:
        c = rng.integers(0, 120, (n, 128))
        o = np.clip(c + rng.integers(-25, 25, (n, 128)), 0, 255)
        o[out] = rng.integers(0, 120, (out.sum(), 128))
    Hg = None
    if kind == "homography":
        # the model maps the OTHER image's keypoint (dst) back onto the centre one (src), as recompute_matching uses it
        Hinv = np.linalg.inv(np.array([[1.01, 0.02, 12.0], [-0.015, 0.99, -7.0], [2e-6, -1e-6, 1.0]]))
        Hg = np.float32(Hinv / Hinv[2, 2])
    return src.astype(np.float32), dst.astype(np.float32), c, o, ~out, Hg, codes


CASES = [  # name, kind, n, use Hg, store M, codebook descriptors
    ("n1", "translation", 1, False, True, False),
    ("n2", "translation", 2, False, True, False),
    ("n7", "translation", 7, False, True, False),
    ("n64_hg", "homography", 64, True, True, False),
    ("n500", "translation", 500, False, True, False),
    ("n500_hg", "homography", 500, True, True, False),
    ("clusters", "clusters", 300, False, True, False),
    ("disjoint", "disjoint", 40, False, True, False),
    ("negative", "negative", 48, False, True, False),
    ("n2000", "translation", 2000, False, False, False),
    ("n5000", "homography", 5000, True, False, True),
]


def run_case(ref, ref_utils, name, kind, n, use_hg, store_m, book, seed):
    rng = np.random.default_rng(seed)
    src, dst, ci, oi, inl, Hg, codes = make_case(kind, n, rng, book)
    F = camera_F(ref_utils, rng)
    mask = (inl ^ (rng.random(n) < 0.05)).astype(np.uint8)
    _RANSAC_MASK["mask"] = mask
    kc = [KP(*p) for p in src]
    ko = [KP(*p) for p in dst]
    matches = [DM(i, i) for i in range(n)]
    captured = {}
    svd = np.linalg.svd

    def spy(a, *args, **kw):
        captured["M"] = np.array(a, copy=True)
        return svd(a, *args, **kw)

    np.linalg.svd = spy
    try:
        feats_c = ci.astype(np.float32)
        feats_o = oi.astype(np.float32)
        segment, H, ransac_mask, original_mask = ref.calculate_M(kc, feats_c, ko, feats_o, F, matches, Opts(), Hg=Hg if use_hg else None)
    finally:
        np.linalg.svd = svd
    M = captured["M"]
    lam_all = np.linalg.eigvalsh(M)
    order = np.argsort(-np.abs(lam_all))
    lam = lam_all[order[0]]
    gap = 1.0 if n == 1 else (abs(lam) - abs(lam_all[order[1]])) / abs(lam)
    if gap < 1e-3:
        return None, f"gap {gap:.2e}"
    near = np.abs(segment - Opts.aff_thresh).min(), np.abs(segment[segment > 0] - 1e-6).min() if (segment > 0).any() else 1.0
    if min(near) < 1e-7:
        return None, f"segment within {min(near):.1e} of a threshold"
    if use_hg:
        q = (Hg @ np.c_[dst, np.ones(n, np.float32)].T).T
        dist = np.linalg.norm(q[:, :2] / q[:, 2:] - src, axis=1)
        cn = feats_c / np.linalg.norm(feats_c, axis=-1, keepdims=True)
        on = feats_o / np.linalg.norm(feats_o, axis=-1, keepdims=True)
        score = np.sum(cn * on, -1)
        if np.abs(dist - Opts.em_radius).min() < 1e-3 or np.abs(score - Opts.score_thresh).min() < 1e-5:
            return None, "a match on the edge of recompute_matching's thresholds"
    feats = dict(c_feats=ci.astype(np.int16), o_feats=oi.astype(np.int16)) if codes is None else \
        dict(codebook=codes[0], c_index=codes[1], o_index=codes[2])      # c_feats = codebook[c_index], o_feats = codebook[o_index]
    rec = dict(src=src, dst=dst, F=F, **feats,
               segment=segment, ransac_mask=ransac_mask, original_mask=original_mask, lam=lam, gap=gap, seed=seed,
               opts=np.array([Opts.epi_weight, Opts.affinity_eps, Opts.aff_thresh, Opts.em_radius, Opts.score_thresh]))
    if use_hg:
        rec["Hg"] = Hg
    else:
        rec["mask"] = mask.astype(np.float32)
    if store_m:
        off = M.copy()
        np.fill_diagonal(off, 0)
        assert np.array_equal(off.astype(np.float32).astype(np.float64), off)
        rec["M_diag"] = np.diag(M).copy()
        rec["M_off"] = off.astype(np.float32)
    return rec, f"lambda {lam:.6g} gap {gap:.3g} inliers {int((segment > Opts.aff_thresh).sum())}/{n}"


def main():
    ref, ref_utils = import_reference()
    want = set(sys.argv[1:])
    for k, (name, kind, n, use_hg, store_m, book) in enumerate(CASES):
        if want and name not in want:
            continue
        seed = 1000 + 17 * k
        while True:
            rec, msg = run_case(ref, ref_utils, name, kind, n, use_hg, store_m, book, seed)
            if rec is not None:
                break
            print(f"  {name} seed {seed}: {msg}; next seed")
            seed += 1
        np.savez_compressed(os.path.join(HERE, f"spectral_{name}.npz"), **rec)
        print(f"spectral_{name}: n={n} seed {seed} {msg}")


if __name__ == "__main__":
    main()
