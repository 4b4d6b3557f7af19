"""Spectral match weighting of the reference's ``pyviz/spectral_method.py`` (the script every shell driver of the reference
runs), the part that needs neither OpenCV nor cvxpy: ``calculate_M`` (:66-133) and its helpers, on the GPU.

* ``calculate_M``: same signature and return value as the reference's.  The dense N x N affinity and its full SVD are
  replaced by ``apap_spectral_weights``: a restarted Lanczos iteration in fp64 whose matrix-vector products recompute the
  float32 affinity tile by tile (no N x N buffer).  ``segment`` agrees with the reference's ``|U[:, 0]| / max`` to about
  N eps / gap; both masks are computed from it exactly as the reference does (include/apap_hip.h).
* ``spectral_weights``: the same on arrays (what ``cv_to_array`` returns), with the options as keywords.
* ``recompute_matching``, ``match_RANSAC``, ``cv_to_array``, ``normalized_feature``: the reference's helpers.
  ``match_RANSAC`` uses THIS REPOSITORY's GPU RANSAC (``_native.find_homography_ransac``), not OpenCV's: sampler, adaptive
  stopping and refinement differ, so its mask is not cv.findHomography's (as in ``baseline_stitch_test``).
* ``model_solve`` (:165-186): the M-step, model.py's LMSSolver / SDPSolver on the GPU (cvx_proj_amd/model.py);
  ``loss="huber"`` (with ``lms=True`` and a parameter > 1e-2) runs the Huber M-step, HuberSolver.
* ``spectral_em``: the EM loop of ``spectral_method()`` (:188-241) on arrays, every round on the device without a host
  synchronisation (``apap_spectral_em``): calculate_M with Hg = the previous round's H_pred, then model_solve.
* ``warp_results``: the two ``image_warping`` calls of the ``-s`` option (:227-229) as one batched kernel launch.
* ``skew_symmetric_transform``, ``fundamental``, ``get_fundamental``: utils.py:162-186, host numpy.
* ``estimate_fundamental``, ``estimate_fundamental_batch``, ``match_fundamental``: F from the matches themselves (GPU RANSAC,
  ``apap_find_fundamental_ransac``), for pairs that have no calibration spreadsheet.

Keypoints and matches are duck-typed: anything with ``.pt`` and ``.queryIdx`` / ``.trainIdx`` (OpenCV's KeyPoint / DMatch
or simple stand-ins).  ``opts`` is any object with ``epi_weight``, ``affinity_eps``, ``aff_thresh``, ``em_radius`` and
``score_thresh`` attributes.  No CPU fallback.
"""
from __future__ import annotations

import time
import warnings
from typing import NamedTuple

import numpy as np

from . import _native

__all__ = ["calculate_M", "spectral_weights", "SpectralResult", "recompute_matching", "match_RANSAC", "cv_to_array",
           "normalized_feature", "model_solve", "spectral_em", "spectral_em_batch", "spectral_em_grid", "EMRound", "EMResult", "warp_results", "skew_symmetric_transform", "fundamental",
           "get_fundamental", "estimate_fundamental", "estimate_fundamental_batch", "match_fundamental"]


class SpectralResult(NamedTuple):
    segment: np.ndarray         # (n,) float64: |v| / max|v|, entries below 1e-6 zeroed
    ransac_mask: np.ndarray     # (n,) float32: the initial mask x aff_thresh, segment where segment > aff_thresh
    original_mask: np.ndarray   # (n,) float32: the initial mask
    H: object                   # Hg, or the RANSAC homography (None when RANSAC found no model)
    lam: float                  # the eigenvalue of largest |lambda| (Rayleigh quotient of the returned vector)
    gap: float                  # relative gap (|l1| - |l2|) / |l1| of the last tridiagonal solve (NaN if none)
    steps: int                  # Lanczos steps (matrix-vector products)
    restarts: int
    residual: float             # last measured |M v - lambda v| / |lambda|
    converged: bool


def cv_to_array(source, target, matches, is_pts=True):
    """utils.py:133-140."""
    if is_pts:
        src = np.float32([source[m.queryIdx].pt for m in matches])
        dst = np.float32([target[m.trainIdx].pt for m in matches])
    else:
        src = np.stack([source[m.queryIdx] for m in matches], axis=0)
        dst = np.stack([target[m.trainIdx] for m in matches], axis=0)
    return src, dst


def normalized_feature(feats_cp, feats_op, match):
    """utils.py:153-160."""
    feat_c = feats_cp[match.queryIdx]
    feat_o = feats_op[match.trainIdx]
    return feat_c / np.linalg.norm(feat_c), feat_o / np.linalg.norm(feat_o)


def match_RANSAC(kpts_cp, kpts_op, matches, swap=False, device=-1, ctx=None):
    """spectral_method.py:25-33 with this repository's GPU RANSAC (5 px) in place of cv.findHomography: (H, mask float32)."""
    if swap:
        dst_pts, src_pts = cv_to_array(kpts_cp, kpts_op, matches)
    else:
        src_pts, dst_pts = cv_to_array(kpts_cp, kpts_op, matches)
    H, mask = _native.find_homography_ransac(src_pts, dst_pts, 5.0, device=device, ctx=ctx)
    return H, mask.astype(np.float32).ravel()


def _params(opts, max_restarts):
    return _native.spectral_params(opts.epi_weight, opts.affinity_eps, opts.aff_thresh, getattr(opts, "em_radius", 6.0),
                                   getattr(opts, "score_thresh", 0.4), 0 if max_restarts is None else max_restarts)


def _descriptors(feats_cp, feats_op, matches):
    # cv_to_array(..., is_pts=False): np.stack keeps the descriptors' dtype (float32 from SIFT)
    return cv_to_array(feats_cp, feats_op, matches, is_pts=False)


def recompute_matching(kpts_cp, feats_cp, kpts_op, feats_op, matches, H, opts, device=-1, ctx=None):
    """spectral_method.py:35-64 on the GPU (the set-up kernel of the spectral weights, in float32): 1.0 where the match's
    other-image keypoint, mapped through H, lies within ``opts.em_radius`` of its centre keypoint and the normalised
    descriptors' score exceeds ``opts.score_thresh``."""
    src, dst = cv_to_array(kpts_cp, kpts_op, matches)
    c, o = _descriptors(feats_cp, feats_op, matches)
    seg, rm, om, info = _native.spectral_weights(src, dst, c, o, np.eye(3), _params(opts, 1), Hg=H, device=device, ctx=ctx)
    return om


def _result(seg, rm, om, info, H):
    status = int(info[3])
    res = SpectralResult(seg, rm, om, H, float(info[0]), float(info[1]), int(info[2]), int(info[4]), float(info[5]),
                         not status & _native.STATUS_NO_CONVERGENCE)
    if not res.converged:
        warnings.warn(f"spectral weights: the eigen-solver did not reach |Mv - lambda v| <= 1e-13 |lambda| in {res.restarts} "
                      f"restarts (last residual {res.residual:.3e}, gap {res.gap:.3e}); the best Ritz vector is used",
                      RuntimeWarning, stacklevel=3)
    return res


def spectral_weights(src_pts, dst_pts, c_feats, o_feats, F, *, epi_weight=0.5, affinity_eps=30.0, aff_thresh=0.5, Hg=None,
                     mask=None, em_radius=6.0, score_thresh=0.4, swap=True, max_restarts=None, device=-1, ctx=None):
    """calculate_M on arrays.  src_pts / dst_pts (n, 2), c_feats / o_feats (n, 128) raw descriptors, F (3, 3).
    The initial mask: recompute_matching with ``Hg``; else ``mask`` (what match_RANSAC returned); else the GPU RANSAC of
    this repository (``swap`` as in match_RANSAC).  Returns a SpectralResult; warns (RuntimeWarning) when the solver hit
    its restart cap (``max_restarts``, default 30)."""
    src = np.ascontiguousarray(src_pts, dtype=np.float32)
    dst = np.ascontiguousarray(dst_pts, dtype=np.float32)
    params = _native.spectral_params(epi_weight, affinity_eps, aff_thresh, em_radius, score_thresh,
                                     0 if max_restarts is None else max_restarts)
    H = Hg
    if Hg is None and mask is None:
        if src.ndim != 2 or len(src) == 0:
            raise ValueError(f"no matches, or points not (n, 2): {src.shape}")
        a, b = (dst, src) if swap else (src, dst)
        H, m = _native.find_homography_ransac(a, b, 5.0, device=device, ctx=ctx)
        mask = m.astype(np.float32).ravel()
    seg, rm, om, info = _native.spectral_weights(src, dst, c_feats, o_feats, F, params, Hg=Hg, mask=mask, device=device, ctx=ctx)
    return _result(seg, rm, om, info, H)


def calculate_M(kpts_cp, feats_cp, kpts_op, feats_op, F, matches, opts, verbose=False, swap=True, init_ransac=True, Hg=None,
                device=-1, ctx=None):
    """spectral_method.py:66-133: ``(segment float64, H, ransac_mask float32, original_mask float32)``."""
    if not init_ransac:
        # the reference computes M and its SVD, then fails on `ransac_mask *= opts.aff_thresh` with ransac_mask = None
        raise TypeError("unsupported operand type(s) for *=: 'NoneType' and 'float'")
    if len(matches) == 0:
        raise ValueError("all the input array dimensions except for the concatenation axis must match exactly "
                         "(no matches: np.hstack at spectral_method.py:105)")
    src, dst = cv_to_array(kpts_cp, kpts_op, matches)
    c, o = _descriptors(feats_cp, feats_op, matches)
    mask = None
    H = Hg
    if Hg is None:
        H, mask = match_RANSAC(kpts_cp, kpts_op, matches, swap, device=device, ctx=ctx)
    res = spectral_weights(src, dst, c, o, F, epi_weight=opts.epi_weight, affinity_eps=opts.affinity_eps,
                           aff_thresh=opts.aff_thresh, Hg=Hg, mask=mask, em_radius=getattr(opts, "em_radius", 6.0),
                           score_thresh=getattr(opts, "score_thresh", 0.4), max_restarts=getattr(opts, "max_restarts", None),
                           device=device, ctx=ctx)
    if verbose:
        # :119-126; the matrix plot needs matplotlib and the dense M (n <= 8192)
        M = _native.spectral_affinity(src, dst, c, o, F, _params(opts, 0), device=device, ctx=ctx)
        for i, m_value in enumerate(res.original_mask):
            print(f"Matching score: {M[i, i]:.4f}\tvalid match: {m_value > 0}/{res.segment[i]}")
        try:
            import matplotlib.pyplot as plt
        except ImportError:
            plt = None
        if plt is not None:
            plt.imshow(M)
            plt.colorbar()
            plt.tight_layout()
            plt.show()
    return res.segment, H, res.ransac_mask, res.original_mask


# ------------------------------------------------------------------ M-step and EM loop (:165-241)
def _check_loss(loss, lms, param):
    """``loss``: None (the solver follows from ``lms`` and the parameter alone) or "huber" (needs lms and a parameter > 1e-2)."""
    if loss is None:
        return False
    if loss != "huber":
        raise ValueError(f"loss must be None or 'huber'; got {loss!r}")
    if not lms:
        raise ValueError("loss='huber' needs lms=True (the Huber loss belongs to LMSSolver)")
    if not param > 1e-2:
        raise ValueError(f"loss='huber' needs a Huber parameter > 1e-2; got {param!r}")
    return True


def model_solve(kpts_cp, kpts_op, matches, weights, param=0.5, max_iter=8000, verbose=False, swap=True, lms=True, device=-1,
                ctx=None, loss=None):
    """spectral_method.py:165-186: the matches with weight > 1e-3 (in order) into LMSSolver(max_iter, param) or
    SDPSolver(max_iter, param, param).  Note the reference's defaults: lms=True with param=0.5 is the Huber loss, which
    raises NotImplementedError under that spelling; ``loss="huber"`` (with lms=True and param > 1e-2, else ValueError) runs
    it: HuberSolver(max_iter, param)."""
    from .model import HuberSolver, LMSSolver, SDPSolver, solve_params
    if _check_loss(loss, lms, param):
        solver = HuberSolver(max_iter, param, device=device, ctx=ctx)
    else:
        solver = LMSSolver(max_iter, param, device=device, ctx=ctx) if lms else SDPSolver(max_iter, param, param, device=device, ctx=ctx)
    params = solver._params(swap)
    params[3] = _native.MODEL_FLOOR
    src, dst = cv_to_array(kpts_cp, kpts_op, matches)
    w = np.ascontiguousarray(weights, dtype=np.float32).ravel()
    if len(src) == 0 or not np.any(w.astype(np.float64) > _native.MODEL_FLOOR):
        raise IndexError("too many indices for array: array is 1-dimensional, but 3 were indexed (no match selected)")
    start = time.time()
    if verbose:
        solver._announce(int(np.count_nonzero(w.astype(np.float64) > _native.MODEL_FLOOR)))
    H, solver.last = solve_params(params, src, dst, w, device=device, ctx=ctx)
    if verbose:
        print(f"Problem solved. Time consumption: {time.time() - start:.3f}")
        print("The optimal value is", solver.last.objective)
        print("Optimal solution:", H.ravel())
    return H


class EMRound(NamedTuple):
    H_pred: np.ndarray          # (3, 3) float32: model_solve's result
    spectral: SpectralResult    # the round's calculate_M (its H: Hg, or the first round's RANSAC homography)
    model: object               # model.ModelResult of the round's M-step


class EMResult(NamedTuple):
    rounds: list                # EMRound per EM step
    H_save: np.ndarray          # (3, 3) float64: inv(H_pred of the last round), normalised (:235-236)


def _model_mode(lms, fluc, huber_param, loss=None):
    if _check_loss(loss, lms, huber_param):
        return _native.model_params(_native.MODEL_HUBER, float(huber_param))
    if lms:
        if huber_param > 1e-2:
            raise NotImplementedError("spectral_em with lms=True and huber_param > 1e-2 (the Huber loss) is not implemented on "
                                      "the GPU: only the least-squares and SDP M-steps are")
        return _native.model_params(_native.MODEL_LMS)
    return _native.model_params(_native.MODEL_SDP, fluc, fluc)


def spectral_em(src_pts, dst_pts, c_feats, o_feats, F, *, em_steps=2, lms=False, fluc=0.5, huber_param=-1.0, epi_weight=0.5,
                affinity_eps=30.0, aff_thresh=0.5, em_radius=6.0, score_thresh=0.4, max_restarts=None, mask=None, swap=True,
                device=-1, ctx=None, loss=None):
    """The EM loop of spectral_method() (:188-241) on arrays: ``em_steps`` rounds of calculate_M (Hg = the previous round's
    H_pred) and model_solve(ransac_mask, param = huber_param if lms else fluc), all enqueued on the device at once.  The
    first round's initial mask: ``mask``, else the GPU RANSAC of this repository (as spectral_weights; ``swap`` sets only the
    direction of that RANSAC, as in match_RANSAC).  The M-step always inverts and normalises its solution (model_solve's
    default swap=True, which spectral_method() uses).  Returns an EMResult.  Raises as model_solve (IndexError when a round selects no match, ValueError for a degenerate selection,
    LinAlgError for a singular solution); warns as spectral_weights and the SDP solver.  ``loss="huber"`` (with lms=True and
    huber_param > 1e-2, else ValueError) runs the Huber M-step in every round; without it that spelling raises
    NotImplementedError."""
    from .model import result_of, warn_no_convergence
    mp = _model_mode(lms, fluc, huber_param, loss)
    src = np.ascontiguousarray(src_pts, dtype=np.float32)
    dst = np.ascontiguousarray(dst_pts, dtype=np.float32)
    sp = _native.spectral_params(epi_weight, affinity_eps, aff_thresh, em_radius, score_thresh,
                                 0 if max_restarts is None else max_restarts)
    H0 = None
    if mask is None:
        if src.ndim != 2 or len(src) == 0:
            raise ValueError(f"no matches, or points not (n, 2): {src.shape}")
        a, b = (dst, src) if swap else (src, dst)
        H0, m = _native.find_homography_ransac(a, b, 5.0, device=device, ctx=ctx)
        mask = m.astype(np.float32).ravel()
    try:
        out = _native.spectral_em(src, dst, c_feats, o_feats, F, sp, mp, em_steps, mask, device=device, ctx=ctx)
    except _native.ApapValueError as e:
        # the info blocks hold results only for rounds the kernels ran (NaN otherwise: an argument error)
        out = getattr(e, "info", None)
        info = out[1] if out is not None else np.empty((0, _native.MODEL_INFO))
        status = info[:, _native.MODEL_INFO_STATUS]
        bad = next((k for k in range(len(info)) if not np.isnan(status[k]) and int(status[k]) & _native.STATUS_MODEL_DEGENERATE),
                   None)
        if bad is not None and info[bad][_native.MODEL_INFO_COUNT] == 0:
            raise IndexError(f"too many indices for array: array is 1-dimensional, but 3 were indexed (EM round {bad} "
                             "selected no match)") from e
        raise
    H, info, seg, rm, om, sinfo = out
    rounds = []
    for k in range(em_steps):
        res = _result(seg[k], rm[k], om[k], sinfo[k], H0 if k == 0 else H[k - 1])
        m = result_of(info[k])
        warn_no_convergence(m)
        rounds.append(EMRound(H[k], res, m))
    H_save = np.linalg.inv(H[-1]).astype(np.float64)
    H_save /= H_save[-1, -1]
    return EMResult(rounds, H_save)


def warp_results(center_img, other_img, H_baseline, H_pred, direct_blend=False, device=-1, ctx=None):
    """spectral_method.py:227-229, the ``-s`` option: ``(warpped_baseline, warpped_result)`` =
    ``(image_warping(center_img, other_img, H_baseline, False), image_warping(center_img, other_img, H_pred, False))`` as one
    batched call - one kernel launch, the two pictures uploaded once.  ``H_baseline``: the first round's
    ``SpectralResult.H`` (the RANSAC homography); ``H_pred``: ``em.rounds[-1].H_pred``."""
    from .utils import image_warping_batch
    if H_baseline is None or H_pred is None:
        raise ValueError("warp_results needs both homographies (RANSAC found no model?)")
    baseline, result = image_warping_batch([(center_img, other_img, H_baseline, direct_blend),
                                            (center_img, other_img, H_pred, direct_blend)], device=device, ctx=ctx)
    return baseline, result


_EM_OPTIONS = {"lms": False, "fluc": 0.5, "huber_param": -1.0, "epi_weight": 0.5, "affinity_eps": 30.0, "aff_thresh": 0.5,
               "em_radius": 6.0, "score_thresh": 0.4, "max_restarts": None}


def spectral_em_batch(pairs, problems, *, em_steps=2, swap=True, device=-1, ctx=None):
    """Many EM problems in one call, advancing in lockstep on the device (``apap_spectral_em_batch``): the number of kernel
    launches does not grow with the number of problems.  ``pairs``: a sequence of ``(src, dst, c_feats, o_feats, F, mask)``
    (``mask`` None: the GPU RANSAC of this repository, once per pair, as spectral_em); ``problems``: a sequence of
    ``(pair_index, options)``, the options being spectral_em's keywords ``lms``, ``fluc``, ``huber_param``, ``epi_weight``,
    ``affinity_eps``, ``aff_thresh``, ``em_radius``, ``score_thresh`` and ``max_restarts`` (equal across the batch).  Returns
    one EMResult per problem, each equal byte for byte to spectral_em's for that problem alone.

    Unlike spectral_em this does not raise for a problem's status (a degenerate selection, a singular solution):
    ``EMRound.model.status`` carries the bits, H_pred is NaN for a degenerate round, and ``H_save`` is all NaN when the last
    H_pred is not finite.  The restart cap and the interior-point cap are warned about once per call, with the count of
    affected problems."""
    from .model import result_of
    pairs, problems = list(pairs), list(problems)
    if not pairs or not problems:
        raise ValueError("spectral_em_batch needs at least one pair and one problem")
    arrays, H0 = [], []
    for i, pair in enumerate(pairs):
        if len(pair) != 6:
            raise ValueError(f"pair {i}: expected (src, dst, c_feats, o_feats, F, mask_or_None)")
        src, dst, c, o, F, n = _native._spectral_inputs(*pair[:5])
        mask, h0 = pair[5], None
        if mask is None:
            a, b = (dst, src) if swap else (src, dst)
            h0, m = _native.find_homography_ransac(a, b, 5.0, device=device, ctx=ctx)
            mask = m
        mask = np.ascontiguousarray(mask, dtype=np.float32).ravel()
        if mask.shape != (n,):
            raise ValueError(f"pair {i}: mask must hold {n} values; got {mask.shape}")
        arrays.append((src, dst, c, o, F, mask))
        H0.append(h0)
    pair_of, sp, mp = [], [], []
    for b, (idx, options) in enumerate(problems):
        if not isinstance(idx, (int, np.integer)) or not 0 <= idx < len(pairs):
            raise ValueError(f"problem {b}: pair_index {idx!r} outside 0 .. {len(pairs) - 1}")
        unknown = set(options) - set(_EM_OPTIONS)
        if unknown:
            raise TypeError(f"problem {b}: unknown option(s) {sorted(unknown)}")
        opt = {**_EM_OPTIONS, **options}
        mp.append(_model_mode(opt["lms"], opt["fluc"], opt["huber_param"]))
        sp.append(_native.spectral_params(opt["epi_weight"], opt["affinity_eps"], opt["aff_thresh"], opt["em_radius"],
                                          opt["score_thresh"], 0 if opt["max_restarts"] is None else opt["max_restarts"]))
        pair_of.append(int(idx))
    cat = [np.concatenate([a[i] for a in arrays]) for i in (0, 1, 2, 3)]
    H, info, seg, rm, om, sinfo, status = _native.spectral_em_batch(
        cat[0], cat[1], cat[2], cat[3], np.stack([a[4] for a in arrays]), np.concatenate([a[5] for a in arrays]),
        [len(a[0]) for a in arrays], pair_of, np.stack(sp), np.stack(mp), em_steps, device=device, ctx=ctx)
    results, capped, ipm_capped = [], 0, 0
    for b, idx in enumerate(pair_of):
        rounds = []
        for k in range(em_steps):
            si = sinfo[b, k]
            res = SpectralResult(seg[b][k], rm[b][k], om[b][k], H0[idx] if k == 0 else H[b, k - 1], float(si[0]), float(si[1]),
                                 int(si[2]), int(si[4]), float(si[5]), not int(si[3]) & _native.STATUS_NO_CONVERGENCE)
            rounds.append(EMRound(H[b, k], res, result_of(info[b, k])))
        capped += bool(status[b] & _native.STATUS_NO_CONVERGENCE)
        ipm_capped += bool(status[b] & _native.STATUS_MODEL_NO_CONVERGENCE)
        if np.all(np.isfinite(H[b, -1])):
            H_save = np.linalg.inv(H[b, -1]).astype(np.float64)
            H_save /= H_save[-1, -1]
        else:
            H_save = np.full((3, 3), np.nan)
        results.append(EMResult(rounds, H_save))
    if capped:
        warnings.warn(f"spectral_em_batch: the eigen-solver hit its restart cap in {capped} of {len(problems)} problems; the best "
                      "Ritz vector is used there", RuntimeWarning, stacklevel=2)
    if ipm_capped:
        warnings.warn(f"spectral_em_batch: the interior-point method hit its iteration cap in {ipm_capped} of {len(problems)} "
                      "problems; the best iterate is returned there", RuntimeWarning, stacklevel=2)
    return results


_GRID_ORDER = ("affinity_eps", "aff_thresh", "epi_weight", "fluc")   # grid_search.sh's loops, outermost first


def spectral_em_grid(pair, grid, **fixed):
    """The parameter grid of the reference's ``grid_search.sh`` on one pair, as one batch: ``grid`` maps option names to value
    lists; ``fixed``: the other options, and spectral_em_batch's ``em_steps`` / ``swap`` / ``device`` / ``ctx``.  Returns
    ``(list of option dicts, list of EMResult)`` in the script's nesting order: ``affinity_eps`` outermost, then
    ``aff_thresh``, ``epi_weight``, ``fluc`` (any other grid key varies faster, in the mapping's order)."""
    import itertools
    call = {k: fixed.pop(k) for k in ("em_steps", "swap", "device", "ctx") if k in fixed}
    names = [k for k in _GRID_ORDER if k in grid] + [k for k in grid if k not in _GRID_ORDER]
    clash = set(names) & set(fixed)
    if clash:
        raise TypeError(f"option(s) {sorted(clash)} both in the grid and fixed")
    options = [{**fixed, **dict(zip(names, values))} for values in itertools.product(*(list(grid[k]) for k in names))]
    if not options:
        raise ValueError("empty grid")
    return options, spectral_em_batch([pair], [(0, o) for o in options], **call)


# ------------------------------------------------------------------ utils.py:162-186
def skew_symmetric_transform(t):
    """utils.py:162-168 (float32, as the reference)."""
    x, y, z = t
    return np.float32([[0, -z, y], [z, 0, -x], [-y, x, 0]])


def fundamental(Rc, Ro, tc, to, K):
    """utils.py:171-178: F from the two camera poses and the intrinsics."""
    Ro_inv = np.linalg.inv(Ro)
    Rr = Ro_inv @ Rc
    tr = Ro_inv @ (tc - to)
    ss_t = skew_symmetric_transform(tr)
    K_inv = np.linalg.inv(K)
    return K_inv.T @ ss_t @ Rr @ K_inv


def estimate_fundamental(src_pts, dst_pts, thresh=3.0, iterations=_native.RANSAC_ITERATIONS, seed=_native.RANSAC_SEED, device=-1,
                         ctx=None):
    """F from the matches alone, for a pair without calibration: ``cv.findFundamentalMat(src_pts, dst_pts, cv.FM_RANSAC,
    thresh)`` with this repository's GPU estimator (include/apap_hip.h; 8-point RANSAC on the Sampson distance, re-fitted to
    its inliers, rank 2).  ``src_pts`` (the centre picture's) and ``dst_pts`` (n, 2), n >= 8, as ``cv_to_array`` returns them.
    Returns ``(F (3, 3) float64 or None, mask (n,) float32)`` with ``dst_h^T F src_h = 0`` - the F that calculate_M,
    spectral_weights and spectral_em take - scaled so that ``|dst^T F src|`` is at most the distance in pixels of ``dst`` from
    the epipolar line of ``src``.  ``None`` when fewer than 8 matches agree."""
    F, mask = _native.find_fundamental_ransac(src_pts, dst_pts, thresh, iterations, seed, device=device, ctx=ctx)
    return F, mask.astype(np.float32).ravel()


def estimate_fundamental_batch(pairs, thresh=3.0, iterations=_native.RANSAC_ITERATIONS, seed=_native.RANSAC_SEED, device=-1,
                               ctx=None):
    """``estimate_fundamental`` for a sequence of ``(src_pts, dst_pts)`` in one call (the number of kernel launches does not grow
    with the number of pairs): a list of ``(F or None, mask float32)``, each equal to the pair's own call."""
    got = _native.find_fundamental_ransac_batch(pairs, thresh, iterations, seed, device=device, ctx=ctx)
    return [(F, mask.astype(np.float32).ravel()) for F, mask in got]


def match_fundamental(kpts_cp, kpts_op, matches, thresh=3.0, device=-1, ctx=None):
    """The counterpart of ``match_RANSAC`` for the epipolar geometry: ``(F, mask float32)`` of the matched keypoints."""
    src_pts, dst_pts = cv_to_array(kpts_cp, kpts_op, matches)
    return estimate_fundamental(src_pts, dst_pts, thresh, device=device, ctx=ctx)


def get_fundamental(case_idx, center_idx, img_idx, root="../diff_1/raw_data"):
    """utils.py:180-186.  Reads ``{root}/case{i}/Parameters.xlsx`` (needs pandas with an xlsx reader, and scipy)."""
    import pandas as pd
    from scipy.spatial.transform import Rotation as Rot

    path = f"{root}/case{case_idx}/Parameters.xlsx"
    poses = pd.read_excel(path, sheet_name="Parameters of UAV").to_numpy()[..., 1:].astype(np.float32)
    position, euler_angles = poses[..., :3], poses[..., 3:]
    Rs = []
    for euler in euler_angles:
        euler[1] = -euler[1]
        Rs.append(Rot.from_euler("yzx", euler, degrees=True).as_matrix())
    R = np.stack(Rs, axis=0)
    K = pd.read_excel(path, sheet_name="Parameters of camera").to_numpy()[..., 1:].astype(np.float32)
    return fundamental(R[center_idx - 1], R[img_idx - 1], position[center_idx - 1], position[img_idx - 1], K)
