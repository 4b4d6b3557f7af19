"""The homography solvers of the reference's ``pyviz/model.py`` (the M-step of the spectral method) on the GPU, without cvxpy.

* ``LMSSolver(max_iter, huber_param=-1.0)``: min ||A h - rhs||^2, the exact least-squares solution (a QR of the rows and
  back-substitution in fp64).  With ``huber_param > 1e-2`` the reference minimises the Huber loss instead; under that
  spelling this class still raises NotImplementedError: the Huber loss is ``HuberSolver``.
* ``HuberSolver(max_iter, huber_param)``: min sum_j phi_M(r_j), r = A h - rhs, phi_M(r) = r^2 for |r| <= M and
  2 M |r| - M^2 beyond (cvxpy's ``huber(x, M)``, M = huber_param > 1e-2), solved to a relative duality gap of 1e-10 by
  Newton steps on the active quadratic piece with a halving line search, inside one kernel launch (include/apap_hip.h,
  DESIGN.md "Huber M-step").  ``.last.gap`` is a certificate computed from the rows: it does not depend on the method.
* ``SDPSolver(max_iter, du=1.0, dv=1.0)``: min r + t subject to the reference's (2N+3)-sized LMI, solved exactly (to a
  relative duality gap of 1e-10) on an equivalent 18 x 18 LMI by a primal-dual interior-point method (include/apap_hip.h,
  DESIGN.md "M-step and EM loop").  The reference hands the same programme to SCS with ``max_iters = max_iter``; its answer
  is SCS's approximation, this one the optimum, so the two differ by however far SCS stopped from it.

``.solve(pts_c, pts_o, weights, verbose=1, swap=True)`` returns the float32 3 x 3 the reference returns (model.py:50-56:
h rounded to float32, [2, 2] = 1, inverted and normalised when ``swap``).  Every match passed is used (model_solve of
spectral_method applies the 1e-3 weight floor).  No point: IndexError, as the reference's ``pts_c[:, None, :]``.  ``.last``
holds the solve's ``ModelResult``.  No CPU fallback.

Deviation for direct calls: points and weights are rounded to float32 and the rows built from them as from model_solve's
float32 arrays.  The reference builds A and rhs in the callers' dtype, so float64 inputs (its own ``validation_test``) give it
float64 rows; here they give the rows of the float32-rounded inputs.  ``spectral_method.model_solve`` always passes float32,
so it is not affected.
"""
from __future__ import annotations

import time
import warnings
from typing import NamedTuple

import numpy as np

from . import _native

__all__ = ["SDPSolver", "LMSSolver", "HuberSolver", "ModelResult"]


class ModelResult(NamedTuple):
    h: np.ndarray          # (8,) float64: the solution before the float32 tail
    objective: float       # SDP: r + t; LMS: ||A h - rhs||^2; Huber: sum phi_M(A h - rhs)
    gap: float             # SDP: tr(S Z) / (r + t) of the returned iterate; LMS: 0; Huber: the relative duality gap of h
    iterations: int        # interior-point iterations (LMS: 0); Huber: accepted steps
    status: int            # APAP_STATUS_* bits (STATUS_MODEL_NO_CONVERGENCE: the gap stayed above 1e-10)
    r: float               # SDP: r (NaN for LMS)
    t: float               # SDP: t (NaN for LMS)
    Z: np.ndarray          # SDP: (3, 3) dual block (order u, v, q), the optimality certificate (NaN for LMS)
    count: int             # matches used


def result_of(info):
    info = np.asarray(info, np.float64)
    return ModelResult(info[_native.MODEL_INFO_H:_native.MODEL_INFO_H + 8].copy(), float(info[_native.MODEL_INFO_OBJECTIVE]),
                       float(info[_native.MODEL_INFO_GAP]), int(info[_native.MODEL_INFO_ITERS]),
                       int(info[_native.MODEL_INFO_STATUS]), float(info[_native.MODEL_INFO_R]), float(info[_native.MODEL_INFO_T]),
                       info[_native.MODEL_INFO_Z:_native.MODEL_INFO_Z + 9].reshape(3, 3).copy(),
                       int(info[_native.MODEL_INFO_COUNT]))


def warn_no_convergence(res, stacklevel=3):
    if res.status & _native.STATUS_MODEL_NO_CONVERGENCE:
        # the SDP reports r and t, the Huber M-step leaves them NaN
        method = "Huber: the Newton iteration" if np.isnan(res.r) else "SDP: the interior-point method"
        warnings.warn(f"{method} stopped at relative gap {res.gap:.3e} after {res.iterations} iterations "
                      "(target 1e-10); the best iterate is returned", RuntimeWarning, stacklevel=stacklevel)


def check_points(pts_c):
    """The reference's exception for no point: np.float32([]) has shape (0,), and pts_c[:, None, :] fails (model.py:30)."""
    if np.size(pts_c) == 0:
        raise IndexError("too many indices for array: array is 1-dimensional, but 3 were indexed (no point)")


def solve_params(params, pts_c, pts_o, weights, device=-1, ctx=None):
    """``_native.model_solve`` with the reference's exception for no point: (H, ModelResult)."""
    check_points(pts_c)
    H, info = _native.model_solve(pts_c, pts_o, weights, params, device=device, ctx=ctx)
    res = result_of(info)
    warn_no_convergence(res, stacklevel=4)
    return H, res


class LMSSolver:
    def __init__(self, max_iter, huber_param=-1.0, *, device=-1, ctx=None) -> None:
        """``max_iter``: the cap the reference gives its cvxpy solver; kept for the signature, an exact solve needs none."""
        self.huber_param = huber_param
        self.max_iter = max_iter
        self.device = device
        self.ctx = ctx
        self.last = None

    @staticmethod
    def get_shifted(pts, num_points, x=1.0):
        """model.py:22-27."""
        padded = np.concatenate([pts, np.repeat(np.float32([[x, 0, 0, 0]]), num_points, axis=0)], axis=-1)
        rolled = np.roll(padded, shift=3, axis=-1)
        return np.concatenate([np.expand_dims(padded, axis=-2), np.expand_dims(rolled, axis=-2)], axis=-2)

    def _params(self, swap):
        if self.huber_param > 1e-2:
            raise NotImplementedError("LMSSolver with huber_param > 1e-2 (the Huber loss) is not implemented on the GPU: "
                                      "only the least-squares and SDP M-steps are")
        return _native.model_params(_native.MODEL_LMS, floor=None, swap=swap)

    def _announce(self, n):
        print(f"Start solving... point num: {n}. Huber Loss Used = [{self.huber_param > 1e-2}]")

    def solve(self, pts_c, pts_o, weights, verbose=1, swap=True):
        params = self._params(swap)
        check_points(pts_c)     # before the announcement, as in the reference
        n = np.shape(pts_c)[0]
        start = time.time()
        if verbose:
            self._announce(n)
        H, self.last = solve_params(params, pts_c, pts_o, weights, device=self.device, ctx=self.ctx)
        if verbose:
            print(f"Problem solved. Time consumption: {time.time() - start:.3f}")
            print("The optimal value is", self.last.objective)
            print("Optimal solution:", H.ravel())
        return H


class SDPSolver(LMSSolver):
    def __init__(self, max_iter, du=1.0, dv=1.0, *, device=-1, ctx=None) -> None:
        """``max_iter``: SCS's iteration cap in the reference (``solve(solver='SCS', max_iters=max_iter)``); the interior-point
        method here stops at a relative duality gap of 1e-10 (or after 80 iterations) and does not use it."""
        super().__init__(max_iter, -1.0, device=device, ctx=ctx)
        self.du = du
        self.dv = dv

    def _params(self, swap):
        return _native.model_params(_native.MODEL_SDP, self.du, self.dv, floor=None, swap=swap)

    def _announce(self, n):
        print(f"Start solving SDP Problem... point num: {n}")


class HuberSolver(LMSSolver):
    def __init__(self, max_iter, huber_param, *, device=-1, ctx=None) -> None:
        """The reference's ``LMSSolver(max_iter, huber_param)`` with ``huber_param > 1e-2`` (model.py:36-41).  ``max_iter``:
        kept for the signature; the iteration here stops at a relative duality gap of 1e-10 (or after 100 steps)."""
        if not huber_param > 1e-2:
            raise ValueError(f"HuberSolver needs huber_param > 1e-2 (got {huber_param!r}); at or below it the reference solves "
                             "least squares: LMSSolver")
        if not np.isfinite(huber_param):
            raise ValueError(f"HuberSolver needs a finite huber_param (got {huber_param!r})")
        super().__init__(max_iter, huber_param, device=device, ctx=ctx)

    def _params(self, swap):
        return _native.model_params(_native.MODEL_HUBER, float(self.huber_param), floor=None, swap=swap)
