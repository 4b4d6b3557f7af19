"""ctypes binding of ``libapap_hip.so`` (the C ABI declared in ``include/apap_hip.h``).

This is the whole Python<->native boundary: plain pointers and sizes, no torch types.
The library is built in-tree by ``cvx_proj_amd/csrc/Makefile`` (see
``__graft_entry__.build``).  There is no CPU fallback: if the library is missing or no
gfx950 device is visible, compute calls raise :class:`ApapError`.
"""
from __future__ import annotations

import ctypes as C
import os
import sys
from typing import NamedTuple

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# APAP_HIP_LIB: load another build of the library (A/B tooling: tools/ab_build.sh); default in-tree
LIB_PATH = os.environ.get("APAP_HIP_LIB") or os.path.join(_HERE, "libapap_hip.so")

OK, ERR_INVALID_ARG, ERR_NO_DEVICE, ERR_HIP, ERR_SINGULAR, ERR_INDEX, ERR_WORKSPACE = range(7)
ABI_VERSION = 6          # APAP_ABI_VERSION of include/apap_hip.h
# kernel slots of apap_ctx_profile_read (include/apap_hip.h)
PROF_NAMES = ("assemble", "eigen", "invert", "lut", "warp", "eq_hist", "eq_apply", "ransac", "spectral")
PROF_SLOTS = len(PROF_NAMES)
TABLE_STRIDE = 32
DENORM_DOUBLES = 36
VARIANT_AUTO, VARIANT_VALU, VARIANT_MFMA, VARIANT_MFMA4, VARIANT_MFMA4X2 = 0, 1, 2, 3, 4
EIGEN_AUTO, EIGEN_JACOBI, EIGEN_INVERSE_ITERATION = 0, 1, 2
# options of a context (include/apap_hip.h)
OPT_SOLVER_VARIANT, OPT_EIGEN_SOLVER, OPT_CAREFUL, OPT_PROFILE, OPT_WANT_WAVES, OPT_WARP_ROWS, OPT_WEIGHT_CHUNK_KB, \
    OPT_FUSED_MAX_CELLS, OPT_WARP_FAST, OPT_OVERLAP_PCIE, OPT_PLAN_CELLS, OPT_MOMENTS, OPT_WEIGHTS_F32, \
    OPT_PLAN_SLOTS, OPT_WARP_SAMPLING = range(15)
SAMPLING_NEAREST, SAMPLING_BILINEAR = 0, 1      # values of OPT_WARP_SAMPLING
SAMPLINGS = {"nearest": SAMPLING_NEAREST, "bilinear": SAMPLING_BILINEAR}


class ApapError(RuntimeError):
    """A native call failed; ``code`` is one of the APAP_ERR_* values.  The conditions the
    reference signals with a specific Python exception raise a subclass that is ALSO that
    exception, so ``except np.linalg.LinAlgError`` / ``except IndexError`` / ``except ValueError``
    around the reference's class keep working around this one."""

    def __init__(self, code, message):
        super().__init__(f"[apap_hip error {code}] {message}")
        self.code = code


class ApapSingularError(ApapError, np.linalg.LinAlgError):
    """APAP_ERR_SINGULAR: ``numpy.linalg.inv`` of a cell raised LinAlgError("Singular matrix")
    (apap.py:165-166,203,252)."""


class ApapIndexError(ApapError, IndexError):
    """APAP_ERR_INDEX: ``np.where(i < mesh_h)[0][0]`` found no edge above a canvas index
    (apap.py:207,209)."""


class ApapValueError(ApapError, ValueError):
    """APAP_ERR_INVALID_ARG: what the reference's shape unpacking rejects with ValueError
    (apap.py:129-130,197,199)."""


_ERROR_CLASSES = {ERR_SINGULAR: ApapSingularError, ERR_INDEX: ApapIndexError, ERR_INVALID_ARG: ApapValueError}

# bits of the device status word of the resident entry points (APAP_STATUS_* of include/apap_hip.h)
STATUS_SINGULAR, STATUS_INDEX, STATUS_UNPREPARED = 1, 2, 4
STATUS_NO_CONVERGENCE = 8     # the spectral eigen-solver hit its restart cap (a warning, not an error)
STATUS_MODEL_DEGENERATE = 16  # M-step: fewer than 4 selected matches or a rank-deficient system (H is NaN)
STATUS_MODEL_NO_CONVERGENCE = 32  # M-step: the interior-point method hit its iteration cap (a warning, not an error)


def raise_for_status(word, who):
    """Raise what the host-buffer calls make of a device status word (``status_to_code`` of csrc/apap_capi.hip: the same
    bits in the same order, the same exception classes and wording); return quietly when none of the bits is set."""
    if word & STATUS_SINGULAR:
        raise ApapSingularError(ERR_SINGULAR, f"{who}: Singular matrix")
    if word & STATUS_INDEX:
        raise ApapIndexError(ERR_INDEX, f"{who}: index 0 is out of bounds for axis 0 with size 0 (mesh edges do not cover the canvas)")
    if word & STATUS_UNPREPARED:
        raise ApapValueError(ERR_INVALID_ARG, f"{who}: the warp workspace holds no lookup tables for this mesh / canvas "
                                              "(APAP_WARP_GEOMETRY)")


_f32p = C.POINTER(C.c_float)
_f64p = C.POINTER(C.c_double)
_u8p = C.POINTER(C.c_uint8)
_i32p = C.POINTER(C.c_int)
_i64p = C.POINTER(C.c_longlong)
_vp = C.c_void_p

# name -> (restype, argtypes).  Must list every symbol include/apap_hip.h declares;
# tests/test_capi_symbols.py parses the header and checks this table against it.
SIGNATURES = {
    "apap_last_error": (C.c_char_p, []),
    "apap_version": (C.c_char_p, []),
    "apap_abi_version": (C.c_int, []),
    "apap_device_count": (C.c_int, []),
    "apap_ctx_create": (C.c_void_p, []),
    "apap_ctx_destroy": (None, [_vp]),
    "apap_ctx_set_option": (C.c_int, [_vp, C.c_int, C.c_int]),
    "apap_ctx_get_option": (C.c_int, [_vp, C.c_int, _i32p]),
    "apap_ctx_set_short_chain": (C.c_int, [_vp, C.c_int]),
    "apap_ctx_get_short_chain": (C.c_int, [_vp, _i32p]),
    "apap_ctx_profile_read": (C.c_int, [_vp, _f32p, _i32p]),
    "apap_ctx_profile_k1_chunks": (C.c_int, [_vp, C.POINTER(C.c_uint), C.POINTER(C.c_uint)]),
    "apap_host_prepare": (C.c_int, [_f32p, _f32p, C.c_int] + [_f32p] * 10),
    "apap_host_dlt_rows": (C.c_int, [_f32p, _f32p, C.c_int, _f32p]),
    "apap_host_prepare_pts": (C.c_int, [_vp, C.c_int, _vp, C.c_int, C.c_int] + [_f32p] * 6 + [_f64p] * 4),
    "apap_host_dlt_rows_pts": (C.c_int, [_f64p, _f64p, C.c_int, C.c_int, _f32p]),
    "apap_host_build_table_rows": (C.c_int, [_f64p, _f32p, C.c_int, _f64p]),
    "apap_host_build_table": (C.c_int, [_f32p, _f32p, _f32p, C.c_int, _f64p]),
    "apap_host_build_table24": (C.c_int, [_f64p, _f32p, C.c_int, _f64p]),
    "apap_host_build_denorm": (C.c_int, [_f32p, _f32p, _f32p, _f32p, _f64p]),
    "apap_local_homography": (C.c_int, [_vp, _f32p, _f32p, C.c_int, _f64p, C.c_int, C.c_int, C.c_double,
                                        C.c_double, _f32p, _f64p, C.c_int]),
    "apap_local_weights": (C.c_int, [_vp, _f32p, C.c_int, _f64p, C.c_int, C.c_double, C.c_double, _f64p, C.c_int]),
    "apap_local_homography_pts": (C.c_int, [_vp, _vp, C.c_int, _vp, C.c_int, C.c_int, _f64p, C.c_int, C.c_int, C.c_double,
                                            C.c_double, _f32p, _f64p, C.c_int]),
    "apap_local_weights_pts": (C.c_int, [_vp, _vp, C.c_int, C.c_int, _f64p, C.c_int, C.c_double, C.c_double, _f64p, C.c_int]),
    "apap_local_warp": (C.c_int, [_vp, _u8p, C.c_int, C.c_int, _f32p, C.c_int, C.c_int, _f64p, C.c_int, _f64p,
                                  C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _u8p, _f32p, C.c_int]),
    "apap_local_warp_f64": (C.c_int, [_vp, _u8p, C.c_int, C.c_int, _f64p, C.c_int, C.c_int, _f64p, C.c_int, _f64p,
                                      C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _u8p, _f64p, C.c_int]),
    "apap_local_stitch": (C.c_int, [_vp, _u8p, C.c_int, C.c_int, _u8p, C.c_int, C.c_int, _f32p, C.c_int, C.c_int, _f64p,
                                    C.c_int, _f64p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _u8p, _f32p, C.c_int]),
    "apap_warp_coords": (C.c_int, [_vp, _f32p, C.c_int, C.c_int, _f64p, C.c_int, _f64p, C.c_int, C.c_int, C.c_int,
                                   C.c_int, C.c_int, _f64p, C.c_int]),
    "apap_invert_normalize_flatten": (C.c_int, [_vp, _f32p, C.c_int, _f64p, C.c_int]),
    "apap_uniform_blend": (C.c_int, [_vp, _u8p, _u8p, C.c_int, C.c_int, _u8p, C.c_int]),
    "apap_solve_workspace_bytes": (C.c_size_t, [_vp, C.c_int, C.c_int]),
    "apap_solve_device": (C.c_int, [_vp, _vp, C.c_int, _vp, C.c_int, C.c_double, C.c_double, _vp, _vp, _vp,
                                    C.c_size_t, _vp]),
    "apap_solve_batch_workspace_bytes": (C.c_size_t, [_vp, C.c_int, C.c_int, C.c_int]),
    "apap_solve_batch_device": (C.c_int, [_vp, _vp, C.c_int, _vp, C.c_longlong, C.c_int, C.c_double, C.c_double, _vp, _vp,
                                          C.c_int, _vp, C.c_size_t, _vp]),
    "apap_solve_warp_batch_device": (C.c_int, [_vp, _vp, C.c_int, _vp, C.c_longlong, C.c_double, C.c_double, _vp, _vp, C.c_int, _vp,
                                               C.c_size_t, C.c_int, C.c_int, _vp, C.c_int, _vp, C.c_int, C.c_int, C.c_int, C.c_int,
                                               C.c_int, _vp, C.c_size_t, _vp, _vp]),
    "apap_weights_device": (C.c_int, [_vp, _vp, C.c_int, _vp, C.c_int, C.c_double, C.c_double, _vp, _vp]),
    "apap_warp_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "apap_warp_device": (C.c_int, [_vp, _vp, C.c_int, C.c_int, _vp, C.c_int, C.c_int, _vp, C.c_int, _vp, C.c_int,
                                   C.c_int, C.c_int, C.c_int, C.c_int, _vp, _vp, _vp, C.c_size_t, _vp, _vp]),
    "apap_warp_f64_device": (C.c_int, [_vp, _vp, C.c_int, C.c_int, _vp, C.c_int, C.c_int, _vp, C.c_int, _vp, C.c_int,
                                       C.c_int, C.c_int, C.c_int, C.c_int, _vp, _vp, _vp, C.c_size_t, _vp, _vp]),
    "apap_warp_rows_device": (C.c_int, [_vp, _vp, C.c_int, C.c_int, _vp, C.c_int, C.c_int, _vp, C.c_int, _vp, C.c_int,
                                        C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _vp, _vp, C.c_size_t, _vp,
                                        _vp]),
    "apap_warp_batch_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "apap_warp_batch_device": (C.c_int, [_vp, _vp, C.c_longlong, C.c_int, C.c_int, _vp, C.c_longlong, C.c_int, C.c_int, _vp, C.c_int,
                                         C.c_int, _vp, C.c_int, _vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                         _vp, C.c_longlong, _vp, C.c_int, C.c_int, _vp, C.c_size_t, _vp, _vp]),
    "apap_stitch_device": (C.c_int, [_vp, _vp, C.c_int, C.c_int, _vp, C.c_int, C.c_int, _vp, C.c_int, C.c_int, _vp, C.c_int,
                                     _vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _vp, _vp, _vp, C.c_size_t, _vp, _vp]),
    "apap_warp_coords_device": (C.c_int, [_vp, _vp, C.c_int, C.c_int, _vp, C.c_int, _vp, C.c_int, C.c_int, C.c_int,
                                          C.c_int, C.c_int, _vp, _vp, C.c_size_t, _vp, _vp]),
    "apap_flatten_device": (C.c_int, [_vp, _vp, C.c_int, _vp, _vp, _vp]),
    "apap_blend_device": (C.c_int, [_vp, _vp, _vp, C.c_int, C.c_int, _vp, _vp]),
    "apap_equalize_hist": (C.c_int, [_vp, _u8p, C.c_int, C.c_int, C.c_int, _u8p, C.c_int]),
    "apap_equalize_workspace_bytes": (C.c_size_t, [C.c_int]),
    "apap_equalize_hist_device": (C.c_int, [_vp, _vp, C.c_int, C.c_int, C.c_int, _vp, _vp, C.c_size_t, _vp]),
    "apap_find_homography_ransac": (C.c_int, [_vp, _f32p, _f32p, C.c_int, C.c_double, C.c_int, C.c_ulonglong, _f64p, _u8p,
                                              _i32p, C.c_int]),
    "apap_ransac_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "apap_ransac_device": (C.c_int, [_vp, _vp, _vp, C.c_int, C.c_double, C.c_int, C.c_ulonglong, _vp, _vp, _vp, _vp,
                                     C.c_size_t, _vp]),
    "apap_spectral_weights": (C.c_int, [_vp, _f32p, _f32p, _f32p, _f32p, C.c_int, _f64p, _f64p, _f32p, _f32p, _f64p, _f32p,
                                        _f32p, _f64p, C.c_int]),
    "apap_spectral_workspace_bytes": (C.c_size_t, [C.c_int]),
    "apap_spectral_device": (C.c_int, [_vp, _vp, _vp, _vp, _vp, C.c_int, _vp, _f64p, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                       C.c_size_t, _vp]),
    "apap_spectral_affinity": (C.c_int, [_vp, _f32p, _f32p, _f32p, _f32p, C.c_int, _f64p, _f64p, _f64p, C.c_int]),
    "apap_model_solve": (C.c_int, [_vp, _f32p, _f32p, _f32p, C.c_int, _f64p, _f32p, _f64p, C.c_int]),
    "apap_model_workspace_bytes": (C.c_size_t, [C.c_int]),
    "apap_model_solve_device": (C.c_int, [_vp, _vp, _vp, _vp, C.c_int, _f64p, _vp, _vp, _vp, _vp, C.c_size_t, _vp]),
    "apap_spectral_em": (C.c_int, [_vp, _f32p, _f32p, _f32p, _f32p, C.c_int, _f64p, _f64p, _f64p, C.c_int, _f32p, _f32p, _f64p,
                                   _f64p, _f32p, _f32p, _f64p, C.c_int]),
    "apap_spectral_em_device": (C.c_int, [_vp, _vp, _vp, _vp, _vp, C.c_int, _vp, _f64p, _f64p, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp,
                                          _vp, _vp, _vp, C.c_size_t, _vp]),
    "apap_spectral_em_batch_workspace_bytes": (C.c_size_t, [_i32p, C.c_int, _i32p, C.c_int]),
    "apap_spectral_em_batch_device": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32p, C.c_int, _i32p, _f64p, _f64p, C.c_int,
                                                C.c_int, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, C.c_size_t, _vp]),
    "apap_spectral_em_batch": (C.c_int, [_vp, _f32p, _f32p, _f32p, _f32p, _f64p, _f32p, _i32p, C.c_int, _i32p, _f64p, _f64p,
                                         C.c_int, C.c_int, _f32p, _f64p, _f64p, _f32p, _f32p, _f64p, _i32p, C.c_int]),
    "apap_local_model_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "apap_local_model_solve_device": (C.c_int, [_vp, _vp, _vp, _vp, C.c_int, _vp, C.c_int, C.c_double, C.c_double, _f64p, _vp, _vp,
                                                _vp, _vp, C.c_size_t, _vp]),
    "apap_local_model_solve": (C.c_int, [_vp, _f32p, _f32p, _f32p, C.c_int, _f64p, C.c_int, C.c_double, C.c_double, _f64p, _f32p,
                                         _f64p, _i32p, C.c_int]),
    "apap_match_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "apap_match_descriptors": (C.c_int, [_vp, _f32p, C.c_int, _f32p, C.c_int, _i32p, _f32p, _i32p, _f32p, C.c_int]),
    "apap_match_descriptors_device": (C.c_int, [_vp, _vp, C.c_int, _vp, C.c_int, _vp, _vp, _vp, _vp, _vp, C.c_size_t, _vp]),
    "apap_match_batch_workspace_bytes": (C.c_size_t, [_i32p, _i32p, C.c_int]),
    "apap_match_descriptors_batch": (C.c_int, [_vp, _f32p, _f32p, _i32p, _i32p, C.c_int, _i32p, _f32p, _i32p, _f32p, C.c_int]),
    "apap_match_descriptors_batch_device": (C.c_int, [_vp, _vp, _vp, _i32p, _i32p, C.c_int, _vp, _vp, _vp, _vp, _vp, C.c_size_t,
                                                      _vp]),
    "apap_guided_records": (C.c_int, [_vp, _f32p, C.c_int, _f64p, C.c_int, _f64p, C.c_int]),
    "apap_guided_records_device": (C.c_int, [_vp, _vp, C.c_int, _vp, C.c_int, _vp, _vp]),
    "apap_match_guided_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "apap_match_guided": (C.c_int, [_vp, _f64p, _f32p, C.c_int, _f64p, _f32p, C.c_int, C.c_int, C.c_double, _i32p, _f32p, _i32p,
                                    _f32p, _i32p, _i32p, _f32p, C.c_int]),
    "apap_match_guided_device": (C.c_int, [_vp, _vp, _vp, C.c_int, _vp, _vp, C.c_int, C.c_int, C.c_double, _vp, _vp, _vp, _vp, _vp,
                                           _vp, _vp, _vp, C.c_size_t, _vp]),
    "apap_match_guided_batch_workspace_bytes": (C.c_size_t, [_i32p, _i32p, C.c_int]),
    "apap_match_guided_batch": (C.c_int, [_vp, _f64p, _f64p, _f32p, _f32p, _i32p, _i32p, C.c_int, C.c_int, _f64p, _i32p, _f32p,
                                          _i32p, _f32p, _i32p, _i32p, _f32p, C.c_int]),
    "apap_match_guided_batch_device": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _i32p, _i32p, C.c_int, C.c_int, _f64p, _vp, _vp, _vp, _vp,
                                                 _vp, _vp, _vp, _vp, C.c_size_t, _vp]),
    "apap_sift_window": (C.c_int, [_f32p]),
    "apap_sift_taps": (C.c_int, [_f32p]),
    "apap_sift_workspace_bytes": (C.c_size_t, [C.c_int]),
    "apap_sift_describe": (C.c_int, [_vp, _u8p, C.c_int, C.c_int, C.c_int, _f32p, C.c_int, _f32p, C.c_int]),
    "apap_sift_describe_device": (C.c_int, [_vp, _vp, C.c_int, C.c_int, C.c_int, _vp, C.c_int, _vp, _vp, C.c_size_t, _vp]),
    "apap_sift_describe_batch": (C.c_int, [_vp, C.POINTER(C.c_void_p), _i32p, _i32p, _i32p, C.c_int, _f32p, _i32p, _f32p, C.c_int]),
    "apap_sift_describe_batch_device": (C.c_int, [_vp, C.POINTER(C.c_void_p), _i32p, _i32p, _i32p, C.c_int, _vp, _i32p, _vp, _vp,
                                                  C.c_size_t, _vp]),
    "apap_sift_orient_window": (C.c_int, [_f32p]),
    "apap_sift_descr_window": (C.c_int, [_f32p]),
    "apap_sift_orient_workspace_bytes": (C.c_size_t, [C.c_int]),
    "apap_sift_orient": (C.c_int, [_vp, _u8p, C.c_int, C.c_int, C.c_int, _f32p, C.c_int, _f32p, C.c_int]),
    "apap_sift_orient_device": (C.c_int, [_vp, _vp, C.c_int, C.c_int, C.c_int, _vp, C.c_int, _vp, _vp, C.c_size_t, _vp]),
    "apap_sift_orient_batch": (C.c_int, [_vp, C.POINTER(C.c_void_p), _i32p, _i32p, _i32p, C.c_int, _f32p, _i32p, _f32p, C.c_int]),
    "apap_sift_orient_batch_device": (C.c_int, [_vp, C.POINTER(C.c_void_p), _i32p, _i32p, _i32p, C.c_int, _vp, _i32p, _vp, _vp,
                                                C.c_size_t, _vp]),
    "apap_sift_describe_oriented": (C.c_int, [_vp, _u8p, C.c_int, C.c_int, C.c_int, _f32p, C.c_int, _f32p, _f32p, _f32p, C.c_int]),
    "apap_sift_describe_oriented_device": (C.c_int, [_vp, _vp, C.c_int, C.c_int, C.c_int, _vp, C.c_int, _vp, _vp, _vp, _vp, C.c_size_t,
                                                     _vp]),
    "apap_sift_describe_oriented_batch": (C.c_int, [_vp, C.POINTER(C.c_void_p), _i32p, _i32p, _i32p, C.c_int, _f32p, _i32p, _f32p,
                                                    _f32p, _f32p, C.c_int]),
    "apap_sift_describe_oriented_batch_device": (C.c_int, [_vp, C.POINTER(C.c_void_p), _i32p, _i32p, _i32p, C.c_int, _vp, _i32p, _vp,
                                                           _vp, _vp, _vp, C.c_size_t, _vp]),
    "apap_corner_workspace_bytes": (C.c_size_t, [_i32p, _i32p, C.c_int, C.c_int]),
    "apap_corner_detect": (C.c_int, [_vp, _u8p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _f32p, _i64p, _i32p, C.c_int]),
    "apap_corner_detect_device": (C.c_int, [_vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _vp, _vp, _vp, _vp,
                                            C.c_size_t, _vp]),
    "apap_corner_detect_batch": (C.c_int, [_vp, C.POINTER(C.c_void_p), _i32p, _i32p, _i32p, C.c_int, C.c_int, C.c_int, C.c_int, _f32p,
                                           _i64p, _i32p, C.c_int]),
    "apap_corner_detect_batch_device": (C.c_int, [_vp, C.POINTER(C.c_void_p), _i32p, _i32p, _i32p, C.c_int, C.c_int, C.c_int, C.c_int,
                                                  _vp, _vp, _vp, _vp, C.c_size_t, _vp]),
    "apap_image_warp_bounds": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, _f64p, _i32p]),
    "apap_image_warp_workspace_bytes": (C.c_size_t, [C.c_int]),
    "apap_image_warp": (C.c_int, [_vp, _u8p, C.c_int, C.c_int, _u8p, C.c_int, C.c_int, _f64p, C.c_int, C.c_int, C.c_int, C.c_int,
                                  C.c_int, _u8p, C.c_int]),
    "apap_image_warp_device": (C.c_int, [_vp, _vp, C.c_int, C.c_int, _vp, C.c_int, C.c_int, _f64p, C.c_int, C.c_int, C.c_int, C.c_int,
                                         C.c_int, _vp, _vp, C.c_size_t, _vp, _vp]),
    "apap_image_warp_batch": (C.c_int, [_vp, C.POINTER(C.c_void_p), _i32p, _i32p, C.POINTER(C.c_void_p), _i32p, _i32p, _f64p, _i32p,
                                        _i32p, _i32p, _i32p, _i32p, C.c_int, _u8p, _i64p, C.c_int]),
    "apap_image_warp_batch_device": (C.c_int, [_vp, C.POINTER(C.c_void_p), _i32p, _i32p, C.POINTER(C.c_void_p), _i32p, _i32p, _f64p,
                                               _i32p, _i32p, _i32p, _i32p, _i32p, C.c_int, _vp, _i64p, _vp, C.c_size_t, _vp, _vp]),
    "apap_panorama_bounds": (C.c_int, [C.c_int, C.c_int, _i32p, _i32p, _i32p, _i32p, C.c_int, _i32p]),
    "apap_panorama_workspace_bytes": (C.c_size_t, [_i32p, _i32p, _i32p, _i32p, C.c_int]),
    "apap_panorama_mean_of": (C.c_uint, [C.c_uint, C.c_uint]),
    "apap_panorama": (C.c_int, [_vp, _u8p, C.c_int, C.c_int, C.POINTER(C.c_void_p), _i32p, _i32p, C.POINTER(C.c_void_p), _i32p, _i32p,
                                C.POINTER(C.c_void_p), _i32p, C.POINTER(C.c_void_p), _i32p, _i32p, _i32p, _i32p, _i32p, C.c_int, C.c_int,
                                _u8p, _i32p, C.c_int]),
    "apap_panorama_device": (C.c_int, [_vp, _vp, C.c_int, C.c_int, C.POINTER(C.c_void_p), _i32p, _i32p, C.POINTER(C.c_void_p), _i32p,
                                       _i32p, C.POINTER(C.c_void_p), _i32p, C.POINTER(C.c_void_p), _i32p, _i32p, _i32p, _i32p, _i32p,
                                       C.c_int, C.c_int, _vp, _vp, C.c_size_t, _vp, _vp]),
    "apap_panorama_ramp_weight": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "apap_panorama_ramp_quotients": (None, [C.POINTER(C.c_uint), C.POINTER(C.c_uint), C.c_int, C.POINTER(C.c_uint)]),
}
# the ramp's entry points: the argument lists of apap_panorama / apap_panorama_device with `ramp` in place of `mode`
SIGNATURES["apap_panorama_ramp"] = SIGNATURES["apap_panorama"]
SIGNATURES["apap_panorama_ramp_device"] = SIGNATURES["apap_panorama_device"]
# gain compensation: the geometry arguments of apap_panorama (up to n_layers) / apap_panorama_device, then each entry point's own
_u64p = C.POINTER(C.c_ulonglong)
_PANO_GEOMETRY = SIGNATURES["apap_panorama"][1][:19]
_PANO_GEOMETRY_DEVICE = SIGNATURES["apap_panorama_device"][1][:19]
SIGNATURES.update({
    "apap_panorama_gain_solve": (C.c_int, [_u64p, _u64p, C.c_int, C.c_double, C.c_double, _f64p, _i32p, _i32p]),
    "apap_panorama_gain_apply": (C.c_int, [_u8p, C.c_int, C.c_int, _u8p]),
    "apap_panorama_gain_stats": (C.c_int, _PANO_GEOMETRY + [C.c_int, _u64p, _u64p, _i32p, C.c_int]),
    "apap_panorama_gain_stats_device": (C.c_int, _PANO_GEOMETRY_DEVICE + [C.c_int, _vp, _vp, _vp, C.c_size_t, _vp, _vp]),
    "apap_panorama_gain": (C.c_int, _PANO_GEOMETRY + [C.c_int, C.c_int, _i32p, _u8p, _i32p, C.c_int]),
    "apap_panorama_gain_device": (C.c_int, _PANO_GEOMETRY_DEVICE + [C.c_int, C.c_int, _i32p, _vp, _vp, C.c_size_t, _vp, _vp]),
    "apap_panorama_auto_gain": (C.c_int, _PANO_GEOMETRY + [C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, _u8p, _u64p, _u64p, _f64p,
                                                           _i32p, _i32p, _i32p, C.c_int]),
    "apap_panorama_auto_gain_device": (C.c_int, _PANO_GEOMETRY_DEVICE + [C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, _vp, _vp, _vp,
                                                                         _vp, _vp, _vp, _vp, C.c_size_t, _vp, _vp]),
})
# the two-band blend: the geometry arguments, then ramp, band, gain_q (host ints or NULL) and the ramp entry points' tails
SIGNATURES.update({
    "apap_box_blur": (C.c_int, [_vp, _u8p, C.c_int, C.c_int, C.c_int, _u8p, C.c_int]),
    "apap_box_blur_device": (C.c_int, [_vp, _vp, C.c_int, C.c_int, C.c_int, _vp, _vp]),
    "apap_panorama_band_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int, _i32p, _i32p, _i32p, _i32p, _i32p, _i32p, C.c_int, C.c_int]),
    "apap_panorama_band": (C.c_int, _PANO_GEOMETRY + [C.c_int, C.c_int, _i32p, _u8p, _i32p, C.c_int]),
    "apap_panorama_band_device": (C.c_int, _PANO_GEOMETRY_DEVICE + [C.c_int, C.c_int, _i32p, _vp, _vp, C.c_size_t, _vp, _vp]),
})
# the fundamental matrix: the argument lists of apap_find_homography_ransac / apap_ransac_device; the batch forms put the pair
# table (host ints) and the number of pairs where those have n
SIGNATURES.update({
    "apap_find_fundamental_ransac": SIGNATURES["apap_find_homography_ransac"],
    "apap_find_fundamental_ransac_batch": (C.c_int, [_vp, _f32p, _f32p, _i32p, C.c_int, C.c_double, C.c_int, C.c_ulonglong, _f64p,
                                                     _u8p, _i32p, C.c_int]),
    "apap_fundamental_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "apap_fundamental_device": SIGNATURES["apap_ransac_device"],
    "apap_fundamental_batch_device": (C.c_int, [_vp, _vp, _vp, _i32p, C.c_int, C.c_double, C.c_int, C.c_ulonglong, _vp, _vp, _vp,
                                                _vp, C.c_size_t, _vp]),
})

# notch denoising (apap_denoise.hip)
SIGNATURES.update({
    "apap_fft_twiddles": (C.c_int, [C.c_int, _f64p]),
    "apap_fft2": (C.c_int, [_vp, _f64p, _f64p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "apap_fft2_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "apap_fft2_device": (C.c_int, [_vp, _vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int, _vp, C.c_size_t, _vp]),
    "apap_notch_spectrum": (C.c_int, [_vp, _f64p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "apap_notch_spectrum_device": (C.c_int, [_vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _vp]),
    "apap_notch_denoise": (C.c_int, [_vp, _u8p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _vp,
                                     C.c_int]),
    "apap_notch_denoise_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "apap_notch_denoise_device": (C.c_int, [_vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                            _vp, _vp, C.c_size_t, _vp]),
})

# co-visibility tracks and triangulation (apap_sfm.hip)
SIGNATURES.update({
    "apap_covis_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "apap_covis_tracks": (C.c_int, [_vp, _f32p, _i32p, _i32p, C.c_int, C.c_float, _i32p, _f32p, _i32p, _i32p, C.c_int]),
    "apap_covis_tracks_device": (C.c_int, [_vp, _vp, _vp, _i32p, C.c_int, C.c_float, _vp, _vp, _vp, _vp, _vp, _vp, C.c_size_t, _vp]),
    "apap_triangulate_rays": (C.c_int, [_vp, _f64p, _f64p, _i32p, C.c_int, _f64p, _f64p, _i32p, C.c_int]),
    "apap_triangulate_rays_device": (C.c_int, [_vp, _vp, _vp, _vp, C.c_int, C.c_int, _vp, _vp, _vp, _vp]),
    "apap_triangulate_tracks": (C.c_int, [_vp, _i32p, _f32p, C.c_int, C.c_int, _f32p, _i32p, _f64p, _f64p, _f64p, C.c_int, C.c_int,
                                          _i32p, C.c_int, _f64p, _f64p, _i32p, C.c_int]),
    "apap_triangulate_tracks_device": (C.c_int, [_vp, _vp, _vp, _vp, C.c_int, C.c_int, _vp, _i32p, _vp, _vp, _vp, C.c_int, C.c_int,
                                                 _i32p, C.c_int, _vp, _vp, _vp, _vp]),
})

# dark-channel dehazing (apap_dehaze.hip)
_u16p = C.POINTER(C.c_uint16)
SIGNATURES.update({
    "apap_dehaze_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "apap_dark_channel": (C.c_int, [_vp, _u8p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _u8p, C.c_int]),
    "apap_dark_channel_device": (C.c_int, [_vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _vp, _vp, C.c_size_t, _vp]),
    "apap_atmospheric_light": (C.c_int, [_vp, _u8p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _u8p, C.c_int]),
    "apap_atmospheric_light_device": (C.c_int, [_vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _vp, _vp, C.c_size_t, _vp]),
    "apap_transmission": (C.c_int, [_vp, _u8p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _u16p, C.c_int]),
    "apap_transmission_device": (C.c_int, [_vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _vp, _vp,
                                           C.c_size_t, _vp]),
    "apap_dehaze": (C.c_int, [_vp, _u8p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _u8p, _u16p, _u8p,
                              C.c_int]),
    "apap_dehaze_device": (C.c_int, [_vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _vp, _vp, _vp,
                                     _vp, C.c_size_t, _vp]),
})

# the image pyramid and its pack (apap_pyramid.hip)
_PTRS = C.POINTER(C.c_void_p)
SIGNATURES.update({
    "apap_pyramid_layout": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, _i32p, _i32p, _i64p, _i32p, _i32p]),
    "apap_pyramid_level_caps": (C.c_int, [C.c_int, C.c_int, C.c_int, _i32p]),
    "apap_pyramid_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "apap_pyramid_build": (C.c_int, [_vp, _u8p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _u8p, C.c_int]),
    "apap_pyramid_build_device": (C.c_int, [_vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _vp, C.c_size_t, _vp, C.c_size_t, _vp]),
    "apap_pyramid_build_batch": (C.c_int, [_vp, _PTRS, _i32p, _i32p, _i32p, C.c_int, C.c_int, C.c_int, _u8p, C.c_int]),
    "apap_pyramid_build_batch_device": (C.c_int, [_vp, _PTRS, _i32p, _i32p, _i32p, C.c_int, C.c_int, C.c_int, _vp, C.c_size_t, _vp,
                                                  C.c_size_t, _vp]),
    "apap_pyramid_keypoints_workspace_bytes": (C.c_size_t, [C.c_int]),
    "apap_pyramid_keypoints": (C.c_int, [_vp, _f32p, _i64p, C.c_int, _i32p, _i32p, _i32p, _i32p, C.c_int, _f32p, _f32p, _i32p, _i64p,
                                         _i32p, C.c_int]),
    "apap_pyramid_keypoints_device": (C.c_int, [_vp, _vp, _vp, C.c_int, _i32p, _i32p, _i32p, _i32p, C.c_int, _vp, _vp, _vp, _vp, _i32p,
                                                _vp, C.c_size_t, _vp]),
})

_lib = None
_torch_at_load = False     # was torch in the process when the library was loaded?  (cvx_proj_amd.resident refuses otherwise)


def lib():
    """Load the shared library once.  Raises ApapError (never falls back) if absent."""
    global _lib, _torch_at_load
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ApapError(ERR_NO_DEVICE, f"{LIB_PATH} not built; run `python -c 'import __graft_entry__ as g; "
                                           "g.build()'` or `make -C cvx_proj_amd/csrc`")
        # One HIP runtime per process.  PyTorch-ROCm bundles its own libamdhip64.so (same SONAME as /opt/rocm's, different
        # file).  When torch is ALREADY imported its copy is in the process and this library binds to it; otherwise the RPATH
        # to /opt/rocm/lib is used and NO torch is imported on the library's behalf (2.3 s against 0.4 s of start-up for a
        # command that needs none: python -m cvx_proj_amd.apap).  The rule for a process that uses both: import torch BEFORE
        # the first call into this module (a later `import torch` would find /opt/rocm's runtime under its own SONAME and see
        # no GPU).  Whether it was kept is recorded here; cvx_proj_amd.resident, the one module through which the package uses
        # torch (pipeline and dist import it), refuses to load in a process that broke it.  APAP_HIP_PRELOAD_TORCH=1 restores
        # the old behaviour (torch imported here first, if it is installed).
        if "torch" not in sys.modules and os.environ.get("APAP_HIP_PRELOAD_TORCH", "0") == "1":
            try:
                import torch  # noqa: F401
            except ImportError:
                pass
        _torch_at_load = "torch" in sys.modules
        handle = C.CDLL(LIB_PATH)
        # a build of another ABI generation keeps the symbol names but not the argument lists: refuse it
        got = handle.apap_abi_version() if hasattr(handle, "apap_abi_version") else 1
        if got != ABI_VERSION:
            raise ApapError(ERR_INVALID_ARG, f"{LIB_PATH} is ABI generation {got}, this binding needs {ABI_VERSION}: rebuild "
                                             "it (make -C cvx_proj_amd/csrc)")
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(handle, name)
            fn.restype = res
            fn.argtypes = args
        _lib = handle
    return _lib


def check(code):
    if code != OK:
        raise _ERROR_CLASSES.get(code, ApapError)(code, lib().apap_last_error().decode("utf-8", "replace"))


class Context:
    """``apap_ctx`` of include/apap_hip.h: solver options, per-kernel profiling and the pool of
    device buffers that host-buffer calls reuse.  The library has no process-wide mutable state;
    pass a context as ``ctx=`` to any wrapper below (``None`` = built-in defaults).  Not to be
    shared between threads; use one per thread."""

    def __init__(self, **options):
        self._h = lib().apap_ctx_create()
        if not self._h:
            raise ApapError(ERR_HIP, "apap_ctx_create failed")
        for k, v in options.items():
            self.set(k, v)

    _NAMES = {"variant": OPT_SOLVER_VARIANT, "eigen": OPT_EIGEN_SOLVER, "careful": OPT_CAREFUL, "profile": OPT_PROFILE,
              "want_waves": OPT_WANT_WAVES, "warp_rows": OPT_WARP_ROWS, "weight_chunk_kb": OPT_WEIGHT_CHUNK_KB,
              "fused_max_cells": OPT_FUSED_MAX_CELLS, "warp_fast": OPT_WARP_FAST, "overlap_pcie": OPT_OVERLAP_PCIE,
              "plan_cells": OPT_PLAN_CELLS, "moments": OPT_MOMENTS, "weights_f32": OPT_WEIGHTS_F32,
              "plan_slots": OPT_PLAN_SLOTS, "warp_sampling": OPT_WARP_SAMPLING}

    def set(self, name, value):
        if name == "short_chain":       # a switch of the context beside the option table (apap_ctx_set_short_chain)
            check(lib().apap_ctx_set_short_chain(self._h, int(value)))
        else:
            check(lib().apap_ctx_set_option(self._h, self._NAMES[name], int(value)))
        return self

    def get(self, name):
        v = C.c_int(0)
        if name == "short_chain":
            check(lib().apap_ctx_get_short_chain(self._h, C.byref(v)))
        else:
            check(lib().apap_ctx_get_option(self._h, self._NAMES[name], C.byref(v)))
        return v.value

    def profile_k1_chunks(self):
        """``(chunks K1 ran on the short weight chain, chunks K1 ran)`` in the profiled launches since the previous read."""
        short, every = C.c_uint(0), C.c_uint(0)
        check(lib().apap_ctx_profile_k1_chunks(self._h, C.byref(short), C.byref(every)))
        return short.value, every.value

    def profile_read(self):
        """``{kernel slot name: (milliseconds, launches)}`` since the previous read."""
        ms = (C.c_float * PROF_SLOTS)()
        cnt = (C.c_int * PROF_SLOTS)()
        check(lib().apap_ctx_profile_read(self._h, ms, cnt))
        return {k: (ms[i], cnt[i]) for i, k in enumerate(PROF_NAMES)}

    @property
    def handle(self):
        return self._h

    def close(self):
        if self._h:
            lib().apap_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:      # noqa: BLE001  (interpreter shutdown)
            pass


def _h(ctx):
    """ctypes handle of ``ctx`` (a Context, a raw handle, or None)."""
    if ctx is None:
        return None
    return C.c_void_p(ctx.handle if isinstance(ctx, Context) else ctx)


def last_error():
    return lib().apap_last_error().decode("utf-8", "replace")


def sampling_value(sampling, who="local_warp"):
    """The ``OPT_WARP_SAMPLING`` value of a ``sampling=`` keyword: ``None`` (whatever the context says) -> ``None``,
    ``"nearest"`` / ``"bilinear"`` -> 0 / 1, anything else a ValueError - raised before any device is touched."""
    if sampling is None:
        return None
    if not isinstance(sampling, str) or sampling not in SAMPLINGS:
        raise ValueError(f"{who}: sampling must be None, 'nearest' or 'bilinear'; got {sampling!r}")
    return SAMPLINGS[sampling]


class sampling_scope:
    """``with sampling_scope(ctx, sampling, who) as c:`` - the context to pass to the native call.  ``sampling=None``: ``ctx``
    itself, untouched.  A string: ``ctx`` (a fresh context when ``ctx`` is None) with ``OPT_WARP_SAMPLING`` set for the body
    and put back to what it was found at on the way out."""

    def __init__(self, ctx, sampling, who="local_warp"):
        self._value = sampling_value(sampling, who)
        self._ctx, self._own, self._before = ctx, None, None

    def __enter__(self):
        if self._value is None:
            return self._ctx
        if self._ctx is None:
            self._own = self._ctx = Context()
        before = C.c_int(0)
        check(lib().apap_ctx_get_option(_h(self._ctx), OPT_WARP_SAMPLING, C.byref(before)))
        self._before = before.value
        check(lib().apap_ctx_set_option(_h(self._ctx), OPT_WARP_SAMPLING, self._value))
        return self._ctx

    def __exit__(self, *exc):
        if self._before is not None:
            lib().apap_ctx_set_option(_h(self._ctx), OPT_WARP_SAMPLING, self._before)
        if self._own is not None:
            self._own.close()
        return False


def _ptr(a, ctype):
    return a.ctypes.data_as(C.POINTER(ctype)) if a is not None else None


def as_f32(a, shape_tail=None):
    a = np.ascontiguousarray(a, dtype=np.float32)
    if shape_tail is not None and tuple(a.shape[-len(shape_tail):]) != tuple(shape_tail):
        raise ValueError(f"expected trailing shape {shape_tail}, got {a.shape}")
    return a


def as_points(a):
    """Keypoints in the dtype the reference would compute with: float32 stays float32 (what utils.get_features returns);
    float64 and integer arrays are taken as float64 (numpy's own reductions promote integers to float64; nothing in
    apap.py:35-100 casts its argument) - both pinned bit for bit by tests/golden/f64pts_ref.npz.  Any OTHER dtype (float16,
    longdouble, bool, ...) is widened to float64 as well, which is NOT what numpy does with it in the reference (a float16
    set mixes with the float32 padding to float32 there): accepted, but without the bit-compatibility claim.
    Returns (contiguous (n, 2) array, is_float64)."""
    a = np.asarray(a)
    a = np.ascontiguousarray(a, dtype=np.float32 if a.dtype == np.float32 else np.float64)
    if a.shape[-1:] != (2,):
        raise ValueError(f"expected trailing shape (2,), got {a.shape}")
    return a, int(a.dtype == np.float64)


def _vptr(a):
    return a.ctypes.data_as(C.c_void_p)


def _ip(a):      # int * of an int32 array
    return a.ctypes.data_as(_i32p)


def _dp(a):      # double * of a float64 array
    return a.ctypes.data_as(_f64p)


def _addrs(addresses):
    """A C array of the listed addresses (``ndarray.ctypes.data``, ``Tensor.data_ptr()``): a ``T *const *`` argument."""
    return (C.c_void_p * len(addresses))(*addresses)


def _i32(values):      # a new contiguous int32 array
    return np.array(values, dtype=np.int32)


def _offsets(lengths, name, one, many, rows, max_count, max_rows):
    """Counts -> int32 offsets (len + 1), checked as the library checks them: 1 .. ``max_count`` counts (``many``, say "pairs"),
    each (``one``: "a pair") of 1 .. ``max_rows`` ``rows``, a power of two, and their sum within int32."""
    lengths = [int(x) for x in lengths]
    if not 1 <= len(lengths) <= max_count:
        raise ValueError(f"{name}: {len(lengths)} {many} (1 .. {max_count})")
    if any(not 1 <= x <= max_rows for x in lengths):
        raise ValueError(f"{name}: {one} holds 1 .. 2^{max_rows.bit_length() - 1} {rows}; got {lengths}")
    if sum(lengths) > np.iinfo(np.int32).max:
        raise ValueError(f"{name}: {sum(lengths)} {rows} in all exceed the int32 offsets")
    off = np.zeros(len(lengths) + 1, np.int32)
    off[1:] = np.cumsum(lengths)
    return off


def _image_table(got):
    """``(array, channels)`` per image -> the batch entry points' (addresses, heights, widths, channels)."""
    return (_addrs([a.ctypes.data for a, _ in got]), _i32([a.shape[0] for a, _ in got]), _i32([a.shape[1] for a, _ in got]),
            _i32([c for _, c in got]))


# ------------------------------------------------------------------ host-only helpers
def host_prepare(src, dst):
    """C restatement of the set-up in apap.py:132-140,165-166, in the dtype of each keypoint set.  Returns a dict: N1 N2 C1 C2
    iC2 iN2 (3x3 float32) and nf1 nf2 cf1 cf2 (n x 2; float32 for a float32 set, float64 for a float64 one)."""
    src, s64 = as_points(src)
    dst, d64 = as_points(dst)
    if src.shape != dst.shape or src.ndim != 2:
        raise ValueError(f"src/dst must both be (n, 2); got {src.shape} and {dst.shape}")
    n = src.shape[0]
    out = {k: np.empty((3, 3), np.float32) for k in ("N1", "N2", "C1", "C2", "iC2", "iN2")}
    if not s64 and not d64:
        out.update({k: np.empty((n, 2), np.float32) for k in ("nf1", "nf2", "cf1", "cf2")})
        check(lib().apap_host_prepare(_ptr(src, C.c_float), _ptr(dst, C.c_float), n,
                                      *[_ptr(out[k], C.c_float) for k in
                                        ("N1", "N2", "C1", "C2", "iC2", "iN2", "nf1", "nf2", "cf1", "cf2")]))
        return out
    wide = {k: np.empty((n, 2), np.float64) for k in ("nf1", "nf2", "cf1", "cf2")}
    check(lib().apap_host_prepare_pts(_vptr(src), s64, _vptr(dst), d64, n,
                                      *[_ptr(out[k], C.c_float) for k in ("N1", "N2", "C1", "C2", "iC2", "iN2")],
                                      *[_ptr(wide[k], C.c_double) for k in ("nf1", "nf2", "cf1", "cf2")]))
    for k, is64 in (("nf1", s64), ("cf1", s64), ("nf2", d64), ("cf2", d64)):
        out[k] = wide[k] if is64 else wide[k].astype(np.float32)        # exact: the values ARE float32
    return out


def host_dlt_rows(cf1, cf2):
    """APAP.matrix_generate (apap.py:103-119): float32 rows; a float64 operand makes the products float64 products rounded
    once on the store, two float32 operands float32 products."""
    cf1, a64 = as_points(cf1)
    cf2, b64 = as_points(cf2)
    n = cf1.shape[0]
    aa = np.empty((2 * n, 9), np.float32)
    if not a64 and not b64:
        check(lib().apap_host_dlt_rows(_ptr(cf1, C.c_float), _ptr(cf2, C.c_float), n, _ptr(aa, C.c_float)))
    else:
        cf1, cf2 = np.ascontiguousarray(cf1, np.float64), np.ascontiguousarray(cf2, np.float64)
        check(lib().apap_host_dlt_rows_pts(_ptr(cf1, C.c_double), _ptr(cf2, C.c_double), n, 1, _ptr(aa, C.c_float)))
    return aa


def _out_f64(out, shape):
    """``out`` as the function's result buffer (e.g. page-locked staging memory of the caller's), or a fresh array."""
    if out is None:
        return np.empty(shape, np.float64)
    if not (isinstance(out, np.ndarray) and out.dtype == np.float64 and out.shape == tuple(shape) and out.flags.c_contiguous):
        raise ValueError(f"out must be a contiguous float64 array of shape {tuple(shape)}")
    return out


def host_build_table(src, cf1, cf2, out=None, moments=30):
    """The device keypoint table of ``apap_solve_device`` and its batch forms.  ``moments`` = 30 (default): the 30 distinct
    entries of ``r1 r1^T + r2 r2^T`` of the reference's float32 DLT rows; 24: the exact-product table of a context with
    ``moments=24`` (``apap_host_build_table24``; pass ``ctx.get("moments")``)."""
    src, s64 = as_points(src)
    cf1, a64 = as_points(cf1)
    cf2, b64 = as_points(cf2)
    n = src.shape[0]
    table = _out_f64(out, (n, TABLE_STRIDE))
    if moments not in (24, 30):
        raise ValueError(f"moments must be 30 or 24, got {moments}")
    if moments == 30 and not (s64 or a64 or b64):
        check(lib().apap_host_build_table(_ptr(src, C.c_float), _ptr(cf1, C.c_float), _ptr(cf2, C.c_float), n,
                                          _ptr(table, C.c_double)))
    else:       # from the DLT rows themselves and the source keypoints as float64
        aa = host_dlt_rows(cf1, cf2)
        src = np.ascontiguousarray(src, np.float64)
        build = lib().apap_host_build_table24 if moments == 24 else lib().apap_host_build_table_rows
        check(build(_ptr(src, C.c_double), _ptr(aa, C.c_float), n, _ptr(table, C.c_double)))
    return table


def host_build_denorm(iC2, C1, iN2, N1, out=None):
    mats = [as_f32(m, (3, 3)) for m in (iC2, C1, iN2, N1)]
    out = _out_f64(out, (DENORM_DOUBLES,))
    check(lib().apap_host_build_denorm(*[_ptr(m, C.c_float) for m in mats], _ptr(out, C.c_double)))
    return out


# ---------------------------------------------------------------- host-buffer compute
def local_homography(src, dst, vertices, gamma, sigma, want_weights=True, device=-1, ctx=None):
    src, s64 = as_points(src)
    dst, d64 = as_points(dst)
    if src.ndim != 2 or src.shape != dst.shape:
        raise ValueError(f"src/dst must both be (n, 2); got {src.shape} and {dst.shape}")
    vertices = np.ascontiguousarray(vertices, dtype=np.float64)
    rows, cols, two = vertices.shape      # ValueError on a wrong rank, like apap.py:130
    if two != 2:
        raise ValueError(f"vertices must be (rows, cols, 2); got {vertices.shape}")
    n = src.shape[0]
    H = np.empty((rows, cols, 3, 3), np.float32)
    W = np.empty((rows, cols, n), np.float64) if want_weights else None
    check(lib().apap_local_homography_pts(_h(ctx), _vptr(src), s64, _vptr(dst), d64, n, _ptr(vertices, C.c_double),
                                          rows, cols, float(gamma), float(sigma), _ptr(H, C.c_float),
                                          _ptr(W, C.c_double), device))
    return H, W


def local_weights(src, points, gamma, sigma, device=-1, ctx=None):
    """``max(exp(-|p - s| / sigma^2), gamma)`` for every (sample point p, keypoint s): ``points`` (..., 2) float64
    -> (..., n) float64.  The weights of reference apap.py:150-153 for any subset of the mesh."""
    src, s64 = as_points(src)
    pts = np.ascontiguousarray(points, dtype=np.float64)
    if pts.shape[-1:] != (2,):
        raise ValueError(f"points must be (..., 2); got {pts.shape}")
    n, cells = src.shape[0], pts.size // 2
    W = np.empty(pts.shape[:-1] + (n,), np.float64)
    if cells:
        check(lib().apap_local_weights_pts(_h(ctx), _vptr(src), s64, n, _ptr(pts, C.c_double), cells, float(gamma),
                                           float(sigma), _ptr(W, C.c_double), device))
    return W


def local_warp(img, H, mesh_w, mesh_h, final_w, final_h, off_x, off_y, want_inverse=True, device=-1, ctx=None, out=None,
               sampling=None):
    """``out``: the caller's own (final_h, final_w, 3) uint8 canvas (e.g. page-locked memory, which the library then neither
    registers nor stages) instead of a fresh array.  ``sampling``: ``None`` (the context's ``warp_sampling``), ``"nearest"`` or
    ``"bilinear"`` for this call only."""
    with sampling_scope(ctx, sampling, "local_warp") as ctx:
        return _local_warp(img, H, mesh_w, mesh_h, final_w, final_h, off_x, off_y, want_inverse, device, ctx, out)


def _local_warp(img, H, mesh_w, mesh_h, final_w, final_h, off_x, off_y, want_inverse, device, ctx, out):
    img = np.ascontiguousarray(img, dtype=np.uint8)
    img_h, img_w, ch = img.shape
    if ch != 3:
        raise ValueError(f"image must be (h, w, 3); got {img.shape}")
    mesh_w = np.ascontiguousarray(mesh_w, dtype=np.float64)
    mesh_h = np.ascontiguousarray(mesh_h, dtype=np.float64)
    if out is None:
        out = np.empty((final_h, final_w, 3), np.uint8)
    elif not (isinstance(out, np.ndarray) and out.shape == (final_h, final_w, 3) and out.dtype == np.uint8 and out.flags.c_contiguous):
        raise ValueError(f"out must be a contiguous uint8 array of shape {(final_h, final_w, 3)}")
    if isinstance(H, np.ndarray) and H.dtype == np.float64:
        # the reference inverts and multiplies in the grid's own dtype (apap.py:201-203,210-213): a
        # float64 grid is not rounded to float32 on the way
        H = np.ascontiguousarray(H)
        if H.shape[-2:] != (3, 3):
            raise ValueError(f"expected trailing shape (3, 3), got {H.shape}")
        rows, cols = H.shape[:2]
        Hinv = np.empty_like(H) if want_inverse else None
        check(lib().apap_local_warp_f64(_h(ctx), _ptr(img, C.c_uint8), img_h, img_w, _ptr(H, C.c_double), rows, cols,
                                        _ptr(mesh_w, C.c_double), mesh_w.size, _ptr(mesh_h, C.c_double), mesh_h.size,
                                        int(final_w), int(final_h), int(off_x), int(off_y), _ptr(out, C.c_uint8),
                                        _ptr(Hinv, C.c_double), device))
        return out, Hinv
    H = as_f32(H, (3, 3))
    rows, cols = H.shape[:2]
    Hinv = np.empty_like(H) if want_inverse else None
    check(lib().apap_local_warp(_h(ctx), _ptr(img, C.c_uint8), img_h, img_w, _ptr(H, C.c_float), rows, cols,
                                _ptr(mesh_w, C.c_double), mesh_w.size, _ptr(mesh_h, C.c_double), mesh_h.size,
                                int(final_w), int(final_h), int(off_x), int(off_y), _ptr(out, C.c_uint8),
                                _ptr(Hinv, C.c_float), device))
    return out, Hinv


def local_stitch(img, center, H, mesh_w, mesh_h, final_w, final_h, off_x, off_y, want_inverse=False, device=-1, ctx=None,
                 sampling=None):
    """Fused local_warp + paste of ``center`` at the offsets + uniform_blend.  ``sampling``: as in :func:`local_warp`."""
    with sampling_scope(ctx, sampling, "local_stitch") as ctx:
        return _local_stitch(img, center, H, mesh_w, mesh_h, final_w, final_h, off_x, off_y, want_inverse, device, ctx)


def _local_stitch(img, center, H, mesh_w, mesh_h, final_w, final_h, off_x, off_y, want_inverse, device, ctx):
    img = np.ascontiguousarray(img, dtype=np.uint8)
    center = np.ascontiguousarray(center, dtype=np.uint8)
    if img.ndim != 3 or img.shape[2] != 3 or center.ndim != 3 or center.shape[2] != 3:
        raise ValueError(f"images must be (h, w, 3); got {img.shape} and {center.shape}")
    H = as_f32(H, (3, 3))
    rows, cols = H.shape[:2]
    mesh_w = np.ascontiguousarray(mesh_w, dtype=np.float64)
    mesh_h = np.ascontiguousarray(mesh_h, dtype=np.float64)
    out = np.empty((final_h, final_w, 3), np.uint8)
    Hinv = np.empty_like(H) if want_inverse else None
    check(lib().apap_local_stitch(_h(ctx), _ptr(img, C.c_uint8), img.shape[0], img.shape[1], _ptr(center, C.c_uint8),
                                  center.shape[0], center.shape[1], _ptr(H, C.c_float), rows, cols,
                                  _ptr(mesh_w, C.c_double), mesh_w.size, _ptr(mesh_h, C.c_double), mesh_h.size,
                                  int(final_w), int(final_h), int(off_x), int(off_y), _ptr(out, C.c_uint8),
                                  _ptr(Hinv, C.c_float), device))
    return out, Hinv


def warp_coords(H, mesh_w, mesh_h, final_w, final_h, off_x, off_y, device=-1, ctx=None):
    H = as_f32(H, (3, 3))
    rows, cols = H.shape[:2]
    mesh_w = np.ascontiguousarray(mesh_w, dtype=np.float64)
    mesh_h = np.ascontiguousarray(mesh_h, dtype=np.float64)
    coords = np.empty((final_h, final_w, 2), np.float64)
    check(lib().apap_warp_coords(_h(ctx), _ptr(H, C.c_float), rows, cols, _ptr(mesh_w, C.c_double), mesh_w.size,
                                 _ptr(mesh_h, C.c_double), mesh_h.size, int(final_w), int(final_h), int(off_x),
                                 int(off_y), _ptr(coords, C.c_double), device))
    return coords


def invert_normalize_flatten(H, device=-1, ctx=None):
    H = as_f32(H, (3, 3))
    cells = H.size // 9
    out = np.empty((cells, 9), np.float64)
    check(lib().apap_invert_normalize_flatten(_h(ctx), _ptr(H, C.c_float), cells, _ptr(out, C.c_double), device))
    return out


def uniform_blend(img1, img2, device=-1, ctx=None):
    a = np.ascontiguousarray(img1, dtype=np.uint8)
    b = np.ascontiguousarray(img2, dtype=np.uint8)
    if a.shape != b.shape or a.ndim != 3 or a.shape[2] != 3:
        raise ValueError(f"images must share shape (h, w, 3); got {a.shape} and {b.shape}")
    out = np.empty_like(a)
    check(lib().apap_uniform_blend(_h(ctx), _ptr(a, C.c_uint8), _ptr(b, C.c_uint8), a.shape[0], a.shape[1],
                                   _ptr(out, C.c_uint8), device))
    return out


def equalize_hist(img, device=-1, ctx=None):
    """Per-channel ``cv.equalizeHist`` of an (h, w) or (h, w, c) uint8 image, c <= 4."""
    a = np.ascontiguousarray(img, dtype=np.uint8)
    if a.ndim not in (2, 3) or (a.ndim == 3 and not 1 <= a.shape[2] <= 4) or a.size == 0:
        raise ValueError(f"image must be (h, w) or (h, w, 1..4) uint8 and non-empty; got {a.shape}")
    channels = 1 if a.ndim == 2 else a.shape[2]
    out = np.empty_like(a)
    check(lib().apap_equalize_hist(_h(ctx), _ptr(a, C.c_uint8), a.shape[0], a.shape[1], channels, _ptr(out, C.c_uint8), device))
    return out


FFT_MIN_LENGTH, FFT_MAX_LENGTH = 2, 4096     # APAP_FFT_MIN_LENGTH, APAP_FFT_MAX_LENGTH
NOTCH_MAX_R = 6                              # APAP_NOTCH_MAX_R
DENOISE_OUT = {"float64": 0, "uint8": 1}     # APAP_DENOISE_OUT_F64, APAP_DENOISE_OUT_U8
DENOISE_MAX_PLANES = 65535


def fft_twiddles(n):
    """``apap_fft_twiddles``: (n, 2) float64, cos and sin of -2 pi k / n - the table the kernels read.  Needs no device."""
    n = int(n)
    if n < 1:
        raise ValueError(f"fft_twiddles: n={n}")
    out = np.empty((n, 2), dtype=np.float64)
    check(lib().apap_fft_twiddles(n, _ptr(out, C.c_double)))
    return out


def _spectra(x, who):
    """``x`` as contiguous complex128 (planes, h, w), and whether it came as one plane."""
    a = np.array(x, dtype=np.complex128, order="C")     # a copy: the in-place entry points may write it
    if a.ndim not in (2, 3) or a.size == 0:
        raise ValueError(f"{who}: a (h, w) or (planes, h, w) complex array expected; got {a.shape}")
    return (a[None] if a.ndim == 2 else a), a.ndim == 2


def fft2(x, inverse=False, device=-1, ctx=None):
    """``apap_fft2``: the engine's 2-D transform of one (h, w) or several (planes, h, w) complex128 planes; lengths 5-smooth,
    2 .. 4096.  The inverse is scaled by 1 / (h w)."""
    a, one = _spectra(x, "fft2")
    out = np.empty_like(a)
    check(lib().apap_fft2(_h(ctx), _ptr(a.view(np.float64), C.c_double), _ptr(out.view(np.float64), C.c_double), a.shape[0], a.shape[1],
                          a.shape[2], 1 if inverse else 0, device))
    return out[0] if one else out


def notch_spectrum(f, spacing=48, r=5, sn=9, device=-1, ctx=None):
    """``apap_notch_spectrum``: the notch schedule on shifted spectra ((h, w) or (planes, h, w) complex); returns new arrays."""
    a, one = _spectra(f, "notch_spectrum")
    check(lib().apap_notch_spectrum(_h(ctx), _ptr(a.view(np.float64), C.c_double), a.shape[0], a.shape[1], a.shape[2], int(spacing),
                                    int(r), int(sn), device))
    return a[0] if one else a


def notch_denoise(imgs, spacing=48, r=5, sn=9, equalize=True, out="float64", device=-1, ctx=None):
    """``apap_notch_denoise``: uint8 pictures (n, h, w, c), c <= 4, all planes in one call; float64 or uint8 of that shape."""
    a = np.ascontiguousarray(imgs, dtype=np.uint8)
    if a.ndim != 4 or a.size == 0:
        raise ValueError(f"notch_denoise: (n, h, w, c) uint8 pictures expected; got {a.shape}")
    if out not in DENOISE_OUT:
        raise ValueError(f"notch_denoise: out={out!r} ('float64' or 'uint8')")
    res = np.empty(a.shape, dtype=np.float64 if out == "float64" else np.uint8)
    check(lib().apap_notch_denoise(_h(ctx), _ptr(a, C.c_uint8), a.shape[0], a.shape[1], a.shape[2], a.shape[3], 1 if equalize else 0,
                                   int(spacing), int(r), int(sn), DENOISE_OUT[out], res.ctypes.data_as(C.c_void_p), device))
    return res


COVIS_MAX_VIEWS = 8                     # APAP_COVIS_MAX_VIEWS
COVIS_MAX_POINTS = 65536                # APAP_COVIS_MAX_POINTS
COVIS_EPS = np.float32(0.1)             # has_affinity's 1e-1, as the float the kernels compare with
STATUS_COVIS_BOUND = 64                 # APAP_STATUS_COVIS_BOUND


def covis_arguments(views, eps, who):
    """The checks of the co-visibility entry points, made before the library (or a device) is touched: 1 .. 8 views, each
    ``(pts (n, 2), idx (n,))`` with n >= 0, at most 65 536 observations in all, ``eps`` finite and >= 0.  Returns (pts (N, 2)
    float32, idx (N,) int32, offsets (V + 1,) int32, eps as float32)."""
    views = list(views)
    if not 1 <= len(views) <= COVIS_MAX_VIEWS:
        raise ValueError(f"{who}: {len(views)} views (1 .. {COVIS_MAX_VIEWS})")
    pts, idx = [], []
    for v, view in enumerate(views):
        if len(view) != 2:
            raise ValueError(f"{who}: view {v} must be (pts (n, 2), idx (n,))")
        p, i = np.asarray(view[0]), np.asarray(view[1])
        if i.size and not np.issubdtype(i.dtype, np.integer):
            raise ValueError(f"{who}: view {v}: idx must be integers; got {i.dtype}")
        if p.size and not np.issubdtype(p.dtype, np.floating):
            raise ValueError(f"{who}: view {v}: pts must be floating point; got {p.dtype}")
        p = np.ascontiguousarray(p, dtype=np.float32).reshape(-1, 2) if p.size % 2 == 0 else None
        if p is None or i.ndim > 1 or len(p) != i.size:
            raise ValueError(f"{who}: view {v}: pts (n, 2) and idx (n,) expected; got {np.shape(view[0])} and {np.shape(view[1])}")
        if i.size and (i.min() < np.iinfo(np.int32).min or i.max() > np.iinfo(np.int32).max):
            raise ValueError(f"{who}: view {v}: idx exceeds int32")
        pts.append(p)
        idx.append(i.astype(np.int32).reshape(-1))
    n = sum(len(p) for p in pts)
    if n > COVIS_MAX_POINTS:
        raise ValueError(f"{who}: {n} observations in all (at most {COVIS_MAX_POINTS}: the first-candidate scan is quadratic)")
    e = np.float32(eps)
    if not (e >= 0 and np.isfinite(e)):
        raise ValueError(f"{who}: eps = {eps} (finite, >= 0)")
    off = np.zeros(len(views) + 1, np.int32)
    off[1:] = np.cumsum([len(p) for p in pts])
    return np.ascontiguousarray(np.concatenate(pts)), np.ascontiguousarray(np.concatenate(idx)), off, e


def covis_workspace_layout(n_points, n_views):
    """Byte offsets of the parts of the resident form's workspace (include/apap_hip.h): ``dict(offsets, first, owner, rank,
    total)``."""
    up = lambda b: (b + 255) // 256 * 256      # noqa: E731
    ints = max(n_points, 1) * 4
    out, at = {}, 0
    for name, b in (("offsets", (n_views + 1) * 4), ("first", ints), ("owner", ints), ("rank", ints)):
        out[name] = at
        at += up(b)
    out["total"] = at
    return out


def covis_tracks(views, eps=COVIS_EPS, device=-1, ctx=None):
    """``apap_covis_tracks``: the reference's ``get_covid`` over ``views`` = [(pts (n_v, 2) float32, idx (n_v,) int32), ...],
    view 0 first.  Returns (table (T, V) int32, track_pts (T, 2) float32, point_track (N,) int32)."""
    pts, idx, off, e = covis_arguments(views, eps, "covis_tracks")
    N, V = len(pts), len(off) - 1
    table = np.empty((N, V), np.int32)
    track_pts = np.empty((N, 2), np.float32)
    point_track = np.empty(N, np.int32)
    T = C.c_int(0)
    check(lib().apap_covis_tracks(_h(ctx), _ptr(pts, C.c_float), _ip(idx), _ip(off), V, C.c_float(float(e)), _ip(table),
                                  _ptr(track_pts, C.c_float), _ip(point_track), C.byref(T), device))
    return table[:T.value].copy(), track_pts[:T.value].copy(), point_track


def _rays(origins, dirs, who):
    o = np.ascontiguousarray(origins, dtype=np.float64)
    d = np.ascontiguousarray(dirs, dtype=np.float64)
    if o.size % 3 or o.size != d.size:
        raise ValueError(f"{who}: origins and dirs of 3 doubles a ray expected; got {o.shape} and {d.shape}")
    return o.reshape(-1, 3), d.reshape(-1, 3)


def ray_offsets(ray_offset, n_rays, who):
    """``ray_offset`` as int32 (T + 1,): starts at 0, ascends, ends at ``n_rays``."""
    off = np.asarray(ray_offset)
    if off.ndim != 1 or off.size < 1 or not np.issubdtype(off.dtype, np.integer):
        raise ValueError(f"{who}: ray_offset must be a 1-D integer array of T + 1 entries")
    if off[0] != 0 or (np.diff(off) < 0).any() or off[-1] != n_rays:
        raise ValueError(f"{who}: ray_offset must start at 0, ascend and end at the number of rays ({n_rays})")
    return np.ascontiguousarray(off, dtype=np.int32)


def triangulate_rays(origins, dirs, ray_offset, device=-1, ctx=None):
    """``apap_triangulate_rays``: the reference's ``solve_3d_position`` for T tracks at once; track k owns rays
    ``ray_offset[k] .. ray_offset[k + 1] - 1`` of ``origins`` / ``dirs`` ((R, 3) float64).  Returns (X (T, 3) float64, lam_min
    (T,) float64: A's smallest eigenvalue before the clamp at 1e-3, n_rays (T,) int32); a track without rays is NaN, NaN, 0."""
    who = "triangulate_rays"
    o, d = _rays(origins, dirs, who)
    off = ray_offsets(ray_offset, len(o), who)
    T = len(off) - 1
    X, lam, n = np.empty((T, 3)), np.empty(T), np.empty(T, np.int32)
    check(lib().apap_triangulate_rays(_h(ctx), _dp(o), _dp(d), _ip(off), T, _dp(X), _dp(lam), _ip(n), device))
    return X, lam, n


def triangulate_tables(n_views, dst_lengths, cams, center_cam, view_cam, min_views, who):
    """The host tables of the track triangulation, checked as the library checks them (before a device is touched): 1 .. 8
    views, one point count >= 0 per view, ``center_cam`` and every ``view_cam[v]`` among the ``cams`` cameras, ``min_views``
    >= 1.  Returns (dst_offset (V + 1,) int32, view_cam (V,) int32)."""
    if not 1 <= n_views <= COVIS_MAX_VIEWS:
        raise ValueError(f"{who}: {n_views} views (1 .. {COVIS_MAX_VIEWS})")
    if len(dst_lengths) != n_views or any(int(x) < 0 for x in dst_lengths):
        raise ValueError(f"{who}: one set of other-picture points per view expected ({n_views}); got {len(dst_lengths)}")
    cam = np.asarray(view_cam)
    if cam.shape != (n_views,) or not np.issubdtype(cam.dtype, np.integer) or (cam < 0).any() or (cam >= cams).any():
        raise ValueError(f"{who}: view_cam must name a camera 0 .. {cams - 1} for each of the {n_views} views; got {view_cam}")
    if not 0 <= int(center_cam) < cams:
        raise ValueError(f"{who}: center_cam = {center_cam} (0 .. {cams - 1})")
    if int(min_views) < 1:
        raise ValueError(f"{who}: min_views = {min_views} (>= 1)")
    off = np.zeros(n_views + 1, np.int32)
    off[1:] = np.cumsum([int(x) for x in dst_lengths])
    return off, np.ascontiguousarray(cam, dtype=np.int32)


def triangulate_tracks(table, track_pts, dst_pts, K_inv, Rs, origins, center_cam, view_cam, min_views=2, device=-1, ctx=None):
    """``apap_triangulate_tracks``: the loop of the reference's ``covid_3d_optimize`` for every track at once.  ``table``
    (T, V) int32 and ``track_pts`` (T, 2) float32 as ``covis_tracks`` returns them; ``dst_pts``: per view the other picture's
    points (n_v, 2) float32 that the table's column indexes; ``K_inv`` (3, 3), ``Rs`` (C, 3, 3), ``origins`` (C, 3) float64;
    the centre picture is camera ``center_cam``, view v camera ``view_cam[v]``.  Returns (X (T, 3), lam_min (T,), n_rays (T,)
    int32); a track seen in fewer than ``min_views`` views is NaN, NaN, 0."""
    who = "triangulate_tracks"
    tb = np.asarray(table)
    if tb.ndim != 2 or not (np.issubdtype(tb.dtype, np.integer) or tb.size == 0):
        raise ValueError(f"{who}: table (T, V) of integers expected; got {tb.shape} {tb.dtype}")
    T, V = tb.shape
    tb = np.ascontiguousarray(tb, dtype=np.int32)
    tp = np.ascontiguousarray(track_pts, dtype=np.float32)
    if tp.shape != (T, 2):
        raise ValueError(f"{who}: track_pts ({T}, 2) expected; got {tp.shape}")
    dst = [np.ascontiguousarray(d, dtype=np.float32).reshape(-1, 2) for d in dst_pts]
    K = np.ascontiguousarray(K_inv, dtype=np.float64)
    R = np.ascontiguousarray(Rs, dtype=np.float64)
    o = np.ascontiguousarray(origins, dtype=np.float64)
    if K.size != 9 or R.ndim < 2 or R.size % 9 or R.size == 0 or o.size != R.size // 3:
        raise ValueError(f"{who}: K_inv (3, 3), Rs (C, 3, 3) and origins (C, 3) expected; got {K.shape}, {R.shape}, {o.shape}")
    R = R.reshape(-1, 9)
    off, cam = triangulate_tables(V, [len(d) for d in dst], len(R), center_cam, view_cam, min_views, who)
    flat = np.ascontiguousarray(np.concatenate(dst)) if dst else np.zeros((0, 2), np.float32)
    X, lam, n = np.empty((T, 3)), np.empty(T), np.empty(T, np.int32)
    check(lib().apap_triangulate_tracks(_h(ctx), _ip(tb), _ptr(tp, C.c_float), T, V, _ptr(flat, C.c_float), _ip(off), _dp(K), _dp(R),
                                        _dp(o), len(R), int(center_cam), _ip(cam), int(min_views), _dp(X), _dp(lam), _ip(n), device))
    return X, lam, n


DEHAZE_MAX_RADIUS = 32                       # APAP_DEHAZE_MAX_RADIUS: of the minimum's window and of the guided filter's
DEHAZE_ONE = 4096                            # the transmission's unit: 12 fractional bits
# the kernels' tile sides (rows, cols) and the pixels a block of the selection scans at a time: APAP_DEHAZE_*_TILE_*, _AIR_CHUNK
DEHAZE_TILES = {"min": (16, 128), "ab": (16, 64), "recover": (16, 64)}
DEHAZE_AIR_CHUNK = 1024
DEHAZE_AIR_MAX_BLOCKS = 1024                 # APAP_DEHAZE_AIR_MAX_BLOCKS: the selection's grid; a larger picture takes passes
DEHAZE_MAX_IMAGES = 65535


def _pictures(imgs, who):
    """``imgs`` as contiguous uint8 (n, h, w, c), c = 1 or 3."""
    a = np.ascontiguousarray(imgs, dtype=np.uint8)
    if a.ndim != 4 or a.size == 0 or a.shape[3] not in (1, 3):
        raise ValueError(f"{who}: (n, h, w, 1) or (n, h, w, 3) uint8 pictures expected; got {a.shape}")
    return a


def dark_channel(imgs, radius=7, device=-1, ctx=None):
    """``apap_dark_channel``: (n, h, w) uint8, the window minimum of the channel minimum of (n, h, w, c) pictures."""
    a = _pictures(imgs, "dark_channel")
    out = np.empty(a.shape[:3], dtype=np.uint8)
    check(lib().apap_dark_channel(_h(ctx), _ptr(a, C.c_uint8), a.shape[0], a.shape[1], a.shape[2], a.shape[3], int(radius),
                                  _ptr(out, C.c_uint8), device))
    return out


def atmospheric_light(imgs, radius=7, device=-1, ctx=None):
    """``apap_atmospheric_light``: (n, c) uint8, the atmospheric light of each of (n, h, w, c) pictures."""
    a = _pictures(imgs, "atmospheric_light")
    out = np.empty((a.shape[0], a.shape[3]), dtype=np.uint8)
    check(lib().apap_atmospheric_light(_h(ctx), _ptr(a, C.c_uint8), a.shape[0], a.shape[1], a.shape[2], a.shape[3], int(radius),
                                       _ptr(out, C.c_uint8), device))
    return out


def transmission(imgs, radius=7, omega_q=243, t0_q=410, refine=30, eps=64, device=-1, ctx=None):
    """``apap_transmission``: (n, h, w) uint16 with 12 fractional bits, refined by the guided filter (refine > 0) or not."""
    a = _pictures(imgs, "transmission")
    out = np.empty(a.shape[:3], dtype=np.uint16)
    check(lib().apap_transmission(_h(ctx), _ptr(a, C.c_uint8), a.shape[0], a.shape[1], a.shape[2], a.shape[3], int(radius), int(omega_q),
                                  int(t0_q), int(refine), int(eps), _ptr(out, C.c_uint16), device))
    return out


def dehaze(imgs, radius=7, omega_q=243, t0_q=410, refine=30, eps=64, parts=False, device=-1, ctx=None):
    """``apap_dehaze``: the dehazed (n, h, w, c) uint8 pictures; with ``parts`` also t (n, h, w) uint16 and A (n, c) uint8."""
    a = _pictures(imgs, "dehaze")
    out = np.empty(a.shape, dtype=np.uint8)
    t = np.empty(a.shape[:3], dtype=np.uint16) if parts else None
    A = np.empty((a.shape[0], a.shape[3]), dtype=np.uint8) if parts else None
    check(lib().apap_dehaze(_h(ctx), _ptr(a, C.c_uint8), a.shape[0], a.shape[1], a.shape[2], a.shape[3], int(radius), int(omega_q), int(t0_q),
                            int(refine), int(eps), _ptr(out, C.c_uint8), _ptr(t, C.c_uint16), _ptr(A, C.c_uint8), device))
    return (out, t, A) if parts else out


WARP_GEOMETRY, WARP_CELLS, WARP_GATHER, WARP_ALL = 1, 2, 4, 7      # phases of apap_warp_batch_device
RANSAC_ITERATIONS = 2048                 # include/apap_hip.h
RANSAC_SEED = 0x5EEDC0DE5EEDC0DE


def find_homography_ransac(src, dst, thresh=5.0, iterations=RANSAC_ITERATIONS, seed=RANSAC_SEED, device=-1, ctx=None):
    """``cv.findHomography(src, dst, cv.RANSAC, thresh)``: ``(H (3, 3) float64 or None, mask (n, 1) uint8)``."""
    s = np.ascontiguousarray(src, dtype=np.float32).reshape(-1, 2)
    d = np.ascontiguousarray(dst, dtype=np.float32).reshape(-1, 2)
    if s.shape != d.shape:
        raise ValueError(f"src and dst must have the same number of points; got {s.shape} and {d.shape}")
    H = np.zeros(9, dtype=np.float64)
    mask = np.zeros(len(s), dtype=np.uint8)
    inliers = C.c_int(0)
    check(lib().apap_find_homography_ransac(_h(ctx), _ptr(s, C.c_float), _ptr(d, C.c_float), len(s), float(thresh), int(iterations),
                                            C.c_ulonglong(seed), _ptr(H, C.c_double), _ptr(mask, C.c_uint8),
                                            C.byref(inliers), device))
    if inliers.value < 4:
        return None, mask.reshape(-1, 1)
    return H.reshape(3, 3), mask.reshape(-1, 1)


FUNDAMENTAL_MIN_POINTS = 8
FUNDAMENTAL_MAX_PAIRS = 65535


def fundamental_arguments(lengths, thresh, iterations, who):
    """The checks of the fundamental-matrix entry points, made before the library (or a device) is touched: pairs of at least
    8 matches, ``thresh`` >= 0 (not NaN), 1 <= ``iterations`` <= 2^24.  Returns the int32 offsets (len + 1)."""
    lengths = [int(x) for x in lengths]
    if not 1 <= len(lengths) <= FUNDAMENTAL_MAX_PAIRS:
        raise ValueError(f"{who}: {len(lengths)} pairs (1 .. {FUNDAMENTAL_MAX_PAIRS})")
    if any(x < FUNDAMENTAL_MIN_POINTS for x in lengths):
        raise ValueError(f"{who}: a fundamental matrix needs {FUNDAMENTAL_MIN_POINTS} matches; got {lengths}")
    if sum(lengths) > np.iinfo(np.int32).max:
        raise ValueError(f"{who}: {sum(lengths)} matches in all exceed the int32 offsets")
    if not float(thresh) >= 0.0:
        raise ValueError(f"{who}: thresh = {thresh} (>= 0)")
    if not 1 <= int(iterations) <= 1 << 24:
        raise ValueError(f"{who}: iterations = {iterations} (1 .. 2^24)")
    off = np.zeros(len(lengths) + 1, np.int32)
    off[1:] = np.cumsum(lengths)
    return off


def fundamental_workspace_layout(n_pairs, iterations):
    """Byte offsets of the parts of the resident forms' workspace (include/apap_hip.h): ``dict(offsets, boxes, hyps, winners,
    counts, total)``."""
    up = lambda b: (b + 255) // 256 * 256      # noqa: E731
    sizes = (("offsets", (n_pairs + 1) * 4), ("boxes", n_pairs * 64), ("hyps", n_pairs * iterations * 72),
             ("winners", n_pairs * 72), ("counts", n_pairs * iterations * 4))
    out, at = {}, 0
    for name, b in sizes:
        out[name] = at
        at += up(b)
    out["total"] = at
    return out


def _match_points(src, dst, who):
    s = np.ascontiguousarray(src, dtype=np.float32).reshape(-1, 2)
    d = np.ascontiguousarray(dst, dtype=np.float32).reshape(-1, 2)
    if s.shape != d.shape:
        raise ValueError(f"{who}: src and dst must have the same number of points; got {s.shape} and {d.shape}")
    return s, d


def find_fundamental_ransac_batch(pairs, thresh=3.0, iterations=RANSAC_ITERATIONS, seed=RANSAC_SEED, device=-1, ctx=None):
    """``apap_find_fundamental_ransac_batch``: ``pairs`` is a sequence of ``(src, dst)``, each (n, 2) with n >= 8; one call, one
    set of kernel launches.  Returns a list of ``(F (3, 3) float64 or None, mask (n, 1) uint8)``, each what
    ``find_fundamental_ransac`` gives for that pair alone."""
    who = "find_fundamental_ransac_batch"
    pts = [_match_points(s, d, who) for s, d in pairs]
    off = fundamental_arguments([len(s) for s, _ in pts], thresh, iterations, who)
    src = np.concatenate([s for s, _ in pts])
    dst = np.concatenate([d for _, d in pts])
    F = np.zeros((len(pts), 9), dtype=np.float64)
    mask = np.zeros(len(src), dtype=np.uint8)
    inliers = np.zeros(len(pts), dtype=np.int32)
    check(lib().apap_find_fundamental_ransac_batch(_h(ctx), _ptr(src, C.c_float), _ptr(dst, C.c_float), _ip(off), len(pts),
                                                   float(thresh), int(iterations), C.c_ulonglong(seed), _ptr(F, C.c_double),
                                                   _ptr(mask, C.c_uint8), _ip(inliers), device))
    out = []
    for p in range(len(pts)):
        m = mask[off[p]:off[p + 1]].reshape(-1, 1)
        out.append((None if inliers[p] < FUNDAMENTAL_MIN_POINTS or not np.isfinite(F[p]).all() else F[p].reshape(3, 3), m))
    return out


def find_fundamental_ransac(src, dst, thresh=3.0, iterations=RANSAC_ITERATIONS, seed=RANSAC_SEED, device=-1, ctx=None):
    """``cv.findFundamentalMat(src, dst, cv.FM_RANSAC, thresh)`` with this repository's estimator (include/apap_hip.h):
    ``(F (3, 3) float64 or None, mask (n, 1) uint8)``; ``dst_h^T F src_h = 0``, ``|dst^T F src|`` at most the distance in
    pixels of ``dst`` from the epipolar line of ``src``.  ``None`` (and a cleared mask) when fewer than 8 matches agree."""
    s, d = _match_points(src, dst, "find_fundamental_ransac")
    fundamental_arguments([len(s)], thresh, iterations, "find_fundamental_ransac")
    F = np.zeros(9, dtype=np.float64)
    mask = np.zeros(len(s), dtype=np.uint8)
    inliers = C.c_int(0)
    check(lib().apap_find_fundamental_ransac(_h(ctx), _ptr(s, C.c_float), _ptr(d, C.c_float), len(s), float(thresh), int(iterations),
                                             C.c_ulonglong(seed), _ptr(F, C.c_double), _ptr(mask, C.c_uint8),
                                             C.byref(inliers), device))
    if inliers.value < FUNDAMENTAL_MIN_POINTS or not np.isfinite(F).all():
        return None, mask.reshape(-1, 1)
    return F.reshape(3, 3), mask.reshape(-1, 1)


# ---------------------------------------------------------------- spectral weights (spectral_method.py:66-133)
SPECTRAL_DIM = 128
SPECTRAL_PARAMS = 6          # epi_weight, affinity_eps, aff_thresh, em_radius, score_thresh, max_restarts
SPECTRAL_INFO = 6            # lambda, gap, steps, status, restarts, residual


def spectral_params(epi_weight=0.5, affinity_eps=30.0, aff_thresh=0.5, em_radius=6.0, score_thresh=0.4, max_restarts=0):
    """The ``params`` block of the spectral entry points (defaults: the reference's options.py; max_restarts 0 = 30)."""
    return np.array([epi_weight, affinity_eps, aff_thresh, em_radius, score_thresh, max_restarts], dtype=np.float64)


def _spectral_inputs(src, dst, c_feats, o_feats, F):
    src = np.ascontiguousarray(src, dtype=np.float32)
    dst = np.ascontiguousarray(dst, dtype=np.float32)
    c = np.ascontiguousarray(c_feats, dtype=np.float32)
    o = np.ascontiguousarray(o_feats, dtype=np.float32)
    F = np.ascontiguousarray(F, dtype=np.float64)
    if src.ndim != 2 or src.shape[1] != 2 or dst.shape != src.shape:
        raise ValueError(f"src/dst must both be (n, 2); got {src.shape} and {dst.shape}")
    n = src.shape[0]
    if c.shape != (n, SPECTRAL_DIM) or o.shape != (n, SPECTRAL_DIM):
        raise ValueError(f"descriptors must be ({n}, {SPECTRAL_DIM}); got {c.shape} and {o.shape}")
    if F.shape != (3, 3):
        raise ValueError(f"F must be 3 x 3; got {F.shape}")
    if n == 0:
        raise ValueError("no matches: the reference's np.hstack of the empty point arrays fails (spectral_method.py:105)")
    return src, dst, c, o, F, n


def spectral_weights(src, dst, c_feats, o_feats, F, params, Hg=None, mask=None, device=-1, ctx=None):
    """``apap_spectral_weights``: (segment float64, ransac_mask float32, original_mask float32, info (6,) float64)."""
    src, dst, c, o, F, n = _spectral_inputs(src, dst, c_feats, o_feats, F)
    params = np.ascontiguousarray(params, dtype=np.float64)
    if params.shape != (SPECTRAL_PARAMS,):
        raise ValueError(f"params must hold {SPECTRAL_PARAMS} values")
    Hg = None if Hg is None else np.ascontiguousarray(Hg, dtype=np.float32)
    if Hg is not None and Hg.shape != (3, 3):
        raise ValueError(f"Hg must be 3 x 3; got {Hg.shape}")
    mask = None if mask is None or Hg is not None else np.ascontiguousarray(mask, dtype=np.float32).ravel()
    if mask is not None and mask.shape != (n,):
        raise ValueError(f"mask must hold {n} values; got {mask.shape}")
    seg = np.empty(n, np.float64)
    rm = np.empty(n, np.float32)
    om = np.empty(n, np.float32)
    info = np.empty(SPECTRAL_INFO, np.float64)
    check(lib().apap_spectral_weights(_h(ctx), _ptr(src, C.c_float), _ptr(dst, C.c_float), _ptr(c, C.c_float), _ptr(o, C.c_float),
                                      n, _ptr(F, C.c_double), _ptr(params, C.c_double), _ptr(Hg, C.c_float), _ptr(mask, C.c_float),
                                      _ptr(seg, C.c_double), _ptr(rm, C.c_float), _ptr(om, C.c_float), _ptr(info, C.c_double),
                                      device))
    return seg, rm, om, info


def spectral_affinity(src, dst, c_feats, o_feats, F, params=None, device=-1, ctx=None):
    """``apap_spectral_affinity``: the reference's dense M, (n, n) float64, n <= 8192."""
    src, dst, c, o, F, n = _spectral_inputs(src, dst, c_feats, o_feats, F)
    params = spectral_params() if params is None else np.ascontiguousarray(params, dtype=np.float64)
    M = np.empty((n, n), np.float64)
    check(lib().apap_spectral_affinity(_h(ctx), _ptr(src, C.c_float), _ptr(dst, C.c_float), _ptr(c, C.c_float), _ptr(o, C.c_float),
                                       n, _ptr(F, C.c_double), _ptr(params, C.c_double), _ptr(M, C.c_double), device))
    return M


# ---------------------------------------------------------------- M-step and EM loop (spectral_method.py:165-241)
MODEL_LMS, MODEL_SDP, MODEL_HUBER = 0, 1, 2      # HUBER: M in the du slot (APAP_MODEL_HUBER_M), n <= 2^20
MODEL_HUBER_THREADS = 256                        # APAP_MODEL_HUBER_THREADS
MODEL_PARAMS = 6
MODEL_INFO = 24
MODEL_INFO_OBJECTIVE, MODEL_INFO_R, MODEL_INFO_T, MODEL_INFO_GAP, MODEL_INFO_ITERS, MODEL_INFO_STATUS, MODEL_INFO_COUNT = range(7)
MODEL_INFO_Z, MODEL_INFO_H = 7, 16
MODEL_FLOOR = 1e-3      # model_solve: `if w <= 1e-3: continue`


def model_params(mode, du=1.0, dv=1.0, floor=MODEL_FLOOR, swap=True, max_iter=0):
    """The ``params`` block of the M-step entry points (``floor=None`` keeps every match; max_iter 0 = the mode's default:
    80 interior-point iterations, 100 Huber steps).  Mode MODEL_HUBER takes M as ``du``; ``dv`` is ignored."""
    return np.array([mode, du, dv, -np.inf if floor is None else floor, 1.0 if swap else 0.0, max_iter], dtype=np.float64)


def _model_inputs(pts_c, pts_o, weights):
    pc = np.ascontiguousarray(pts_c, dtype=np.float32)
    po = np.ascontiguousarray(pts_o, dtype=np.float32)
    w = np.ascontiguousarray(weights, dtype=np.float32).ravel()
    if pc.ndim != 2 or pc.shape[1] != 2 or po.shape != pc.shape or w.shape != (pc.shape[0],):
        raise ValueError(f"pts_c / pts_o must be (n, 2) and weights (n,); got {pc.shape}, {po.shape}, {w.shape}")
    return pc, po, w


def model_solve(pts_c, pts_o, weights, params, device=-1, ctx=None):
    """``apap_model_solve``: (H float32 3 x 3, info (24,) float64).  Raises ApapValueError for bad arguments or a degenerate
    selection and ApapSingularError when the inverse meets a zero pivot; the info block is on the exception as ``.info``
    (all NaN when the kernels did not run).  Points and weights are rounded to float32 (the rows of model_solve)."""
    pc, po, w = _model_inputs(pts_c, pts_o, weights)
    params = np.ascontiguousarray(params, dtype=np.float64)
    if params.shape != (MODEL_PARAMS,):
        raise ValueError(f"params must hold {MODEL_PARAMS} values")
    H = np.full((3, 3), np.nan, np.float32)
    info = np.full(MODEL_INFO, np.nan)
    code = lib().apap_model_solve(_h(ctx), _ptr(pc, C.c_float), _ptr(po, C.c_float), _ptr(w, C.c_float), len(pc),
                                  _ptr(params, C.c_double), _ptr(H, C.c_float), _ptr(info, C.c_double), device)
    _check_with_info(code, info)
    return H, info


def _check_with_info(code, info):
    try:
        check(code)
    except ApapError as e:
        e.info = info
        raise


def spectral_em(src, dst, c_feats, o_feats, F, spec_params, model_params_, em_steps, mask, device=-1, ctx=None):
    """``apap_spectral_em``: per round (H (k, 3, 3) float32, model info (k, 24), segment (k, n) float64, ransac_mask (k, n)
    float32, original_mask (k, n) float32, spectral info (k, 6)).  Errors as model_solve (``.info`` holds every round's
    outputs as the tuple above; H and the model info all NaN when the kernels did not run)."""
    src, dst, c, o, F, n = _spectral_inputs(src, dst, c_feats, o_feats, F)
    sp = np.ascontiguousarray(spec_params, dtype=np.float64)
    mp = np.ascontiguousarray(model_params_, dtype=np.float64)
    if sp.shape != (SPECTRAL_PARAMS,) or mp.shape != (MODEL_PARAMS,):
        raise ValueError("spectral / model parameter blocks of the wrong size")
    mask = np.ascontiguousarray(mask, dtype=np.float32).ravel()
    if mask.shape != (n,):
        raise ValueError(f"mask must hold {n} values; got {mask.shape}")
    k = int(em_steps)
    H = np.full((k, 3, 3), np.nan, np.float32)
    info = np.full((k, MODEL_INFO), np.nan)
    seg = np.empty((k, n), np.float64)
    rm = np.empty((k, n), np.float32)
    om = np.empty((k, n), np.float32)
    sinfo = np.empty((k, SPECTRAL_INFO), np.float64)
    code = lib().apap_spectral_em(_h(ctx), _ptr(src, C.c_float), _ptr(dst, C.c_float), _ptr(c, C.c_float), _ptr(o, C.c_float), n,
                                  _ptr(F, C.c_double), _ptr(sp, C.c_double), _ptr(mp, C.c_double), k, _ptr(mask, C.c_float),
                                  _ptr(H, C.c_float), _ptr(info, C.c_double), _ptr(seg, C.c_double), _ptr(rm, C.c_float),
                                  _ptr(om, C.c_float), _ptr(sinfo, C.c_double), device)
    out = (H, info, seg, rm, om, sinfo)
    _check_with_info(code, out)
    return out


def em_batch_tables(pair_lengths, pair_of, spec_params, model_params_):
    """The host tables of the batch entry points, checked: (pair_offset (P + 1,) int32, pair_of (B,) int32, spec_params
    (B, 6) float64, model_params (B, 6) float64).  ``pair_lengths``: the number of matches of each pair."""
    lengths = np.asarray(pair_lengths, dtype=np.int64).ravel()
    if len(lengths) == 0 or np.any(lengths < 1):
        raise ValueError("a batch needs at least one pair, and every pair at least one match")
    off = np.zeros(len(lengths) + 1, np.int32)
    off[1:] = np.cumsum(lengths)
    po = np.asarray(pair_of)
    if po.ndim != 1 or len(po) == 0 or not np.issubdtype(po.dtype, np.integer):
        raise ValueError("pair_of must be a non-empty 1-D integer array")
    if np.any(po < 0) or np.any(po >= len(lengths)):
        raise ValueError(f"pair_of holds a pair index outside 0 .. {len(lengths) - 1}")
    po = np.ascontiguousarray(po, dtype=np.int32)
    sp = np.ascontiguousarray(spec_params, dtype=np.float64)
    mp = np.ascontiguousarray(model_params_, dtype=np.float64)
    if sp.shape != (len(po), SPECTRAL_PARAMS) or mp.shape != (len(po), MODEL_PARAMS):
        raise ValueError(f"spectral / model parameter blocks must be ({len(po)}, {SPECTRAL_PARAMS}) and ({len(po)}, {MODEL_PARAMS}); "
                         f"got {sp.shape} and {mp.shape}")
    if np.any(sp[:, 5] != sp[0, 5]):
        raise ValueError("max_restarts must be equal across the problems of a batch (the cap fixes how many cycles are enqueued)")
    return off, po, sp, mp


def em_batch_split(flat, lengths, em_steps):
    """A per-match output of a batch call (problem-major, round-major inside a problem) as a list of (em_steps, n_b) views."""
    out, at = [], 0
    for n in lengths:
        out.append(flat[at:at + em_steps * n].reshape(em_steps, n))
        at += em_steps * n
    return out


def spectral_em_batch(src, dst, c_feats, o_feats, F, mask, pair_lengths, pair_of, spec_params, model_params_, em_steps, device=-1,
                      ctx=None):
    """``apap_spectral_em_batch``: B EM problems in lockstep.  src / dst (N, 2), c_feats / o_feats (N, 128), mask (N,): the
    pairs concatenated, pair p of ``pair_lengths[p]`` matches; F (P, 3, 3); ``pair_of`` (B,): the pair of each problem;
    ``spec_params`` (B, 6), ``model_params_`` (B, 6).  Returns (H (B, k, 3, 3) float32, model info (B, k, 24), segment, ransac_mask,
    original_mask: lists of B arrays (k, n_b), spectral info (B, k, 6), status (B,) int32).  Every problem's outputs equal
    ``spectral_em``'s for that problem alone, byte for byte.  A degenerate, singular or unconverged problem does not raise: its
    bits are in ``status`` and in its info blocks."""
    src = np.ascontiguousarray(src, dtype=np.float32)
    dst = np.ascontiguousarray(dst, dtype=np.float32)
    c = np.ascontiguousarray(c_feats, dtype=np.float32)
    o = np.ascontiguousarray(o_feats, dtype=np.float32)
    F = np.ascontiguousarray(F, dtype=np.float64)
    off, po, sp, mp = em_batch_tables(pair_lengths, pair_of, spec_params, model_params_)
    N, P, B, k = int(off[-1]), len(off) - 1, len(po), int(em_steps)
    if src.shape != (N, 2) or dst.shape != (N, 2):
        raise ValueError(f"src/dst must both be ({N}, 2); got {src.shape} and {dst.shape}")
    if c.shape != (N, SPECTRAL_DIM) or o.shape != (N, SPECTRAL_DIM):
        raise ValueError(f"descriptors must be ({N}, {SPECTRAL_DIM}); got {c.shape} and {o.shape}")
    if F.shape != (P, 3, 3):
        raise ValueError(f"F must be ({P}, 3, 3); got {F.shape}")
    mask = np.ascontiguousarray(mask, dtype=np.float32).ravel()
    if mask.shape != (N,):
        raise ValueError(f"mask must hold {N} values; got {mask.shape}")
    if not 1 <= k <= 64:
        raise ValueError(f"em_steps {k} (1 .. 64)")
    lengths = [int(off[p + 1] - off[p]) for p in po]
    M = sum(lengths)
    H = np.full((B, k, 3, 3), np.nan, np.float32)
    info = np.full((B, k, MODEL_INFO), np.nan)
    seg = np.empty(k * M, np.float64)
    rm = np.empty(k * M, np.float32)
    om = np.empty(k * M, np.float32)
    sinfo = np.empty((B, k, SPECTRAL_INFO), np.float64)
    status = np.zeros(B, np.int32)
    check(lib().apap_spectral_em_batch(_h(ctx), _ptr(src, C.c_float), _ptr(dst, C.c_float), _ptr(c, C.c_float), _ptr(o, C.c_float),
                                       _ptr(F, C.c_double), _ptr(mask, C.c_float), _ptr(off, C.c_int), P, _ptr(po, C.c_int),
                                       _ptr(sp, C.c_double), _ptr(mp, C.c_double), B, k, _ptr(H, C.c_float), _ptr(info, C.c_double),
                                       _ptr(seg, C.c_double), _ptr(rm, C.c_float), _ptr(om, C.c_float), _ptr(sinfo, C.c_double),
                                       _ptr(status, C.c_int), device))
    return (H, info, em_batch_split(seg, lengths, k), em_batch_split(rm, lengths, k), em_batch_split(om, lengths, k), sinfo, status)


# ---------------------------------------------------------------- robust moving DLT: the M-step's solve per mesh cell
LOCAL_MODEL_CHUNK = 4096            # APAP_LOCAL_MODEL_CHUNK: cells whose scratch apap_local_model_workspace_bytes asks for
LOCAL_MODEL_MAX_CELLS = 1 << 24     # APAP_LOCAL_MODEL_MAX_CELLS


def local_model_inputs(pts_c, pts_o, vertices, params, match_weights):
    """The host arrays of the robust moving DLT's entry points, checked: (pts_c, pts_o (n, 2) float32, vertices (..., 2)
    float64, params (6,) float64, match_weights (n,) float32 or None)."""
    pc = np.ascontiguousarray(pts_c, dtype=np.float32)
    po = np.ascontiguousarray(pts_o, dtype=np.float32)
    if pc.ndim != 2 or pc.shape[1] != 2 or po.shape != pc.shape:
        raise ValueError(f"pts_c / pts_o must both be (n, 2); got {pc.shape} and {po.shape}")
    v = np.ascontiguousarray(vertices, dtype=np.float64)
    if v.ndim < 1 or v.shape[-1] != 2:
        raise ValueError(f"vertices must be (..., 2); got {v.shape}")
    params = np.ascontiguousarray(params, dtype=np.float64)
    if params.shape != (MODEL_PARAMS,):
        raise ValueError(f"params must hold {MODEL_PARAMS} values")
    mw = None
    if match_weights is not None:
        mw = np.ascontiguousarray(match_weights, dtype=np.float32).ravel()
        if mw.shape != (pc.shape[0],):
            raise ValueError(f"match_weights must hold {pc.shape[0]} values; got {mw.shape}")
    return pc, po, v, params, mw


def local_model_solve(pts_c, pts_o, vertices, gamma, sigma, params, match_weights=None, device=-1, ctx=None):
    """``apap_local_model_solve``: the M-step's solve (``params``: ``model_params``) for every sample point of ``vertices``
    (..., 2) float64, with the weight vector ``float32(local_weights(pts_c, vertex, gamma, sigma)) * match_weights`` - never
    stored.  Returns (H (..., 3, 3) float32, info (..., 24) float64, status (...,) int32); every cell equals ``model_solve``
    on its own weight vector, byte for byte.  A degenerate, singular or unconverged cell does not raise: its bits are in
    ``status`` and in its info block, its H is NaN when degenerate.  ``match_weights``: (n,) float32, typically the last round's
    ``ransac_mask`` of ``spectral_em``."""
    pc, po, v, params, mw = local_model_inputs(pts_c, pts_o, vertices, params, match_weights)
    lead, cells = v.shape[:-1], v.size // 2
    H = np.full(lead + (3, 3), np.nan, np.float32)
    info = np.full(lead + (MODEL_INFO,), np.nan)
    status = np.zeros(lead, np.int32)
    if cells:
        check(lib().apap_local_model_solve(_h(ctx), _ptr(pc, C.c_float), _ptr(po, C.c_float), _ptr(mw, C.c_float), len(pc),
                                           _ptr(v, C.c_double), cells, float(gamma), float(sigma), _ptr(params, C.c_double),
                                           _ptr(H, C.c_float), _ptr(info, C.c_double), _ptr(status, C.c_int), device))
    return H, info, status


# ---------------------------------------------------------------- descriptor matching: exact nearest and second-nearest
MATCH_DIM = 128                 # APAP_MATCH_DIM
MATCH_QUERY_TILE = 64           # APAP_MATCH_QUERY_TILE: queries per block
MATCH_TRAIN_CHUNK = 128         # APAP_MATCH_TRAIN_CHUNK: train rows per staged chunk
MATCH_WANT_BLOCKS = 4096        # APAP_MATCH_WANT_BLOCKS: the train axis is split until a pair has about this many blocks
MATCH_MAX_ROWS = 1 << 24        # queries / train rows of one pair
MATCH_MAX_PAIRS = 65535


def train_splits(nq, nt, q_tile, chunk, want):
    """Into how many splits the train axis of an (nq, nt) pair is cut, and of how many chunks each (the last may be shorter),
    by a matcher whose blocks take ``q_tile`` queries and chunks of ``chunk`` train rows and that wants about ``want`` blocks:
    the rule of include/apap_hip.h.  No output depends on it; tests use it to place shapes at its edges."""
    q_tiles = -(-int(nq) // q_tile)
    chunks = -(-int(nt) // chunk)
    per = -(-chunks // min(chunks, -(-want // q_tiles)))
    return -(-chunks // per), per


def match_splits(nq, nt):
    """``train_splits`` for the exact matcher's tiling."""
    return train_splits(nq, nt, MATCH_QUERY_TILE, MATCH_TRAIN_CHUNK, MATCH_WANT_BLOCKS)


def as_descriptors(a, name="descriptors"):
    """(n, 128) descriptors as a contiguous float32 array: uint8 (or any integer or float dtype) is converted."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    if a.ndim != 2 or a.shape[1] != MATCH_DIM:
        raise ValueError(f"{name} must be (n, {MATCH_DIM}); got {a.shape}")
    return a


def match_offsets(lengths, name):
    """Row counts of the pairs -> int32 offsets (len + 1), checked as the library checks them."""
    return _offsets(lengths, name, "a pair", "pairs", "rows", MATCH_MAX_PAIRS, MATCH_MAX_ROWS)


def _match_batch_args(q, t, q_lengths, t_lengths, who):
    """The descriptors and row counts of a batch call of either matcher -> (q, t, query offsets, train offsets), checked."""
    q, t = as_descriptors(q, "q"), as_descriptors(t, "t")
    if len(q_lengths) != len(t_lengths):
        raise ValueError(f"{who}: {len(q_lengths)} query counts, {len(t_lengths)} train counts")
    qo, to = match_offsets(q_lengths, "q_lengths"), match_offsets(t_lengths, "t_lengths")
    if qo[-1] != len(q) or to[-1] != len(t):
        raise ValueError(f"{who}: the counts sum to {qo[-1]} and {to[-1]} rows; got {len(q)} and {len(t)}")
    return q, t, qo, to


def _match_out(n, dtype, wanted=True):
    """An output of ``n`` rows, or None where the caller did not ask for it."""
    return np.empty(n, dtype) if wanted else None


def match_descriptors(q, t, second=True, device=-1, ctx=None):
    """``apap_match_descriptors``: for every row of ``q`` (nq, 128) the nearest row of ``t`` (nt, 128) under the L2 distance,
    exactly (float32 sum of squared differences; exact for integer descriptors in 0 .. 255), and with ``second`` the
    runner-up.  uint8 or float descriptors are taken as float32.  Returns (idx (nq,) int32, dist (nq,) float32, idx2, dist2)
    - the last two ``None`` without ``second``.  Ties go to the lowest index; a NaN distance is never selected; where nothing
    can be selected (the runner-up of a single train row) the index is -1 and the distance +inf."""
    q, t = as_descriptors(q, "q"), as_descriptors(t, "t")
    if not 1 <= len(q) <= MATCH_MAX_ROWS or not 1 <= len(t) <= MATCH_MAX_ROWS:
        raise ValueError(f"match_descriptors: {len(q)} queries, {len(t)} train rows (1 .. 2^24 each)")
    idx, dist = _match_out(len(q), np.int32), _match_out(len(q), np.float32)
    idx2, dist2 = _match_out(len(q), np.int32, second), _match_out(len(q), np.float32, second)
    check(lib().apap_match_descriptors(_h(ctx), _ptr(q, C.c_float), len(q), _ptr(t, C.c_float), len(t), _ptr(idx, C.c_int),
                                       _ptr(dist, C.c_float), _ptr(idx2, C.c_int), _ptr(dist2, C.c_float), device))
    return idx, dist, idx2, dist2


def match_descriptors_batch(q, t, q_lengths, t_lengths, second=True, device=-1, ctx=None):
    """``apap_match_descriptors_batch``: many pairs in one call (two kernel launches, whatever their number).  ``q`` / ``t``:
    the pairs' descriptors concatenated, pair p of ``q_lengths[p]`` queries and ``t_lengths[p]`` train rows.  Returns the four
    arrays of ``match_descriptors`` laid out like ``q``; a pair's indices count from its own first train row, and its outputs
    equal its own single call's byte for byte."""
    q, t, qo, to = _match_batch_args(q, t, q_lengths, t_lengths, "match_descriptors_batch")
    idx, dist = _match_out(len(q), np.int32), _match_out(len(q), np.float32)
    idx2, dist2 = _match_out(len(q), np.int32, second), _match_out(len(q), np.float32, second)
    check(lib().apap_match_descriptors_batch(_h(ctx), _ptr(q, C.c_float), _ptr(t, C.c_float), _ptr(qo, C.c_int), _ptr(to, C.c_int),
                                             len(qo) - 1, _ptr(idx, C.c_int), _ptr(dist, C.c_float), _ptr(idx2, C.c_int),
                                             _ptr(dist2, C.c_float), device))
    return idx, dist, idx2, dist2


# ---------------------------------------------------------------- guided descriptor matching: the matcher under a gate
GUIDED_REC_POINT, GUIDED_REC_PROJECT, GUIDED_REC_LINE = 0, 1, 2     # APAP_GUIDED_REC_*
GUIDED_POINT, GUIDED_LINE = 0, 1                                    # APAP_GUIDED_*: the gate
GUIDED_QUERY_TILE = 256         # APAP_GUIDED_QUERY_TILE: queries per block, one per lane
GUIDED_TRAIN_CHUNK = 128        # APAP_GUIDED_TRAIN_CHUNK: train records per staged chunk
GUIDED_DRAIN = 64               # APAP_GUIDED_DRAIN: survivors a wave sums at once
GUIDED_WANT_BLOCKS = 1024       # APAP_GUIDED_WANT_BLOCKS
GUIDED_WHAT = {"point": GUIDED_REC_POINT, "project": GUIDED_REC_PROJECT, "line": GUIDED_REC_LINE}
GUIDED_KIND = {"point": GUIDED_POINT, "line": GUIDED_LINE}


def guided_splits(nq, nt):
    """``train_splits`` for the guided matcher's tiling: (splits of the train axis, chunks of each)."""
    return train_splits(nq, nt, GUIDED_QUERY_TILE, GUIDED_TRAIN_CHUNK, GUIDED_WANT_BLOCKS)


def guided_what(what):
    """'point' | 'project' | 'line' (or the constant) -> APAP_GUIDED_REC_*."""
    if what not in GUIDED_WHAT and what not in GUIDED_WHAT.values():
        raise ValueError(f"what must be one of {sorted(GUIDED_WHAT)}; got {what!r}")
    return GUIDED_WHAT.get(what, what)


def guided_kind(kind):
    """'point' | 'line' (or the constant) -> APAP_GUIDED_POINT / APAP_GUIDED_LINE."""
    if kind not in GUIDED_KIND and kind not in GUIDED_KIND.values():
        raise ValueError(f"kind must be one of {sorted(GUIDED_KIND)}; got {kind!r}")
    return GUIDED_KIND.get(kind, kind)


def guided_r2(r2, n_pairs):
    """The squared radius of every pair (a number, or one per pair) as float64: >= 0 or +inf, as the library checks it."""
    r2 = np.ascontiguousarray(np.broadcast_to(np.asarray(r2, dtype=np.float64), (n_pairs,)))
    if not np.all(r2 >= 0):
        raise ValueError(f"r2 must be >= 0 (or +inf); got {r2.tolist()}")
    return r2


def as_guided_model(model, what):
    """The 3 x 3 model of a record as 9 contiguous float64, or None; 'project' and 'line' need one."""
    if model is None:
        if what != GUIDED_REC_POINT:
            raise ValueError("records: a model is needed unless what='point'")
        return None
    m = np.ascontiguousarray(model, dtype=np.float64)
    if m.size != 9:
        raise ValueError(f"records: the model must hold 9 values; got {m.shape}")
    return m.reshape(9)


def as_guided_records(rec, n, name):
    rec = np.ascontiguousarray(rec, dtype=np.float64)
    if rec.shape != (n, 3):
        raise ValueError(f"{name} must be ({n}, 3) float64 records; got {rec.shape}")
    return rec


def guided_records(pts, model=None, what="point", device=-1, ctx=None):
    """``apap_guided_records``: the (n, 3) float64 records of ``pts`` (n, 2) float32 under ``model`` (3 x 3, float64)."""
    what = guided_what(what)
    pts = np.ascontiguousarray(pts, dtype=np.float32)
    if pts.ndim != 2 or pts.shape[1] != 2 or not 1 <= len(pts) <= MATCH_MAX_ROWS:
        raise ValueError(f"records: pts must be (n, 2) with 1 <= n <= 2^24; got {pts.shape}")
    m = as_guided_model(model, what)
    rec = np.empty((len(pts), 3), np.float64)
    check(lib().apap_guided_records(_h(ctx), _ptr(pts, C.c_float), len(pts), _ptr(m, C.c_double), what, _ptr(rec, C.c_double), device))
    return rec


def match_guided_batch(q, t, rec_q, rec_t, q_lengths, t_lengths, kind, r2, second=True, count=True, reverse=False, device=-1,
                       ctx=None):
    """``apap_match_guided_batch``: ``match_descriptors_batch`` under the gate ``kind`` with the squared radius ``r2`` (a number
    or one per pair).  Returns (idx, dist, idx2, dist2, count, ridx, rdist): the first five laid out like ``q``, the
    last two like ``t``; whatever was not asked for is ``None``."""
    kind = guided_kind(kind)
    q, t, qo, to = _match_batch_args(q, t, q_lengths, t_lengths, "match_guided_batch")
    rec_q, rec_t = as_guided_records(rec_q, len(q), "rec_q"), as_guided_records(rec_t, len(t), "rec_t")
    r2 = guided_r2(r2, len(qo) - 1)
    idx, dist = _match_out(len(q), np.int32), _match_out(len(q), np.float32)
    idx2, dist2 = _match_out(len(q), np.int32, second), _match_out(len(q), np.float32, second)
    cnt = _match_out(len(q), np.int32, count)
    ridx, rdist = _match_out(len(t), np.int32, reverse), _match_out(len(t), np.float32, reverse)
    check(lib().apap_match_guided_batch(_h(ctx), _ptr(rec_q, C.c_double), _ptr(rec_t, C.c_double), _ptr(q, C.c_float),
                                        _ptr(t, C.c_float), _ptr(qo, C.c_int), _ptr(to, C.c_int), len(qo) - 1, kind,
                                        _ptr(r2, C.c_double), _ptr(idx, C.c_int), _ptr(dist, C.c_float), _ptr(idx2, C.c_int),
                                        _ptr(dist2, C.c_float), _ptr(cnt, C.c_int), _ptr(ridx, C.c_int), _ptr(rdist, C.c_float), device))
    return idx, dist, idx2, dist2, cnt, ridx, rdist


def match_guided(q, t, rec_q, rec_t, kind, r2, second=True, count=True, reverse=False, device=-1, ctx=None):
    """``apap_match_guided``: one pair (the batch of one)."""
    q, t = as_descriptors(q, "q"), as_descriptors(t, "t")
    if not 1 <= len(q) <= MATCH_MAX_ROWS or not 1 <= len(t) <= MATCH_MAX_ROWS:
        raise ValueError(f"match_guided: {len(q)} queries, {len(t)} train rows (1 .. 2^24 each)")
    return match_guided_batch(q, t, rec_q, rec_t, [len(q)], [len(t)], kind, r2, second=second, count=count, reverse=reverse,
                              device=device, ctx=ctx)


# ---------------------------------------------------------------- descriptor extraction: SIFT at given keypoints
SIFT_DIM = 128                  # APAP_SIFT_DIM
SIFT_SAMPLES = 49               # APAP_SIFT_SAMPLES: the offsets |i|, |j| <= 3
SIFT_TAPS = 13                  # APAP_SIFT_TAPS
SIFT_PATCH = 21                 # APAP_SIFT_PATCH: the side of the grey patch one keypoint reads
SIFT_WINDOW_COLS = 8            # APAP_SIFT_WINDOW_COLS
SIFT_BLOCK_KEYPOINTS = 4        # APAP_SIFT_BLOCK_KEYPOINTS: keypoints per block (a wave each)
SIFT_MIN_SIDE, SIFT_MAX_SIDE = 7, 32768
SIFT_MAX_KEYPOINTS = 1 << 24    # per image
SIFT_MAX_IMAGES = 65535


def sift_window():
    """``apap_sift_window`` (host only): the (49, 8) float32 table of the samples, rows in the order (i, j) ascending over
    -3 .. 3: rbin, cbin, window weight, frac(rbin), frac(cbin), floor(rbin), floor(cbin), 0 - the kernel's own constants."""
    out = np.empty((SIFT_SAMPLES, SIFT_WINDOW_COLS), np.float32)
    check(lib().apap_sift_window(_ptr(out, C.c_float)))
    return out


def sift_taps():
    """``apap_sift_taps`` (host only): the 13 float32 taps of the base image's Gaussian - the kernel's own constants."""
    out = np.empty(SIFT_TAPS, np.float32)
    check(lib().apap_sift_taps(_ptr(out, C.c_float)))
    return out


def as_sift_image(img, name="img"):
    """A (h, w) grey or (h, w, 3) BGR uint8 image, contiguous; refuses every other dtype, shape or side outside 7 .. 32768.
    Returns (array, channels)."""
    img = np.asarray(img)
    if img.dtype != np.uint8:
        raise ValueError(f"{name} must be uint8; got {img.dtype}")
    if img.ndim not in (2, 3) or (img.ndim == 3 and img.shape[2] not in (1, 3)):
        raise ValueError(f"{name} must be (h, w) grey or (h, w, 3) BGR; got {img.shape}")
    if not all(SIFT_MIN_SIDE <= x <= SIFT_MAX_SIDE for x in img.shape[:2]):
        raise ValueError(f"{name}: sides must be {SIFT_MIN_SIDE} .. {SIFT_MAX_SIDE}; got {img.shape[:2]}")
    return np.ascontiguousarray(img), 1 if img.ndim == 2 else int(img.shape[2])


def as_sift_points(pts, name="pts"):
    """Keypoint coordinates (n, 2) as contiguous float32 (x, y): float64 and integers are cast first."""
    pts = np.ascontiguousarray(pts, dtype=np.float32)
    if pts.ndim != 2 or pts.shape[1] != 2:
        raise ValueError(f"{name} must be (n, 2); got {pts.shape}")
    return pts


def sift_offsets(lengths, name="lengths"):
    """Keypoint counts of the images -> int32 offsets (len + 1), checked as the library checks them."""
    return _offsets(lengths, name, "an image", "images", "keypoints", SIFT_MAX_IMAGES, SIFT_MAX_KEYPOINTS)


def sift_describe_batch(imgs, pts, lengths, device=-1, ctx=None):
    """``apap_sift_describe_batch``: the SIFT descriptors of OpenCV's ``KeyPoint(x, y, 1)`` at the given coordinates, many
    images in one call (one kernel launch, whatever their number).  ``imgs``: a sequence of (h, w) grey or (h, w, 3) BGR uint8
    arrays of any shapes; ``pts`` (N, 2): their keypoints (x, y) concatenated, image m of ``lengths[m]``.  Returns float32
    (N, 128) with integer values 0 .. 255; an image's rows equal its own single call's byte for byte.  A keypoint with no
    valid sample (on or beyond the border) gives zeros; a non-finite coordinate is refused."""
    got = [as_sift_image(im, f"imgs[{m}]") for m, im in enumerate(imgs)]
    pts = as_sift_points(pts)
    if len(got) != len(lengths):
        raise ValueError(f"sift_describe_batch: {len(got)} images, {len(lengths)} keypoint counts")
    off = sift_offsets(lengths)
    if off[-1] != len(pts):
        raise ValueError(f"sift_describe_batch: the counts sum to {off[-1]} keypoints; got {len(pts)}")
    ptrs, hs, ws, cs = _image_table(got)
    out = np.empty((len(pts), SIFT_DIM), np.float32)
    check(lib().apap_sift_describe_batch(_h(ctx), ptrs, _ip(hs), _ip(ws), _ip(cs), len(got), _ptr(pts, C.c_float), _ip(off),
                                         _ptr(out, C.c_float), device))
    return out


def sift_describe(img, pts, device=-1, ctx=None):
    """``apap_sift_describe``: float32 (n, 128) SIFT descriptors of ``KeyPoint(x, y, 1)`` at ``pts`` (n, 2) of one uint8 image
    (see ``sift_describe_batch``; the single call is the batch of one)."""
    img, ch = as_sift_image(img)
    pts = as_sift_points(pts)
    if not 1 <= len(pts) <= SIFT_MAX_KEYPOINTS:
        raise ValueError(f"sift_describe: {len(pts)} keypoints (1 .. 2^24)")
    out = np.empty((len(pts), SIFT_DIM), np.float32)
    check(lib().apap_sift_describe(_h(ctx), _ptr(img, C.c_uint8), img.shape[0], img.shape[1], ch, _ptr(pts, C.c_float), len(pts),
                                   _ptr(out, C.c_float), device))
    return out


# ---------------------------------------------------------------- keypoint orientation and the descriptor at an orientation
SIFT_ORIENT_SAMPLES = 25        # APAP_SIFT_ORIENT_SAMPLES: the offsets |i|, |j| <= 2
SIFT_DESCR_SAMPLES = 121        # APAP_SIFT_DESCR_SAMPLES: the offsets |i|, |j| <= 5
SIFT_ORIENT_PATCH = 25          # APAP_SIFT_ORIENT_PATCH: the side of the grey patch one keypoint reads
SIFT_ORIENT_MIN_SIDE = 13


def sift_orient_window():
    """``apap_sift_orient_window`` (host only): the 25 float32 weights of the orientation samples, (i, j) ascending."""
    out = np.empty(SIFT_ORIENT_SAMPLES, np.float32)
    check(lib().apap_sift_orient_window(_ptr(out, C.c_float)))
    return out


def sift_descr_window():
    """``apap_sift_descr_window`` (host only): the 121 float32 weights of the oriented descriptor's samples, (i, j) ascending."""
    out = np.empty(SIFT_DESCR_SAMPLES, np.float32)
    check(lib().apap_sift_descr_window(_ptr(out, C.c_float)))
    return out


def as_sift_orient_image(img, name="img"):
    """``as_sift_image`` with the oriented entry points' smallest side, 13."""
    img, ch = as_sift_image(img, name)
    if min(img.shape[:2]) < SIFT_ORIENT_MIN_SIDE:
        raise ValueError(f"{name}: sides must be {SIFT_ORIENT_MIN_SIDE} .. {SIFT_MAX_SIDE}; got {img.shape[:2]}")
    return img, ch


def as_sift_angles(angles, n, name="angles"):
    """Keypoint angles (n,) as contiguous float32, each in [0, 360] (``cv.KeyPoint.angle``)."""
    angles = np.ascontiguousarray(angles, dtype=np.float32)
    if angles.shape != (n,):
        raise ValueError(f"{name} must be ({n},); got {angles.shape}")
    if not np.all((angles >= 0) & (angles <= 360)):
        raise ValueError(f"{name} must lie in [0, 360]")
    return angles


def _sift_batch_args(imgs, pts, lengths, who):
    got = [as_sift_orient_image(im, f"imgs[{m}]") for m, im in enumerate(imgs)]
    pts = as_sift_points(pts)
    if len(got) != len(lengths):
        raise ValueError(f"{who}: {len(got)} images, {len(lengths)} keypoint counts")
    off = sift_offsets(lengths)
    if off[-1] != len(pts):
        raise ValueError(f"{who}: the counts sum to {off[-1]} keypoints; got {len(pts)}")
    return got, pts, off


def sift_orient_batch(imgs, pts, lengths, device=-1, ctx=None):
    """``apap_sift_orient_batch``: the dominant orientation of every keypoint, many images in one call.  Arguments as
    ``sift_describe_batch`` (sides from 13).  Returns float32 (N,) angles in [0, 360), ``cv.KeyPoint.angle``'s convention; a
    keypoint with no valid sample, or on a flat patch, has angle 0."""
    got, pts, off = _sift_batch_args(imgs, pts, lengths, "sift_orient_batch")
    ptrs, hs, ws, cs = _image_table(got)
    angles = np.empty(len(pts), np.float32)
    check(lib().apap_sift_orient_batch(_h(ctx), ptrs, _ip(hs), _ip(ws), _ip(cs), len(got), _ptr(pts, C.c_float), _ip(off),
                                       _ptr(angles, C.c_float), device))
    return angles


def sift_orient(img, pts, device=-1, ctx=None):
    """``apap_sift_orient``: float32 (n,) orientations at ``pts`` (n, 2) of one uint8 image (see ``sift_orient_batch``)."""
    return sift_orient_batch([img], pts, [len(as_sift_points(pts))], device=device, ctx=ctx)


def sift_describe_oriented_batch(imgs, pts, lengths, angles=None, device=-1, ctx=None):
    """``apap_sift_describe_oriented_batch``: the SIFT descriptors of ``KeyPoint(x, y, 1, angle)``, many images in one call.
    ``angles`` (N,) in [0, 360]: returns float32 (N, 128).  ``angles=None``: orientation and descriptor in one pass; returns
    ``(feats, angles)``, the same bytes as ``sift_orient_batch`` followed by the call with its angles."""
    got, pts, off = _sift_batch_args(imgs, pts, lengths, "sift_describe_oriented_batch")
    ptrs, hs, ws, cs = _image_table(got)
    out = np.empty((len(pts), SIFT_DIM), np.float32)
    given = None if angles is None else as_sift_angles(angles, len(pts))
    found = np.empty(len(pts), np.float32) if angles is None else None
    check(lib().apap_sift_describe_oriented_batch(
        _h(ctx), ptrs, _ip(hs), _ip(ws), _ip(cs), len(got), _ptr(pts, C.c_float), _ip(off),
        None if given is None else _ptr(given, C.c_float), None if found is None else _ptr(found, C.c_float), _ptr(out, C.c_float), device))
    return out if angles is not None else (out, found)


def sift_describe_oriented(img, pts, angles=None, device=-1, ctx=None):
    """``apap_sift_describe_oriented``: one image (see ``sift_describe_oriented_batch``; the single call is the batch of one)."""
    return sift_describe_oriented_batch([img], pts, [len(as_sift_points(pts))], angles=angles, device=device, ctx=ctx)


# ---------------------------------------------------------------- corner detection: exact integer Harris corners
CORNER_TILE_W, CORNER_TILE_H = 64, 32   # APAP_CORNER_TILE_W, APAP_CORNER_TILE_H
CORNER_MAX_RADIUS = 16                  # APAP_CORNER_MAX_RADIUS
CORNER_MAX_IMAGES = 65535


def corner_bound(h, w, radius):
    """``ceil(h / (radius + 1)) * ceil(w / (radius + 1))``: no image of that shape has more corners."""
    s = int(radius) + 1
    return -(-int(h) // s) * -(-int(w) // s)


def corner_params(max_corners, radius, quality_permille, who="corner_detect"):
    """The three parameters as ints, checked as the library checks them."""
    max_corners, radius, quality_permille = int(max_corners), int(radius), int(quality_permille)
    if max_corners < 1:
        raise ValueError(f"{who}: max_corners must be >= 1; got {max_corners}")
    if not 1 <= radius <= CORNER_MAX_RADIUS:
        raise ValueError(f"{who}: radius must be 1 .. {CORNER_MAX_RADIUS}; got {radius}")
    if not 0 <= quality_permille <= 1000:
        raise ValueError(f"{who}: quality_permille must be 0 .. 1000; got {quality_permille}")
    return max_corners, radius, quality_permille


def corner_detect_batch(imgs, max_corners, radius=5, quality_permille=10, device=-1, ctx=None, full=False):
    """``apap_corner_detect_batch``: exact integer Harris corners (include/apap_hip.h "corner detection") of many images in
    one call (two kernel launches, whatever their number).  ``imgs``: a sequence of (h, w) grey or (h, w, 3) BGR uint8 arrays
    of any shapes.  Returns a list of ``(pts, response)`` per image: float32 (n, 2) integer-valued (x, y) and int64 (n,), by
    response descending then index ascending, ``n <= max_corners``; an image's outputs equal its own single call's byte for
    byte.  ``max_corners`` beyond the largest image's bound on the corner count asks for no more rows than that bound.
    With ``full``: the slabs as the library wrote them, ``(pts (n, rows, 2), response (n, rows), count (n,))``."""
    got = [as_sift_image(im, f"imgs[{m}]") for m, im in enumerate(imgs)]
    if not 1 <= len(got) <= CORNER_MAX_IMAGES:
        raise ValueError(f"corner_detect_batch: {len(got)} images (1 .. {CORNER_MAX_IMAGES})")
    max_corners, radius, quality_permille = corner_params(max_corners, radius, quality_permille, "corner_detect_batch")
    rows = min(max_corners, max(corner_bound(a.shape[0], a.shape[1], radius) for a, _ in got))
    ptrs, hs, ws, cs = _image_table(got)
    pts = np.empty((len(got), rows, 2), np.float32)
    resp = np.empty((len(got), rows), np.int64)
    count = np.empty(len(got), np.int32)
    check(lib().apap_corner_detect_batch(_h(ctx), ptrs, _ip(hs), _ip(ws), _ip(cs), len(got), rows, radius, quality_permille,
                                         _ptr(pts, C.c_float), _ptr(resp, C.c_longlong), _ip(count), device))
    if full:
        return pts, resp, count
    return [(pts[m, :count[m]].copy(), resp[m, :count[m]].copy()) for m in range(len(got))]


def corner_detect(img, max_corners, radius=5, quality_permille=10, device=-1, ctx=None, full=False):
    """``apap_corner_detect``: the exact integer Harris corners of one uint8 image, (h, w) grey or (h, w, 3) BGR: ``(pts,
    response)`` trimmed to the count - float32 (n, 2) integer-valued (x, y), directly usable as keypoints of ``sift_describe``,
    and int64 (n,) responses, by response descending then index ascending.  An image without corners gives two empty arrays.
    With ``full``: ``(pts, response, count)`` as the library wrote them, all ``max_corners`` rows (zero from ``count`` on)."""
    img, ch = as_sift_image(img)
    max_corners, radius, quality_permille = corner_params(max_corners, radius, quality_permille)
    rows = max_corners if full else min(max_corners, corner_bound(img.shape[0], img.shape[1], radius))
    pts = np.empty((rows, 2), np.float32)
    resp = np.empty(rows, np.int64)
    count = C.c_int(-1)
    check(lib().apap_corner_detect(_h(ctx), _ptr(img, C.c_uint8), img.shape[0], img.shape[1], ch, rows, radius, quality_permille,
                                   _ptr(pts, C.c_float), _ptr(resp, C.c_longlong), C.byref(count), device))
    if full:
        return pts, resp, count.value
    return pts[:count.value].copy(), resp[:count.value].copy()


# ---------------------------------------------------------------- image pyramid: levels at scales 2^-k and (3/4) 2^-k
PYRAMID_MAX_LEVELS = 16                 # APAP_PYRAMID_MAX_LEVELS
PYRAMID_MIN_SIDE = 32                   # APAP_PYRAMID_MIN_SIDE
PYRAMID_TILE_W, PYRAMID_TILE_H = 64, 32   # APAP_PYRAMID_TILE_W, APAP_PYRAMID_TILE_H: the source tile of a block


def pyramid_levels_arg(n_levels, who="pyramid"):
    n_levels = int(n_levels)
    if not 1 <= n_levels <= PYRAMID_MAX_LEVELS:
        raise ValueError(f"{who}: levels must be 1 .. {PYRAMID_MAX_LEVELS}; got {n_levels}")
    return n_levels


def as_pyramid_image(img, name="img"):
    """``as_sift_image`` with the pyramid's smallest side, 32."""
    img, ch = as_sift_image(img, name)
    if min(img.shape[:2]) < PYRAMID_MIN_SIDE:
        raise ValueError(f"{name}: sides must be {PYRAMID_MIN_SIDE} .. {SIFT_MAX_SIDE}; got {img.shape[:2]}")
    return img, ch


def pyramid_layout(h, w, n_levels=6, half_steps=True):
    """``apap_pyramid_layout`` (host only): ``(heights, widths, offsets, scale_num, scale_shift)`` of the levels that exist,
    at most ``n_levels`` - int32 arrays of their number, ``offsets`` int64 with one more entry: level l lies at byte
    ``offsets[l]`` of the level buffer, whose size is ``offsets[-1]``; its scale is ``scale_num[l] / 2 ** scale_shift[l]``."""
    n_levels = pyramid_levels_arg(n_levels, "pyramid_layout")
    hs, ws, num, shift = (np.zeros(n_levels, np.int32) for _ in range(4))
    off = np.zeros(n_levels + 1, np.int64)
    n = lib().apap_pyramid_layout(int(h), int(w), n_levels, int(bool(half_steps)), _ip(hs), _ip(ws), _ptr(off, C.c_longlong), _ip(num),
                                  _ip(shift))
    if n < 1:
        raise ApapValueError(ERR_INVALID_ARG, lib().apap_last_error().decode("utf-8", "replace"))
    return hs[:n].copy(), ws[:n].copy(), off[:n + 1].copy(), num[:n].copy(), shift[:n].copy()


def pyramid_level_caps(max_corners, n_levels=6, half_steps=True):
    """``apap_pyramid_level_caps`` (host only): the corner budget of every level, int32 (n_levels,) - a constant number of
    corners per unit area, at least 16 and at most ``max_corners``."""
    n_levels = pyramid_levels_arg(n_levels, "pyramid_level_caps")
    caps = np.zeros(n_levels, np.int32)
    check(lib().apap_pyramid_level_caps(int(max_corners), n_levels, int(bool(half_steps)), _ip(caps)))
    return caps


def pyramid_batch(imgs, n_levels=6, half_steps=True, device=-1, ctx=None):
    """``apap_pyramid_build_batch``: the grey pyramids of many uint8 pictures, (h, w) grey or (h, w, 3) BGR of any shapes from
    32 a side, in one call (1 + ceil((n_levels - 1) / 2) kernel launches at most, whatever their number).  Returns a list per
    picture of its levels, uint8 (h_l, w_l) arrays: level 0 the grey picture, even levels halved k times, odd levels the
    3/4 reduction halved k times (``half_steps=False``: halvings only); fewer than ``n_levels`` where the next level would
    have a side under 32.  A picture's levels equal its own single call's byte for byte."""
    n_levels = pyramid_levels_arg(n_levels, "pyramid_batch")
    got = [as_pyramid_image(im, f"imgs[{m}]") for m, im in enumerate(imgs)]
    if not 1 <= len(got) <= CORNER_MAX_IMAGES:
        raise ValueError(f"pyramid_batch: {len(got)} images (1 .. {CORNER_MAX_IMAGES})")
    lays = [pyramid_layout(a.shape[0], a.shape[1], n_levels, half_steps) for a, _ in got]
    buf = np.empty(sum(int(lay[2][-1]) for lay in lays), np.uint8)
    ptrs, hs, ws, cs = _image_table(got)
    check(lib().apap_pyramid_build_batch(_h(ctx), ptrs, _ip(hs), _ip(ws), _ip(cs), len(got), n_levels, int(bool(half_steps)),
                                         _ptr(buf, C.c_uint8), device))
    out, at = [], 0
    for lh, lw, off, _, _ in lays:
        out.append([buf[at + off[k]:at + off[k] + int(lh[k]) * int(lw[k])].reshape(lh[k], lw[k]).copy() for k in range(len(lh))])
        at += int(off[-1])
    return out


def pyramid(img, n_levels=6, half_steps=True, device=-1, ctx=None):
    """``apap_pyramid_build``: the list of grey levels of one uint8 picture (see ``pyramid_batch``; the batch of one)."""
    return pyramid_batch([img], n_levels, half_steps, device=device, ctx=ctx)[0]


def pyramid_keypoints(slab_pts, slab_response, counts, scale_num, scale_shift, level_index, device=-1, ctx=None):
    """``apap_pyramid_keypoints``: the pack.  ``slab_pts`` (n, rows, 2) float32 and ``slab_response`` (n, rows) int64: the
    batched detector's slabs over n level images; ``counts`` (n,): the rows to keep of each (the detector's count clamped to
    the level's cap); ``scale_num``, ``scale_shift``, ``level_index`` (n,): each level image's scale and level number.
    Returns ``(pts, level_pts, level, response, level_offset)``: float32 (N, 2) base-frame coordinates, float32 (N, 2) level
    coordinates, int32 (N,), int64 (N,) and int32 (n + 1,) offsets."""
    slab_pts = np.ascontiguousarray(slab_pts, dtype=np.float32)
    slab_response = np.ascontiguousarray(slab_response, dtype=np.int64)
    if slab_pts.ndim != 3 or slab_pts.shape[2] != 2 or slab_response.shape != slab_pts.shape[:2] or slab_pts.shape[1] < 1:
        raise ValueError(f"pyramid_keypoints: slabs must be (n, rows, 2) and (n, rows); got {slab_pts.shape} and {slab_response.shape}")
    n, rows = slab_pts.shape[:2]
    counts, num, shift, index = (_i32(np.asarray(a).reshape(-1)) for a in (counts, scale_num, scale_shift, level_index))
    if not 1 <= n <= CORNER_MAX_IMAGES or any(len(a) != n for a in (counts, num, shift, index)):
        raise ValueError(f"pyramid_keypoints: {n} level images (1 .. {CORNER_MAX_IMAGES}) need as many counts, scales and indices")
    if counts.min() < 0 or counts.max() > rows:
        raise ValueError(f"pyramid_keypoints: counts must be 0 .. {rows}; got {counts.tolist()}")
    N = int(counts.sum())
    pts, lpts = np.empty((N, 2), np.float32), np.empty((N, 2), np.float32)
    level, resp, off = np.empty(N, np.int32), np.empty(N, np.int64), np.empty(n + 1, np.int32)
    check(lib().apap_pyramid_keypoints(_h(ctx), _ptr(slab_pts, C.c_float), _ptr(slab_response, C.c_longlong), rows, _ip(counts), _ip(num),
                                       _ip(shift), _ip(index), n, _ptr(pts, C.c_float), _ptr(lpts, C.c_float), _ip(level),
                                       _ptr(resp, C.c_longlong), _ip(off), device))
    return pts, lpts, level, resp, off


# ---------------------------------------------------------------- global warp and blend: image_warping of utils.py:93-127
IMAGE_WARP_MAX_SIDE = 32767         # APAP_IMAGE_WARP_MAX_SIDE
IMAGE_WARP_MAX_PROBLEMS = 65535     # APAP_IMAGE_WARP_MAX_PROBLEMS


def as_warp_image(img, name="img"):
    """An (h, w, 3) uint8 picture, contiguous; every other dtype or shape is a ValueError (the reference's blend loop and
    three-channel paste take nothing else)."""
    img = np.asarray(img)
    if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] != 3:
        raise ValueError(f"{name} must be (h, w, 3) uint8; got {img.dtype} {img.shape}")
    if not all(1 <= x <= IMAGE_WARP_MAX_SIDE for x in img.shape[:2]):
        raise ValueError(f"{name}: sides must be 1 .. {IMAGE_WARP_MAX_SIDE}; got {img.shape[:2]}")
    return np.ascontiguousarray(img)


def as_homography(H, name="H"):
    """A 3 x 3 homography in its own float dtype (float32 stays float32: the reference multiplies it as it is)."""
    H = np.asarray(H)
    if H.shape != (3, 3):
        raise ValueError(f"{name} must be 3 x 3; got {H.shape}")
    return H if H.dtype in (np.float32, np.float64) else H.astype(np.float64)


def image_warp_bounds(h1, w1, h2, w2, H):
    """``apap_image_warp_bounds`` (host only): (xmin, ymin, xmax, ymax) of utils.py:101-106 for an h1 x w1 base picture and an
    h2 x w2 picture warped by ``H``.  A canvas with a side outside 1 .. 32767, or a non-finite corner, is a ValueError."""
    H = np.ascontiguousarray(as_homography(H), dtype=np.float64)
    out = np.empty(4, np.int32)
    check(lib().apap_image_warp_bounds(int(h1), int(w1), int(h2), int(w2), _ptr(H, C.c_double), _ptr(out, C.c_int)))
    return tuple(int(v) for v in out)


def image_warp_geometry(h1, w1, h2, w2, H):
    """What utils.py:99-114 derives from the shapes and ``H``: ``(M, canvas_w, canvas_h, off_x, off_y)`` with ``M`` the
    reference's own ``Ht.dot(H)`` as contiguous float64 (the native layer never forms it: no BLAS summation order in the C
    contract)."""
    H = as_homography(H)
    xmin, ymin, xmax, ymax = image_warp_bounds(h1, w1, h2, w2, H)
    t = [-xmin, -ymin]
    Ht = np.array([
        [1, 0, t[0]],
        [0, 1, t[1]],
        [0, 0, 1]])
    M = np.ascontiguousarray(Ht.dot(H), dtype=np.float64)
    return M, xmax - xmin, ymax - ymin, t[0], t[1]


def image_warp_tables(shapes_base, shapes_src, Ms, canvases, offsets, directs, out_offsets=None, who="image_warp_batch"):
    """The host arrays of the batch entry points from per-problem lists: ``(n, base_h, base_w, src_h, src_w, M, canvas_w,
    canvas_h, off_x, off_y, direct, out_offset, sizes)``; ``out_offsets`` default to the canvases packed back to back."""
    n = len(Ms)
    if not 1 <= n <= IMAGE_WARP_MAX_PROBLEMS:
        raise ValueError(f"{who}: {n} problems (1 .. {IMAGE_WARP_MAX_PROBLEMS})")
    if not all(len(x) == n for x in (shapes_base, shapes_src, canvases, offsets, directs)):
        raise ValueError(f"{who}: the per-problem lists differ in length")
    M = np.ascontiguousarray(np.stack([np.asarray(m, np.float64).reshape(3, 3) for m in Ms]), dtype=np.float64)
    cw, ch = _i32([c[0] for c in canvases]), _i32([c[1] for c in canvases])
    sizes = [int(h) * int(w) * 3 for w, h in canvases]
    if out_offsets is None:
        out_offsets = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    off = np.ascontiguousarray(out_offsets, dtype=np.int64)
    if off.shape != (n,):
        raise ValueError(f"{who}: {n} problems, out_offsets of shape {off.shape}")
    return (n, _i32([s[0] for s in shapes_base]), _i32([s[1] for s in shapes_base]), _i32([s[0] for s in shapes_src]),
            _i32([s[1] for s in shapes_src]), M, cw, ch, _i32([o[0] for o in offsets]), _i32([o[1] for o in offsets]),
            _i32([1 if d else 0 for d in directs]), off, sizes)


def image_warp_batch(bases, srcs, Ms, canvases, offsets, directs, out=None, out_offsets=None, device=-1, ctx=None):
    """``apap_image_warp_batch``: many global warps and blends in one kernel launch.  Per problem: ``bases[p]`` and ``srcs[p]``
    (h, w, 3) uint8 (problems may share pictures: the same array is uploaded once), ``Ms[p]`` 3 x 3 float64 (canvas <- source),
    ``canvases[p]`` = (width, height), ``offsets[p]`` = (off_x, off_y) of the base picture, ``directs[p]`` the blend mode.
    ``out``: a flat contiguous uint8 array receiving problem p's canvas at byte ``out_offsets[p]`` (default: a new array, the
    canvases back to back).  Returns the list of canvases, views of ``out``; each equals its own single call's byte for byte."""
    bases = [as_warp_image(b, f"bases[{p}]") for p, b in enumerate(bases)]
    srcs = [as_warp_image(s, f"srcs[{p}]") for p, s in enumerate(srcs)]
    n, bh, bw, sh, sw, M, cw, ch, ox, oy, direct, off, sizes = image_warp_tables(
        [b.shape for b in bases], [s.shape for s in srcs], Ms, canvases, offsets, directs, out_offsets)
    if (cw < 1).any() or (ch < 1).any() or (cw > IMAGE_WARP_MAX_SIDE).any() or (ch > IMAGE_WARP_MAX_SIDE).any():
        raise ValueError(f"image_warp_batch: canvas sides must be 1 .. {IMAGE_WARP_MAX_SIDE}")
    if (off < 0).any():
        raise ValueError("image_warp_batch: negative output offset")
    need = int(max(o + s for o, s in zip(off, sizes)))
    if out is None:
        out = np.empty(need, np.uint8)
    if not isinstance(out, np.ndarray) or out.dtype != np.uint8 or out.ndim != 1 or not out.flags.c_contiguous or out.size < need:
        raise ValueError(f"image_warp_batch: out must be a flat contiguous uint8 array of at least {need} bytes")
    check(lib().apap_image_warp_batch(_h(ctx), _addrs([a.ctypes.data for a in bases]), _ip(bh), _ip(bw),
                                      _addrs([a.ctypes.data for a in srcs]), _ip(sh), _ip(sw), _dp(M), _ip(cw), _ip(ch), _ip(ox), _ip(oy),
                                      _ip(direct), n, _ptr(out, C.c_uint8), _ptr(off, C.c_longlong), device))
    return [out[int(o):int(o) + s].reshape(int(h), int(w), 3) for o, s, w, h in zip(off, sizes, cw, ch)]


def image_warp(base, src, M, canvas_w, canvas_h, off_x, off_y, direct_blend=True, device=-1, ctx=None):
    """``apap_image_warp``: ``src`` warped by ``M`` (3 x 3 float64, canvas <- source) onto a canvas_h x canvas_w canvas, ``base``
    pasted (``direct_blend``) or mean-blended at (off_x, off_y): (canvas_h, canvas_w, 3) uint8."""
    base, src = as_warp_image(base, "base"), as_warp_image(src, "src")
    M = np.ascontiguousarray(np.asarray(M, np.float64).reshape(3, 3))
    canvas_w, canvas_h = int(canvas_w), int(canvas_h)
    if not (1 <= canvas_w <= IMAGE_WARP_MAX_SIDE and 1 <= canvas_h <= IMAGE_WARP_MAX_SIDE):
        raise ValueError(f"image_warp: canvas sides must be 1 .. {IMAGE_WARP_MAX_SIDE}; got {canvas_h} x {canvas_w}")
    out = np.empty((canvas_h, canvas_w, 3), np.uint8)
    check(lib().apap_image_warp(_h(ctx), _ptr(base, C.c_uint8), base.shape[0], base.shape[1], _ptr(src, C.c_uint8), src.shape[0],
                                src.shape[1], _ptr(M, C.c_double), canvas_w, canvas_h, int(off_x), int(off_y), 1 if direct_blend else 0,
                                _ptr(out, C.c_uint8), device))
    return out


# ---------------------------------------------------------------- panorama: every view of a case on one canvas
PANORAMA_MAX_LAYERS = 16            # APAP_PANORAMA_MAX_LAYERS
PANORAMA_MEAN, PANORAMA_PASTE = 0, 1
PANORAMA_MODES = {"mean": PANORAMA_MEAN, "paste": PANORAMA_PASTE}
PANORAMA_MAX_RAMP = 256             # APAP_PANORAMA_MAX_RAMP


class PanoramaLayer(NamedTuple):
    """One neighbour of a panorama: what ``APAP.local_warp`` takes for its pair.  ``img`` (h, w, 3) uint8, ``local_homography``
    the forward grid (rows, cols, 3, 3) float32, ``mesh`` = (mesh_w, mesh_h) edges, ``final_size`` = (width, height) of the
    pair canvas, ``offset`` = (x, y) of the centre picture on it."""
    img: object
    local_homography: object
    mesh: object
    final_size: object
    offset: object


def panorama_mode(blend, who="panorama"):
    if blend not in PANORAMA_MODES:
        raise ValueError(f"{who}: blend must be 'mean', 'paste', 'ramp' or 'band'; got {blend!r}")
    return PANORAMA_MODES[blend]


def panorama_entry(blend, ramp, who="panorama", device_form=False):
    """The C entry point of ``blend`` and its mode argument: ``apap_panorama[_device]`` with the mode of 'mean' or 'paste' (``ramp``
    is ignored), ``apap_panorama_ramp[_device]`` with the ramp width for 'ramp' - an integer 1 .. 256, or ValueError."""
    suffix = "_device" if device_form else ""
    if blend != "ramp":
        return getattr(lib(), "apap_panorama" + suffix), panorama_mode(blend, who)
    if isinstance(ramp, bool) or not isinstance(ramp, (int, np.integer)) or not 1 <= ramp <= PANORAMA_MAX_RAMP:
        raise ValueError(f"{who}: ramp must be an integer 1 .. {PANORAMA_MAX_RAMP}; got {ramp!r}")
    return getattr(lib(), "apap_panorama_ramp" + suffix), int(ramp)


def panorama_geometry(layers, who="panorama"):
    """The int32 tables (final_w, final_h, off_x, off_y) of ``layers`` (PanoramaLayer-like objects or 5-tuples)."""
    layers = [l if isinstance(l, PanoramaLayer) else PanoramaLayer(*l) for l in layers]
    if not 1 <= len(layers) <= PANORAMA_MAX_LAYERS:
        raise ValueError(f"{who}: {len(layers)} layers (1 .. {PANORAMA_MAX_LAYERS})")
    geo = np.array([[int(l.final_size[0]), int(l.final_size[1]), int(l.offset[0]), int(l.offset[1])] for l in layers], dtype=np.int64)
    if np.abs(geo).max() >= 2 ** 31:
        raise ValueError(f"{who}: canvas geometry beyond int32")
    return layers, [np.ascontiguousarray(geo[:, k], dtype=np.int32) for k in range(4)]


def panorama_bounds(center_shape, final_w, final_h, off_x, off_y):
    """``apap_panorama_bounds`` (host only): (W, H, OX, OY) of the union canvas; ValueError when the centre does not fit a
    pair canvas or the canvas has 2^31 pixels or more."""
    arrs = [np.ascontiguousarray(a, dtype=np.int32) for a in (final_w, final_h, off_x, off_y)]
    out = np.zeros(4, np.int32)
    check(lib().apap_panorama_bounds(int(center_shape[0]), int(center_shape[1]), *[_ptr(a, C.c_int) for a in arrs], int(arrs[0].size),
                                     _ptr(out, C.c_int)))
    return tuple(int(v) for v in out)


def panorama_mean_of(total, count):
    """``apap_panorama_mean_of``: the kernel's multiply-and-shift division on the host."""
    return int(lib().apap_panorama_mean_of(int(total), int(count)))


def panorama_ramp_weight(x, y, w, h, ramp):
    """``apap_panorama_ramp_weight`` (host only): the weight of pixel (x, y) of a w x h picture."""
    return int(lib().apap_panorama_ramp_weight(int(x), int(y), int(w), int(h), int(ramp)))


def panorama_ramp_quotients(total, wsum):
    """``apap_panorama_ramp_quotients``: the ramp kernel's division on the host, element by element (uint32 arrays)."""
    total = np.ascontiguousarray(total, dtype=np.uint32)
    wsum = np.ascontiguousarray(wsum, dtype=np.uint32)
    if total.shape != wsum.shape:
        raise ValueError(f"panorama_ramp_quotients: {total.shape} sums and {wsum.shape} weight sums")
    out = np.zeros(total.shape, np.uint32)
    lib().apap_panorama_ramp_quotients(_ptr(total, C.c_uint), _ptr(wsum, C.c_uint), int(total.size), _ptr(out, C.c_uint))
    return out


PANORAMA_RAMP = 2                    # APAP_PANORAMA_RAMP: a mode of the gain entry points only
PANORAMA_GAIN_MAX_STEP = 64         # APAP_PANORAMA_GAIN_MAX_STEP
PANORAMA_GAIN_MIN_Q, PANORAMA_GAIN_MAX_Q = 1024, 16383


class PanoramaGains(NamedTuple):
    """Gain compensation of a panorama's K + 1 views (the centre first): ``gains`` float64, ``q = clamp(rint(4096 gains), 1024,
    16383)`` int32, and the overlap statistics ``N``, ``S`` (K + 1, K + 1) uint64 they were fitted to."""
    gains: object
    q: object
    N: object
    S: object


def panorama_gain_mode(blend, ramp, who="panorama"):
    """(mode, ramp) of the gain entry points, which take the ramp as a mode."""
    if blend != "ramp":
        return panorama_mode(blend, who), 0
    panorama_entry(blend, ramp, who)
    return PANORAMA_RAMP, int(ramp)


def panorama_gain_q(gain_q, n_views, who="panorama"):
    """``gain_q`` as the int32 array of ``n_views`` values the library takes (it checks their range)."""
    q = np.asarray(gain_q)
    if q.shape != (n_views,) or q.dtype.kind not in "iu":
        raise ValueError(f"{who}: gain_q must be {n_views} integers (the centre, then every layer); got {gain_q!r}")
    if (q < -2 ** 31).any() or (q >= 2 ** 31).any():
        raise ValueError(f"{who}: gain_q beyond int32")
    return np.ascontiguousarray(q, dtype=np.int32)


def panorama_gain_apply(values, q):
    """``apap_panorama_gain_apply`` (host only): ``min(255, (c q + 2048) >> 12)`` of every byte of ``values``."""
    values = np.ascontiguousarray(values, dtype=np.uint8)
    out = np.empty_like(values)
    check(lib().apap_panorama_gain_apply(_ptr(values, C.c_uint8), int(values.size), int(q), _ptr(out, C.c_uint8)))
    return out


def panorama_gain_solve(N, S, sigma_n=10.0, sigma_g=0.1):
    """``apap_panorama_gain_solve`` (host only): ``(g float64, q int32, flag)`` of the (V, V) uint64 overlap statistics - the
    bits the device solve of the resident chain gives."""
    N, S = np.ascontiguousarray(N, dtype=np.uint64), np.ascontiguousarray(S, dtype=np.uint64)
    if N.ndim != 2 or N.shape[0] != N.shape[1] or S.shape != N.shape:
        raise ValueError(f"panorama_gain_solve: N and S must be (V, V); got {N.shape} and {S.shape}")
    v = N.shape[0]
    g, q, flag = np.zeros(v, np.float64), np.zeros(v, np.int32), np.zeros(1, np.int32)
    check(lib().apap_panorama_gain_solve(_ptr(N, C.c_ulonglong), _ptr(S, C.c_ulonglong), v, float(sigma_n), float(sigma_g),
                                         _ptr(g, C.c_double), _ip(q), _ip(flag)))
    return g, q, int(flag[0])


def _panorama_inputs(center, layers, who):
    """The host arrays of a panorama call and its leading C arguments after the context: (args, keep-alive, n, bounds)."""
    layers, (fw, fh, ox, oy) = panorama_geometry(layers, who)
    n = len(layers)
    center = np.ascontiguousarray(center, dtype=np.uint8)
    if center.ndim != 3 or center.shape[2] != 3:
        raise ValueError(f"{who}: the centre must be (h, w, 3); got {center.shape}")
    imgs, grids, mws, mhs = [], [], [], []
    for k, l in enumerate(layers):
        img = np.ascontiguousarray(l.img, dtype=np.uint8)
        if img.ndim != 3 or img.shape[2] != 3:
            raise ValueError(f"{who}: layer {k}: the picture must be (h, w, 3); got {img.shape}")
        H = as_f32(l.local_homography, (3, 3))
        if H.ndim != 4:
            raise ValueError(f"{who}: layer {k}: the grid must be (rows, cols, 3, 3); got {H.shape}")
        imgs.append(img)
        grids.append(H)
        mws.append(np.ascontiguousarray(l.mesh[0], dtype=np.float64))
        mhs.append(np.ascontiguousarray(l.mesh[1], dtype=np.float64))
    ih, iw = _i32([a.shape[0] for a in imgs]), _i32([a.shape[1] for a in imgs])
    mr, mc = _i32([a.shape[0] for a in grids]), _i32([a.shape[1] for a in grids])
    nw, nh = _i32([a.size for a in mws]), _i32([a.size for a in mhs])
    bounds = panorama_bounds(center.shape, fw, fh, ox, oy)
    p = [_addrs([a.ctypes.data for a in arrs]) for arrs in (imgs, grids, mws, mhs)]
    args = [_ptr(center, C.c_uint8), center.shape[0], center.shape[1], p[0], _ip(ih), _ip(iw), p[1], _ip(mr), _ip(mc),
            p[2], _ip(nw), p[3], _ip(nh), _ip(fw), _ip(fh), _ip(ox), _ip(oy), n]
    return args, (center, imgs, grids, mws, mhs, ih, iw, mr, mc, nw, nh, fw, fh, ox, oy, p), n, bounds


def _gain_step(step, who):
    if isinstance(step, bool) or not isinstance(step, (int, np.integer)):
        raise ValueError(f"{who}: the lattice step must be an integer 1 .. {PANORAMA_GAIN_MAX_STEP}; got {step!r}")
    return int(step)


def panorama_gain_stats(center, layers, step=4, device=-1, ctx=None, sampling=None):
    """``apap_panorama_gain_stats``: ``(N, S)``, the (K + 1, K + 1) uint64 overlap statistics of the centre and the layers over
    the canvas pixels with ``X % step == 0 and Y % step == 0``."""
    who = "panorama_gain_stats"
    step = _gain_step(step, who)
    with sampling_scope(ctx, sampling, who) as ctx:
        args, keep, n, _ = _panorama_inputs(center, layers, who)
        N, S = np.zeros((n + 1, n + 1), np.uint64), np.zeros((n + 1, n + 1), np.uint64)
        status = np.zeros(n, np.int32)
        check(lib().apap_panorama_gain_stats(_h(ctx), *args, step, _ptr(N, C.c_ulonglong), _ptr(S, C.c_ulonglong), _ip(status), device))
    return N, S


PANORAMA_BAND = 3                   # APAP_PANORAMA_BAND: the two-band blend's kernel mode; no entry point takes it as a mode
PANORAMA_MAX_BAND = 32              # APAP_PANORAMA_MAX_BAND


def panorama_band_radius(band, who="panorama"):
    """``band`` of the two-band blend as an int 0 .. 32, or ValueError."""
    if isinstance(band, bool) or not isinstance(band, (int, np.integer)) or not 0 <= band <= PANORAMA_MAX_BAND:
        raise ValueError(f"{who}: band must be an integer 0 .. {PANORAMA_MAX_BAND}; got {band!r}")
    return int(band)


def box_blur(img, radius, device=-1, ctx=None):
    """``apap_box_blur``: the low-pass picture of the two-band blend, ``(T + (n^2 >> 1)) // n^2`` with ``n = 2 radius + 1`` and T
    the sum over the n x n window with the border replicated; ``img`` (h, w, 3) uint8, ``radius`` 0 .. 32."""
    radius = panorama_band_radius(radius, "box_blur")
    img = np.ascontiguousarray(img, dtype=np.uint8)
    if img.ndim != 3 or img.shape[2] != 3:
        raise ValueError(f"box_blur: the picture must be (h, w, 3); got {img.shape}")
    out = np.empty_like(img)
    check(lib().apap_box_blur(_h(ctx), _ptr(img, C.c_uint8), img.shape[0], img.shape[1], radius, _ptr(out, C.c_uint8), device))
    return out


def panorama(center, layers, blend="mean", device=-1, ctx=None, return_status=False, ramp=32, sampling=None, gain_q=None, band=8):
    """See :func:`_panorama`; ``sampling``: ``None`` (the context's ``warp_sampling``), ``"nearest"`` or ``"bilinear"`` for this
    call only - every layer is then sampled that way.  ``gain_q``: ``None``, or K + 1 integers 1024 .. 16383 (4096 = 1.0), the
    gain of the centre and of every layer (``apap_panorama_gain``; ``apap_panorama_band`` takes them itself).  ``band``: the
    radius 0 .. 32 of the low-pass pictures of ``blend="band"``; every other blend ignores it."""
    with sampling_scope(ctx, sampling, "panorama") as ctx:
        return _panorama(center, layers, blend, device, ctx, return_status, ramp, gain_q, band)


def panorama_auto_gain(center, layers, blend="mean", device=-1, ctx=None, ramp=32, sampling=None, step=4, sigma_n=10.0, sigma_g=0.1):
    """``apap_panorama_auto_gain``: the statistics, the solve and the gained blend in one call.  Returns ``(canvas, (W, H, OX,
    OY), PanoramaGains)``."""
    who = "panorama"
    step = _gain_step(step, who)
    mode, width = panorama_gain_mode(blend, ramp, who)
    with sampling_scope(ctx, sampling, who) as ctx:
        args, keep, n, (W, Hc, OX, OY) = _panorama_inputs(center, layers, who)
        out = np.empty((Hc, W, 3), np.uint8)
        N, S = np.zeros((n + 1, n + 1), np.uint64), np.zeros((n + 1, n + 1), np.uint64)
        g, q, flag, status = np.zeros(n + 1, np.float64), np.zeros(n + 1, np.int32), np.zeros(1, np.int32), np.zeros(n, np.int32)
        check(lib().apap_panorama_auto_gain(_h(ctx), *args, mode, width, step, float(sigma_n), float(sigma_g), _ptr(out, C.c_uint8),
                                            _ptr(N, C.c_ulonglong), _ptr(S, C.c_ulonglong), _ptr(g, C.c_double), _ip(q), _ip(flag),
                                            _ip(status), device))
    return out, (W, Hc, OX, OY), PanoramaGains(g, q, N, S)


def _panorama(center, layers, blend, device, ctx, return_status, ramp, gain_q=None, band=8):
    """``apap_panorama`` (``blend`` 'mean' or 'paste'), ``apap_panorama_ramp`` ('ramp', with the ramp width ``ramp``, which 'mean'
    and 'paste' ignore) or ``apap_panorama_band`` ('band', with ``ramp`` and the radius ``band``): the centre picture and every
    layer (a :class:`PanoramaLayer` or a 5-tuple in its order) on one canvas.
    Returns ``(canvas (H, W, 3) uint8, (W, H, OX, OY))`` - with ``return_status=True`` also the per-layer status words, and
    then a status does not raise.  Neither the grids nor any other input is modified."""
    who = "panorama"
    if blend == "band":
        panorama_entry("ramp", ramp, who)
        entry = lib().apap_panorama_band
        tail = [int(ramp), panorama_band_radius(band, who)]
    elif gain_q is None:
        entry, mode = panorama_entry(blend, ramp, who)
        tail = [mode]
    else:
        entry = lib().apap_panorama_gain
        tail = list(panorama_gain_mode(blend, ramp, who))
    args, keep, n, (W, Hc, OX, OY) = _panorama_inputs(center, layers, who)
    if gain_q is not None:
        q = panorama_gain_q(gain_q, n + 1, who)
        tail.append(_ip(q))
    elif blend == "band":
        tail.append(None)       # apap_panorama_band takes NULL for no gains
    out = np.empty((Hc, W, 3), np.uint8)
    status = np.zeros(n, np.int32)
    code = entry(_h(ctx), *args, *tail, _ptr(out, C.c_uint8), _ip(status), device)
    if return_status and code in (ERR_SINGULAR, ERR_INDEX):
        return out, (W, Hc, OX, OY), status
    check(code)
    return (out, (W, Hc, OX, OY), status) if return_status else (out, (W, Hc, OX, OY))
