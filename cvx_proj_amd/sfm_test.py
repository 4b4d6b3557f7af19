"""Drop-in for the reference's ``pyviz/sfm_test.py``: co-visibility tracks over the pairs of a case and the 3-D point of
every track, on the GPU (csrc/apap_sfm.hip through ``_native.covis_tracks`` / ``_native.triangulate_tracks``; the resident
forms are ``resident.hip_covis_tracks`` / ``hip_triangulate_rays`` / ``hip_triangulate_tracks``).  No CPU fallback.

Same names and argument orders as the reference.  What differs, on purpose:

* ``covid_3d_optimize`` returns the (T, 3) positions instead of printing them, and takes the poses (``Rs``, ``ts``, ``K``) as
  arguments; with ``Rs=None`` it reads ``Parameters.xlsx`` of ``case_idx`` the way ``spectral_method.get_fundamental`` does.
* ``solve_3d_position`` clamps every eigenvalue of A at 1e-3 by ``max``; the reference scales its last singular value by
  ``s / |s|``, which is 0 / 0 at exact degeneracy.
* the displays (``visualize_covid``, the 3-D plot, ``imshow``) are left out: there is no window system.
"""
from __future__ import annotations

import numpy as np

from . import _native

CENTER_PIC_ID = 3
PIC_LIST = (1, 2, 3, 4, 5)

__all__ = ["CENTER_PIC_ID", "PIC_LIST", "has_affinity", "match_all", "get_covid", "solve_3d_position", "covid_3d_optimize"]


def has_affinity(res_src_pts: list, pt: np.ndarray) -> int:
    """sfm_test.py:23-28: the first point of ``res_src_pts`` within 0.1 px of ``pt`` in both axes, or -1 (float32, strict)."""
    p = np.asarray(pt, np.float32).reshape(2)
    for i, kpt in enumerate(res_src_pts):
        k = np.asarray(kpt, np.float32).reshape(2)
        if abs(k[0] - p[0]) < _native.COVIS_EPS and abs(k[1] - p[1]) < _native.COVIS_EPS:
            return i
    return -1


def match_all(case_idx: int, debug_disp: bool = False, verbose: bool = False, root: str = None, device=-1):
    """sfm_test.py:30-74: equalise the five pictures, match the centre picture against each other one at the keypoints of
    ``keypoints.mat`` and keep the RANSAC inliers.  Returns ``(imgs, all_src_pts, all_dst_pts, all_matches)``.  ``debug_disp``
    is accepted for signature compatibility."""
    import scipy.io

    from . import features, utils
    from .baseline_stitch_test import find_homography

    root = utils.DEFAULT_ROOT if root is None else root
    feature_mat = scipy.io.loadmat(f"{utils.get_base_path(case_idx, root)}/keypoints.mat")["keypoints"]
    imgs = [utils.visualize_equalized_hist(case_idx=case_idx, img_idx=idx, root=root, device=device) for idx in PIC_LIST]
    center_img = imgs[CENTER_PIC_ID - 1]
    all_src_pts, all_dst_pts, all_matches = [], [], []
    for idx in PIC_LIST:
        if idx == CENTER_PIC_ID:
            continue
        feat_mat = feature_mat[idx - 1 if idx < CENTER_PIC_ID else idx - 2][0]
        raw_kpts_op, raw_kpts_cp = feat_mat[3:-1, :].T, feat_mat[:2, :].T
        kpts_cp, _, kpts_op, _, matches = features.coarse_matching(center_img, imgs[idx - 1], raw_kpts_cp, raw_kpts_op, device=device)
        src_pts = np.float32([kpts_cp[m.queryIdx].pt for m in matches]).reshape(-1, 1, 2)
        dst_pts = np.float32([kpts_op[m.trainIdx].pt for m in matches]).reshape(-1, 1, 2)
        _, mask = find_homography(src_pts, dst_pts, 5.0, device=device)
        keep = np.asarray(mask).ravel().astype(bool)
        all_src_pts.append([p for p, k in zip(src_pts, keep) if k])
        all_matches.append([m for m, k in zip(matches, keep) if k])
        all_dst_pts.append(dst_pts)
        if verbose:
            print(f"Matching image {idx} against image {CENTER_PIC_ID}...")
            print(f"Number of valid matches: {int(keep.sum())}. Number of total matches: {len(matches)}")
    return imgs, all_src_pts, all_dst_pts, all_matches


def _views(all_src_pts, all_matches):
    if len(all_src_pts) != len(all_matches):
        raise ValueError(f"get_covid: {len(all_src_pts)} point lists and {len(all_matches)} match lists")
    views = []
    for v, (pts, matches) in enumerate(zip(all_src_pts, all_matches)):
        if len(pts) != len(matches):
            raise ValueError(f"get_covid: view {v} holds {len(pts)} points and {len(matches)} matches")
        views.append((np.array([np.asarray(p, np.float32).reshape(2) for p in pts], np.float32).reshape(-1, 2),
                      np.array([m.trainIdx for m in matches], np.int64)))
    return views


def get_covid(all_src_pts: list, all_matches: list, device=-1, ctx=None):
    """sfm_test.py:79-95: ``(res_src_pts, covid)``; ``covid[i]`` lists, per view, the ``trainIdx`` of the match that saw track
    i's point (or -1), ``res_src_pts[i]`` is that point, shaped as the first view's points are (``(1, 2)`` float32 from
    ``match_all``).  ``all_matches`` holds objects with a ``trainIdx`` (``matching.DMatch``, ``cv.DMatch``).  The row length
    is the number of views (the reference's is fixed at 4); up to 8 views, 65 536 matches in all."""
    table, track_pts, _ = _native.covis_tracks(_views(all_src_pts, all_matches), device=device, ctx=ctx)
    shape = next((np.shape(p) for pts in all_src_pts for p in pts), (1, 2))
    return [p.reshape(shape).copy() for p in track_pts], [[int(x) for x in row] for row in table]


def solve_3d_position(wf_origins: np.ndarray, wf_ray_dir: np.ndarray, verbose=False, device=-1, ctx=None):
    """sfm_test.py:125-136: the point nearest to the rays ``(wf_origins[k], wf_ray_dir[k])``, (n, 3, 1) each -> (3, 1)."""
    o = np.asarray(wf_origins, np.float64).reshape(-1, 3)
    d = np.asarray(wf_ray_dir, np.float64).reshape(-1, 3)
    X, lam, _ = _native.triangulate_rays(o, d, [0, len(o)], device=device, ctx=ctx)
    if verbose and lam[0] < 1e-3:
        print(f"The last eigen value is too small: {abs(lam[0])}. Ill-conditioned matrix.")
    return X[0].reshape(3, 1)


def _read_poses(case_idx, root):
    """utils.read_rot_trans_int, as ``spectral_method.get_fundamental`` reads it (needs pandas with an xlsx reader, and scipy)."""
    import pandas as pd
    from scipy.spatial.transform import Rotation as Rot

    path = f"{root}/case{case_idx}/Parameters.xlsx"
    poses = pd.read_excel(path, sheet_name="Parameters of UAV").to_numpy()[..., 1:].astype(np.float32)
    position, euler_angles = poses[..., :3], poses[..., 3:]
    Rs = []
    for euler in euler_angles:
        euler[1] = -euler[1]
        Rs.append(Rot.from_euler("yzx", euler, degrees=True).as_matrix())
    K = pd.read_excel(path, sheet_name="Parameters of camera").to_numpy()[..., 1:].astype(np.float32)
    return np.stack(Rs, axis=0), position, K


def covid_3d_optimize(covid, res_src_pts, all_dst_pts, case_idx=1, visualize=False, Rs=None, ts=None, K=None, min_views=2,
                      root="../diff_1/raw_data", device=-1, ctx=None):
    """sfm_test.py:139-167 for every track in one call: the rays of the centre picture's point and of each view's matched
    point, intersected.  ``Rs`` (5, 3, 3), ``ts`` (5, 3) and ``K`` (3, 3) are the poses and intrinsics of pictures 1 .. 5
    (``None``: read from ``Parameters.xlsx`` of ``case_idx``); view j is picture ``j + 1`` before the centre picture and
    ``j + 2`` after it, as in the reference.  Returns (T, 3) float64; a track seen in fewer than ``min_views`` views (the
    reference skips ``<= 1``) is NaN.  ``visualize`` is accepted for signature compatibility."""
    if Rs is None or ts is None or K is None:
        Rs, ts, K = _read_poses(case_idx, root)
    n_views = len(all_dst_pts)
    table = np.array(covid, np.int64).reshape(len(covid), n_views)
    view_cam = [j if j < CENTER_PIC_ID - 1 else j + 1 for j in range(n_views)]
    track_pts = np.array([np.asarray(p, np.float32).reshape(2) for p in res_src_pts], np.float32).reshape(-1, 2)
    dst = [np.asarray(d, np.float32).reshape(-1, 2) for d in all_dst_pts]
    K_inv = np.linalg.inv(np.asarray(K, np.float64))
    X, _, _ = _native.triangulate_tracks(table, track_pts, dst, K_inv, np.asarray(Rs, np.float64), np.asarray(ts, np.float64).reshape(-1, 3),
                                         CENTER_PIC_ID - 1, view_cam, min_views=min_views, device=device, ctx=ctx)
    return X
