"""The specification of the co-visibility tracks and the ray triangulation (csrc/apap_sfm.hip; the reference's
pyviz/sfm_test.py get_covid :79-95 with has_affinity :23-28, solve_3d_position :125-136, utils.world_frame_ray_dir :188-202).

Plain loops; every floating-point operation is rounded on its own and there is nothing but + - * / sqrt, abs and
comparisons, so the kernels (built with -ffp-contract=off) equal it bit for bit.  The tracks compute in float32, the rays and
the intersection in float64 (Python floats).

A case's input is ``views``: a list of ``(pts (n, 2) float32, idx (n,) int32)``, view 0 first.
"""
import math

import numpy as np

EPS = np.float32(0.1)
MAX_VIEWS = 8
MAX_POINTS = 65536
LAM_FLOOR = 1e-3
MAX_SWEEPS = 16
NAN = float("nan")


def in_box(q, p, eps):
    """``fabsf(q.x - p.x) < eps and fabsf(q.y - p.y) < eps`` in float32; false for NaN."""
    with np.errstate(invalid="ignore"):
        return bool(abs(np.float32(q[0]) - np.float32(p[0])) < eps) and bool(abs(np.float32(q[1]) - np.float32(p[1])) < eps)


def _first_in_box(tx, ty, count, p, eps):
    """The first i < count with (tx[i], ty[i]) in p's box, or -1.  One float32 subtraction, abs and comparison per element,
    as in_box; written over arrays only so that the tests' larger inputs take milliseconds (``plain`` below is the loop)."""
    with np.errstate(invalid="ignore"):
        hit = (np.abs(tx[:count] - p[0]) < eps) & (np.abs(ty[:count] - p[1]) < eps)
    i = int(hit.argmax()) if count else 0
    return i if count and hit[i] else -1


def flatten(views):
    """views -> (pts (N, 2) float32, idx (N,) int32, offsets (V + 1,) int32)."""
    pts = np.concatenate([np.asarray(p, np.float32).reshape(-1, 2) for p, _ in views]) if views else np.zeros((0, 2), np.float32)
    idx = np.concatenate([np.asarray(i, np.int32).reshape(-1) for _, i in views]) if views else np.zeros(0, np.int32)
    off = np.zeros(len(views) + 1, np.int32)
    off[1:] = np.cumsum([len(np.asarray(i).reshape(-1)) for _, i in views])
    return np.ascontiguousarray(pts), np.ascontiguousarray(idx), off


def covis_tracks(views, eps=EPS, plain=False):
    """The reference's sequence.  Returns (table (T, V) int32, track_pts (T, 2) float32, point_track (N,) int32)."""
    eps = np.float32(eps)
    V = len(views)
    assert 1 <= V <= MAX_VIEWS
    pts, idx, off = flatten(views)
    N = len(pts)
    tx, ty = np.zeros(N, np.float32), np.zeros(N, np.float32)       # at most N tracks
    table = np.full((N, V), -1, np.int32)
    point_track = np.zeros(N, np.int32)
    T = 0
    for g in range(off[0], off[1]):                                  # view 0: every observation opens a track
        tx[T], ty[T] = pts[g]
        table[T, 0] = idx[g]
        point_track[g] = T
        T += 1
    for v in range(1, V):
        for g in range(off[v], off[v + 1]):
            p = pts[g]
            if plain:
                i = -1
                for k in range(T):
                    if in_box((tx[k], ty[k]), p, eps):
                        i = k
                        break
            else:
                i = _first_in_box(tx, ty, T, p, eps)
            if i < 0:
                i = T
                tx[T], ty[T] = p
                T += 1
            table[i, v] = idx[g]                                     # the last of a view wins
            point_track[g] = i
    return table[:T].copy(), np.stack([tx[:T], ty[:T]], axis=1), point_track


def covis_tracks_fixed_point(views, eps=EPS):
    """The parallel form the kernels take, restated: the same outputs, and the number of rounds.

    Positions g run over the concatenated observations.  ``first[g]`` is the first position e < g in g's box (all of view 0
    precedes every later observation).  owner[g] = the position that founded g's track: first[g] when that lies in view 0;
    g itself when no candidate is left; else, walking the in-box positions c < g in order, the first one that founded a
    track (owner[c] == c) - decided once every candidate before it is known to have founded none.  A round decides every
    observation whose walk meets no undecided candidate, from the owners of the round before."""
    eps = np.float32(eps)
    pts, idx, off = flatten(views)
    N, V, n0 = len(pts), len(views), int(off[1])
    with np.errstate(invalid="ignore"):
        box = (np.abs(pts[None, :, 0] - pts[:, None, 0]) < eps) & (np.abs(pts[None, :, 1] - pts[:, None, 1]) < eps)
    box &= np.arange(N)[None, :] < np.arange(N)[:, None]            # box[g, e]: e < g in g's box
    owner = np.full(N, -1, np.int64)
    owner[:n0] = np.arange(n0)
    cand = [np.flatnonzero(box[g]) for g in range(N)]
    for g in range(n0, N):
        if len(cand[g]) == 0:
            owner[g] = g
        elif cand[g][0] < n0:
            owner[g] = cand[g][0]
    rounds = 0
    while (owner < 0).any():
        rounds += 1
        assert rounds <= N
        new = owner.copy()
        for g in np.flatnonzero(owner < 0):
            dec = g
            for c in cand[g]:
                if owner[c] < 0:
                    dec = -1
                    break
                if owner[c] == c:
                    dec = c
                    break
            new[g] = dec
        owner = new
    founder = owner == np.arange(N)
    rank = np.cumsum(founder) - 1                                    # view 0 founds tracks 0 .. n0 - 1
    point_track = rank[owner].astype(np.int32)
    T = int(founder.sum())
    table = np.full((T, V), -1, np.int32)
    view = np.searchsorted(off[1:], np.arange(N), side="right")
    for g in range(N):                                               # in order: the last wins
        table[point_track[g], view[g]] = idx[g]
    return table, pts[founder], point_track, rounds


# ------------------------------------------------------------------ rays
def pixel_ray(Kinv, R, u, v):
    """world_frame_ray_dir for one pixel: Kinv (9 floats, row-major), R (9 floats), pixel (u, v) as floats."""
    cx = (Kinv[0] * u + Kinv[1] * v) + Kinv[2]
    cy = (Kinv[3] * u + Kinv[4] * v) + Kinv[5]
    cz = (Kinv[6] * u + Kinv[7] * v) + Kinv[8]
    wx, wy, wz = cx, cz, -cy
    with np.errstate(all="ignore"):
        norm = float(np.sqrt(np.float64((wx * wx + wy * wy) + wz * wz)))
        wx, wy, wz = (float(np.float64(w) / np.float64(norm)) for w in (wx, wy, wz))
    return (_dot3(R[0], R[1], R[2], wx, wy, wz), _dot3(R[3], R[4], R[5], wx, wy, wz), _dot3(R[6], R[7], R[8], wx, wy, wz))


def _dot3(a0, a1, a2, b0, b1, b2):
    return (a0 * b0 + a1 * b1) + a2 * b2


def world_frame_ray_dir(K_inv, pix, Rs):
    """The reference's shapes: K_inv (3, 3), pix (n, 2, 1), Rs (n, 3, 3) -> (n, 3, 1) float64."""
    K = [float(x) for x in np.asarray(K_inv, np.float64).ravel()]
    out = np.zeros((len(pix), 3, 1))
    for k in range(len(pix)):
        R = [float(x) for x in np.asarray(Rs[k], np.float64).ravel()]
        out[k, :, 0] = pixel_ray(K, R, float(pix[k][0][0]), float(pix[k][1][0]))
    return out


# ------------------------------------------------------------------ intersection
def _jacobi_turn(a, v, p, q, r):
    """One turn on the pair (p, q) of the symmetric 3 x 3 ``a`` (a list of lists, both triangles kept equal), r the third
    index; ``v`` collects the rotations.  Returns whether it rotated."""
    apq = a[p][q]
    if apq == 0.0:
        return False
    g = 100.0 * abs(apq)
    if abs(a[p][p]) + g == abs(a[p][p]) and abs(a[q][q]) + g == abs(a[q][q]):
        a[p][q] = a[q][p] = 0.0
        return False
    with np.errstate(all="ignore"):
        theta = float(np.float64(a[q][q] - a[p][p]) / np.float64(apq + apq))
        t = float(np.float64(1.0) / np.float64(abs(theta) + float(np.sqrt(np.float64(theta * theta + 1.0)))))
        if theta < 0.0:
            t = -t
        c = float(np.float64(1.0) / np.sqrt(np.float64(t * t + 1.0)))
    s = t * c
    h = t * apq
    a[p][p] = a[p][p] - h
    a[q][q] = a[q][q] + h
    a[p][q] = a[q][p] = 0.0
    arp, arq = a[r][p], a[r][q]
    a[r][p] = a[p][r] = c * arp - s * arq
    a[r][q] = a[q][r] = s * arp + c * arq
    for k in range(3):
        vp, vq = v[k][p], v[k][q]
        v[k][p] = c * vp - s * vq
        v[k][q] = s * vp + c * vq
    return True


def ray_sums(origins, dirs):
    """A (3 x 3 as lists) and p of the rays in order; the six distinct entries of I - d d^T are formed once per ray."""
    a = [[0.0] * 3 for _ in range(3)]
    p = [0.0, 0.0, 0.0]
    for o, d in zip(origins, dirs):
        ox, oy, oz = (float(x) for x in o)
        dx, dy, dz = (float(x) for x in d)
        m00, m11, m22 = 1.0 - dx * dx, 1.0 - dy * dy, 1.0 - dz * dz
        m01, m02, m12 = -(dx * dy), -(dx * dz), -(dy * dz)
        m = [[m00, m01, m02], [m01, m11, m12], [m02, m12, m22]]
        for i in range(3):
            for j in range(3):
                a[i][j] = a[i][j] + m[i][j]
            p[i] = p[i] + _dot3(m[i][0], m[i][1], m[i][2], ox, oy, oz)
    return a, p


def solve_rays(origins, dirs, info=None):
    """solve_3d_position for one track: (X (3,) float64, lam_min, n_rays).  No rays: NaN, NaN, 0."""
    n = len(origins)
    if n == 0:
        return np.full(3, NAN), NAN, 0
    a, p = ray_sums(origins, dirs)
    v = [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]
    sweeps = 0
    for _ in range(MAX_SWEEPS):
        rot = _jacobi_turn(a, v, 0, 1, 2)
        rot = _jacobi_turn(a, v, 0, 2, 1) or rot
        rot = _jacobi_turn(a, v, 1, 2, 0) or rot
        if not rot:
            break
        sweeps += 1
    if info is not None:
        info["sweeps"] = sweeps
    lam = [a[0][0], a[1][1], a[2][2]]
    m = lam[0]
    if lam[1] < m:
        m = lam[1]
    if lam[2] < m:
        m = lam[2]
    lam_min = NAN if m != m else m
    lam = [LAM_FLOOR if x < LAM_FLOOR else x for x in lam]
    with np.errstate(all="ignore"):
        z = [float(np.float64(_dot3(v[0][k], v[1][k], v[2][k], p[0], p[1], p[2])) / np.float64(lam[k])) for k in range(3)]
    x = [_dot3(v[i][0], v[i][1], v[i][2], z[0], z[1], z[2]) for i in range(3)]
    if not all(abs(c) < math.inf for c in x):
        x = [NAN, NAN, NAN]
    return np.array(x, np.float64), lam_min, n


def triangulate_rays(origins, dirs, ray_offset):
    """The batched form: origins, dirs (R, 3) float64, ray_offset (T + 1,).  Returns X (T, 3), lam_min (T,), n_rays (T,) int32."""
    T = len(ray_offset) - 1
    X, lam, n = np.zeros((T, 3)), np.zeros(T), np.zeros(T, np.int32)
    for k in range(T):
        a, b = int(ray_offset[k]), int(ray_offset[k + 1])
        X[k], lam[k], n[k] = solve_rays(origins[a:b], dirs[a:b])
    return X, lam, n


def track_rays(table, track_pts, dst_pts, dst_offset, Kinv, R, origins, center_cam, view_cam, min_views=2):
    """The rays of every track as a CSR (origins (R, 3), dirs (R, 3), ray_offset): the centre picture's first, then the views
    ascending whose column holds an index inside the view's points; fewer than ``min_views`` such views: none."""
    K = [float(x) for x in np.asarray(Kinv, np.float64).ravel()]
    Rl = [[float(x) for x in np.asarray(r, np.float64).ravel()] for r in R]
    o_out, d_out, off = [], [], [0]
    for k in range(len(table)):
        seen = [v for v in range(table.shape[1]) if 0 <= table[k, v] < dst_offset[v + 1] - dst_offset[v]]
        if len(seen) >= min_views:
            u, w = track_pts[k]
            o_out.append(origins[center_cam])
            d_out.append(pixel_ray(K, Rl[center_cam], float(u), float(w)))
            for v in seen:
                u, w = dst_pts[dst_offset[v] + table[k, v]]
                o_out.append(origins[view_cam[v]])
                d_out.append(pixel_ray(K, Rl[view_cam[v]], float(u), float(w)))
        off.append(len(o_out))
    return (np.array(o_out, np.float64).reshape(-1, 3), np.array(d_out, np.float64).reshape(-1, 3), np.array(off, np.int32))


def triangulate_tracks(table, track_pts, dst_pts, dst_offset, Kinv, R, origins, center_cam, view_cam, min_views=2):
    return triangulate_rays(*track_rays(table, track_pts, dst_pts, dst_offset, Kinv, R, origins, center_cam, view_cam, min_views))
