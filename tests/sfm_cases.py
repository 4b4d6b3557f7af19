"""Inputs of the co-visibility and triangulation tests: seeded by integer hashing and built with + - * / only, so they are the
same on every numpy.  tests/golden/sfm_ref.npz holds what the reference's own get_covid, world_frame_ray_dir and
solve_3d_position return for them (tests/golden/make_sfm_golden.py)."""
import numpy as np

from denoise_cases import _words

F32 = np.float32
EPS_BELOW = np.nextafter(F32(0.1), F32(0.0))       # nextafterf(0.1f, 0)


def uniform(count, seed, stream):
    """``count`` float64 in [0, 1) on a 2^-32 grid."""
    return (_words(count, seed, stream) >> np.uint64(32)).astype(np.float64) / 2.0 ** 32


def integers(count, seed, stream, high):
    return (_words(count, seed, stream) % np.uint64(high)).astype(np.int64)


def jittered_views(n_views, n, base_n, jitter, seed, chain=0, spread=700.0):
    """``n_views`` views of ``n`` observations: points of a base set of ``base_n``, each moved by up to ``jitter`` px.  With
    ``chain``, the first ``chain`` observations of view 2 lie 0.09 px apart on a line: each is inside the box of the one
    before it and of no other."""
    base = (uniform(2 * base_n, seed, 0) * spread).astype(F32).reshape(base_n, 2)
    views = []
    for v in range(n_views):
        pick = integers(n, seed, 10 + v, base_n)
        pts = (base[pick] + (uniform(2 * n, seed, 30 + v) * jitter).astype(F32).reshape(n, 2)).astype(F32)
        if chain and v == 2:
            pts[:chain, 0] = (10.0 + 0.09 * np.arange(chain)).astype(F32)
            pts[:chain, 1] = F32(5.0)
        views.append((pts, integers(n, seed, 50 + v, 1000).astype(np.int32)))
    return views


def _view(points, first_idx):
    pts = np.array(points, F32).reshape(-1, 2)
    return pts, np.arange(first_idx, first_idx + len(pts), dtype=np.int32)


def track_cases():
    """name -> views.  The first three are the issue's prototype cases; the rest each reach one edge of the definition."""
    z = np.zeros((0, 2), F32)
    return {
        "jitter_4x40": jittered_views(4, 40, 30, 0.15, seed=1),
        "chain_4x120": jittered_views(4, 120, 60, 0.12, seed=2, chain=60),
        "repeats_4x200": jittered_views(4, 200, 150, 0.0, seed=3),
        "exactly_eps_apart": [_view([(0.0, 2.0)], 10), _view([(F32(0.1), 2.0)], 20)],                 # no match
        "just_below_eps": [_view([(0.0, 2.0)], 10), _view([(EPS_BELOW, 2.0)], 20)],                   # a match
        "inside_in_x_only": [_view([(0.0, 0.0)], 10), _view([(0.05, 3.0)], 20)],
        "identical_in_view0": [_view([(7.0, 7.0), (7.0, 7.0)], 10), _view([(7.0, 7.0)], 20), _view([(7.05, 7.0)], 30)],
        "last_of_a_view_wins": [_view([(3.0, 3.0)], 10), _view([(3.0, 3.0), (9.0, 9.0), (3.01, 3.0)], 20)],
        "empty_view_in_the_middle": [_view([(1.0, 1.0), (5.0, 5.0)], 10), (z, np.zeros(0, np.int32)), _view([(1.0, 1.05), (8.0, 8.0)], 30),
                                     _view([(8.0, 8.05), (5.0, 5.0)], 40)],
        "empty_view0": [(z, np.zeros(0, np.int32)), _view([(1.0, 1.0), (1.05, 1.0), (4.0, 4.0)], 20), _view([(4.0, 4.05), (1.0, 1.0)], 30)],
        "single_view": [_view([(1.0, 1.0), (1.0, 1.0), (2.0, 2.0)], 10)],
        "nan_point": [_view([(1.0, 1.0)], 10), _view([(np.nan, 1.0), (1.0, 1.0), (np.nan, 1.0)], 20)],
    }


REFERENCE_TRACK_CASES = [k for k in track_cases() if k != "nan_point"]     # the reference's row length is 4 and its kpt - pt
                                                                            # warns on NaN: that one is the specification's alone


def random_views(n_total, n_views, seed, base_frac=0.6, jitter=0.13):
    """``n_total`` observations over ``n_views`` views of unequal sizes (the last takes the rest), for the scan's edges."""
    cuts = np.sort(integers(n_views - 1, seed, 90, n_total + 1)) if n_views > 1 else np.zeros(0, np.int64)
    sizes = np.diff(np.concatenate([[0], cuts, [n_total]]))
    base_n = max(1, int(n_total * base_frac))
    base = (uniform(2 * base_n, seed, 0) * 300.0).astype(F32).reshape(base_n, 2)
    views = []
    for v, n in enumerate(int(s) for s in sizes):
        pick = integers(n, seed, 100 + v, base_n)
        pts = (base[pick] + (uniform(2 * n, seed, 130 + v) * jitter).astype(F32).reshape(n, 2)).astype(F32)
        views.append((pts, integers(n, seed, 160 + v, 5000).astype(np.int32)))
    return views


def chain_views(length):
    """Two views; view 1 is a chain of ``length`` points 0.09 px apart: the fixed point needs about ``length`` rounds."""
    pts = np.stack([(10.0 + 0.09 * np.arange(length)).astype(F32), np.full(length, 5.0, F32)], axis=1)
    return [_view([(500.0, 500.0)], 7), (pts, np.arange(length, dtype=np.int32))]


def interlocked_views(far=1500, length=1100, spaced=False):
    """Three views.  View 0: ``far`` points far from the rest (so the later views do not start at a round position).  Views 1
    and 2: chains of ``length`` points 0.09 px apart on one row, the second chain half a step beside the first - point k of
    view 2 has points k and k + 1 of view 1 and its own predecessor in its box, in that order, and only every second point of
    view 1 founds a track: for odd k the walk passes a decided observation that founded nothing and goes on behind it.
    With ``spaced`` a far-away point (each founds a track of its own) follows every point of view 1's chain, so that the next
    in-box observation is not the next position."""
    k = np.arange(length)
    row = np.full(length, 5.0, F32)
    chain1 = np.stack([(10.0 + 0.09 * k).astype(F32), row], axis=1)
    chain2 = np.stack([(10.045 + 0.09 * k).astype(F32), row], axis=1)
    away = np.stack([(1000.0 + 3.0 * np.arange(far)).astype(F32), np.full(far, 900.0, F32)], axis=1)
    if spaced:
        between = np.stack([(1000.0 + 3.0 * k).astype(F32), np.full(length, 1800.0, F32)], axis=1)
        chain1 = np.stack([chain1, between], axis=1).reshape(-1, 2)
    return [(away, np.arange(far, dtype=np.int32)), (chain1, 10000 + np.arange(len(chain1), dtype=np.int32)),
            (chain2, 20000 + np.arange(length, dtype=np.int32))]


# The resolver (csrc/apap_sfm.hip, k_covis_resolve) is one workgroup of this many threads; thread t owns the observations
# n0 + t, n0 + t + RESOLVE_THREADS, ...  The cases below give a thread several links of one chain.
RESOLVE_THREADS = 1024
LONG_CHAIN = 2200                    # chain_views(LONG_CHAIN): three links of one chain per thread
LARGE_RANDOM = dict(n_total=12000, n_views=8, seed=9)


# ------------------------------------------------------------------ triangulation
def rotation(q):
    """The rotation of a quaternion (w, x, y, z), not normalised: + - * / only."""
    w, x, y, z = (float(c) for c in q)
    n = w * w + x * x + y * y + z * z
    s = 2.0 / n
    return np.array([[1.0 - s * (y * y + z * z), s * (x * y - z * w), s * (x * z + y * w)],
                     [s * (x * y + z * w), 1.0 - s * (x * x + z * z), s * (y * z - x * w)],
                     [s * (x * z - y * w), s * (y * z + x * w), 1.0 - s * (x * x + y * y)]])


def ray_case(count, seed):
    """``count`` tracks of 2 .. 5 rays from cameras 60 .. 80 above the ground plane z = 0 towards a point on it, the
    directions disturbed by 0.02; in every fourth track the cameras nearly coincide (1e-3, in every eighth 1e-7), so the
    rays are nearly parallel and the clamp fires.  Returns (origins (R, 3), dirs (R, 3), ray_offset (count + 1,) int32)."""
    n = 2 + integers(count, seed, 0, 4)
    off = np.zeros(count + 1, np.int32)
    off[1:] = np.cumsum(n)
    R = int(off[-1])
    u = uniform(3 * R, seed, 1).reshape(R, 3)
    origins = np.stack([u[:, 0] * 50.0, u[:, 1] * 50.0, 60.0 + u[:, 2] * 20.0], axis=1)
    spread = (uniform(3 * R, seed, 2).reshape(R, 3) - 0.5)
    noise = (uniform(3 * R, seed, 3).reshape(R, 3) - 0.5) * 0.04
    target = uniform(2 * count, seed, 4).reshape(count, 2) * 50.0
    dirs = np.zeros((R, 3))
    for k in range(count):
        a, b = off[k], off[k + 1]
        if k % 4 == 0:
            origins[a:b] = origins[a] + spread[a:b] * (2e-3 if k % 8 else 2e-7)
        d = np.array([target[k, 0], target[k, 1], 0.0]) - origins[a:b] + noise[a:b]
        dirs[a:b] = d / np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])[:, None]
    return origins, dirs, off


RAY_CASE = dict(count=240, seed=13)      # (seeds 11 and 12 put one track's smallest singular value between 5e-4 and 2e-3)


def camera_case(n_views, n_tracks, seed, nearly_coincident=False):
    """A centre camera and ``n_views`` others above a ground plane, and tracks seen in a random two thirds of the views at
    random pixels (the rays need not meet: it is the arithmetic that is compared).  Returns dict(Kinv, R (C, 3, 3), origins (C, 3), center_cam, view_cam, table, track_pts, dst_pts, dst_offset)."""
    C = n_views + 1
    K = np.array([[800.0, 0.0, 384.0], [0.0, 800.0, 384.0], [0.0, 0.0, 1.0]])
    Kinv = np.array([[1.0 / 800.0, 0.0, -384.0 / 800.0], [0.0, 1.0 / 800.0, -384.0 / 800.0], [0.0, 0.0, 1.0]])
    u = uniform(7 * C, seed, 0).reshape(C, 7)
    # small rotations about the identity: any proper rotation serves the arithmetic
    R = np.stack([rotation((1.0, 0.2 * (u[c, 0] - 0.5), 0.2 * (u[c, 1] - 0.5), 0.2 * (u[c, 2] - 0.5))) for c in range(C)])
    origins = np.stack([u[:, 3] * 50.0, u[:, 4] * 50.0, 60.0 + u[:, 5] * 20.0], axis=1)
    n_dst = 37
    dst_offset = np.arange(n_views + 1, dtype=np.int32) * n_dst
    dst_pts = (uniform(2 * n_dst * n_views, seed, 1) * 768.0).astype(F32).reshape(-1, 2)
    track_pts = (uniform(2 * n_tracks, seed, 2) * 768.0).astype(F32).reshape(-1, 2)
    if nearly_coincident:       # one orientation, origins 1e-4 apart, pixels 0.01 px apart: every track's rays are nearly parallel
        origins = origins[0] + (u[:, 3:6] - 0.5) * 2e-4
        R = np.stack([R[0]] * C)
        dst_pts = (F32(400.0) + dst_pts * F32(0.01 / 768.0)).astype(F32)
        track_pts = (F32(400.0) + track_pts * F32(0.01 / 768.0)).astype(F32)
    table = integers(n_tracks * n_views, seed, 3, n_dst).astype(np.int32).reshape(n_tracks, n_views)
    keep = integers(n_tracks * n_views, seed, 4, 3).reshape(n_tracks, n_views) > 0      # a third of the columns empty
    table[~keep] = -1
    return dict(K=K, Kinv=Kinv, R=R, origins=origins, center_cam=n_views // 2, view_cam=[c if c < n_views // 2 else c + 1 for c in range(n_views)],
                table=table, track_pts=track_pts, dst_pts=dst_pts, dst_offset=dst_offset)
