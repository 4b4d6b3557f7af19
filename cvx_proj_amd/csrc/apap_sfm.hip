// Co-visibility tracks and ray triangulation (pyviz/sfm_test.py: get_covid :79-95 with has_affinity :23-28,
// solve_3d_position :125-136; utils.world_frame_ray_dir :188-202).  tests/sfm_spec.py is the specification, bit for bit.
//
// Tracks.  The observations of all views lie in one array, view after view; g is a position in it, n0 the size of view 0.
// The reference's first-fit in sequence is reproduced by a fixed point (DESIGN.md "Co-visibility tracks and triangulation"):
//   S1 k_covis_scan     for every observation g >= n0 the FIRST position e < g inside its box (every view-0 point precedes
//                       every later observation, so one number tells both "first view-0 point" and "first earlier
//                       observation"): grid of 256 queries x 512 entries, entries staged in LDS, combined by atomicMin
//   S2 k_covis_resolve  one workgroup: owner[g] = the position that founded g's track, decided as soon as every earlier
//                       in-box observation up to the first founder is decided; then the founders' prefix sum
//   S3 k_covis_rows     point_track, track_pts, the founders' table rows set to -1
//   S4 k_covis_last     table[track][view] = max position (an integer atomicMax: "the last wins", whatever the arrival order)
//   S5 k_covis_index    positions replaced by the observations' indices
// Kernel boundaries carry every ordering; no workgroup waits for another inside a launch.
//
// Triangulation.  One lane per track, everything in registers: the rays are summed into A = sum (I - d d^T) and
// p = sum (I - d d^T) o as they are built, A's eigen-decomposition is a cyclic Jacobi iteration in the pair order (0, 1),
// (0, 2), (1, 2) and X = V diag(1 / max(lam, 1e-3)) V^T p.
#include <hip/hip_runtime.h>

#include <cmath>

#include "apap_internal.h"

namespace {

constexpr int kQueries = 256;        // observations a block of the scan asks for
constexpr int kTile = 256;           // entries staged at a time, 8 bytes each
constexpr int kChunk = 512;          // entries one block scans: two tiles (2048 took 59 us of a 98 us call at 4 x 500: few, long blocks)
constexpr int kResolveThreads = 1024;
constexpr int kThreads = 256;
constexpr int kMaxViews = APAP_COVIS_MAX_VIEWS;
constexpr int kMaxSweeps = 16;       // Jacobi sweeps of a 3 x 3 matrix: 5 at most seen, the cap only bounds NaN input
constexpr double kLamFloor = 1e-3;

struct CovisLayout {
    size_t offsets, first, owner, rank, total;
};
CovisLayout covis_layout(int n_points, int n_views) {
    CovisLayout L;
    size_t at = 0;
    const size_t ints = apap::up256((size_t)(n_points > 0 ? n_points : 1) * sizeof(int));
    L.offsets = at; at += apap::up256((size_t)(n_views + 1) * sizeof(int));
    L.first = at; at += ints;
    L.owner = at; at += ints;
    L.rank = at; at += ints;
    L.total = at;
    return L;
}

__device__ __forceinline__ bool in_box(float2 q, float2 p, float eps) {
    return fabsf(q.x - p.x) < eps && fabsf(q.y - p.y) < eps;      // false for NaN
}

// ---------------------------------------------------------------- S1
// first[g] (preset to -1, the largest unsigned) = min over the blocks of a query row of the first in-box entry e < g.
__global__ __launch_bounds__(kQueries) void k_covis_scan(const float2 *__restrict__ pts, int N, int n0, float eps,
                                                         int *__restrict__ first) {
    __shared__ float2 tile[kTile];
    const int t = threadIdx.x;
    const int g = n0 + blockIdx.x * kQueries + t;                    // this lane's observation
    const int g_last = min(N, n0 + (blockIdx.x + 1) * kQueries) - 1;  // the block's last one: entries lie before it
    const int e0 = blockIdx.y * kChunk, e1 = min(e0 + kChunk, g_last);
    if (e0 >= e1) return;                                            // uniform over the block
    const bool live = g < N;
    const float2 p = live ? pts[g] : make_float2(0.0f, 0.0f);
    int hit = -1;
    for (int base = e0; base < e1; base += kTile) {
        const int cnt = min(kTile, e1 - base);
        if (t < cnt) tile[t] = pts[base + t];
        __syncthreads();
#pragma unroll 8
        for (int k = 0; k < cnt; ++k) {
            const bool in = in_box(tile[k], p, eps) && base + k < g;
            if (hit < 0 && in) hit = base + k;
        }
        if (__syncthreads_and(hit >= 0 || !live)) break;             // also keeps the tile until every lane has read it
    }
    if (live && hit >= 0) atomicMin((unsigned *)&first[g], (unsigned)hit);
}

// ---------------------------------------------------------------- S2
__device__ __forceinline__ int peek(const int *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ void post(int *p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }

// owner[g], g >= n0: -1 undecided, else the position that founded g's track (g itself: g opens one).  cand[g] enters as
// S1's first[g] and moves forward past decided observations that opened nothing.  An owner is written once and is final, so
// reading one that another wave decides in the same round only saves a round.  The earliest undecided observation is
// decided in every round: at most N - n0 rounds; the count is kept as the loop's bound all the same.
__global__ __launch_bounds__(kResolveThreads) void k_covis_resolve(const float2 *__restrict__ pts, int N, int n0, float eps, int *cand,
                                                                   int *owner, int *__restrict__ rank, int *__restrict__ n_tracks,
                                                                   int *status) {
    __shared__ int s_count[kResolveThreads];
    const int t = threadIdx.x;
    for (int g = n0 + t; g < N; g += kResolveThreads) {
        const int c = cand[g];
        post(&owner[g], c < 0 ? g : (c < n0 ? c : -1));
    }
    __syncthreads();
    bool overrun = false;
    for (int round = 0;; ++round) {
        int pending = 0;
        for (int g = n0 + t; g < N; g += kResolveThreads) {
            if (peek(&owner[g]) != -1) continue;
            const float2 p = pts[g];
            int c = cand[g];
            for (;;) {                              // c only grows and stays below g
                if (c < 0) {
                    post(&owner[g], g);
                    break;
                }
                const int oc = peek(&owner[c]);
                if (oc == -1) {
                    pending = 1;
                    break;
                }
                if (oc == c) {
                    post(&owner[g], c);
                    break;
                }
                int next = -1;                      // c joined another track: the scan goes on behind it
                for (int e = c + 1; e < g; ++e)
                    if (in_box(pts[e], p, eps)) {
                        next = e;
                        break;
                    }
                c = next;
            }
            cand[g] = c;
        }
        if (!__syncthreads_or(pending)) break;
        if (round >= N) {                           // uniform; unreachable by the argument above
            overrun = true;
            break;
        }
    }
    if (overrun) {
        for (int g = n0 + t; g < N; g += kResolveThreads)
            if (peek(&owner[g]) == -1) post(&owner[g], g);
        if (t == 0) atomicOr(status, APAP_STATUS_COVIS_BOUND);
        __syncthreads();
    }
    // the founders' prefix sum: a contiguous run of observations per thread
    const int M = N - n0, per = (M + kResolveThreads - 1) / kResolveThreads;
    const int a = min(N, n0 + t * per), b = min(N, a + per);
    int mine = 0;
    for (int g = a; g < b; ++g) mine += peek(&owner[g]) == g;
    s_count[t] = mine;
    __syncthreads();
    for (int step = 1; step < kResolveThreads; step <<= 1) {
        const int add = t >= step ? s_count[t - step] : 0;
        __syncthreads();
        s_count[t] += add;
        __syncthreads();
    }
    int at = n0 + s_count[t] - mine;
    for (int g = a; g < b; ++g)
        if (peek(&owner[g]) == g) rank[g] = at++;
    if (t == kResolveThreads - 1) *n_tracks = n0 + s_count[t];
}

// ---------------------------------------------------------------- S3 - S5
__global__ __launch_bounds__(kThreads) void k_covis_rows(const float2 *__restrict__ pts, int N, int n0, int V, const int *__restrict__ owner,
                                                         const int *__restrict__ rank, int *__restrict__ table,
                                                         float2 *__restrict__ track_pts, int *__restrict__ point_track) {
    const int g = blockIdx.x * kThreads + threadIdx.x;
    if (g >= N) return;
    const int o = g < n0 ? g : owner[g];
    const int track = o < n0 ? o : rank[o];
    point_track[g] = track;
    if (o == g) {
        track_pts[track] = pts[g];
        for (int v = 0; v < V; ++v) table[(size_t)track * V + v] = -1;
    }
}

__global__ __launch_bounds__(kThreads) void k_covis_last(int N, int V, const int *__restrict__ offsets, const int *__restrict__ point_track,
                                                         int *__restrict__ table) {
    const int g = blockIdx.x * kThreads + threadIdx.x;
    if (g >= N) return;
    int view = 0;
    for (int v = 1; v < V; ++v)
        if (g >= offsets[v]) view = v;
    atomicMax(&table[(size_t)point_track[g] * V + view], g);
}

__global__ __launch_bounds__(kThreads) void k_covis_index(int V, const int *__restrict__ idx, const int *__restrict__ n_tracks,
                                                          int *__restrict__ table) {
    const size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= (size_t)*n_tracks * V) return;
    const int pos = table[i];
    if (pos >= 0) table[i] = idx[pos];
}

// ---------------------------------------------------------------- triangulation
struct RaySum {
    double a00 = 0.0, a01 = 0.0, a02 = 0.0, a11 = 0.0, a12 = 0.0, a22 = 0.0, p0 = 0.0, p1 = 0.0, p2 = 0.0;
};

__device__ __forceinline__ double dot3(double a0, double a1, double a2, double b0, double b1, double b2) {
    return (a0 * b0 + a1 * b1) + a2 * b2;
}

// A += I - d d^T, p += (I - d d^T) o; the six distinct entries are formed once
__device__ __forceinline__ void add_ray(RaySum &S, double ox, double oy, double oz, double dx, double dy, double dz) {
    const double m00 = 1.0 - dx * dx, m11 = 1.0 - dy * dy, m22 = 1.0 - dz * dz;
    const double m01 = -(dx * dy), m02 = -(dx * dz), m12 = -(dy * dz);
    S.a00 = S.a00 + m00; S.a01 = S.a01 + m01; S.a02 = S.a02 + m02;
    S.a11 = S.a11 + m11; S.a12 = S.a12 + m12; S.a22 = S.a22 + m22;
    S.p0 = S.p0 + dot3(m00, m01, m02, ox, oy, oz);
    S.p1 = S.p1 + dot3(m01, m11, m12, ox, oy, oz);
    S.p2 = S.p2 + dot3(m02, m12, m22, ox, oy, oz);
}

// world_frame_ray_dir for one pixel: K^-1 (u, v, 1), the axes turned (x, z, -y), normalised, rotated into the world frame
__device__ __forceinline__ void pixel_ray(const double *__restrict__ Kinv, const double *__restrict__ R, double u, double v, double &dx,
                                          double &dy, double &dz) {
    const double cx = (Kinv[0] * u + Kinv[1] * v) + Kinv[2];
    const double cy = (Kinv[3] * u + Kinv[4] * v) + Kinv[5];
    const double cz = (Kinv[6] * u + Kinv[7] * v) + Kinv[8];
    double wx = cx, wy = cz, wz = -cy;
    const double norm = sqrt((wx * wx + wy * wy) + wz * wz);
    wx = wx / norm; wy = wy / norm; wz = wz / norm;
    dx = dot3(R[0], R[1], R[2], wx, wy, wz);
    dy = dot3(R[3], R[4], R[5], wx, wy, wz);
    dz = dot3(R[6], R[7], R[8], wx, wy, wz);
}

// One Jacobi turn on the pair (p, q) of a symmetric 3 x 3 matrix, r the third index: a_pq == 0 does nothing; an a_pq that
// is negligible beside both diagonal terms is set to zero; otherwise the rotation that annihilates it (the angle formula
// of apap_fundamental.hip).  Returns whether it rotated.
__device__ __forceinline__ bool jacobi_turn(double &app, double &aqq, double &apq, double &arp, double &arq, double &v0p, double &v0q,
                                            double &v1p, double &v1q, double &v2p, double &v2q) {
    if (apq == 0.0) return false;
    const double g = 100.0 * fabs(apq);
    if (fabs(app) + g == fabs(app) && fabs(aqq) + g == fabs(aqq)) {
        apq = 0.0;
        return false;
    }
    const double theta = (aqq - app) / (apq + apq);
    double t = 1.0 / (fabs(theta) + sqrt(theta * theta + 1.0));
    if (theta < 0.0) t = -t;
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
    const double h = t * apq;
    app = app - h;
    aqq = aqq + h;
    apq = 0.0;
    const double np = c * arp - s * arq, nq = s * arp + c * arq;
    arp = np; arq = nq;
    const double n0p = c * v0p - s * v0q, n0q = s * v0p + c * v0q;
    const double n1p = c * v1p - s * v1q, n1q = s * v1p + c * v1q;
    const double n2p = c * v2p - s * v2q, n2q = s * v2p + c * v2q;
    v0p = n0p; v0q = n0q; v1p = n1p; v1q = n1q; v2p = n2p; v2q = n2q;
    return true;
}

// X, the smallest eigenvalue before the clamp; a non-finite X is three canonical NaN, a NaN eigenvalue the canonical NaN
__device__ __forceinline__ void solve_point(RaySum S, double &x0, double &x1, double &x2, double &lam_min) {
    double v00 = 1.0, v01 = 0.0, v02 = 0.0, v10 = 0.0, v11 = 1.0, v12 = 0.0, v20 = 0.0, v21 = 0.0, v22 = 1.0;
#pragma unroll 1
    for (int sweep = 0; sweep < kMaxSweeps; ++sweep) {
        bool rot = jacobi_turn(S.a00, S.a11, S.a01, S.a02, S.a12, v00, v01, v10, v11, v20, v21);
        rot |= jacobi_turn(S.a00, S.a22, S.a02, S.a01, S.a12, v00, v02, v10, v12, v20, v22);
        rot |= jacobi_turn(S.a11, S.a22, S.a12, S.a01, S.a02, v01, v02, v11, v12, v21, v22);
        if (!rot) break;
    }
    double m = S.a00;
    if (S.a11 < m) m = S.a11;
    if (S.a22 < m) m = S.a22;
    const double nan = __builtin_nan("");
    lam_min = m != m ? nan : m;
    const double l0 = S.a00 < kLamFloor ? kLamFloor : S.a00, l1 = S.a11 < kLamFloor ? kLamFloor : S.a11,
                 l2 = S.a22 < kLamFloor ? kLamFloor : S.a22;
    const double z0 = dot3(v00, v10, v20, S.p0, S.p1, S.p2) / l0;
    const double z1 = dot3(v01, v11, v21, S.p0, S.p1, S.p2) / l1;
    const double z2 = dot3(v02, v12, v22, S.p0, S.p1, S.p2) / l2;
    x0 = dot3(v00, v01, v02, z0, z1, z2);
    x1 = dot3(v10, v11, v12, z0, z1, z2);
    x2 = dot3(v20, v21, v22, z0, z1, z2);
    const double big = __builtin_inf();
    const bool finite = fabs(x0) < big && fabs(x1) < big && fabs(x2) < big;      // false for NaN
    if (!finite) x0 = x1 = x2 = nan;
}

__device__ __forceinline__ void store_point(int track, int rays, const RaySum &S, double *__restrict__ X, double *__restrict__ lam,
                                            int *__restrict__ n_rays) {
    const double nan = __builtin_nan("");
    double x0 = nan, x1 = nan, x2 = nan, lm = nan;
    if (rays > 0) solve_point(S, x0, x1, x2, lm);
    X[(size_t)3 * track] = x0;
    X[(size_t)3 * track + 1] = x1;
    X[(size_t)3 * track + 2] = x2;
    lam[track] = lm;
    n_rays[track] = rays;
}

// The rays as given: track k holds rays ray_offset[k] .. ray_offset[k + 1] - 1 of origins / dirs (3 doubles each).  A range
// that is empty, reversed or outside [0, n_rays_total] is a track without rays.
__global__ __launch_bounds__(kThreads) void k_triangulate_rays(const double *__restrict__ origins, const double *__restrict__ dirs,
                                                               const int *__restrict__ ray_offset, int n_rays_total, int n_tracks,
                                                               double *__restrict__ X, double *__restrict__ lam,
                                                               int *__restrict__ n_rays) {
    const int track = blockIdx.x * kThreads + threadIdx.x;
    if (track >= n_tracks) return;
    const int r0 = ray_offset[track], r1 = ray_offset[track + 1];
    const bool ok = r0 >= 0 && r1 > r0 && r1 <= n_rays_total;
    RaySum S;
    if (ok)
        for (int r = r0; r < r1; ++r) {
            const double *o = origins + (size_t)3 * r, *d = dirs + (size_t)3 * r;
            add_ray(S, o[0], o[1], o[2], d[0], d[1], d[2]);
        }
    store_point(track, ok ? r1 - r0 : 0, S, X, lam, n_rays);
}

// What the tracks' kernel needs besides its arrays: the views' tables travel in the kernel argument.
struct TrackViews {
    int n_views, center_cam, min_views;
    int dst_offset[kMaxViews + 1];
    int view_cam[kMaxViews];
};

// The rays built from the tracks: the centre picture's (track_pts, camera center_cam) first, then every view whose column
// holds an index inside that view's points, ascending.  Fewer than min_views of those: no rays.
__global__ __launch_bounds__(kThreads) void k_triangulate_tracks(const int *__restrict__ table, const float2 *__restrict__ track_pts,
                                                                 const int *__restrict__ n_tracks_or_null, int max_tracks,
                                                                 const float2 *__restrict__ dst_pts, const double *__restrict__ Kinv,
                                                                 const double *__restrict__ R, const double *__restrict__ origins,
                                                                 TrackViews T, double *__restrict__ X, double *__restrict__ lam,
                                                                 int *__restrict__ n_rays) {
    const int track = blockIdx.x * kThreads + threadIdx.x;
    int n_tracks = max_tracks;
    if (n_tracks_or_null) n_tracks = min(max(*n_tracks_or_null, 0), max_tracks);
    if (track >= n_tracks) return;
    int seen = 0;
    for (int v = 0; v < T.n_views; ++v) {
        const int k = table[(size_t)track * T.n_views + v];
        seen += k >= 0 && k < T.dst_offset[v + 1] - T.dst_offset[v];
    }
    RaySum S;
    int rays = 0;
    if (seen >= T.min_views) {
        double dx, dy, dz;
        const float2 c = track_pts[track];
        pixel_ray(Kinv, R + 9 * T.center_cam, (double)c.x, (double)c.y, dx, dy, dz);
        const double *o = origins + 3 * T.center_cam;
        add_ray(S, o[0], o[1], o[2], dx, dy, dz);
        rays = 1;
        for (int v = 0; v < T.n_views; ++v) {
            const int k = table[(size_t)track * T.n_views + v];
            if (k < 0 || k >= T.dst_offset[v + 1] - T.dst_offset[v]) continue;
            const float2 q = dst_pts[T.dst_offset[v] + k];
            const int cam = T.view_cam[v];
            pixel_ray(Kinv, R + 9 * cam, (double)q.x, (double)q.y, dx, dy, dz);
            o = origins + 3 * cam;
            add_ray(S, o[0], o[1], o[2], dx, dy, dz);
            ++rays;
        }
    }
    store_point(track, rays, S, X, lam, n_rays);
}

}  // namespace

namespace apap {

int covis_check(const int *view_offset, int n_views, float eps, const char *who) {
    if (n_views < 1 || n_views > kMaxViews) return fail(APAP_ERR_INVALID_ARG, "%s: n_views = %d (1 .. %d)", who, n_views, kMaxViews);
    if (!view_offset) return fail(APAP_ERR_INVALID_ARG, "%s: null view_offset", who);
    if (view_offset[0] != 0) return fail(APAP_ERR_INVALID_ARG, "%s: view_offset[0] = %d (the views start at 0)", who, view_offset[0]);
    for (int v = 0; v < n_views; ++v)
        if (view_offset[v + 1] < view_offset[v])
            return fail(APAP_ERR_INVALID_ARG, "%s: view_offset is not ascending at view %d (%d after %d)", who, v, view_offset[v + 1],
                        view_offset[v]);
    if (view_offset[n_views] > APAP_COVIS_MAX_POINTS)
        return fail(APAP_ERR_INVALID_ARG, "%s: %d observations in all (at most %d: the first-candidate scan is quadratic)", who,
                    view_offset[n_views], APAP_COVIS_MAX_POINTS);
    if (!(eps >= 0.0f) || !(eps <= 3.0e38f)) return fail(APAP_ERR_INVALID_ARG, "%s: eps = %g (finite, >= 0)", who, (double)eps);
    return APAP_OK;
}

int triangulate_tracks_check(int max_tracks, int n_views, const int *dst_offset, int n_cams, int center_cam, const int *view_cam,
                             int min_views, const char *who) {
    if (max_tracks < 0) return fail(APAP_ERR_INVALID_ARG, "%s: %d tracks (>= 0)", who, max_tracks);
    if (n_views < 1 || n_views > kMaxViews) return fail(APAP_ERR_INVALID_ARG, "%s: n_views = %d (1 .. %d)", who, n_views, kMaxViews);
    if (!dst_offset || !view_cam) return fail(APAP_ERR_INVALID_ARG, "%s: null dst_offset or view_cam", who);
    if (dst_offset[0] != 0) return fail(APAP_ERR_INVALID_ARG, "%s: dst_offset[0] = %d (the views' points start at 0)", who, dst_offset[0]);
    for (int v = 0; v < n_views; ++v)
        if (dst_offset[v + 1] < dst_offset[v]) return fail(APAP_ERR_INVALID_ARG, "%s: dst_offset is not ascending at view %d", who, v);
    if (n_cams < 1) return fail(APAP_ERR_INVALID_ARG, "%s: n_cams = %d (>= 1)", who, n_cams);
    if (center_cam < 0 || center_cam >= n_cams) return fail(APAP_ERR_INVALID_ARG, "%s: center_cam = %d (0 .. %d)", who, center_cam, n_cams - 1);
    for (int v = 0; v < n_views; ++v)
        if (view_cam[v] < 0 || view_cam[v] >= n_cams)
            return fail(APAP_ERR_INVALID_ARG, "%s: view_cam[%d] = %d (0 .. %d)", who, v, view_cam[v], n_cams - 1);
    if (min_views < 1) return fail(APAP_ERR_INVALID_ARG, "%s: min_views = %d (>= 1)", who, min_views);
    return APAP_OK;
}

}  // namespace apap

extern "C" {

size_t apap_covis_workspace_bytes(int n_points, int n_views) {
    if (n_views < 1 || n_views > kMaxViews || n_points < 0 || n_points > APAP_COVIS_MAX_POINTS) return 0;
    return covis_layout(n_points, n_views).total;
}

int apap_covis_tracks_device(apap_ctx *ctx, const float *d_pts, const int *d_idx, const int *view_offset, int n_views, float eps,
                             int *d_table, float *d_track_pts, int *d_point_track, int *d_n_tracks, int *d_status, void *d_work,
                             size_t work_bytes, void *stream) {
    const char *who = "apap_covis_tracks_device";
    (void)ctx;
    int rc = apap::covis_check(view_offset, n_views, eps, who);
    if (rc) return rc;
    if (!d_pts || !d_idx || !d_table || !d_track_pts || !d_point_track || !d_n_tracks || !d_status || !d_work)
        return apap::fail(APAP_ERR_INVALID_ARG, "%s: null device pointer", who);
    const int N = view_offset[n_views], n0 = view_offset[1], M = N - n0;
    const CovisLayout L = covis_layout(N, n_views);
    if (work_bytes < L.total) return apap::fail(APAP_ERR_WORKSPACE, "%s: workspace %zu < %zu bytes", who, work_bytes, L.total);
    if (((uintptr_t)d_work & 255) != 0 || ((uintptr_t)d_pts & 7) != 0 || ((uintptr_t)d_track_pts & 7) != 0)
        return apap::fail(APAP_ERR_INVALID_ARG, "%s: workspace must be 256-byte, points 8-byte aligned", who);
    if ((((uintptr_t)d_idx | (uintptr_t)d_table | (uintptr_t)d_point_track | (uintptr_t)d_n_tracks | (uintptr_t)d_status) & 3) != 0)
        return apap::fail(APAP_ERR_INVALID_ARG, "%s: int arrays must be 4-byte aligned", who);
    hipStream_t s = (hipStream_t)stream;
    char *w = (char *)d_work;
    int *d_offsets = (int *)(w + L.offsets), *d_first = (int *)(w + L.first), *d_owner = (int *)(w + L.owner), *d_rank = (int *)(w + L.rank);
    const float2 *pts = (const float2 *)d_pts;
    // from pageable memory in stream order: the copy returns once its source has been consumed
    hipError_t e = hipMemcpyAsync(d_offsets, view_offset, ((size_t)n_views + 1) * sizeof(int), hipMemcpyHostToDevice, s);
    if (e != hipSuccess) return apap::hip_fail(e, "apap_covis_tracks_device: offset upload");
    if (N > 0 && (e = hipMemsetAsync(d_first, 0xFF, (size_t)N * sizeof(int), s)) != hipSuccess)
        return apap::hip_fail(e, "apap_covis_tracks_device: candidate fill");
    if (M > 0 && N > 1)
        hipLaunchKernelGGL(k_covis_scan, dim3((M + kQueries - 1) / kQueries, (N - 1 + kChunk - 1) / kChunk), dim3(kQueries), 0, s, pts, N,
                           n0, eps, d_first);
    hipLaunchKernelGGL(k_covis_resolve, dim3(1), dim3(kResolveThreads), 0, s, pts, N, n0, eps, d_first, d_owner, d_rank, d_n_tracks,
                       d_status);
    if (N > 0) {
        const int blocks = (N + kThreads - 1) / kThreads;
        hipLaunchKernelGGL(k_covis_rows, dim3(blocks), dim3(kThreads), 0, s, pts, N, n0, n_views, (const int *)d_owner,
                           (const int *)d_rank, d_table, (float2 *)d_track_pts, d_point_track);
        hipLaunchKernelGGL(k_covis_last, dim3(blocks), dim3(kThreads), 0, s, N, n_views, (const int *)d_offsets,
                           (const int *)d_point_track, d_table);
        hipLaunchKernelGGL(k_covis_index, dim3((unsigned)(((size_t)N * n_views + kThreads - 1) / kThreads)), dim3(kThreads), 0, s, n_views,
                           d_idx, (const int *)d_n_tracks, d_table);
    }
    e = hipGetLastError();
    if (e != hipSuccess) return apap::hip_fail(e, "apap_covis_tracks_device launch");
    return APAP_OK;
}

int apap_triangulate_rays_device(apap_ctx *ctx, const double *d_origins, const double *d_dirs, const int *d_ray_offset, int n_rays_total,
                                 int n_tracks, double *d_X, double *d_lam_min, int *d_n_rays, void *stream) {
    const char *who = "apap_triangulate_rays_device";
    (void)ctx;
    if (n_tracks < 0 || n_rays_total < 0) return apap::fail(APAP_ERR_INVALID_ARG, "%s: %d tracks of %d rays (>= 0)", who, n_tracks, n_rays_total);
    if (!d_origins || !d_dirs || !d_ray_offset || !d_X || !d_lam_min || !d_n_rays)
        return apap::fail(APAP_ERR_INVALID_ARG, "%s: null device pointer", who);
    if ((((uintptr_t)d_origins | (uintptr_t)d_dirs | (uintptr_t)d_X | (uintptr_t)d_lam_min) & 7) != 0 ||
        (((uintptr_t)d_ray_offset | (uintptr_t)d_n_rays) & 3) != 0)
        return apap::fail(APAP_ERR_INVALID_ARG, "%s: doubles must be 8-byte, ints 4-byte aligned", who);
    if (n_tracks == 0) return APAP_OK;
    hipLaunchKernelGGL(k_triangulate_rays, dim3((n_tracks + kThreads - 1) / kThreads), dim3(kThreads), 0, (hipStream_t)stream, d_origins,
                       d_dirs, d_ray_offset, n_rays_total, n_tracks, d_X, d_lam_min, d_n_rays);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return apap::hip_fail(e, "apap_triangulate_rays_device launch");
    return APAP_OK;
}

int apap_triangulate_tracks_device(apap_ctx *ctx, const int *d_table, const float *d_track_pts, const int *d_n_tracks, int max_tracks,
                                   int n_views, const float *d_dst_pts, const int *dst_offset, const double *d_Kinv, const double *d_R,
                                   const double *d_origins, int n_cams, int center_cam, const int *view_cam, int min_views, double *d_X,
                                   double *d_lam_min, int *d_n_rays, void *stream) {
    const char *who = "apap_triangulate_tracks_device";
    (void)ctx;
    int rc = apap::triangulate_tracks_check(max_tracks, n_views, dst_offset, n_cams, center_cam, view_cam, min_views, who);
    if (rc) return rc;
    if (!d_table || !d_track_pts || !d_dst_pts || !d_Kinv || !d_R || !d_origins || !d_X || !d_lam_min || !d_n_rays)
        return apap::fail(APAP_ERR_INVALID_ARG, "%s: null device pointer", who);
    if ((((uintptr_t)d_track_pts | (uintptr_t)d_dst_pts | (uintptr_t)d_Kinv | (uintptr_t)d_R | (uintptr_t)d_origins | (uintptr_t)d_X |
          (uintptr_t)d_lam_min) & 7) != 0 ||
        (((uintptr_t)d_table | (uintptr_t)d_n_tracks | (uintptr_t)d_n_rays) & 3) != 0)
        return apap::fail(APAP_ERR_INVALID_ARG, "%s: points and doubles must be 8-byte, ints 4-byte aligned", who);
    if (max_tracks == 0) return APAP_OK;
    TrackViews T;
    T.n_views = n_views;
    T.center_cam = center_cam;
    T.min_views = min_views;
    for (int v = 0; v < kMaxViews; ++v) {
        T.dst_offset[v + 1] = dst_offset[v < n_views ? v + 1 : n_views];
        T.view_cam[v] = v < n_views ? view_cam[v] : 0;
    }
    T.dst_offset[0] = 0;
    hipLaunchKernelGGL(k_triangulate_tracks, dim3((max_tracks + kThreads - 1) / kThreads), dim3(kThreads), 0, (hipStream_t)stream, d_table,
                       (const float2 *)d_track_pts, d_n_tracks, max_tracks, (const float2 *)d_dst_pts, d_Kinv, d_R, d_origins, T, d_X,
                       d_lam_min, d_n_rays);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return apap::hip_fail(e, "apap_triangulate_tracks_device launch");
    return APAP_OK;
}

}  // extern "C"
