"""The host-buffer entry points as one layer: different calls in turn on one context's pooled buffers, optional outputs,
batches that do not start at zero, and a good call after a failed one.  Every assertion is byte equality between two calls
of the same library, so there is no tolerance anywhere in this file."""
import ctypes as C
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, ROOT)
from cvx_proj_amd.synth import synth_pair  # noqa: E402
from tools.spectral_rate import synth as spectral_synth  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def native_gpu(native):
    if native.lib().apap_device_count() < 1:
        pytest.skip("no HIP device")
    return native


def same(got, want, what):
    assert len(got) == len(want), what
    for k, (g, w) in enumerate(zip(got, want)):
        assert (g is None) == (w is None), (what, k)
        if g is not None:
            assert g.dtype == w.dtype and g.shape == w.shape, (what, k, g.dtype, w.dtype, g.shape, w.shape)
            assert g.tobytes() == w.tobytes(), (what, k)


def fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float)) if a is not None else None


def dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double)) if a is not None else None


def ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int)) if a is not None else None


# ---------------------------------------------------------------------------------------------------------------------
# The good calls: name -> f(native, ctx, half) -> tuple of arrays.  `half` halves the sizes (the first three calls only).

def pair_of(half):
    return synth_pair(32, 24, 20, 2, seed=5) if half else synth_pair(64, 48, 40, 2, seed=3)


def grid_of(p, rows=2, cols=2):
    """A float32 grid around the pair's global homography, each cell moved by up to half a pixel."""
    rng = np.random.default_rng(11)
    H = np.tile(p.Hg, (rows, cols, 1, 1))
    H[..., :2, 2] += rng.uniform(-0.5, 0.5, (rows, cols, 2))
    return H.astype(np.float32)


def call_local_warp(native, ctx, half=False):
    p = pair_of(half)
    return native.local_warp(p.img, grid_of(p), p.mesh[0], p.mesh[1], p.final_w, p.final_h, p.off_x, p.off_y, ctx=ctx)


def call_ransac(native, ctx, half=False):
    p = pair_of(half)
    H, mask = native.find_homography_ransac(p.src, p.dst, 5.0, ctx=ctx)
    assert H is not None        # the synthetic matches follow one homography
    return H, mask


def call_corner_detect(native, ctx, half=False):
    side = 20 if half else 40
    img = np.random.default_rng(2).integers(0, 256, (side, side), dtype=np.uint8)
    return native.corner_detect(img, 16, radius=2, ctx=ctx)


def call_match(native, ctx, half=False):
    rng = np.random.default_rng(6)
    q, t = (rng.integers(0, 256, (n, native.MATCH_DIM)).astype(np.float32) for n in (5, 7))
    return native.match_descriptors(q, t, ctx=ctx)


def call_equalize(native, ctx, half=False):
    return (native.equalize_hist(np.random.default_rng(7).integers(0, 200, (33, 17, 3), dtype=np.uint8), ctx=ctx),)


def model_inputs(n):
    p = synth_pair(64, 48, n, 2, seed=8)
    return p.src, p.dst, np.random.default_rng(9).uniform(0.1, 1.0, n).astype(np.float32)


def call_model_solve(native, ctx, half=False):
    return native.model_solve(*model_inputs(12), native.model_params(native.MODEL_LMS), ctx=ctx)


def call_local_homography(native, ctx, half=False, want_weights=False):
    p = synth_pair(64, 48, 16, 2, seed=4)
    x, y = np.meshgrid(np.linspace(10.0, 50.0, 3), np.linspace(12.0, 36.0, 2))      # 2 rows x 3 columns of cells
    H, W = native.local_homography(p.src, p.dst, np.stack([x, y], axis=-1), p.gamma, p.sigma, want_weights=want_weights, ctx=ctx)
    assert (W is not None) == want_weights
    return H, W


def call_local_homography_weights(native, ctx, half=False):
    return call_local_homography(native, ctx, half, want_weights=True)


def call_sift(native, ctx, half=False):
    img = np.random.default_rng(12).integers(0, 256, (48, 48), dtype=np.uint8)
    pts = np.array([[12.0, 13.5], [24.25, 24.0], [30.0, 17.0], [40.5, 41.0]], np.float32)
    return (native.sift_describe(img, pts, ctx=ctx),)


def call_blend(native, ctx, half=False):
    rng = np.random.default_rng(13)
    a, b = (rng.integers(0, 256, (31, 45, 3), dtype=np.uint8) for _ in range(2))
    return (native.uniform_blend(a, b, ctx=ctx),)


def call_flatten(native, ctx, half=False):
    return (native.invert_normalize_flatten(grid_of(pair_of(False), 3, 2), ctx=ctx),)


def call_local_stitch(native, ctx, half=False):
    p = pair_of(False)
    center = np.random.default_rng(14).integers(0, 256, p.shape, dtype=np.uint8)
    return native.local_stitch(p.img, center, grid_of(p), p.mesh[0], p.mesh[1], p.final_w, p.final_h, p.off_x, p.off_y,
                               want_inverse=True, ctx=ctx)


CALLS = {"local_warp": call_local_warp, "find_homography_ransac": call_ransac, "corner_detect": call_corner_detect,
         "match_descriptors": call_match, "equalize_hist": call_equalize, "model_solve": call_model_solve,
         "local_homography": call_local_homography, "local_homography with weights": call_local_homography_weights,
         "sift_describe": call_sift, "uniform_blend": call_blend, "invert_normalize_flatten": call_flatten,
         "local_stitch": call_local_stitch}
ORDER = list(CALLS)


@pytest.fixture(scope="module")
def fresh(native_gpu):
    """(name, half) -> the call's outputs on a context of its own, made for that call and closed after it; computed once."""
    cache = {}

    def get(name, half=False):
        if (name, half) not in cache:
            ctx = native_gpu.Context()
            try:
                cache[name, half] = CALLS[name](native_gpu, ctx, half)
            finally:
                ctx.close()
        return cache[name, half]
    return get


def run_in_turn(native, ctx, fresh):
    """Between them these calls put unrelated data into S_IMG, S_AUX, S_OUT, S_WORK, S_H, S_STATUS and S_DENORM of one pool."""
    for name in ORDER + ORDER[::-1]:
        same(CALLS[name](native, ctx), fresh(name), name)
    for name in ORDER[:3]:      # a slot that has grown serves a smaller request
        same(CALLS[name](native, ctx, True), fresh(name, True), name + " at half the size")


def test_entry_points_in_turn_on_one_context(native_gpu, fresh):
    ctx = native_gpu.Context()
    try:
        run_in_turn(native_gpu, ctx, fresh)
    finally:
        ctx.close()


def test_entry_points_in_turn_on_the_shared_pool(native_gpu, fresh):
    run_in_turn(native_gpu, None, fresh)


# ---------------------------------------------------------------------------------------------------------------------
# Optional outputs: what is asked for does not depend on what else is asked for.

MATCH_SENTINEL = (-9, -3.0, -9, -3.0)


def match_batch(native, q, t, qo, to, want2=(True, True)):
    """apap_match_descriptors_batch through ctypes: the four arrays, sentinel-filled before the call; an absent one is None."""
    n = len(q)
    out = [np.full(n, s, d) for s, d in zip(MATCH_SENTINEL, (np.int32, np.float32, np.int32, np.float32))]
    if not want2[0]:
        out[2] = None
    if not want2[1]:
        out[3] = None
    native.check(native.lib().apap_match_descriptors_batch(None, fp(q), fp(t), ip(qo), ip(to), len(qo) - 1, ip(out[0]), fp(out[1]),
                                                           ip(out[2]), fp(out[3]), -1))
    return out


def match_pairs(native, lead_q=0, lead_t=0):
    """Two pairs (5 x 7 and 9 x 4 descriptors) after `lead_q` / `lead_t` rows of NaN that no call may read."""
    rng = np.random.default_rng(21)
    i32 = lambda v: np.array(v, np.int32)      # noqa: E731
    q = np.full((lead_q + 14, native.MATCH_DIM), np.nan, np.float32)
    t = np.full((lead_t + 11, native.MATCH_DIM), np.nan, np.float32)
    q[lead_q:] = rng.integers(0, 256, (14, native.MATCH_DIM))
    t[lead_t:] = rng.integers(0, 256, (11, native.MATCH_DIM))
    return q, t, i32([lead_q, lead_q + 5, lead_q + 14]), i32([lead_t, lead_t + 7, lead_t + 11])


def test_match_second_neighbour_arrays_are_optional_one_by_one(native_gpu):
    # (the single form without both, against the oracle: tests/test_gpu_match.py::test_nearest_only)
    q, t, qo, to = match_pairs(native_gpu)
    full = match_batch(native_gpu, q, t, qo, to)
    for want2 in ((False, False), (True, False), (False, True)):
        got = match_batch(native_gpu, q, t, qo, to, want2)
        assert (got[2] is not None, got[3] is not None) == want2
        same([g for g in got if g is not None], [f for f, g in zip(full, got) if g is not None], want2)


def local_model_raw(native, pc, po, mw, v, params, want_info=True, want_status=True):
    cells = v.size // 2
    H = np.full((cells, 3, 3), np.nan, np.float32)
    info = np.full((cells, native.MODEL_INFO), np.nan) if want_info else None
    status = np.full(cells, -1, np.int32) if want_status else None
    native.check(native.lib().apap_local_model_solve(None, fp(pc), fp(po), fp(mw), len(pc), dp(v), cells, 0.5, 100.0, dp(params), fp(H),
                                                     dp(info), ip(status), -1))
    return H, info, status


def test_local_model_optional_arrays(native_gpu):
    native = native_gpu
    pc, po, w = model_inputs(24)
    x, y = np.meshgrid(np.linspace(10.0, 50.0, 3), np.linspace(12.0, 36.0, 2))
    v = np.ascontiguousarray(np.stack([x, y], axis=-1))
    params = native.model_params(native.MODEL_SDP, 0.5, 0.5)
    H, info, status = local_model_raw(native, pc, po, w, v, params)
    assert not np.isnan(H).any() and not (status == -1).any()
    same(local_model_raw(native, pc, po, w, v, params, want_info=False), (H, None, status), "no info_out")
    same(local_model_raw(native, pc, po, w, v, params, want_status=False), (H, info, None), "no status_out")
    same(local_model_raw(native, pc, po, w, v, params, want_info=False, want_status=False), (H, None, None), "H alone")
    # no match weights = every match weight 1 (a float32 product with 1 is exact); each cell against apap_model_solve without
    # them: tests/test_gpu_local_model.py::test_every_cell_equals_its_own_model_solve, kind "none"
    same(local_model_raw(native, pc, po, None, v, params), local_model_raw(native, pc, po, np.ones(24, np.float32), v, params),
         "no match_weights")


def em_pairs(lead=0):
    """Two pairs of 24 and 40 matches after `lead` rows of NaN, two problems on each: the arguments of the batch call."""
    pairs = [spectral_synth(24, seed=3), spectral_synth(40, seed=4)]
    cat = [np.concatenate([p[k] for p in pairs]) for k in (0, 1, 2, 3, 5)]
    cat = [np.concatenate([np.full((lead,) + a.shape[1:], np.nan, a.dtype), a]).astype(np.float32) for a in cat]
    F = np.ascontiguousarray(np.stack([p[4] for p in pairs]), dtype=np.float64)
    off = np.array([lead, lead + 24, lead + 64], np.int32)
    return cat, F, off, np.array([0, 1, 1, 0], np.int32)


def em_batch_raw(native, lead=0, want_status=True, em_steps=2):
    (src, dst, c, o, mask), F, off, pair_of_ = em_pairs(lead)
    B, M, k = len(pair_of_), 24 + 40 + 40 + 24, em_steps
    sp = np.stack([native.spectral_params(epi_weight=0.4 + 0.1 * b) for b in range(B)])
    mp = np.stack([native.model_params(native.MODEL_SDP, 0.5, 0.5) if b % 2 else native.model_params(native.MODEL_LMS) for b in range(B)])
    H = np.full((B, k, 3, 3), np.nan, np.float32)
    info = np.full((B, k, native.MODEL_INFO), np.nan)
    seg, rm, om = np.full(k * M, -5.0), np.full(k * M, -5.0, np.float32), np.full(k * M, -5.0, np.float32)
    sinfo = np.full((B, k, native.SPECTRAL_INFO), np.nan)
    status = np.full(B, -1, np.int32) if want_status else None
    native.check(native.lib().apap_spectral_em_batch(None, fp(src), fp(dst), fp(c), fp(o), dp(F), fp(mask), ip(off), 2, ip(pair_of_),
                                                     dp(sp), dp(mp), B, k, fp(H), dp(info), dp(seg), fp(rm), fp(om), dp(sinfo),
                                                     ip(status), -1))
    assert not (seg == -5.0).any() and not (rm == -5.0).any() and not (om == -5.0).any()
    return H, info, seg, rm, om, sinfo, status


@pytest.fixture(scope="module")
def em_zero_based(native_gpu):
    return em_batch_raw(native_gpu)


def test_em_batch_without_status_out(native_gpu, em_zero_based):
    assert not (em_zero_based[6] == -1).any()
    same(em_batch_raw(native_gpu, want_status=False), em_zero_based[:6] + (None,), "no status_out")


def test_local_warp_with_and_without_the_inverse(native_gpu):
    p = pair_of(False)
    args = (p.img, grid_of(p), p.mesh[0], p.mesh[1], p.final_w, p.final_h, p.off_x, p.off_y)
    canvas, hinv = native_gpu.local_warp(*args, want_inverse=True)
    alone, none = native_gpu.local_warp(*args, want_inverse=False)
    assert none is None and hinv is not None and np.isfinite(hinv).all()
    same((alone,), (canvas,), "canvas without the inverse")


# ---------------------------------------------------------------------------------------------------------------------
# Batches that do not start at zero: read from the first offset on, written at the offset positions, nothing before them.

def test_match_batch_with_a_first_offset(native_gpu):
    zero = match_batch(native_gpu, *match_pairs(native_gpu))
    got = match_batch(native_gpu, *match_pairs(native_gpu, lead_q=3, lead_t=2))
    for g, z, s in zip(got, zero, MATCH_SENTINEL):
        assert (g[:3] == s).all()
        same((g[3:],), (z,), "after the first offset")


def test_sift_batch_with_a_first_offset(native_gpu):
    native = native_gpu
    rng = np.random.default_rng(31)
    imgs = [rng.integers(0, 256, (23, 31), dtype=np.uint8), rng.integers(0, 256, (40, 48, 3), dtype=np.uint8)]
    pts = np.concatenate([rng.uniform(0, [im.shape[1], im.shape[0]], (n, 2)) for im, n in zip(imgs, (4, 6))]).astype(np.float32)
    i32 = lambda v: np.array(v, np.int32)      # noqa: E731
    hs, ws, cs = i32([23, 40]), i32([31, 48]), i32([1, 3])
    ptrs = (C.c_void_p * 2)(*[im.ctypes.data for im in imgs])

    def run(lead):
        p = np.concatenate([np.full((lead, 2), np.nan, np.float32), pts])     # the host-buffer form refuses a NaN where it reads one
        out = np.full((lead + 10, native.SIFT_DIM), -7.0, np.float32)
        native.check(native.lib().apap_sift_describe_batch(None, ptrs, ip(hs), ip(ws), ip(cs), 2, fp(p), ip(i32([lead, lead + 4, lead + 10])),
                                                           fp(out), -1))
        return out
    zero, got = run(0), run(3)
    assert not (zero == -7.0).any() and (got[:3] == -7.0).all()
    same((got[3:],), (zero,), "after the first offset")


def test_em_batch_with_a_first_offset(native_gpu, em_zero_based):
    # (the outputs of this call are per problem: the offsets say where its inputs are read)
    same(em_batch_raw(native_gpu, lead=5), em_zero_based, "first offset 5")


# ---------------------------------------------------------------------------------------------------------------------
# An error, then a good call, on one context.  Status-word and argument errors only: nothing here faults the GPU.

def test_a_good_call_after_a_failed_one(native_gpu, fresh):
    native = native_gpu
    p = pair_of(False)
    ctx = native.Context()
    try:
        short = p.mesh[1].copy()
        short[-1] = p.final_h - 5.0          # the last canvas rows lie in no cell
        with pytest.raises(native.ApapIndexError):
            native.local_warp(p.img, grid_of(p), p.mesh[0], short, p.final_w, p.final_h, p.off_x, p.off_y, ctx=ctx)
        same(call_local_warp(native, ctx), fresh("local_warp"), "local_warp after an index error")
        with pytest.raises(native.ApapSingularError):
            native.local_warp(p.img, np.zeros((2, 2, 3, 3), np.float32), p.mesh[0], p.mesh[1], p.final_w, p.final_h, p.off_x, p.off_y,
                              ctx=ctx)
        same(call_local_warp(native, ctx), fresh("local_warp"), "local_warp after a singular grid")

        pc, po, w = model_inputs(12)
        refused = native.model_params(native.MODEL_LMS)
        refused[0] = 3                       # no such mode: the device entry point refuses it, after the uploads
        with pytest.raises(native.ApapValueError) as e:
            native.model_solve(pc, po, w, refused, ctx=ctx)
        assert np.isnan(e.value.info).all()
        H, info = np.zeros((3, 3), np.float32), np.zeros(native.MODEL_INFO)      # the same call through ctypes: H is NaN too
        code = native.lib().apap_model_solve(native._h(ctx), fp(pc), fp(po), fp(w), 12, dp(refused), fp(H), dp(info), -1)
        assert code == native.ERR_INVALID_ARG and np.isnan(H).all() and np.isnan(info).all()
        same(call_model_solve(native, ctx), fresh("model_solve"), "model_solve after a refused mode")
        with pytest.raises(native.ApapValueError) as e:      # three matches determine no homography: decoded after the download
            native.model_solve(pc[:3], po[:3], w[:3], native.model_params(native.MODEL_LMS), ctx=ctx)
        assert int(e.value.info[native.MODEL_INFO_STATUS]) & native.STATUS_MODEL_DEGENERATE
        H = np.zeros((3, 3), np.float32)
        info = np.zeros(native.MODEL_INFO)
        params = native.model_params(native.MODEL_LMS)
        code = native.lib().apap_model_solve(native._h(ctx), fp(pc[:3].copy()), fp(po[:3].copy()), fp(w[:3].copy()), 3, dp(params), fp(H),
                                             dp(info), -1)
        assert code == native.ERR_INVALID_ARG and np.isnan(H).all()
        same((info,), (e.value.info,), "the degenerate call twice")
        same(call_model_solve(native, ctx), fresh("model_solve"), "model_solve after a degenerate selection")
    finally:
        ctx.close()
