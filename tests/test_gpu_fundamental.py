"""The fundamental-matrix kernels (csrc/apap_fundamental.hip) on the MI355X against tests/fundamental_spec.py, byte for byte:
every hypothesis, every count, the winner, its count and mask, and F by its float64 bits (NaN pattern included), with guard
bytes around every output and the workspace pre-filled with 0xFF.  The resident form shows all of these; the host-buffer form
returns F, the mask and the count.  Inputs: tests/fundamental_cases.py (tests/test_fundamental_inputs.py asserts what each
reaches)."""
import ctypes

import numpy as np
import pytest

import fundamental_cases as C
import fundamental_spec as S

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
GUARD = 64
CASES = C.shape_cases() + C.edge_cases()


@pytest.fixture(scope="module")
def native_gpu(native):
    if native.lib().apap_device_count() < 1:
        pytest.skip("no HIP device")
    return native


def device():
    import torch
    return torch.device("cuda:0")


class Guarded:
    """``nbytes`` of device memory between two guards of sentinel bytes."""

    def __init__(self, nbytes, fill=SENTINEL):
        import torch
        self.n = nbytes
        self.buf = torch.full((nbytes + 2 * GUARD,), SENTINEL, dtype=torch.uint8, device=device())
        self.buf[GUARD:GUARD + nbytes] = fill
        assert self.buf.data_ptr() % 256 == 0
        self.ptr = self.buf.data_ptr() + GUARD

    def read(self, dtype):
        got = self.buf.cpu().numpy()
        assert (got[:GUARD] == SENTINEL).all() and (got[GUARD + self.n:] == SENTINEL).all(), "bytes outside an output were written"
        return got[GUARD:GUARD + self.n].copy().view(dtype)


def run_resident(native, src, dst, offsets, thresh, iterations, seed, single=False):
    """One call of apap_fundamental_batch_device (``single``: apap_fundamental_device) on guarded buffers.  ``offsets`` are
    absolute rows of src / dst.  Returns dict(F (P, 9), mask (rows of src), result (P, 2), boxes, H, winners, counts)."""
    import torch
    dev = device()
    P = len(offsets) - 1
    d_src = torch.from_numpy(np.ascontiguousarray(src)).to(dev)
    d_dst = torch.from_numpy(np.ascontiguousarray(dst)).to(dev)
    F, mask, result = Guarded(P * 72), Guarded(len(src)), Guarded(P * 8)
    lay = native.fundamental_workspace_layout(P, iterations)
    need = native.lib().apap_fundamental_workspace_bytes(int(offsets[-1] - offsets[0]), P, iterations)
    assert need == lay["total"]
    # [0, 256) guard, [256, 256 + need) the workspace pre-filled with 0xFF, then GUARD bytes of guard
    work = torch.full((256 + need + GUARD,), SENTINEL, dtype=torch.uint8, device=dev)
    work[256:256 + need] = 0xFF
    assert work.data_ptr() % 256 == 0
    w_ptr = work.data_ptr() + 256
    if single:
        assert P == 1 and offsets[0] == 0
        rc = native.lib().apap_fundamental_device(None, d_src.data_ptr(), d_dst.data_ptr(), int(offsets[1]), float(thresh), iterations,
                                                  ctypes.c_ulonglong(seed), F.ptr, mask.ptr, result.ptr, w_ptr, need, None)
    else:
        off = native._i32(offsets)
        rc = native.lib().apap_fundamental_batch_device(None, d_src.data_ptr(), d_dst.data_ptr(), native._ip(off), P, float(thresh),
                                                        iterations, ctypes.c_ulonglong(seed), F.ptr, mask.ptr, result.ptr, w_ptr, need,
                                                        None)
    native.check(rc)
    torch.cuda.synchronize()
    w = work.cpu().numpy()
    assert (w[:256] == SENTINEL).all() and (w[256 + need:] == SENTINEL).all(), "bytes outside the workspace were written"
    w = w[256:256 + need].copy()
    part = lambda name, count, dtype: w[lay[name]:lay[name] + count * np.dtype(dtype).itemsize].view(dtype)      # noqa: E731
    assert np.array_equal(part("offsets", P + 1, np.int32), np.asarray(offsets, np.int32))
    return dict(F=F.read(np.float64).reshape(P, 9), mask=mask.read(np.uint8), result=result.read(np.int32).reshape(P, 2),
                boxes=part("boxes", P * 8, np.float64).reshape(P, 8), H=part("hyps", P * iterations * 9, np.float64).reshape(P, iterations, 9),
                winners=part("winners", P * 9, np.float64).reshape(P, 9), counts=part("counts", P * iterations, np.int32).reshape(P, iterations))


def run_host(native, src, dst, thresh, iterations, seed):
    """apap_find_fundamental_ransac on guarded numpy buffers: (F (9,), mask (n,), count)."""
    n = len(src)
    s, d = np.ascontiguousarray(src, np.float32), np.ascontiguousarray(dst, np.float32)
    F = np.full(9 + 16, -7.0)
    mask = np.full(n + 2 * GUARD, SENTINEL, np.uint8)
    inl = np.full(3, -3, np.int32)
    native.check(native.lib().apap_find_fundamental_ransac(
        None, native._ptr(s, ctypes.c_float), native._ptr(d, ctypes.c_float), n, float(thresh), iterations, ctypes.c_ulonglong(seed),
        native._dp(F[8:]), native._ptr(mask[GUARD:], ctypes.c_uint8), native._ip(inl[1:]), -1))
    assert (F[:8] == -7.0).all() and (F[17:] == -7.0).all() and (mask[:GUARD] == SENTINEL).all() and (mask[GUARD + n:] == SENTINEL).all()
    assert inl[0] == -3 and inl[2] == -3
    return F[8:17].copy(), mask[GUARD:GUARD + n].copy(), int(inl[1])


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(got, want, what):
    bad = np.flatnonzero(bits(got).ravel() != bits(want).ravel())
    assert bad.size == 0, f"{what}: {bad.size} of {got.size} doubles differ, the first at {int(bad[0])}: " \
                          f"{got.ravel()[bad[0]]!r} against {want.ravel()[bad[0]]!r}"


def check_pair(got, p, rows, e, what):
    """Pair ``p`` of a resident call (its matches are ``rows`` of the mask) against the specification's core ``e``."""
    same_bits(got["boxes"][p], e["box"], f"{what}: boxes")
    same_bits(got["H"][p], e["H"], f"{what}: hypotheses")
    assert np.array_equal(got["counts"][p], e["counts"]), f"{what}: counts"
    assert got["result"][p].tolist() == [e["best"], e["count"]], f"{what}: winner and count"
    same_bits(got["winners"][p], e["winner"], f"{what}: the winner's matrix")
    assert np.array_equal(got["mask"][rows], e["mask"]), f"{what}: mask"
    same_bits(got["F"][p], e["F"], f"{what}: F")


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_resident_and_host_forms_equal_the_specification(native_gpu, case):
    e = C.expected(case)
    n = len(case.src)
    got = run_resident(native_gpu, case.src, case.dst, [0, n], case.thresh, case.iterations, case.seed)
    check_pair(got, 0, slice(0, n), e, case.name)
    F, mask, count = run_host(native_gpu, case.src, case.dst, case.thresh, case.iterations, case.seed)
    same_bits(F, e["F"], f"{case.name}: host F")
    no_model = bool(np.isnan(e["F"]).all())
    assert count == e["count"] and np.array_equal(mask, np.zeros_like(e["mask"]) if no_model else e["mask"])
    Fp, maskp = native_gpu.find_fundamental_ransac(case.src, case.dst, case.thresh, case.iterations, case.seed)
    Fs, masks = S.find_fundamental(case.src, case.dst, case.thresh, case.iterations, case.seed)
    assert (Fp is None) == (Fs is None) == no_model and np.array_equal(maskp, masks)
    if Fp is not None:
        same_bits(Fp, Fs, f"{case.name}: find_fundamental_ransac")


def test_single_pair_entry_point_and_a_reused_workspace(native_gpu):
    case = CASES[0]
    n = len(case.src)
    got = run_resident(native_gpu, case.src, case.dst, [0, n], case.thresh, case.iterations, case.seed, single=True)
    check_pair(got, 0, slice(0, n), C.expected(case), "apap_fundamental_device")
    # torch wrappers, one workspace for two calls of different size
    import torch
    from cvx_proj_amd import resident
    dev = device()
    work = torch.full((resident.fundamental_workspace_bytes(1000, 1, 64),), 0xFF, dtype=torch.uint8, device=dev)
    for name in ("n1000", "n63"):
        c = next(c for c in CASES if c.name == name)
        F, mask, result = resident.hip_fundamental(torch.from_numpy(c.src).to(dev), torch.from_numpy(c.dst).to(dev), c.thresh, c.iterations,
                                                   c.seed, work=work)
        e = C.expected(c)
        same_bits(F.cpu().numpy().reshape(9), e["F"], name)
        assert np.array_equal(mask.cpu().numpy(), e["mask"]) and result.cpu().tolist() == [e["best"], e["count"]]


def test_batch_equals_each_pairs_own_call(native_gpu):
    src, dst, off = C.batch_case()
    it, thresh, seed = 64, 3.0, S.SEED
    got = run_resident(native_gpu, src, dst, off, thresh, it, seed)
    assert (got["mask"][:off[0]] == SENTINEL).all()           # the rows before the first pair are not the call's
    own = []
    for p in range(len(off) - 1):
        s, d = src[off[p]:off[p + 1]], dst[off[p]:off[p + 1]]
        e = S.core(s, d, thresh, it, seed)
        check_pair(got, p, slice(off[p], off[p + 1]), e, f"pair {p} of the batch")
        alone = run_resident(native_gpu, s, d, [0, len(s)], thresh, it, seed)
        for k in ("F", "boxes", "H", "winners", "counts", "result"):
            assert got[k][p].tobytes() == alone[k][0].tobytes(), (p, k)
        own.append(e)
    # the host-buffer batch with the same offsets: rows before the first pair stay untouched
    F = np.full((len(off) - 1, 9), -7.0)
    mask = np.full(len(src), SENTINEL, np.uint8)
    inl = np.full(len(off) - 1, -3, np.int32)
    native_gpu.check(native_gpu.lib().apap_find_fundamental_ransac_batch(
        None, native_gpu._ptr(src, ctypes.c_float), native_gpu._ptr(dst, ctypes.c_float), native_gpu._ip(off), len(off) - 1, thresh, it,
        ctypes.c_ulonglong(seed), native_gpu._dp(F), native_gpu._ptr(mask, ctypes.c_uint8), native_gpu._ip(inl), -1))
    assert (mask[:off[0]] == SENTINEL).all()
    for p, e in enumerate(own):
        same_bits(F[p], e["F"], f"host batch, pair {p}")
        assert inl[p] == e["count"] and np.array_equal(mask[off[p]:off[p + 1]], e["mask"])
    # and the Python forms
    pairs = [(src[off[p]:off[p + 1]], dst[off[p]:off[p + 1]]) for p in range(len(off) - 1)]
    from cvx_proj_amd import spectral_method as SM
    for (Fb, mb), e in zip(SM.estimate_fundamental_batch(pairs, thresh, it, seed), own):
        same_bits(Fb, e["F"], "estimate_fundamental_batch")
        assert mb.dtype == np.float32 and np.array_equal(mb, e["mask"].astype(np.float32))


def test_device_f_feeds_the_resident_em(native_gpu):
    """hip_spectral_em given hip_fundamental's device tensor equals spectral_em given the host F: no host trip is needed."""
    import torch
    import spectral_spec as SP
    from cvx_proj_amd import resident
    native = native_gpu
    src, dst, c, o = SP.make_inputs("homography", 200, np.random.default_rng(3))
    F_host, fmask = native.find_fundamental_ransac(src, dst, 3.0, 256)
    assert F_host is not None and fmask.sum() >= 100
    _, hmask = native.find_homography_ransac(dst, src, 5.0)
    m = hmask.astype(np.float32).ravel()
    sp, mp = native.spectral_params(), native.model_params(native.MODEL_SDP, 0.5, 0.5)
    host = native.spectral_em(src, dst, c, o, F_host, sp, mp, 2, m)
    dev = device()
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)      # noqa: E731
    d_src, d_dst = t(src), t(dst)
    F_dev, _, result = resident.hip_fundamental(d_src, d_dst, 3.0, 256)
    out = resident.hip_spectral_em(d_src, d_dst, t(c), t(o), F_dev, sp, mp, 2, t(m))
    torch.cuda.synchronize()
    assert F_dev.cpu().numpy().tobytes() == F_host.tobytes() and int(result[1]) == int(fmask.sum())
    for a, b in zip(out, host):
        assert a.cpu().numpy().tobytes() == b.tobytes()
    # the batch form's F (P, 3, 3) is hip_spectral_em_batch's
    Fb, _, _ = resident.hip_fundamental_batch(torch.cat([d_src, d_src]), torch.cat([d_dst, d_dst]), [200, 200], 3.0, 256)
    assert Fb.shape == (2, 3, 3) and Fb.is_contiguous() and Fb[1].cpu().numpy().tobytes() == F_host.tobytes()


def test_device_argument_errors_write_nothing(native_gpu):
    import torch
    native = native_gpu
    dev = device()
    n, it = 64, 64
    src = torch.zeros((n, 2), dtype=torch.float32, device=dev)
    F, mask, result = Guarded(72), Guarded(n), Guarded(8)
    need = native.lib().apap_fundamental_workspace_bytes(n, 1, it)
    work = torch.full((need + 256,), SENTINEL, dtype=torch.uint8, device=dev)
    lib = native.lib()

    def call(n=n, thresh=3.0, it=it, src_ptr=src.data_ptr(), F_ptr=F.ptr, w_ptr=work.data_ptr(), w_bytes=need):
        return lib.apap_fundamental_device(None, src_ptr, src.data_ptr(), n, thresh, it, ctypes.c_ulonglong(1), F_ptr, mask.ptr, result.ptr,
                                           w_ptr, w_bytes, None)
    E = native.ERR_INVALID_ARG
    assert call(n=7) == E and call(thresh=-1.0) == E and call(thresh=float("nan")) == E and call(it=0) == E and call(it=(1 << 24) + 1) == E
    assert call(src_ptr=None) == E and call(F_ptr=None) == E and call(w_ptr=None) == E
    assert call(src_ptr=src.data_ptr() + 4) == E and call(F_ptr=F.ptr + 4) == E and call(w_ptr=work.data_ptr() + 8) == E
    assert call(w_bytes=need - 1) == native.ERR_WORKSPACE
    torch.cuda.synchronize()
    for g in (F, mask, result):
        assert (g.read(np.uint8) == SENTINEL).all()
    assert bool((work == SENTINEL).all())
