"""The dehazing kernels (csrc/apap_dehaze.hip) on the MI355X against tests/dehaze_spec.py, byte for byte: the dark channel, the
atmospheric light, the transmission raw and refined, and the dehazed picture - through the host-buffer forms, the _device forms
and resident.hip_dehaze, on every named case of tests/dehaze_cases.py and on the synthetic scenes; and the contracts: guard
bytes around every output, a workspace whose prior contents do not matter, pooled buffers reused, a batch equal to its
single calls, out= in place of a fresh tensor, the result fed unchanged into the corner detector."""
import functools

import numpy as np
import pytest

import dehaze_cases as C
import dehaze_spec as S

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
GUARD = 256

ITEMS = dict(C.cases())
for _name in C.SCENES:
    _, _I, _, _p = C.scene(_name)
    ITEMS[_name] = (_I, _p)


@functools.lru_cache(maxsize=None)
def want(name):
    """The specification's stages of a case, computed once: D, A, t without refinement, t, J."""
    img, p = ITEMS[name]
    J, t, A = S.dehaze_q(img, **p)
    return dict(D=S.dark_channel(img, p["radius"]), A=A, raw=S.transmission_q(img, **dict(p, refine=0)), t=t, J=J)


@pytest.fixture(scope="module")
def native_gpu(native):
    if native.lib().apap_device_count() < 1:
        pytest.skip("no HIP device")
    return native


def device():
    import torch
    return torch.device("cuda:0")


class Guarded:
    """``nbytes`` of device memory between two guards of sentinel bytes, pre-filled with ``fill``."""

    def __init__(self, nbytes, fill=0xFF):
        import torch
        self.n = nbytes
        self.buf = torch.full((nbytes + 2 * GUARD,), SENTINEL, dtype=torch.uint8, device=device())
        self.buf[GUARD:GUARD + nbytes] = fill
        assert self.buf.data_ptr() % 256 == 0
        self.ptr = self.buf.data_ptr() + GUARD

    def read(self, dtype, shape=None):
        got = self.buf.cpu().numpy()
        assert (got[:GUARD] == SENTINEL).all() and (got[GUARD + self.n:] == SENTINEL).all(), "bytes outside a buffer were written"
        out = got[GUARD:GUARD + self.n].copy().view(dtype)
        return out if shape is None else out.reshape(shape)


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def as_batch(img):
    return np.ascontiguousarray(img[None, ..., None] if img.ndim == 2 else img[None])


@pytest.mark.parametrize("name", sorted(ITEMS))
def test_host_buffer_forms(native_gpu, name):
    from cvx_proj_amd import dehaze
    img, p = ITEMS[name]
    w = want(name)
    kw = dict(radius=p["radius"], omega=p["omega_q"] / 256.0, t0=p["t0_q"] / 4096.0, refine=p["refine"], eps=p["eps"])
    assert dehaze.dehaze_arguments(**kw) == C.pack(p)
    assert same(dehaze.dark_channel(img, p["radius"]), w["D"])
    assert same(dehaze.atmospheric_light(img, p["radius"]), w["A"])
    assert same(dehaze.transmission(img, **dict(kw, refine=0)), w["raw"])
    assert same(dehaze.transmission(img, **kw), w["t"])
    assert same(dehaze.dehaze(img, **kw), w["J"])
    J, t, A = dehaze.dehaze(img, return_parts=True, **kw)
    assert same(J, w["J"]) and same(t, w["t"]) and same(A, w["A"])


@pytest.mark.parametrize("name", sorted(ITEMS))
def test_device_forms_between_guard_bytes(native_gpu, name):
    """Every _device entry point: its outputs and its workspace (full of 0xFF on entry) between guard bytes."""
    import torch
    lib = native_gpu.lib()
    img, p = ITEMS[name]
    w = want(name)
    a = as_batch(img)
    _, h, wd, c = a.shape
    N, q = h * wd, C.pack(p)
    d_img = torch.from_numpy(a).to(device())
    need = lib.apap_dehaze_workspace_bytes(1, h, wd, c, p["refine"])
    need0 = lib.apap_dehaze_workspace_bytes(1, h, wd, c, 0)

    work, out = Guarded(need0), Guarded(N)
    native_gpu.check(lib.apap_dark_channel_device(None, d_img.data_ptr(), 1, h, wd, c, p["radius"], out.ptr, work.ptr, need0, None))
    torch.cuda.synchronize()
    work.read(np.uint8)
    assert same(out.read(np.uint8, (h, wd)), w["D"])

    work, out = Guarded(need0), Guarded(c)
    native_gpu.check(lib.apap_atmospheric_light_device(None, d_img.data_ptr(), 1, h, wd, c, p["radius"], out.ptr, work.ptr, need0, None))
    torch.cuda.synchronize()
    work.read(np.uint8)
    assert same(out.read(np.uint8), w["A"])

    for refine, key, size in ((0, "raw", need0), (p["refine"], "t", need)):
        work, out = Guarded(size), Guarded(2 * N)
        native_gpu.check(lib.apap_transmission_device(None, d_img.data_ptr(), 1, h, wd, c, q[0], q[1], q[2], refine, q[4], out.ptr, work.ptr, size, None))
        torch.cuda.synchronize()
        work.read(np.uint8)
        assert same(out.read(np.uint16, (h, wd)), w[key]), key

    work, out, t_out, A_out = Guarded(need), Guarded(N * c), Guarded(2 * N), Guarded(c)
    native_gpu.check(lib.apap_dehaze_device(None, d_img.data_ptr(), 1, h, wd, c, *q, out.ptr, t_out.ptr, A_out.ptr, work.ptr, need, None))
    torch.cuda.synchronize()
    work.read(np.uint8)
    assert same(out.read(np.uint8, img.shape), w["J"]) and same(t_out.read(np.uint16, (h, wd)), w["t"]) and same(A_out.read(np.uint8), w["A"])
    out = Guarded(N * c)                # t and A not asked for
    native_gpu.check(lib.apap_dehaze_device(None, d_img.data_ptr(), 1, h, wd, c, *q, out.ptr, None, None, work.ptr, need, None))
    torch.cuda.synchronize()
    work.read(np.uint8)
    assert same(out.read(np.uint8, img.shape), w["J"])


@pytest.mark.parametrize("name", sorted(ITEMS))
def test_resident_form(native_gpu, name):
    import torch
    from cvx_proj_amd import resident
    img, p = ITEMS[name]
    w = want(name)
    kw = dict(radius=p["radius"], omega=p["omega_q"] / 256.0, t0=p["t0_q"] / 4096.0, refine=p["refine"], eps=p["eps"])
    d_img = torch.from_numpy(np.ascontiguousarray(img)).to(device())
    J, t, A = resident.hip_dehaze(d_img, return_parts=True, **kw)
    assert J.dtype == torch.uint8 and J.shape == d_img.shape and t.dtype == torch.uint16
    assert same(J.cpu().numpy(), w["J"]) and same(t.cpu().numpy(), w["t"]) and same(A.cpu().numpy(), w["A"])
    assert same(resident.hip_dehaze(d_img, **kw).cpu().numpy(), w["J"])


def test_a_batch_equals_its_single_calls(native_gpu):
    import torch
    from cvx_proj_amd import dehaze, resident
    for channels in (3, 0):
        pics = [C.blocks(35, 131, 201, 5, channels), C.picture(35, 131, 202, channels), C._noise(35, 131, 203, channels)]
        for kw in (dict(radius=3, refine=5), dict(radius=2, refine=0), dict()):
            J, t, A = dehaze.dehaze_batch(pics, return_parts=True, **kw)
            assert J.shape == (3, *pics[0].shape) and t.shape == (3, 35, 131) and A.shape == (3, max(channels, 1))
            for k in range(3):
                wJ, wt, wA = S.dehaze(pics[k], **kw)
                assert same(J[k], wJ) and same(t[k], wt) and same(A[k], wA)
                assert same(dehaze.dehaze(pics[k], **kw), J[k])
            assert same(dehaze.dehaze_batch(np.stack(pics), **kw), J)
            d = torch.from_numpy(np.stack(pics)[..., None] if not channels else np.stack(pics)).to(device())
            rJ, rt, rA = resident.hip_dehaze(d, return_parts=True, **kw)
            assert same(rJ.cpu().numpy().reshape(J.shape), J) and same(rt.cpu().numpy(), t) and same(rA.cpu().numpy(), A)
    a = np.stack([as_batch(m)[0] for m in pics])
    assert same(native_gpu.dark_channel(a, 4), np.stack([S.dark_channel(m, 4) for m in pics]))
    assert same(native_gpu.atmospheric_light(a, 4), np.stack([S.atmospheric_light(m, 4) for m in pics]))
    assert same(native_gpu.transmission(a, 4, 200, 300, 6, 9), np.stack([S.transmission_q(m, 4, 200, 300, 6, 9) for m in pics]))


def test_a_dirty_workspace_and_out(native_gpu):
    """The workspace's prior contents (0xFF, then 0x00, then what the call before left, of another shape) do not matter; ``work=`` and
    ``out=`` are used; ``out`` may not be the picture itself."""
    import torch
    from cvx_proj_amd import resident
    lib = native_gpu.lib()
    name = "scene_60x50"
    img, p = ITEMS[name]
    w = want(name)
    h, wd, c = img.shape
    q = C.pack(p)
    d_img = torch.from_numpy(img).to(device())
    need = lib.apap_dehaze_workspace_bytes(1, h, wd, c, p["refine"])
    assert need == resident.dehaze_workspace_bytes(1, h, wd, c, p["refine"])
    work = None
    for fill in (0xFF, 0x00, None):
        work = Guarded(need, fill) if fill is not None else work
        out = Guarded(img.size)
        native_gpu.check(lib.apap_dehaze_device(None, d_img.data_ptr(), 1, h, wd, c, *q, out.ptr, None, None, work.ptr, need, None))
        torch.cuda.synchronize()
        work.read(np.uint8)
        assert same(out.read(np.uint8, img.shape), w["J"])
    kw = dict(radius=p["radius"], omega=p["omega_q"] / 256.0, t0=p["t0_q"] / 4096.0, refine=p["refine"], eps=p["eps"])
    scratch = torch.full((need + 4096,), 0x5A, dtype=torch.uint8, device=device())
    other, po = ITEMS["tile_recover_17x65"]
    resident.hip_dehaze(torch.from_numpy(other).to(device()), radius=po["radius"], refine=po["refine"], work=scratch)     # leaves its own behind
    out = torch.full_like(d_img, 7)
    got = resident.hip_dehaze(d_img, out=out, work=scratch, **kw)
    assert got is out and same(out.cpu().numpy(), w["J"])
    with pytest.raises(ValueError, match="out must be"):
        resident.hip_dehaze(d_img, out=d_img, **kw)
    with pytest.raises(ValueError, match="out must be"):
        resident.hip_dehaze(d_img, out=out[:-1], **kw)


def test_pooled_buffers_are_reused(native_gpu):
    from cvx_proj_amd import dehaze
    ctx = native_gpu.Context()
    a, pa = ITEMS["scene_40x200"]
    b, pb = ITEMS["grey_refine0"]
    ka, kb = dict(radius=pa["radius"], refine=pa["refine"]), dict(radius=pb["radius"], refine=pb["refine"])
    first = dehaze.dehaze(a, ctx=ctx, **ka)
    other = dehaze.dehaze(b, ctx=ctx, return_parts=True, **kb)
    assert same(first, want("scene_40x200")["J"]) and same(dehaze.dehaze(a, ctx=ctx, **ka), first)
    assert same(other[0], want("grey_refine0")["J"]) and same(other[1], want("grey_refine0")["t"])
    assert same(dehaze.dark_channel(a, pa["radius"], ctx=ctx), want("scene_40x200")["D"])
    assert same(dehaze.transmission(b, radius=pb["radius"], refine=0, ctx=ctx), want("grey_refine0")["raw"])
    ctx.close()


def test_the_result_feeds_the_corner_detector(native_gpu):
    import torch
    from cvx_proj_amd import resident
    name = "scene_96x128"
    img, p = ITEMS[name]
    d_J = resident.hip_dehaze(torch.from_numpy(img).to(device()), radius=p["radius"], refine=p["refine"])
    pts, resp, count = resident.hip_corner_detect(d_J, 200)
    ref = resident.hip_corner_detect(torch.from_numpy(want(name)["J"]).to(device()), 200)
    assert int(count) > 0 and int(count) == int(ref[2])
    assert same(pts.cpu().numpy(), ref[0].cpu().numpy()) and same(resp.cpu().numpy(), ref[1].cpu().numpy())
