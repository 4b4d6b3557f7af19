"""The resident (``*_device``) entry points of ``libapap_hip.so`` on torch tensors, launched on the current stream of the
tensors' device: every solve through ``apap_solve_batch_device`` or ``apap_solve_warp_batch_device``, every warp through
``apap_warp_batch_device`` (the C ABI's single-pair forms wrap these).  ``pipeline`` and ``dist`` reach the GPU through this
module.  No CPU fallback.  Importing it in a process that loaded the library before torch raises ``_native.ApapError``."""
from __future__ import annotations

import ctypes

import numpy as np

from . import _native
from ._native import _addrs, _dp, _i32, _ip

if _native._lib is not None and not _native._torch_at_load:
    raise _native.ApapError(_native.ERR_HIP, "cvx_proj_amd's library was loaded before torch was imported: torch cannot see the GPU "
                                             "in this process.  Import torch first (or set APAP_HIP_PRELOAD_TORCH=1)")

import torch  # noqa: E402


def solve_workspace_bytes(ctx, n, cells, batch=1):
    """Scratch of a solve of ``batch`` pairs of ``n`` keypoints over ``cells`` cells (at least 256 bytes)."""
    return max(_native.lib().apap_solve_batch_workspace_bytes(_native._h(ctx), n, cells, batch), 256)


def warp_workspace_bytes(shape, final_w, final_h, batch=1):
    """Workspace of a warp of ``batch`` pairs over a ``shape`` = (rows, cols) mesh onto a final_w x final_h canvas."""
    return _native.lib().apap_warp_batch_workspace_bytes(shape[0], shape[1], final_w, final_h, batch)


def _scratch(work, nbytes, dev):
    """``work`` when it holds ``nbytes``, else a new uint8 tensor of that size."""
    return work if work is not None and work.numel() >= nbytes else torch.empty(nbytes, dtype=torch.uint8, device=dev)


def _stream(dev):
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _needs_device(t, who):
    if not t.is_cuda:
        raise _native.ApapError(_native.ERR_NO_DEVICE, f"{who} needs CUDA/HIP tensors; there is no CPU fallback")


def _contiguous(tensors, dev, who):
    """Every ``(tensor, dtype)`` of ``tensors`` must be a contiguous tensor of that dtype on ``dev``."""
    for t, want in tensors:
        if t.dtype != want or not t.is_contiguous() or t.device != dev:
            raise ValueError(f"{who}: inputs must be contiguous {want} tensors on {dev}")


def _status(status, shape, dev, who, flat=False):
    """``status`` checked - contiguous int32 on ``dev``, of ``shape`` or, with ``flat``, of as many elements - or a new zeroed one."""
    if status is None:
        return torch.zeros(shape, dtype=torch.int32, device=dev)
    n = int(np.prod(shape))
    if status.dtype != torch.int32 or (status.numel() != n if flat else status.shape != shape) or status.device != dev \
            or not status.is_contiguous():
        raise ValueError(f"{who}: status must be a contiguous int32 tensor of {n} elements on {dev}")
    return status


def _solve(tables, denorms, vertices, gamma, sigma, batch, ctx=None, out=None, work=None):
    """``apap_solve_batch_device``: ``batch`` pairs (``tables`` (batch, n, 32) or (n, 32), ``denorms`` (batch, 36) or (36,)) over
    one set of ``vertices`` (cells, 2) -> H (batch * cells, 9) float32.  ``out`` and ``work`` are used when large enough."""
    n, cells, dev = tables.shape[-2], vertices.shape[0], tables.device
    H = out[:batch * cells] if out is not None and out.shape[0] >= batch * cells else \
        torch.empty((batch * cells, 9), dtype=torch.float32, device=dev)
    if cells == 0:
        return H
    work = _scratch(work, solve_workspace_bytes(ctx, n, cells, batch), dev)
    _native.check(_native.lib().apap_solve_batch_device(_native._h(ctx), tables.data_ptr(), n, vertices.data_ptr(), 0, cells,
                                                        float(gamma), float(sigma), denorms.data_ptr(), H.data_ptr(), batch,
                                                        work.data_ptr(), work.numel(), _stream(dev)))
    return H


def _image(t):
    """(pointer, stride in bytes, h, w) of one (h, w, 3) image shared by every pair, of a (B, h, w, 3) stack, or of None."""
    if t is None:
        return None, 0, 0, 0
    if t.dim() == 3:
        return t.data_ptr(), 0, t.shape[0], t.shape[1]
    return t.data_ptr(), t.shape[1] * t.shape[2] * 3, t.shape[1], t.shape[2]


def _warp(ctx, phases, shape, mesh_w, mesh_h, final_w, final_h, off_x, off_y, batch, work, status, imgs=None, H=None, out=None,
          centers=None, rows=None, hinv_out=None):
    """``apap_warp_batch_device`` on ``work``'s device.  ``rows`` = (row_begin, row_count), default the whole canvas."""
    row_begin, row_count = (0, final_h) if rows is None else rows
    i_ptr, i_stride, ih, iw = _image(imgs)
    c_ptr, c_stride, ch, cw = _image(centers)
    _native.check(_native.lib().apap_warp_batch_device(
        _native._h(ctx), i_ptr, i_stride, ih, iw, c_ptr, c_stride, ch, cw, None if H is None else H.data_ptr(), shape[0], shape[1],
        mesh_w.data_ptr(), mesh_w.numel(), mesh_h.data_ptr(), mesh_h.numel(), final_w, final_h, off_x, off_y, row_begin, row_count,
        None if out is None else out.data_ptr(), row_count * final_w * 3, None if hinv_out is None else hinv_out.data_ptr(), batch,
        int(phases), work.data_ptr(), work.numel(), status.data_ptr(), _stream(work.device)))


def hip_solve(table, denorm, vertices, gamma, sigma, ctx=None, out=None, work=None):
    """Default ``solve_fn`` of :mod:`cvx_proj_amd.dist`: one pair, H (cells, 9) float32.  ``out`` (>= cells x 9 float32) and
    ``work`` (uint8 scratch) are reused when given and large enough - a solver that runs every step keeps them - else allocated."""
    _needs_device(table, "hip_solve")
    return _solve(table, denorm, vertices, gamma, sigma, 1, ctx, out, work)


def hip_solve_batch(tables, denorms, vertices, gamma, sigma, ctx=None):
    """Several pairs (equal keypoint and cell counts, one shared mesh) in ONE launch:
    ``tables`` (B, n, 32), ``denorms`` (B, 36), ``vertices`` (cells, 2) -> H (B, cells, 9)."""
    _needs_device(tables, "hip_solve_batch")
    batch = tables.shape[0]
    return _solve(tables, denorms, vertices, gamma, sigma, batch, ctx).view(batch, vertices.shape[0], 9)


def hip_warp_rows(img, H, mesh_w, mesh_h, final_w, final_h, off_x, off_y, row_begin, row_count, out_band, shape, ctx=None,
                  work=None, status=None, sampling=None):
    """Default ``warp_fn`` of :mod:`cvx_proj_amd.dist`: warps canvas rows ``[row_begin, row_begin + row_count)`` of one pair into
    ``out_band``.  ``work`` / ``status`` are reused when given.  ``sampling``: as in :func:`hip_warp_batch`."""
    _native.sampling_value(sampling, "hip_warp_rows")
    _needs_device(img, "hip_warp_rows")
    return hip_warp_batch(img, H.view(1, -1, 9), mesh_w, mesh_h, final_w, final_h, off_x, off_y, shape, out=out_band, ctx=ctx,
                          work=work, status=status, rows=(row_begin, row_count), sampling=sampling)[1]


def hip_warp_batch(imgs, H, mesh_w, mesh_h, final_w, final_h, off_x, off_y, shape, out=None, centers=None, ctx=None,
                   work=None, status=None, phases=_native.WARP_ALL, rows=None, hinv_out=None, sampling=None):
    """Backward warp of a BATCH of independent pairs in one set of launches (``apap_warp_batch_device``, grid.z = pair):
    ``imgs`` (B, h, w, 3) uint8 - or (h, w, 3): one image for every pair -, ``H`` (B, cells, 9) float32 (what
    ``hip_solve_batch`` returns), one set of edges, canvas size and offsets for all -> canvases (B, final_h, final_w, 3).
    ``centers`` (B, ch, cw, 3) or (ch, cw, 3): the fused stitch (warp + paste + uniform_blend).  ``phases``: which of
    geometry tables / per-cell set-up / gather run on ``work`` (a caller that keeps ``work`` runs the geometry once).
    ``rows`` = (row_begin, row_count): a band of every canvas; ``out`` is then (B, row_count, final_w, 3).  ``sampling``:
    ``None`` (the context's ``warp_sampling``), ``"nearest"`` or ``"bilinear"`` for this call only."""
    _native.sampling_value(sampling, "hip_warp_batch")
    _needs_device(H, "hip_warp_batch")
    batch, dev = H.shape[0], H.device
    if out is None:
        out = torch.empty((batch, final_h if rows is None else rows[1], final_w, 3), dtype=torch.uint8, device=dev)
    work = _scratch(work, warp_workspace_bytes(shape, final_w, final_h, batch), dev)
    if status is None:
        status = torch.zeros(1, dtype=torch.int32, device=dev)
    with _native.sampling_scope(ctx, sampling, "hip_warp_batch") as ctx:
        _warp(ctx, phases, shape, mesh_w, mesh_h, final_w, final_h, off_x, off_y, batch, work, status, imgs=imgs, H=H, out=out,
              centers=centers, rows=rows, hinv_out=hinv_out)
    return out, status


class WarpPlan:
    """One mesh / canvas geometry's warp workspace, kept between pairs (what the resident callers - ``Pipeline``, ``bench.py`` -
    hold): the canvas row / column -> cell tables are built ONCE, here (``APAP_WARP_GEOMETRY``: they depend on the edges,
    the canvas size and the offsets only); ``solve()`` is the per-cell solve whose tail leaves every cell warp ready in
    this workspace (``apap_solve_warp_batch_device``); ``cells()`` does that for a grid that came from elsewhere
    (``APAP_WARP_CELLS``); ``gather()`` is K3 alone (``APAP_WARP_GATHER``).  ``batch`` pairs share the geometry.
    ``status``: the device status word of the plan's phases.  The geometry phase's bits (``geo_status``) hold for the plan's
    life and stay in it; ``begin()`` drops the others (kernels only OR bits in) before a pair, so one pair's singular grid is
    not every later pair's."""

    def __init__(self, mesh, shape, final_w, final_h, off_x, off_y, dev, batch=1, ctx=None):
        self.rows, self.cols = shape
        self.geo = (int(final_w), int(final_h), int(off_x), int(off_y))
        self.dev, self.batch, self.ctx = dev, int(batch), ctx
        self.mesh_w = torch.from_numpy(np.ascontiguousarray(mesh[0], dtype=np.float64)).to(dev)
        self.mesh_h = torch.from_numpy(np.ascontiguousarray(mesh[1], dtype=np.float64)).to(dev)
        self.nbytes = warp_workspace_bytes(shape, self.geo[0], self.geo[1], self.batch)
        if not self.nbytes:
            raise ValueError("WarpPlan: bad geometry")
        self.work = torch.zeros(self.nbytes, dtype=torch.uint8, device=dev)
        self.status = torch.zeros(1, dtype=torch.int32, device=dev)
        self._phase(_native.WARP_GEOMETRY)
        self.geo_status = int(self.status.cpu()[0])      # the geometry phase's bits, what begin() re-seeds the word with

    def begin(self):
        """Drop the per-pair status bits (singular cell, unprepared workspace) before a pair's phases."""
        self.status.fill_(self.geo_status)

    def status_word(self):
        """``status`` as an int (synchronises)."""
        return int(self.status.cpu()[0])

    def _phase(self, phases, ctx=None, **kw):
        fw, fh, ox, oy = self.geo
        _warp(self.ctx if ctx is None else ctx, phases, (self.rows, self.cols), self.mesh_w, self.mesh_h, fw, fh, ox, oy, self.batch,
              self.work, self.status, **kw)

    def solve(self, tables, denorms, vertices, gamma, sigma, out=None, work=None):
        """``tables`` (B, n, 32) or (n, 32), ``denorms`` (B, 36) or (36,), ``vertices`` (cells, 2) -> H (B * cells, 9) float32, and
        every cell's inverse / record / exact floats in this plan's workspace."""
        _needs_device(tables, "WarpPlan.solve")
        n = tables.shape[-2]
        cells = self.rows * self.cols
        if vertices.shape[0] != cells:
            raise ValueError(f"WarpPlan.solve: {vertices.shape[0]} vertices for a {self.rows} x {self.cols} mesh")
        H = out if out is not None else torch.empty((self.batch * cells, 9), dtype=torch.float32, device=self.dev)
        work = _scratch(work, solve_workspace_bytes(self.ctx, n, cells, self.batch), self.dev)
        fw, fh, ox, oy = self.geo
        _native.check(_native.lib().apap_solve_warp_batch_device(
            _native._h(self.ctx), tables.data_ptr(), n, vertices.data_ptr(), 0, float(gamma), float(sigma), denorms.data_ptr(),
            H.data_ptr(), self.batch, work.data_ptr(), work.numel(), self.rows, self.cols, self.mesh_w.data_ptr(), self.mesh_w.numel(),
            self.mesh_h.data_ptr(), self.mesh_h.numel(), fw, fh, ox, oy, self.work.data_ptr(), self.nbytes, self.status.data_ptr(),
            _stream(self.dev)))
        return H

    def cells(self, H, hinv_out=None):
        """Per-cell set-up from a grid that was not solved into this plan (``H`` (B * cells, 9) float32)."""
        self._phase(_native.WARP_CELLS, H=H, hinv_out=hinv_out)

    def gather(self, imgs, out=None, centers=None, rows=None, sampling=None):
        """K3: ``imgs`` (B, h, w, 3) or (h, w, 3) -> canvases (B, rows, final_w, 3).  ``sampling``: ``None`` (the plan's context's
        ``warp_sampling``), ``"nearest"`` or ``"bilinear"`` for this gather only; the set-up phases do not depend on it."""
        _native.sampling_value(sampling, "WarpPlan.gather")
        fw, fh, _, _ = self.geo
        if out is None:
            out = torch.empty((self.batch, fh if rows is None else rows[1], fw, 3), dtype=torch.uint8, device=self.dev)
        with _native.sampling_scope(self.ctx, sampling, "WarpPlan.gather") as ctx:
            self._phase(_native.WARP_GATHER, ctx=ctx, imgs=imgs, out=out, centers=centers, rows=rows)
        return out


def fundamental_workspace_bytes(n_total, n_pairs=1, iterations=_native.RANSAC_ITERATIONS):
    """Workspace of ``hip_fundamental`` / ``hip_fundamental_batch`` for ``n_pairs`` pairs of ``n_total`` matches in all
    (``_native.fundamental_workspace_layout`` names its parts); 0 for invalid arguments."""
    return _native.lib().apap_fundamental_workspace_bytes(int(n_total), int(n_pairs), int(iterations))


def hip_fundamental_batch(src, dst, pair_lengths, thresh=3.0, iterations=_native.RANSAC_ITERATIONS, seed=_native.RANSAC_SEED,
                          ctx=None, work=None):
    """``apap_fundamental_batch_device`` on the current stream of the tensors' device, no host synchronisation: the fundamental
    matrices of many pairs in five kernel launches.  src / dst (N, 2) float32, the pairs concatenated, pair p of
    ``pair_lengths[p]`` >= 8 matches (a host list).  Returns (F (P, 3, 3) float64 - all NaN where a pair has no model -, mask
    (N,) uint8: the winning hypothesis's inliers, result (P, 2) int32: {winning hypothesis, its inlier count}) as device
    tensors.  ``F[p]`` is what ``hip_spectral`` / ``hip_spectral_em`` take as their ``F``, and ``F`` what
    ``hip_spectral_em_batch`` takes.  ``work`` (uint8) is used when it holds ``fundamental_workspace_bytes(N, P, iterations)``;
    afterwards it holds every hypothesis and count.  Same bytes as ``_native.find_fundamental_ransac_batch``."""
    who = "hip_fundamental_batch"
    _needs_device(src, who)
    dev = src.device
    off = _native.fundamental_arguments(pair_lengths, thresh, iterations, who)
    N, P = int(off[-1]), len(off) - 1
    _contiguous(((src, torch.float32), (dst, torch.float32)), dev, who)
    if src.shape != (N, 2) or dst.shape != src.shape:
        raise ValueError(f"{who}: shapes ({N}, 2), ({N}, 2) expected; got {tuple(src.shape)} and {tuple(dst.shape)}")
    F = torch.empty((P, 3, 3), dtype=torch.float64, device=dev)
    mask = torch.empty(N, dtype=torch.uint8, device=dev)
    result = torch.empty((P, 2), dtype=torch.int32, device=dev)
    work = _scratch(work, fundamental_workspace_bytes(N, P, iterations), dev)
    _native.check(_native.lib().apap_fundamental_batch_device(
        _native._h(ctx), src.data_ptr(), dst.data_ptr(), _ip(off), P, float(thresh), int(iterations), ctypes.c_ulonglong(seed),
        F.data_ptr(), mask.data_ptr(), result.data_ptr(), work.data_ptr(), work.numel(), _stream(dev)))
    return F, mask, result


def hip_fundamental(src, dst, thresh=3.0, iterations=_native.RANSAC_ITERATIONS, seed=_native.RANSAC_SEED, ctx=None, work=None):
    """``apap_fundamental_device``: one pair, the batch of one (see ``hip_fundamental_batch``).  Returns (F (3, 3) float64, mask
    (n,) uint8, result (2,) int32) as device tensors, not synchronised."""
    _needs_device(src, "hip_fundamental")
    F, mask, result = hip_fundamental_batch(src, dst, [src.shape[0]], thresh, iterations, seed, ctx=ctx, work=work)
    return F[0], mask, result[0]


def hip_fft2(x, inverse=False, ctx=None, work=None, out=None):
    """``apap_fft2_device`` on the current stream of the tensor's device: the 2-D transform of an (h, w) or (planes, h, w)
    complex128 tensor, 5-smooth lengths 2 .. 4096; the inverse is scaled by 1 / (h w).  ``out`` may be ``x`` itself.  ``work``
    (uint8, 256-byte aligned) receives the twiddle tables and, for h > 1024, a turned copy of the planes.  Same bytes as ``_native.fft2``.  Not synchronised."""
    who = "hip_fft2"
    _needs_device(x, who)
    dev = x.device
    _contiguous(((x, torch.complex128),), dev, who)
    if x.dim() not in (2, 3) or x.numel() == 0:
        raise ValueError(f"{who}: an (h, w) or (planes, h, w) tensor expected; got {tuple(x.shape)}")
    planes, h, w = (1, *x.shape) if x.dim() == 2 else x.shape
    if out is None:
        out = torch.empty_like(x)
    else:
        _contiguous(((out, torch.complex128),), dev, who)
        if out.shape != x.shape:
            raise ValueError(f"{who}: out must have the shape of x")
    work = _scratch(work, max(_native.lib().apap_fft2_workspace_bytes(int(planes), int(h), int(w)), 256), dev)
    _native.check(_native.lib().apap_fft2_device(_native._h(ctx), x.data_ptr(), out.data_ptr(), int(planes), int(h), int(w),
                                                 1 if inverse else 0, work.data_ptr(), work.numel(), _stream(dev)))
    return out


def notch_denoise_workspace_bytes(n_images, h, w, channels):
    """Workspace of ``hip_notch_denoise`` (0 for invalid arguments): twiddles, planes x h x w complex128 (twice for h > 1024), the
    equalised pictures."""
    return _native.lib().apap_notch_denoise_workspace_bytes(int(n_images), int(h), int(w), int(channels))


def hip_notch_denoise(imgs, spacing=48, r=5, sn=9, equalize=True, out="float64", ctx=None, work=None):
    """``apap_notch_denoise_device`` on the current stream of the tensor's device, no host synchronisation: uint8 pictures
    (h, w), (h, w, c) or (n, h, w, c), c <= 4; returns a float64 or uint8 tensor of that shape.  The uint8 result is what
    ``hip_corner_detect`` takes, so a resident chain denoises and then detects without a host trip.  Same bytes as
    ``denoise.notch_denoise``."""
    who = "hip_notch_denoise"
    _needs_device(imgs, who)
    dev = imgs.device
    _contiguous(((imgs, torch.uint8),), dev, who)
    if imgs.dim() not in (2, 3, 4) or imgs.numel() == 0 or out not in _native.DENOISE_OUT:
        raise ValueError(f"{who}: uint8 pictures (h, w), (h, w, c) or (n, h, w, c) and out 'float64' or 'uint8' expected")
    n, h, w, c = {2: (1, *imgs.shape, 1), 3: (1, *imgs.shape), 4: tuple(imgs.shape)}[imgs.dim()]
    res = torch.empty(imgs.shape, dtype=torch.float64 if out == "float64" else torch.uint8, device=dev)
    work = _scratch(work, max(notch_denoise_workspace_bytes(n, h, w, c), 256), dev)
    _native.check(_native.lib().apap_notch_denoise_device(
        _native._h(ctx), imgs.data_ptr(), int(n), int(h), int(w), int(c), 1 if equalize else 0, int(spacing), int(r), int(sn),
        _native.DENOISE_OUT[out], res.data_ptr(), work.data_ptr(), work.numel(), _stream(dev)))
    return res


def covis_workspace_bytes(n_points, n_views):
    """Workspace of ``hip_covis_tracks`` (``_native.covis_workspace_layout`` names its parts); 0 for invalid arguments."""
    return _native.lib().apap_covis_workspace_bytes(int(n_points), int(n_views))


def hip_covis_tracks(pts, idx, view_lengths, eps=_native.COVIS_EPS, status=None, ctx=None, work=None):
    """``apap_covis_tracks_device`` on the current stream of the tensors' device, no host synchronisation: the reference's
    ``get_covid``.  pts (N, 2) float32 and idx (N,) int32 hold the views' observations one after the other, view v of
    ``view_lengths[v]`` >= 0 (a host list of 1 .. 8 lengths, N <= 65 536).  Returns (table (N, V) int32, track_pts (N, 2)
    float32, point_track (N,) int32, n_tracks (1,) int32) as device tensors: table and track_pts are sized for the worst
    case and only their first n_tracks rows are written.  ``status`` (one int32, zeroed): see APAP_STATUS_COVIS_BOUND.  Same
    bytes as ``_native.covis_tracks``."""
    who = "hip_covis_tracks"
    _needs_device(pts, who)
    dev = pts.device
    lengths = [int(x) for x in view_lengths]
    if not 1 <= len(lengths) <= _native.COVIS_MAX_VIEWS or any(x < 0 for x in lengths):
        raise ValueError(f"{who}: 1 .. {_native.COVIS_MAX_VIEWS} views of >= 0 observations; got {lengths}")
    N, V = sum(lengths), len(lengths)
    if N > _native.COVIS_MAX_POINTS:
        raise ValueError(f"{who}: {N} observations in all (at most {_native.COVIS_MAX_POINTS}: the first-candidate scan is quadratic)")
    e = np.float32(eps)
    if not (e >= 0 and np.isfinite(e)):
        raise ValueError(f"{who}: eps = {eps} (finite, >= 0)")
    _contiguous(((pts, torch.float32), (idx, torch.int32)), dev, who)
    if pts.shape != (N, 2) or idx.shape != (N,):
        raise ValueError(f"{who}: shapes ({N}, 2) and ({N},) expected; got {tuple(pts.shape)} and {tuple(idx.shape)}")
    off = np.zeros(V + 1, np.int32)
    off[1:] = np.cumsum(lengths)
    rows = max(N, 1)        # (an empty tensor has no address)
    table = torch.empty((rows, V), dtype=torch.int32, device=dev)
    track_pts = torch.empty((rows, 2), dtype=torch.float32, device=dev)
    point_track = torch.empty(rows, dtype=torch.int32, device=dev)
    n_tracks = torch.empty(1, dtype=torch.int32, device=dev)
    status = _status(status, (1,), dev, who)
    src_pts, src_idx = (pts, idx) if N else (track_pts, point_track)
    work = _scratch(work, covis_workspace_bytes(N, V), dev)
    _native.check(_native.lib().apap_covis_tracks_device(
        _native._h(ctx), src_pts.data_ptr(), src_idx.data_ptr(), _ip(off), V, ctypes.c_float(float(e)), table.data_ptr(),
        track_pts.data_ptr(), point_track.data_ptr(), n_tracks.data_ptr(), status.data_ptr(), work.data_ptr(), work.numel(), _stream(dev)))
    return table[:N], track_pts[:N], point_track[:N], n_tracks


def hip_triangulate_rays(origins, dirs, ray_offset, ctx=None):
    """``apap_triangulate_rays_device`` on the current stream, no host synchronisation: origins, dirs (R, 3) float64 and
    ray_offset (T + 1,) int32 device tensors; a range of ray_offset that is reversed or leaves 0 .. R counts as empty.
    Returns (X (T, 3) float64, lam_min (T,) float64, n_rays (T,) int32).  Same bytes as ``_native.triangulate_rays``."""
    who = "hip_triangulate_rays"
    _needs_device(origins, who)
    dev = origins.device
    _contiguous(((origins, torch.float64), (dirs, torch.float64), (ray_offset, torch.int32)), dev, who)
    if origins.dim() != 2 or origins.shape[1] != 3 or dirs.shape != origins.shape or ray_offset.dim() != 1 or ray_offset.numel() < 1:
        raise ValueError(f"{who}: origins, dirs (R, 3) and ray_offset (T + 1,) expected")
    T, R = ray_offset.numel() - 1, origins.shape[0]
    X = torch.empty((T, 3), dtype=torch.float64, device=dev)
    lam = torch.empty(T, dtype=torch.float64, device=dev)
    n = torch.empty(T, dtype=torch.int32, device=dev)
    if T and R:
        _native.check(_native.lib().apap_triangulate_rays_device(_native._h(ctx), origins.data_ptr(), dirs.data_ptr(), ray_offset.data_ptr(),
                                                                 R, T, X.data_ptr(), lam.data_ptr(), n.data_ptr(), _stream(dev)))
    elif T:
        X.fill_(float("nan")), lam.fill_(float("nan")), n.zero_()
    return X, lam, n


def hip_triangulate_tracks(table, track_pts, n_tracks, dst_pts, dst_lengths, K_inv, Rs, origins, center_cam, view_cam, min_views=2, ctx=None):
    """``apap_triangulate_tracks_device`` on the current stream, no host synchronisation: what ``hip_covis_tracks`` returns
    (table (rows, V) int32, track_pts (rows, 2) float32, n_tracks (1,) int32 or None for every row) goes in as it is.  dst_pts
    (D, 2) float32: the views' other-picture points one after the other, view v of ``dst_lengths[v]`` (host list); K_inv (3, 3),
    Rs (C, 3, 3), origins (C, 3) float64 device tensors; ``center_cam`` and ``view_cam`` (host) name cameras.  Returns (X (rows,
    3), lam_min (rows,), n_rays (rows,) int32); rows behind n_tracks are not written.  Same bytes as
    ``_native.triangulate_tracks``."""
    who = "hip_triangulate_tracks"
    _needs_device(table, who)
    dev = table.device
    if table.dim() != 2:
        raise ValueError(f"{who}: table (rows, V) expected; got {tuple(table.shape)}")
    rows, V = table.shape
    off, cam = _native.triangulate_tables(V, list(dst_lengths), max(Rs.numel() // 9, 1), center_cam, view_cam, min_views, who)
    tensors = [(table, torch.int32), (track_pts, torch.float32), (dst_pts, torch.float32), (K_inv, torch.float64), (Rs, torch.float64),
               (origins, torch.float64)] + ([(n_tracks, torch.int32)] if n_tracks is not None else [])
    _contiguous(tensors, dev, who)
    cams = Rs.numel() // 9
    if track_pts.shape != (rows, 2) or dst_pts.shape != (int(off[-1]), 2) or K_inv.numel() != 9 or Rs.numel() != cams * 9 or cams < 1 \
            or origins.numel() != cams * 3 or (n_tracks is not None and n_tracks.numel() != 1):
        raise ValueError(f"{who}: track_pts ({rows}, 2), dst_pts ({int(off[-1])}, 2), K_inv (3, 3), Rs (C, 3, 3), origins (C, 3) expected")
    X = torch.empty((rows, 3), dtype=torch.float64, device=dev)
    lam = torch.empty(rows, dtype=torch.float64, device=dev)
    n = torch.empty(rows, dtype=torch.int32, device=dev)
    if rows:
        d_dst = dst_pts if dst_pts.numel() else track_pts       # (an empty tensor has no address; no index can point into it)
        _native.check(_native.lib().apap_triangulate_tracks_device(
            _native._h(ctx), table.data_ptr(), track_pts.data_ptr(), n_tracks.data_ptr() if n_tracks is not None else None, rows, V,
            d_dst.data_ptr(), _ip(off), K_inv.data_ptr(), Rs.data_ptr(), origins.data_ptr(), cams, int(center_cam), _ip(cam),
            int(min_views), X.data_ptr(), lam.data_ptr(), n.data_ptr(), _stream(dev)))
    return X, lam, n


def spectral_workspace_bytes(n):
    """Scratch of ``hip_spectral`` for ``n`` matches: O(n), no n x n buffer."""
    return _native.lib().apap_spectral_workspace_bytes(n)


def hip_spectral(src, dst, c_feats, o_feats, F, params, Hg=None, mask=None, status=None, ctx=None, work=None):
    """``apap_spectral_device`` on the current stream of the tensors' device: calculate_M's weights of resident data.
    src / dst (n, 2) float32, c_feats / o_feats (n, 128) float32, F (3, 3) float64, Hg (3, 3) float32 or ``mask`` (n,)
    float32 on the device; ``params``: host ``_native.spectral_params(...)``.  Returns (segment float64, ransac_mask
    float32, original_mask float32, info (6,) float64) as device tensors, not synchronised.  ``status`` (int32, 1
    element) receives STATUS_NO_CONVERGENCE when the restart cap is hit (also in info[3])."""
    _needs_device(src, "hip_spectral")
    dev, n = src.device, src.shape[0]
    _contiguous(((src, torch.float32), (dst, torch.float32), (c_feats, torch.float32), (o_feats, torch.float32), (F, torch.float64)),
                dev, "hip_spectral")
    if dst.shape != src.shape or c_feats.shape != (n, _native.SPECTRAL_DIM) or o_feats.shape != c_feats.shape or F.shape != (3, 3):
        raise ValueError("hip_spectral: shapes (n, 2), (n, 2), (n, 128), (n, 128), (3, 3) expected")
    params = np.ascontiguousarray(params, dtype=np.float64)
    seg = torch.empty(n, dtype=torch.float64, device=dev)
    rm = torch.empty(n, dtype=torch.float32, device=dev)
    om = torch.empty(n, dtype=torch.float32, device=dev)
    info = torch.empty(_native.SPECTRAL_INFO, dtype=torch.float64, device=dev)
    work = _scratch(work, spectral_workspace_bytes(n), dev)
    _native.check(_native.lib().apap_spectral_device(
        _native._h(ctx), src.data_ptr(), dst.data_ptr(), c_feats.data_ptr(), o_feats.data_ptr(), n, F.data_ptr(),
        _dp(params), None if Hg is None else Hg.data_ptr(),
        None if mask is None or Hg is not None else mask.data_ptr(), seg.data_ptr(), rm.data_ptr(), om.data_ptr(), info.data_ptr(),
        None if status is None else status.data_ptr(), work.data_ptr(), work.numel(), _stream(dev)))
    return seg, rm, om, info


def model_workspace_bytes(n):
    """Scratch of the M-step for ``n`` matches (``apap_model_workspace_bytes``)."""
    return _native.lib().apap_model_workspace_bytes(n)


def hip_model_solve(pts_c, pts_o, weights, params, status=None, ctx=None, work=None):
    """``apap_model_solve_device`` on the current stream of the tensors' device: one M-step (LMS, SDP or Huber) on resident
    data.  pts_c / pts_o (n, 2) float32, weights (n,) float32 on the device; ``params``: host ``_native.model_params(...)``.
    Returns (H (3, 3) float32, info (24,) float64) as device tensors, not synchronised: a degenerate or singular solve shows in
    info[MODEL_INFO_STATUS] and in ``status`` (int32, 1 element, OR-ed into), not as an exception."""
    _needs_device(pts_c, "hip_model_solve")
    dev, n = pts_c.device, pts_c.shape[0]
    _contiguous(((pts_c, torch.float32), (pts_o, torch.float32), (weights, torch.float32)), dev, "hip_model_solve")
    if pts_c.shape != (n, 2) or pts_o.shape != pts_c.shape or weights.shape != (n,):
        raise ValueError("hip_model_solve: shapes (n, 2), (n, 2), (n,) expected")
    mp = np.ascontiguousarray(params, dtype=np.float64)
    if mp.shape != (_native.MODEL_PARAMS,):
        raise ValueError(f"hip_model_solve: params must hold {_native.MODEL_PARAMS} values")
    H = torch.empty((3, 3), dtype=torch.float32, device=dev)
    info = torch.empty(_native.MODEL_INFO, dtype=torch.float64, device=dev)
    work = _scratch(work, model_workspace_bytes(n), dev)
    _native.check(_native.lib().apap_model_solve_device(
        _native._h(ctx), pts_c.data_ptr(), pts_o.data_ptr(), weights.data_ptr(), n, _dp(mp), H.data_ptr(), info.data_ptr(),
        None if status is None else status.data_ptr(), work.data_ptr(), work.numel(), _stream(dev)))
    return H, info


def hip_spectral_em(src, dst, c_feats, o_feats, F, spec_params, model_params, em_steps, mask, status=None, ctx=None, work=None):
    """``apap_spectral_em_device`` on the current stream of the tensors' device: ``em_steps`` rounds of calculate_M and the
    M-step on resident data, no host synchronisation: every spectral restart cycle is enqueued (those after convergence return
    at once but cost their launch), so this form is slower than the host-buffer ``spectral_method.spectral_em``, which stops
    at convergence; the results are the same.  Inputs as hip_spectral, ``mask`` (n,) float32 the first round's initial
    mask; ``spec_params`` / ``model_params``: host ``_native.spectral_params(...)`` / ``_native.model_params(...)``.  Returns
    (H (k, 3, 3) float32, model info (k, 24), segment (k, n) float64, ransac_mask (k, n), original_mask (k, n), spectral
    info (k, 6)) as device tensors, not synchronised.  ``status`` (int32, 1 element) collects every round's status bits."""
    _needs_device(src, "hip_spectral_em")
    dev, n, k = src.device, src.shape[0], int(em_steps)
    _contiguous(((src, torch.float32), (dst, torch.float32), (c_feats, torch.float32), (o_feats, torch.float32), (F, torch.float64),
                 (mask, torch.float32)), dev, "hip_spectral_em")
    if dst.shape != src.shape or c_feats.shape != (n, _native.SPECTRAL_DIM) or o_feats.shape != c_feats.shape or F.shape != (3, 3) \
            or mask.shape != (n,):
        raise ValueError("hip_spectral_em: shapes (n, 2), (n, 2), (n, 128), (n, 128), (3, 3), (n,) expected")
    sp = np.ascontiguousarray(spec_params, dtype=np.float64)
    mp = np.ascontiguousarray(model_params, dtype=np.float64)
    H = torch.empty((k, 3, 3), dtype=torch.float32, device=dev)
    info = torch.empty((k, _native.MODEL_INFO), dtype=torch.float64, device=dev)
    seg = torch.empty((k, n), dtype=torch.float64, device=dev)
    rm = torch.empty((k, n), dtype=torch.float32, device=dev)
    om = torch.empty((k, n), dtype=torch.float32, device=dev)
    sinfo = torch.empty((k, _native.SPECTRAL_INFO), dtype=torch.float64, device=dev)
    work = _scratch(work, spectral_workspace_bytes(n) + model_workspace_bytes(n), dev)
    _native.check(_native.lib().apap_spectral_em_device(
        _native._h(ctx), src.data_ptr(), dst.data_ptr(), c_feats.data_ptr(), o_feats.data_ptr(), n, F.data_ptr(),
        _dp(sp), _dp(mp), k, mask.data_ptr(), H.data_ptr(), info.data_ptr(), seg.data_ptr(),
        rm.data_ptr(), om.data_ptr(), sinfo.data_ptr(), None if status is None else status.data_ptr(), work.data_ptr(),
        work.numel(), _stream(dev)))
    return H, info, seg, rm, om, sinfo


def em_batch_workspace_bytes(pair_lengths, pair_of):
    """Scratch of ``hip_spectral_em_batch``: linear in the sum over the problems of their pair's matches."""
    off = np.zeros(len(pair_lengths) + 1, np.int32)
    off[1:] = np.cumsum(pair_lengths)
    po = np.ascontiguousarray(pair_of, dtype=np.int32)
    return _native.lib().apap_spectral_em_batch_workspace_bytes(_ip(off), len(off) - 1, _ip(po), len(po))


def hip_spectral_em_batch(src, dst, c_feats, o_feats, F, mask, pair_lengths, pair_of, spec_params, model_params, em_steps,
                          status=None, ctx=None, work=None):
    """``apap_spectral_em_batch_device`` on the current stream of the tensors' device: B EM problems in lockstep on resident
    data, no host synchronisation (every restart cycle is enqueued).  src / dst (N, 2), c_feats / o_feats (N, 128), mask (N,)
    float32: the pairs concatenated, pair p of ``pair_lengths[p]`` matches; F (P, 3, 3) float64; ``pair_of`` (B,), ``spec_params``
    (B, 6), ``model_params`` (B, 6): host arrays.  Returns (H (B, k, 3, 3) float32, model info (B, k, 24), segment, ransac_mask,
    original_mask: flat tensors, problem b's (k, n_b) block at k x (the matches of the problems before b), spectral info
    (B, k, 6), status (B,) int32) as device tensors, not synchronised.  ``status`` (int32, B elements, zeroed by the caller)
    is used when given; each word collects its own problem's bits.  Same bytes as ``_native.spectral_em_batch``."""
    _needs_device(src, "hip_spectral_em_batch")
    dev, k = src.device, int(em_steps)
    off, po, sp, mp = _native.em_batch_tables(pair_lengths, pair_of, spec_params, model_params)
    N, P, B = int(off[-1]), len(off) - 1, len(po)
    _contiguous(((src, torch.float32), (dst, torch.float32), (c_feats, torch.float32), (o_feats, torch.float32), (F, torch.float64),
                 (mask, torch.float32)), dev, "hip_spectral_em_batch")
    if src.shape != (N, 2) or dst.shape != src.shape or c_feats.shape != (N, _native.SPECTRAL_DIM) or o_feats.shape != c_feats.shape \
            or F.shape != (P, 3, 3) or mask.shape != (N,):
        raise ValueError(f"hip_spectral_em_batch: shapes ({N}, 2), ({N}, 2), ({N}, 128), ({N}, 128), ({P}, 3, 3), ({N},) expected")
    status = _status(status, (B,), dev, "hip_spectral_em_batch")
    M = int(sum(int(off[p + 1] - off[p]) for p in po))
    H = torch.empty((B, k, 3, 3), dtype=torch.float32, device=dev)
    info = torch.empty((B, k, _native.MODEL_INFO), dtype=torch.float64, device=dev)
    seg = torch.empty(k * M, dtype=torch.float64, device=dev)
    rm = torch.empty(k * M, dtype=torch.float32, device=dev)
    om = torch.empty(k * M, dtype=torch.float32, device=dev)
    sinfo = torch.empty((B, k, _native.SPECTRAL_INFO), dtype=torch.float64, device=dev)
    work = _scratch(work, em_batch_workspace_bytes([int(off[p + 1] - off[p]) for p in range(P)], po), dev)
    _native.check(_native.lib().apap_spectral_em_batch_device(
        _native._h(ctx), src.data_ptr(), dst.data_ptr(), c_feats.data_ptr(), o_feats.data_ptr(), F.data_ptr(), mask.data_ptr(),
        _ip(off), P, _ip(po), _dp(sp), _dp(mp), B, k, H.data_ptr(),
        info.data_ptr(), seg.data_ptr(), rm.data_ptr(), om.data_ptr(), sinfo.data_ptr(), status.data_ptr(), work.data_ptr(),
        work.numel(), _stream(dev)))
    return H, info, seg, rm, om, sinfo, status


def local_model_workspace_bytes(n, cells):
    """Scratch of ``hip_local_model_solve``: that of ``min(cells, _native.LOCAL_MODEL_CHUNK)`` cells of ``n`` matches."""
    return _native.lib().apap_local_model_workspace_bytes(n, cells)


def hip_local_model_solve(pts_c, pts_o, vertices, gamma, sigma, params, match_weights=None, status=None, ctx=None, work=None):
    """``apap_local_model_solve_device`` on the current stream of the tensors' device: the robust moving DLT on resident
    data.  pts_c / pts_o (n, 2) float32, vertices (..., 2) float64, match_weights (n,) float32 or None: contiguous device
    tensors; ``params`` (6,): a host array (``_native.model_params``).  Returns (H (..., 3, 3) float32, info (..., 24) float64,
    status (...,) int32) as device tensors, not synchronised.  ``status`` (int32, one element per cell, zeroed by the
    caller) is used when given; each word collects its own cell's bits.  ``work`` (uint8) is used AS GIVEN: the cells are
    processed in chunks of as many as it holds (at least one cell's scratch, ``local_model_workspace_bytes(n, 1)``); default
    ``local_model_workspace_bytes(n, cells)``.  Same bytes as ``_native.local_model_solve`` whatever the chunking."""
    _needs_device(pts_c, "hip_local_model_solve")
    dev = pts_c.device
    params = np.ascontiguousarray(params, dtype=np.float64)
    if params.shape != (_native.MODEL_PARAMS,):
        raise ValueError(f"hip_local_model_solve: params must hold {_native.MODEL_PARAMS} values")
    tensors = [(pts_c, torch.float32), (pts_o, torch.float32), (vertices, torch.float64)]
    if match_weights is not None:
        tensors.append((match_weights, torch.float32))
    _contiguous(tensors, dev, "hip_local_model_solve")
    n = pts_c.shape[0]
    if pts_c.shape != (n, 2) or pts_o.shape != pts_c.shape or vertices.dim() < 1 or vertices.shape[-1] != 2 \
            or (match_weights is not None and match_weights.shape != (n,)):
        raise ValueError(f"hip_local_model_solve: shapes ({n}, 2), ({n}, 2), (..., 2) and ({n},) expected")
    lead = tuple(vertices.shape[:-1])
    cells = vertices.numel() // 2
    status = _status(status, lead, dev, "hip_local_model_solve", flat=True)
    H = torch.empty(lead + (3, 3), dtype=torch.float32, device=dev)
    info = torch.empty(lead + (_native.MODEL_INFO,), dtype=torch.float64, device=dev)
    if cells == 0:
        return H, info, status
    if work is None:
        work = torch.empty(local_model_workspace_bytes(n, cells), dtype=torch.uint8, device=dev)
    _native.check(_native.lib().apap_local_model_solve_device(
        _native._h(ctx), pts_c.data_ptr(), pts_o.data_ptr(), None if match_weights is None else match_weights.data_ptr(), n,
        vertices.data_ptr(), cells, float(gamma), float(sigma), _dp(params), H.data_ptr(),
        info.data_ptr(), status.data_ptr(), work.data_ptr(), work.numel(), _stream(dev)))
    return H, info, status


def _match_workspace(single, batch, q_lengths, t_lengths):
    """A matcher's scratch from its two library functions: of one (nq, nt) pair, or of the pairs' row counts."""
    if np.ndim(q_lengths) == 0:
        return single(int(q_lengths), int(t_lengths))
    qo, to = _native.match_offsets(q_lengths, "q_lengths"), _native.match_offsets(t_lengths, "t_lengths")
    return batch(_ip(qo), _ip(to), min(len(qo), len(to)) - 1)


def _match_batch_args(q, t, q_lengths, t_lengths, who):
    """``_native._match_batch_args`` for device tensors: the checks of a batch call of either matcher -> (query offsets, train
    offsets)."""
    dev = q.device
    for x in (q, t):
        if x.dtype != torch.float32 or not x.is_contiguous() or x.device != dev or x.dim() != 2 or x.shape[1] != _native.MATCH_DIM:
            raise ValueError(f"{who}: descriptors must be contiguous float32 (n, {_native.MATCH_DIM}) tensors on {dev}")
    if len(q_lengths) != len(t_lengths):
        raise ValueError(f"{who}: {len(q_lengths)} query counts, {len(t_lengths)} train counts")
    qo, to = _native.match_offsets(q_lengths, "q_lengths"), _native.match_offsets(t_lengths, "t_lengths")
    if qo[-1] != q.shape[0] or to[-1] != t.shape[0]:
        raise ValueError(f"{who}: the counts sum to {qo[-1]} and {to[-1]} rows; got {q.shape[0]} and {t.shape[0]}")
    return qo, to


def _match_out(dev):
    """The allocator of a matcher's outputs on ``dev``: ``out(n, dtype, wanted)``, None for what was not asked for."""
    return lambda n, dtype, wanted=True: torch.empty(n, dtype=dtype, device=dev) if wanted else None


def _ptr(x):
    return None if x is None else x.data_ptr()


def match_workspace_bytes(q_lengths, t_lengths=None):
    """Scratch of ``hip_match_descriptors(q, t)`` as ``match_workspace_bytes(nq, nt)``, or of ``hip_match_descriptors_batch``
    as ``match_workspace_bytes(q_lengths, t_lengths)`` with the pairs' row counts: 16 bytes per query and split of its pair's
    train axis.  0 for invalid arguments."""
    return _match_workspace(_native.lib().apap_match_workspace_bytes, _native.lib().apap_match_batch_workspace_bytes, q_lengths, t_lengths)


def hip_match_descriptors_batch(q, t, q_lengths, t_lengths, second=True, ctx=None, work=None):
    """``apap_match_descriptors_batch_device`` on the current stream of the tensors' device, no host synchronisation: many
    pairs in two kernel launches.  q / t: contiguous float32 (N, 128) device tensors, the pairs concatenated, pair p of
    ``q_lengths[p]`` queries and ``t_lengths[p]`` train rows (host lists).  Returns (idx int32, dist float32, idx2, dist2) laid
    out like ``q`` (the last two ``None`` without ``second``), not synchronised; a pair's indices count from its own first
    train row.  ``work`` (uint8) is used when it holds ``match_workspace_bytes(q_lengths, t_lengths)``.  Same bytes as
    ``_native.match_descriptors_batch``, and per pair as ``hip_match_descriptors``.  What follows - gathering keypoints and
    descriptors by ``idx`` into ``hip_spectral_em``'s inputs - is plain tensor indexing and stays with the caller."""
    _needs_device(q, "hip_match_descriptors_batch")
    dev = q.device
    qo, to = _match_batch_args(q, t, q_lengths, t_lengths, "hip_match_descriptors_batch")
    n, out = q.shape[0], _match_out(dev)
    idx, dist, idx2, dist2 = out(n, torch.int32), out(n, torch.float32), out(n, torch.int32, second), out(n, torch.float32, second)
    p_qo, p_to = _ip(qo), _ip(to)
    work = _scratch(work, _native.lib().apap_match_batch_workspace_bytes(p_qo, p_to, len(qo) - 1), dev)
    _native.check(_native.lib().apap_match_descriptors_batch_device(
        _native._h(ctx), q.data_ptr(), t.data_ptr(), p_qo, p_to, len(qo) - 1, idx.data_ptr(), dist.data_ptr(), _ptr(idx2), _ptr(dist2),
        work.data_ptr(), work.numel(), _stream(dev)))
    return idx, dist, idx2, dist2


def hip_match_descriptors(q, t, second=True, ctx=None, work=None):
    """``apap_match_descriptors_device``: the nearest and (with ``second``) second-nearest row of ``t`` (nt, 128) for every
    row of ``q`` (nq, 128), exact L2; the batch of one pair (see ``hip_match_descriptors_batch``)."""
    _needs_device(q, "hip_match_descriptors")
    return hip_match_descriptors_batch(q, t, [q.shape[0]], [t.shape[0]], second=second, ctx=ctx, work=work)


def hip_guided_records(pts, model=None, what="point", ctx=None):
    """``apap_guided_records_device`` on the current stream, no host synchronisation: the (n, 3) float64 records of ``pts``
    (n, 2) float32, a contiguous device tensor.  ``model``: a 3 x 3 (or 9-element) tensor on the same device - a device ``H`` of
    ``find_homography`` or ``hip_spectral_em`` (float32 is widened on the device, exactly), a device ``F`` of
    ``hip_fundamental`` - or ``None`` with ``what='point'``."""
    _needs_device(pts, "hip_guided_records")
    what = _native.guided_what(what)
    dev = pts.device
    if pts.dtype != torch.float32 or not pts.is_contiguous() or pts.dim() != 2 or pts.shape[1] != 2:
        raise ValueError("hip_guided_records: pts must be a contiguous float32 (n, 2) tensor")
    if model is None:
        if what != _native.GUIDED_REC_POINT:
            raise ValueError("hip_guided_records: a model is needed unless what='point'")
    else:
        if model.device != dev or model.numel() != 9:
            raise ValueError(f"hip_guided_records: the model must hold 9 values on {dev}")
        model = model.to(torch.float64).contiguous()
    rec = torch.empty((pts.shape[0], 3), dtype=torch.float64, device=dev)
    _native.check(_native.lib().apap_guided_records_device(
        _native._h(ctx), pts.data_ptr(), pts.shape[0], None if model is None else model.data_ptr(), what, rec.data_ptr(), _stream(dev)))
    return rec


def guided_workspace_bytes(q_lengths, t_lengths=None):
    """Scratch of ``hip_guided_match(…)`` as ``guided_workspace_bytes(nq, nt)``, or of ``hip_guided_match_batch`` with the
    pairs' row counts.  0 for invalid arguments."""
    return _match_workspace(_native.lib().apap_match_guided_workspace_bytes, _native.lib().apap_match_guided_batch_workspace_bytes,
                            q_lengths, t_lengths)


def hip_guided_match_batch(q, t, rec_q, rec_t, q_lengths, t_lengths, kind, r2, second=True, count=True, reverse=False, ctx=None,
                           work=None):
    """``apap_match_guided_batch_device`` on the current stream of the tensors' device, no host synchronisation.  q / t:
    contiguous float32 (N, 128) device tensors, rec_q / rec_t: contiguous float64 (N, 3) records (``hip_guided_records``), the
    pairs concatenated; ``q_lengths``, ``t_lengths`` and the squared radius ``r2`` (a number, or one per pair) stay on the host.  Returns (idx,
    dist, idx2, dist2, count, ridx, rdist), not synchronised: the first five laid out like ``q``, the last two like ``t``,
    ``None`` for what was not asked for.  Same bytes as ``_native.match_guided_batch``, and per pair as ``hip_guided_match``."""
    _needs_device(q, "hip_guided_match_batch")
    dev = q.device
    kind = _native.guided_kind(kind)
    qo, to = _match_batch_args(q, t, q_lengths, t_lengths, "hip_guided_match_batch")
    for x, d in ((rec_q, q), (rec_t, t)):
        if x.dtype != torch.float64 or not x.is_contiguous() or x.device != dev or tuple(x.shape) != (d.shape[0], 3):
            raise ValueError(f"hip_guided_match_batch: records must be contiguous float64 ({d.shape[0]}, 3) tensors on {dev}")
    r2 = _native.guided_r2(r2, len(qo) - 1)
    nq, nt, out = q.shape[0], t.shape[0], _match_out(dev)
    idx, dist = out(nq, torch.int32), out(nq, torch.float32)
    idx2, dist2, cnt = out(nq, torch.int32, second), out(nq, torch.float32, second), out(nq, torch.int32, count)
    ridx, rdist = out(nt, torch.int32, reverse), out(nt, torch.float32, reverse)
    p_qo, p_to = _ip(qo), _ip(to)
    work = _scratch(work, _native.lib().apap_match_guided_batch_workspace_bytes(p_qo, p_to, len(qo) - 1), dev)
    _native.check(_native.lib().apap_match_guided_batch_device(
        _native._h(ctx), rec_q.data_ptr(), rec_t.data_ptr(), q.data_ptr(), t.data_ptr(), p_qo, p_to, len(qo) - 1, kind,
        _dp(r2), idx.data_ptr(), dist.data_ptr(), _ptr(idx2), _ptr(dist2), _ptr(cnt), _ptr(ridx), _ptr(rdist),
        work.data_ptr(), work.numel(), _stream(dev)))
    return idx, dist, idx2, dist2, cnt, ridx, rdist


def hip_guided_match(q, t, rec_q, rec_t, kind, r2, second=True, count=True, reverse=False, ctx=None, work=None):
    """``apap_match_guided_device``: one pair, the batch of one (see ``hip_guided_match_batch``)."""
    _needs_device(q, "hip_guided_match")
    return hip_guided_match_batch(q, t, rec_q, rec_t, [q.shape[0]], [t.shape[0]], kind, r2, second=second, count=count,
                                  reverse=reverse, ctx=ctx, work=work)


def _image_table(imgs, dev, who):
    """The checks of a list of uint8 images on ``dev``, (h, w) grey or (h, w, 3) BGR - what ``_native.as_sift_image`` asks of a
    host array, with its side limits - and the batch entry points' (addresses, heights, widths, channels)."""
    for m, im in enumerate(imgs):
        if im.dtype != torch.uint8 or not im.is_contiguous() or im.device != dev or im.dim() not in (2, 3) or \
                (im.dim() == 3 and im.shape[2] not in (1, 3)):
            raise ValueError(f"{who}: imgs[{m}] must be a contiguous uint8 (h, w) or (h, w, 3) tensor on {dev}")
        if not all(_native.SIFT_MIN_SIDE <= x <= _native.SIFT_MAX_SIDE for x in im.shape[:2]):
            raise ValueError(f"{who}: imgs[{m}]: sides must be {_native.SIFT_MIN_SIDE} .. {_native.SIFT_MAX_SIDE}; got {tuple(im.shape[:2])}")
    return (_addrs([im.data_ptr() for im in imgs]), _i32([im.shape[0] for im in imgs]), _i32([im.shape[1] for im in imgs]),
            _i32([1 if im.dim() == 2 else im.shape[2] for im in imgs]))


def sift_workspace_bytes(n_images=1):
    """Scratch of ``hip_sift_describe`` / ``hip_sift_describe_batch`` of ``n_images`` images: 32 bytes per image, a 256-byte
    multiple.  0 for an invalid count."""
    return _native.lib().apap_sift_workspace_bytes(int(n_images))


def hip_sift_describe_batch(imgs, pts, lengths, ctx=None, work=None):
    """``apap_sift_describe_batch_device`` on the current stream of the tensors' device, no host synchronisation: the SIFT
    descriptors of ``KeyPoint(x, y, 1)`` at given coordinates, many images in one kernel launch.  ``imgs``: a sequence of
    contiguous uint8 device tensors, (h, w) grey or (h, w, 3) BGR, of any shapes; ``pts``: contiguous float32 (N, 2) device
    tensor, the images' keypoints (x, y) concatenated, image m of ``lengths[m]`` (a host list).  Returns float32 (N, 128), not
    synchronised: what ``hip_match_descriptors`` takes.  A keypoint with no valid sample or a non-finite coordinate gives
    zeros.  ``work`` (uint8) is used when it holds ``sift_workspace_bytes(len(imgs))``.  Same bytes as
    ``_native.sift_describe_batch``, and per image as ``hip_sift_describe``."""
    who = "hip_sift_describe_batch"
    _needs_device(pts, who)
    dev = pts.device
    if pts.dtype != torch.float32 or not pts.is_contiguous() or pts.dim() != 2 or pts.shape[1] != 2:
        raise ValueError(f"{who}: keypoints must be a contiguous float32 (n, 2) tensor")
    imgs = list(imgs)
    if len(imgs) != len(lengths):
        raise ValueError(f"{who}: {len(imgs)} images, {len(lengths)} keypoint counts")
    ptrs, hs, ws, cs = _image_table(imgs, dev, who)
    off = _native.sift_offsets(lengths)
    if off[-1] != pts.shape[0]:
        raise ValueError(f"{who}: the counts sum to {off[-1]} keypoints; got {pts.shape[0]}")
    out = torch.empty((pts.shape[0], _native.SIFT_DIM), dtype=torch.float32, device=dev)
    work = _scratch(work, sift_workspace_bytes(len(imgs)), dev)
    _native.check(_native.lib().apap_sift_describe_batch_device(
        _native._h(ctx), ptrs, _ip(hs), _ip(ws), _ip(cs), len(imgs), pts.data_ptr(), _ip(off), out.data_ptr(), work.data_ptr(), work.numel(),
        _stream(dev)))
    return out


def hip_sift_describe(img, pts, ctx=None, work=None):
    """``apap_sift_describe_device``: float32 (n, 128) SIFT descriptors at ``pts`` (n, 2) of one uint8 device image; the batch
    of one image (see ``hip_sift_describe_batch``)."""
    _needs_device(pts, "hip_sift_describe")
    return hip_sift_describe_batch([img], pts, [pts.shape[0]], ctx=ctx, work=work)


def sift_orient_workspace_bytes(n_images=1):
    """Scratch of the ``hip_sift_orient*`` and ``hip_sift_describe_oriented*`` calls of ``n_images`` images: 32 bytes per image,
    a 256-byte multiple.  0 for an invalid count."""
    return _native.lib().apap_sift_orient_workspace_bytes(int(n_images))


def _oriented_args(imgs, pts, lengths, who):
    _needs_device(pts, who)
    dev = pts.device
    if pts.dtype != torch.float32 or not pts.is_contiguous() or pts.dim() != 2 or pts.shape[1] != 2:
        raise ValueError(f"{who}: keypoints must be a contiguous float32 (n, 2) tensor")
    imgs = list(imgs)
    if len(imgs) != len(lengths):
        raise ValueError(f"{who}: {len(imgs)} images, {len(lengths)} keypoint counts")
    table = _image_table(imgs, dev, who)
    for m, im in enumerate(imgs):
        if min(im.shape[:2]) < _native.SIFT_ORIENT_MIN_SIDE:
            raise ValueError(f"{who}: imgs[{m}]: sides must be {_native.SIFT_ORIENT_MIN_SIDE} .. {_native.SIFT_MAX_SIDE}; got {tuple(im.shape[:2])}")
    off = _native.sift_offsets(lengths)
    if off[-1] != pts.shape[0]:
        raise ValueError(f"{who}: the counts sum to {off[-1]} keypoints; got {pts.shape[0]}")
    return dev, len(imgs), table, off


def hip_sift_orient_batch(imgs, pts, lengths, ctx=None, work=None):
    """``apap_sift_orient_batch_device`` on the current stream, no host synchronisation: the dominant orientation of every
    keypoint, many images in one kernel launch.  Arguments as ``hip_sift_describe_batch`` (sides from 13).  Returns float32 (N,)
    angles in [0, 360); a keypoint with no valid sample or a non-finite coordinate has angle 0."""
    dev, n, (ptrs, hs, ws, cs), off = _oriented_args(imgs, pts, lengths, "hip_sift_orient_batch")
    angles = torch.empty(pts.shape[0], dtype=torch.float32, device=dev)
    work = _scratch(work, sift_orient_workspace_bytes(n), dev)
    _native.check(_native.lib().apap_sift_orient_batch_device(
        _native._h(ctx), ptrs, _ip(hs), _ip(ws), _ip(cs), n, pts.data_ptr(), _ip(off), angles.data_ptr(), work.data_ptr(), work.numel(),
        _stream(dev)))
    return angles


def hip_sift_orient(img, pts, ctx=None, work=None):
    """``apap_sift_orient_device``: one image, the batch of one (see ``hip_sift_orient_batch``)."""
    _needs_device(pts, "hip_sift_orient")
    return hip_sift_orient_batch([img], pts, [pts.shape[0]], ctx=ctx, work=work)


def hip_sift_describe_oriented_batch(imgs, pts, lengths, angles=None, ctx=None, work=None):
    """``apap_sift_describe_oriented_batch_device`` on the current stream, no host synchronisation.  ``angles``: a contiguous
    float32 (N,) device tensor of ``cv.KeyPoint.angle`` values - returns the float32 (N, 128) descriptors at them (a zero row
    for an angle outside [0, 360]).  ``angles=None``: orientation and descriptor in one launch - returns ``(feats, angles)``,
    the same bytes as ``hip_sift_orient_batch`` followed by the call with its angles."""
    who = "hip_sift_describe_oriented_batch"
    dev, n, (ptrs, hs, ws, cs), off = _oriented_args(imgs, pts, lengths, who)
    if angles is not None and (angles.dtype != torch.float32 or not angles.is_contiguous() or angles.device != dev or
                               tuple(angles.shape) != (pts.shape[0],)):
        raise ValueError(f"{who}: angles must be a contiguous float32 ({pts.shape[0]},) tensor on {dev}")
    out = torch.empty((pts.shape[0], _native.SIFT_DIM), dtype=torch.float32, device=dev)
    found = torch.empty(pts.shape[0], dtype=torch.float32, device=dev) if angles is None else None
    work = _scratch(work, sift_orient_workspace_bytes(n), dev)
    _native.check(_native.lib().apap_sift_describe_oriented_batch_device(
        _native._h(ctx), ptrs, _ip(hs), _ip(ws), _ip(cs), n, pts.data_ptr(), _ip(off), None if angles is None else angles.data_ptr(),
        None if found is None else found.data_ptr(), out.data_ptr(), work.data_ptr(), work.numel(), _stream(dev)))
    return out if angles is not None else (out, found)


def hip_sift_describe_oriented(img, pts, angles=None, ctx=None, work=None):
    """``apap_sift_describe_oriented_device``: one image, the batch of one (see ``hip_sift_describe_oriented_batch``)."""
    _needs_device(pts, "hip_sift_describe_oriented")
    return hip_sift_describe_oriented_batch([img], pts, [pts.shape[0]], angles=angles, ctx=ctx, work=work)


def hip_describe_and_match(c_img, o_img, pts_c, pts_o, second=True, ctx=None, oriented=False):
    """Both images described in one batched launch, then ``hip_match_descriptors`` of the centre image's descriptors against
    the other's: three kernels on the current stream, nothing returns to the host in between.  Returns (idx, dist, idx2, dist2,
    feats_c, feats_o): the matcher's four outputs (``idx2`` and ``dist2`` ``None`` without ``second``) and the float32 (n, 128)
    descriptors, views of one tensor.  ``oriented``: every keypoint described in its own dominant orientation (the fused
    ``hip_sift_describe_oriented_batch``), so that the match survives an in-plane rotation between the images."""
    _needs_device(pts_c, "hip_describe_and_match")
    nc, no = pts_c.shape[0], pts_o.shape[0]
    if oriented:
        feats, _ = hip_sift_describe_oriented_batch([c_img, o_img], torch.cat([pts_c, pts_o]), [nc, no], ctx=ctx)
    else:
        feats = hip_sift_describe_batch([c_img, o_img], torch.cat([pts_c, pts_o]), [nc, no], ctx=ctx)
    return hip_match_descriptors(feats[:nc], feats[nc:], second=second, ctx=ctx) + (feats[:nc], feats[nc:])


def corner_workspace_bytes(shapes, radius=5):
    """Scratch of ``hip_corner_detect`` / ``hip_corner_detect_batch`` for images of ``shapes`` (a sequence of (h, w, ...)):
    per image 64 bytes and twice 16 bytes per possible corner (the second time rounded up to a power of two); a 256-byte
    multiple.  0 for invalid arguments."""
    hs, ws = _i32([s[0] for s in shapes]), _i32([s[1] for s in shapes])
    return _native.lib().apap_corner_workspace_bytes(_ip(hs), _ip(ws), len(hs), int(radius))


def hip_corner_detect_batch(imgs, max_corners, radius=5, quality_permille=10, ctx=None, work=None):
    """``apap_corner_detect_batch_device`` on the current stream of the tensors' device, no host synchronisation: the exact
    integer Harris corners of many images in two kernel launches.  ``imgs``: a sequence of contiguous uint8 device tensors,
    (h, w) grey or (h, w, 3) BGR, of any shapes.  Returns ``(pts, response, count)``, not synchronised: float32
    (n_images, max_corners, 2) integer-valued (x, y), int64 (n_images, max_corners) and int32 (n_images,); rows from an image's
    count on are zero.  ``work`` (uint8) is used when it holds ``corner_workspace_bytes(shapes, radius)``.  Same bytes as
    ``_native.corner_detect_batch``, and per image as ``hip_corner_detect``."""
    who = "hip_corner_detect_batch"
    imgs = list(imgs)
    if not imgs:
        raise ValueError(f"{who}: no image")
    _needs_device(imgs[0], who)
    dev = imgs[0].device
    ptrs, hs, ws, cs = _image_table(imgs, dev, who)
    max_corners, radius, quality_permille = _native.corner_params(max_corners, radius, quality_permille, who)
    pts = torch.empty((len(imgs), max_corners, 2), dtype=torch.float32, device=dev)
    resp = torch.empty((len(imgs), max_corners), dtype=torch.int64, device=dev)
    count = torch.empty(len(imgs), dtype=torch.int32, device=dev)
    p_hs, p_ws = _ip(hs), _ip(ws)
    work = _scratch(work, _native.lib().apap_corner_workspace_bytes(p_hs, p_ws, len(imgs), radius), dev)
    _native.check(_native.lib().apap_corner_detect_batch_device(
        _native._h(ctx), ptrs, p_hs, p_ws, _ip(cs), len(imgs), max_corners, radius,
        quality_permille, pts.data_ptr(), resp.data_ptr(), count.data_ptr(), work.data_ptr(), work.numel(), _stream(dev)))
    return pts, resp, count


def hip_corner_detect(img, max_corners, radius=5, quality_permille=10, ctx=None, work=None):
    """``apap_corner_detect_device``: ``(pts (max_corners, 2), response (max_corners,), count ())`` of one uint8 device image;
    the batch of one image (see ``hip_corner_detect_batch``)."""
    pts, resp, count = hip_corner_detect_batch([img], max_corners, radius, quality_permille, ctx=ctx, work=work)
    return pts[0], resp[0], count[0]


def hip_detect_describe_match(c_img, o_img, max_corners, radius=5, quality_permille=10, second=True, ctx=None, oriented=False):
    """From two uint8 device images to matches: both images' corners in one batched call, their descriptors in one batched
    call, then ``hip_match_descriptors`` of the centre image's descriptors against the other's.  Between detection and
    description the two corner counts (8 bytes) are read back: the chain's only host synchronisation, needed because the
    describe and match entry points take their lengths on the host.  Returns (idx, dist, idx2, dist2, feats_c, feats_o, pts_c,
    pts_o): ``hip_describe_and_match``'s six outputs and the float32 (n, 2) corners.  An image without corners is refused
    (``ValueError``): there is nothing to describe or match.  ``oriented``: as ``hip_describe_and_match``."""
    pts, _, count = hip_corner_detect_batch([c_img, o_img], max_corners, radius, quality_permille, ctx=ctx)
    nc, no = (int(x) for x in count.tolist())
    if nc < 1 or no < 1:
        raise ValueError(f"hip_detect_describe_match: {nc} and {no} corners; both images need at least one")
    pts_c, pts_o = pts[0, :nc], pts[1, :no]
    return hip_describe_and_match(c_img, o_img, pts_c, pts_o, second=second, ctx=ctx, oriented=oriented) + (pts_c, pts_o)


def pyramid_workspace_bytes(n_images=1, levels=6):
    """Scratch of ``hip_pyramid`` / ``hip_pyramid_batch``: 64 bytes per picture and level, a 256-byte multiple.  0 for invalid
    arguments."""
    return _native.lib().apap_pyramid_workspace_bytes(int(n_images), int(levels))


def hip_pyramid_batch(imgs, levels=6, half_steps=True, ctx=None, work=None):
    """``apap_pyramid_build_batch_device`` on the current stream of the tensors' device, no host synchronisation: the grey
    pyramids of many uint8 device pictures, (h, w) grey or (h, w, 3) BGR of any shapes from 32 a side, in
    1 + ceil((levels - 1) / 2) kernel launches at most.  Returns a list per picture of its levels, uint8 (h_l, w_l) views of
    one buffer (every level on a 256-byte boundary), not synchronised: what ``hip_corner_detect_batch`` and
    ``hip_sift_describe_batch`` take as images.  Same bytes as ``_native.pyramid_batch``, and per picture as ``hip_pyramid``."""
    who = "hip_pyramid_batch"
    levels = _native.pyramid_levels_arg(levels, who)
    imgs = list(imgs)
    if not imgs:
        raise ValueError(f"{who}: no image")
    _needs_device(imgs[0], who)
    dev = imgs[0].device
    ptrs, hs, ws, cs = _image_table(imgs, dev, who)
    for m, im in enumerate(imgs):
        if min(im.shape[:2]) < _native.PYRAMID_MIN_SIDE:
            raise ValueError(f"{who}: imgs[{m}]: sides must be {_native.PYRAMID_MIN_SIDE} .. {_native.SIFT_MAX_SIDE}; got {tuple(im.shape[:2])}")
    lays = [_native.pyramid_layout(im.shape[0], im.shape[1], levels, half_steps) for im in imgs]
    buf = torch.empty(sum(int(lay[2][-1]) for lay in lays), dtype=torch.uint8, device=dev)
    work = _scratch(work, pyramid_workspace_bytes(len(imgs), levels), dev)
    _native.check(_native.lib().apap_pyramid_build_batch_device(
        _native._h(ctx), ptrs, _ip(hs), _ip(ws), _ip(cs), len(imgs), levels, int(bool(half_steps)), buf.data_ptr(), buf.numel(),
        work.data_ptr(), work.numel(), _stream(dev)))
    out, at = [], 0
    for lh, lw, off, _, _ in lays:
        out.append([buf[at + int(off[k]):at + int(off[k]) + int(lh[k]) * int(lw[k])].view(int(lh[k]), int(lw[k])) for k in range(len(lh))])
        at += int(off[-1])
    return out


def hip_pyramid(img, levels=6, half_steps=True, work=None, ctx=None):
    """``apap_pyramid_build_device``: the list of grey levels of one uint8 device picture; the batch of one (see
    ``hip_pyramid_batch``)."""
    return hip_pyramid_batch([img], levels, half_steps, ctx=ctx, work=work)[0]


def hip_pyramid_keypoints(slab_pts, slab_response, counts, scale_num, scale_shift, level_index, ctx=None, work=None):
    """``apap_pyramid_keypoints_device`` on the current stream, no host synchronisation: the pack.  ``slab_pts`` (n, rows, 2)
    float32 and ``slab_response`` (n, rows) int64: ``hip_corner_detect_batch``'s slabs over n level images; ``counts``,
    ``scale_num``, ``scale_shift``, ``level_index``: HOST sequences of n ints (the rows to keep of each level image, its scale
    and its level number).  Returns ``(pts, level_pts, level, response, level_offset)``: float32 (N, 2) base-frame
    coordinates, float32 (N, 2) level coordinates, int32 (N,), int64 (N,) device tensors and a host int32 (n + 1,) array."""
    who = "hip_pyramid_keypoints"
    _needs_device(slab_pts, who)
    dev = slab_pts.device
    _contiguous([(slab_pts, torch.float32), (slab_response, torch.int64)], dev, who)
    if slab_pts.dim() != 3 or slab_pts.shape[2] != 2 or tuple(slab_response.shape) != tuple(slab_pts.shape[:2]) or slab_pts.shape[1] < 1:
        raise ValueError(f"{who}: slabs must be (n, rows, 2) and (n, rows); got {tuple(slab_pts.shape)} and {tuple(slab_response.shape)}")
    n, rows = slab_pts.shape[:2]
    counts, num, shift, index = (_i32(np.asarray(a).reshape(-1)) for a in (counts, scale_num, scale_shift, level_index))
    if not 1 <= n <= _native.CORNER_MAX_IMAGES or any(len(a) != n for a in (counts, num, shift, index)):
        raise ValueError(f"{who}: {n} level images (1 .. {_native.CORNER_MAX_IMAGES}) need as many counts, scales and indices")
    if counts.min() < 0 or counts.max() > rows:
        raise ValueError(f"{who}: counts must be 0 .. {rows}; got {counts.tolist()}")
    N = int(counts.sum())
    pts, lpts = (torch.empty((N, 2), dtype=torch.float32, device=dev) for _ in range(2))
    level = torch.empty(N, dtype=torch.int32, device=dev)
    resp = torch.empty(N, dtype=torch.int64, device=dev)
    off = np.empty(n + 1, np.int32)
    work = _scratch(work, _native.lib().apap_pyramid_keypoints_workspace_bytes(n), dev)
    # an empty tensor has no address: the library asks for one, and follows none when N = 0
    ptr = lambda t: t.data_ptr() if N else work.data_ptr()      # noqa: E731
    _native.check(_native.lib().apap_pyramid_keypoints_device(
        _native._h(ctx), slab_pts.data_ptr(), slab_response.data_ptr(), rows, _ip(counts), _ip(num), _ip(shift), _ip(index), n, ptr(pts),
        ptr(lpts), ptr(level), ptr(resp), _ip(off), work.data_ptr(), work.numel(), _stream(dev)))
    return pts, lpts, level, resp, off


def hip_pyramid_detect_describe(imgs, max_corners, levels=6, half_steps=True, radius=5, quality_permille=10, ctx=None, oriented=False):
    """Per picture ``(pts, feats, level, response)`` over its pyramid, all pictures together: the pyramids in one batched call,
    one batched detection over all level images, the level counts (4 bytes each) read back - the chain's only host
    synchronisation - the pack, and one batched description with the level images as the images.  Device tensors: float32
    (n, 2) base-frame keypoints, float32 (n, 128) descriptors, int32 (n,) levels, int64 (n,) responses."""
    who = "hip_pyramid_detect_describe"
    levels = _native.pyramid_levels_arg(levels, who)
    max_corners, radius, quality_permille = _native.corner_params(max_corners, radius, quality_permille, who)
    pyrs = hip_pyramid_batch(imgs, levels, half_steps, ctx=ctx)
    flat = [a for lv in pyrs for a in lv]
    slab_pts, slab_resp, count = hip_corner_detect_batch(flat, max_corners, radius, quality_permille, ctx=ctx)
    caps = _native.pyramid_level_caps(max_corners, levels, half_steps)
    num, shift, index = [], [], []
    for lv in pyrs:
        _, _, _, n, s = _native.pyramid_layout(lv[0].shape[0], lv[0].shape[1], levels, half_steps)
        num += n.tolist()
        shift += s.tolist()
        index += range(len(lv))
    keep = np.minimum(count.cpu().numpy(), caps[index])
    pts, lpts, level, resp, off = hip_pyramid_keypoints(slab_pts, slab_resp, keep, num, shift, index, ctx=ctx)
    full = [(a, int(k)) for a, k in zip(flat, keep) if k > 0]      # the batch takes no image without a keypoint
    if not full:
        feats = torch.zeros((0, _native.SIFT_DIM), dtype=torch.float32, device=pts.device)
    elif oriented:
        feats, _ = hip_sift_describe_oriented_batch([a for a, _ in full], lpts, [k for _, k in full], ctx=ctx)
    else:
        feats = hip_sift_describe_batch([a for a, _ in full], lpts, [k for _, k in full], ctx=ctx)
    out, m0 = [], 0
    for lv in pyrs:
        a, b = int(off[m0]), int(off[m0 + len(lv)])
        out.append((pts[a:b], feats[a:b], level[a:b], resp[a:b]))
        m0 += len(lv)
    return out


def hip_pyramid_detect_describe_match(c_img, o_img, max_corners, levels=6, half_steps=True, radius=5, quality_permille=10, second=True,
                                      ctx=None, oriented=False):
    """From two uint8 device images to matches that survive a change of scale between them: ``hip_pyramid_detect_describe`` of
    both pictures, then ``hip_match_descriptors`` of the centre image's descriptors against the other's.  One host
    synchronisation, the level counts, where ``hip_detect_describe_match`` reads its two.  Returns (idx, dist, idx2, dist2,
    feats_c, feats_o, pts_c, pts_o) as ``hip_detect_describe_match`` does, the keypoints in the pictures' own frames.  A
    picture without corners on any level is refused (``ValueError``)."""
    (pc, fc, _, _), (po, fo, _, _) = hip_pyramid_detect_describe([c_img, o_img], max_corners, levels, half_steps, radius, quality_permille,
                                                                 ctx=ctx, oriented=oriented)
    if pc.shape[0] < 1 or po.shape[0] < 1:
        raise ValueError(f"hip_pyramid_detect_describe_match: {pc.shape[0]} and {po.shape[0]} corners; both images need at least one")
    return hip_match_descriptors(fc, fo, second=second, ctx=ctx) + (fc, fo, pc, po)


def image_warp_workspace_bytes(n_problems=1):
    """Scratch of ``hip_image_warp`` / ``hip_image_warp_batch`` of ``n_problems`` problems: 144 bytes per problem, a 256-byte
    multiple, no contract on its contents.  0 for an invalid count."""
    return _native.lib().apap_image_warp_workspace_bytes(int(n_problems))


def _warp_picture(t, dev, who, name):
    if t.dtype != torch.uint8 or not t.is_contiguous() or t.device != dev or t.dim() != 3 or t.shape[2] != 3:
        raise ValueError(f"{who}: {name} must be a contiguous uint8 (h, w, 3) tensor on {dev}")
    if not all(1 <= x <= _native.IMAGE_WARP_MAX_SIDE for x in t.shape[:2]):
        raise ValueError(f"{who}: {name}: sides must be 1 .. {_native.IMAGE_WARP_MAX_SIDE}; got {tuple(t.shape[:2])}")


def hip_image_warp_batch(problems, out=None, out_offsets=None, status=None, ctx=None, work=None):
    """``apap_image_warp_batch_device`` on the current stream of the tensors' device, no host synchronisation: the reference's
    ``image_warping`` (utils.py:93-127) for a sequence of ``(img_base, img2warp, H, direct_blend)`` in one kernel launch.  The
    pictures are contiguous uint8 (h, w, 3) device tensors (problems may share them), ``H`` a host 3 x 3 array: bounds, canvas
    and ``Ht.dot(H)`` are host arithmetic on nine numbers.  ``out``: a flat uint8 device tensor receiving problem p's canvas
    at byte ``out_offsets[p]`` (default: a new tensor, the canvases back to back).  ``status`` (an int32 tensor, may be None)
    is passed on and never written.  ``work`` (uint8) is used when it holds ``image_warp_workspace_bytes(len(problems))``.
    Returns the list of canvases, views of ``out``, not synchronised: the same bytes as ``utils.image_warping``."""
    who = "hip_image_warp_batch"
    problems = list(problems)
    if not problems:
        raise ValueError(f"{who}: no problems")
    _needs_device(problems[0][0], who)
    dev = problems[0][0].device
    geo = []
    for p, (base, src, H, _) in enumerate(problems):
        _warp_picture(base, dev, who, f"problems[{p}]: img_base")
        _warp_picture(src, dev, who, f"problems[{p}]: img2warp")
        geo.append(_native.image_warp_geometry(base.shape[0], base.shape[1], src.shape[0], src.shape[1], H))
    n, bh, bw, sh, sw, M, cw, ch, ox, oy, direct, off, sizes = _native.image_warp_tables(
        [b.shape for b, _, _, _ in problems], [s.shape for _, s, _, _ in problems], [g[0] for g in geo], [(g[1], g[2]) for g in geo],
        [(g[3], g[4]) for g in geo], [bool(d) for _, _, _, d in problems], out_offsets, who)
    if (off < 0).any():
        raise ValueError(f"{who}: negative output offset")
    need = int(max(o + s for o, s in zip(off, sizes)))
    if out is None:
        out = torch.empty(need, dtype=torch.uint8, device=dev)
    if out.dtype != torch.uint8 or out.dim() != 1 or not out.is_contiguous() or out.device != dev or out.numel() < need:
        raise ValueError(f"{who}: out must be a flat contiguous uint8 tensor of at least {need} bytes on {dev}")
    work = _scratch(work, image_warp_workspace_bytes(n), dev)
    _native.check(_native.lib().apap_image_warp_batch_device(
        _native._h(ctx), _addrs([b.data_ptr() for b, _, _, _ in problems]), _ip(bh), _ip(bw),
        _addrs([s.data_ptr() for _, s, _, _ in problems]), _ip(sh), _ip(sw), _dp(M), _ip(cw), _ip(ch), _ip(ox), _ip(oy), _ip(direct), n,
        out.data_ptr(), _native._ptr(off, ctypes.c_longlong), work.data_ptr(), work.numel(),
        status.data_ptr() if status is not None else None, _stream(dev)))
    return [out[int(o):int(o) + s].view(int(h), int(w), 3) for o, s, w, h in zip(off, sizes, cw, ch)]


def hip_image_warp(img_base, img2warp, H, direct_blend=True, status=None, ctx=None, work=None):
    """``apap_image_warp_device``: ``utils.image_warping`` on device tensors, on the current stream, not synchronised.  Returns
    the (canvas_h, canvas_w, 3) uint8 canvas (see ``hip_image_warp_batch``; the single call is the batch of one)."""
    who = "hip_image_warp"
    _needs_device(img_base, who)
    dev = img_base.device
    _warp_picture(img_base, dev, who, "img_base")
    _warp_picture(img2warp, dev, who, "img2warp")
    M, cw, ch, tx, ty = _native.image_warp_geometry(img_base.shape[0], img_base.shape[1], img2warp.shape[0], img2warp.shape[1], H)
    out = torch.empty((ch, cw, 3), dtype=torch.uint8, device=dev)
    work = _scratch(work, image_warp_workspace_bytes(1), dev)
    _native.check(_native.lib().apap_image_warp_device(
        _native._h(ctx), img_base.data_ptr(), img_base.shape[0], img_base.shape[1], img2warp.data_ptr(), img2warp.shape[0],
        img2warp.shape[1], _dp(M), cw, ch, tx, ty, 1 if direct_blend else 0, out.data_ptr(),
        work.data_ptr(), work.numel(), status.data_ptr() if status is not None else None, _stream(dev)))
    return out


def panorama_workspace_bytes(layers):
    """Scratch of ``hip_panorama`` for these layers (``PanoramaLayer``-like): every layer's warp workspace, a 256-byte
    multiple each, no contract on its contents.  0 for invalid arguments."""
    layers, (fw, fh, _, _) = _native.panorama_geometry(layers, "panorama_workspace_bytes")
    mr = _i32([l.local_homography.shape[0] for l in layers])
    mc = _i32([l.local_homography.shape[1] for l in layers])
    return _native.lib().apap_panorama_workspace_bytes(_ip(mr), _ip(mc), _ip(fw), _ip(fh), len(layers))


def panorama_band_workspace_bytes(center, layers, band):
    """Scratch of ``hip_panorama(blend="band", band=band)``: ``panorama_workspace_bytes(layers)`` and, for ``band`` > 0, a
    256-byte aligned slot per view (the centre, then every layer) for its low-pass picture.  0 for invalid arguments."""
    band = _native.panorama_band_radius(band, "panorama_band_workspace_bytes")
    layers, (fw, fh, _, _) = _native.panorama_geometry(layers, "panorama_band_workspace_bytes")
    ih, iw = _i32([l.img.shape[0] for l in layers]), _i32([l.img.shape[1] for l in layers])
    mr = _i32([l.local_homography.shape[0] for l in layers])
    mc = _i32([l.local_homography.shape[1] for l in layers])
    return _native.lib().apap_panorama_band_workspace_bytes(int(center.shape[0]), int(center.shape[1]), _ip(ih), _ip(iw), _ip(mr), _ip(mc),
                                                            _ip(fw), _ip(fh), len(layers), band)


def hip_box_blur(img, radius, out=None, ctx=None):
    """``apap_box_blur_device`` on the current stream, not synchronised: the two-band blend's low-pass picture of ``img``, a
    contiguous (h, w, 3) uint8 device tensor, for ``radius`` 0 .. 32 (``_native.box_blur`` on device tensors).  ``out``: a
    tensor like ``img`` to write into, not ``img`` itself."""
    who = "hip_box_blur"
    radius = _native.panorama_band_radius(radius, who)
    _needs_device(img, who)
    if img.dtype != torch.uint8 or not img.is_contiguous() or img.dim() != 3 or img.shape[2] != 3:
        raise ValueError(f"{who}: the picture must be a contiguous uint8 (h, w, 3) tensor")
    if out is None:
        out = torch.empty_like(img)
    if out.dtype != torch.uint8 or out.shape != img.shape or not out.is_contiguous() or out.device != img.device:
        raise ValueError(f"{who}: out must be a contiguous uint8 tensor of shape {tuple(img.shape)} on {img.device}")
    _native.check(_native.lib().apap_box_blur_device(_native._h(ctx), img.data_ptr(), img.shape[0], img.shape[1], radius, out.data_ptr(),
                                                     _stream(img.device)))
    return out


def dehaze_workspace_bytes(n_images, h, w, channels, refine=30):
    """Workspace of ``hip_dehaze`` (0 for invalid arguments): the counts and the winners' words, the dark channel, the raw
    transmission (3 bytes a pixel) and, with refinement, the guided filter's coefficients (12 more)."""
    return _native.lib().apap_dehaze_workspace_bytes(int(n_images), int(h), int(w), int(channels), int(refine))


def hip_dehaze(imgs, radius=7, omega=0.95, t0=0.1, refine=30, eps=64, return_parts=False, out=None, work=None, ctx=None):
    """``apap_dehaze_device`` on the current stream of the tensor's device, no host synchronisation: uint8 pictures (h, w),
    (h, w, 3), (n, h, w, 1) or (n, h, w, 3); returns a uint8 tensor of that shape (``out`` when given: a tensor like ``imgs``, not
    ``imgs`` itself), or with ``return_parts`` ``(J, t, A)`` with t uint16 of the pictures' (n, h, w) or (h, w) and A uint8
    (n, channels) or (channels,).  The result is what ``hip_corner_detect``, ``hip_sift_describe``, ``hip_notch_denoise`` and
    ``hip_panorama`` take, so a resident chain dehazes and then detects without a host trip.  Same bytes as ``dehaze.dehaze``."""
    from .dehaze import dehaze_arguments
    who = "hip_dehaze"
    q = dehaze_arguments(radius, omega, t0, refine, eps, who=who)
    _needs_device(imgs, who)
    dev = imgs.device
    _contiguous(((imgs, torch.uint8),), dev, who)
    if imgs.dim() not in (2, 3, 4) or imgs.numel() == 0 or (imgs.dim() == 3 and imgs.shape[2] != 3) or (imgs.dim() == 4 and imgs.shape[3] not in (1, 3)):
        raise ValueError(f"{who}: uint8 pictures (h, w), (h, w, 3), (n, h, w, 1) or (n, h, w, 3) expected; got {tuple(imgs.shape)}")
    n, h, w, c = {2: (1, *imgs.shape, 1), 3: (1, *imgs.shape), 4: tuple(imgs.shape)}[imgs.dim()]
    if out is None:
        out = torch.empty_like(imgs)
    elif out.dtype != torch.uint8 or out.shape != imgs.shape or not out.is_contiguous() or out.device != dev or out.data_ptr() == imgs.data_ptr():
        raise ValueError(f"{who}: out must be another contiguous uint8 tensor of shape {tuple(imgs.shape)} on {dev}")
    t = A = None
    if return_parts:
        t = torch.empty((n, h, w) if imgs.dim() == 4 else (h, w), dtype=torch.uint16, device=dev)
        A = torch.empty((n, c) if imgs.dim() == 4 else (c,), dtype=torch.uint8, device=dev)
    work = _scratch(work, max(dehaze_workspace_bytes(n, h, w, c, q[3]), 256), dev)
    _native.check(_native.lib().apap_dehaze_device(
        _native._h(ctx), imgs.data_ptr(), int(n), int(h), int(w), int(c), *q, out.data_ptr(), t.data_ptr() if return_parts else None,
        A.data_ptr() if return_parts else None, work.data_ptr(), work.numel(), _stream(dev)))
    return (out, t, A) if return_parts else out


def hip_panorama(center, layers, blend="mean", out=None, status=None, ctx=None, work=None, ramp=32, sampling=None, gain=None,
                 gain_step=4, sigma_n=10.0, sigma_g=0.1, return_gains=False, band=8):
    """``apap_panorama_device`` (``blend="ramp"``: ``apap_panorama_ramp_device`` with the ramp width ``ramp``, an integer 1 ..
    256 that the other blends ignore) on the current stream of the tensors' device, no host synchronisation: the centre picture and
    every layer on one canvas in one fused pass (``apap.panorama`` on device tensors).  ``center`` (h, w, 3) uint8; a layer is
    a ``PanoramaLayer`` (or a 5-tuple in its order) of device tensors - ``img`` (h, w, 3) uint8, ``local_homography`` (rows,
    cols, 3, 3) float32, ``mesh`` = (mesh_w, mesh_h) float64 - with host ``final_size`` and ``offset``; layers may share
    tensors.  ``out``: a contiguous (H, W, 3) uint8 tensor to write into; ``status``: an int32 tensor of at least one word per
    layer, zeroed by the caller (default: a new one), into which layer k's set-up ORs its bits at [k]; ``work`` (uint8) is
    used when it holds ``panorama_workspace_bytes(layers)``.  Returns ``(canvas, (W, H, OX, OY), status)``, not synchronised;
    ``_native.raise_for_status(int(status[k]), ...)`` turns a word into the reference's exception.  The grids are not
    modified.  ``sampling``: ``None`` (the context's ``warp_sampling``), ``"nearest"`` or ``"bilinear"`` for this call only.

    ``gain``: ``None`` (the call above), K + 1 host integers ``q`` (``apap_panorama_gain_device``), or ``"auto"``
    (``apap_panorama_auto_gain_device``): the overlap statistics on every ``gain_step``-th canvas row and column, the solve
    on the device and the gained blend, one after the other on the stream - nothing waits for the host.  With
    ``return_gains=True`` and ``"auto"`` a fourth value follows: ``_native.PanoramaGains`` of device tensors (``gains``
    float64, ``q`` int32, ``N``, ``S`` int64 holding the uint64 statistics), not synchronised.

    ``blend="band"``: ``apap_panorama_band_device``, the two-band blend of ``apap.panorama`` with the ramp width ``ramp`` and
    the low-pass radius ``band``, an integer 0 .. 32 that every other blend ignores; ``work`` is used when it holds
    ``panorama_band_workspace_bytes(center, layers, band)``.  K + 1 integers as ``gain`` go into the same call.  With
    ``gain="auto"`` the statistics run on the stream, the call WAITS for them once, solves on the host and enqueues the blend
    under the gains it found (``return_gains`` then gives host arrays); there is no fused resident form of that."""
    who = "hip_panorama"
    _native.sampling_value(sampling, who)
    _needs_device(center, who)
    dev = center.device
    auto = isinstance(gain, str)
    if auto and gain != "auto":
        raise ValueError(f"{who}: gain must be None, 'auto' or K + 1 integers; got {gain!r}")
    if return_gains and not auto:
        raise ValueError(f"{who}: return_gains goes with gain='auto'")
    is_band = blend == "band"
    host_gains = None
    if is_band:
        _native.panorama_entry("ramp", ramp, who)
        band = _native.panorama_band_radius(band, who)
        if auto:        # the statistics, one wait, the solve on the host; then the blend under q
            N, S, _ = hip_panorama_gain_stats(center, layers, step=gain_step, status=status, ctx=ctx, work=work, sampling=sampling)
            N, S = N.cpu().numpy().view(np.uint64), S.cpu().numpy().view(np.uint64)
            g, q, _ = _native.panorama_gain_solve(N, S, sigma_n, sigma_g)
            host_gains = _native.PanoramaGains(g, q, N, S)
            gain, auto = q, False
        entry = _native.lib().apap_panorama_band_device
        tail = [int(ramp), band]
    elif gain is None:
        entry, mode = _native.panorama_entry(blend, ramp, who, device_form=True)
        tail = [mode]
    else:
        tail = list(_native.panorama_gain_mode(blend, ramp, who))
        entry = _native.lib().apap_panorama_auto_gain_device if auto else _native.lib().apap_panorama_gain_device
    layers, (fw, fh, ox, oy) = _native.panorama_geometry(layers, who)
    n = len(layers)
    gains = None
    if auto:
        tail += [_native._gain_step(gain_step, who), float(sigma_n), float(sigma_g)]
    elif gain is not None:
        q_host = _native.panorama_gain_q(gain, n + 1, who)
        tail.append(_ip(q_host))
    elif is_band:
        tail.append(None)       # apap_panorama_band_device takes NULL for no gains

    def tensor(t, dtype, name, k):
        if not isinstance(t, torch.Tensor) or t.dtype != dtype or not t.is_contiguous() or t.device != dev:
            raise ValueError(f"{who}: layer {k}: {name} must be a contiguous {dtype} tensor on {dev}")
        return t

    if center.dtype != torch.uint8 or not center.is_contiguous() or center.dim() != 3 or center.shape[2] != 3:
        raise ValueError(f"{who}: the centre must be a contiguous uint8 (h, w, 3) tensor")
    imgs, grids, mws, mhs = [], [], [], []
    for k, l in enumerate(layers):
        imgs.append(tensor(l.img, torch.uint8, "img", k))
        grids.append(tensor(l.local_homography, torch.float32, "local_homography", k))
        mws.append(tensor(l.mesh[0], torch.float64, "mesh_w", k))
        mhs.append(tensor(l.mesh[1], torch.float64, "mesh_h", k))
        if imgs[k].dim() != 3 or imgs[k].shape[2] != 3 or grids[k].dim() != 4 or tuple(grids[k].shape[2:]) != (3, 3):
            raise ValueError(f"{who}: layer {k}: img must be (h, w, 3) and local_homography (rows, cols, 3, 3)")
    W, H, OX, OY = _native.panorama_bounds(center.shape, fw, fh, ox, oy)
    if out is None:
        out = torch.empty((H, W, 3), dtype=torch.uint8, device=dev)
    if out.dtype != torch.uint8 or tuple(out.shape) != (H, W, 3) or not out.is_contiguous() or out.device != dev:
        raise ValueError(f"{who}: out must be a contiguous uint8 tensor of shape {(H, W, 3)} on {dev}")
    if status is None:
        status = torch.zeros(n, dtype=torch.int32, device=dev)
    if status.dtype != torch.int32 or status.numel() < n or not status.is_contiguous() or status.device != dev:
        raise ValueError(f"{who}: status must be a contiguous int32 tensor of at least {n} words on {dev}")
    ih, iw = _i32([t.shape[0] for t in imgs]), _i32([t.shape[1] for t in imgs])
    mr, mc = _i32([t.shape[0] for t in grids]), _i32([t.shape[1] for t in grids])
    nw, nh = _i32([t.numel() for t in mws]), _i32([t.numel() for t in mhs])
    table = [_addrs([t.data_ptr() for t in ts]) for ts in (imgs, grids, mws, mhs)]
    p_mr, p_mc, p_fw, p_fh = _ip(mr), _ip(mc), _ip(fw), _ip(fh)
    if is_band:
        need = _native.lib().apap_panorama_band_workspace_bytes(center.shape[0], center.shape[1], _ip(ih), _ip(iw), p_mr, p_mc, p_fw, p_fh, n, band)
    else:
        need = _native.lib().apap_panorama_workspace_bytes(p_mr, p_mc, p_fw, p_fh, n)
    work = _scratch(work, need, dev)
    after = []
    if auto:
        gains = _native.PanoramaGains(torch.empty(n + 1, dtype=torch.float64, device=dev), torch.empty(n + 1, dtype=torch.int32, device=dev),
                                      torch.empty((n + 1, n + 1), dtype=torch.int64, device=dev),
                                      torch.empty((n + 1, n + 1), dtype=torch.int64, device=dev))
        flag = torch.empty(1, dtype=torch.int32, device=dev)
        after = [gains.N.data_ptr(), gains.S.data_ptr(), gains.gains.data_ptr(), gains.q.data_ptr(), flag.data_ptr()]
    with _native.sampling_scope(ctx, sampling, who) as ctx:
        _native.check(entry(
            _native._h(ctx), center.data_ptr(), center.shape[0], center.shape[1], table[0], _ip(ih), _ip(iw), table[1], p_mr, p_mc,
            table[2], _ip(nw), table[3], _ip(nh), p_fw, p_fh, _ip(ox), _ip(oy), n, *tail, out.data_ptr(), *after, work.data_ptr(),
            work.numel(), status.data_ptr(), _stream(dev)))
    return (out, (W, H, OX, OY), status, host_gains or gains) if return_gains else (out, (W, H, OX, OY), status)


def hip_panorama_gain_stats(center, layers, step=4, N=None, S=None, status=None, ctx=None, work=None, sampling=None):
    """``apap_panorama_gain_stats_device`` on the current stream, not synchronised: the overlap statistics of the centre and
    the layers (as in :func:`hip_panorama`) over the canvas pixels with ``X % step == 0 and Y % step == 0``.  ``N``, ``S``:
    contiguous (K + 1, K + 1) int64 tensors to write into (the uint64 counts and sums; the call zeroes them itself; default:
    new ones); ``work`` as in :func:`hip_panorama`.  Returns ``(N, S, status)``."""
    who = "hip_panorama_gain_stats"
    _native.sampling_value(sampling, who)
    _needs_device(center, who)
    dev = center.device
    step = _native._gain_step(step, who)
    layers, (fw, fh, ox, oy) = _native.panorama_geometry(layers, who)
    n = len(layers)
    if center.dtype != torch.uint8 or not center.is_contiguous() or center.dim() != 3 or center.shape[2] != 3:
        raise ValueError(f"{who}: the centre must be a contiguous uint8 (h, w, 3) tensor")
    for k, l in enumerate(layers):
        for t, dtype, name in ((l.img, torch.uint8, "img"), (l.local_homography, torch.float32, "local_homography"),
                               (l.mesh[0], torch.float64, "mesh_w"), (l.mesh[1], torch.float64, "mesh_h")):
            if not isinstance(t, torch.Tensor) or t.dtype != dtype or not t.is_contiguous() or t.device != dev:
                raise ValueError(f"{who}: layer {k}: {name} must be a contiguous {dtype} tensor on {dev}")
        if l.img.dim() != 3 or l.img.shape[2] != 3 or l.local_homography.dim() != 4 or tuple(l.local_homography.shape[2:]) != (3, 3):
            raise ValueError(f"{who}: layer {k}: img must be (h, w, 3) and local_homography (rows, cols, 3, 3)")
    _native.panorama_bounds(center.shape, fw, fh, ox, oy)
    tables = []
    for t, name in ((N, "N"), (S, "S")):
        if t is None:
            t = torch.empty((n + 1, n + 1), dtype=torch.int64, device=dev)
        if t.dtype != torch.int64 or tuple(t.shape) != (n + 1, n + 1) or not t.is_contiguous() or t.device != dev:
            raise ValueError(f"{who}: {name} must be a contiguous int64 tensor of shape {(n + 1, n + 1)} on {dev}")
        tables.append(t)
    if status is None:
        status = torch.zeros(n, dtype=torch.int32, device=dev)
    if status.dtype != torch.int32 or status.numel() < n or not status.is_contiguous() or status.device != dev:
        raise ValueError(f"{who}: status must be a contiguous int32 tensor of at least {n} words on {dev}")
    ih, iw = _i32([l.img.shape[0] for l in layers]), _i32([l.img.shape[1] for l in layers])
    mr, mc = _i32([l.local_homography.shape[0] for l in layers]), _i32([l.local_homography.shape[1] for l in layers])
    nw, nh = _i32([l.mesh[0].numel() for l in layers]), _i32([l.mesh[1].numel() for l in layers])
    table = [_addrs([t.data_ptr() for t in ts]) for ts in ([l.img for l in layers], [l.local_homography for l in layers],
                                                           [l.mesh[0] for l in layers], [l.mesh[1] for l in layers])]
    p_mr, p_mc, p_fw, p_fh = _ip(mr), _ip(mc), _ip(fw), _ip(fh)
    work = _scratch(work, _native.lib().apap_panorama_workspace_bytes(p_mr, p_mc, p_fw, p_fh, n), dev)
    with _native.sampling_scope(ctx, sampling, who) as ctx:
        _native.check(_native.lib().apap_panorama_gain_stats_device(
            _native._h(ctx), center.data_ptr(), center.shape[0], center.shape[1], table[0], _ip(ih), _ip(iw), table[1], p_mr, p_mc,
            table[2], _ip(nw), table[3], _ip(nh), p_fw, p_fh, _ip(ox), _ip(oy), n, step, tables[0].data_ptr(), tables[1].data_ptr(),
            work.data_ptr(), work.numel(), status.data_ptr(), _stream(dev)))
    return tables[0], tables[1], status
