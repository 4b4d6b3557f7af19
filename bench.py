#!/usr/bin/env python3
"""Benchmark of the APAP hot path on MI355X: local homographies/s and warp Mpix/s on the
4K pair / 200x200 mesh / 2000 keypoints configuration of BASELINE.json (C3).

    python bench.py [--gpus N] [--steps K] [--warmup W] [--config C3] [--cells-config C4]
                    [--variant auto|valu|mfma|mfma4|mfma4x2] [--full [--no-cpu-baseline] [--no-cells] [--no-call-level]]
                    [--dump-outputs DIR]

A "step" is one pass of the hot path over one image pair with all inputs resident in
HBM: the per-cell solve (assemble + eigen-solve kernels) and the backward warp
(set-up + gather kernels).  The two halves of the metric are timed in two regions of
exactly K steps each, both bracketed by a barrier and a device synchronise:
``value`` = cells * K * N / t_solve (homographies/s), ``warp.value`` = canvas pixels
* K * N / t_warp (Mpix/s), ``ms_per_step`` = (t_solve + t_warp) / K.

A plain run does only what that headline needs: it sets up the pair, conditions the clock and warms up, times the K steps,
writes ``--dump-outputs`` and prints the line (``value``, ``warp``, ``ms_per_step``, ``pair_per_rank`` and the configuration).
``--full`` goes on to measure everything below in the same process and adds it to the same line; every timed region of
that part takes ``extra_steps`` = min(K, 50) steps, so that the run's length follows K * ``ms_per_step`` plus a fixed part.
The ``--no-*`` switches leave objects out of a ``--full`` run and do nothing without it.

``--gpus N`` with N > 1 and no WORLD_SIZE in the environment starts the N ranks itself (a child
``python -m torch.distributed.run --nproc-per-node N bench.py ...`` before anything touches the
GPU); under torch.distributed.run it is one rank per GPU over RCCL.  A ``--full`` run measures BOTH ways
the path shards and puts both in the one JSON line:

* the headline (``value``, ``pair_per_rank``): every rank owns a 4K pair (config C3) - independent
  units, no data-path collective, weak scaling;
* ``pairs`` = BASELINE config 5 as it is written: 64 independent 4K pairs at 100 x 100, dealt over the
  ranks, each rank's share in ONE batched launch, no collective - strong scaling;
* ``cells`` = ONE pair of ``--cells-config`` (C4: 8K, 5000 keypoints, 400 x 400 mesh) with its mesh
  rows sharded over the ranks by cvx_proj_amd.dist.ShardedSolver: table broadcast from rank 0 once
  per pair, per-rank solve, all-gather of the H grid; warp by canvas-row bands + all-gather - strong
  scaling.  At N = 1 it is the single-GPU baseline of that curve.

Further objects of ``--full``: ``roofline`` for the dominant kernel (K1, timed live with HIP events on the launch
stream); ``roofline_warp`` / ``roofline_warp_cold`` for K3 on the headline canvas (launches back to back,
source and canvas warm / rotated through 640 MB), ``cells.roofline_warp`` for the same kernel on the
cells configuration's canvas and ``pairs.warp.roofline`` for the batched warp of config 5; ``standalone``
(the solve and the warp as calls of their own, without the warp-ready tail / with the set-up launch);
``call_level`` (numpy in -> numpy out through the host-buffer entry points: host set-up, PCIe and
synchronisation included); ``pipeline`` (apap.py's __main__ as one resident pass: from ordinary numpy
arrays, from page-locked ones, and as the reference's chain of calls); ``cli`` (fresh-process wall time of the drop-in command, one
pair and sixteen); ``configs`` (BASELINE's other single-GPU configurations, C1 and C2, on the headline's definitions); ``moments24``
(the opt-in 24-sum solve forms beside the default, with how far their grids are from it) and ``cpu_baseline`` (the oracle's
faithful-loop numpy port on this host: 1 thread, default BLAS threads, all usable cores).

Multi-rank runs: a 120 s collective timeout, a tiny first collective and a phase marker on stderr before
every phase; a failure ends in a non-zero exit code with ``bench_failed`` on stderr.
``APAP_BENCH_BACKEND=gloo`` rehearses more ranks than GPUs; ``APAP_BENCH_FORCE_GROUP=1`` (with RANK=0,
WORLD_SIZE=1, MASTER_ADDR / MASTER_PORT) runs ONE rank through an ``nccl`` group and every collective
of the multi-rank paths - first contact with RCCL on a one-GPU box; ``APAP_BENCH_SELFTEST=1`` is the
launch + rendezvous + one collective without a GPU.

``--dump-outputs DIR`` writes what the headline's timed path computed in its last step, as its caller receives it, to
``DIR/*.npy`` (see ``dump_outputs``): the inputs are seeded, so two builds run with the same arguments can be compared
output for output.
"""
import os

os.environ.setdefault("OPENBLAS_NUM_THREADS", "1")   # the CPU baseline's first row is the 1-thread port
os.environ.setdefault("OMP_NUM_THREADS", "1")
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")

import argparse
import ctypes
import json
import socket
import subprocess
import sys
import time

import numpy as np
import torch

T0 = time.time()
ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

from cvx_proj_amd import _native as N  # noqa: E402
from cvx_proj_amd.synth import CONFIGS, config_pair  # noqa: E402

METRIC = "local homographies/sec + Mpix/sec warp, 4K pair 200x200 mesh"
# Peaks (DESIGN.md section "Rooflines"): fp64 matrix = fp64 vector = 78.6 TFLOP/s is AMD's
# MI355X datasheet figure (256 CU x 4 SIMD x 2.4 GHz x 32 flop/clk); HBM 8 TB/s spec from
# /opt/skills/guides/MI355X_MICROARCH.md.
PEAK_FP64_TFLOPS = 78.6
PEAK_HBM_GBS = 8000.0
# algorithmic flops per (cell, keypoint) of K1, SURVEY.md 8(d): 8 (weight) + 48 (24 FMAs) + 2
K1_FLOPS_PER_CELL_POINT = 58.0
#: the most timed steps of any region other than the headline's two (the default --steps: a default run times every region as
#: many times as the headline)
EXTRA_STEPS = 50
VARIANTS = {"auto": 0, "valu": 1, "mfma": 2, "mfma4": 3, "mfma4x2": 4}


class Resident:
    """One image pair (or a batch of pairs sharing mesh and image) with everything the hot
    path reads resident in HBM."""

    def __init__(self, pair, dev, batch=1, seed_pairs=None, ctx=None):
        self.pair = pair
        self.batch = batch
        self.ctx = N._h(ctx)
        moments = ctx.get("moments") if ctx is not None else 30      # the table's layout follows the context (APAP_OPT_MOMENTS)
        q = N.host_prepare(pair.src, pair.dst)
        table = N.host_build_table(pair.src, q["cf1"], q["cf2"], moments=moments)
        den = N.host_build_denorm(q["iC2"], q["C1"], q["iN2"], q["N1"])
        if batch > 1:      # independent keypoint sets (different seeds), same mesh
            tabs, dens = [table], [den]
            for extra in seed_pairs:
                qe = N.host_prepare(extra.src, extra.dst)
                tabs.append(N.host_build_table(extra.src, qe["cf1"], qe["cf2"], moments=moments))
                dens.append(N.host_build_denorm(qe["iC2"], qe["C1"], qe["iN2"], qe["N1"]))
            table, den = np.stack(tabs), np.stack(dens)
        self.n = len(pair.src)
        self.rows, self.cols = pair.vertices.shape[:2]
        self.cells = self.rows * self.cols
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
        self.table, self.den = t(table), t(den)
        self.vert = t(pair.vertices.reshape(-1, 2))
        self.H = torch.zeros((batch * self.cells, 9), dtype=torch.float32, device=dev)
        self.work_bytes = max(N.lib().apap_solve_batch_workspace_bytes(self.ctx, self.n, self.cells, batch), 256)
        self.work = torch.empty(self.work_bytes, dtype=torch.uint8, device=dev)
        self.img = t(pair.img)
        self.mesh_w, self.mesh_h = t(pair.mesh[0]), t(pair.mesh[1])
        self.out = torch.zeros((pair.final_h, pair.final_w, 3), dtype=torch.uint8, device=dev)
        self.wwork_bytes = N.lib().apap_warp_workspace_bytes(self.rows, self.cols, pair.final_w, pair.final_h)
        self.wwork = torch.empty(self.wwork_bytes, dtype=torch.uint8, device=dev)
        self.status = torch.zeros(1, dtype=torch.int32, device=dev)
        # the resident pipeline's form of the step (one pair per launch): the canvas row / column tables of this geometry are
        # built once (here), the solve's tail leaves every cell warp ready in `pwork`, the warp step is the gather kernel alone
        self.resident = batch == 1
        self.pwork = torch.zeros(self.wwork_bytes, dtype=torch.uint8, device=dev)
        self._warp_phases(torch.cuda.current_stream().cuda_stream, N.WARP_GEOMETRY, self.pwork)

    def _warp_phases(self, stream, phases, work, img=None, out=None):
        p = self.pair
        img = self.img if img is None else img
        out = self.out if out is None else out
        N.check(N.lib().apap_warp_batch_device(self.ctx, img.data_ptr(), 0, p.shape[0], p.shape[1], None, 0, 0, 0, self.H.data_ptr(),
                                               self.rows, self.cols, self.mesh_w.data_ptr(), p.mesh.shape[1], self.mesh_h.data_ptr(),
                                               p.mesh.shape[1], p.final_w, p.final_h, p.off_x, p.off_y, 0, p.final_h, out.data_ptr(), 0,
                                               None, 1, phases, work.data_ptr(), self.wwork_bytes, self.status.data_ptr(),
                                               ctypes.c_void_p(stream)))

    def solve_plain(self, stream):
        """The solve alone (H grid only): what a caller that does not warp on this GPU runs."""
        p = self.pair
        N.check(N.lib().apap_solve_batch_device(self.ctx, self.table.data_ptr(), self.n, self.vert.data_ptr(), 0, self.cells,
                                                p.gamma, p.sigma, self.den.data_ptr(), self.H.data_ptr(), self.batch,
                                                self.work.data_ptr(), self.work_bytes, ctypes.c_void_p(stream)))

    def solve(self, stream):
        """The solve of the resident pipeline: H grid + every cell warp ready (apap_solve_warp_batch_device)."""
        if not self.resident:
            return self.solve_plain(stream)
        p = self.pair
        N.check(N.lib().apap_solve_warp_batch_device(self.ctx, self.table.data_ptr(), self.n, self.vert.data_ptr(), 0, p.gamma, p.sigma,
                                                     self.den.data_ptr(), self.H.data_ptr(), 1, self.work.data_ptr(), self.work_bytes,
                                                     self.rows, self.cols, self.mesh_w.data_ptr(), p.mesh.shape[1],
                                                     self.mesh_h.data_ptr(), p.mesh.shape[1], p.final_w, p.final_h, p.off_x, p.off_y,
                                                     self.pwork.data_ptr(), self.wwork_bytes, self.status.data_ptr(),
                                                     ctypes.c_void_p(stream)))

    def warp(self, stream, img=None, out=None):
        """The warp step of the resident pipeline: the gather kernel on the tables the solve left (no set-up launch)."""
        if not self.resident:
            return self.warp_standalone(stream, img, out)
        self._warp_phases(stream, N.WARP_GATHER, self.pwork, img, out)

    def warp_standalone(self, stream, img=None, out=None):
        """apap_warp_device on a grid from anywhere: set-up launch (inverses, records, lookup tables) + gather."""
        self._warp_phases(stream, N.WARP_ALL, self.wwork, img, out)

    def second_lane(self):
        """A second canvas, workspace and status word on a stream of its own: the same pair warped twice at once
        (what a caller with several pairs in flight gets; timed as an extra, not part of ``value``)."""
        if not hasattr(self, "_lane2"):
            self._lane2 = (torch.zeros_like(self.out), torch.empty_like(self.wwork), torch.zeros_like(self.status),
                           torch.cuda.Stream(self.out.device))
        return self._lane2

    def warp_lane2(self):
        p = self.pair
        out, work, status, stream = self.second_lane()
        N.check(N.lib().apap_warp_device(self.ctx, self.img.data_ptr(), p.shape[0], p.shape[1], self.H.data_ptr(), self.rows,
                                         self.cols, self.mesh_w.data_ptr(), p.mesh.shape[1], self.mesh_h.data_ptr(),
                                         p.mesh.shape[1], p.final_w, p.final_h, p.off_x, p.off_y,
                                         out.data_ptr(), None, work.data_ptr(), self.wwork_bytes,
                                         status.data_ptr(), ctypes.c_void_p(stream.cuda_stream)))

    def cold_sets(self, min_bytes):
        """Copies of (source image, canvas) whose total exceeds `min_bytes`: warping them in rotation, every launch
        finds its 25 MB source and its 27 MB canvas in HBM only - the 256 MiB Infinity Cache and the L2s hold the
        sets touched last (MI355X_MICROARCH.md, Infinity Cache: a buffer stays resident only while everything
        touched between two uses of it fits ~256 MiB)."""
        if not hasattr(self, "_cold"):
            per = self.img.numel() + self.out.numel()
            n = max(2, -(-int(min_bytes) // per))
            self._cold = [(self.img.clone(), torch.zeros_like(self.out)) for _ in range(n)]
        return self._cold

    def equalize(self, stream):
        """Per-channel histogram equalisation of the source image (the pre-processing of
        apap.py:236-237); timed as an extra, not part of ``value``."""
        p = self.pair
        if not hasattr(self, "eq_out"):
            self.eq_out = torch.empty_like(self.img)
            self.eq_work = torch.zeros(N.lib().apap_equalize_workspace_bytes(3), dtype=torch.uint8, device=self.img.device)
        N.check(N.lib().apap_equalize_hist_device(self.ctx, self.img.data_ptr(), p.shape[0], p.shape[1], 3, self.eq_out.data_ptr(),
                                                  self.eq_work.data_ptr(), self.eq_work.numel(), ctypes.c_void_p(stream)))

    def ransac(self, stream):
        """Device half of the seed-homography estimator (baseline_stitch_test.py:42) on the pair's
        correspondences; timed as an extra, not part of ``value``."""
        p = self.pair
        if not hasattr(self, "r_src"):
            dev = self.img.device
            self.r_src = torch.from_numpy(np.ascontiguousarray(p.src, dtype=np.float32)).to(dev)
            self.r_dst = torch.from_numpy(np.ascontiguousarray(p.dst, dtype=np.float32)).to(dev)
            self.r_wb = N.lib().apap_ransac_workspace_bytes(self.n, N.RANSAC_ITERATIONS)
            self.r_work = torch.zeros(self.r_wb, dtype=torch.uint8, device=dev)
            self.r_H = torch.zeros(9, dtype=torch.float64, device=dev)
            self.r_mask = torch.zeros(self.n, dtype=torch.uint8, device=dev)
            self.r_res = torch.zeros(2, dtype=torch.int32, device=dev)
        N.check(N.lib().apap_ransac_device(self.ctx, self.r_src.data_ptr(), self.r_dst.data_ptr(), self.n, 5.0, N.RANSAC_ITERATIONS,
                                           ctypes.c_ulonglong(N.RANSAC_SEED), self.r_H.data_ptr(), self.r_mask.data_ptr(),
                                           self.r_res.data_ptr(), self.r_work.data_ptr(), self.r_wb,
                                           ctypes.c_void_p(stream)))

    def stitch(self, stream):
        """Fused warp + paste + uniform_blend (the reference's commented-out tail,
        apap.py:258-262); timed as an extra, not part of ``value``."""
        p = self.pair
        if not hasattr(self, "center"):
            g = torch.Generator(device="cpu").manual_seed(1)
            self.center = torch.randint(0, 256, p.shape, dtype=torch.uint8, generator=g).to(self.img.device)
        N.check(N.lib().apap_stitch_device(self.ctx, self.img.data_ptr(), p.shape[0], p.shape[1], self.center.data_ptr(),
                                           p.shape[0], p.shape[1], self.H.data_ptr(), self.rows, self.cols,
                                           self.mesh_w.data_ptr(), p.mesh.shape[1], self.mesh_h.data_ptr(),
                                           p.mesh.shape[1], p.final_w, p.final_h, p.off_x, p.off_y,
                                           self.out.data_ptr(), None, self.wwork.data_ptr(), self.wwork_bytes,
                                           self.status.data_ptr(), ctypes.c_void_p(stream)))


class PairBatch:
    """BASELINE config 5: independent pairs sharing one mesh shape, this rank's share solved in ONE batched
    launch (blockIdx.z = pair) and warped in ONE batched set of launches (one set-up launch over every pair's cells,
    one gather launch over every canvas); keypoint tables, de-normalisation blocks, vertices, the H grids, the source
    images and the canvases resident."""

    def __init__(self, cfg, indices, dev, ctx=None, with_images=True):
        self.ctx = N._h(ctx)
        self.batch = len(indices)
        tabs, dens, imgs = [], [], []
        pair = None
        for k in indices:
            pair = config_pair(cfg, with_image=with_images, seed_offset=k)
            q = N.host_prepare(pair.src, pair.dst)
            tabs.append(N.host_build_table(pair.src, q["cf1"], q["cf2"]))
            dens.append(N.host_build_denorm(q["iC2"], q["C1"], q["iN2"], q["N1"]))
            if with_images:
                imgs.append(torch.from_numpy(pair.img).to(dev))        # 25 MB per 4K pair: upload at once, keep the host small
                if k != indices[0]:
                    pair.img = None
                else:
                    self.first = pair
        self.pair = pair
        self.n = len(pair.src)
        self.rows, self.cols = pair.vertices.shape[:2]
        self.cells = self.rows * self.cols
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
        self.table, self.den = t(np.stack(tabs)), t(np.stack(dens))
        self.vert = t(pair.vertices.reshape(-1, 2))        # every pair of a configuration has the same canvas, hence mesh
        self.H = torch.zeros((self.batch * self.cells, 9), dtype=torch.float32, device=dev)
        self.work_bytes = max(N.lib().apap_solve_batch_workspace_bytes(self.ctx, self.n, self.cells, self.batch), 256)
        self.work = torch.empty(self.work_bytes, dtype=torch.uint8, device=dev)
        if with_images:
            self.imgs = torch.stack(imgs)
            del imgs
            self.mesh_w, self.mesh_h = t(pair.mesh[0]), t(pair.mesh[1])
            self.out = torch.zeros((self.batch, pair.final_h, pair.final_w, 3), dtype=torch.uint8, device=dev)
            self.wwork_bytes = N.lib().apap_warp_batch_workspace_bytes(self.rows, self.cols, pair.final_w, pair.final_h, self.batch)
            self.wwork = torch.empty(self.wwork_bytes, dtype=torch.uint8, device=dev)
            self.status = torch.zeros(1, dtype=torch.int32, device=dev)

    def solve(self, stream):
        p = self.pair
        N.check(N.lib().apap_solve_batch_device(self.ctx, self.table.data_ptr(), self.n, self.vert.data_ptr(), 0, self.cells,
                                                p.gamma, p.sigma, self.den.data_ptr(), self.H.data_ptr(), self.batch,
                                                self.work.data_ptr(), self.work_bytes, ctypes.c_void_p(stream)))

    def warp(self, stream, phases=N.WARP_ALL):
        p = self.pair
        N.check(N.lib().apap_warp_batch_device(self.ctx, self.imgs.data_ptr(), self.imgs[0].numel(), p.shape[0], p.shape[1], None, 0, 0, 0,
                                               self.H.data_ptr(), self.rows, self.cols, self.mesh_w.data_ptr(), p.mesh.shape[1],
                                               self.mesh_h.data_ptr(), p.mesh.shape[1], p.final_w, p.final_h, p.off_x, p.off_y, 0,
                                               p.final_h, self.out.data_ptr(), self.out[0].numel(), None, self.batch, phases,
                                               self.wwork.data_ptr(), self.wwork_bytes, self.status.data_ptr(), ctypes.c_void_p(stream)))

    def prepare_whole_job(self, chunks):
        """Split the rank's pairs into `chunks` groups, each with a warp workspace of its own (geometry tables built once, here):
        the whole job then runs solve(group k + 1) on one stream beside warp(group k) on another."""
        dev = self.out.device
        p = self.pair
        chunks = max(1, min(chunks, self.batch))
        cuts = [self.batch * k // chunks for k in range(chunks + 1)]
        self.groups = []
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            nb = hi - lo
            wb = N.lib().apap_warp_batch_workspace_bytes(self.rows, self.cols, p.final_w, p.final_h, nb)
            g = {"lo": lo, "n": nb, "wwork": torch.zeros(wb, dtype=torch.uint8, device=dev), "wb": wb,
                 "sb": max(N.lib().apap_solve_batch_workspace_bytes(self.ctx, self.n, self.cells, nb), 256)}
            g["swork"] = torch.empty(g["sb"], dtype=torch.uint8, device=dev)
            g["event"] = torch.cuda.Event()
            self.groups.append(g)
            N.check(N.lib().apap_warp_batch_device(self.ctx, None, 0, 0, 0, None, 0, 0, 0, None, self.rows, self.cols,
                                                   self.mesh_w.data_ptr(), p.mesh.shape[1], self.mesh_h.data_ptr(), p.mesh.shape[1],
                                                   p.final_w, p.final_h, p.off_x, p.off_y, 0, p.final_h, None, 0, None, nb,
                                                   N.WARP_GEOMETRY, g["wwork"].data_ptr(), wb, self.status.data_ptr(),
                                                   ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
        self.side = torch.cuda.Stream(dev)
        torch.cuda.synchronize()

    def whole_job(self, overlapped=True):
        """Solve and warp every pair of the rank: group by group, the solve's tail leaving the cells warp ready, the gather of
        group k on the side stream while group k + 1 is solved on the main stream (`overlapped`), or everything on one stream."""
        p = self.pair
        main = torch.cuda.current_stream()
        for g in self.groups:
            lo, nb = g["lo"], g["n"]
            N.check(N.lib().apap_solve_warp_batch_device(
                self.ctx, self.table[lo:].data_ptr(), self.n, self.vert.data_ptr(), 0, p.gamma, p.sigma, self.den[lo:].data_ptr(),
                self.H[lo * self.cells:].data_ptr(), nb, g["swork"].data_ptr(), g["sb"], self.rows, self.cols, self.mesh_w.data_ptr(),
                p.mesh.shape[1], self.mesh_h.data_ptr(), p.mesh.shape[1], p.final_w, p.final_h, p.off_x, p.off_y, g["wwork"].data_ptr(),
                g["wb"], self.status.data_ptr(), ctypes.c_void_p(main.cuda_stream)))
            st = main
            if overlapped:
                g["event"].record(main)
                self.side.wait_event(g["event"])
                st = self.side
            N.check(N.lib().apap_warp_batch_device(self.ctx, self.imgs[lo:].data_ptr(), self.imgs[0].numel(), p.shape[0], p.shape[1], None,
                                                   0, 0, 0, self.H[lo * self.cells:].data_ptr(), self.rows, self.cols,
                                                   self.mesh_w.data_ptr(), p.mesh.shape[1], self.mesh_h.data_ptr(), p.mesh.shape[1],
                                                   p.final_w, p.final_h, p.off_x, p.off_y, 0, p.final_h, self.out[lo:].data_ptr(),
                                                   self.out[0].numel(), None, nb, N.WARP_GATHER, g["wwork"].data_ptr(), g["wb"],
                                                   self.status.data_ptr(), ctypes.c_void_p(st.cuda_stream)))
        if overlapped:
            main.wait_stream(self.side)

    def check_against_single_launches(self, stream, which=(0,)):
        """The batched canvases of pairs `which` (positions in this batch) against one apap_warp_device launch each."""
        p = self.pair
        wb = N.lib().apap_warp_workspace_bytes(self.rows, self.cols, p.final_w, p.final_h)
        work = torch.empty(wb, dtype=torch.uint8, device=self.out.device)
        one = torch.zeros_like(self.out[0])
        for i in which:
            N.check(N.lib().apap_warp_device(self.ctx, self.imgs[i].data_ptr(), p.shape[0], p.shape[1],
                                             self.H[i * self.cells:].data_ptr(), self.rows, self.cols, self.mesh_w.data_ptr(),
                                             p.mesh.shape[1], self.mesh_h.data_ptr(), p.mesh.shape[1], p.final_w, p.final_h, p.off_x,
                                             p.off_y, one.data_ptr(), None, work.data_ptr(), wb, self.status.data_ptr(),
                                             ctypes.c_void_p(stream)))
            torch.cuda.synchronize()
            assert torch.equal(one, self.out[i]) and bool(one.any()), f"batched canvas of pair {i} differs from its own launch"


# ------------------------------------------------------------------------------------ CPU baseline
_DEFAULT_THREADS_SNIPPET = r"""
import json, sys, time
sys.path.insert(0, {root!r})
import numpy as np
from oracle import apap_oracle as O
from cvx_proj_amd.synth import config_pair
p = config_pair({cfg!r}, with_image=False)
rows, cols = p.vertices.shape[:2]
flat = np.random.default_rng(0).choice(rows * cols, size=min({cells}, rows * cols), replace=False)
done, t0 = 0, time.perf_counter()
for f in flat:
    O.local_homography_loop(p.src, p.dst, p.vertices, p.gamma, p.sigma, cells=[(int(f // cols), int(f % cols))], want_weights=True)
    done += 1
    if time.perf_counter() - t0 > {budget}:
        break
try:
    from threadpoolctl import threadpool_info
    threads = max([i.get("num_threads", 1) for i in threadpool_info()] or [1])
except Exception:
    threads = None
print(json.dumps({{"cells": done, "seconds": time.perf_counter() - t0, "blas_threads": threads}}))
"""


def usable_cores():
    """Cores this process may really use: the affinity mask, cut by the cgroup CPU quota when there
    is one (a container on a 256-thread host is often allowed a fraction of it)."""
    try:
        n = len(os.sched_getaffinity(0))
    except AttributeError:
        n = os.cpu_count() or 1
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()[:2]           # cgroup v2
        if quota != "max":
            n = min(n, max(1, -(-int(quota) // int(period))))
    except (OSError, ValueError):
        try:
            quota = int(open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us").read())           # cgroup v1
            period = int(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
            if quota > 0:
                n = min(n, max(1, -(-quota // period)))
        except (OSError, ValueError):
            pass
    return n


def cpu_baseline(cfg, budget_cells, budget_rows, pool_workers, default_threads_budget_s=8.0):
    """The oracle's faithful-loop port on this host: a bounded, seeded sample of the same workload
    (cells spread over the mesh; every k-th canvas row).  Three rows, SURVEY.md 8(d): one thread (the
    headline of this object), default BLAS threading (a subprocess without the thread pins), all usable
    cores (a process pool over the same cells, one BLAS thread each)."""
    from oracle import apap_oracle as O
    p = config_pair(cfg)
    rows, cols = p.vertices.shape[:2]
    rng = np.random.default_rng(0)
    flat = rng.choice(rows * cols, size=min(budget_cells, rows * cols), replace=False)
    cells = [(int(f // cols), int(f % cols)) for f in flat]
    t0 = time.perf_counter()
    H, _ = O.local_homography_loop(p.src, p.dst, p.vertices, p.gamma, p.sigma, cells=cells, want_weights=True)
    t_solve = time.perf_counter() - t0
    H_full, _ = O.local_homography_fast(p.src, p.dst, p.vertices, p.gamma, p.sigma)
    sub = list(range(0, p.final_h, max(1, p.final_h // budget_rows)))[:budget_rows]
    hinv = H_full.copy()
    t0 = time.perf_counter()
    O.local_warp_loop(p.img, hinv, p.mesh, (p.final_w, p.final_h), (p.off_x, p.off_y), rows_subset=sub)
    t_warp = time.perf_counter() - t0
    # the in-place inversion of all cells is part of local_warp; it is inside t_warp, as in the reference

    default_threads = None
    if default_threads_budget_s > 0:
        env = {k: v for k, v in os.environ.items() if k not in ("OPENBLAS_NUM_THREADS", "OMP_NUM_THREADS", "MKL_NUM_THREADS")}
        code = _DEFAULT_THREADS_SNIPPET.format(root=ROOT, cfg=cfg, cells=min(budget_cells, 4000), budget=default_threads_budget_s)
        try:
            r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True,
                               timeout=default_threads_budget_s * 6 + 120)
            d = json.loads(r.stdout.strip().splitlines()[-1])
            default_threads = {"value": d["cells"] / d["seconds"], "unit": "homographies/s", "cores": d["blas_threads"],
                               "kind": "port",
                               "sample": f"{d['cells']} seeded cells in {d['seconds']:.1f} s, the same loop in a subprocess "
                                         f"with no OPENBLAS/OMP thread limit (what a user of the reference gets by default)"}
        except Exception as e:      # noqa: BLE001  (a baseline row must not take the GPU numbers down with it)
            default_threads = {"error": repr(e)[:200]}

    pool = None
    if pool_workers > 1:
        # "best-effort CPU" row: the same loop over a process pool, 1 BLAS thread each
        try:
            Hp, t_pool = O.local_homography_pool(p.src, p.dst, p.vertices, p.gamma, p.sigma, cells, pool_workers)
            assert np.array_equal(Hp, H)
            pool = {"value": len(cells) / t_pool, "unit": "homographies/s", "cores": pool_workers, "kind": "port",
                    "sample": f"same {len(cells)} cells over a {pool_workers}-process pool (1 BLAS thread each; worker "
                              f"start-up excluded), {t_pool:.2f} s"}
        except Exception as e:      # noqa: BLE001
            pool = {"error": repr(e)[:200]}
    return {
        "value": len(cells) / t_solve, "unit": "homographies/s", "cores": 1, "kind": "port",
        "sample": f"{len(cells)} of {rows * cols} cells (seeded random), {len(sub)} of {p.final_h} canvas rows + all "
                  f"{rows * cols} cell inversions; oracle faithful-loop numpy port, OPENBLAS_NUM_THREADS=1, "
                  f"host has {os.cpu_count()} logical cores, {usable_cores()} usable by this process; two liberties of the port, both "
                  f"in the CPU's favour: the two 3 x 3 inverses the reference recomputes in every cell (apap.py:164-165) are taken "
                  f"once per pair, and point_normalize / matrix_generate (apap.py:92-119, Python loops over the keypoints in the "
                  f"reference) are vectorised",
        "warp_value": len(sub) * p.final_w / t_warp / 1e6, "warp_unit": "Mpix/s",
        "solve_s": t_solve, "warp_s": t_warp,
        "default_blas_threads": default_threads,
        "all_cores": pool,
    }


# --------------------------------------------------------------------------------------- call level
def call_level(cfg, reps=7):
    """numpy in -> numpy out through the host-buffer entry points (what a caller of the reference's
    class sees): host set-up (a2-a5 + table), H2D, kernels, D2H and the synchronisation included."""
    p = config_pair(cfg)

    def med(f, n):
        ts = []
        for _ in range(n):
            t0 = time.perf_counter()
            f()
            ts.append(time.perf_counter() - t0)
        return sorted(ts)[len(ts) // 2]

    H, _ = N.local_homography(p.src, p.dst, p.vertices, p.gamma, p.sigma, want_weights=False)     # warm-up: pool allocation
    cells = H.shape[0] * H.shape[1]
    t_h = med(lambda: N.local_homography(p.src, p.dst, p.vertices, p.gamma, p.sigma, want_weights=False), reps)
    N.local_warp(p.img, H, p.mesh[0], p.mesh[1], p.final_w, p.final_h, p.off_x, p.off_y)
    t_w = med(lambda: N.local_warp(p.img, H, p.mesh[0], p.mesh[1], p.final_w, p.final_h, p.off_x, p.off_y), max(reps - 2, 3))
    t_hw = med(lambda: N.local_homography(p.src, p.dst, p.vertices, p.gamma, p.sigma, want_weights=True), 3)
    # the reference's own signature through the mirror class: (H, W) with W computed when looked at
    from cvx_proj_amd.apap import APAP
    eng = APAP(p.gamma, p.sigma, [p.final_w, p.final_h], [p.off_x, p.off_y])
    t_def = med(lambda: eng.local_homography(p.src, p.dst, p.vertices), reps)
    _, W = eng.local_homography(p.src, p.dst, p.vertices)
    t_cell = med(lambda: W[cells // (2 * H.shape[1]), 7], 5)
    ovl = N.Context(overlap_pcie=1)
    N.local_warp(p.img, H, p.mesh[0], p.mesh[1], p.final_w, p.final_h, p.off_x, p.off_y, ctx=ovl)      # first use of the buffers: pinning
    t_w_ovl = med(lambda: N.local_warp(p.img, H, p.mesh[0], p.mesh[1], p.final_w, p.final_h, p.off_x, p.off_y, ctx=ovl), 5)
    ovl.close()
    return {"workload": cfg, "local_homography_ms": t_h * 1e3, "homographies_per_s": cells / t_h,
            "local_warp_ms": t_w * 1e3, "warp_mpix_per_s": p.final_w * p.final_h / t_w / 1e6,
            "local_warp_overlapped_ms": t_w_ovl * 1e3,
            "local_homography_default_signature_ms": t_def * 1e3, "default_signature_homographies_per_s": cells / t_def,
            "lazy_weights_one_cell_ms": t_cell * 1e3,
            "local_homography_with_weights_ms": t_hw * 1e3, "weights_bytes": cells * len(p.src) * 8,
            "note": "median wall time of apap_local_homography / apap_local_warp called with host (numpy) buffers: "
                    "host set-up, H2D/D2H over PCIe and the final synchronisation are inside; never `value`.  "
                    "local_warp_overlapped_ms: APAP_OPT_OVERLAP_PCIE = 1 (buffers pinned for the call; upload, banded warp and download "
                    "on three streams) in steady state - the first use of a buffer costs ~8 ms, hence opt-in; default_signature = APAP.local_homography(src, dst, vertices) of the mirror "
                    "class, whose second return value is computed when looked at (lazy_weights_one_cell_ms: W[i, j]); "
                    "with_weights = the eager 640 MB tensor"}


def pipeline_level(cfg, reps=5):
    """apap.py __main__ between loading and saving (apap.py:238-264), numpy in -> the `.mat` array (and the canvas)
    out: the resident pass of cvx_proj_amd.pipeline against the chain of calls of the mirror class."""
    from cvx_proj_amd import apap as A
    from cvx_proj_amd.pipeline import Pipeline
    p = config_pair(cfg)
    m = p.vertices.shape[0]
    pipe = Pipeline()

    def med(f, n):
        ts = []
        for _ in range(n):
            t0 = time.perf_counter()
            f()
            ts.append(time.perf_counter() - t0)
        return sorted(ts)[len(ts) // 2]

    args = (p.src, p.dst, p.Hg, p.shape, p.shape, m, p.gamma, p.sigma)
    import contextlib
    import io
    with contextlib.redirect_stdout(io.StringIO()):          # the mirror class prints the reference's progress lines
        pipe.run_pair(*args, other_img=p.img)                # warm-up: buffers
        A.run_pair_by_calls(*args, other_img=p.img)
        t_solve = med(lambda: pipe.run_pair(*args), reps)
        tl_solve = dict(pipe.timeline)
        t_warp = med(lambda: pipe.run_pair(*args, other_img=p.img), reps)
        tl_warp = dict(pipe.timeline)
        c_solve = med(lambda: A.run_pair_by_calls(*args), reps)
        c_warp = med(lambda: A.run_pair_by_calls(*args, other_img=p.img), max(reps - 2, 3))
        # a caller that reads its images into page-locked arrays of the pipeline's and takes the canvas in one
        pin_img = pipe.pinned_array(p.img.shape)
        np.copyto(pin_img, p.img)
        pin_out = pipe.pinned_array((p.final_h, p.final_w, 3))
        flat_a, canvas_a = pipe.run_pair(*args, other_img=p.img)
        flat_b, canvas_b = pipe.run_pair(*args, other_img=pin_img, canvas_out=pin_out)
        assert np.array_equal(flat_a, flat_b) and np.array_equal(canvas_a, canvas_b)
        t_pinned = med(lambda: pipe.run_pair(*args, other_img=pin_img, canvas_out=pin_out), max(reps, 9))
        pipe.trace = True
        pipe.run_pair(*args, other_img=pin_img, canvas_out=pin_out)
        marks = {k: round(v, 1) for k, v in pipe.device_marks}
        pipe.trace = False
    return {"workload": cfg, "solve_to_mat_array_ms": t_solve * 1e3, "solve_warp_to_mat_array_and_canvas_ms": t_warp * 1e3,
            "chain_of_calls_solve_ms": c_solve * 1e3, "chain_of_calls_solve_warp_ms": c_warp * 1e3,
            "solve_warp_with_page_locked_image_and_canvas_ms": t_pinned * 1e3,
            "page_locked_pass_device_marks_us": marks,
            "timeline_solve": tl_solve, "timeline_solve_warp": tl_warp,
            "note": "numpy in -> numpy out, everything between resident in HBM on one stream, one trip back "
                    "(cvx_proj_amd/pipeline.py); chain_of_calls = the mirror class call by call as apap.py:238-264 is written "
                    "(local_homography, local_warp with its own copy of the grid, invert_normalize_flatten); with the warp both "
                    "are bound by 25 MB up + 27 MB down over PCIe from pageable numpy arrays; with_page_locked = the same pass when the "
                    "caller keeps its image and canvas in Pipeline.pinned_array() buffers (every copy of the pass page-locked and asynchronous: "
                    "the image upload runs beside the host set-up, the small uploads and the solve; device_marks = HIP events at the "
                    "stage boundaries of one such pass, microseconds from its first enqueue); never `value`"}


def cli_level(cfg="C1", reps=3):
    """Wall time of the drop-in command in a FRESH process (python -m cvx_proj_amd.apap 1 1 --synth C1: interpreter, numpy, the HIP
    runtime coming up, the first launch with its code-object load, one pair, savemat) - what the reference's one-process-per-pair
    driver (run_all.sh) pays per pair - and of 16 pairs in one process (--cases 1-4 --imgs 1,2,4,5).  Children of this process
    (never exec)."""
    import tempfile

    def run(args):
        with tempfile.TemporaryDirectory() as tmp:
            cmd = [sys.executable, "-m", "cvx_proj_amd.apap"] + args + ["--out-prefix", tmp + "/", "--timing"]
            t0 = time.perf_counter()
            r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
            wall = time.perf_counter() - t0
        if r.returncode != 0:
            raise RuntimeError(r.stderr[-500:])
        return wall, json.loads([ln for ln in r.stderr.splitlines() if ln.startswith("{")][-1])
    try:
        one = min((run(["1", "1", "--synth", cfg]) for _ in range(reps)), key=lambda x: x[0])
        loop = min((run(["--cases", "1-4", "--imgs", "1,2,4,5", "--synth", cfg]) for _ in range(reps)), key=lambda x: x[0])
    except Exception as e:      # noqa: BLE001  (never take the GPU numbers down)
        return {"error": repr(e)[:300]}
    st = one[1]
    return {"workload": f"{cfg}, fresh process: python -m cvx_proj_amd.apap 1 1 --synth {cfg}", "wall_ms": one[0] * 1e3,
            "interpreter_and_numpy_ms": one[0] * 1e3 - st["total_ms"], "runtime_init_ms": st["runtime_init_ms"],
            "first_pair_compute_ms": st["pairs"][0]["compute_ms"], "savemat_ms": st["pairs"][0]["save_ms"],
            "sixteen_pairs_one_process_wall_ms": loop[0] * 1e3, "later_pair_compute_ms": loop[1]["pairs"][-1]["compute_ms"],
            "note": "min of %d fresh processes; no torch in them (rounds 1-5 imported it: 1.39 s, profiles/r06_cli.txt).  Not part "
                    "of `value`" % reps}


# ------------------------------------------------------------------------------------ self-launch
def free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def self_launch(gpus):
    """Start the ranks as a CHILD process tree (never exec: this parent has not touched the GPU and
    must not be replaced once anything has) and return its exit code."""
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(free_port()), os.path.abspath(__file__)] + sys.argv[1:]
    return subprocess.call(cmd)


def selftest(rank, world):
    """APAP_BENCH_SELFTEST=1: exercise the launch + rendezvous + one collective without a GPU (the
    CPU test of the self-launch path): every rank contributes rank + 1, rank 0 prints the sum."""
    import torch.distributed as dist
    dist.init_process_group("gloo")
    t = torch.tensor([float(rank + 1)])
    dist.all_reduce(t)
    if rank == 0:
        print(json.dumps({"selftest": True, "n_gpus": world, "sum": float(t[0]),
                          "ranks_env": [os.environ.get(k) for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR")]}), flush=True)
    dist.barrier()
    dist.destroy_process_group()


# --------------------------------------------------------------------------------------------- main
DUMP_CANVAS_SAMPLES = 1 << 21       # canvas bytes kept by --dump-outputs: 8 MB of float32 values + 16 MB of float64 indices


def dump_outputs(out_dir, res):
    """--dump-outputs: the outputs of the timed path's last step (rank 0), copied back after the timed regions.
    ``H.npy``: the float32 homography grid, (batch, rows, cols, 3, 3), whole.  ``canvas_sample.npy``: the warped uint8
    canvas as float32 at a fixed, seeded sample of its flat positions (the whole canvas in float32 would be ~108 MB at C3),
    ``canvas_sample_index.npy``: those positions (float64, sorted)."""
    os.makedirs(out_dir, exist_ok=True)
    H = res.H.cpu().numpy().reshape(res.batch, res.rows, res.cols, 3, 3).astype(np.float32)
    canvas = res.out.cpu().numpy().reshape(-1)
    idx = np.sort(np.random.default_rng(0).choice(canvas.size, size=min(DUMP_CANVAS_SAMPLES, canvas.size), replace=False))
    np.save(os.path.join(out_dir, "H.npy"), H)
    np.save(os.path.join(out_dir, "canvas_sample.npy"), canvas[idx].astype(np.float32))
    np.save(os.path.join(out_dir, "canvas_sample_index.npy"), idx.astype(np.float64))


def roofline_k2(config, res, kern, kern_plain, tj, fused):
    """K2 (k_eigen_denorm) against HBM: counter bytes per launch (profiles/pmc_traffic.json: 2 x FETCH_SIZE - its reads are
    16 bytes per lane, the case the guide's correction doubles - + WRITE_SIZE) and the bytes the algorithm needs, over the
    kernel's own duration, for the stand-alone solve's K2 and for the resident step's (whose tail also writes every cell's
    inverse and float32-estimate record for the warp)."""
    if fused or not kern.get("eigen"):
        return None
    cells = res.cells * res.batch
    splits = N.lib().apap_solve_workspace_bytes(res.ctx, res.n, res.cells) // (30 * 8 * ((res.cells + 63) // 64 * 64))
    # reads: the moment slabs (30 doubles per cell and keypoint split) + 2 vertices doubles; writes: 9 floats
    algo_plain = cells * (splits * 240 + 16 + 36)
    # the tail: + 2 x 2 edge doubles read, + 10 doubles of padded inverse and a 48-byte record written
    algo_ready = algo_plain + cells * (32 + 80 + 48)
    out = {"kernel": "k_eigen_denorm", "bound": "latency", "priced_against": "hbm", "peak": PEAK_HBM_GBS, "unit": "GB/s",
           "keypoint_splits": int(splits),
           "note": "one wave per SIMD walking a ~900-instruction dependent chain per cell: bound by that chain's latency, not by bytes "
                   "or flops - the fraction (bytes over the kernel's time against HBM) says how little of the HBM a launch of 625 waves "
                   "can ask for.  A single slab (no keypoint splits: K2 reads "
                   "half) was measured: K2 -0.7 us, K1 +32 us (625 blocks on 256 CUs), profiles/r05_summary.txt"}
    for tag, ms, algo in (("plain", kern_plain.get("eigen"), algo_plain), ("warp_ready", kern.get("eigen"), algo_ready)):
        if not ms:
            continue
        counter = tj.get(f"{config}:k_eigen_denorm:{tag}")
        out[tag] = {"kernel_ms": ms, "timing": "a pair of HIP events per launch (+ ~2 us of event handling)",
                    "algorithmic_bytes": int(algo), "achieved": algo / (ms * 1e-3) / 1e9, "frac": algo / (ms * 1e-3) / 1e9 / PEAK_HBM_GBS,
                    "traffic": counter, "traffic_gbs": None if counter is None else counter / (ms * 1e-3) / 1e9}
    return out


def small_config(cfg, dev, stream, steps, timed, condition, back_to_back):
    """One of BASELINE's other single-GPU configurations (C1, C2) on the same definitions as the headline: the resident step
    (solve with the warp-ready tail, gather-only warp), exactly `steps` steps each, kernel times by HIP events."""
    ctx = N.Context()
    pair = config_pair(cfg)
    res = Resident(pair, dev, ctx=ctx)
    condition(lambda: res.solve(stream))
    for _ in range(5):
        res.solve(stream)
        res.warp(stream)
    t_solve = timed(lambda: res.solve(stream), steps)
    t_warp = timed(lambda: res.warp(stream), steps)
    assert int(res.status.cpu()[0]) == 0
    ctx.set("profile", 1)
    for _ in range(steps):
        res.solve(stream)
        res.warp(stream)
    torch.cuda.synchronize()
    kern = read_kernel_ms(ctx)
    ctx.set("profile", 0)
    k1_ms = back_to_back(lambda: res.solve(stream), max(steps, 50))      # the solve's launches back to back (K1 + K2, or the fused one)
    k3_ms = back_to_back(lambda: res.warp(stream), max(steps, 50))
    fused = res.cells <= ctx.get("fused_max_cells")
    flops = K1_FLOPS_PER_CELL_POINT * res.n * res.cells
    nz = int((res.out.view(-1, 3).amax(dim=1) > 0).sum().cpu())
    wbytes = 6 * nz + 3 * (pair.final_w * pair.final_h - nz)
    out = {"workload": f"{cfg}: {CONFIGS[cfg][0]}x{CONFIGS[cfg][1]} pair, {res.n} correspondences, {res.rows}x{res.cols} mesh, canvas "
                       f"{pair.final_w}x{pair.final_h}",
           "value": res.cells * steps / t_solve, "unit": "homographies/s", "solve_ms_per_step": t_solve / steps * 1e3,
           "warp": {"value": pair.final_w * pair.final_h * steps / t_warp / 1e6, "unit": "Mpix/s", "ms_per_step": t_warp / steps * 1e3},
           "solve_launch": "k_solve_small (K1 + K2 fused, one launch)" if fused else "k_assemble_mfma + k_eigen_denorm",
           "kernels_ms": {k: kern.get(k) for k in ("assemble", "eigen", "warp")},
           "solve_ms_back_to_back": k1_ms, "warp_ms_back_to_back": k3_ms,
           "roofline": {"kernel": "k_solve_small (the K2 tail is inside the time, only K1's flops are counted)" if fused else "k_assemble_mfma",
                        "bound": "latency" if fused else "mfma", "priced_against": "mfma", "achieved": flops / (kern["assemble"] * 1e-3) / 1e12,
                        "peak": PEAK_FP64_TFLOPS, "unit": "TFLOP/s", "frac": flops / (kern["assemble"] * 1e-3) / 1e12 / PEAK_FP64_TFLOPS},
           "roofline_warp": {"kernel": "k_warp_fast", "cache": "warm", "bound": "hbm", "achieved": wbytes / (k3_ms * 1e-3) / 1e9,
                             "peak": PEAK_HBM_GBS, "unit": "GB/s", "frac": wbytes / (k3_ms * 1e-3) / 1e9 / PEAK_HBM_GBS, "kernel_ms": k3_ms},
           "note": "small launches: a few microseconds of kernel behind ~4-5 us of launch, first table trips and last stores - the "
                   "fractions say how much of the chip one such launch can use, not how good the kernel is at size (C3, C4 and the "
                   "batched C5 are the same kernels at size)"}
    del res
    ctx.close()
    return out


def opt_in_modes(cfg, pair, dev, stream, steps, timed, condition, H_default, k1_default_ms):
    """The opt-in forms of the solve (APAP_OPT_MOMENTS = 24, alone and with APAP_OPT_WEIGHTS_F32) beside the default, same
    configuration and step definition (the resident step's solve).  NOT bit-identical (tests/test_gpu_moments24.py): the object
    says by how much.  `value` of the line stays the default's."""
    def rmse_delta(Ha, Hb, pts):
        """north_star's measure: per cell, the RMS over keypoints of |proj(Ha, p) - proj(Hb, p)| (pixels)."""
        q = np.concatenate([pts.astype(np.float64), np.ones((len(pts), 1))], axis=1)
        pa, pb = (np.einsum("rcij,kj->rcki", H.astype(np.float64), q) for H in (Ha, Hb))
        pa, pb = pa[..., :2] / pa[..., 2:3], pb[..., :2] / pb[..., 2:3]
        return np.sqrt(((pa - pb) ** 2).sum(axis=-1).mean(axis=-1))
    out = {"note": "24 sums of the exact products instead of the 30 that keep apap.py:103-119's float32-rounded products: one "
                   "v_mfma_f64_16x16x4_f64 + two v_mfma_f64_4x4x4_4b_f64 per 4-keypoint step instead of two 16x16x4 (VERDICT r5 item "
                   "1: predicted K1 149 -> ~131 us, value +10-13 %; measured 150.7 -> 135.3 us, +11 %); f32_weights = the same with w^2 "
                   "evaluated in float32.  Opt-in and OUTSIDE north_star's bar at this size: the grids differ from the reference's by at "
                   "most one float32 ulp in ~0.3 % of their entries, and one ulp of H[0,0] ~ 1 moves a keypoint at x = 3840 by 4.6e-4 px "
                   "(vs_default_grid.rmse_delta_max_px) - at 4K the 1e-4 px bar is a demand for the reference's float32 bits, which only "
                   "the default meets.  The headline `value` is the bit-identical default", "k1_default_ms": k1_default_ms}
    for tag, opts in (("fp64_weights", {"moments": 24}), ("f32_weights", {"moments": 24, "weights_f32": 1})):
        ctx = N.Context(**opts)
        res = Resident(pair, dev, ctx=ctx)
        condition(lambda: res.solve(stream))
        for _ in range(5):
            res.solve(stream)
        t = timed(lambda: res.solve(stream), steps)
        ctx.set("profile", 1)
        for _ in range(steps):
            res.solve(stream)
        torch.cuda.synchronize()
        kern = read_kernel_ms(ctx)
        ctx.set("profile", 0)
        H = res.H.cpu().numpy().reshape(res.rows, res.cols, 3, 3)
        d = rmse_delta(H[::8], H_default[::8], pair.src[:128])
        a32, b32 = H.view(np.int32).astype(np.int64), H_default.view(np.int32).astype(np.int64)
        flops = K1_FLOPS_PER_CELL_POINT * res.n * res.cells
        out[tag] = {"value": res.cells * steps / t, "unit": "homographies/s", "solve_ms_per_step": t / steps * 1e3,
                    "kernels_ms": {k: kern.get(k) for k in ("assemble", "eigen")},
                    "k1_vs_default": kern["assemble"] / k1_default_ms,
                    "roofline": {"kernel": "k_assemble_mfma<24 sums>", "bound": "mfma", "achieved": flops / (kern["assemble"] * 1e-3) / 1e12,
                                 "peak": PEAK_FP64_TFLOPS, "unit": "TFLOP/s", "frac": flops / (kern["assemble"] * 1e-3) / 1e12 / PEAK_FP64_TFLOPS,
                                 "note": "the same algorithmic 58 flops per (cell, keypoint) as the default's roofline"},
                    "vs_default_grid": {"float32_values_differing": int((H != H_default).sum()), "of": int(H.size),
                                        "max_ulp": int(np.abs(a32 - b32).max()), "rmse_delta_max_px": float(d.max()),
                                        "rmse_delta_rows": "every 8th mesh row, 128 keypoints"}}
        out[tag]["vs_default_grid"]["within_north_star_bar"] = bool(np.isfinite(H).all() and d.max() < 1e-4)
        del res
        ctx.close()
    return out


def read_kernel_ms(ctx):
    """Average milliseconds per launch of every kernel slot the context bracketed since the last read."""
    prof = ctx.profile_read()
    return {k: (ms / max(cnt, 1)) for i, (k, (ms, cnt)) in enumerate(prof.items()) if cnt or i < 5}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--condition-ms", type=float, default=250.0,
                    help="untimed load before each timed region so that it runs at the sustained clock (0 = off)")
    ap.add_argument("--config", default="C3", choices=sorted(CONFIGS))
    ap.add_argument("--cells-config", default="C4", choices=sorted(CONFIGS),
                    help="the ONE pair whose mesh rows are sharded over the ranks in the `cells` object")
    ap.add_argument("--variant", default="auto", choices=sorted(VARIANTS))
    ap.add_argument("--full", action="store_true",
                    help="after the headline, measure and check everything else (kernel times, rooflines, other configurations, "
                         "pairs, cells, call level, CPU baseline) and add it to the line; the --no-* switches leave parts of it out")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-cells", action="store_true", help="skip the `cells` (strong-scaling) object")
    ap.add_argument("--no-call-level", action="store_true")
    ap.add_argument("--no-configs", action="store_true", help="skip the `configs` (C1, C2) and `moments24` objects")
    ap.add_argument("--no-c5", action="store_true", help="skip the `pairs` object (BASELINE config 5: 64 pairs over the ranks)")
    ap.add_argument("--c5-pairs", type=int, default=64)
    ap.add_argument("--c5-chunks", type=int, default=4, help="groups the rank's pairs are split into for the overlapped whole job")
    ap.add_argument("--batch", type=int, default=1,
                    help="solve this many independent pairs per step in ONE batched launch (config C5 style); "
                         "the warp half then runs once per pair")
    ap.add_argument("--graph", action="store_true",
                    help="capture the solve and the warp step into HIP graphs and time graph replays")
    ap.add_argument("--want-waves", type=int, help="tuning: APAP_OPT_WANT_WAVES of the context (K1 keypoint splits)")
    ap.add_argument("--warp-rows", type=int, choices=[0, 1, 2, 4, 5, 6, 8], help="APAP_OPT_WARP_ROWS (1 = chosen from the size of the launch: the default; 0 = flat-order warp kernel)")
    ap.add_argument("--warp-fast", type=int, choices=[0, 1], help="tuning: APAP_OPT_WARP_FAST (0 = float64 for every pixel of K3)")
    ap.add_argument("--fused-max-cells", type=int, help="tuning: APAP_OPT_FUSED_MAX_CELLS (fused K1 + K2 launch for small meshes)")
    ap.add_argument("--cold-mb", type=float, default=640.0,
                    help="cold-cache warp leg: rotate over this many MB of (image, canvas) copies (0 = skip)")
    ap.add_argument("--cpu-cells", type=int, default=40000)
    ap.add_argument("--cpu-rows", type=int, default=400)
    ap.add_argument("--cpu-pool", type=int, default=-1,
                    help="workers of the all-cores CPU row (-1 = every core this process may use, 0 = skip)")
    ap.add_argument("--dump-outputs", metavar="DIR",
                    help="write the outputs of the last timed step (H grid, canvas sample) to DIR/*.npy (rank 0)")
    a = ap.parse_args()
    if a.steps < 1:
        ap.error("--steps must be at least 1")
    # --steps is the number of timed steps of the headline (`value`, `ms_per_step`); every other timed region of a --full run
    # (extras, configs, pairs, cells, kernel times) takes at most EXTRA_STEPS steps, so that the run's length follows the headline's
    xs = min(a.steps, EXTRA_STEPS)

    if "WORLD_SIZE" not in os.environ and a.gpus > 1:
        sys.exit(self_launch(a.gpus))       # nothing above this line touches the GPU
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    a.gpus = world
    if os.environ.get("APAP_BENCH_SELFTEST") == "1":
        return selftest(rank, world)
    # one rank per GPU; if a rehearsal runs more ranks than GPUs (e.g. 2 gloo ranks on a 1-GPU
    # box, APAP_BENCH_BACKEND=gloo) the ranks share devices round-robin
    dev_index = local_rank % max(torch.cuda.device_count(), 1)
    torch.cuda.set_device(dev_index)
    dev = torch.device("cuda", dev_index)
    backend = None
    # APAP_BENCH_FORCE_GROUP=1: a process group (and every collective of the multi-rank code paths) also with ONE rank - first contact
    # with RCCL's initialisation and collectives on a one-GPU box (RANK / WORLD_SIZE / MASTER_ADDR / MASTER_PORT from the environment)
    if world > 1 or os.environ.get("APAP_BENCH_FORCE_GROUP") == "1":
        import torch.distributed as dist
        if world == 1:
            import cvx_proj_amd.dist as _D
            _D.REHEARSE_ONE_RANK = True     # the one rank runs the broadcasts and all-gathers of `cells` instead of the single-process shortcuts
        backend = os.environ.get("APAP_BENCH_BACKEND", "nccl")      # nccl = RCCL on ROCm
        # first contact with RCCL must not hang silently: a short collective timeout (the default is 10 minutes, the
        # driver's limit for the whole run is not much more) and a phase marker on stderr before every phase that
        # holds a collective, so that a run killed at its limit has said where it was
        import datetime
        tmo = datetime.timedelta(seconds=float(os.environ.get("APAP_BENCH_COLLECTIVE_TIMEOUT_S", "120")))
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=dev, timeout=tmo)
        else:
            dist.init_process_group(backend, timeout=tmo)
    else:
        dist = None

    def phase(name):
        if rank == 0:
            print(json.dumps({"bench_phase": name, "n_gpus": world, "backend": backend, "t": round(time.time() - T0, 2)}),
                  file=sys.stderr, flush=True)

    def finish(line):
        if rank == 0:
            print(json.dumps(line), flush=True)
        if dist is not None:
            dist.barrier()
            dist.destroy_process_group()

    phase("process group up")
    if dist is not None:
        # one tiny collective first: if the transport is broken this fails within the timeout, before any long phase
        probe = torch.ones(1, device=dev)
        dist.all_reduce(probe)
        torch.cuda.synchronize()
        assert int(probe.cpu()[0]) == world, "all_reduce across the ranks returned a wrong sum"
        phase("first collective done")

    ctx = N.Context(variant=VARIANTS[a.variant])        # options + profiling live in a context, not in the process
    if a.want_waves:
        ctx.set("want_waves", a.want_waves)
    if a.warp_rows is not None:
        ctx.set("warp_rows", a.warp_rows)
    if a.fused_max_cells is not None:
        ctx.set("fused_max_cells", a.fused_max_cells)
    if a.warp_fast is not None:
        ctx.set("warp_fast", a.warp_fast)
    stream = torch.cuda.current_stream().cuda_stream

    def barrier():
        if dist is not None:
            torch.cuda.synchronize()
            dist.barrier()
        torch.cuda.synchronize()

    def timed(fn, steps):
        """EXACTLY `steps` calls between two barrier + synchronise brackets; max over ranks."""
        barrier()
        t0 = time.perf_counter()
        for _ in range(steps):
            fn()
        barrier()
        t = time.perf_counter() - t0
        if dist is not None:
            tt = torch.tensor([t], dtype=torch.float64, device=dev)
            dist.all_reduce(tt, op=dist.ReduceOp.MAX)
            t = float(tt.cpu()[0])
        return t

    def condition(fn):
        """Untimed: keep the GPU busy with `fn` for --condition-ms before a timed region.  The chip raises its
        clocks only under sustained load: from idle, the first ~100 solve steps (~20 ms) run 5-10 % slower than
        the steady state (C3: K1 159-166 us in the first 50 steps, 150.6 us from step ~150 on; C1: 9-10 us per
        solve over 30 launches, 7.8 us over 1000).  W warm-up steps of a few hundred microseconds each do not
        get there; this does, and exactly K steps are timed after it, as before."""
        if a.condition_ms <= 0:
            return
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < a.condition_ms * 1e-3:
            for _ in range(20):
                fn()
            torch.cuda.synchronize()

    # ------------------------------------------------------------------ pairs: the headline
    phase("pair_per_rank (no data-path collective; barriers only)")
    pair = config_pair(a.config, seed_offset=rank * a.batch)
    extras = [config_pair(a.config, with_image=False, seed_offset=rank * a.batch + k) for k in range(1, a.batch)]
    res = Resident(pair, dev, a.batch, extras, ctx=ctx)
    units_solve = res.cells * a.batch * world
    units_warp = pair.final_w * pair.final_h * world

    condition(lambda: res.solve(stream))
    for _ in range(a.warmup):
        res.solve(stream)
        res.warp(stream)
    run_solve, run_warp = (lambda: res.solve(stream)), (lambda: res.warp(stream))
    if a.graph:
        # the entry points only enqueue kernels (no allocation, no synchronisation), so a step
        # can be captured once and replayed: one host call per step instead of one per kernel
        torch.cuda.synchronize()
        g_solve, g_warp = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
        with torch.cuda.graph(g_solve):
            res.solve(torch.cuda.current_stream().cuda_stream)
        with torch.cuda.graph(g_warp):
            res.warp(torch.cuda.current_stream().cuda_stream)
        run_solve, run_warp = g_solve.replay, g_warp.replay
        run_solve()
        run_warp()
    t_solve = timed(run_solve, a.steps)
    t_warp = timed(run_warp, a.steps)
    assert int(res.status.cpu()[0]) == 0, "device status word set during the timed region"
    if a.dump_outputs and rank == 0:
        dump_outputs(a.dump_outputs, res)
    line = None
    if rank == 0:
        line = {
            "metric": METRIC, "value": units_solve * a.steps / t_solve, "unit": "homographies/s",
            "n_gpus": world, "steps": a.steps, "warmup": a.warmup, "conditioning_ms": a.condition_ms,
            "ms_per_step": (t_solve + t_warp) / a.steps * 1e3, "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": "f64", "data": "synthetic",
            "config": {"workload": f"{a.config}: {CONFIGS[a.config][0]}x{CONFIGS[a.config][1]} pair, "
                                   f"{res.n} correspondences, {res.rows}x{res.cols} mesh, canvas "
                                   f"{pair.final_w}x{pair.final_h}", "mode": "pairs", "variant": a.variant,
                       "pairs_per_solve_launch": a.batch,
                       "launch": "hip graph replay" if a.graph else "eager",
                       "parallelism": f"pairsx{world}"},
            "warp": {"value": units_warp * a.steps / t_warp / 1e6, "unit": "Mpix/s",
                     "ms_per_step": t_warp / a.steps * 1e3},
            "solve_ms_per_step": t_solve / a.steps * 1e3,
            "step_form": ("resident pipeline: canvas row / column tables built once per geometry, the eigen-solve kernel's tail leaves "
                          "every cell warp ready (apap_solve_warp_batch_device), the warp step is the gather kernel alone "
                          "(apap_warp_batch_device, APAP_WARP_GATHER); the per-cell set-up is inside solve_ms_per_step") if res.resident
                         else "solve and stand-alone warp (a batch of pairs per solve launch)",
            "pair_per_rank": {"workload": f"{a.config} x {world} (one pair per rank)", "world_size": world, "scaling": "weak",
                              "value": units_solve * a.steps / t_solve, "unit": "homographies/s",
                              "solve_ms_per_step": t_solve / a.steps * 1e3,
                              "warp": {"value": units_warp * a.steps / t_warp / 1e6, "unit": "Mpix/s",
                                       "ms_per_step": t_warp / a.steps * 1e3},
                              "collectives_per_step": "none (independent pairs)"},
        }
    if not a.full:
        finish(line)
        return

    # ------------------------------------------------------------------ --full: everything else, added to the same line
    canvas_resident = res.out.clone()
    # the same two halves as separate services: the solve alone, and the warp of a grid from anywhere (its own set-up launch)
    for _ in range(a.warmup):
        res.solve_plain(stream)
        res.warp_standalone(stream)
    t_solve_plain = timed(lambda: res.solve_plain(stream), xs)
    t_warp_alone = timed(lambda: res.warp_standalone(stream), xs)
    assert torch.equal(res.out, canvas_resident), "stand-alone warp and resident warp step disagree"
    del canvas_resident
    res.solve(stream)       # leave the resident tables in place for what follows

    def extra(fn):      # rank-local extras, not part of `value`
        fn(stream)
        condition(lambda: fn(stream))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(xs):
            fn(stream)
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    # the warp again with cold caches: rotate over >= 640 MB of (image, canvas) copies
    cold = res.cold_sets(a.cold_mb * 1e6) if a.cold_mb > 0 else None
    t_warp_cold = None
    if cold:
        turn = [0]

        def warp_cold():
            i, o = cold[turn[0] % len(cold)]
            turn[0] += 1
            res.warp(stream, i, o)
        for _ in range(len(cold)):
            warp_cold()
        t_warp_cold = timed(warp_cold, xs)
        assert torch.equal(cold[0][1], res.out), "cold-cache canvas differs from the warm one"

    # two warps of the pair in flight at once (two streams, two canvases): the set-up kernel, the ramp and the tail of one
    # run under the gather kernel of the other
    res.second_lane()
    torch.cuda.synchronize()

    def warp_pair_of_lanes():
        res.warp_standalone(stream)
        res.warp_lane2()
    for _ in range(a.warmup):
        warp_pair_of_lanes()
    t_warp2 = timed(warp_pair_of_lanes, xs)
    assert torch.equal(res.second_lane()[0], res.out), "second lane's canvas differs"

    t_stitch = extra(res.stitch)
    res.warp(stream)            # leave the plain warped canvas in res.out for the byte count below
    torch.cuda.synchronize()
    t_eq = extra(res.equalize)
    t_ransac = extra(res.ransac)

    # per-kernel durations, HIP events on the launch stream (rank-local)
    condition(lambda: res.solve(stream))
    ctx.set("profile", 1)
    for _ in range(xs):
        res.solve(stream)
        res.warp(stream)
        res.equalize(stream)
        res.ransac(stream)
    torch.cuda.synchronize()
    kern = read_kernel_ms(ctx)
    for _ in range(xs):                 # the set-up launch of the stand-alone warp (the resident step has none)
        res.warp_standalone(stream)
    torch.cuda.synchronize()
    kern["invert"] = read_kernel_ms(ctx)["invert"]
    for _ in range(xs):                 # K2 without the warp-ready tail (the stand-alone solve)
        res.solve_plain(stream)
    torch.cuda.synchronize()
    kern_plain = read_kernel_ms(ctx)
    res.solve(stream)
    kern_cold = None
    if cold:
        for _ in range(max(xs, len(cold))):
            warp_cold()
        torch.cuda.synchronize()
        kern_cold = read_kernel_ms(ctx)
    ctx.set("profile", 0)

    def back_to_back(fn, n):
        """Average duration of n launches of one kernel issued back to back, between two HIP events on the launch stream: the
        kernel's duration plus the ~1 us gap between dependent launches - what rocprofv3's per-kernel average agrees with.  (A
        pair of events around EVERY launch, the context's profiling slots, adds ~2 us of event handling to each launch: 13 % of a
        15 us kernel, nothing next to K1's 150 us.)"""
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / n
    condition(lambda: res.warp(stream))
    k3_warm_ms = back_to_back(lambda: res.warp(stream), max(xs, 20))
    k3_cold_ms = None
    if cold:
        for _ in range(len(cold)):
            warp_cold()
        k3_cold_ms = back_to_back(warp_cold, max(xs, len(cold)))

    # a caller's FIRST solve from an idle chip (clocks down): one call, bracketed by synchronisation
    from_idle = []
    for _ in range(3):
        torch.cuda.synchronize()
        time.sleep(0.4)
        t0 = time.perf_counter()
        res.solve(stream)
        torch.cuda.synchronize()
        from_idle.append(time.perf_counter() - t0)
    t_idle = sorted(from_idle)[1]

    # ------------------------------------------------------------------ BASELINE's other 1-GPU configurations, the opt-in solve forms
    configs_obj = modes_obj = None
    if world == 1 and not a.no_configs:
        phase("configs C1, C2; opt-in solve forms")
        configs_obj = {c: small_config(c, dev, stream, xs, timed, condition, back_to_back) for c in ("C1", "C2") if c != a.config}
        if a.batch == 1 and a.variant == "auto":
            H_default = res.H.cpu().numpy().reshape(res.rows, res.cols, 3, 3)
            modes_obj = opt_in_modes(a.config, pair, dev, stream, xs, timed, condition, H_default, kern["assemble"])

    # ------------------------------------------------------------------ pairs as BASELINE config 5 states them
    c5_obj = None
    if not a.no_c5:
        phase("pairs (config 5; no data-path collective)")
        total_pairs = a.c5_pairs
        mine = list(range(rank, total_pairs, world))          # dealt round-robin: 64 / N per rank
        pb = PairBatch("C5", mine, dev, ctx=ctx) if mine else None
        if pb is not None:
            condition(lambda: pb.solve(stream))
            for _ in range(a.warmup):
                pb.solve(stream)
        t_c5 = timed((lambda: pb.solve(stream)) if pb is not None else (lambda: None), xs)
        # the warp half of config 5: this rank's pairs in one set-up launch + one gather launch (grid.z = pair)
        if pb is not None:
            for _ in range(max(a.warmup, 2)):
                pb.warp(stream)
            pb.check_against_single_launches(stream, which=sorted({0, pb.batch - 1}))
        w_steps = max(4, xs // 4)               # a step is 64 / N pairs: ~1 ms
        t_c5w = timed((lambda: pb.warp(stream)) if pb is not None else (lambda: None), w_steps)
        # ... and with the geometry tables kept from the first call (they depend on the edges and the canvas only)
        t_c5g = timed((lambda: pb.warp(stream, N.WARP_CELLS | N.WARP_GATHER)) if pb is not None else (lambda: None), w_steps)
        # the whole job: solve + warp of every pair, in groups, the warp of group k beside the solve of group k + 1
        t_job = t_job_seq = None
        if pb is not None:
            canv = pb.out.clone()
            pb.prepare_whole_job(a.c5_chunks)
            for ov in (False, True):
                pb.out.zero_()
                pb.whole_job(ov)
                torch.cuda.synchronize()
                assert torch.equal(pb.out, canv), "whole-job canvases differ from the batched warp's"
            del canv
        j_steps = max(3, xs // 8)
        t_job_seq = timed((lambda: pb.whole_job(False)) if pb is not None else (lambda: None), j_steps)
        t_job = timed((lambda: pb.whole_job(True)) if pb is not None else (lambda: None), j_steps)
        if pb is not None:
            assert int(pb.status.cpu()[0]) == 0, "device status word set by the batched warp"
        cells_c5 = CONFIGS["C5"][3] ** 2
        c5_pixels = (pb.pair.final_w * pb.pair.final_h) if pb is not None else 0
        # algorithmic bytes of the rank's batched warp: 6 B per pixel inside the source, 3 B per blank one, summed over its canvases
        c5_bytes = 0
        if pb is not None:
            nzp = int((pb.out.view(pb.batch, -1, 3).amax(dim=2) > 0).sum().cpu())
            c5_bytes = 6 * nzp + 3 * (pb.batch * c5_pixels - nzp)
        if dist is not None:
            tt = torch.tensor([float(c5_pixels)], dtype=torch.float64, device=dev)
            dist.all_reduce(tt, op=dist.ReduceOp.MAX)
            c5_pixels = int(tt.cpu()[0])
        c5_obj = {"workload": f"C5: {total_pairs} independent 3840x2160 pairs, 2000 correspondences, 100x100 mesh each; "
                              f"{len(mine)} per rank in ONE batched launch", "world_size": world, "scaling": "strong",
                  "value": total_pairs * cells_c5 * xs / t_c5, "unit": "homographies/s",
                  "solve_ms_per_step": t_c5 / xs * 1e3, "pairs_per_s": total_pairs * xs / t_c5,
                  "pairs_per_rank": len(mine), "collectives_per_step": "none (independent pairs)",
                  "whole_job": {"pairs_per_s": total_pairs * j_steps / t_job, "ms_per_step": t_job / j_steps * 1e3,
                                "one_stream_ms_per_step": t_job_seq / j_steps * 1e3, "groups": a.c5_chunks, "steps": j_steps,
                                "note": "solve AND warp of all the pairs, numpy-free and resident: the rank's pairs in groups, every "
                                        "group's solve leaving its cells warp ready (apap_solve_warp_batch_device), the gather of "
                                        "group k on a second stream beside the solve of group k + 1; one_stream = the same launches in "
                                        "sequence.  Measured: the overlap buys ~9 % over one stream and nothing over the two batched "
                                        "launches of `solve_ms_per_step` + `warp.ms_per_step` - K1 keeps every SIMD's issue pipe busy, "
                                        "and half of the warp's time is VALU work that has to queue behind it; canvases checked against "
                                        "the batched warp's"},
                  "warp": {"value": total_pairs * c5_pixels * w_steps / t_c5w / 1e6, "unit": "Mpix/s",
                           "ms_per_step": t_c5w / w_steps * 1e3, "us_per_pair": t_c5w / w_steps / max(len(mine), 1) * 1e6,
                           "steps": w_steps,
                           "geometry_kept_us_per_pair": t_c5g / w_steps / max(len(mine), 1) * 1e6,
                           "roofline": {"kernels": "k_warp_setup + k_warp_fast over the rank's pairs (rank 0)", "bound": "hbm",
                                        "achieved": c5_bytes / (t_c5g / w_steps) / 1e9, "peak": PEAK_HBM_GBS, "unit": "GB/s",
                                        "frac": c5_bytes / (t_c5g / w_steps) / 1e9 / PEAK_HBM_GBS,
                                        "note": "whole batched step (per-cell set-up launch + gather launch), wall clock: the steady "
                                                "state of K3 - many generations of waves, the ~4.5 us of launch, first table trips and "
                                                "last stores paid once for all the pairs"},
                           "note": "apap_warp_batch_device: one set-up launch over every pair's cells and one gather launch over "
                                   "every canvas of the rank's pairs (grid.z = pair), source images and canvases resident; the "
                                   "canvases of the first and last pair are checked against one apap_warp_device launch each; "
                                   "us_per_pair is per pair of ONE rank's share; geometry_kept = APAP_WARP_CELLS | APAP_WARP_GATHER on "
                                   "a workspace whose canvas row / column tables are kept from an earlier call"}}
        del pb

    # ------------------------------------------------------------------ cells: one pair sharded
    cells_obj = None
    if not a.no_cells:
        phase("cells (config 4: table broadcast, H all-gather, canvas all-gather)")
        from cvx_proj_amd.dist import ShardedSolver
        cp = config_pair(a.cells_config, with_image=(rank == 0))
        cs = ShardedSolver(cp, dev, dist, ctx=ctx)
        barrier()
        t0 = time.perf_counter()
        cs.broadcast_inputs()           # once per pair: keypoint table + de-normalisation block from rank 0
        barrier()
        t_bcast = time.perf_counter() - t0
        cs.solve()
        barrier()
        t0 = time.perf_counter()
        cs.warp()                       # first call: the source image travels from rank 0 (set-up), then one warp
        barrier()
        t_first_warp = time.perf_counter() - t0
        # conditioning by COUNT here (the same on every rank: solve() holds a collective), ~condition_ms of C4 solves
        for _ in range(int(a.condition_ms * world / 1.4) if a.condition_ms > 0 else 0):
            cs.solve()
        for _ in range(a.warmup):
            cs.solve()
            cs.warp()
        tc_solve = timed(cs.solve, xs)
        tc_other = None
        if world > 1:           # the other form of the solve (one launch + one gather / two launches, first gather overlapped)
            co = ShardedSolver(cp, dev, dist, ctx=ctx, overlap=not cs.overlap)
            co.broadcast_inputs()
            for _ in range(a.warmup + 3):
                co.solve()
            tc_other = timed(co.solve, xs)
            del co
        tc_warp = timed(cs.warp, xs)
        tc_bands = timed(lambda: cs.warp(gather=False), xs)           # the canvas left distributed: no collective
        tc_step = timed(cs.step, xs)                                  # solve + H gather in flight + own band + wait
        assert int(cs.status.cpu()[0]) == 0
        ctx.set("profile", 1)
        for _ in range(min(xs, 10)):
            cs.solve()
            cs.warp()
        torch.cuda.synchronize()
        ckern = read_kernel_ms(ctx)
        ctx.set("profile", 0)
        # K3 alone on this configuration's whole canvas (one rank): the gather kernel on a kept workspace, launches back to back
        c_k3 = None
        if world == 1 and cp.img is not None:
            from cvx_proj_amd.dist import WarpPlan
            wp = WarpPlan(cp.mesh, (cs.rows, cs.cols), cp.final_w, cp.final_h, cp.off_x, cp.off_y, dev, ctx=ctx)
            wp.cells(cs.H)
            c_img = torch.from_numpy(np.ascontiguousarray(cp.img)).to(dev)
            c_out = torch.empty((1, cp.final_h, cp.final_w, 3), dtype=torch.uint8, device=dev)
            for _ in range(5):
                wp.gather(c_img, out=c_out)
            c_ms = back_to_back(lambda: wp.gather(c_img, out=c_out), max(xs, 20))
            assert torch.equal(c_out[0], cs.warp()) and int(wp.status.cpu()[0]) == 0
            c_nz = int((c_out[0].amax(dim=2) > 0).sum().cpu())
            c_bytes = 6 * c_nz + 3 * (cp.final_w * cp.final_h - c_nz)
            c_k3 = {"kernel": "k_warp_fast, whole canvas of this configuration, warm, launches back to back", "bound": "hbm",
                    "kernel_ms": c_ms, "algorithmic_bytes": c_bytes, "achieved": c_bytes / (c_ms * 1e-3) / 1e9, "peak": PEAK_HBM_GBS,
                    "unit": "GB/s", "frac": c_bytes / (c_ms * 1e-3) / 1e9 / PEAK_HBM_GBS,
                    "note": "the same kernel as roofline_warp on a 4 x larger canvas: its time is ~4.5 us per launch + bytes at a "
                            "marginal rate (profiles/r04_k3_experiments.txt), so the fraction grows with the canvas"}
            del wp, c_img, c_out
        c_flops = K1_FLOPS_PER_CELL_POINT * cs.n * cs.my_cells       # THIS rank's cells: what its K1 launch worked on
        c_ach = c_flops / (ckern["assemble"] * 1e-3) / 1e12 if ckern.get("assemble") else None
        cells_obj = {
            "workload": f"{a.cells_config}: {CONFIGS[a.cells_config][0]}x{CONFIGS[a.cells_config][1]} pair, {cs.n} "
                        f"correspondences, {cs.rows}x{cs.cols} mesh, canvas {cp.final_w}x{cp.final_h}; mesh rows and canvas "
                        f"rows sharded over the ranks",
            "world_size": world, "backend": ("rccl (nccl)" if backend == "nccl" else backend) if world > 1 else "none (1 rank)",
            "scaling": "strong", "value": cs.cells_total * xs / tc_solve, "unit": "homographies/s",
            "solve_ms_per_step": tc_solve / xs * 1e3,
            "warp": {"value": cp.final_w * cp.final_h * xs / tc_warp / 1e6, "unit": "Mpix/s",
                     "ms_per_step": tc_warp / xs * 1e3,
                     "note": "row bands + all-gather: the whole canvas on every rank after every step"},
            "warp_bands_only": {"value": cp.final_w * cp.final_h * xs / tc_bands / 1e6, "unit": "Mpix/s",
                                "ms_per_step": tc_bands / xs * 1e3,
                                "note": "row bands left where they are computed (no collective): the part of the warp that "
                                        "shards; SURVEY.md 8e expects the gathered form to be transfer-dominated.  Bands are aligned to the "
                                        "mesh rows a rank solved: its set-up kernel inverts 1 / world of the cells"},
            "pipelined_step": {"ms_per_step": tc_step / xs * 1e3,
                               "note": "ShardedSolver.step(): each rank solves its mesh rows, starts the all-gather of the H grid, "
                                       "warps ITS band (the canvas rows of its own mesh rows, from its own rows of the grid) "
                                       "while the gather runs, then waits: solve + warp_bands_only with the collective hidden"},
            "table_broadcast_ms": t_bcast * 1e3, "first_warp_incl_image_broadcast_ms": t_first_warp * 1e3,
            "collectives_per_step": "solve: the H grid (36 B per cell) in 2 all-gathers, the first beside the second half's "
                                    "kernels; warp: 1 all-gather of the canvas bands" if world > 1 else "none",
            "collectives_overlapped": bool(cs.overlap),
            "solve_other_form_ms_per_step": None if tc_other is None else tc_other / xs * 1e3,
            "solve_forms_note": "solve_ms_per_step is ShardedSolver's default for this world size (two launches per rank with the "
                                "first all-gather beside the second for 2-4 ranks, one launch + one gather above: a model, "
                                "cvx_proj_amd/dist.py); solve_other_form_ms_per_step is the other form on the same ranks",
            "rank0_cells": cs.my_cells, "kernels_ms": ckern,
            "roofline": None if c_ach is None else {
                "kernel": "k_assemble (rank 0's shard)", "bound": "mfma", "achieved": c_ach, "peak": PEAK_FP64_TFLOPS,
                "unit": "TFLOP/s", "frac": c_ach / PEAK_FP64_TFLOPS},
            "roofline_warp": c_k3,
        }
        del cs

    if rank == 0:
        flops = K1_FLOPS_PER_CELL_POINT * res.n * res.cells * res.batch          # rank 0's own launch
        t_k1 = kern["assemble"] * 1e-3
        achieved = flops / t_k1 / 1e12
        resolved = "mfma" if a.variant == "auto" else a.variant      # auto = mfma (apap_kernels.hip plan_solve)
        # small meshes under AUTO take ONE fused launch (K1 + K2): it is timed in the `assemble` slot and `eigen` stays empty
        fused = a.variant == "auto" and res.cells * res.batch <= ctx.get("fused_max_cells")
        if fused:
            kern["solve_small (K1 + K2 fused, reported in the assemble slot)"] = kern["assemble"]
        # HBM bytes per launch from the PMC counters, collected in separate rocprofv3 passes
        # (tools/profile.sh) and committed under profiles/: (2 x FETCH_SIZE + WRITE_SIZE) KiB,
        # FETCH_SIZE doubled as MI355X_MICROARCH.md prescribes for 16-B-per-lane reads.
        traffic, traffic_warp, tj = None, None, {}
        tfile = os.path.join(ROOT, "profiles", "pmc_traffic.json")
        if os.path.exists(tfile):
            tj = json.load(open(tfile))
            traffic = tj.get(f"{a.config}:k_assemble_{resolved}")
            traffic_warp = tj.get(f"{a.config}:k_warp_fast", tj.get(f"{a.config}:k_warp_rows"))
        # K3 (HBM-bound half of the metric): 6 B per in-range pixel, 3 B per blank one
        k3_name = "k_warp_fast"
        out_pixels = pair.final_w * pair.final_h
        nz = int((res.out.view(-1, 3).amax(dim=1) > 0).sum().cpu())
        warp_bytes = 6 * nz + 3 * (out_pixels - nz)
        line.update({
            "extra_steps": xs,
            "standalone": {"solve_ms_per_step": t_solve_plain / xs * 1e3, "value": units_solve * xs / t_solve_plain,
                           "warp_ms_per_step": t_warp_alone / xs * 1e3,
                           "warp_value": units_warp * xs / t_warp_alone / 1e6, "warp_unit": "Mpix/s",
                           "note": "the two halves as separate services: apap_solve_device (H grid only) and apap_warp_device on a "
                                   "grid from anywhere (its own set-up launch: inverses, records, lookup tables, then the gather)"},
            "warp_two_in_flight": {"value": 2 * units_warp * xs / t_warp2 / 1e6, "unit": "Mpix/s",
                                   "ms_per_pair": t_warp2 / xs / 2 * 1e3,
                                   "note": "the same warp step issued twice per step on two streams into two canvases: one warp "
                                           "step alone leaves the chip partly idle (a set-up kernel of one wave per SIMD, then 1.45 "
                                           "generations of waves that compute together and wait together); a second, independent one "
                                           "fills it.  What a caller with several pairs in flight gets; extra, not `warp.value`"},
            "configs": configs_obj,
            "moments24": modes_obj,
            "pairs": c5_obj,
            "cells": cells_obj,
            "stitch": {
                "value": pair.final_w * pair.final_h * xs / t_stitch / 1e6, "unit": "Mpix/s (rank 0)",
                "ms_per_step": t_stitch / xs * 1e3,
                "note": "fused warp + paste + uniform_blend, apap.py:258-262; extra, not in `value`"},
            "equalize": {
                "value": pair.shape[0] * pair.shape[1] * xs / t_eq / 1e6, "unit": "Mpix/s (rank 0)",
                "ms_per_step": t_eq / xs * 1e3,
                "roofline": {"kernels": "k_eq_hist + k_eq_apply", "bound": "hbm",
                             "achieved": 3.0 * pair.img.size / ((kern["eq_hist"] + kern["eq_apply"]) * 1e-3) / 1e9,
                             "peak": PEAK_HBM_GBS, "unit": "GB/s",
                             "frac": 3.0 * pair.img.size / ((kern["eq_hist"] + kern["eq_apply"]) * 1e-3) / 1e9 / PEAK_HBM_GBS},
                "note": "per-channel cv.equalizeHist of the 4K source image, utils.py:85-91; algorithmic "
                        "traffic 3 bytes per image byte (read, read, write); extra, not in `value`"},
            "ransac": {
                "ms_per_call": t_ransac / xs * 1e3, "hypotheses": N.RANSAC_ITERATIONS, "points": res.n,
                "inliers": int(res.r_res.cpu()[1]),
                "note": "device half of the seed homography (4-point hypotheses, 5 px), baseline_stitch_test.py:42; "
                        "three small latency-bound kernels (fusing the selection into the scoring kernel's last block was measured in round 6: slower, profiles/r06_frontend_fusion.txt); extra, not in `value`"},
            "kernels_ms": kern,
            "roofline": {"kernel": "k_solve_small (fused K1 + K2: the K2 tail is inside the time, only K1's flops are counted)"
                                   if fused else "k_assemble_" + resolved, "bound": "mfma",
                         "achieved": achieved, "peak": PEAK_FP64_TFLOPS, "unit": "TFLOP/s",
                         "frac": achieved / PEAK_FP64_TFLOPS, "traffic": traffic,
                         "traffic_vs_algorithmic": None if traffic is None else traffic / (36.0 * res.cells * res.batch + 16.0 * res.n),
                         "traffic_note": "the moment slab K1 writes and K2 reads back (30 doubles per cell and keypoint split) is "
                                         "~17x the algorithmic 36 B per cell + 16 B per keypoint; at ~165 GB/s it is 2 % of HBM",
                         "hbm_gbs": None if traffic is None else traffic / t_k1 / 1e9,
                         "note": "fp64 work, issue-bound: no vector instruction co-executes with an f64 MFMA on gfx950 "
                                 "(profiles/r02_coexec.txt), so the datasheet's single 78.6 TF figure covers the 32 "
                                 "accumulation FMAs AND the ~20-instruction fp64 weight chain per (cell, keypoint), which "
                                 "the algorithmic count prices at 58 flops; the kernel runs ~266 issue cycles per 64 "
                                 "pairs whatever the MFMA shape (profiles/r02_k1_variants.txt, DESIGN.md section 3)"},
            "roofline_k2": roofline_k2(a.config, res, kern, kern_plain, tj, fused),
            "roofline_warp": {
                "kernel": k3_name, "cache": "warm", "bound": "hbm", "achieved": warp_bytes / (k3_warm_ms * 1e-3) / 1e9,
                "peak": PEAK_HBM_GBS, "unit": "GB/s", "frac": warp_bytes / (k3_warm_ms * 1e-3) / 1e9 / PEAK_HBM_GBS,
                "kernel_ms": k3_warm_ms, "kernel_ms_with_an_event_pair_per_launch": kern["warp"],
                "timing": "HIP events on the launch stream around a run of launches issued back to back (duration + launch gap)",
                "traffic": traffic_warp, "traffic_raw": tj.get(f"{a.config}:k_warp_fast:raw"),
                "traffic_note": "traffic_raw = FETCH_SIZE + WRITE_SIZE as the counters read (profiles/pmc_traffic.json); traffic = "
                                "1.54 x FETCH_SIZE + WRITE_SIZE, the factor CHOSEN so that a cold launch's fetch equals the 24.9 MB "
                                "image it must read (the counter does not count dword gathers in full): equal to the algorithmic "
                                "bytes by construction, not a measurement of them.  Either way: no wasted traffic",
                "note": "the bench warps the same 25 MB image into the same 27 MB canvas back to back: both stay in the "
                        "256 MiB Infinity Cache, so this figure is priced against a memory the kernel mostly does not "
                        "touch; roofline_warp_cold is the HBM one"},
            "value_from_idle": {"value": res.cells * res.batch / t_idle, "unit": "homographies/s",
                                "ms": t_idle * 1e3,
                                "note": "ONE solve call from an idle chip (0.4 s pause before it, median of 3), launch + both "
                                        "kernels + synchronisation; `value` is the steady state after conditioning_ms of load"},
        })
        if cold:
            line["warp_cold"] = {"value": units_warp * xs / t_warp_cold / 1e6, "unit": "Mpix/s",
                                 "ms_per_step": t_warp_cold / xs * 1e3, "buffer_sets": len(cold),
                                 "bytes_rotated": len(cold) * (res.img.numel() + res.out.numel())}
            line["roofline_warp_cold"] = {
                "kernel": k3_name, "cache": "cold", "bound": "hbm",
                "achieved": warp_bytes / (k3_cold_ms * 1e-3) / 1e9, "peak": PEAK_HBM_GBS, "unit": "GB/s",
                "frac": warp_bytes / (k3_cold_ms * 1e-3) / 1e9 / PEAK_HBM_GBS, "kernel_ms": k3_cold_ms,
                "kernel_ms_with_an_event_pair_per_launch": kern_cold["warp"],
                "traffic": tj.get(f"{a.config}:k_warp_fast:cold"), "traffic_raw": tj.get(f"{a.config}:k_warp_fast:raw"),
                "note": f"{len(cold)} (image, canvas) sets = {len(cold) * (res.img.numel() + res.out.numel()) / 1e6:.0f} MB "
                        f"warped in rotation: every launch reads its source from HBM and writes a canvas that is not cached"}
        if world == 1 and not a.no_call_level:
            line["call_level"] = call_level(a.config)
            line["pipeline"] = pipeline_level(a.config)
            line["cli"] = cli_level()
        if world == 1 and not a.no_cpu_baseline:
            workers = usable_cores() if a.cpu_pool < 0 else a.cpu_pool
            line["cpu_baseline"] = cpu_baseline(a.config, a.cpu_cells, a.cpu_rows, min(workers, 256))
    finish(line)


if __name__ == "__main__":
    try:
        main()
    except SystemExit:
        raise
    except BaseException as e:      # noqa: BLE001  (leave evidence and a non-zero exit code; never re-exec a process that touched the GPU)
        import traceback
        traceback.print_exc()
        print(json.dumps({"bench_failed": repr(e)[:300], "rank": os.environ.get("RANK", "0")}), file=sys.stderr, flush=True)
        sys.stdout.flush()
        os._exit(1)                 # a hung collective's threads must not keep the process alive
