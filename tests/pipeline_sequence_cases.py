"""One sequence of unlike pairs for ONE resident ``Pipeline`` (cvx_proj_amd/pipeline.py): builders only, numpy only.

Between passes a ``Pipeline`` keeps device buffers that only grow (a pass works on prefix views of them), a FIFO of at most
``PLAN_CAPACITY`` warp plans keyed by the canvas geometry and the mesh (each with the geometry tables, the per-cell records that
the solve's tail writes, a status word and a device copy of the mesh's vertices), page-locked staging and a side stream.  The
sequence below makes every one of them meet a pass it was not left in shape for.  tests/test_pipeline_sequence_inputs.py asserts
on the CPU, from the oracle alone, that the steps reach what the right-hand column says; tests/test_gpu_pipeline_sequence.py
runs them.

A step is ``(pair, mesh, mode, sampling, transfer)``: ``mode`` none (no picture: no plan, ``hip_solve``), warp or stitch;
``sampling`` None, "nearest" or "bilinear"; ``transfer`` pageable, pinned (the pictures in page-locked arrays) or
pinned+canvas_out (and the canvas into one).  ``expect`` is ok, singular (``np.linalg.LinAlgError``) or nofit (``ValueError``:
the centre picture does not fit the canvas at the offsets, what the reference's paste raises).

 step  pair /mesh  mode    sampling  transfer           plan     what it is there for
    0  A    /65    warp    -         pageable           miss     the largest first: 320 x 200, n = 300, 4225 cells > 4096: K1 + K2, and
                                                                 K2's tail writes the plan's records
    1  B    /4     warp    -         pageable           miss     the smallest directly after: 128 x 128, n = 33, 16 cells: the fused
                                                                 kernel's tail writes the records; every pooled buffer is a short view
    2  B2   /4     stitch  -         pageable           hit      the same geometry, other keypoints: records and status word are B's
    3  B2   /4     none    -         -                  -        no picture: no plan, the plain solve on the pooled buffers
    4  B2   /4     warp    -         pageable           hit      the plan again after the pass that went round it
    5  A    /2     warp    -         pinned             miss     the same canvas as step 0, cells 167 px wide (> 128: the all-float64
                                                                 strips); the page-locked picture buffer at its full size
    6  A    /10    warp    -         pageable           miss     a third plan on the one canvas size
    7  C    /10    warp    bilinear  pageable           miss     176 x 144: as many cells as step 6, so a vertex table of equal length
                                                                 and other contents
    8  C    /10    warp    -         pageable           hit      the sampling switched on one cached plan: the default,
    9  C    /10    warp    nearest   pageable           hit      the keyword,
   10  C2   /10    stitch  bilinear  pageable           hit      and bilinear again under the blend
   11  D63  /5     warp    -         pageable           miss     n = 63: one keypoint short of a 64-keypoint chunk
   12  D64  /5     stitch  -         pageable           hit      n = 64: exactly one chunk
   13  D65  /5     warp    -         pageable           hit      n = 65: one keypoint in a second chunk
   14  E    /8     warp    -         pageable           miss     the transfer kinds in turn on one geometry: pageable,
   15  E2   /8     stitch  -         pinned             hit      page-locked pictures (prefix views of the buffers of step 5),
   16  E    /8     warp    -         pinned+canvas_out  hit      a page-locked canvas as well,
   17  E2   /8     stitch  -         pageable           hit      pageable again
   18  F    /7     stitch  -         pageable           miss     the eighth plan: the FIFO is full
   19  G    /16    warp    bilinear  pageable           miss     the ninth: step 0's plan is dropped
   20  K    /20    warp    -         pageable           miss     the tenth: step 1's plan (B /4) is dropped
   21  B    /4     warp    -         pageable           rebuilt  the dropped geometry again: a new plan (A /2 is dropped)
   22  D64  /5     warp    -         pageable           hit      a geometry that is still cached: the plan of step 11
   23  O1   /6     warp    -         pageable           miss     ox = 23, oy = 17; a 260 x 150 picture, a 320 x 200 centre (A /10 dropped)
   24  O1   /6     stitch  -         pageable           hit      that centre does not fit the 312 x 208 canvas at (23, 17): ValueError
   25  O2   /6     warp    -         pageable           miss     the two shapes exchanged: 343 x 217, the same offsets (C /10 dropped)
   26  O2   /6     stitch  bilinear  pageable           hit      the centre pasted at (23, 17)
   27  Z    /5     stitch  -         pageable           hit      every keypoint zero: LinAlgError, on a plan that has served four pairs
   28  D65  /5     stitch  -         pageable           hit      a good pair on that plan: its status word is the geometry's again
   29  A    /65    warp    -         pageable           rebuilt  step 0 again, on a new plan: the bytes of step 0

The FIFO holds A65 B4 A2 A10 C10 D5 after step 13, is full after step 18 and drops its oldest plan at steps 19, 20, 21, 23, 25
and 29; a hit does not renew a plan.  Twelve distinct keys in all.
"""
from collections import namedtuple
from functools import lru_cache

import numpy as np

from cvx_proj_amd import geometry
from cvx_proj_amd.synth import synth_pair

PLAN_CAPACITY = 8           # Pipeline._plan's FIFO
FUSED_MAX_CELLS = 4096      # APAP_OPT_FUSED_MAX_CELLS' default: more cells than this take K1 + K2
WIDE_CELL = 128.0           # px: the float32-estimate gather kernel's limit on a cell's width
CHUNK = 64                  # keypoints per K1 chunk

OFFSET_HG = np.array([[0.97, 0.02, -23.5], [0.01, 1.03, -17.25], [2e-5, -1e-5, 1.0]])

Step = namedtuple("Step", "pair mesh mode sampling transfer expect")
Pair = namedtuple("Pair", "name img center src dst Hg other_shape center_shape gamma sigma")

# name -> (width, height, keypoints, seed, gamma, sigma) of a cvx_proj_amd.synth pair
SYNTH = {
    "A": (320, 200, 300, 101, 0.5, 100.0),
    "B": (128, 128, 33, 102, 0.5, 40.0),
    "B2": (128, 128, 33, 103, 0.5, 40.0),
    "C": (176, 144, 120, 104, 0.5, 15.0),
    "C2": (176, 144, 97, 105, 0.25, 30.0),
    "D63": (160, 120, 63, 106, 0.5, 12.0),
    "D64": (160, 120, 64, 107, 0.5, 12.0),
    "D65": (160, 120, 65, 108, 0.5, 12.0),
    "E": (200, 150, 150, 109, 0.5, 100.0),
    "E2": (200, 150, 90, 110, 0.5, 50.0),
    "F": (240, 135, 200, 111, 0.5, 60.0),
    "G": (256, 256, 257, 112, 0.5, 100.0),
    "K": (320, 200, 128, 113, 0.5, 100.0),
}
# name -> ((other width, height), (centre width, height), keypoints, seed, gamma, sigma): OFFSET_HG, unequal shapes
OFFSET = {
    "O1": ((260, 150), (320, 200), 140, 114, 0.5, 50.0),
    "O2": ((320, 200), (260, 150), 140, 115, 0.5, 50.0),
}
SINGULAR = {"Z": "D64"}     # name -> the pair whose pictures it keeps; every keypoint is (0, 0)

SEQUENCE = (
    Step("A", 65, "warp", None, "pageable", "ok"),
    Step("B", 4, "warp", None, "pageable", "ok"),
    Step("B2", 4, "stitch", None, "pageable", "ok"),
    Step("B2", 4, "none", None, "pageable", "ok"),
    Step("B2", 4, "warp", None, "pageable", "ok"),
    Step("A", 2, "warp", None, "pinned", "ok"),
    Step("A", 10, "warp", None, "pageable", "ok"),
    Step("C", 10, "warp", "bilinear", "pageable", "ok"),
    Step("C", 10, "warp", None, "pageable", "ok"),
    Step("C", 10, "warp", "nearest", "pageable", "ok"),
    Step("C2", 10, "stitch", "bilinear", "pageable", "ok"),
    Step("D63", 5, "warp", None, "pageable", "ok"),
    Step("D64", 5, "stitch", None, "pageable", "ok"),
    Step("D65", 5, "warp", None, "pageable", "ok"),
    Step("E", 8, "warp", None, "pageable", "ok"),
    Step("E2", 8, "stitch", None, "pinned", "ok"),
    Step("E", 8, "warp", None, "pinned+canvas_out", "ok"),
    Step("E2", 8, "stitch", None, "pageable", "ok"),
    Step("F", 7, "stitch", None, "pageable", "ok"),
    Step("G", 16, "warp", "bilinear", "pageable", "ok"),
    Step("K", 20, "warp", None, "pageable", "ok"),
    Step("B", 4, "warp", None, "pageable", "ok"),
    Step("D64", 5, "warp", None, "pageable", "ok"),
    Step("O1", 6, "warp", None, "pageable", "ok"),
    Step("O1", 6, "stitch", None, "pageable", "nofit"),
    Step("O2", 6, "warp", None, "pageable", "ok"),
    Step("O2", 6, "stitch", "bilinear", "pageable", "ok"),
    Step("Z", 5, "stitch", None, "pageable", "singular"),
    Step("D65", 5, "stitch", None, "pageable", "ok"),
    Step("A", 65, "warp", None, "pageable", "ok"),
)

# what the docstring's table says of the steps, for the CPU test
ITEMS = {
    "largest": 0, "smallest": 1, "same geometry, other data": (2, 3, 4), "wide cells": 5, "one canvas, three meshes": (0, 5, 6),
    "equal cell counts": (6, 7), "sampling": (7, 8, 9, 10), "chunk": (11, 12, 13), "transfers": (14, 15, 16, 17),
    "dropped": 20, "rebuilt": (21, 29), "revisit cached": 22, "offsets": (23, 24, 25, 26), "singular": 27, "after singular": 28,
    "first again": 29,
}
PLAN = ("miss", "miss", "hit", "none", "hit", "miss", "miss", "miss", "hit", "hit", "hit", "miss", "hit", "hit", "miss", "hit", "hit",
        "hit", "miss", "miss", "miss", "rebuilt", "hit", "miss", "hit", "miss", "hit", "hit", "hit", "rebuilt")


class _Shape:
    def __init__(self, shape):
        self.shape = tuple(shape)


def _center(seed, shape):
    """A centre picture with no black pixel (``uniform_blend`` takes a black pixel for an absent one)."""
    return np.random.default_rng(seed).integers(1, 256, shape, dtype=np.uint8)


def _offset_pair(name):
    """cvx_proj_amd.synth's recipe with OFFSET_HG and a centre picture of another shape."""
    (ow, oh), (cw, ch), n, seed, gamma, sigma = OFFSET[name]
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, (oh, ow, 3), dtype=np.uint8)
    src = (rng.random((n, 2)) * [ow, oh]).astype(np.float32)
    s = src.astype(np.float64)
    q = np.concatenate([s, np.ones((n, 1))], axis=1) @ OFFSET_HG.T
    dst = q[:, :2] / q[:, 2:3] + 0.25 * np.sin(s * 9.6 / ow) + rng.normal(0.0, 0.5, (n, 2))
    return Pair(name, img, _center(seed + 1000, (ch, cw, 3)), src, dst.astype(np.float32), OFFSET_HG.copy(), (oh, ow, 3), (ch, cw, 3),
                gamma, sigma)


@lru_cache(maxsize=None)
def pair(name):
    """The pair of that name.  Cached: callers must not write into its arrays (the GPU test checks that nothing does)."""
    if name in OFFSET:
        return _offset_pair(name)
    if name in SINGULAR:
        p = pair(SINGULAR[name])
        return p._replace(name=name, src=np.zeros_like(p.src), dst=np.zeros_like(p.dst))
    w, h, n, seed, gamma, sigma = SYNTH[name]
    p = synth_pair(w, h, n, 1, seed)
    return Pair(name, p.img, _center(seed + 1000, p.shape), p.src, p.dst, p.Hg, p.shape, p.shape, gamma, sigma)


def final(step):
    """(fw, fh, ox, oy) of the step's canvas, as ``Pipeline.run_pair`` takes them."""
    p = pair(step.pair)
    return tuple(int(v) for v in geometry.final_size(_Shape(p.center_shape), _Shape(p.other_shape), p.Hg))


def mesh(step):
    fw, fh, _, _ = final(step)
    return geometry.get_mesh((fw, fh), step.mesh + 1)


def vertices(step):
    fw, fh, ox, oy = final(step)
    return geometry.get_vertice((fw, fh), step.mesh, (ox, oy))


def key(step):
    """The key under which ``Pipeline._plan`` keeps the step's plan."""
    fw, fh, ox, oy = final(step)
    return (step.mesh, step.mesh, fw, fh, ox, oy, mesh(step).tobytes())


def fifo(sequence, capacity=PLAN_CAPACITY):
    """A model of the plan cache: per step "none" (no picture, no plan), "hit", "miss" (a key never seen) or "rebuilt" (a key
    that was dropped); a dict keeps its insertion order and a hit does not renew an entry."""
    held, seen, out = [], set(), []
    for s in sequence:
        if s.mode == "none":
            out.append("none")
            continue
        k = key(s)
        if k in held:
            out.append("hit")
            continue
        out.append("rebuilt" if k in seen else "miss")
        seen.add(k)
        if len(held) >= capacity:
            held.pop(0)
        held.append(k)
    return out


def centre_fits(step):
    fw, fh, ox, oy = final(step)
    ch, cw = pair(step.pair).center_shape[:2]
    return ox + cw <= fw and oy + ch <= fh


def marks(step):
    """The names of ``Pipeline.device_marks`` for the step, in the order ``run_pair`` records them:
      begin                 always (side stream)
      image up (side)       page-locked pictures: their copies are enqueued before anything else
      main: first enqueue   always: the host set-up is done
      small uploads done    a plan: keypoint table, de-normalisation and vertices are enqueued, the status word re-seeded
      solve done            a plan
      image here            page-locked pictures: the main stream has waited for the side stream's copies
      warp done             a plan
      canvas down           ``canvas_out``"""
    pinned = step.mode != "none" and step.transfer.startswith("pinned")
    plan = step.mode != "none"
    names = ["begin"] + ["image up (side)"] * pinned + ["main: first enqueue"] + ["small uploads done", "solve done"] * plan
    return names + ["image here"] * pinned + ["warp done"] * plan + ["canvas down"] * (plan and step.transfer == "pinned+canvas_out")
