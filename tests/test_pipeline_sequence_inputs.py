"""The sequence of tests/pipeline_sequence_cases.py reaches what its table says: asserted from the builders, cvx_proj_amd.geometry,
the oracle and the numpy specs alone, so that tests/test_gpu_pipeline_sequence.py cannot pass without a ``Pipeline`` having
shrunk its buffers, met a second geometry, dropped a plan, rebuilt one and served a cached one.  The expectations are part of
the test.  ``oracle_grid``, ``coordinates`` and ``canvas`` are what the GPU test compares the passes with."""
import functools

import numpy as np
import pytest

import pipeline_sequence_cases as C
import warp_bilinear_spec as S
from oracle import apap_oracle as O

SEQ = C.SEQUENCE
PICTURE = [k for k, s in enumerate(SEQ) if s.mode != "none" and s.expect != "singular"]      # the steps that gather a canvas

# step -> (mesh, fw, fh, ox, oy): Pipeline's key is (mesh, mesh, fw, fh, ox, oy, the edges' bytes)
GEOMETRY = {
    "A": (335, 207, 0, 2), "B": (136, 133, 0, 0), "C": (186, 149, 0, 1), "D": (168, 124, 0, 1), "E": (210, 155, 0, 1),
    "F": (250, 140, 0, 2), "G": (273, 267, 0, 1), "K": (335, 207, 0, 2), "O1": (312, 208, 23, 17), "O2": (343, 217, 23, 17),
}


@functools.lru_cache(maxsize=None)
def oracle_grid(pair, mesh):
    """The reference's loop (float64 SVD per cell) for a pair on a mesh: (mesh, mesh, 3, 3) float32."""
    step = next(s for s in SEQ if (s.pair, s.mesh) == (pair, mesh))
    p = C.pair(pair)
    return O.local_homography_loop(p.src, p.dst, C.vertices(step), p.gamma, p.sigma, want_weights=False)[0]


def coordinates(step, grid):
    """The oracle's float64 source coordinates of every canvas pixel for a float32 grid."""
    fw, fh, ox, oy = C.final(step)
    return O.warp_coords_fast(O.invert_cells_f32(grid), C.mesh(step), (fw, fh), (ox, oy))


def canvas(step, tx, ty):
    """The step's canvas over those coordinates: the truncating rule of ``O.local_warp_fast`` or the bilinear definition, and
    ``local_stitch``'s paste and blend on top of either (ValueError when the centre does not fit)."""
    p = C.pair(step.pair)
    warped = (S.sample if step.sampling == "bilinear" else S.truncate)(p.img, tx, ty)
    return S.stitch(warped, p.center, C.final(step)[2:]) if step.mode == "stitch" else warped


def family(name):
    return name if name in ("O1", "O2") else name[0]


def test_the_key_of_every_step():
    for k, s in enumerate(SEQ):
        want = GEOMETRY["D" if s.pair == "Z" else family(s.pair)]
        assert C.final(s) == want, (k, C.final(s))
        key = C.key(s)
        assert key[:6] == (s.mesh, s.mesh) + want and key[6] == C.mesh(s).tobytes()
        edges = np.frombuffer(key[6], dtype=np.float64).reshape(2, s.mesh + 1)
        assert edges[0, 0] == edges[1, 0] == 0 and edges[0, -1] == want[0] and edges[1, -1] == want[1]
        assert C.vertices(s).shape == (s.mesh, s.mesh, 2)
        p = C.pair(s.pair)
        assert p.img.shape == p.other_shape and p.center.shape == p.center_shape and p.center.all(axis=-1).all()
        assert p.img.shape[0] * p.img.shape[1] <= 256 * 256 and len(p.src) <= 300 and p.src.dtype == p.dst.dtype == np.float32
    assert len({C.key(s) for s in SEQ}) == 12 > C.PLAN_CAPACITY


def test_the_plan_cache_hits_misses_drops_and_rebuilds_where_the_table_says():
    model = C.fifo(SEQ)
    assert tuple(model) == C.PLAN
    assert [k for k, m in enumerate(model) if m == "none"] == [3]
    assert [k for k, m in enumerate(model) if m == "rebuilt"] == list(C.ITEMS["rebuilt"]) == [21, 29]
    assert [k for k, m in enumerate(model) if m == "miss"] == [0, 1, 5, 6, 7, 11, 14, 18, 19, 20, 23, 25]
    # the FIFO is full at step 18; steps 19 and 20 drop the plans of steps 0 and 1; step 21 rebuilds step 1's
    assert sum(m == "miss" for m in model[:19]) == C.PLAN_CAPACITY
    assert C.key(SEQ[21]) == C.key(SEQ[1]) and C.key(SEQ[29]) == C.key(SEQ[0])
    assert SEQ[29] == SEQ[0] and SEQ[21] == SEQ[1]
    # the revisit of a cached geometry, and the singular pair, are on the plan of step 11, which has served four pairs
    assert model[22] == model[27] == model[28] == "hit"
    assert C.key(SEQ[22]) == C.key(SEQ[27]) == C.key(SEQ[28]) == C.key(SEQ[11])
    assert [SEQ[k].expect for k in (11, 12, 13, 22)] == ["ok"] * 4 and SEQ[27].expect == "singular" and SEQ[27].mode == "stitch"
    assert not C.pair("Z").src.any() and not C.pair("Z").dst.any() and SEQ[28].expect == "ok"
    # a step that is served from the cache meets records that another pair's solve wrote
    for k in C.ITEMS["same geometry, other data"]:
        assert C.key(SEQ[k]) == C.key(SEQ[1]) and SEQ[k].pair != SEQ[1].pair
    assert [SEQ[k].mode for k in C.ITEMS["same geometry, other data"]] == ["stitch", "none", "warp"]
    assert not np.array_equal(C.pair("B").src, C.pair("B2").src)


def test_which_steps_leave_the_fused_solve_and_the_float32_gather():
    cells = [s.mesh * s.mesh for s in SEQ]
    assert [k for k, c in enumerate(cells) if c > C.FUSED_MAX_CELLS] == [0, 29] and cells[0] == 4225
    assert cells[1] == 16 and min(cells) == 4
    wide = [k for k, s in enumerate(SEQ) if C.final(s)[0] / s.mesh > C.WIDE_CELL]
    assert wide == [5] and C.final(SEQ[5])[0] / 2 > 160
    # three plans on one canvas size; equal cell counts on two canvases, with vertex tables of one length and other contents
    a, b, c = (SEQ[k] for k in C.ITEMS["one canvas, three meshes"])
    assert C.final(a) == C.final(b) == C.final(c) and len({C.key(a), C.key(b), C.key(c)}) == 3
    a, b = (SEQ[k] for k in C.ITEMS["equal cell counts"])
    assert C.ITEMS["equal cell counts"] == (6, 7) and a.mesh == b.mesh and C.final(a) != C.final(b)
    assert C.vertices(a).shape == C.vertices(b).shape and not np.array_equal(C.vertices(a), C.vertices(b))
    # keypoint counts round one chunk on one geometry, in successive steps
    chunk = [SEQ[k] for k in C.ITEMS["chunk"]]
    assert [len(C.pair(s.pair).src) for s in chunk] == [C.CHUNK - 1, C.CHUNK, C.CHUNK + 1] and len({C.key(s) for s in chunk}) == 1


def test_consecutive_steps_shrink_and_grow_every_pooled_buffer():
    def sizes(s):
        p, (fw, fh, _, _) = C.pair(s.pair), C.final(s)
        return len(p.src), s.mesh * s.mesh, fw * fh * 3, p.img.size

    table = np.array([sizes(s) for s in SEQ])
    for column, name in enumerate(("keypoints", "cells", "canvas bytes", "picture bytes")):
        d = np.diff(table[:, column])
        assert (d < 0).any() and (d > 0).any(), name
    assert (np.diff(table[:2], axis=0) < 0).all()           # the second step is smaller in everything
    assert (table[0] == table.max(axis=0))[[0, 1]].all()    # the first step has the most keypoints and cells


def test_sampling_transfers_and_offsets():
    assert [(SEQ[k].sampling, SEQ[k].mode) for k in C.ITEMS["sampling"]] == \
        [("bilinear", "warp"), (None, "warp"), ("nearest", "warp"), ("bilinear", "stitch")]
    assert len({C.key(SEQ[k]) for k in C.ITEMS["sampling"]}) == 1
    assert [SEQ[k].transfer for k in C.ITEMS["transfers"]] == ["pageable", "pinned", "pinned+canvas_out", "pageable"]
    assert len({C.key(SEQ[k]) for k in C.ITEMS["transfers"]}) == 1
    # the page-locked picture buffer served a larger picture before (step 5)
    assert SEQ[5].transfer == "pinned" and C.pair(SEQ[5].pair).img.size > C.pair(SEQ[15].pair).img.size
    off = [SEQ[k] for k in C.ITEMS["offsets"]]
    assert [(s.pair, s.mode) for s in off] == [("O1", "warp"), ("O1", "stitch"), ("O2", "warp"), ("O2", "stitch")]
    for s in off:
        assert C.final(s)[2:] == (23, 17) and np.array_equal(C.pair(s.pair).Hg, C.OFFSET_HG)
    o1, o2 = C.pair("O1"), C.pair("O2")
    assert o1.other_shape == o2.center_shape == (150, 260, 3) and o1.center_shape == o2.other_shape == (200, 320, 3)
    # the centre fits every canvas but O1's: there the reference's paste raises, and so does the numpy definition
    assert [k for k, s in enumerate(SEQ) if s.mode == "stitch" and not C.centre_fits(s)] == [24]
    assert [k for k, s in enumerate(SEQ) if s.expect == "nofit"] == [24]
    assert [k for k, s in enumerate(SEQ) if s.expect == "singular"] == [27]


def test_the_marks_of_a_traced_pass():
    assert C.marks(SEQ[3]) == ["begin", "main: first enqueue"]
    assert C.marks(SEQ[0]) == ["begin", "main: first enqueue", "small uploads done", "solve done", "warp done"]
    assert C.marks(SEQ[16]) == ["begin", "image up (side)", "main: first enqueue", "small uploads done", "solve done", "image here",
                                "warp done", "canvas down"]
    assert C.marks(SEQ[15]) == C.marks(SEQ[16])[:-1]


@pytest.mark.parametrize("k", PICTURE)
def test_the_oracle_s_canvas_of_a_step(k):
    """More than half of the canvas gathers a pixel, the two samplers disagree, and no coordinate lies within 1e-9 of an integer
    (the picture's borders are integers): the rule that lets a pixel differ admits none on these inputs."""
    s = SEQ[k]
    p = C.pair(s.pair)
    tx, ty = coordinates(s, oracle_grid(s.pair, s.mesh))
    h, w = p.img.shape[:2]
    inside = S.present(tx, ty, w, h)
    ok = np.isfinite(tx) & np.isfinite(ty)
    near = np.minimum(np.abs(tx[ok] - np.rint(tx[ok])), np.abs(ty[ok] - np.rint(ty[ok])))
    print(f"step {k}: {inside.mean():.3f} of the canvas inside the picture, nearest integer {near.min():.3e} away")
    assert near.min() > 1e-9
    trunc, bilinear = S.truncate(p.img, tx, ty), S.sample(p.img, tx, ty)
    assert (trunc != bilinear).any()
    if s.expect == "nofit":
        with pytest.raises(ValueError):
            canvas(s, tx, ty)
        assert trunc.any(axis=-1).mean() > 0.5
        return
    out = canvas(s, tx, ty)
    fw, fh, _, _ = C.final(s)
    assert out.shape == (fh, fw, 3) and out.any(axis=-1).mean() > 0.5 and inside.mean() > 0.5
    if s.mode == "stitch":
        assert (out != (bilinear if s.sampling == "bilinear" else trunc)).any()
