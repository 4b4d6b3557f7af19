"""ONE resident ``Pipeline`` over the sequence of unlike pairs of tests/pipeline_sequence_cases.py (its docstring lists the steps
and what each is there for; tests/test_pipeline_sequence_inputs.py shows on the CPU that they get there).

A ``Pipeline`` is the one object here whose result could depend on what ran through it before: buffers that only grow, a FIFO
of warp plans with the records and the status word of the previous pair, a cached vertex table per plan, page-locked staging.
Every step is therefore held to something that knows nothing of the sequence:

  grid     within RMSE_BAR of the oracle's loop (the two 30-sum pipelines; the 24-sum form is not held to it, as in
           tests/test_gpu_k1_forms_edges.py)
  .mat     the bytes of ``native.invert_normalize_flatten(grid)``, and ``O.invert_normalize_flatten(grid)`` within the bound of
           test_cli_writes_reference_mat_layout
  canvas   the numpy definition (tests/warp_bilinear_spec.py: ``truncate`` is ``O.local_warp_fast``'s rule, ``sample`` the
           bilinear one, ``stitch`` the paste and blend) over the oracle's coordinates of the RETURNED grid; a pixel may differ
           only under ``check_warp``'s rule (tests/test_gpu_parity.py): its oracle coordinate within 1e-9 of an integer, and fewer
           than 1e-5 of the canvas.  The inputs admit no such pixel (asserted on the CPU for the oracle's grid)
  alone    grid, .mat array and canvas byte-equal to a fresh ``Pipeline`` of the same options running that step alone, and for
           the default context to ``apap.run_pair_by_calls``
  cache    ``pipe._plans`` against the FIFO model of the cases: never more than 8, a hit served by the same ``WarpPlan`` object, a
           rebuilt geometry by a new one, no plan for a pass without a picture, the status word back at the geometry's bits
           after the pass that follows the singular pair
  pool     where a pass works on the head of a longer pooled buffer (grid, .mat array, canvas), what lies behind the head is
           unchanged by it
and the inputs are unchanged after every step, the outputs of earlier steps unchanged at the end, and no returned array lies
in the pipeline's page-locked memory.  The last step is the first again and gives its bytes.
"""
import numpy as np
import pytest

import pipeline_sequence_cases as C
import test_pipeline_sequence_inputs as I
from oracle import apap_oracle as O

pytestmark = pytest.mark.gpu

RMSE_BAR = 1e-4          # px, north_star (tests/test_gpu_parity.py)
SEQ = C.SEQUENCE
CONTEXTS = {"default": None, "nofuse": {"fused_max_cells": 0}, "moments24": {"moments": 24}}
ERRORS = {"singular": np.linalg.LinAlgError, "nofit": ValueError}
ARRAYS = ("img", "center", "src", "dst", "Hg")
POOLED_OUTPUTS = ("H", "flat", "canvas")      # Pipeline._buf's names of what the kernels of a pass write

_alone, _coords = {}, {}


@pytest.fixture(scope="module", autouse=True)
def need_gpu(native):
    assert native.lib().apap_device_count() >= 1, "these tests need a GPU; the library found none"


def context(native, name):
    return None if CONTEXTS[name] is None else native.Context(**CONTEXTS[name])


def into(buf, a):
    """``a`` copied into the head of the flat page-locked ``buf``; the view of its shape."""
    v = buf[:a.size].reshape(a.shape)
    np.copyto(v, a)
    return v


def run(pipe, step, pinned=None):
    """The step through ``pipe``: (flat, canvas, grid).  ``pinned``: the page-locked buffers that the step's transfer kind uses."""
    p = C.pair(step.pair)
    other = center = out = None
    if step.mode != "none":
        other, center = p.img, p.center if step.mode == "stitch" else None
        if pinned is not None and step.transfer.startswith("pinned"):
            other = into(pinned["img"], p.img)
            center = into(pinned["center"], p.center) if center is not None else None
            if step.transfer == "pinned+canvas_out":
                fw, fh, _, _ = C.final(step)
                out = pinned["canvas"][:fh * fw * 3].reshape(fh, fw, 3)
                out[:] = 0x5C
    return pipe.run_pair(p.src, p.dst, p.Hg, p.other_shape, p.center_shape, step.mesh, p.gamma, p.sigma, other_img=other,
                         center_img=center, want_grid=True, canvas_out=out, sampling=step.sampling)


def outcome(fn):
    """``fn()``'s result, or the exception of a refused pass: the status word's or an argument check's, nothing else."""
    try:
        return fn()
    except (np.linalg.LinAlgError, ValueError, IndexError) as e:
        return e


def alone(native, name, step):
    """The step on a fresh ``Pipeline`` of the same options and, for the default context, through the chain of calls: computed
    once per (options, pair, mesh, mode, sampling) and left unchanged."""
    from cvx_proj_amd import apap
    from cvx_proj_amd.pipeline import Pipeline
    k = (name, step.pair, step.mesh, step.mode, step.sampling)
    if k not in _alone:
        ctx = context(native, name)
        fresh = outcome(lambda: run(Pipeline(ctx=ctx), step))
        calls = None
        if name == "default":
            p = C.pair(step.pair)
            other = p.img if step.mode != "none" else None
            center = p.center if step.mode == "stitch" else None
            calls = outcome(lambda: apap.run_pair_by_calls(p.src, p.dst, p.Hg, p.other_shape, p.center_shape, step.mesh, p.gamma, p.sigma,
                                                           other_img=other, center_img=center, sampling=step.sampling))
        if ctx is not None:
            ctx.close()
        _alone[k] = (fresh, calls)
    return _alone[k]


def coordinates(step, grid):
    k = (step.pair, step.mesh, grid.tobytes())
    if k not in _coords:
        _coords[k] = I.coordinates(step, grid)
    return _coords[k]


def same(a, b):
    return (a is None and b is None) or (a is not None and b is not None and a.dtype == b.dtype and a.shape == b.shape
                                         and a.tobytes() == b.tobytes())


def page_locked(pipe):
    """(first, one past the last) address of every page-locked block the pipeline owns."""
    blocks = [getattr(pipe, n, None) for n in ("_flat_host", "_stage_t", "_status_host")] + list(pipe._pinned)
    return [(t.data_ptr(), t.data_ptr() + t.numel() * t.element_size()) for t in blocks if t is not None]


def check_output(native, name, k, step, got, wrong, totals):
    """Grid, .mat array and canvas of one good step against the oracle and against the step alone."""
    p = C.pair(step.pair)
    flat, canvas, grid = got
    tag = f"[{name}] step {k} ({step.pair} /{step.mesh} {step.mode})"
    cells = step.mesh * step.mesh
    if not (grid.shape == (step.mesh, step.mesh, 3, 3) and grid.dtype == np.float32 and flat.shape == (cells, 9)
            and flat.dtype == np.float64 and np.isfinite(grid).all()):
        wrong.append(f"{tag}: shapes, types or a value that is not finite")
        return
    # the grid
    ref = I.oracle_grid(step.pair, step.mesh)
    d = float(O.reprojection_rmse_delta(grid, ref, p.src).max())
    differ = int((grid != ref).sum())
    if name != "moments24":
        totals["rmse"] = max(totals["rmse"], d)
        if not d < RMSE_BAR:
            wrong.append(f"{tag}: grid: rmse delta {d:.3e} px against the oracle's loop")
    # the .mat array
    if flat.tobytes() != native.invert_normalize_flatten(grid).tobytes():
        wrong.append(f"{tag}: .mat array: not the bytes of invert_normalize_flatten(grid)")
    want = O.invert_normalize_flatten(grid)
    if not np.allclose(flat, want, rtol=1e-5, atol=1e-7):
        wrong.append(f"{tag}: .mat array: outside rtol 1e-5 / atol 1e-7 of the oracle's")
    flat_differ = int((flat != want).sum())
    totals["flat"] += flat_differ
    # the canvas
    pixels = 0
    if step.mode == "none":
        if canvas is not None:
            wrong.append(f"{tag}: a canvas without a picture")
    else:
        tx, ty = coordinates(step, grid)
        want = I.canvas(step, tx, ty)
        if canvas is None or canvas.shape != want.shape or canvas.dtype != np.uint8:
            wrong.append(f"{tag}: canvas: {None if canvas is None else canvas.shape}, wanted {want.shape}")
        else:
            diff = (canvas != want).any(axis=-1)
            pixels = int(diff.sum())
            totals["pixels"] += pixels
            if pixels:
                near = np.minimum(np.abs(tx[diff] - np.round(tx[diff])), np.abs(ty[diff] - np.round(ty[diff])))
                if not ((near < 1e-9).all() and diff.mean() < 1e-5):
                    y, x = np.argwhere(diff)[0]
                    wrong.append(f"{tag}: canvas: {pixels} pixels differ from the definition over the oracle's coordinates, first at "
                                 f"(y, x) = ({y}, {x}): {canvas[y, x]} != {want[y, x]}")
    print(f"{tag}: rmse-delta max {d:.3e} px, {differ} grid entries, {flat_differ} .mat entries and {pixels} pixels differ from the oracle's")
    # the step alone
    fresh, calls = alone(native, name, step)
    if isinstance(fresh, Exception) or not all(same(a, b) for a, b in zip(got, fresh)):
        wrong.append(f"{tag}: not the bytes of a fresh Pipeline running this step alone")
    if calls is not None and (isinstance(calls, Exception) or not (same(flat, calls[0]) and same(canvas, calls[1]))):
        wrong.append(f"{tag}: not the bytes of run_pair_by_calls")


def run_sequence(native, name):
    import torch
    from cvx_proj_amd.pipeline import Pipeline
    ctx = context(native, name)
    pipe = Pipeline(ctx=ctx)
    big = max(C.pair(s.pair).img.size for s in SEQ)
    pinned = {"img": pipe.pinned_array((big,)), "center": pipe.pinned_array((big,)),
              "canvas": pipe.pinned_array((max(C.final(s)[0] * C.final(s)[1] for s in SEQ) * 3,))}
    original = {n: {a: getattr(C.pair(n), a).copy() for a in ARRAYS} for n in {s.pair for s in SEQ}}
    model = C.fifo(SEQ)
    wrong, kept, dropped = [], [], {}
    totals = {"rmse": 0.0, "flat": 0, "pixels": 0}
    for k, (step, expect) in enumerate(zip(SEQ, model)):
        tag = f"[{name}] step {k} ({step.pair} /{step.mesh} {step.mode})"
        key, before = C.key(step), dict(pipe._plans)
        pool = {n: (t, t.clone()) for n, t in pipe._buf.items() if n in POOLED_OUTPUTS}
        got = outcome(lambda: run(pipe, step, pinned))
        # the pool: a pass writes the head of a longer buffer and nothing behind it
        cells, (fw, fh, _, _) = step.mesh * step.mesh, C.final(step)
        used = {"H": cells * 9, "flat": cells * 9, "canvas": 0 if step.mode == "none" else fw * fh * 3}
        for n, (t, was) in pool.items():
            if pipe._buf[n] is t and not torch.equal(t[used[n]:], was[used[n]:]):
                wrong.append(f"{tag}: the pass wrote behind the first {used[n]} elements of the pooled buffer '{n}'")
        # the plan cache
        after = pipe._plans
        if len(after) > C.PLAN_CAPACITY:
            wrong.append(f"{tag}: {len(after)} plans held")
        for old_key, old in before.items():
            if old_key not in after:
                dropped[old_key] = old          # kept alive: a rebuilt plan cannot be the dropped object at its old address
        if expect == "none":
            if list(after.items()) != list(before.items()):
                wrong.append(f"{tag}: a pass without a picture changed the plans")
        elif expect == "hit":
            if key not in before or after.get(key) is not before[key] or len(after) != len(before):
                wrong.append(f"{tag}: a cached geometry was not served by its plan")
        else:
            if key in before or key not in after or (expect == "rebuilt") != (key in dropped) or after[key] is dropped.get(key):
                wrong.append(f"{tag}: the model says '{expect}'; the plans say otherwise")
            elif list(after)[-1] != key or list(after)[:-1] != list(before)[-(len(after) - 1):]:
                wrong.append(f"{tag}: not the oldest plan was dropped")
        # the inputs
        for a in ARRAYS:
            if getattr(C.pair(step.pair), a).tobytes() != original[step.pair][a].tobytes():
                wrong.append(f"{tag}: the pass wrote into its input '{a}'")
        # the outputs
        if step.expect != "ok":
            if not isinstance(got, ERRORS[step.expect]):
                wrong.append(f"{tag}: {ERRORS[step.expect].__name__} expected, got {type(got).__name__}")
            fresh, calls = alone(native, name, step)
            if not isinstance(fresh, ERRORS[step.expect]) or not (calls is None or isinstance(calls, ERRORS[step.expect])):
                wrong.append(f"{tag}: alone, the step does not raise {ERRORS[step.expect].__name__}")
            continue
        if isinstance(got, Exception):
            wrong.append(f"{tag}: {type(got).__name__}: {got}")
            continue
        check_output(native, name, k, step, got, wrong, totals)
        if k == C.ITEMS["after singular"] and after[key].status_word() != after[key].geo_status:
            wrong.append(f"{tag}: the status word is {after[key].status_word()}, the geometry's bits are {after[key].geo_status}")
        flat, canvas, grid = got
        if step.transfer == "pinned+canvas_out":
            if canvas is None or not np.shares_memory(canvas, pinned["canvas"]):
                wrong.append(f"{tag}: the canvas did not go into canvas_out")
            canvas = None
        mine = [a for a in (flat, canvas, grid) if a is not None]
        for a in mine:
            if any(lo <= a.ctypes.data < hi for lo, hi in page_locked(pipe)):
                wrong.append(f"{tag}: a returned array lies in the pipeline's page-locked memory")
        kept.append((tag, mine, [a.copy() for a in mine]))
    for tag, mine, copies in kept:
        if not all(same(a, b) for a, b in zip(mine, copies)):
            wrong.append(f"{tag}: a later pass wrote into this step's results")
    first, last = kept[0][1], kept[-1][1]
    if not (SEQ[-1] == SEQ[0] and len(first) == len(last) == 3 and all(same(a, b) for a, b in zip(first, last))):
        wrong.append(f"[{name}] the last step is the first again and does not give its bytes")
    bar = "not held to the bar" if name == "moments24" else f"rmse-delta max {totals['rmse']:.3e} px"
    print(f"[{name}] {len(SEQ)} steps: {bar}, {totals['pixels']} pixels and {totals['flat']} .mat entries differ from the oracle's")
    del pipe
    if ctx is not None:
        ctx.close()
    return wrong


@pytest.mark.parametrize("name", list(CONTEXTS))
def test_one_pipeline_over_the_sequence(native, name):
    """``Pipeline()``, ``fused_max_cells = 0`` (every mesh takes K1 + K2, whose tail writes the records) and ``moments = 24``."""
    wrong = run_sequence(native, name)
    assert not wrong, "\n".join([f"{len(wrong)} findings:"] + wrong)


def test_device_marks_of_a_traced_pipeline(native):
    """``trace = True`` over the same sequence: only ``device_marks`` is looked at.  Its names come in the order that
    ``pipeline_sequence_cases.marks`` documents, and its times do not decrease.  (Marks of one stream are ordered by the stream,
    "image here" follows "image up (side)" through the event the main stream waits for; that "main: first enqueue" follows
    "image up (side)" rests on the host set-up taking longer than a page-locked copy of at most 192 KB.)"""
    from cvx_proj_amd.pipeline import Pipeline
    pipe = Pipeline()
    pipe.trace = True
    big = max(C.pair(s.pair).img.size for s in SEQ)
    pinned = {"img": pipe.pinned_array((big,)), "center": pipe.pinned_array((big,)),
              "canvas": pipe.pinned_array((max(C.final(s)[0] * C.final(s)[1] for s in SEQ) * 3,))}
    wrong = []
    for k, step in enumerate(SEQ):
        got = outcome(lambda: run(pipe, step, pinned))
        if step.expect != "ok":
            continue
        if isinstance(got, Exception):
            wrong.append(f"step {k}: {type(got).__name__}: {got}")
            continue
        names, times = [n for n, _ in pipe.device_marks], [t for _, t in pipe.device_marks]
        if names != C.marks(step):
            wrong.append(f"step {k}: marks {names}, wanted {C.marks(step)}")
        if times[0] != 0 or any(b < a for a, b in zip(times, times[1:])):
            wrong.append(f"step {k}: times {times} of {names}")
    assert not wrong, "\n".join(wrong)


@pytest.mark.parametrize("flag", ["--warp", "--stitch"])
def test_command_line_loop_resident_or_not(native, tmp_path, flag):
    """``--cases 1-2 --imgs 1,4 --resident`` takes ONE Pipeline through four pairs: the four .mat bodies (after the 128-byte header,
    which carries the creation time) and the four canvases are those of the same command without ``--resident``, and the pairs
    differ from one another."""
    from cvx_proj_amd.apap import main
    jobs = [(c, i) for c in (1, 2) for i in (1, 4)]
    out = {}
    for kind, extra in (("resident", ["--resident"]), ("calls", [])):
        d = tmp_path / kind
        d.mkdir()
        assert main(["--synth", "C1", "--cases", "1-2", "--imgs", "1,4", "--out-prefix", str(d / "res") + "/"] + extra
                    + [flag, str(d / "canvas.npy")]) == 0
        out[kind] = ([(d / "res" / f"case{c}" / f"H3{i}_apap.mat").read_bytes()[128:] for c, i in jobs],
                     [np.load(d / f"canvas_case{c}_{i}.npy") for c, i in jobs])
    for a, b in zip(out["resident"][0], out["calls"][0]):
        assert len(a) > 400 * 9 * 8 and a == b
    for a, b in zip(out["resident"][1], out["calls"][1]):
        assert a.dtype == np.uint8 and a.ndim == 3 and a.any() and same(a, b)
    assert len(set(out["calls"][0])) == 4 and len({c.tobytes() for c in out["calls"][1]}) == 4
