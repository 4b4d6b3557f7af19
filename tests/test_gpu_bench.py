"""bench.py on one GPU: a plain run prints the headline line alone (and writes --dump-outputs); --full adds the other objects
to the same line."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = {"metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "n_gpus", "steps", "warmup", "config", "warp",
            "solve_ms_per_step", "pair_per_rank"}
FULL_ONLY = {"extra_steps", "kernels_ms", "roofline", "roofline_warp", "standalone", "configs", "pairs", "cells", "call_level",
             "cpu_baseline"}


def run_bench(*args):
    env = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT", "APAP_BENCH_SELFTEST", "APAP_BENCH_FORCE_GROUP"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--config", "C2", "--steps", "3", "--warmup", "1", *args],
                       env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def test_plain_run_prints_the_headline_alone(tmp_path):
    d = run_bench("--dump-outputs", str(tmp_path))
    assert HEADLINE <= set(d) and not FULL_ONLY & set(d), sorted(d)
    assert d["unit"] == "homographies/s" and d["higher_is_better"] is True and d["dtype"] == "f64" and d["steps"] == 3
    assert d["value"] > 0 and d["warp"]["value"] > 0
    assert d["ms_per_step"] == pytest.approx(d["solve_ms_per_step"] + d["warp"]["ms_per_step"])
    assert d["pair_per_rank"]["value"] == d["value"]
    assert sorted(os.listdir(tmp_path)) == ["H.npy", "canvas_sample.npy", "canvas_sample_index.npy"]


def test_full_run_adds_the_other_objects_to_the_headline():
    d = run_bench("--full", "--no-cpu-baseline", "--no-call-level", "--no-cells", "--no-c5", "--no-configs", "--cold-mb", "0")
    assert HEADLINE <= set(d), sorted(d)
    assert d["extra_steps"] == 3 and d["kernels_ms"]["assemble"] > 0 and 0 < d["roofline"]["frac"] < 1
    assert d["standalone"]["value"] > 0 and d["pairs"] is None and d["cells"] is None and "cpu_baseline" not in d
