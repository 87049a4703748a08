"""-m gpu: bench.py prints ONE JSON line with the driver's contract keys (small workload, no CPU baseline, no profiler children);
a plain run reports the timed steps alone and --dump-outputs writes what the last timed step computed."""
import json
import os
import time
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_line_has_the_contract_keys():
    out = subprocess.check_output([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "2", "--warmup", "1", "--pairs", "4", "--points", "8192",
                                   "--full", "--no-cpu-baseline", "--no-traffic"], cwd=ROOT, stderr=subprocess.DEVNULL, timeout=600).decode()
    lines = [l for l in out.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config",
              "roofline"):
        assert k in d, k
    assert d["n_gpus"] == 1 and d["steps"] == 2 and d["warmup"] == 1 and d["higher_is_better"] is True and d["scaling"] == "weak"
    assert d["vs_baseline"] is None and d["data"] == "synthetic" and "workload" in d["config"]
    assert d["value"] > 0 and abs(d["value"] - 4 * 2 / (d["ms_per_step"] * 2e-3)) <= 1e-6 * d["value"]
    r = d["roofline"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert k in r, k
    assert r["bound"] == "hbm" and r["peak"] == 8000.0 and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-12


def test_plain_run_times_the_steps_only_and_dumps_the_last_step(tmp_path):
    d = tmp_path / "out"
    t0 = time.perf_counter()
    out = subprocess.check_output([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--pairs", "4",
                                   "--points", "8192", "--dump-outputs", str(d)], cwd=ROOT, stderr=subprocess.DEVNULL, timeout=600).decode()
    wall = time.perf_counter() - t0
    lines = [l for l in out.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    r = json.loads(lines[0])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in r, k
    assert r["steps"] == 3 and r["warmup"] == 1 and r["value"] > 0 and abs(r["value"] - 4 * 3 / (r["ms_per_step"] * 3e-3)) <= 1e-6 * r["value"]
    for k in ("roofline", "cpu_baseline", "parity_gate", "other_order", "fast_value"):   # the side measurements are --full's
        assert k not in r, k
    assert wall < 120, wall
    rec = np.load(d / "records.npy")
    assert rec.dtype == np.float64 and rec.shape == (4, 20) and np.array_equal(rec[:, 0], np.arange(4))
    best, score = np.load(d / "loop_candidate_score.npy")
    conv = rec[:, 1] > 0.5
    assert conv.any() and int(best) == int(np.flatnonzero(conv)[np.argmin(rec[conv, 2])]) and score == rec[int(best), 2]
    T = np.load(d / "loop_relative_pose.npy")
    assert T.dtype == np.float64 and np.array_equal(T, rec[int(best), 4:20].reshape(4, 4).astype(np.float32))
    assert np.load(d / "loop_relative_pose2D.npy").shape == (3, 3)
