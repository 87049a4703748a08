"""PCL_NDT_HIP measurements on one GPU (recorded in DESIGN.md section 6i, not gated); prints one JSON line.

  registrations/s of the 32 x 65,536 loop shard (synth.loop_batch, factory settings -- resolution 0.5 --, resident candidates, fitness
  included), iterations and evaluations per pair of that shard, single-pair latency at 65,536 (kitti_pair) and 200,000 (indoor_pair)
  points; beside each the nearest existing work on the same inputs: NDT_OMP with the KDTREE neighbourhood in the upstream order.
  `--runs R` repeats every timing R times (each the median of --steps calls) and reports the runs and their spread (max - min) / median.

usage: python scripts/bench_pcl_ndt.py [--warmup W] [--steps K] [--runs R]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from delta_graph_slam_amd import _lib as L  # noqa: E402
from delta_graph_slam_amd import synth  # noqa: E402
from delta_graph_slam_amd.registration import Registration  # noqa: E402


def timed(fn, warmup, steps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(steps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts))


def runs_of(fn, warmup, steps, runs):
    ms = [1e3 * timed(fn, warmup, steps) for _ in range(runs)]
    return {"ms_runs": ms, "ms": float(np.median(ms)), "spread": float((max(ms) - min(ms)) / np.median(ms))}


METHODS = (("pcl_ndt_hip", "PCL_NDT_HIP", {}),
           ("ndt_omp_kdtree", "NDT_OMP", {"ndt_search_method": L.NDT_SEARCH["KDTREE"]}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--runs", type=int, default=3)
    a = ap.parse_args()
    torch.cuda.init()
    out = {"metric": "pcl_ndt_hip"}

    tgt, cands, guesses, _ = synth.loop_batch(n_candidates=32, n_points=65536, seed=40, distinct_scans=32)
    g = np.stack([np.asarray(x, np.float32) for x in guesses])
    for key, method, extra in METHODS:
        reg = Registration(method, device=0, **extra)
        ct = reg.make_cloud(tgt)
        cs = [reg.make_cloud(c) for c in cands]

        def shard():
            reg.setInputTarget(ct)
            return reg.align_batch(cs, g, compute_fitness=True)

        t = runs_of(shard, a.warmup, a.steps, a.runs)
        res = shard()
        out[key] = {"shard": dict(t, registrations_per_s=32.0 / (t["ms"] * 1e-3),
                                  iterations_per_pair_mean=float(np.mean([r["iterations"] for r in res])),
                                  evaluations_per_pair_mean=float(np.mean([r["evaluations"] for r in res])),
                                  converged=int(sum(r["converged"] for r in res)))}
        reg.close()
    for name, (T, S, _) in (("65536", synth.kitti_pair()), ("200000", synth.indoor_pair())):
        for key, method, extra in METHODS:
            r1 = Registration(method, device=0, **extra)
            r1.setInputTarget(T)
            r1.setInputSource(S)
            t = runs_of(lambda: r1.align(), a.warmup, a.steps, a.runs)
            out[key][f"single_{name}"] = dict(t, iterations=r1.last_result.iterations, evaluations=r1.last_result.evaluations)
            r1.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
