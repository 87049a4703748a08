"""GICP_HIP measurements on one GPU; prints one JSON line.

  registrations/s of the 32 x 65,536 loop shard (synth.loop_batch, factory settings, resident candidates, fitness included), outer and
  BFGS inner iterations, evaluation passes and round launches per pair of that shard, and single-pair latency at 65,536 (kitti_pair)
  and 200,000 (indoor_pair) points.  `shard_round_ms` / `shard_round_launches`: the round launches of one shard without the fitness
  pass, event-timed.  Kernel table: `--shard-only` runs K shards without fitness and nothing else, for
  `rocprofv3 --kernel-trace --stats -- python scripts/bench_pcl_gicp.py --shard-only`.

usage: python scripts/bench_pcl_gicp.py [--warmup W] [--steps K] [--shard-only]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--shard-only", action="store_true", help="K shards without fitness, nothing else (for a rocprofv3 run)")
    a = ap.parse_args()
    torch.cuda.init()
    out = {"metric": "gicp_hip"}

    tgt, cands, guesses, _ = synth.loop_batch(n_candidates=32, n_points=65536, seed=40, distinct_scans=32)
    reg = Registration("GICP_HIP", device=0)
    ct = reg.make_cloud(tgt)
    cs = [reg.make_cloud(c) for c in cands]
    g = np.stack([np.asarray(x, np.float32) for x in guesses])

    def shard():
        reg.setInputTarget(ct)
        return reg.align_batch(cs, g, compute_fitness=True)

    if a.shard_only:
        reg.setInputTarget(ct)
        for _ in range(a.warmup):
            reg.align_batch(cs, g, compute_fitness=False)
        torch.cuda.synchronize()
        for _ in range(a.steps):
            reg.align_batch(cs, g, compute_fitness=False)
        print(json.dumps({"metric": "gicp_hip_shard_only", "shards": a.steps}))
        return
    t = timed(shard, a.warmup, a.steps)
    res = shard()
    iters = [r["iterations"] for r in res]
    inner = [int(reg.pcl_gicp_trajectory(i)["inner"].sum()) for i in range(32)]
    out["shard_registrations_per_s"] = 32.0 / t
    out["shard_ms"] = 1e3 * t
    out["outer_iterations_per_pair_mean"] = float(np.mean(iters))
    out["outer_iterations_per_pair_max"] = int(np.max(iters))
    out["inner_iterations_per_pair_mean"] = float(np.mean(inner))
    out["passes_per_pair_mean"] = float(np.mean([r["evaluations"] for r in res]))   # correspondence + evaluation passes
    out["converged"] = int(sum(bool(r["converged"]) for r in res))
    # the round launches alone: no fitness pass, covariances and indices already built
    reg.setInputTarget(ct)
    reg.align_batch(cs, g, compute_fitness=False)
    reg.profile_enable(True)
    reg.profile_reset()
    res = reg.align_batch(cs, g, compute_fitness=False)
    ms, launches = reg.profile_get(L.K_NN_SEARCH)
    reg.profile_enable(False)
    out["shard_round_ms"] = ms
    out["shard_round_launches"] = launches   # one per round of the slowest pair, queued in chunks of 8 (up to 15 idle at the end)
    out["shard_round_us_per_launch"] = 1e3 * ms / max(launches, 1)

    for name, (T, S, _) in (("65536", synth.kitti_pair()), ("200000", synth.indoor_pair())):
        r1 = Registration("GICP_HIP", device=0)
        r1.setInputTarget(T)
        r1.setInputSource(S)
        out[f"single_ms_{name}"] = 1e3 * timed(lambda: r1.align(), a.warmup, a.steps)
        out[f"single_iterations_{name}"] = r1.last_result.iterations
        out[f"single_passes_{name}"] = r1.last_result.evaluations
    print(json.dumps(out))


if __name__ == "__main__":
    main()
