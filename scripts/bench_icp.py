"""ICP_HIP measurements on one GPU; prints one JSON line.

  registrations/s of the 32 x 65,536 loop shard (synth.loop_batch, factory settings, resident candidates, fitness included),
  iterations per pair of that shard, single-pair latency at 65,536 (kitti_pair) and 200,000 (indoor_pair)
  points, the reciprocal mode's cost on the kitti pair, and the algorithmic bytes of the shard's correspondence passes (from shapes and
  pass counts).  `shard_iterate_ms` / `shard_iterate_launches`: the iteration launches of one shard without the fitness pass, event-timed.
  HBM fraction: `--shard-only` runs K shards without fitness and nothing else; under `rocprofv3 --kernel-trace --stats` divide
  K x `shard_algorithmic_bytes` by the total time of icp_iterate_kernel<false>.

usage: python scripts/bench_icp.py [--warmup W] [--steps K] [--shard-only]
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


def shard_bytes(res, clouds):
    """Algorithmic bytes of a shard's correspondence passes: per pass and source point, the point read (16 B) and written (16 B), its
    source-index record (16 B), one target index leaf (8 x 16 B) at least, the target point gathered (16 B); one 256-B row per slice."""
    total = 0
    for r, c in zip(res, clouds):
        n = len(c)
        total += r["evaluations"] * (n * (16 + 16 + 16 + 8 * 16 + 16) + ((n + 255) // 256) * 256)
    return int(total)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--shard-only", action="store_true", help="K shards without fitness, nothing else (for a rocprofv3 run)")
    a = ap.parse_args()
    torch.cuda.init()
    out = {"metric": "icp_hip"}

    tgt, cands, guesses, _ = synth.loop_batch(n_candidates=32, n_points=65536, seed=40, distinct_scans=32)
    reg = Registration("ICP_HIP", device=0)
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
            res = reg.align_batch(cs, g, compute_fitness=False)
        print(json.dumps({"metric": "icp_hip_shard_only", "shards": a.steps, "shard_algorithmic_bytes": shard_bytes(res, cands)}))
        return
    t = timed(shard, a.warmup, a.steps)
    res = shard()
    iters = [r["iterations"] for r in res]
    out["shard_registrations_per_s"] = 32.0 / t
    out["shard_ms"] = 1e3 * t
    out["iterations_per_pair_mean"] = float(np.mean(iters))
    out["iterations_per_pair_max"] = int(np.max(iters))
    # the iteration launches alone: no fitness pass (it is timed under the same id), index and clouds already built
    reg.setInputTarget(ct)
    reg.align_batch(cs, g, compute_fitness=False)
    reg.profile_enable(True)
    reg.profile_reset()
    res = reg.align_batch(cs, g, compute_fitness=False)
    ms, launches = reg.profile_get(L.K_NN_SEARCH)
    reg.profile_enable(False)
    out["shard_iterate_ms"] = ms
    out["shard_iterate_launches"] = launches        # queued in chunks of 4: up to 3 after the last pair finished do no work
    out["shard_correspondence_passes"] = int(sum(r["evaluations"] for r in res))
    out["shard_algorithmic_bytes"] = shard_bytes(res, cands)
    out["shard_iterate_TBps_event_timed"] = out["shard_algorithmic_bytes"] / (ms * 1e-3) / 1e12

    for name, (T, S, _) in (("65536", synth.kitti_pair()), ("200000", synth.indoor_pair())):
        r1 = Registration("ICP_HIP", device=0)
        r1.setInputTarget(T)
        r1.setInputSource(S)
        out[f"single_ms_{name}"] = 1e3 * timed(lambda: r1.align(), a.warmup, a.steps)
        out[f"single_iterations_{name}"] = r1.last_result.iterations
    T, S, _ = synth.kitti_pair()
    rr = Registration("ICP_HIP", device=0, icp_use_reciprocal_correspondences=True)
    rr.setInputTarget(T)
    rr.setInputSource(S)
    out["reciprocal_single_ms_65536"] = 1e3 * timed(lambda: rr.align(), a.warmup, a.steps)
    out["reciprocal_iterations_65536"] = rr.last_result.iterations
    print(json.dumps(out))


if __name__ == "__main__":
    main()
