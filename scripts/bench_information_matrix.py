"""A tick's information matrices (apps/delta_graph_slam_nodelet.cpp:572,820) three ways, alternating in one process.  Not bench.py:
recorded in DESIGN.md 6k, not gated.

Keyframes are synth.hdl64_scan clouds of 65,536 points 2 m apart; edge e is (k_{e+1}, k_e, pose_{e+1}^-1 pose_e), the odometry chain.
  a        the route before the batch call: B calls of dgs_calc_fitness_score on host arrays (two uploads, an index build, a walk, a wait each)
  b        dgs_calc_fitness_score_batch_clouds on resident clouds that have no index yet: one batched build, one walk (the uploads are not timed)
  b_upload the same with the B + 1 uploads (dgs_cloud_create) inside the timed window
  c        the batch call on resident clouds whose indices exist
Host clocks around calls that end in a stream synchronisation.  One JSON line per B: the median of `--repeats` calls, and over `--runs`
repetitions of that the lowest and highest median (the run-to-run spread); the scores of the three ways are compared first.

    python scripts/bench_information_matrix.py [--edges 1 4 12] [--repeats 20] [--warmup 3] [--runs 3] [--points 65536]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--edges", type=int, nargs="+", default=[1, 4, 12])
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--points", type=int, default=65536)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_information_matrix.py measures on the GPU; none is available")
    from delta_graph_slam_amd import synth
    from delta_graph_slam_amd.registration import Registration
    reg = Registration("NDT_OMP", device=0)
    n_key = max(args.edges) + 1
    scans = [synth.hdl64_scan((2.0 * i, 0.0, 0.0), 50 + i, args.points) for i in range(n_key)]
    clouds = [s[0] for s in scans]
    rel = [(np.linalg.inv(scans[e + 1][1]) @ scans[e][1]).astype(np.float32) for e in range(n_key - 1)]

    def median_ms(fn, setup=None):
        for _ in range(args.warmup):
            fn(setup() if setup else None)
        t, keep = [], None
        for _ in range(args.repeats):
            keep = None   # what the last call made goes now (dgs_cloud_destroy waits for the device), outside the window
            s = setup() if setup else None
            t0 = time.perf_counter()
            keep = fn(s)
            t.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(t)

    for B in args.edges:
        def way_a(_):
            return [reg.calc_fitness_score(clouds[e + 1], clouds[e], rel[e]) for e in range(B)]

        def fresh():
            return [reg.make_cloud(clouds[i]) for i in range(B + 1)]

        def batch(dc):
            return reg.calc_fitness_score_batch(dc[1:B + 1], dc[0:B], rel[:B])

        def way_b_upload(_):
            dc = fresh()
            return dc, batch(dc)

        resident = fresh()
        sa, sc = np.array(way_a(None)), batch(resident)
        warm_counts = (batch(resident), reg.fitness_batch_counts())[1]
        sb = batch(fresh())
        cold_counts = reg.fitness_batch_counts()
        assert np.array_equal(sb, sc) and np.all(np.abs(sa - sc) <= 1e-12 * sa), (sa, sb, sc)
        ways = {"a": (way_a, None), "b": (batch, fresh), "b_upload": (way_b_upload, None), "c": (lambda _: batch(resident), None)}
        meds = {k: [] for k in ways}
        for _ in range(args.runs):                 # alternating: a, b, b_upload, c, a, b, ...
            for k, (fn, setup) in ways.items():
                meds[k].append(median_ms(fn, setup))
        row = {k: [round(statistics.median(v), 4), round(min(v), 4), round(max(v), 4)] for k, v in meds.items()}
        print(json.dumps(dict(what="information_matrix_fitness", edges=B, points=args.points, ms=row, cold_counts=cold_counts, warm_counts=warm_counts,
                              repeats=args.repeats, warmup=args.warmup, runs=args.runs, columns="median, lowest, highest median of the runs")), flush=True)


if __name__ == "__main__":
    main()
