"""The price of batch-independent results (dgs_set_batch_independent): loop ticks with the switch off and on, alternating
in one process on ONE handle (the switch may change between calls).  Not bench.py: recorded in DESIGN.md 6p, not gated.

  big    32 candidates of 65,536 points against one 65,536-point target (synth.loop_batch, bench.py's step): one align_batch
  tick   10 new keyframes x 3 candidates of ~26.7 k points (synth.vlp16_stream, scripts/bench_tick_pairs.py's shape):
         FAST_GICP one align_pairs over the 30 pairs; FAST_VGICP, whose target model lives on the handle, setInputTarget + align_batch per keyframe

FAST_GICP and FAST_VGICP run both shapes; NDT_OMP (upstream order, DIRECT7, resolution 1.0: bench.py's registration) runs `big`, which
re-measures the fixed-slices figure of ndt_strict.h through the setter.  Every cloud is resident and has been registered once in both
modes before anything is timed.  Fitness is computed in every leg.  Host clocks around calls that end in a stream synchronisation.  Per
leg: `--warmup` ticks of each mode, then `--repeats` ticks of each, taken alternately; the median of each mode; `--runs` repetitions of
that, medians in order.  One JSON line per leg with ms per tick and the on / off ratio of the run medians' medians.

    python scripts/bench_batch_independent.py [--legs FAST_GICP:big FAST_GICP:tick FAST_VGICP:big FAST_VGICP:tick NDT_OMP:big] [--repeats 50] [--warmup 5] [--runs 3]
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

ALL_LEGS = ["FAST_GICP:big", "FAST_GICP:tick", "FAST_VGICP:big", "FAST_VGICP:tick", "NDT_OMP:big"]


def make_registration(method):
    from delta_graph_slam_amd import _lib as L
    from delta_graph_slam_amd.registration import Registration
    if method == "FAST_GICP":
        return Registration("FAST_GICP", device=0, gicp_max_correspondence_distance=2.0, transformation_epsilon=0.1)   # the launch files' values
    if method == "FAST_VGICP":
        return Registration("FAST_VGICP", device=0, vgicp_resolution=1.0, transformation_epsilon=0.1)
    return Registration("NDT_OMP", device=0, ndt_resolution=1.0, ndt_search_method=L.NDT_SEARCH["DIRECT7"], transformation_epsilon=0.01, maximum_iterations=64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", nargs="+", default=ALL_LEGS, choices=ALL_LEGS)
    ap.add_argument("--repeats", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--runs", type=int, default=3)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_batch_independent.py measures on the GPU; none is available")
    from delta_graph_slam_amd import synth

    data = {}

    def big():
        if "big" not in data:
            data["big"] = synth.loop_batch(n_candidates=32, n_points=65536, seed=40)
        return data["big"]

    def stream():
        if "tick" not in data:
            data["tick"] = synth.vlp16_stream(n_frames=10 + 12)
        return data["tick"]

    for leg in args.legs:
        method, shape = leg.split(":")
        reg = make_registration(method)
        if shape == "big":
            tgt, sources, guesses, _ = big()
            reg.setInputTarget(reg.make_cloud(tgt))
            srcs = [reg.make_cloud(s) for s in sources]
            g = np.asarray(guesses, np.float32)

            def tick():
                return reg.align_batch(srcs, g, compute_fitness=True)
            shape_note = dict(pairs=len(sources), points=int(sources[0].shape[0]))
        else:
            frames, poses = stream()
            resident = [reg.make_cloud(f) for f in frames]
            rng = np.random.default_rng(0)
            plan = []
            for i in range(10):
                src = [10 + (i * 3 + j) % 12 for j in range(3)]
                gs = [(np.linalg.inv(poses[i]) @ poses[s] @ synth.make_transform(rng.uniform(-0.05, 0.05, 3), rng.uniform(-0.005, 0.005, 3))).astype(np.float32) for s in src]
                plan.append((i, src, gs))
            if method == "FAST_GICP":
                def tick():
                    return reg.align_pairs([resident[i] for i, src, _ in plan for _ in src], [resident[s] for _, src, _ in plan for s in src],
                                           [gg for _, _, gs in plan for gg in gs], compute_fitness=True)
            else:
                def tick():
                    out = []
                    for i, src, gs in plan:
                        reg.setInputTarget(resident[i])
                        out += reg.align_batch([resident[s] for s in src], gs, compute_fitness=True)
                    return out
            shape_note = dict(pairs=30, points=int(frames[0].shape[0]))

        def run(on):
            reg.set_batch_independent(on)
            return tick()

        a, b = run(False), run(True)   # caches every index, covariance and voxel map in both modes; and the two modes are compared
        worst = max(float(np.abs(x["T"] - y["T"]).max()) for x, y in zip(a, b))
        same_iters = sum(x["iterations"] == y["iterations"] for x, y in zip(a, b))
        med = {False: [], True: []}
        for _ in range(args.runs):
            for _ in range(args.warmup):
                run(False)
                run(True)
            ts = {False: [], True: []}
            for _ in range(args.repeats):   # alternating: whatever else the machine does falls on both
                for on in (False, True):
                    t0 = time.perf_counter()
                    run(on)
                    ts[on].append((time.perf_counter() - t0) * 1e3)
            for on in med:
                med[on].append(round(statistics.median(ts[on]), 4))
        off_ms, on_ms = statistics.median(med[False]), statistics.median(med[True])
        print(json.dumps(dict(leg=leg, **shape_note, repeats=args.repeats, warmup=args.warmup, off_ms=med[False], on_ms=med[True],
                              ratio_on_over_off=round(on_ms / off_ms, 4), max_abs_T_difference_off_on=worst,
                              pairs_with_equal_iterations=same_iters, evaluations=int(sum(x["evaluations"] for x in b)))), flush=True)
        reg.close()


if __name__ == "__main__":
    main()
