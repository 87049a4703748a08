"""A loop-detection tick of K new keyframes x c candidates over resident VLP-16-shaped clouds, FAST_GICP or GICP_HIP (--method), two ways,
alternating in one process.  Not bench.py: recorded in DESIGN.md 6n (FAST_GICP) and 6o (GICP_HIP), not gated.

  seq    today's sequence: per new keyframe setInputTarget(cloud) + align_batch(its c candidates)   (K calls pairs, K chains of rounds)
  pairs  one align_pairs over all K x c (new keyframe, candidate, guess) pairs                       (one chain of rounds)

Clouds are frames of synth.vlp16_stream; new keyframe i is frame i, its candidates are later frames of the same drive, the guess is the
stream's relative pose moved by a few centimetres.  Every cloud is a DeviceCloud; both ways run once before anything is timed, so the
indices and covariances of all clouds exist in both legs.  Fitness is computed in both.  Host clocks around calls that end in a stream
synchronisation (both return their results to the host).  Per (K, c): the median of `--repeats` ticks of each way, taken alternately, and
over `--runs` repetitions of that the medians in order; the kernel launches of one tick of each way from dgs_profile_get (a run of its
own with the profiler on, after the timed ones), and the poses of the two ways compared first.  One JSON line per (K, c).

FAST_GICP runs with the launch files' values; GICP_HIP with the factory settings, as scripts/bench_pcl_gicp.py does.  For GICP_HIP the
evaluations and the score of the two ways are compared too (its sums are formed over fixed slices: bit-equality is expected).

    python scripts/bench_tick_pairs.py [--method FAST_GICP|GICP_HIP] [--keyframes 1 4 10] [--candidates 1 3 8] [--repeats 50] [--warmup 5] [--runs 3]

--fresh measures the first-use tick instead: per (K, c) one align_pairs over K + K c clouds that nothing has seen before, so
that their indices and covariances are made inside the timed call; per run the median tick and, from profiled ticks, the device time and
the passes of the covariance stage alone (--keyframes 3 --candidates 10: 33 clouds).
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
    ap.add_argument("--keyframes", type=int, nargs="+", default=[1, 4, 10])
    ap.add_argument("--candidates", type=int, nargs="+", default=[1, 3, 8])
    ap.add_argument("--repeats", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--method", choices=["FAST_GICP", "GICP_HIP"], default="FAST_GICP")
    ap.add_argument("--fresh", action="store_true", help="the first-use tick instead: every cloud of every timed align_pairs is a new DeviceCloud (DESIGN.md 6s)")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_tick_pairs.py measures on the GPU; none is available")
    from delta_graph_slam_amd import _lib as L
    from delta_graph_slam_amd import synth
    from delta_graph_slam_amd.registration import Registration

    K_max, c_max = max(args.keyframes), max(args.candidates)
    n_pool = 12                                   # candidate frames, shared between the new keyframes as old keyframes are in a real graph
    frames, poses = synth.vlp16_stream(n_frames=K_max + n_pool)
    if args.method == "GICP_HIP":
        reg = Registration("GICP_HIP", device=0)   # the factory settings (scripts/bench_pcl_gicp.py)
    else:
        reg = Registration("FAST_GICP", device=0, gicp_max_correspondence_distance=2.0, transformation_epsilon=0.1)   # the launch files' values
    rng = np.random.default_rng(0)
    if args.fresh:
        # The first-use tick: K new keyframes x c candidates, K + K c clouds that nothing has seen before -- their indices and covariances
        # are made inside the timed align_pairs.  Per repeat the clouds are uploaded anew (not timed).  Per run the median tick and, from a
        # profiled tick, the device time and the passes of the covariance stage alone.
        for K in args.keyframes:
            for c in args.candidates:
                fr, ps = synth.vlp16_stream(n_frames=K + K * c)
                tgt = [i for i in range(K) for _ in range(c)]
                src = [K + i * c + j for i in range(K) for j in range(c)]
                g = [(np.linalg.inv(ps[t]) @ ps[s]).astype(np.float32) for t, s in zip(tgt, src)]

                def one(profile=False):
                    clouds = [reg.make_cloud(f) for f in fr]
                    reg.synchronize()
                    if profile:
                        reg.profile_enable(True)
                        reg.profile_reset()
                    t0 = time.perf_counter()
                    reg.align_pairs([clouds[t] for t in tgt], [clouds[s] for s in src], g, compute_fitness=True)
                    ms = (time.perf_counter() - t0) * 1e3
                    cov = reg.profile_get(L.K_GICP_COVARIANCE) if profile else None
                    if profile:
                        reg.profile_enable(False)
                    for cl in clouds:
                        cl.close()
                    return ms, cov

                med, cov_ms, cov_n = [], [], 0
                for _ in range(args.runs):
                    for _ in range(args.warmup):
                        one()
                    med.append(round(statistics.median(one()[0] for _ in range(args.repeats)), 4))
                    cov = [one(profile=True)[1] for _ in range(5)]
                    cov_ms.append(round(statistics.median(x[0] for x in cov), 4))
                    cov_n = cov[0][1]
                print(json.dumps(dict(fresh=True, method=args.method, K=K, c=c, clouds=K + K * c, points_per_cloud=int(fr[0].shape[0]), tick_ms=med,
                                      covariance_stage_ms=cov_ms, covariance_passes=cov_n)), flush=True)
        return
    resident = [reg.make_cloud(f) for f in frames]

    def tick(K, c):
        """-> per new keyframe (target index, [source indices], [guesses])"""
        out = []
        for i in range(K):
            src = [K_max + (i * 3 + j) % n_pool for j in range(c)]
            g = [(np.linalg.inv(poses[i]) @ poses[s] @ synth.make_transform(rng.uniform(-0.05, 0.05, 3), rng.uniform(-0.005, 0.005, 3))).astype(np.float32)
                 for s in src]
            out.append((i, src, g))
        return out

    def run_seq(t):
        res = []
        for i, src, g in t:
            reg.setInputTarget(resident[i])
            res += reg.align_batch([resident[s] for s in src], g, compute_fitness=True)
        return res

    def run_pairs(t):
        return reg.align_pairs([resident[i] for i, src, _ in t for _ in src], [resident[s] for _, src, _ in t for s in src],
                               [gg for _, _, g in t for gg in g], compute_fitness=True)

    def launches(fn, t):
        reg.profile_enable(True)
        reg.profile_reset()
        fn(t)
        n = {name: reg.profile_get(k)[1] for name, k in (("nn_search", L.K_NN_SEARCH), ("gicp_linearize", L.K_GICP_LINEARIZE), ("gicp_covariance", L.K_GICP_COVARIANCE))}
        reg.profile_enable(False)
        return n

    print(json.dumps(dict(method=args.method, points_per_cloud=[int(f.shape[0]) for f in frames[:3]], repeats=args.repeats, warmup=args.warmup, runs=args.runs)), flush=True)
    for K in args.keyframes:
        for c in args.candidates:
            t = tick(K, c)
            a, b = run_seq(t), run_pairs(t)   # caches every index and covariance; and the two ways must agree
            worst = max(float(np.abs(x["T"] - y["T"]).max()) for x, y in zip(a, b))
            same_counts = all(x["converged"] == y["converged"] and x["iterations"] == y["iterations"] for x, y in zip(a, b))
            same_bits = all(np.array_equal(x["T"], y["T"]) and x["evaluations"] == y["evaluations"] and x["score"] == y["score"] for x, y in zip(a, b))
            med = {"seq": [], "pairs": []}
            for _ in range(args.runs):
                for _ in range(args.warmup):
                    run_seq(t)
                    run_pairs(t)
                ts = {"seq": [], "pairs": []}
                for _ in range(args.repeats):   # alternating: whatever else the machine does falls on both
                    for name, fn in (("seq", run_seq), ("pairs", run_pairs)):
                        t0 = time.perf_counter()
                        fn(t)
                        ts[name].append((time.perf_counter() - t0) * 1e3)
                for name in med:
                    med[name].append(round(statistics.median(ts[name]), 4))
            print(json.dumps(dict(K=K, c=c, pairs=K * c, seq_ms=med["seq"], pairs_ms=med["pairs"],
                                  pairs_faster_in_all_runs=all(p < s for p, s in zip(med["pairs"], med["seq"])),
                                  launches_seq=launches(run_seq, t), launches_pairs=launches(run_pairs, t),
                                  iterations=[x["iterations"] for x in a], evaluations=[x["evaluations"] for x in a], max_abs_T_difference=worst,
                                  same_flags_and_iterations=same_counts, same_transform_evaluations_and_score_bits=same_bits)), flush=True)


if __name__ == "__main__":
    main()
