"""Frames per second of B scan-matching odometry streams on one GPU: ScanMatchingOdometryFleet (one step advances all B streams) against
the same B streams run one after another through B ScanMatchingOdometry objects, the path as it was before the fleet existed.

    python scripts/bench_odometry_fleet.py [--frames 200] [--streams 1 2 4 8 16 32] [--repeats 3] [--out profiles/odometry_fleet.jsonl]

Every stream is a copy of synth.vlp16_stream (VLP-16-shaped frames of ~26k points, resident on the device), down-sampled with VOXELGRID
0.1 m and registered with FAST_GICP at the launch file's values (k 20, max correspondence distance 2.0, epsilon 0.1), keyframe thresholds
as scripts/bench_configs.py's cfg3.  Per B and repeat the two paths are timed in turn in this one process, each over the whole stream
after a warm-up pass over its first frames; a pass ends with the device idle (both paths wait for their results on the host).  Per B a
profiled step then counts what the library counts: launches and host waits of the batched down-sampling and of the index build and
scoring calls, and the profiler's launch slots of the registration rounds.  Numbers are recorded, not gated.  Needs a GPU."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

KEYFRAMES = dict(keyframe_delta_trans=1.0, keyframe_delta_angle=1.0, keyframe_delta_time=1e9)
DOWN = dict(downsample_method="VOXELGRID", downsample_resolution=0.1)


def make_registration():
    from delta_graph_slam_amd.registration import Registration
    return Registration("FAST_GICP", gicp_max_correspondence_distance=2.0, transformation_epsilon=0.1)


def run_solo(odos, clouds, frames):
    traj = None
    for k in frames:
        traj = [o.matching(0.1 * k, clouds[k]) for o in odos]
    return traj


def run_fleet(fleet, clouds, frames):
    traj = None
    for k in frames:
        traj = fleet.step([0.1 * k] * fleet.n_streams, [clouds[k]] * fleet.n_streams)
    return traj


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--streams", type=int, nargs="+", default=[1, 2, 4, 8, 16, 32])
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_odometry_fleet.py measures on a GPU: none is usable here")
    from delta_graph_slam_amd import _lib as L
    from delta_graph_slam_amd import synth
    from delta_graph_slam_amd.odometry import ScanMatchingOdometry, ScanMatchingOdometryFleet

    host, _ = synth.vlp16_stream(n_frames=args.frames)
    clouds = [torch.from_numpy(c).cuda() for c in host]
    torch.cuda.synchronize()
    timed = range(args.frames)
    rows = []
    for B in args.streams:
        solo_fps, fleet_fps = [], []
        end_diff = 0.0
        for _ in range(args.repeats):
            # fresh objects per repeat: both paths start from their first frame
            regs = [make_registration() for _ in range(B)]
            odos = [ScanMatchingOdometry(r, dict(KEYFRAMES, **DOWN)) for r in regs]
            run_solo(odos, clouds, range(args.warmup))
            for o in odos:
                o.keyframe = None
            t0 = time.perf_counter()
            a = run_solo(odos, clouds, timed)
            for r in regs:
                r.synchronize()
            solo_fps.append(B * args.frames / (time.perf_counter() - t0))
            for r in regs:
                r.close()

            reg = make_registration()
            fleet = ScanMatchingOdometryFleet(reg, B, dict(KEYFRAMES, **DOWN))
            run_fleet(fleet, clouds, range(args.warmup))
            fleet = ScanMatchingOdometryFleet(reg, B, dict(KEYFRAMES, **DOWN))
            t0 = time.perf_counter()
            b = run_fleet(fleet, clouds, timed)
            reg.synchronize()
            fleet_fps.append(B * args.frames / (time.perf_counter() - t0))
            end_diff = max(end_diff, max(float(np.abs(b[j] - a[j]).max()) for j in range(B)))
            if _ == args.repeats - 1:   # counts of one steady step, profiler on: not part of any timing
                reg.profile_enable(True)
                reg.profile_reset()
                fleet.step([0.1 * args.frames] * B, [clouds[args.frames // 2]] * B)
                assign, fb, cb = reg.cloud_assign_counts(), reg.fitness_batch_counts(), reg.covariance_batch_counts()
                slots = {name: reg.profile_get(k)[1] for name, k in (("correspondence", L.K_NN_SEARCH), ("linearize", L.K_GICP_LINEARIZE), ("covariance", L.K_GICP_COVARIANCE))}
                counts = {"downsample_launches": assign["launches"], "downsample_host_waits": assign["host_waits"], "index_build_launches": fb["launches"],
                          "index_build_host_waits": fb["host_waits"], "round_launch_slots": slots,
                          # beside the "covariance" slot count (passes, one per cloud): what the batched pass launched for them
                          "covariance_launches": cb["launches"], "covariance_chunks": cb["chunks"], "covariance_clouds": cb["covered"],
                          "covariance_host_waits": cb["host_waits"], "covariance_fallback": cb["fallback"]}
                reg.profile_enable(False)
            reg.close()
        row = {"streams": B, "frames": args.frames, "solo_fps": [round(v, 1) for v in solo_fps], "fleet_fps": [round(v, 1) for v in fleet_fps],
               "fleet_over_solo_median": round(float(np.median(fleet_fps) / np.median(solo_fps)), 3), "end_pose_max_abs_diff": end_diff, "fleet_step_counts": counts}
        print(json.dumps(row), flush=True)
        rows.append(row)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            for row in rows:
                f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
