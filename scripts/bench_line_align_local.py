"""align_local for one keyframe against its near buildings: one batched device call against the same items as single calls and against the
shared header compiled for the host (tests/cpp/line_align_local_driver.cpp, mode `host`).  Not bench.py: recorded in DESIGN.md 6g, not gated.

The keyframe sees about 20 wall pieces around a street crossing; every building is a rectangle of four lines (the source of its item, as
in apps/delta_graph_slam_nodelet.cpp:687) and the keyframe's lines are the target.  Prints one JSON line per batch size B.

    python scripts/bench_line_align_local.py [--sizes 8 32 64] [--repeats 30] [--warmup 5]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def keyframe_and_buildings(n_buildings, seed=0):
    import line_align_reference as R
    rng = np.random.default_rng(seed)
    blocks = [R.rectangle(sx * 14.0, sy * 12.0, 16.0, 12.0) for sx in (-1, 1) for sy in (-1, 1)]       # four blocks around the crossing
    seen = np.concatenate([R.trim(b, 0.6) for b in blocks] + [R.trim(R.rectangle(0.0, 40.0, 10.0, 6.0), 0.6)])   # 20 wall pieces
    lidar = R.move(seen, 0.35, -0.2, np.deg2rad(2.5))                                                   # the odometry's error
    buildings = []
    for k in range(n_buildings):
        if k < 4:
            buildings.append(blocks[k])
        else:                                                                                           # further buildings of the tile
            a = 2 * np.pi * k / n_buildings
            buildings.append(R.rectangle(45.0 * np.cos(a), 45.0 * np.sin(a), rng.uniform(8, 16), rng.uniform(6, 12), rng.uniform(0, np.pi / 2)))
    return lidar, buildings


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[8, 32, 64])
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    from delta_graph_slam_amd.line_align import LineScanMatcher
    from delta_graph_slam_amd.registration import Registration
    import line_align_local_reference as LR     # the scene helpers and the driver's file format; no test module is imported
    _lines, write_items = LR.feature_lines, LR.write_items
    reg = Registration("NDT_OMP", device=0)
    m = LineScanMatcher(registration=reg)
    tmp = tempfile.mkdtemp()
    exe = os.path.join(tmp, "line_align_local_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "line_align_local_driver.cpp"), "-o", exe,
                           os.path.join(ROOT, "delta_graph_slam_amd", "libdgs_reg.so"), "-Wl,-rpath," + os.path.join(ROOT, "delta_graph_slam_amd"),
                           "-Wl,-rpath,/opt/rocm/lib"])
    for B in args.sizes:
        lidar, buildings = keyframe_and_buildings(B)
        items = [(_lines(b), _lines(lidar)) for b in buildings]

        def timed(fn):
            for _ in range(args.warmup):
                fn()
            t = []
            for _ in range(args.repeats):
                t0 = time.perf_counter()
                fn()
                t.append((time.perf_counter() - t0) * 1e3)
            return statistics.median(t)

        batch_ms = timed(lambda: m.align_local_batch(items, 0.5))
        cb = m.local_counts()
        single_ms = timed(lambda: [m.align_local(s, t, 0.5) for s, t in items])
        cs = m.local_counts()
        ip, op = os.path.join(tmp, "items.bin"), os.path.join(tmp, "out.bin")
        write_items(ip, [(b, lidar) for b in buildings])
        host = json.loads(subprocess.check_output([exe, "host", ip, op, "0.5", f"repeat={args.repeats}"]).decode().splitlines()[-1])
        cpp = json.loads(subprocess.check_output([exe, "run", ip, op, "0.5", f"repeat={args.repeats}"]).decode().splitlines()[-1])
        cpp1 = json.loads(subprocess.check_output([exe, "run", ip, op, "0.5", f"repeat={args.repeats}", "single=1"]).decode().splitlines()[-1])
        res = m.align_local_batch(items, 0.5)
        print(json.dumps(dict(
            buildings=B, lidar_lines=int(lidar.shape[0]), batch_ms=round(batch_ms, 4), single_calls_ms=round(single_ms, 4),
            batch_ms_cpp_wrapper=round(cpp["ms_per_call"], 4), single_calls_ms_cpp_wrapper=round(cpp1["ms_per_call"], 4), host_header_ms=round(host["ms_per_call"], 4),
            launches_batch=cb["launches"], host_waits_batch=cb["host_waits"], launches_single_calls=cs["launches"] * B,
            host_waits_single_calls=cs["host_waits"] * B, hypotheses_edge=cb["hypotheses_edge"], hypotheses_line=cb["hypotheses_line"],
            survivors_edge=cb["survivors_edge"], survivors_line=cb["survivors_line"], workgroups=cb["workgroups"],
            aligned=sum(r.status in ("ALIGNED", "LINE_ALIGNED") for r in res), repeats=args.repeats, warmup=args.warmup)), flush=True)


if __name__ == "__main__":
    main()
