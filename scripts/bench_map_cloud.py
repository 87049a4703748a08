"""Map cloud (MapCloudGenerator::generate) on one GPU over resident keyframe clouds; prints one JSON line.

  Keyframes: VLP-16-shaped synth.street_scan frames every 0.5 m along a trajectory that runs up and down the synthetic street (so
  the map is revisited, as a SLAM graph is), through the prefilter chain with the launch file's parameters.  `flat`: the
  /flat_filtered_points clouds with the 2-D snapshot poses KeyFrameSnapshot makes; `3d`: the /filtered_points clouds with the full
  sensor poses.  Every keyframe cloud is made resident once (dgs_cloud); per map only the poses travel.
  ms per map: median over K calls of dgs_map_cloud_generate_clouds after warm-up, for the key table (dedup HASH) and for the sort of
  all keys (dedup SORT).  The call blocks the host until the map is done (the growth replay and the counts are read back on the
  way), and the library works on the handle's own stream: the two events around it sit on torch's current stream and measure the
  host's wall time for the call, every wait included -- which is what a caller pays.  Kernel times: run one size (--keyframes N
  --kinds K --resolutions R) under `rocprofv3 --kernel-trace --stats`.

usage: python scripts/bench_map_cloud.py [--keyframes 256,2048] [--resolutions 0.05,0.01] [--kinds flat,3d] [--dedup HASH,SORT]
                                         [--warmup W] [--steps K]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from delta_graph_slam_amd import synth  # noqa: E402
from delta_graph_slam_amd.map_cloud import MapCloudGenerator, snapshot_pose  # noqa: E402
from delta_graph_slam_amd.prefilter import Prefilter  # noqa: E402
from delta_graph_slam_amd.registration import Registration  # noqa: E402

LAUNCH = dict(distance_near_thresh=0.1, outlier_removal_method="RADIUS", radius_radius=0.5, radius_min_neighbors=2)
STEP_M = 0.5      # keyframe_delta_trans of the launch files
HALF_M = 55.0     # the street is ~130 m long


def trajectory(n):
    """(x, y, yaw) every STEP_M: up the street, back on the other lane, and again with the lanes a little further out"""
    out = []
    x, direction, lane = -HALF_M, 1.0, 0
    for _ in range(n):
        y = (1.5 + 0.4 * (lane // 2)) * (1.0 if direction > 0 else -1.0)
        out.append((x, y + 0.3 * np.sin(0.2 * x), 0.0 if direction > 0 else np.pi))
        x += direction * STEP_M
        if abs(x) > HALF_M:
            direction, lane = -direction, lane + 1
            x += direction * STEP_M
    return out


def ev_ms(fn, warmup, steps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts)), float(np.min(ts)), float(np.max(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keyframes", default="256,2048")
    ap.add_argument("--resolutions", default="0.05,0.01")
    ap.add_argument("--kinds", default="flat,3d")
    ap.add_argument("--dedup", default="HASH,SORT")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps", type=int, default=10)
    a = ap.parse_args()
    sizes = [int(v) for v in a.keyframes.split(",")]
    reg = Registration("NDT_OMP")    # one handle: the resident clouds belong to its device
    gens = {d: MapCloudGenerator(registration=reg, params={"dedup_method": d}) for d in a.dedup.split(",")}
    pf = Prefilter(LAUNCH, registration=reg)
    clouds = {"flat": [], "3d": []}
    poses = {"flat": [], "3d": []}
    for k, (x, y, yaw) in enumerate(trajectory(max(sizes))):
        xyz, T = synth.street_scan((x, y, yaw), 16, (15.0, -15.0), 1875, 100 + k)
        f3, f2 = pf.cloud_callback(torch.from_numpy(synth._xyz1(xyz)).cuda())
        est = np.array([[np.cos(yaw), -np.sin(yaw), x], [np.sin(yaw), np.cos(yaw), y], [0, 0, 1]], np.float64)
        clouds["flat"].append(reg.make_cloud(f2))
        poses["flat"].append(snapshot_pose(est))
        clouds["3d"].append(reg.make_cloud(f3))
        poses["3d"].append(T)
    out = {"device": torch.cuda.get_device_name(0), "warmup": a.warmup, "steps": a.steps, "rows": []}
    lib = reg._lib
    for kind in a.kinds.split(","):
        for n in sizes:
            arr = (C.c_void_p * n)(*[c._c.value for c in clouds[kind][:n]])
            p16 = np.ascontiguousarray(np.array([p.T.reshape(16) for p in poses[kind][:n]], np.float64))
            points = int(sum(len(c) for c in clouds[kind][:n]))
            for res in [float(v) for v in a.resolutions.split(",")]:
                row = {"kind": kind, "keyframes": n, "points": points, "resolution": res}
                for d, g in gens.items():
                    m = C.c_int64(0)

                    def call():
                        reg._check(lib.dgs_map_cloud_generate_clouds(reg._h, C.byref(g.params), n, arr, p16.ctypes.data_as(C.c_void_p), res, C.byref(m)))

                    med, lo, hi = ev_ms(call, a.warmup, a.steps)
                    grid = g.grid()
                    row.update({f"{d.lower()}_ms": round(med, 3), f"{d.lower()}_min_ms": round(lo, 3), f"{d.lower()}_max_ms": round(hi, 3),
                                "voxels": int(m.value), "depth": grid["depth"], "growths": grid["growths"]})
                out["rows"].append(row)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
