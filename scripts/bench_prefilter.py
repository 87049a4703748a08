"""Prefilter chain (PrefilteringNodelet::cloud_callback, distance filter to flatten) on one GPU; prints one JSON line.

  ms per frame from device events around dgs_prefilter (device tensor in, device tensors out) on raw synth.street_scan frames:
  HDL-64 (64 x 4096 rays) and VLP-16 (16 x 1875 rays), with the launch file's parameters (RADIUS 0.5 / 2) and the code defaults
  (STATISTICAL 20 / 1.0), both with VOXELGRID 0.1; and a per-stage split from the single-stage entry points on the chain's
  intermediate clouds.  Kernel times: run `--chain-only` under `rocprofv3 --kernel-trace --stats`.
  Raw-scan row (`*_scan_ms`): filter_scan (dgs_prefilter_scan) on the same frame with an angular velocity and a base_link transform
  given; `*_scan_chain_ms` is dgs_prefilter alone on that frame deskewed and transformed beforehand (the same work behind the head),
  and `*_head_ms` the difference: what deskewing and the transform cost per frame.  `*_ms` stays dgs_prefilter on the raw frame.

usage: python scripts/bench_prefilter.py [--warmup W] [--steps K] [--chain-only]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from delta_graph_slam_amd import synth  # noqa: E402
from delta_graph_slam_amd.prefilter import Prefilter  # noqa: E402

DEFAULTS = {}
LAUNCH = dict(distance_near_thresh=0.1, outlier_removal_method="RADIUS", radius_radius=0.5, radius_min_neighbors=2, statistical_mean_k=30,
              statistical_stddev=1.2)
IMU = (0.3, -0.8, 1.1)                      # rad/s
BASE_LINK = np.array([[0.954, -0.2955, -0.0478, 0.4], [0.2951, 0.9553, -0.0148, -0.2], [0.05, 0.0, 0.9988, 1.7], [0.0, 0.0, 0.0, 1.0]])


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
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--chain-only", action="store_true")
    a = ap.parse_args()
    scans = {"hdl64": synth.street_scan((0.0, 0.0, 0.0), 64, (2.0, -24.8), 4096, 3)[0],
             "vlp16": synth.street_scan((-30.0, 1.0, 0.1), 16, (15.0, -15.0), 1875, 21)[0]}
    out = {}
    for sname, xyz in scans.items():
        c = torch.from_numpy(synth._xyz1(xyz)).cuda()
        out[f"{sname}_points"] = int(c.shape[0])
        for pname, params in (("launch", LAUNCH), ("defaults", DEFAULTS)):
            pf = Prefilter(params)
            key = f"{sname}_{pname}"
            f3, f2 = pf.cloud_callback(c)
            out[f"{key}_n3d"], out[f"{key}_n2d"] = int(f3.shape[0]), int(f2.shape[0])
            out[f"{key}_ms"] = round(ev_ms(lambda: pf.cloud_callback(c), a.warmup, a.steps), 4)
            if hasattr(pf, "filter_scan"):   # absent from a build of an earlier commit run for comparison
                s3, s2, lidar = pf.filter_scan(c, IMU, BASE_LINK)
                out[f"{key}_scan_n3d"], out[f"{key}_scan_n2d"] = int(s3.shape[0]), int(s2.shape[0])
                out[f"{key}_scan_ms"] = round(ev_ms(lambda: pf.filter_scan(c, IMU, BASE_LINK), a.warmup, a.steps), 4)
                mid = pf.deskew(c, IMU, BASE_LINK)       # the same work behind the head: the chain alone on the deskewed, transformed frame
                out[f"{key}_scan_chain_ms"] = round(ev_ms(lambda: pf.cloud_callback(mid, lidar), a.warmup, a.steps), 4)
                out[f"{key}_head_ms"] = round(out[f"{key}_scan_ms"] - out[f"{key}_scan_chain_ms"], 4)
            if a.chain_only:
                continue
            d = pf.distance_filter(c)
            ds = pf.downsample(d)
            o = pf.outlier_removal(ds)
            h = pf.height_filtering(o)
            out[f"{key}_split_ms"] = {
                "distance": round(ev_ms(lambda: pf.distance_filter(c), a.warmup, a.steps), 4),
                "voxelgrid": round(ev_ms(lambda: pf.downsample(d), a.warmup, a.steps), 4),
                "outlier": round(ev_ms(lambda: pf.outlier_removal(ds), a.warmup, a.steps), 4),
                "normal": round(ev_ms(lambda: pf.normal_filtering(h), a.warmup, a.steps), 4),
            }
    print(json.dumps(out))


if __name__ == "__main__":
    main()
