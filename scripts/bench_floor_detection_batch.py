"""Floor detection over many scans in one device call (FloorDetector.detect_batch) against B x detect, on one GPU; prints one JSON line
per (scan, normal filter, B) and run.

  B in {1, 2, 4, 8, 16, 32} copies of the VLP-16 (16 x 1875 rays) and the HDL-64 (64 x 1024 rays) synth.street_scan after the prefilter
  (Prefilter.cloud_callback's 3-D output), device-resident, as bench_floor_detection.py takes them; sensor_height 1.73, the normal
  filter on and off.  "seq" is B x detect, "batch" one detect_batch.  Before anything is timed the two legs are compared for equality,
  scan by scan (status, coefficient bits, filtered cloud bits).  Per leg: --warmup calls, then --steps timed calls, the legs alternating
  call by call; ms between two HIP events around a call that ends behind its last host wait (the host clock beside it); the median of
  the timed calls.  --runs such runs in one process.  Launches, host waits and rounds are batch_counts() of the batched call; the
  library does not count the single call's (three host waits per scan with the normal filter, two without).

  --single-only: B x detect alone, for comparing two builds of the library (DGS_REG_LIB) in fresh processes, alternated by the caller.

usage: python scripts/bench_floor_detection_batch.py [--warmup 5] [--steps 21] [--runs 3] [--sizes 1,2,4,8,16,32] [--scans vlp16,hdl64]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from delta_graph_slam_amd import synth  # noqa: E402
from delta_graph_slam_amd.floor_detection import FloorDetector  # noqa: E402
from delta_graph_slam_amd.prefilter import Prefilter  # noqa: E402

SCANS = {"vlp16": ((-30.0, 1.0, 0.1), 16, (15.0, -15.0), 1875, 21), "hdl64": ((0.0, 0.0, 0.0), 64, (2.0, -24.8), 1024, 3)}
SENSOR_Z = 1.73


def filtered_points(kind):
    pose, beams, fov, azimuths, seed = SCANS[kind]
    raw = torch.from_numpy(synth._xyz1(synth.street_scan(pose, beams, fov, azimuths, seed)[0])).cuda()
    return Prefilter().cloud_callback(raw)[0]


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=21)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--sizes", default="1,2,4,8,16,32")
    ap.add_argument("--scans", default="vlp16,hdl64")
    ap.add_argument("--single-only", action="store_true")
    a = ap.parse_args()
    sizes = [int(v) for v in a.sizes.split(",")]
    for kind in a.scans.split(","):
        f3 = filtered_points(kind)
        copies = [f3.clone() for _ in range(max(sizes))]
        for normal in (1, 0):
            det = FloorDetector(dict(sensor_height=SENSOR_Z, use_normal_filtering=normal))
            for n in sizes:
                clouds = copies[:n]

                def seq():
                    return [det.detect(c) for c in clouds]

                def batch():
                    return det.detect_batch(clouds)

                if a.single_only:
                    for run in range(a.runs):
                        for _ in range(a.warmup):
                            seq()
                        ts = [timed(seq) for _ in range(a.steps)]
                        print(json.dumps({"scan": kind, "normal": normal, "n": n, "run": run, "points": int(f3.shape[0]),
                                          "seq_ms": round(float(np.median([t[0] for t in ts])), 4), "seq_wall_ms": round(float(np.median([t[1] for t in ts])), 4),
                                          "lib": os.environ.get("DGS_REG_LIB", "")}), flush=True)
                    continue
                # equal results before anything is timed
                cos = batch()
                for i, c in enumerate(clouds):
                    co = det.detect(c)
                    assert det.status == det.statuses[i] and (co is None) == (cos[i] is None)
                    assert co is None or np.array_equal(co.view(np.uint32), cos[i].view(np.uint32))
                    assert torch.equal(det.filtered(c).view(torch.int32), det.batch_filtered(i, c).view(torch.int32))
                batch()
                counts = det.batch_counts()
                for run in range(a.runs):
                    for _ in range(a.warmup):
                        seq()
                        batch()
                    torch.cuda.synchronize()
                    ts, tb = [], []
                    for _ in range(a.steps):
                        ts.append(timed(seq))
                        tb.append(timed(batch))
                    s_ms, b_ms = float(np.median([t[0] for t in ts])), float(np.median([t[0] for t in tb]))
                    print(json.dumps({
                        "scan": kind, "normal": normal, "n": n, "run": run, "points": int(f3.shape[0]), "status": det.statuses[0],
                        "seq_ms": round(s_ms, 4), "batch_ms": round(b_ms, 4), "ratio": round(s_ms / b_ms, 3),
                        "seq_wall_ms": round(float(np.median([t[1] for t in ts])), 4), "batch_wall_ms": round(float(np.median([t[1] for t in tb])), 4),
                        "batch_launches": int(counts[0]), "batch_host_waits": int(counts[1]), "batch_rounds": int(counts[7]), "fallbacks": int(counts[4]),
                    }), flush=True)


if __name__ == "__main__":
    main()
