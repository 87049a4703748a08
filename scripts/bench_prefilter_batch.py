"""The prefilter over many scans in one device call (Prefilter.filter_scan_batch) against N x filter_scan, on one GPU; prints one JSON
line per run.

  N in {1, 2, 4, 8, 16} raw synth.street_scan frames (different seeds), VLP-16 (16 x 1875 rays) and HDL-64 (64 x 4096 rays) as in
  bench_prefilter.py, with the launch file's parameters (RADIUS 0.5 / 2) and the code defaults (STATISTICAL 20 / 1.0), both with
  VOXELGRID 0.1; device tensors in, device tensors out, an angular velocity and a base_link transform given.
  "seq" is N x filter_scan, "batch" one filter_scan_batch.  Before anything is timed the outputs of the two legs are compared for
  equality, scan by scan.  Per leg: 5 warm-up calls, then 50 timed calls, the legs alternating call by call; ms from a host clock around
  calls that end in a device synchronise; the median of the 50.  Three such runs (--runs), the median of the three medians reported
  beside the three.  Launches and host waits: the batch leg's are batch_counts() of the call.  The library does not count the single
  call's, so the seq leg reports N x batch_counts() of a batch of one frame: the same stages and the same host waits; the single call's
  own index and voxel-grid builds take more launches than the batched ones, so this is a lower bound for it.

usage: python scripts/bench_prefilter_batch.py [--warmup 5] [--steps 50] [--runs 3] [--sizes 1,2,4,8,16] [--shapes vlp16,hdl64]
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
from delta_graph_slam_amd.prefilter import Prefilter  # noqa: E402

DEFAULTS = {}
LAUNCH = dict(distance_near_thresh=0.1, outlier_removal_method="RADIUS", radius_radius=0.5, radius_min_neighbors=2, statistical_mean_k=30,
              statistical_stddev=1.2)
IMU = (0.3, -0.8, 1.1)                      # rad/s
BASE_LINK = np.array([[0.954, -0.2955, -0.0478, 0.4], [0.2951, 0.9553, -0.0148, -0.2], [0.05, 0.0, 0.9988, 1.7], [0.0, 0.0, 0.0, 1.0]])
SHAPES = {"vlp16": ((-30.0, 1.0, 0.1), 16, (15.0, -15.0), 1875, 21), "hdl64": ((0.0, 0.0, 0.0), 64, (2.0, -24.8), 4096, 3)}


def frames(shape, n):
    pose, beams, fov, azimuths, seed = SHAPES[shape]
    return [torch.from_numpy(synth._xyz1(synth.street_scan(pose, beams, fov, azimuths, seed + k)[0])).cuda() for k in range(n)]


def timed(fn):
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--sizes", default="1,2,4,8,16")
    ap.add_argument("--shapes", default="vlp16,hdl64")
    a = ap.parse_args()
    sizes = [int(v) for v in a.sizes.split(",")]
    for shape in a.shapes.split(","):
        all_frames = frames(shape, max(sizes))
        for pname, params in (("launch", LAUNCH), ("defaults", DEFAULTS)):
            pf = Prefilter(params)
            pf.filter_scan_batch(all_frames[:1], [IMU], [BASE_LINK])
            base = pf.batch_counts()                    # one frame alone
            for n in sizes:
                fr = all_frames[:n]
                avs, tfs = [IMU] * n, [BASE_LINK] * n

                def seq():
                    return [pf.filter_scan(c, IMU, BASE_LINK) for c in fr]

                def batch():
                    return pf.filter_scan_batch(fr, avs, tfs)

                # equal outputs before anything is timed
                s, (b, st) = seq(), batch()
                assert not st.any()
                for x, y in zip(s, b):
                    assert torch.equal(x[0].view(torch.int32), y[0].view(torch.int32)) and torch.equal(x[1].view(torch.int32), y[1].view(torch.int32))
                    assert np.array_equal(x[2], y[2])
                counts = pf.batch_counts()
                runs = []
                for _ in range(a.runs):
                    for _ in range(a.warmup):
                        seq()
                        batch()
                    torch.cuda.synchronize()
                    ts, tb = [], []
                    for _ in range(a.steps):
                        ts.append(timed(seq))
                        tb.append(timed(batch))
                    runs.append((float(np.median(ts)), float(np.median(tb))))
                seq_ms, batch_ms = [r[0] for r in runs], [r[1] for r in runs]
                print(json.dumps({
                    "shape": shape, "params": pname, "n": n, "points": [int(c.shape[0]) for c in fr][:2], "n3d": int(b[0][0].shape[0]), "n2d": int(b[0][1].shape[0]),
                    "seq_ms": round(float(np.median(seq_ms)), 4), "batch_ms": round(float(np.median(batch_ms)), 4),
                    "ratio": round(float(np.median(seq_ms)) / float(np.median(batch_ms)), 3),
                    "seq_runs_ms": [round(v, 4) for v in seq_ms], "batch_runs_ms": [round(v, 4) for v in batch_ms],
                    "batch_faster_in_all_runs": bool(max(batch_ms) < min(seq_ms)),
                    "batch_launches": int(counts[0]), "batch_host_waits": int(counts[1]), "seq_launches": int(base[0]) * n, "seq_host_waits": int(base[1]) * n,
                }), flush=True)


if __name__ == "__main__":
    main()
