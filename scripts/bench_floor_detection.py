#!/usr/bin/env python
"""ms per floor detection (FloorDetector.detect) on the prefilter's 3-D output (/filtered_points) of the synthetic HDL-64 and VLP-16
street scans, device-resident, with and without the normal filter.  Device time from HIP events around the call (it includes the
host's waits: the two counts of the filter stage and one per chunk of hypotheses; that is what a frame pays), median of --repeats runs
after one warm-up; the hypotheses actually scored, the walk's iterations and the chunks launched; the numpy restatement's wall time for
scale.  One JSON line per case.  Recorded in DESIGN.md 6j, not gated.
Under `rocprofv3 --kernel-trace --stats -- python scripts/bench_floor_detection.py` the kernel table gives the split by kernel."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from delta_graph_slam_amd import synth                      # noqa: E402
from delta_graph_slam_amd.floor_detection import FloorDetector   # noqa: E402
from delta_graph_slam_amd.prefilter import Prefilter       # noqa: E402
from delta_graph_slam_amd.registration import Registration  # noqa: E402

SENSOR_Z = 1.73   # synth.street_scan's sensor height over the street
SCANS = {"hdl64": dict(beams=64, elev_deg=(2.0, -24.8), azimuths=2048, seed=31), "vlp16": dict(beams=16, elev_deg=(15.0, -15.0), azimuths=1875, seed=21)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=21)
    ap.add_argument("--no-reference", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_floor_detection.py needs a GPU: a CPU run gives no time")
    reg = Registration("NDT_OMP", device=0)
    for scan_name, sc in SCANS.items():
        xyz, _ = synth.street_scan((-30.0, 1.0, 0.1), sc["beams"], sc["elev_deg"], sc["azimuths"], sc["seed"])
        scan = np.concatenate([xyz, np.ones((xyz.shape[0], 1))], 1).astype(np.float32)
        f3, _, _ = Prefilter(registration=reg).filter_scan(torch.from_numpy(scan).cuda())
        for normal in (1, 0):
            prm = dict(sensor_height=SENSOR_Z, use_normal_filtering=normal)
            det = FloorDetector(prm, registration=reg)
            det.detect(f3)
            ms = []
            for _ in range(args.repeats):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                coeffs = det.detect(f3)
                b.record()
                b.synchronize()
                ms.append(a.elapsed_time(b))
            t = det.trace()
            out = dict(scan=scan_name, normal_filter=normal, points=int(f3.shape[0]), clipped=t["n_clipped"], filtered=t["n_filtered"], status=det.status,
                       coeffs=None if coeffs is None else [float(v) for v in coeffs], ms_median=float(np.median(ms)), ms_min=float(min(ms)),
                       ms_max=float(max(ms)), hypotheses_scored=t["hypotheses_scored"], iterations=t["iterations"], draws=t["draws"],
                       chunks_launched=t["chunks_launched"], inliers=t["count"])
            if not args.no_reference:
                import floor_detection_reference as R
                t0 = time.perf_counter()
                r = R.detect(f3.cpu().numpy(), prm)
                out.update(restatement_s=time.perf_counter() - t0, restatement_status=r["status"], restatement_iterations=r["trace"]["iterations"])
            print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
