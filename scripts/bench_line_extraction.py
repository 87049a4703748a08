#!/usr/bin/env python
"""ms per line extraction (LineExtractor.extract) on the flat cloud of the synthetic HDL-64 and VLP-16 street scans after the prefilter
chain, with the launch file's values (launch/delta_graph_slam.launch:149-156) and with the constructor's defaults.  Device time from
HIP events around the call (it includes the host's waits between rounds: that is what a frame pays), median of --repeats runs after
one warm-up; rounds, kernel launches and host waits per round; the numpy restatement's wall time for scale.  One JSON line per case.
Under `rocprofv3 --kernel-trace --stats -- python scripts/bench_line_extraction.py` the kernel table gives the split by kernel."""
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
from delta_graph_slam_amd.line_extraction import LineExtractor   # noqa: E402
from delta_graph_slam_amd.prefilter import Prefilter       # noqa: E402
from delta_graph_slam_amd.registration import Registration  # noqa: E402

PF_LAUNCH = dict(distance_near_thresh=0.1, outlier_removal_method="RADIUS", radius_radius=0.5, radius_min_neighbors=2)
LE_LAUNCH = dict(min_cluster_size=40, max_cluster_size=25000, cluster_tolerance=1.5, sac_distance_threshold=0.1, max_iterations=100,
                 merror_threshold=0.1, line_length_threshold=1.5)
SCANS = {"hdl64": dict(beams=64, elev_deg=(2.0, -24.8), azimuths=2048, seed=31), "vlp16": dict(beams=16, elev_deg=(15.0, -15.0), azimuths=1875, seed=21)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--no-reference", action="store_true")
    args = ap.parse_args()
    reg = Registration("NDT_OMP", device=0)
    for scan_name, sc in SCANS.items():
        xyz, _ = synth.street_scan((-30.0, 1.0, 0.1), sc["beams"], sc["elev_deg"], sc["azimuths"], sc["seed"])
        scan = np.concatenate([xyz, np.ones((xyz.shape[0], 1))], 1).astype(np.float32)
        _, flat, _ = Prefilter(PF_LAUNCH, registration=reg).filter_scan(torch.from_numpy(scan).cuda())
        for pname, prm in (("launch", LE_LAUNCH), ("defaults", {})):
            ex = LineExtractor(prm, registration=reg)
            ex.extract(flat)
            ms = []
            for _ in range(args.repeats):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                lines = ex.extract(flat)
                b.record()
                b.synchronize()
                ms.append(a.elapsed_time(b))
            rounds, c = ex.rounds(), ex.counts()
            out = dict(scan=scan_name, params=pname, flat_points=int(flat.shape[0]), lines=len(lines), status=ex.status, rounds=len(rounds),
                       ms_median=float(np.median(ms)), ms_min=float(min(ms)), ms_max=float(max(ms)),
                       launches_per_round=c["launches"] / max(c["rounds_launched"], 1), sort_calls_per_round=c["sort_calls"] / max(c["rounds_launched"], 1),
                       host_waits_per_round=c["host_waits"] / max(c["rounds_launched"], 1))
            if not args.no_reference:
                import line_extraction_reference as R
                t = time.perf_counter()
                rl, rr, rs = R.line_extraction(flat.cpu().numpy(), prm)
                out.update(restatement_s=time.perf_counter() - t, restatement_lines=len(rl), restatement_rounds=len(rr))
            print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
