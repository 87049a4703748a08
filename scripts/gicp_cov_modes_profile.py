"""The covariance pass of FAST_GICP in dgs_params.gicp_cov_jacobi_svd = 0 (tree sums, the default) and 2 (upstream order), in one run.

  python scripts/gicp_cov_modes_profile.py                 workload: covariances of 65,536-point HDL-64E-shaped clouds and ~26 k-point VLP-16 frames in
                                                           both modes (run it under `rocprofv3 --kernel-trace --output-format csv -d DIR --`), then the first
                                                           FAST_GICP align of a cfg2 pair (wall clock, covariances of both clouds included) in both modes
  python scripts/gicp_cov_modes_profile.py summary DIR     per-kernel medians of the trace, grouped by kernel and grid size (= cloud size), as JSON lines
"""
import collections
import csv
import glob
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def summary(d):
    rows = []
    for f in glob.glob(d + "/**/*kernel_trace.csv", recursive=True):
        rows += list(csv.DictReader(open(f)))
    acc = collections.OrderedDict()
    for r in sorted(rows, key=lambda r: int(r["Start_Timestamp"])):
        name = r["Kernel_Name"].split("(")[0].replace("void ", "").replace("dgs::", "")
        if "gicp_cov" not in name and "gicp_knn" not in name:
            continue
        grid = r.get("Grid_Size") or r.get("Grid_Size_X")
        wg = r.get("Workgroup_Size") or r.get("Workgroup_Size_X")
        acc.setdefault((name, int(grid), int(wg)), []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    for (name, grid, wg), us in acc.items():
        s = sorted(us)
        print(json.dumps({"kernel": name, "grid_threads": grid, "workgroup": wg, "calls": len(us), "median_us": round(s[len(s) // 2], 2), "min_us": round(s[0], 2),
                          "max_us": round(s[-1], 2)}))


def workload():
    import numpy as np
    import torch
    from delta_graph_slam_amd import synth
    from delta_graph_slam_amd.registration import Registration
    tgt, sources, _, _ = synth.loop_batch(n_candidates=3, n_points=65536, seed=40, distinct_scans=3)
    frames = synth.vlp16_stream(n_frames=3)[0]
    reps = int(os.environ.get("COV_REPS", "6"))
    for mode in (0, 2):
        reg = Registration("FAST_GICP", gicp_max_correspondence_distance=2.0, gicp_cov_jacobi_svd=mode)
        for name, clouds in (("hdl64", [tgt] + list(sources)), ("vlp16", frames)):
            dev = [torch.from_numpy(np.ascontiguousarray(c, dtype=np.float32)).cuda() for c in clouds]
            for _ in range(reps):
                for c in dev:
                    reg.setInputTarget(c)
                    reg.gicp_covariances("target")
            print(json.dumps({"mode": mode, "clouds": name, "points": [int(c.shape[0]) for c in clouds], "passes": reps * len(dev)}), flush=True)
        reg.close()
    # first align of a cfg2 pair: index builds, k-NN, covariances of both clouds and the LM iterations
    tgt, src, Tgt = synth.kitti_pair(n_points=65536)
    guess = Tgt.copy().astype(np.float32)
    guess[0, 3] -= 0.2
    for mode in (0, 2):
        reg = Registration("FAST_GICP", gicp_cov_jacobi_svd=mode)
        ms = []
        for _ in range(7):
            reg.setInputTarget(tgt)
            reg.setInputSource(src)
            reg.synchronize()
            t0 = time.perf_counter()
            reg.align(guess)
            ms.append((time.perf_counter() - t0) * 1e3)
        s = sorted(ms[1:])   # the first one loads the code objects
        print(json.dumps({"mode": mode, "first_align_cfg2_ms_median": round(s[len(s) // 2], 3), "min": round(s[0], 3), "max": round(s[-1], 3),
                          "iterations": int(reg.last_result.iterations), "converged": bool(reg.hasConverged())}), flush=True)
        reg.close()


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "summary":
        summary(sys.argv[2])
    else:
        workload()
