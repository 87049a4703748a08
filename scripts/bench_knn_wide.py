"""Time of the k-NN + covariance pass (DGS_K_GICP_COVARIANCE through dgs_profile_get) by k, covariance mode and wide k-NN search.

Clouds: the 65,536-point cfg2 target (synth.kitti_pair) and one ~26.7 k-point cfg3 frame (synth.vlp16_stream).  For k in 20, 32, 33, 40, 64,
in default and upstream-order covariance mode; for k > 32 under both wide searches (the wave-per-leaf search, and DGS_KNN_LEAF_WIDE=0:
the per-query walk).  Every figure is the median of `--runs` runs of `--passes` passes each (a pass = setInputSource on a fresh cloud +
the covariance pass of one align's start).  Prints one JSON line per figure.

    python scripts/bench_knn_wide.py [--runs 3] [--passes 20] [--lib PATH]     # --lib: another build of libdgs_reg.so, for A/B against a parent
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from delta_graph_slam_amd import _lib as L  # noqa: E402
from delta_graph_slam_amd import synth  # noqa: E402
from delta_graph_slam_amd.registration import Registration  # noqa: E402


def _time(cloud, k, mode, leaf_wide, passes, lib_path):
    os.environ["DGS_KNN_LEAF_WIDE"] = "1" if leaf_wide else "0"
    r = Registration("FAST_GICP", lib_path=lib_path, gicp_correspondence_randomness=k, gicp_cov_jacobi_svd=mode)
    r.profile_enable(True)
    r.setInputTarget(cloud)
    r.gicp_covariances("target", cloud.shape[0])          # warm-up: index build, first launch
    r.profile_reset()
    for _ in range(passes):
        r.setInputTarget(cloud)                            # a new cloud state: the covariances are made again
        r.gicp_covariances("target", cloud.shape[0])
    ms, n = r.profile_get(L.K_GICP_COVARIANCE)
    r.close()
    return ms / max(n, 1)


def _first_align(tgt, src, k, lib_path):
    """wall time of the first FAST_GICP align of a frame pair on a fresh pair of clouds: both covariance passes, both index builds and the
    optimiser; the handle has aligned another pair before (no first-launch costs)"""
    import time
    r = Registration("FAST_GICP", lib_path=lib_path, gicp_correspondence_randomness=k, gicp_max_correspondence_distance=2.0,
                     transformation_epsilon=0.1)
    out = []
    for _ in range(4):                                     # the first is the warm-up
        r.setInputTarget(tgt)
        r.setInputSource(src)
        r.synchronize()
        t0 = time.perf_counter()
        r.align()
        r.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    r.close()
    return statistics.median(out[1:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--passes", type=int, default=20)
    ap.add_argument("--lib", default=None)
    ap.add_argument("--ks", default="20,32,33,40,64")
    ap.add_argument("--first-align", action="store_true", help="time the first FAST_GICP align of a cfg3 frame pair at k = 20 and 40 instead")
    a = ap.parse_args()
    if a.first_align:
        frames = synth.vlp16_stream(n_frames=2)[0]
        tgt, src = (np.ascontiguousarray(f, np.float32) for f in frames[:2])
        for k in (20, 40):
            if k > 32 and a.lib is not None:
                continue
            runs = [_first_align(tgt, src, k, a.lib) for _ in range(a.runs)]
            print(json.dumps({"first_align": "cfg3 frame 1 on frame 0", "n": [int(tgt.shape[0]), int(src.shape[0])], "k": k,
                              "ms_runs": [round(x, 4) for x in runs], "ms_median": round(statistics.median(runs), 4)}), flush=True)
        return
    clouds = {"cfg2 65,536": np.ascontiguousarray(synth.kitti_pair()[0], np.float32),
              "vlp16 frame": np.ascontiguousarray(synth.vlp16_stream(n_frames=1)[0][0], np.float32)}
    for name, cloud in clouds.items():
        for k in (int(x) for x in a.ks.split(",")):
            for mode in (0, 2):
                for leaf_wide in ((False, True) if k > 32 else (False,)):
                    if k > 32 and a.lib is not None:
                        continue                           # a parent build refuses wide k
                    runs = [_time(cloud, k, mode, leaf_wide, a.passes, a.lib) for _ in range(a.runs)]
                    print(json.dumps({"cloud": name, "n": int(cloud.shape[0]), "k": k, "mode": "upstream_order" if mode == 2 else "default",
                                      "wide_search": ("leaf" if leaf_wide else "walk") if k > 32 else None,
                                      "ms_runs": [round(x, 4) for x in runs], "ms_median": round(statistics.median(runs), 4)}), flush=True)


if __name__ == "__main__":
    main()
