"""The overlap rounds of the optimisation tick (apps/delta_graph_slam_nodelet.cpp:857-899): the pair search over all buildings and the
batched align_overlapped_buildings of the overlapped pairs, on the device against the shared header compiled for the host
(tests/cpp/building_overlap_driver.cpp, mode `host`) on the same inputs.  Not bench.py: recorded in DESIGN.md 6h, not gated.

Buildings are rectangles and L-shapes on a jittered grid, a few percent of them overlapped.  One JSON line per size: the median of
`--repeats` calls, and over `--runs` repetitions of that the lowest and highest median (the run-to-run spread).

    python scripts/bench_building_overlap.py [--buildings 256 1024 4096] [--pairs 8 32 64] [--repeats 30] [--warmup 5] [--runs 3]
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


def city(B, seed=0, pitch=16.0, jitter=3.4):
    import building_overlap_reference as BR     # the scene helpers and the driver's file formats; no test module is imported
    rng = np.random.default_rng(seed)
    side = int(np.ceil(np.sqrt(B)))
    bl, ce = [], []
    for k in range(B):
        cx, cy = pitch * (k % side) + rng.uniform(-jitter, jitter), pitch * (k // side) + rng.uniform(-jitter, jitter)
        w, h, ang = rng.uniform(7, 11), rng.uniform(6, 11), rng.uniform(0, np.pi)
        bl.append(BR.rectangle(cx, cy, w, h, ang) if rng.integers(0, 2) else BR.l_shape(cx, cy, w, h, 0.4 * w, 0.45 * h, ang))
        ce.append([cx, cy, 0.0])
    return bl, np.array(ce, np.float64).reshape(B, 3)


def in_source_frame(a, ca, b, cb):
    """The pair in a frame whose origin is A's centre: the stand-in for the caller's building_pose.inverse()"""
    return a - ca, b - ca, np.zeros(3), cb - ca


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--buildings", type=int, nargs="+", default=[256, 1024, 4096])
    ap.add_argument("--pairs", type=int, nargs="+", default=[8, 32, 64])
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--runs", type=int, default=3)
    args = ap.parse_args()
    import building_overlap_reference as BR
    from delta_graph_slam_amd.building_overlap import BuildingOverlap
    from delta_graph_slam_amd.line_align import LineScanMatcher
    from delta_graph_slam_amd.registration import Registration
    from line_align_local_reference import feature_lines
    reg = Registration("NDT_OMP", device=0)
    ov, m = BuildingOverlap(registration=reg), LineScanMatcher(registration=reg)
    tmp = tempfile.mkdtemp()
    exe = os.path.join(tmp, "building_overlap_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "building_overlap_driver.cpp"), "-o", exe,
                           os.path.join(ROOT, "delta_graph_slam_amd", "libdgs_reg.so"), "-Wl,-rpath," + os.path.join(ROOT, "delta_graph_slam_amd"),
                           "-Wl,-rpath,/opt/rocm/lib"])

    def timed(fn):
        meds = []
        for _ in range(args.runs):
            for _ in range(args.warmup):
                fn()
            t = []
            for _ in range(args.repeats):
                t0 = time.perf_counter()
                fn()
                t.append((time.perf_counter() - t0) * 1e3)
            meds.append(statistics.median(t))
        return [round(statistics.median(meds), 4), round(min(meds), 4), round(max(meds), 4)]

    def driver(mode, what, ip, op, repeats):
        meds = [json.loads(subprocess.check_output([exe, mode, what, ip, op, f"repeat={repeats}"]).decode().splitlines()[-1]) for _ in range(args.runs)]
        assert all(r["ok"] for r in meds), meds
        ms = [r["ms_per_call"] for r in meds]
        return [round(statistics.median(ms), 4), round(min(ms), 4), round(max(ms), 4)], meds[0]["count"]

    ip, op = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    pool = None
    for B in args.buildings:
        bl, ce = city(B)
        device_ms = timed(lambda: ov.overlapped_pairs(bl, ce))
        c = ov.counts()
        BR.write_buildings(ip, bl, ce)
        lib_ms, n_dev = driver("device", "pairs", ip, op, args.repeats)
        dev_pairs = np.fromfile(op, np.int32).reshape(-1, 2)
        host_ms, n_host = driver("host", "pairs", ip, op, max(3, args.repeats // 10) if B >= 2048 else args.repeats)
        assert np.array_equal(dev_pairs, np.fromfile(op, np.int32).reshape(-1, 2))
        print(json.dumps(dict(what="pair_search", buildings=B, lines=int(sum(b.shape[0] for b in bl)), pairs=int(n_dev),
                              buildings_in_a_pair=round(float(np.unique(dev_pairs).size) / B, 4), device_call_python_ms=device_ms,
                              library_alone_ms=lib_ms, host_header_ms=host_ms, launches=c["launches"], host_waits=c["host_waits"],
                              repeats=args.repeats, warmup=args.warmup, runs=args.runs, columns="median, lowest, highest median of the runs")), flush=True)
        pool = (bl, ce, dev_pairs)
    bl, ce, pairs = pool
    for P in args.pairs:
        assert pairs.shape[0] >= P, "the largest city has too few overlapped pairs"
        items = [in_source_frame(bl[i], ce[i], bl[j], ce[j]) for i, j in pairs[:P]]
        feats = [(feature_lines(s), feature_lines(t), cs, ct) for s, t, cs, ct in items]
        device_ms = timed(lambda: m.align_overlapped_batch(feats))
        c = m.overlapped_counts()
        res = m.align_overlapped_batch(feats)
        BR.write_items(ip, items)
        lib_ms, hyp = driver("device", "align", ip, op, args.repeats)
        host_ms, hyp_host = driver("host", "align", ip, op, args.repeats)
        assert hyp == hyp_host == c["hypotheses"]
        print(json.dumps(dict(what="align_overlapped_batch", pairs=P, hypotheses=int(hyp), angle_passed=int(sum(r.counts["angle_passed"] for r in res)),
                              not_overlapped=int(sum(r.counts["not_overlapped"] for r in res)), resolved=sum(r.status == "ALIGNED" for r in res),
                              device_call_python_ms=device_ms, library_alone_ms=lib_ms, host_header_ms=host_ms, launches=c["launches"],
                              host_waits=c["host_waits"], repeats=args.repeats, warmup=args.warmup, runs=args.runs,
                              columns="median, lowest, highest median of the runs")), flush=True)


if __name__ == "__main__":
    main()
