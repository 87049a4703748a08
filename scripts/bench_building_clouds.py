"""The two shapes in which the nodelet samples lines into clouds, on the device and in the numpy restatement
(tests/building_cloud_reference.py) on the same inputs.  Not bench.py: recorded in DESIGN.md 6m, not gated.

  frame: what a synchronised frame does (apps/delta_graph_slam_nodelet.cpp:280-288, :327-336): about 40 aligned and not-aligned lines,
         about 2 x 10^4 points, one shared transform (map_pose4f).
  tick:  what publish_buildings_clouds does (:751-757): 200 buildings of 12 lines, about 10^6 points, a transform per building.

The device time is taken with HIP events on the handle's stream around dgs_building_cloud_generate: from the call's first upload to
the end of the fill kernel, the host's packing and its one wait included.  One JSON line per shape: the median of `--repeats` calls
with the lowest and the highest, the same for the restatement, launches and host waits, and the bytes the fill kernel writes per second
of the whole call (16 bytes per point; the kernel alone is faster than that figure says).

    python scripts/bench_building_clouds.py [--repeats 9] [--warmup 3]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def rigid(deg, tx, ty):
    t = np.deg2rad(deg)
    m = np.eye(4, dtype=np.float32)
    m[0, 0], m[0, 1], m[1, 0], m[1, 1] = np.cos(t), -np.sin(t), np.sin(t), np.cos(t)
    m[0, 3], m[1, 3] = tx, ty
    return m


def frame_scene(seed=0):
    """two lists (aligned, not aligned) of 28 and 12 wall segments of 4 - 16 m around the sensor"""
    rng = np.random.default_rng(seed)
    a = rng.uniform(-40.0, 40.0, (40, 3))
    a[:, 2] = 0.0
    ang = rng.uniform(0.0, 2.0 * np.pi, 40)
    length = rng.uniform(4.0, 16.0, 40)
    b = a + np.stack([length * np.cos(ang), length * np.sin(ang), np.zeros(40)], axis=1)
    lines = np.stack([a, b], axis=1)
    return [lines[:28], lines[28:]], rigid(33.0, 120.0, -75.0)


def tick_scene(seed=1):
    """200 buildings with a closed outline of 12 walls, 100 m of outline each, and a small pose correction per building"""
    rng = np.random.default_rng(seed)
    items, mats = [], []
    for k in range(200):
        c = np.array([60.0 * (k % 15), 60.0 * (k // 15)]) + rng.uniform(-10.0, 10.0, 2)
        t = np.sort(rng.uniform(0.0, 2.0 * np.pi, 12))
        r = rng.uniform(12.0, 20.0, 12)
        p = np.concatenate([c + np.stack([r * np.cos(t), r * np.sin(t)], axis=1), np.zeros((12, 1))], axis=1)
        q = np.roll(p, -1, axis=0)
        items.append(np.stack([p, q], axis=1))
        mats.append(rigid(rng.uniform(-1.0, 1.0), *rng.uniform(-0.5, 0.5, 2)))
    return items, mats


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    import torch
    import building_cloud_reference as R     # the restatement; no test module is imported
    from delta_graph_slam_amd.building_cloud import BuildingClouds
    from delta_graph_slam_amd.registration import Registration
    assert torch.cuda.is_available(), "this benchmark needs the GPU"
    reg = Registration("NDT_OMP", device=0)
    stream = torch.cuda.Stream()
    reg.set_stream(stream)
    bc = BuildingClouds(registration=reg)

    def spread(ms):
        return [round(statistics.median(ms), 4), round(min(ms), 4), round(max(ms), 4)]

    for what, (items, mats) in (("frame", frame_scene()), ("tick", tick_scene())):
        shared = isinstance(mats, np.ndarray)
        pts, off = bc.clouds(items, mats)
        want, woff = R.clouds(items, mats)
        assert np.array_equal(off, woff) and R.same_bits(pts, want)          # faster and different is not faster
        # the call's arguments, packed once: what a C++ caller holds
        flat = np.concatenate(items)
        feats = np.zeros((flat.shape[0], 10), np.float64)
        feats[:, :6] = flat.reshape(-1, 6)
        loff = np.concatenate([[0], np.cumsum([i.shape[0] for i in items])]).astype(np.int64)
        m16 = np.ascontiguousarray(np.array([m.T.reshape(16) for m in ([mats] if shared else mats)], np.float32))
        index = None if shared else np.arange(len(items), dtype=np.int32)
        total = C.c_int64(0)

        def call():
            rc = bc._lib.dgs_building_cloud_generate(bc._h, C.byref(bc.params), feats.ctypes.data, loff.ctypes.data, len(items), m16.ctypes.data,
                                                     None if index is None else index.ctypes.data, C.byref(total))
            assert rc == 0, rc

        dev_ms, wall_ms = [], []
        with torch.cuda.stream(stream):
            for it in range(args.warmup + args.repeats):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                stream.synchronize()
                t0 = time.perf_counter()
                e0.record(stream)
                call()
                e1.record(stream)
                e1.synchronize()
                t1 = time.perf_counter()
                if it >= args.warmup:
                    dev_ms.append(e0.elapsed_time(e1))
                    wall_ms.append((t1 - t0) * 1e3)
        counts = bc.counts()
        py_ms = []
        for it in range(args.repeats):
            t0 = time.perf_counter()
            bc.clouds(items, mats)
            py_ms.append((time.perf_counter() - t0) * 1e3)
        ref_ms = []
        for it in range(args.repeats):
            t0 = time.perf_counter()
            R.clouds(items, mats)
            ref_ms.append((time.perf_counter() - t0) * 1e3)
        med = statistics.median(dev_ms)
        print(json.dumps(dict(what=what, items=len(items), lines=int(flat.shape[0]), points=int(total.value), transforms=int(m16.shape[0]),
                              device_call_events_ms=spread(dev_ms), device_call_wall_ms=spread(wall_ms),
                              python_call_with_copy_out_ms=spread(py_ms), numpy_restatement_ms=spread(ref_ms),
                              launches=int(counts["launches"]), host_waits=int(counts["host_waits"]), table_entries=int(counts["table_entries"]),
                              bytes_written=int(total.value) * 16, gb_per_s_over_the_call=round(total.value * 16 / (med * 1e-3) / 1e9, 2),
                              repeats=args.repeats, warmup=args.warmup, columns="median, lowest, highest")), flush=True)


if __name__ == "__main__":
    main()
