#!/usr/bin/env python
"""ms per align_global (LineScanMatcher.align_global from a line list) with the lines of the synthetic HDL-64 and VLP-16 street scans
(prefilter chain and line extraction with the launch file's values) against a ring of synthetic rectangular buildings, once with few
and once with many buildings.  The library runs on the handle's own stream and the call blocks the host, so the HIP events around it
(recorded on the framework's stream) measure the host wall time of the whole call: the ctypes marshalling of every line, the host's
merge and edge extraction, the kernels, the one wait and the refinement pass -- what a frame pays from Python.  `ms_library` is the
same interval around dgs_line_align_global alone, with the lines already marshalled.  Medians of --repeats runs after one warm-up;
hypotheses, survivors, kernel launches and host waits; the numpy restatement's wall time (median of --ref-repeats) beside it.  One JSON line per case; recorded in DESIGN.md 6f, not gated.

Every row carries the library time twice: `ms_library` with the edges extracted on the host (edges_on_device = 0, the default) and
`ms_library_device_edges` with edges_on_device = 1, in the same run on the same lines, with the two results compared field by field
(`identical`).  `ms_host_edges` is the host's dgs_line_edges over the merged target and over the source alone, `ms_device_edges` the
device extraction of the same two segments alone (dgs_line_edge_extraction_batch, upload and both waits included): the split DESIGN.md
6l records.  The `crossing` scene (tests/line_edges_scenes.py) is a scan that sees two perpendicular facades of a few buildings, so the
source has edges and the search kernels run at scale; the street scans' walls are parallel and give Es = 0.  --runs N repeats the whole
measurement N times (the spread DESIGN.md 5 uses).
Under `rocprofv3 --kernel-trace --stats -- python scripts/bench_line_align.py --no-reference` the kernel table gives the split."""
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
from delta_graph_slam_amd.line_align import LineScanMatcher  # noqa: E402
from delta_graph_slam_amd.line_extraction import LineExtractor, LineFeature   # noqa: E402
from delta_graph_slam_amd.prefilter import Prefilter       # noqa: E402
from delta_graph_slam_amd.registration import Registration  # noqa: E402

PF_LAUNCH = dict(distance_near_thresh=0.1, outlier_removal_method="RADIUS", radius_radius=0.5, radius_min_neighbors=2)
LE_LAUNCH = dict(min_cluster_size=40, max_cluster_size=25000, cluster_tolerance=1.5, sac_distance_threshold=0.1, max_iterations=100,
                 merror_threshold=0.1, line_length_threshold=1.5)
SCANS = {"hdl64": dict(beams=64, elev_deg=(2.0, -24.8), azimuths=2048, seed=31), "vlp16": dict(beams=16, elev_deg=(15.0, -15.0), azimuths=1875, seed=21)}


def measure(reg, name, nb, lines, tl, src, trg, args, R):
    """One row: align_global of `lines` against `tl`, host edges and device edges."""
    import ctypes as C
    from delta_graph_slam_amd import _lib as L
    from delta_graph_slam_amd.line_align import _to_c, merge_lines
    import line_edges_scenes as S
    m = LineScanMatcher(registration=reg)
    res = m.align_global(lines, tl)
    ms = []
    for _ in range(args.repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        res = m.align_global(lines, tl)
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    cs, ct = _to_c(lines), _to_c(tl)
    co, al = (L.LineFeatureC * max(len(lines), 1))(), L.LineAlignment()

    def library(on):
        m.params.edges_on_device = on
        t_ms = []
        for k in range(args.repeats + 1):                    # the first call of a mode sizes its buffers: not timed
            t = time.perf_counter()
            reg._check(m._lib.dgs_line_align_global(m._h, C.byref(m.params), C.cast(cs, C.c_void_p), len(lines), C.cast(ct, C.c_void_p), len(tl), 0,
                                                    float("inf"), C.cast(co, C.c_void_p), C.byref(al)))
            if k:
                t_ms.append((time.perf_counter() - t) * 1e3)
        rec = bytes(al) + bytes(co)
        return float(np.median(t_ms)), rec, m.counts()

    lib_dev, rec_dev, c_dev = library(1)
    lib_ms, rec_host, c = library(0)
    # the edge extraction alone, on the merged target and the source: host function, and the device call with its upload and waits
    merged = merge_lines(tl)
    segs = [src, np.array([[l.pointA, l.pointB] for l in merged], np.float64).reshape(-1, 2, 3)]
    t_host, t_dev = [], []
    feats = [S.features(sg) for sg in segs]
    room = np.zeros((max(res.counts["edges_source"], res.counts["edges_target"], 1), 3, 3))
    ne = C.c_int64(0)
    for _ in range(args.repeats):
        t = time.perf_counter()
        for sg, f in zip(segs, feats):                       # one call per side with room for its edges, as the aligner's host path pays it
            assert reg._lib.dgs_line_edges_angular(f.ctypes.data, len(sg), 0, 7.0, room.ctypes.data, room.shape[0], C.byref(ne)) == 0
        t_host.append((time.perf_counter() - t) * 1e3)
    for k in range(args.repeats + 1):
        t = time.perf_counter()
        rc, e, _, _ = S.device_batch_raw(reg._lib, reg._h, segs, [(False, 7.0)] * 2, capacity=res.counts["edges_source"] + res.counts["edges_target"])
        if k:
            t_dev.append((time.perf_counter() - t) * 1e3)
    out = dict(scan=name, buildings=nb, lines_source=len(lines), lines_target=res.counts["lines_target"], edges_source=res.counts["edges_source"],
               edges_target=res.counts["edges_target"], hypotheses=c["hypotheses"], survivors=c["survivors"], winner=res.winner,
               refine_steps=res.refine_steps, status=res.status, score=res.score, ms_median=float(np.median(ms)), ms_min=float(min(ms)),
               ms_max=float(max(ms)), ms_library=lib_ms, ms_library_device_edges=lib_dev, identical=rec_dev == rec_host,
               ms_host_edges=float(np.median(t_host)), ms_device_edges=float(np.median(t_dev)), launches=c["launches"], host_waits=c["host_waits"],
               launches_device_edges=c_dev["launches"], host_waits_device_edges=c_dev["host_waits"])
    if not args.no_reference:
        rs = []
        for _ in range(args.ref_repeats):
            t = time.perf_counter()
            ref = R.align_global(src, trg)
            rs.append(time.perf_counter() - t)
        out.update(restatement_s=float(np.median(rs)), restatement_winner=ref["winner"], restatement_score=ref["score_final"])
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--ref-repeats", type=int, default=3)
    ap.add_argument("--no-reference", action="store_true")
    ap.add_argument("--buildings", type=int, nargs="+", default=[8, 32, 64])
    ap.add_argument("--scenes", nargs="+", default=["hdl64", "vlp16", "crossing"], choices=["hdl64", "vlp16", "crossing"])
    ap.add_argument("--runs", type=int, default=1)
    args = ap.parse_args()
    import line_align_reference as R
    import line_edges_scenes as S
    reg = Registration("NDT_OMP", device=0)
    feat = lambda arr: [LineFeature(t[0].copy(), t[1].copy(), 0.0, 0.0, 0.0, 0.0) for t in arr]
    for _ in range(args.runs):
        for scan_name, sc in SCANS.items():
            if scan_name not in args.scenes:
                continue
            xyz, _ = synth.street_scan((-30.0, 1.0, 0.1), sc["beams"], sc["elev_deg"], sc["azimuths"], sc["seed"])
            scan = np.concatenate([xyz, np.ones((xyz.shape[0], 1))], 1).astype(np.float32)
            _, flat, _ = Prefilter(PF_LAUNCH, registration=reg).filter_scan(torch.from_numpy(scan).cuda())
            lines = LineExtractor(LE_LAUNCH, registration=reg).extract(flat)
            src = np.array([[l.pointA, l.pointB] for l in lines], np.float64).reshape(-1, 2, 3)
            for nb in args.buildings:
                # the scan's own lines seen from a pose that is off by (0.3, -0.2) m and 2 degrees, among a ring of other buildings
                trg = np.concatenate([R.move(src, 0.3, -0.2, np.deg2rad(2.0)), R.ring(nb, radius=35.0, seed=nb)])
                measure(reg, scan_name, nb, lines, feat(trg), src, trg, args, R)
        if "crossing" in args.scenes:
            for nb in args.buildings:
                src, trg = S.crossing(nb)
                measure(reg, "crossing", nb, feat(src), feat(trg), src, trg, args, R)


if __name__ == "__main__":
    main()
