#!/usr/bin/env python3
"""Reads the per-workgroup stamps of the item-compacted NDT kernel that the stamp build leaves (`make stamps` in delta_graph_slam_amd/csrc;
run any workload with DGS_REG_LIB=.../libdgs_reg_stamps.so DGS_DEAL_STAMPS_FILE=out.bin [DGS_DEAL_STAMPS_AT=first launch to record]) and
prints one JSON object:

  per_kind        median / mean workgroup duration (us, start -> end of the derivative work) per evaluation kind, in launches with >= --many
                  active pairs, and the medians relative to their workgroup-weighted mean
  dispatch_order  the share of neighbouring blockIdx whose start times are in order, and the rank correlation of start time with blockIdx
  split_per_kind  wave 0's life per evaluation kind, medians in us over the same workgroups: start -> end of the prologue barrier (dealing,
                  header), its tile prologues and its item loops in all, the row reduction, the drain of the row's stores + barrier, the
                  ticket + barrier; `outside_item_loops_share` = 1 - items / (start -> ticket taken); and the closing of the workgroups that closed
  idle_share      per launch 1 - sum(workgroup durations) / (slots x launch duration), mean over the launches with >= --many active pairs and
                  over the rest (slots: the workgroups the chip holds at once, 512 for this kernel on 256 CUs)
  launch_us       mean launch duration (first start -> last end, closings included) of the two groups

Usage: deal_stamps.py out.bin [--many 16] [--slots 512]"""
import argparse
import json

import numpy as np

LAUNCHES, GRID, WORDS = 256, 2048, 16   # kStampLaunches, kStampGrid, kStampWords (ndt_strict.h)
TICK_US = 0.01                         # wall_clock64: 100 MHz


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("file")
    ap.add_argument("--many", type=int, default=16)
    ap.add_argument("--slots", type=int, default=512)
    a = ap.parse_args()
    raw = np.fromfile(a.file, dtype=np.uint64).reshape(LAUNCHES, GRID, WORDS)
    per_kind = {0: [], 1: [], 2: []}
    split = {k: {p: [] for p in ("prologue", "tile_prologues", "item_loops", "row_reduction", "drain", "ticket", "whole", "closing")} for k in (0, 1, 2)}
    groups = {"many": dict(idle=[], us=[], n=0), "few": dict(idle=[], us=[], n=0)}
    in_order, neighbours, rho = 0, 0, []
    for l in range(LAUNCHES):
        rec = raw[l]
        used = rec[:, 0] != 0
        if not used.any():
            continue
        rec = rec[used]
        t0, t1, t2 = rec[:, 0].astype(np.int64), rec[:, 1].astype(np.int64), rec[:, 2].astype(np.int64)
        block = (rec[:, 3] & np.uint64(0xFFFFFFFF)).astype(np.int64)
        slice1 = (rec[:, 4] & np.uint64(0xFFFFFFFF)).astype(np.int64)    # 0: a solver workgroup
        kind = (rec[:, 4] >> np.uint64(32)).astype(np.int64)
        n_active = int((rec[:, 5] & np.uint64(0xFFFFFFFF)).astype(np.int64).max())
        end = np.maximum(t1, t2)
        span = (end.max() - t0.min()) * TICK_US
        work = slice1 > 0
        busy = ((end - t0) * TICK_US).sum()
        g = groups["many" if n_active >= a.many else "few"]
        g["idle"].append(1.0 - busy / (a.slots * span))
        g["us"].append(span)
        g["n"] += 1
        if n_active >= a.many:
            for k in (0, 1, 2):
                per_kind[k].append(((t1 - t0) * TICK_US)[work & (kind == k)])
                w = rec[work & (kind == k)][:, :12].astype(np.int64)
                for name, ticks in (("prologue", w[:, 6] - w[:, 0]), ("tile_prologues", w[:, 7]), ("item_loops", w[:, 8]), ("row_reduction", w[:, 10] - w[:, 9]),
                                    ("drain", w[:, 1] - w[:, 10]), ("ticket", w[:, 11] - w[:, 1]), ("whole", w[:, 11] - w[:, 0])):
                    split[k][name].append(ticks * TICK_US)
                closed = w[w[:, 2] != 0]
                split[k]["closing"].append((closed[:, 2] - closed[:, 11]) * TICK_US)
        o = np.argsort(block[work])
        s = t0[work][o]
        in_order += int((np.diff(s) >= 0).sum())
        neighbours += s.size - 1
        if s.size > 2:
            r = np.argsort(np.argsort(s, kind="stable"))
            rho.append(float(np.corrcoef(r, np.arange(s.size))[0, 1]))
    out = {"launches": {k: v["n"] for k, v in groups.items()}, "many_means_n_active_at_least": a.many, "slots": a.slots}
    med, cnt = {}, {}
    out["per_kind"] = {}
    for k in (0, 1, 2):
        d = np.concatenate(per_kind[k]) if per_kind[k] else np.zeros(0)
        cnt[k] = int(d.size)
        med[k] = float(np.median(d)) if d.size else None
        out["per_kind"][str(k)] = {"workgroups": cnt[k], "median_us": med[k], "mean_us": float(d.mean()) if d.size else None,
                                   "p10_us": float(np.percentile(d, 10)) if d.size else None, "p90_us": float(np.percentile(d, 90)) if d.size else None}
    tot = sum(cnt.values())
    if tot and all(med[k] is not None for k in med):
        mean = sum(med[k] * cnt[k] for k in med) / tot
        out["per_kind_relative_to_mean"] = {str(k): med[k] / mean for k in med}
        out["mix"] = {str(k): cnt[k] / tot for k in cnt}
        out["heaviest_first"] = sorted(med, key=lambda k: -med[k])
    out["split_per_kind"] = {}
    for k in (0, 1, 2):
        parts = {name: np.concatenate(v) if v else np.zeros(0) for name, v in split[k].items()}
        if not parts["whole"].size:
            continue
        row = {name + "_median_us": float(np.median(v)) for name, v in parts.items() if v.size}
        row["outside_item_loops_share"] = float(1.0 - parts["item_loops"].sum() / parts["whole"].sum())
        out["split_per_kind"][str(k)] = row
    out["dispatch_order"] = {"neighbouring_blockIdx_started_in_order": in_order / max(1, neighbours), "mean_rank_correlation": float(np.mean(rho)) if rho else None}
    out["idle_share"] = {k: (float(np.mean(v["idle"])) if v["idle"] else None) for k, v in groups.items()}
    out["launch_us"] = {k: (float(np.mean(v["us"])) if v["us"] else None) for k, v in groups.items()}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
