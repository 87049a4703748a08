"""LineBasedScanmatcher::align_global on the device (upstream src/hdl_graph_slam/line_based_scanmatcher.cpp:109-203;
dgs_line_align_global in include/dgs_reg.h).

`LineScanMatcher(params)` takes the matcher's `g_*` member names (line_based_scanmatcher.hpp:142-146), the nodelet's
`delta_global_*` parameter names (apps/delta_graph_slam_nodelet.cpp:98-102) and, for a cloud source, the line extraction's
parameters.  `align_global(source, lines_target, constrain_angle, max_range)` takes the source as a list of `LineFeature` or as the
flat cloud (float32 [N,4], numpy or device tensor), which goes through a `LineExtractor` on the same handle first; an extraction that
yields no lines falls through as upstream does (the identity with the empty score).  `merge_lines` and `edge_extraction` are the
host-only pieces and need no GPU.

`LineScanMatcher.edge_extraction(lines, only_angular_edges, max_dist_angular_edge)` and `edge_extraction_batch(items)` are the same
edge extraction on the device (dgs_line_edge_extraction_batch): the same `EdgeFeature` objects, bit for bit.  The
parameter `edges_on_device=1` makes align_global and align_local / align_local_batch take their edges from those kernels instead of the
host (the default, 0); the results are identical, the call pays one more host wait.

`align_local(lines_source, lines_target, max_range)` and `align_local_batch(items, max_range)` are LineBasedScanmatcher::align_local
(:205-297; dgs_line_align_local_batch): a batch of independent (source lines, target lines) items -- a keyframe's near
buildings -- goes to the device in one call.  The matcher's `l_*` members and the nodelet's `delta_local_*` names set weight_local,
except `delta_local_avg_distance_weight`: upstream's setter of that name writes the global member, so the nodelet never changes
l_avg_distance_weight; the name is accepted and ignored here, as dgs::HipLineAligner does not read it.

`align_overlapped(lines_source, lines_target, center_source, center_target)` and `align_overlapped_batch(items)` are
LineBasedScanmatcher::align_overlapped_buildings (:29-107; dgs_line_align_overlapped_batch) from the building-frame lines
on: the smallest move of the source building that passes the pi / 3 angle gate and leaves the two shrunken polygons apart.  The frame
transforms around it stay with the caller.
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass, field
from typing import List, Optional

import numpy as np

from . import _lib as L
from .line_extraction import LineFeature

__all__ = ["LineScanMatcher", "BestFitAlignment", "LocalAlignment", "OverlapAlignment", "FitnessScore", "EdgeFeature", "merge_lines", "edge_extraction",
           "params_from_dict"]

_NAMES = {   # member name -> the nodelet's parameter name
    "g_avg_distance_weight": "delta_global_avg_distance_weight", "g_coverage_weight": "delta_global_coverage_weight",
    "g_transform_weight": "delta_global_transform_weight", "g_max_score_distance": "delta_global_max_score_distance",
    "g_max_score_translation": "delta_global_max_score_translation",
    # delta_local_avg_distance_weight does not set l_avg_distance_weight: upstream's setter of that name (line_based_scanmatcher.hpp:117)
    # writes the global member, so the nodelet never changes the local one; dgs::HipLineAligner does not read it either.  params_from_dict
    # accepts and ignores the name; the member name sets the weight.
    "l_avg_distance_weight": None, "l_coverage_weight": "delta_local_coverage_weight",
    "l_transform_weight": "delta_local_transform_weight", "l_max_score_distance": "delta_local_max_score_distance",
    "l_max_score_translation": "delta_local_max_score_translation",
}
_EXTRA = ("max_distance", "max_angle", "l_max_distance", "l_max_angle", "angle_gate_float_chain", "nn_tie_highest_index", "refine_three_nearest",
          "edges_on_device")


@dataclass
class FitnessScore:
    real_avg_distance: float
    avg_distance: float
    coverage: float
    coverage_percentage: float


@dataclass
class EdgeFeature:
    edgePoint: np.ndarray
    pointA: np.ndarray
    pointB: np.ndarray


@dataclass
class BestFitAlignment:
    not_aligned_lines: List[LineFeature]
    aligned_lines: List[LineFeature]
    transformation: np.ndarray            # 4 x 4 float64
    fitness_score: FitnessScore
    score: float = 0.0                    # weight_global of the result
    winner: int = -1                      # the winning hypothesis h = es * Et + et; -1 when none beat the identity
    refine_steps: int = 0
    status: str = "NONE_BETTER"           # L.LA_STATUS
    counts: dict = field(default_factory=dict)   # hypotheses, survivors, edges_source, edges_target, lines_target


@dataclass
class LocalAlignment(BestFitAlignment):
    """align_local's BestFitAlignment; `winner` is the edge-pair phase's h, `winner_line` the line-pair phase's k = i * Lt + r."""
    isEdgeAligned: bool = False
    winner_line: int = -1
    edge_transformation: Optional[np.ndarray] = None      # best_trans: the edge-pair phase's result
    edge_fitness_score: Optional[FitnessScore] = None
    edge_score: float = 0.0
    baseline_fitness_score: Optional[FitnessScore] = None
    baseline_score: float = 0.0


@dataclass
class OverlapAlignment:
    """align_overlapped_buildings' BestFitAlignment in the source building's frame (upstream sets no fitness score there)."""
    not_aligned_lines: List[LineFeature]
    aligned_lines: List[LineFeature]
    transformation: np.ndarray            # 4 x 4 float64: the winner's transform, or the identity
    translation_norm: float               # DBL_MAX without a winner
    winner: int                           # h = es * Et + et, then Es * Et + i * Lt + j; -1: none
    is_identity: bool                     # the nodelet adds no edge then (:875)
    status: str                           # L.LA_STATUS
    counts: dict = field(default_factory=dict)   # hypotheses_edge, hypotheses_line, angle_passed, not_overlapped, edges_source, edges_target


def params_from_dict(params: Optional[dict] = None):
    """-> (LineAlignParams, the remaining entries): the constructor's defaults (line_based_scanmatcher.hpp:91-95), align_global's 2.0 and
    pi / 9, overridden by `params`; what is not an alignment parameter is left for the line extraction."""
    pr = dict(params or {})
    pr.pop("delta_local_avg_distance_weight", None)
    p = L.LineAlignParams()
    rc = L.load().dgs_line_align_params_init(C.byref(p))
    if rc:
        raise L.DgsError(rc, "dgs_line_align_params_init")
    for member, ros in _NAMES.items():
        for k in (ros, member):
            if k is not None and k in pr:
                setattr(p, member, float(pr.pop(k)))
    for k in _EXTRA:
        if k in pr:
            v = pr.pop(k)
            setattr(p, k, float(v) if "max_" in k else int(v))
    return p, pr


def _to_c(lines):
    arr = (L.LineFeatureC * max(len(lines), 1))()
    for f, l in zip(arr, lines):
        f.point_a[:] = [float(v) for v in np.asarray(l.pointA, np.float64)]
        f.point_b[:] = [float(v) for v in np.asarray(l.pointB, np.float64)]
        f.mean_error, f.std_sigma, f.max_error, f.min_error = float(l.mean_error), float(l.std_sigma), float(l.max_error), float(l.min_error)
    return arr


def _from_c(arr, n):
    return [LineFeature(np.array(f.point_a[:], np.float64), np.array(f.point_b[:], np.float64), f.mean_error, f.std_sigma, f.max_error,
                        f.min_error) for f in arr[:n]]


def _check(rc, what):
    if rc:
        raise L.DgsError(rc, what)


def merge_lines(lines: List[LineFeature]) -> List[LineFeature]:
    """merge_lines (:1086-1103) on the host; no handle, no device."""
    out = (L.LineFeatureC * max(len(lines), 1))()
    n = C.c_int64(0)
    _check(L.load().dgs_line_merge(C.cast(_to_c(lines), C.c_void_p), len(lines), C.cast(out, C.c_void_p), C.byref(n)), "dgs_line_merge")
    return _from_c(out, n.value)


def edge_extraction(lines: List[LineFeature], only_angular_edges: Optional[bool] = None, max_dist_angular_edge: float = 7.0) -> List[EdgeFeature]:
    """edge_extraction (:459-471) on the host; no handle, no device.  With `only_angular_edges` given, upstream's two further arguments
    go through dgs_line_edges_angular."""
    lib = L.load()
    arr = _to_c(lines)
    n = C.c_int64(0)
    if only_angular_edges is None:
        call = lambda buf, cap: lib.dgs_line_edges(C.cast(arr, C.c_void_p), len(lines), buf, cap, C.byref(n))
    else:
        call = lambda buf, cap: lib.dgs_line_edges_angular(C.cast(arr, C.c_void_p), len(lines), 1 if only_angular_edges else 0,
                                                           float(max_dist_angular_edge), buf, cap, C.byref(n))
    rc = call(None, 0)
    if rc and n.value == 0:
        _check(rc, "dgs_line_edges")
    out = (L.EdgeFeatureC * max(n.value, 1))()
    _check(call(C.cast(out, C.c_void_p), n.value), "dgs_line_edges")
    return [EdgeFeature(np.array(e.edge_point[:]), np.array(e.point_a[:]), np.array(e.point_b[:])) for e in out[:n.value]]


class LineScanMatcher:
    def __init__(self, params: Optional[dict] = None, registration=None, device: Optional[int] = None):
        from .line_extraction import LineExtractor
        from .registration import Registration
        self.params, rest = params_from_dict(params)
        if registration is None:
            registration = Registration("NDT_OMP", device=device)   # any handle: only its stream and the aligner's own buffers are used
        self.registration = registration
        self._lib = registration._lib
        self.extractor = LineExtractor(rest, registration=registration)
        self._local_sizes = []
        self._overlap_sizes = []

    @property
    def _h(self):
        return self.registration._h

    def align_global(self, source, lines_target: List[LineFeature], constrain_angle: bool = False, max_range: float = math.inf) -> BestFitAlignment:
        if isinstance(source, (list, tuple)):
            lines_source = list(source)
        else:
            lines_source = self.extractor.extract(source)
        n = len(lines_source)
        src = _to_c(lines_source)
        out = (L.LineFeatureC * max(n, 1))()
        al = L.LineAlignment()
        self.registration._check(self._lib.dgs_line_align_global(
            self._h, C.byref(self.params), C.cast(src, C.c_void_p), n, C.cast(_to_c(lines_target), C.c_void_p), len(lines_target),
            1 if constrain_angle else 0, float(max_range), C.cast(out, C.c_void_p), C.byref(al)))
        return BestFitAlignment(
            not_aligned_lines=lines_source, aligned_lines=_from_c(out, n), transformation=np.array(al.transformation[:], np.float64).reshape(4, 4),
            fitness_score=FitnessScore(*al.fitness_score[:]), score=al.score, winner=al.winner, refine_steps=al.refine_steps,
            status=L.LA_STATUS[al.status],
            counts=dict(hypotheses=al.n_hypotheses, survivors=al.n_survivors, edges_source=al.n_edges_source, edges_target=al.n_edges_target,
                        lines_target=al.n_lines_target))

    def align_local(self, lines_source: List[LineFeature], lines_target: List[LineFeature], max_range: float = 0.5) -> "LocalAlignment":
        """align_local (:205-297) of one item: a batch of one."""
        return self.align_local_batch([(lines_source, lines_target)], max_range)[0]

    def align_local_batch(self, items, max_range: float = 0.5) -> List["LocalAlignment"]:
        """`items`: a sequence of (lines_source, lines_target) pairs, e.g. (building lines, the keyframe's lines in that building's frame)
        for every near building.  One device call: one upload, one download, one host wait, a fixed number of launches."""
        items = [(list(s), list(t)) for s, t in items]
        n = len(items)
        so = (C.c_int64 * (n + 1))()
        to = (C.c_int64 * (n + 1))()
        for b, (s, t) in enumerate(items):
            so[b + 1], to[b + 1] = so[b] + len(s), to[b] + len(t)
        src = _to_c([l for s, _ in items for l in s])
        trg = _to_c([l for _, t in items for l in t])
        out = (L.LineFeatureC * max(so[n], 1))()
        al = (L.LineLocalAlignment * max(n, 1))()
        self.registration._check(self._lib.dgs_line_align_local_batch(
            self._h, C.byref(self.params), n, C.cast(src, C.c_void_p), C.cast(so, C.c_void_p), C.cast(trg, C.c_void_p), C.cast(to, C.c_void_p),
            float(max_range), C.cast(out, C.c_void_p), C.cast(al, C.c_void_p)))
        aligned = _from_c(out, so[n])
        self._local_sizes = [(al[b].n_hypotheses_edge, al[b].n_hypotheses_line) for b in range(n)]   # what local_hypotheses may read
        res = []
        for b, (s, t) in enumerate(items):
            a = al[b]
            res.append(LocalAlignment(
                not_aligned_lines=s, aligned_lines=aligned[so[b]:so[b + 1]], transformation=np.array(a.transformation[:], np.float64).reshape(4, 4),
                fitness_score=FitnessScore(*a.fitness_score[:]), score=a.score, winner=a.winner_edge, status=L.LA_STATUS[a.status],
                counts=dict(hypotheses_edge=a.n_hypotheses_edge, survivors_edge=a.n_survivors_edge, hypotheses_line=a.n_hypotheses_line,
                            survivors_line=a.n_survivors_line, edges_source=a.n_edges_source, edges_target=a.n_edges_target),
                isEdgeAligned=bool(a.is_edge_aligned), winner_line=a.winner_line,
                edge_transformation=np.array(a.edge_transformation[:], np.float64).reshape(4, 4),
                edge_fitness_score=FitnessScore(*a.edge_fitness_score[:]), edge_score=a.edge_score,
                baseline_fitness_score=FitnessScore(*a.baseline_fitness_score[:]), baseline_score=a.baseline_score))
        return res

    def align_overlapped(self, lines_source: List[LineFeature], lines_target: List[LineFeature], center_source=(0.0, 0.0, 0.0),
                         center_target=(0.0, 0.0, 0.0)) -> "OverlapAlignment":
        """align_overlapped_buildings (:29-107) of one pair in the source building's frame: a batch of one."""
        return self.align_overlapped_batch([(lines_source, lines_target, center_source, center_target)])[0]

    def align_overlapped_batch(self, items) -> List["OverlapAlignment"]:
        """`items`: a sequence of (lines_source, lines_target, center_source, center_target), e.g. every overlapped pair (A, B) of a round
        in A's frame.  One device call: one upload, one download, one host wait, three launches."""
        items = [(list(s), list(t), cs, ct) for s, t, cs, ct in items]
        n = len(items)
        so = (C.c_int64 * (n + 1))()
        to = (C.c_int64 * (n + 1))()
        for b, (s, t, _, _) in enumerate(items):
            so[b + 1], to[b + 1] = so[b] + len(s), to[b] + len(t)
        src = _to_c([l for it in items for l in it[0]])
        trg = _to_c([l for it in items for l in it[1]])
        cs = np.ascontiguousarray(np.array([np.asarray(it[2], np.float64).reshape(3) for it in items], np.float64).reshape(-1, 3))
        ct = np.ascontiguousarray(np.array([np.asarray(it[3], np.float64).reshape(3) for it in items], np.float64).reshape(-1, 3))
        out = (L.LineFeatureC * max(so[n], 1))()
        al = (L.LineOverlapAlignment * max(n, 1))()
        self.registration._check(self._lib.dgs_line_align_overlapped_batch(
            self._h, C.byref(self.params), n, C.cast(src, C.c_void_p), C.cast(so, C.c_void_p), C.cast(trg, C.c_void_p), C.cast(to, C.c_void_p),
            cs.ctypes.data if n else None, ct.ctypes.data if n else None, C.cast(out, C.c_void_p), C.cast(al, C.c_void_p)))
        aligned = _from_c(out, so[n])
        self._overlap_sizes = [al[b].n_hypotheses_edge + al[b].n_hypotheses_line for b in range(n)]   # what overlapped_hypotheses may read
        return [OverlapAlignment(
            not_aligned_lines=it[0], aligned_lines=aligned[so[b]:so[b + 1]], transformation=np.array(al[b].transformation[:], np.float64).reshape(4, 4),
            translation_norm=al[b].translation_norm, winner=al[b].winner, is_identity=bool(al[b].is_identity), status=L.LA_STATUS[al[b].status],
            counts=dict(hypotheses_edge=al[b].n_hypotheses_edge, hypotheses_line=al[b].n_hypotheses_line, angle_passed=al[b].n_angle_passed,
                        not_overlapped=al[b].n_not_overlapped, edges_source=al[b].n_edges_source, edges_target=al[b].n_edges_target))
            for b, it in enumerate(items)]

    def edge_extraction(self, lines: List[LineFeature], only_angular_edges: bool = False, max_dist_angular_edge: float = 7.0) -> List[EdgeFeature]:
        """edge_extraction (:459-471) of one list of lines on the device: a batch of one segment.  The defaults are align_global's call."""
        return self.edge_extraction_batch([(lines, only_angular_edges, max_dist_angular_edge)])[0]

    def edge_extraction_batch(self, items) -> List[List[EdgeFeature]]:
        """`items`: a sequence of (lines, only_angular_edges, max_dist_angular_edge), e.g. (source lines, True, 0.01) and (target lines, True,
        7.0) for align_local.  One list of `EdgeFeature` per item, each what the module-level `edge_extraction` returns for it."""
        arr, off = self._edge_batch_raw(items)
        return [[EdgeFeature(np.array(e[0]), np.array(e[1]), np.array(e[2])) for e in arr[off[b]:off[b + 1]]] for b in range(len(off) - 1)]

    def _edge_batch_raw(self, items):
        """-> (float64 [n_edges, 3, 3]: edgePoint, pointA, pointB; int64 [n_items + 1] edge offsets)."""
        items = [(list(l), bool(o), float(d)) for l, o, d in items]
        n = len(items)
        lo = (C.c_int64 * (n + 1))()
        for b, (l, _, _) in enumerate(items):
            lo[b + 1] = lo[b] + len(l)
        lines = _to_c([f for l, _, _ in items for f in l])
        only = (C.c_int32 * max(n, 1))(*[1 if o else 0 for _, o, _ in items])
        dist = (C.c_double * max(n, 1))(*[d for _, _, d in items])
        eo = (C.c_int64 * (n + 1))()
        ne = C.c_int64(0)
        args = (self._h, C.cast(lines, C.c_void_p), C.cast(lo, C.c_void_p), n, C.cast(only, C.c_void_p), C.cast(dist, C.c_void_p))
        rc = self._lib.dgs_line_edge_extraction_batch(*args, None, 0, C.cast(eo, C.c_void_p), C.byref(ne))   # the count
        if rc and ne.value == 0:
            self.registration._check(rc)
        out = np.zeros((max(ne.value, 1), 3, 3), np.float64)
        self.registration._check(self._lib.dgs_line_edge_extraction_batch(*args, out.ctypes.data, ne.value, C.cast(eo, C.c_void_p), C.byref(ne)))
        return out[:ne.value], np.array(eo[:], np.int64)

    # -- test hooks ----------------------------------------------------------------------------------------------------------
    def edge_counts(self):
        """-> dict(launches, host_waits, pairs, edges) of the last device edge extraction on this handle."""
        c = (C.c_int64 * 4)()
        self.registration._check(self._lib.dgs_line_edges_get_counts(self._h, C.cast(c, C.c_void_p)))
        return dict(launches=c[0], host_waits=c[1], pairs=c[2], edges=c[3])

    def hypotheses(self, first: int = 0, count: Optional[int] = None):
        """Per-hypothesis records of the last call as arrays: gate, slot, rotation [n,4], translation [n,3], fitness [n,4], score."""
        if count is None:
            count = self.counts()["hypotheses"] - first
        rec = (L.LineAlignHypothesis * max(count, 1))()
        self.registration._check(self._lib.dgs_line_align_get_hypotheses(self._h, first, count, C.cast(rec, C.c_void_p), None))
        a = np.frombuffer(rec, dtype=np.dtype([("gate", "<i4"), ("slot", "<i4"), ("rotation", "<f8", 4), ("translation", "<f8", 3),
                                               ("fitness", "<f8", 4), ("score", "<f8")]))[:count]
        return {k: a[k].copy() for k in a.dtype.names}

    def counts(self):
        """-> dict(launches, host_waits, hypotheses, survivors) of the last call's device phase."""
        c = (C.c_int64 * 4)()
        self.registration._check(self._lib.dgs_line_align_get_hypotheses(self._h, 0, 0, None, C.cast(c, C.c_void_p)))
        return dict(launches=c[0], host_waits=c[1], hypotheses=c[2], survivors=c[3])

    def local_hypotheses(self, item: int, phase: int, first: int = 0, count: Optional[int] = None):
        """Per-hypothesis records of the last align_local / align_local_batch call for one item and phase (0: edge pairs, 1: line pairs)
        as arrays: gate, target, rotation [n,4], translation [n,3], fitness [n,4], score.  `count` None: all of the item's hypotheses of
        that phase from `first` on."""
        if count is None:
            count = self._local_sizes[item][phase] - first
        rec = (L.LineAlignLocalHypothesis * max(count, 1))()
        self.registration._check(self._lib.dgs_line_align_local_get_hypotheses(self._h, item, phase, first, count, C.cast(rec, C.c_void_p), None))
        a = np.frombuffer(rec, dtype=np.dtype([("gate", "<i4"), ("target", "<i4"), ("rotation", "<f8", 4), ("translation", "<f8", 3),
                                               ("fitness", "<f8", 4), ("score", "<f8")]))[:count]
        return {k: a[k].copy() for k in a.dtype.names}

    def local_counts(self):
        """-> dict(launches, host_waits, items, hypotheses_edge, hypotheses_line, survivors_edge, survivors_line, workgroups) of the last
        align_local / align_local_batch call."""
        c = (C.c_int64 * 8)()
        self.registration._check(self._lib.dgs_line_align_local_get_hypotheses(self._h, 0, 0, 0, 0, None, C.cast(c, C.c_void_p)))
        return dict(launches=c[0], host_waits=c[1], items=c[2], hypotheses_edge=c[3], hypotheses_line=c[4], survivors_edge=c[5],
                    survivors_line=c[6], workgroups=c[7])

    def overlapped_hypotheses(self, item: int, first: int = 0, count: Optional[int] = None):
        """Per-hypothesis records of the last align_overlapped / align_overlapped_batch call for one item as arrays: gate, rotation [n,4],
        translation [n,3], tn.  `count` None: all of the item's hypotheses from `first` on."""
        if count is None:
            count = self._overlap_sizes[item] - first
        rec = (L.LineAlignOverlappedHypothesis * max(count, 1))()
        self.registration._check(self._lib.dgs_line_align_overlapped_get_hypotheses(self._h, item, first, count, C.cast(rec, C.c_void_p)))
        a = np.frombuffer(rec, dtype=np.dtype([("gate", "<i4"), ("reserved", "<i4"), ("rotation", "<f8", 4), ("translation", "<f8", 3),
                                               ("tn", "<f8")]))[:count]
        return {k: a[k].copy() for k in ("gate", "rotation", "translation", "tn")}

    def overlapped_counts(self):
        """-> dict(launches, host_waits, items, hypotheses) of the last align_overlapped / align_overlapped_batch call."""
        c = (C.c_int64 * 8)()
        self.registration._check(self._lib.dgs_building_overlap_get_counts(self._h, C.cast(c, C.c_void_p)))
        return dict(launches=c[4], host_waits=c[5], items=c[6], hypotheses=c[7])
