"""LineBasedScanmatcher::align_global on the device (upstream src/hdl_graph_slam/line_based_scanmatcher.cpp:109-203;
dgs_line_align_global in include/dgs_reg.h).

`LineScanMatcher(params)` takes the matcher's `g_*` member names (line_based_scanmatcher.hpp:142-146), the nodelet's
`delta_global_*` parameter names (apps/delta_graph_slam_nodelet.cpp:98-102) and, for a cloud source, the line extraction's
parameters.  `align_global(source, lines_target, constrain_angle, max_range)` takes the source as a list of `LineFeature` or as the
flat cloud (float32 [N,4], numpy or device tensor), which goes through a `LineExtractor` on the same handle first; an extraction that
yields no lines falls through as upstream does (the identity with the empty score).  `merge_lines` and `edge_extraction` are the
host-only pieces and need no GPU.
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass, field
from typing import List, Optional

import numpy as np

from . import _lib as L
from .line_extraction import LineFeature

__all__ = ["LineScanMatcher", "BestFitAlignment", "FitnessScore", "EdgeFeature", "merge_lines", "edge_extraction", "params_from_dict"]

_NAMES = {   # member name -> the nodelet's parameter name
    "g_avg_distance_weight": "delta_global_avg_distance_weight", "g_coverage_weight": "delta_global_coverage_weight",
    "g_transform_weight": "delta_global_transform_weight", "g_max_score_distance": "delta_global_max_score_distance",
    "g_max_score_translation": "delta_global_max_score_translation",
}
_EXTRA = ("max_distance", "max_angle", "angle_gate_float_chain", "nn_tie_highest_index")


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


def params_from_dict(params: Optional[dict] = None):
    """-> (LineAlignParams, the remaining entries): the constructor's defaults (line_based_scanmatcher.hpp:91-95), align_global's 2.0 and
    pi / 9, overridden by `params`; what is not an alignment parameter is left for the line extraction."""
    pr = dict(params or {})
    p = L.LineAlignParams()
    rc = L.load().dgs_line_align_params_init(C.byref(p))
    if rc:
        raise L.DgsError(rc, "dgs_line_align_params_init")
    for member, ros in _NAMES.items():
        for k in (ros, member):
            if k in pr:
                setattr(p, member, float(pr.pop(k)))
    for k in _EXTRA:
        if k in pr:
            v = pr.pop(k)
            setattr(p, k, float(v) if k.startswith("max_") else int(v))
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


def edge_extraction(lines: List[LineFeature]) -> List[EdgeFeature]:
    """edge_extraction (:459-471) on the host; no handle, no device."""
    lib = L.load()
    arr = _to_c(lines)
    n = C.c_int64(0)
    rc = lib.dgs_line_edges(C.cast(arr, C.c_void_p), len(lines), None, 0, C.byref(n))
    if rc and n.value == 0:
        _check(rc, "dgs_line_edges")
    out = (L.EdgeFeatureC * max(n.value, 1))()
    _check(lib.dgs_line_edges(C.cast(arr, C.c_void_p), len(lines), C.cast(out, C.c_void_p), n.value, C.byref(n)), "dgs_line_edges")
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

    # -- test hooks ----------------------------------------------------------------------------------------------------------
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
