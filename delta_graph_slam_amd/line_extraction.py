"""LineBasedScanmatcher::line_extraction on the device (upstream src/hdl_graph_slam/line_based_scanmatcher.cpp:299-457;
dgs_line_extraction in include/dgs_reg.h).

`LineExtractor(params)` takes the matcher's member names (line_based_scanmatcher.hpp:132-139) or the nodelet's `delta_*` parameter
names (apps/delta_graph_slam_nodelet.cpp:79-96) with the constructor's defaults.  `extract(flat_cloud)` takes the flat cloud as float32
[N,4], a numpy array or a device tensor -- what `Prefilter.filter_scan` returns as its 2-D output goes in unchanged -- and returns the
`LineFeature`s upstream hands to merge_lines.  Like the Prefilter, an extractor may share a Registration's handle: it works in buffers
of its own, so the registration's target, source and results, the prefilter's scratch and the map are untouched.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import List, Optional

import numpy as np

from . import _lib as L
from .registration import Registration, _cloud_ptr

__all__ = ["LineExtractor", "LineFeature", "params_from_dict"]

_NAMES = {   # member name -> the nodelet's parameter name
    "min_cluster_size": "delta_MinClusterSize", "max_cluster_size": "delta_MaxClusterSize", "cluster_tolerance": "delta_ClusterTolerance",
    "sac_distance_threshold": "delta_SACDistanceThreshold", "max_iterations": "delta_Max_iterations",
    "merror_threshold": "delta_Merror_threshold", "line_length_threshold": "delta_lenght_threshold", "sac_method_type": "delta_SACMethodType",
}
_EXTRA = ("sample_good_any_axis", "sqnorm_order", "cluster_inclusive", "max_rounds", "record_lists")


@dataclass
class LineFeature:
    pointA: np.ndarray
    pointB: np.ndarray
    mean_error: float
    std_sigma: float
    max_error: float
    min_error: float

    def lenght(self) -> float:   # upstream's spelling
        return float(np.float32(np.linalg.norm(self.pointA - self.pointB)))

    def middlePoint(self) -> np.ndarray:
        return self.pointA + (self.pointB - self.pointA) / 2.0


def params_from_dict(params: Optional[dict] = None) -> L.LineExtractionParams:
    """The constructor's defaults (line_based_scanmatcher.hpp:80-89) overridden by `params`.  An unknown delta_SACMethodType string keeps
    SAC_RANSAC, as the nodelet's loop does (:87-96); a known one other than SAC_RANSAC is refused by dgs_line_extraction."""
    pr = dict(params or {})
    p = L.LineExtractionParams()
    rc = L.load().dgs_line_extraction_params_init(C.byref(p))
    if rc:
        raise L.DgsError(rc, "dgs_line_extraction_params_init")
    known = set(_NAMES) | set(_NAMES.values()) | set(_EXTRA)
    for k in pr:
        if k not in known:
            raise KeyError(f"unknown line extraction parameter {k!r}")
    for member, ros in _NAMES.items():
        v = pr.get(member, pr.get(ros))
        if v is None:
            continue
        if member == "sac_method_type":
            v = (L.SAC_METHODS.index(v) if v in L.SAC_METHODS else 0) if isinstance(v, str) else int(v)
        kind = dict(p._fields_)[member]
        setattr(p, member, float(v) if kind is C.c_float else int(v))
    for k in _EXTRA:
        if k in pr:
            v = pr[k]
            setattr(p, k, L.PF_NORM_ORDER[v] if k == "sqnorm_order" and isinstance(v, str) else int(v))
    return p


class LineExtractor:
    def __init__(self, params: Optional[dict] = None, registration: Optional[Registration] = None, device: Optional[int] = None):
        self.params = params_from_dict(params)
        if registration is None:
            registration = Registration("NDT_OMP", device=device)   # any handle: only its stream and the extractor's own buffers are used
        self.registration = registration
        self._lib = registration._lib
        self.status = "DONE"                 # L.LE_STATUS of the last extraction

    @property
    def _h(self):
        return self.registration._h

    def extract(self, flat_cloud, rng_raw=None) -> List[LineFeature]:
        """rng_raw: optional uint32 values that stand in for boost::mt19937(12345)() >> 1 (restarted every round)."""
        ptr, n, dev, keep = _cloud_ptr(flat_cloud)
        cap = n // max(int(self.params.min_cluster_size), 1) + 1
        out = (L.LineFeatureC * cap)()
        m, st = C.c_int64(0), C.c_int32(0)
        raw = None if rng_raw is None else np.ascontiguousarray(rng_raw, dtype=np.uint32)
        self.registration._check(self._lib.dgs_line_extraction(
            self._h, C.byref(self.params), ptr, n, dev, None if raw is None else raw.ctypes.data_as(C.c_void_p), 0 if raw is None else raw.size,
            C.cast(out, C.c_void_p), cap, C.byref(m), C.byref(st)))
        self.status = L.LE_STATUS[st.value]
        return [LineFeature(np.array(f.point_a[:], np.float64), np.array(f.point_b[:], np.float64), f.mean_error, f.std_sigma, f.max_error,
                            f.min_error) for f in out[:m.value]]

    # -- test hooks ----------------------------------------------------------------------------------------------------------
    def rounds(self):
        """One dict per round of the last extraction: n_before, draws, iterations, sample, inliers, cluster, emitted."""
        n = C.c_int64(0)
        self.registration._check(self._lib.dgs_line_extraction_get_rounds(self._h, None, 0, C.byref(n), -1, None, None, None))
        rec = (L.LineExtractionRound * max(n.value, 1))()
        self.registration._check(self._lib.dgs_line_extraction_get_rounds(self._h, C.cast(rec, C.c_void_p), n.value, C.byref(n), -1, None, None, None))
        return [dict(n_before=r.n_before, draws=r.draws, iterations=r.iterations, sample=(r.sample0, r.sample1), inliers=r.inliers,
                     cluster=r.cluster, emitted=r.emitted) for r in rec[:n.value]]

    def round_lists(self, r: int, inliers: int, cluster: int):
        """With record_lists: (inlier positions, cluster positions) of round r, ascending."""
        n = C.c_int64(0)
        il, cl = np.zeros(max(inliers, 1), np.int32), np.zeros(max(cluster, 1), np.int32)
        self.registration._check(self._lib.dgs_line_extraction_get_rounds(self._h, None, 0, C.byref(n), r, il.ctypes.data_as(C.c_void_p),
                                                                          cl.ctypes.data_as(C.c_void_p), None))
        return il[:inliers], cl[:cluster]

    def counts(self):
        """-> dict(launches, host_waits, rounds_launched, sort_calls) of the last extraction."""
        n = C.c_int64(0)
        c = (C.c_int64 * 4)()
        self.registration._check(self._lib.dgs_line_extraction_get_rounds(self._h, None, 0, C.byref(n), -1, None, None, C.cast(c, C.c_void_p)))
        return dict(launches=c[0], host_waits=c[1], rounds_launched=c[2], sort_calls=c[3])
