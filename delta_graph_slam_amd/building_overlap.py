"""getOverlappedBuildings on the device (upstream apps/delta_graph_slam_nodelet.cpp:767-787 with are_buildings_overlapped,
include/hdl_graph_slam/check_overlapping.hpp; dgs_building_overlap_pairs in include/dgs_reg.h).

`BuildingOverlap(registration=..., device=...).overlapped_pairs(buildings_lines, centers)` takes every building's lines (a list of
`LineFeature`, or a float64 array [L, 2, 3]) and its centre, and returns every pair i < j whose shrunken polygons intersect, in upstream's
order: i ascending, then j ascending.  The predicate is upstream's as it is: a building wholly inside another is not overlapped, and
parallel or collinear walls never intersect.  The batched resolution of the pairs is `LineScanMatcher.align_overlapped_batch`.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np

from . import _lib as L

__all__ = ["BuildingOverlap"]


def _lines_array(lines):
    if isinstance(lines, np.ndarray):
        return np.ascontiguousarray(lines, np.float64).reshape(-1, 2, 3)
    return np.array([[np.asarray(l.pointA, np.float64), np.asarray(l.pointB, np.float64)] for l in lines], np.float64).reshape(-1, 2, 3)


class BuildingOverlap:
    def __init__(self, registration=None, device: Optional[int] = None):
        from .registration import Registration
        if registration is None:
            registration = Registration("NDT_OMP", device=device)   # any handle: only its stream and the search's own buffers are used
        self.registration = registration
        self._lib = registration._lib

    @property
    def _h(self):
        return self.registration._h

    def overlapped_pairs(self, buildings_lines, centers, capacity: Optional[int] = None) -> np.ndarray:
        """-> int32 [P, 2].  `capacity` None: room for 4 pairs per building, and a second call when there are more.  With a capacity
        given, more pairs than that raise DgsError (DGS_ERR_CAPACITY); `last_count` holds the full count and `last_pairs` the first
        `capacity` pairs."""
        arrays = [_lines_array(b) for b in buildings_lines]
        B = len(arrays)
        centers = np.ascontiguousarray(np.asarray(centers, np.float64).reshape(B, 3))
        off = np.zeros(B + 1, np.int64)
        if B:
            off[1:] = np.cumsum([a.shape[0] for a in arrays])
        feats = (L.LineFeatureC * max(int(off[B]), 1))()
        flat = np.concatenate(arrays) if B else np.zeros((0, 2, 3))
        for f, l in zip(feats, flat):
            f.point_a[:] = l[0].tolist()
            f.point_b[:] = l[1].tolist()
        n = C.c_int64(0)

        def call(cap):
            out = np.zeros((max(cap, 1), 2), np.int32)
            rc = self._lib.dgs_building_overlap_pairs(self._h, C.cast(feats, C.c_void_p), off.ctypes.data, centers.ctypes.data if B else None, B,
                                                      out.ctypes.data if cap else None, cap, C.byref(n))
            return rc, out

        cap = max(4 * B, 64) if capacity is None else int(capacity)
        rc, out = call(cap)
        if rc == L.DGS_ERR_CAPACITY and capacity is None:
            rc, out = call(n.value)
        self.last_count = n.value
        self.last_pairs = out[:min(n.value, out.shape[0] if cap else 0)].copy()
        self.registration._check(rc)
        return self.last_pairs

    def counts(self):
        """-> dict(launches, host_waits, buildings, pairs) of the last overlapped_pairs device call."""
        c = (C.c_int64 * 8)()
        self.registration._check(self._lib.dgs_building_overlap_get_counts(self._h, C.cast(c, C.c_void_p)))
        return dict(launches=c[0], host_waits=c[1], buildings=c[2], pairs=c[3])
