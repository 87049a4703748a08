"""interpolate, BuildingTools::buildPointCloud and Building::getCloud on the device (upstream src/hdl_graph_slam/ros_utils.cpp:146-165,
building_tools.cpp:166-196, building.cpp:7-22; dgs_building_cloud_generate in include/dgs_reg.h).

`BuildingClouds(registration=..., device=..., params=...)` samples line segments into clouds of one point per 2 cm:

* `interpolate(a, b)`: one segment, upstream's free function.
* `building_cloud(lines)`: a building's cloud from its outline, `*cloud += *interpolate(...)` over its lines in order.
* `get_cloud(lines, trans3D)`: the same through pcl::transformPointCloud(trans3D), what Building::getCloud returns.
* `clouds(items, transforms=None)`: many items in one call (the buildings of a tick, or a frame's aligned / not-aligned lists) ->
  (points float32 [N, 4], offsets int64 [len(items) + 1]).  `transforms`: None, one 4 x 4 for all items, or one entry per item (a
  4 x 4 or None).
* `building_transform(pose, estimate)`: the matrix getCloud builds (building.cpp:11-15), scalar host arithmetic.

Lines are a list of `LineFeature` (pointA / pointB) or a float64 array [L, 2, 3].  Results are numpy arrays; `device=True` returns the
points as a torch tensor on the device instead.  Like the other stages, it may share a Registration's handle: it works in buffers of
its own."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np

from . import _lib as L
from .building_overlap import _lines_array
from .transforms import transform2Dto3D

__all__ = ["BuildingClouds", "building_transform", "params_from_dict"]


def params_from_dict(params: Optional[dict] = None) -> L.BuildingCloudParams:
    """dgs_building_cloud_params: the defaults with the given fields replaced (sqnorm_order by name or number)."""
    p = L.BuildingCloudParams()
    rc = L.load().dgs_building_cloud_params_init(C.byref(p))
    if rc:
        raise L.DgsError(rc, "dgs_building_cloud_params_init")
    for k, v in dict(params or {}).items():
        if k == "struct_size" or not hasattr(p, k):
            raise TypeError(f"unknown building cloud parameter {k!r}")
        if k == "sample_step":
            p.sample_step = float(v)
        else:
            setattr(p, k, L.PF_NORM_ORDER[v] if k == "sqnorm_order" and isinstance(v, str) else int(v))
    return p


def building_transform(pose, estimate) -> np.ndarray:
    """Building::getCloud's matrix (building.cpp:11-15).  pose: the building's Eigen::Isometry2d, estimate: node->estimate().toIsometry(),
    both 3 x 3 doubles -> float32 4 x 4.  [UPSTREAM-RECALL] Eigen 3.3: an Isometry's inverse() is (R^T, -(R^T t)), and the product of
    two of them is (Ra Rb, Ra tb + ta)."""
    P, E = np.asarray(pose, np.float64).tolist(), np.asarray(estimate, np.float64).tolist()
    r00, r01, r10, r11 = P[0][0], P[1][0], P[0][1], P[1][1]          # the inverse's rotation: the transpose
    px, py = P[0][2], P[1][2]
    ix, iy = -(r00 * px + r01 * py), -(r10 * px + r11 * py)
    t00, t01 = r00 * E[0][0] + r01 * E[1][0], r00 * E[0][1] + r01 * E[1][1]
    t10, t11 = r10 * E[0][0] + r11 * E[1][0], r10 * E[0][1] + r11 * E[1][1]
    tx, ty = (r00 * E[0][2] + r01 * E[1][2]) + ix, (r10 * E[0][2] + r11 * E[1][2]) + iy
    tx += px - (t00 * px + t01 * py)
    ty += py - (t10 * px + t11 * py)
    trans = np.array([[t00, t01, tx], [t10, t11, ty], [0.0, 0.0, 1.0]], np.float64)
    return transform2Dto3D(trans.astype(np.float32))


class BuildingClouds:
    def __init__(self, registration=None, device: Optional[int] = None, params: Optional[dict] = None):
        from .registration import Registration
        self.params = params_from_dict(params)
        if registration is None:
            registration = Registration("NDT_OMP", device=device)   # any handle: only its stream and the stage's own buffers are used
        self.registration = registration
        self._lib = registration._lib

    @property
    def _h(self):
        return self.registration._h

    building_transform = staticmethod(building_transform)

    # ---- the batched call
    def clouds(self, items, transforms=None, device: bool = False):
        arrays = [_lines_array(it) for it in items]
        n = len(arrays)
        off = np.zeros(n + 1, np.int64)
        if n:
            off[1:] = np.cumsum([a.shape[0] for a in arrays])
        flat = np.concatenate(arrays) if n else np.zeros((0, 2, 3))
        feats = np.zeros((max(int(off[n]), 1), 10), np.float64)          # dgs_line_feature: ten doubles
        feats[:flat.shape[0], :6] = flat.reshape(-1, 6)
        mats, index = None, None
        if transforms is not None:
            if isinstance(transforms, np.ndarray) and transforms.shape == (4, 4):
                mats = [transforms]
            else:
                transforms = list(transforms)
                if len(transforms) != n:
                    raise ValueError("one transform per item, or one 4 x 4 for all")
                index = np.full(max(n, 1), -1, np.int32)
                mats = []
                for i, t in enumerate(transforms):
                    if t is not None:
                        index[i] = len(mats)
                        mats.append(t)
            # column-major, Eigen's data()
            mats = np.ascontiguousarray(np.array([np.asarray(m, np.float32).T.reshape(16) for m in mats], np.float32).reshape(-1, 16))
            if mats.shape[0] == 0:
                mats, index = None, None
        total = C.c_int64(0)
        self.registration._check(self._lib.dgs_building_cloud_generate(
            self._h, C.byref(self.params), feats.ctypes.data, off.ctypes.data, n, None if mats is None else mats.ctypes.data,
            None if index is None else index.ctypes.data, C.byref(total)))
        return self.last(device=device)

    def last(self, device: bool = False):
        """The last result again (it stays on the handle until the next call) -> (points, offsets)."""
        m = C.c_int64(0)
        self.registration._check(self._lib.dgs_building_cloud_get(self._h, None, 0, 0, None, C.byref(m), None))
        offsets = np.zeros(int(self.counts()["items"]) + 1, np.int64)
        if device:
            from .registration import torch
            prm = self.registration.params
            dev = torch.device("cuda", prm.device if prm is not None and prm.device >= 0 else torch.cuda.current_device())
            out = torch.empty((max(m.value, 1), 4), dtype=torch.float32, device=dev)
            self.registration._check(self._lib.dgs_building_cloud_get(self._h, C.c_void_p(out.data_ptr()), m.value, 1, offsets.ctypes.data, C.byref(m), None))
            return out[:m.value], offsets
        out = np.empty((max(m.value, 1), 4), np.float32)
        self.registration._check(self._lib.dgs_building_cloud_get(self._h, out.ctypes.data, m.value, 0, offsets.ctypes.data, C.byref(m), None))
        return out[:m.value].copy(), offsets

    # ---- upstream's three shapes
    def interpolate(self, a, b, device: bool = False):
        line = np.array([[np.asarray(a, np.float64).reshape(3), np.asarray(b, np.float64).reshape(3)]], np.float64)
        return self.clouds([line], device=device)[0]

    def building_cloud(self, lines, device: bool = False):
        return self.clouds([lines], device=device)[0]

    def get_cloud(self, lines, trans3D, device: bool = False):
        return self.clouds([lines], [np.asarray(trans3D, np.float32)], device=device)[0]

    def counts(self):
        """Test hook -> dict(launches, host_waits, lines, points, table_entries, table_added, tile, items) of the last call."""
        c = (C.c_int64 * 8)()
        self.registration._check(self._lib.dgs_building_cloud_get_counts(self._h, C.cast(c, C.c_void_p)))
        return dict(launches=c[0], host_waits=c[1], lines=c[2], points=c[3], table_entries=c[4], table_added=c[5], tile=c[6], items=c[7])
