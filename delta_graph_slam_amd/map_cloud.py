"""MapCloudGenerator::generate on the device: src/hdl_graph_slam/map_cloud_generator.cpp:13-50 over
dgs_map_cloud_generate (include/dgs_reg.h).

`MapCloudGenerator().generate(keyframes, resolution)` transforms every keyframe cloud by its pose, concatenates them and returns the
centres of the occupied voxels of a pcl::octree::OctreePointCloud of `resolution`, in the octree's depth-first order; with
resolution <= 0 it returns the concatenation.  A keyframe is an object with `.cloud` and `.pose` (a 4x4 double matrix, what
KeyFrameSnapshot holds) or a `(cloud, pose)` pair; a cloud is a float32 [N,4] numpy array, a device tensor or a DeviceCloud.  Device
input gives a device tensor back, host input numpy.  With a LoopDetector the clouds of its KeyFrames are the ones it keeps resident
in HBM: per map only the poses travel.  An empty keyframe list returns None, as upstream (:14-17).  Like the Prefilter, the
generator may share a Registration's handle: it works in buffers of its own.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np

from . import _lib as L
from .registration import DeviceCloud, Registration, _cloud_ptr, torch
from .transforms import transform2Dto3D

__all__ = ["MapCloudGenerator", "snapshot_pose", "params_from_dict"]


def snapshot_pose(estimate) -> np.ndarray:
    """KeyFrameSnapshot(key) (keyframe.cpp:34): transform2Dto3D(key->estimate().matrix().cast<float>()).cast<double>()."""
    return transform2Dto3D(np.asarray(estimate, np.float64).astype(np.float32)).astype(np.float64)


def params_from_dict(params: Optional[dict] = None) -> L.MapCloudParams:
    """dgs_map_cloud_params: the defaults with the given fields replaced (dedup_method by name or number)."""
    p = L.MapCloudParams()
    rc = L.load().dgs_map_cloud_params_init(C.byref(p))
    if rc:
        raise L.DgsError(rc, "dgs_map_cloud_params_init")
    for k, v in dict(params or {}).items():
        if k == "struct_size" or not hasattr(p, k):
            raise TypeError(f"unknown map cloud parameter {k!r}")
        setattr(p, k, L.MAP_DEDUP[v] if k == "dedup_method" and isinstance(v, str) else int(v))
    return p


def _is_device(x) -> bool:
    return torch is not None and isinstance(x, torch.Tensor) and x.is_cuda


class MapCloudGenerator:
    def __init__(self, registration: Optional[Registration] = None, device: Optional[int] = None, params: Optional[dict] = None):
        self.params = params_from_dict(params)
        if registration is None:
            registration = Registration("NDT_OMP", device=device)   # any handle: only its stream and the map's own buffers are used
        self.registration = registration
        self._lib = registration._lib

    @property
    def _h(self):
        return self.registration._h

    def _check(self, rc: int):
        self.registration._check(rc)

    @staticmethod
    def _split(keyframes, loop_detector):
        clouds, poses = [], []
        for kf in keyframes:
            if isinstance(kf, (tuple, list)):
                cloud, pose = kf
            else:
                pose = kf.pose if hasattr(kf, "pose") else snapshot_pose(kf.estimate)
                cloud = loop_detector.resident(kf) if loop_detector is not None and hasattr(kf, "estimate") else kf.cloud
            pose = np.asarray(pose, np.float64)
            if pose.shape != (4, 4):
                raise ValueError("a keyframe pose must be a 4x4 matrix")
            clouds.append(cloud)
            poses.append(pose.T.reshape(16))    # column-major, Eigen::Isometry3d::matrix()
        return clouds, np.ascontiguousarray(np.array(poses, np.float64).reshape(-1, 16))

    def generate(self, keyframes, resolution: float, loop_detector=None):
        """-> float32 [M,4] map cloud (device tensor when any input cloud lives on the device), or None for an empty list."""
        keyframes = list(keyframes)
        if len(keyframes) == 0:
            return None    # "warning: keyframes empty!!" (:14-17)
        clouds, poses = self._split(keyframes, loop_detector)
        n = len(clouds)
        m = C.c_int64(0)
        pp = poses.ctypes.data_as(C.c_void_p)
        if all(isinstance(c, DeviceCloud) for c in clouds):
            arr = (C.c_void_p * n)(*[c._c.value for c in clouds])
            self._check(self._lib.dgs_map_cloud_generate_clouds(self._h, C.byref(self.params), n, arr, pp, float(resolution), C.byref(m)))
            device_out = True
        else:
            if any(isinstance(c, DeviceCloud) for c in clouds):
                raise TypeError("resident clouds and arrays cannot be mixed in one map")
            dev_flags = [_is_device(c) for c in clouds]
            if any(dev_flags) and not all(dev_flags):
                raise TypeError("host arrays and device tensors cannot be mixed in one map")
            ptrs, sizes, keep = [], [], []
            for c in clouds:
                ptr, k, _, ka = _cloud_ptr(c)
                ptrs.append(ptr.value if k else None)
                sizes.append(k)
                keep.append(ka)
            arr = (C.c_void_p * n)(*ptrs)
            sz = (C.c_int64 * n)(*sizes)
            device_out = bool(dev_flags[0])
            self._check(self._lib.dgs_map_cloud_generate(self._h, C.byref(self.params), n, arr, sz, 1 if device_out else 0, pp, float(resolution),
                                                         C.byref(m)))
        return self.last(device=device_out)

    def last(self, device: bool = False):
        """The last map again (it stays on the handle until the next map call)."""
        m = C.c_int64(0)
        self._check(self._lib.dgs_map_cloud_get(self._h, None, 0, 0, C.byref(m)))
        if device:
            dev = torch.device("cuda", self.registration.params.device if self.registration.params is not None and self.registration.params.device >= 0
                               else torch.cuda.current_device())
            out = torch.empty((max(m.value, 1), 4), dtype=torch.float32, device=dev)
            self._check(self._lib.dgs_map_cloud_get(self._h, C.c_void_p(out.data_ptr()), m.value, 1, C.byref(m)))
            return out[:m.value]
        out = np.empty((max(m.value, 1), 4), np.float32)
        self._check(self._lib.dgs_map_cloud_get(self._h, out.ctypes.data_as(C.c_void_p), m.value, 0, C.byref(m)))
        return out[:m.value].copy()

    def grid(self):
        """Test hook: the octree of the last map with resolution > 0 -> dict(min, max, depth, growths)."""
        mn, mx = np.zeros(3, np.float64), np.zeros(3, np.float64)
        d, g = C.c_int32(0), C.c_int32(0)
        self._check(self._lib.dgs_map_cloud_get_grid(self._h, mn.ctypes.data_as(C.c_void_p), mx.ctypes.data_as(C.c_void_p), C.byref(d), C.byref(g)))
        return dict(min=mn, max=mx, depth=d.value, growths=g.value)
