"""PrefilteringNodelet's cloud_callback on the device: /root/reference/apps/prefiltering_nodelet.cpp:111-164, from the raw scan
(dgs_prefilter_scan) or from the distance filter (dgs_prefilter) to flatten (include/dgs_reg.h).

`Prefilter(params)` takes the nodelet's private parameter names with initialize_params' defaults (:55-109).
`filter_scan(cloud, angular_velocity, base_link_transform)` takes the scan as the driver delivers it: deskewing (:293-354) and the
base_link transform (:122-150) run fused into the distance filter's pass, and it returns (/filtered_points, /flat_filtered_points,
lidar_position).  `ImuQueue` is the nodelet's IMU queue (:107-109, :318-328).  `cloud_callback(cloud, lidar_position)` is the chain
alone, for a caller that has done the two steps itself.  Clouds are float32 [N,4]: numpy in gives numpy out, a device tensor in gives device
tensors out.  Like InformationMatrixCalculator, a Prefilter may share a Registration's handle: it uses buffers and an NN index of
its own, so the registration's target, source and results are untouched.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np

from . import _lib as L
from .registration import Registration, _cloud_ptr, torch

__all__ = ["Prefilter", "ImuQueue", "params_from_dict"]


def params_from_dict(params: Optional[dict] = None) -> L.PrefilterParams:
    """initialize_params (:55-109): the nodelet's parameter names and defaults.  An unknown downsample_method is NONE (:71-76), an
    unknown outlier_removal_method is NONE (:97-99); use_distance_filter is read (:100) and ignored, as upstream (:153)."""
    pr = dict(params or {})
    lib = L.load()
    p = L.PrefilterParams()
    rc = lib.dgs_prefilter_params_init(C.byref(p))
    if rc:
        raise L.DgsError(rc, "dgs_prefilter_params_init")
    p.downsample_method = L.PF_DOWNSAMPLE.get(str(pr.get("downsample_method", "VOXELGRID")), L.PF_DOWNSAMPLE["NONE"])
    p.downsample_resolution = float(pr.get("downsample_resolution", p.downsample_resolution))
    p.outlier_removal_method = L.PF_OUTLIER.get(str(pr.get("outlier_removal_method", "STATISTICAL")), L.PF_OUTLIER["NONE"])
    p.statistical_mean_k = int(pr.get("statistical_mean_k", p.statistical_mean_k))
    p.statistical_stddev = float(pr.get("statistical_stddev", p.statistical_stddev))
    p.radius_radius = float(pr.get("radius_radius", p.radius_radius))
    p.radius_min_neighbors = int(pr.get("radius_min_neighbors", p.radius_min_neighbors))
    p.use_distance_filter = 1 if pr.get("use_distance_filter", True) else 0
    p.distance_near_thresh = float(pr.get("distance_near_thresh", p.distance_near_thresh))
    p.distance_far_thresh = float(pr.get("distance_far_thresh", p.distance_far_thresh))
    p.radius_inclusive = 1 if pr.get("radius_inclusive", True) else 0
    p.statistical_sqrt_float = 1 if pr.get("statistical_sqrt_float", True) else 0
    return p


class ImuQueue:
    """The nodelet's imu_queue: imu_callback (:107-109) is push, the search in deskewing (:318-328) is select."""

    def __init__(self):
        self.queue = []                      # (stamp, angular_velocity) in arrival order

    def __len__(self):
        return len(self.queue)

    def push(self, stamp, angular_velocity):
        self.queue.append((stamp, tuple(float(v) for v in angular_velocity)))

    def select(self, scan_stamp):
        """-> the angular velocity deskewing uses for a scan stamped scan_stamp, or None when the queue is empty (:295-297).
        The first message stamped after the scan (strictly) is chosen, else the last one; everything before the position where
        the search stopped is erased (:328).  So when no message is later than the scan the queue is emptied, and the next scan
        goes through without deskewing unless a message arrives first: upstream's behaviour, kept."""
        if not self.queue:
            return None
        loc = 0
        chosen = self.queue[0]
        while loc < len(self.queue):
            chosen = self.queue[loc]
            if chosen[0] > scan_stamp:
                break
            loc += 1
        del self.queue[:loc]
        return chosen[1]


class Prefilter:
    def __init__(self, params: Optional[dict] = None, registration: Optional[Registration] = None, device: Optional[int] = None):
        self.params = params_from_dict(params)
        self.deskew_norm_order = 0           # dgs_prefilter_scan_params.deskew_norm_order (L.PF_NORM_ORDER)
        self.transform_sets_w = 1            # dgs_prefilter_scan_params.transform_sets_w
        if registration is None:
            registration = Registration("NDT_OMP", device=device)   # any handle: only its stream and the prefilter's own buffers are used
        self.registration = registration
        self._lib = registration._lib

    @property
    def _h(self):
        return self.registration._h

    def _check(self, rc: int):
        self.registration._check(rc)

    @staticmethod
    def _lidar(lidar_position):
        return (C.c_double * 3)(*[float(v) for v in lidar_position])

    def _new(self, like, n: int):
        if _is_device(like):
            return torch.empty((max(n, 1), 4), dtype=torch.float32, device=like.device)
        return np.empty((max(n, 1), 4), dtype=np.float32)

    @staticmethod
    def _ptr(out):
        return C.c_void_p(out.data_ptr()) if _is_device(out) else out.ctypes.data_as(C.c_void_p)

    @staticmethod
    def _take(out, m: int):
        return out[:m] if _is_device(out) else out[:m].copy()

    def cloud_callback(self, cloud, lidar_position=(0.0, 0.0, 0.0)):
        """-> (filtered3d, filtered2d): what cloud_callback publishes on /filtered_points and /flat_filtered_points."""
        ptr, n, dev, keep = _cloud_ptr(cloud)
        o3, o2 = self._new(cloud, n), self._new(cloud, n)
        m3, m2 = C.c_int64(0), C.c_int64(0)
        self._check(self._lib.dgs_prefilter(self._h, C.byref(self.params), ptr, n, dev, self._lidar(lidar_position), self._ptr(o3), n,
                                            self._ptr(o2), n, dev, C.byref(m3), C.byref(m2)))
        return self._take(o3, m3.value), self._take(o2, m2.value)

    def _scan_params(self, angular_velocity, base_link_transform, scan_period) -> L.PrefilterScanParams:
        sp = L.PrefilterScanParams()
        self._check(self._lib.dgs_prefilter_scan_params_init(C.byref(sp)))
        sp.scan_period = float(scan_period)
        sp.deskew_norm_order = int(self.deskew_norm_order)
        sp.transform_sets_w = 1 if self.transform_sets_w else 0
        if angular_velocity is not None:     # None is the empty IMU queue (:295-297), not a zero angular velocity
            sp.has_angular_velocity = 1
            sp.angular_velocity[:] = [float(v) for v in angular_velocity]
        if base_link_transform is not None:
            m = np.array(base_link_transform, np.float64).reshape(4, 4)
            m[0, 3] = 0.0                    # lidar scans should be centered in base_link (:141-142)
            m[1, 3] = 0.0
            sp.has_transform = 1
            sp.transform[:] = m.reshape(16).tolist()
        return sp

    def filter_scan(self, cloud, angular_velocity=None, base_link_transform=None, scan_period=0.1):
        """cloud_callback from the raw scan (:120-160) -> (filtered3d, filtered2d, lidar_position).  angular_velocity: the IMU
        message's, as ImuQueue.select returns it, or None (no deskewing); base_link_transform: the 4 x 4 matrix of the tf lookup
        (:131-138) or None; lidar_position: float64 [3], (0, 0, m[2,3]) with a transform, zero without."""
        ptr, n, dev, keep = _cloud_ptr(cloud)
        sp = self._scan_params(angular_velocity, base_link_transform, scan_period)
        o3, o2 = self._new(cloud, n), self._new(cloud, n)
        m3, m2 = C.c_int64(0), C.c_int64(0)
        lidar = np.zeros(3, np.float64)
        self._check(self._lib.dgs_prefilter_scan(self._h, C.byref(self.params), C.byref(sp), ptr, n, dev, self._ptr(o3), n, self._ptr(o2), n, dev,
                                                 C.byref(m3), C.byref(m2), lidar.ctypes.data_as(C.c_void_p)))
        return self._take(o3, m3.value), self._take(o2, m2.value), lidar

    def filter_scan_batch(self, clouds, angular_velocities=None, base_link_transforms=None, scan_period=0.1):
        """filter_scan over many scans in one device call (dgs_prefilter_scan_batch): the frames of several streams.
        -> ([(filtered3d, filtered2d, lidar_position)] per scan, statuses int32 [n]).  Scan i receives the bits filter_scan gives it
        alone; statuses[i] is what that single call would have returned (0 = ok; otherwise the scan's outputs are empty and the other
        scans are unaffected).  angular_velocities / base_link_transforms: one entry per scan (None entries allowed), or None for all.
        clouds: all numpy (numpy out) or all device tensors (device tensors out, views of two slabs)."""
        n = len(clouds)
        avs = list(angular_velocities) if angular_velocities is not None else [None] * n
        tfs = list(base_link_transforms) if base_link_transforms is not None else [None] * n
        if len(avs) != n or len(tfs) != n:
            raise ValueError("angular_velocities and base_link_transforms need one entry per scan")
        statuses = np.zeros(n, np.int32)
        if n == 0:
            self._check(self._lib.dgs_prefilter_scan_batch(self._h, C.byref(self.params), 0, None, None, None, 0, None, None, None, None, 0, None, None, None, None))
            return [], statuses
        dev = _is_device(clouds[0])
        if any(_is_device(c) != dev for c in clouds):
            raise ValueError("filter_scan_batch takes all numpy arrays or all device tensors")
        ptrs = [_cloud_ptr(c, sync=False) for c in clouds]
        if dev:
            torch.cuda.current_stream(clouds[0].device).synchronize()   # once for the whole batch
        sizes = np.array([q[1] for q in ptrs], np.int64)
        offs = np.concatenate([[0], np.cumsum(np.maximum(sizes, 1))]).astype(np.int64)
        slab3, slab2 = self._new(clouds[0], int(offs[-1])), self._new(clouds[0], int(offs[-1]))
        o3 = [slab3[offs[i]:offs[i + 1]] for i in range(n)]
        o2 = [slab2[offs[i]:offs[i + 1]] for i in range(n)]
        sps = (L.PrefilterScanParams * n)(*[self._scan_params(avs[i], tfs[i], scan_period) for i in range(n)])
        in_p = (C.c_void_p * n)(*[q[0] for q in ptrs])
        o3_p = (C.c_void_p * n)(*[self._ptr(o) for o in o3])
        o2_p = (C.c_void_p * n)(*[self._ptr(o) for o in o2])
        m3, m2 = np.zeros(n, np.int64), np.zeros(n, np.int64)
        lidar = np.zeros((n, 3), np.float64)
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        self._check(self._lib.dgs_prefilter_scan_batch(self._h, C.byref(self.params), n, sps, in_p, vp(sizes), 1 if dev else 0, o3_p, vp(sizes), o2_p, vp(sizes),
                                                       1 if dev else 0, vp(m3), vp(m2), vp(lidar), vp(statuses)))
        return [(self._take(o3[i], int(m3[i])), self._take(o2[i], int(m2[i])), lidar[i].copy()) for i in range(n)], statuses

    def batch_counts(self) -> np.ndarray:
        """counts8 of the last filter_scan_batch: [0] kernel launches, [1] host waits, [2] scans listed, [3] scans that reached the
        normal filter, [4] scans served by a per-scan fallback, [5] chunks, [6] indices built."""
        c = np.zeros(8, np.int64)
        self._check(self._lib.dgs_prefilter_batch_get_counts(self._h, c.ctypes.data_as(C.c_void_p)))
        return c

    def batch_statistics(self) -> np.ndarray:
        """float64 [n, 4]: {mean, stddev, threshold, points} of every scan's statistical pass in the last filter_scan_batch; zeros
        where that pass did not run."""
        n = C.c_int64(0)
        self._check(self._lib.dgs_prefilter_batch_get_statistics(self._h, None, 0, C.byref(n)))
        s = np.zeros((n.value, 4), np.float64)
        self._check(self._lib.dgs_prefilter_batch_get_statistics(self._h, s.ctypes.data_as(C.c_void_p), n.value, C.byref(n)))
        return s

    def deskew(self, cloud, angular_velocity=None, base_link_transform=None, scan_period=0.1):
        """Deskewing and the base_link transform alone (dgs_prefilter_deskew): every point at its own place, non-finite ones included."""
        ptr, n, dev, keep = _cloud_ptr(cloud)
        sp = self._scan_params(angular_velocity, base_link_transform, scan_period)
        out = self._new(cloud, n)
        m = C.c_int64(0)
        self._check(self._lib.dgs_prefilter_deskew(self._h, C.byref(sp), ptr, n, dev, self._ptr(out), n, dev, C.byref(m)))
        return self._take(out, m.value)

    def _stage(self, fn, cloud, *args):
        ptr, n, dev, keep = _cloud_ptr(cloud)
        out = self._new(cloud, n)
        m = C.c_int64(0)
        self._check(fn(self._h, ptr, n, dev, *args, self._ptr(out), n, dev, C.byref(m)))
        return self._take(out, m.value)

    # -- single stages ------------------------------------------------------------------------------------------------------
    def distance_filter(self, cloud):
        p = self.params
        return self._stage(self._lib.dgs_prefilter_distance, cloud, p.distance_near_thresh, p.distance_far_thresh)

    def downsample(self, cloud):
        p = self.params
        if p.downsample_method == L.PF_DOWNSAMPLE["NONE"]:
            return cloud
        return self.registration.voxel_grid_filter(cloud, p.downsample_resolution, approximate=p.downsample_method == L.PF_DOWNSAMPLE["APPROX_VOXELGRID"])

    def radius_outlier_removal(self, cloud):
        p = self.params
        return self._stage(self._lib.dgs_prefilter_radius, cloud, p.radius_radius, p.radius_min_neighbors, p.radius_inclusive)

    def statistical_outlier_removal(self, cloud):
        p = self.params
        return self._stage(self._lib.dgs_prefilter_statistical, cloud, p.statistical_mean_k, p.statistical_stddev, p.statistical_sqrt_float)

    def outlier_removal(self, cloud):
        m = self.params.outlier_removal_method
        if m == L.PF_OUTLIER["STATISTICAL"]:
            return self.statistical_outlier_removal(cloud)
        if m == L.PF_OUTLIER["RADIUS"]:
            return self.radius_outlier_removal(cloud)
        return cloud

    def height_filtering(self, cloud, lidar_position=(0.0, 0.0, 0.0)):
        """:192-212, a plain predicate: kept iff z > lidar_position.z in double (on the host side of the caller's array)."""
        if _is_device(cloud):
            return cloud[cloud[:, 2].double() > float(lidar_position[2])]
        a = np.asarray(cloud, np.float32)
        return a[a[:, 2].astype(np.float64) > float(lidar_position[2])].copy()

    def normal_filtering(self, cloud, lidar_position=(0.0, 0.0, 0.0)):
        return self._stage(self._lib.dgs_prefilter_normal, cloud, self._lidar(lidar_position))

    @staticmethod
    def flatten(cloud):
        out = cloud.clone() if _is_device(cloud) else np.array(cloud, np.float32, copy=True)
        out[:, 2] = 0.0
        return out

    # -- test hooks ----------------------------------------------------------------------------------------------------------
    def statistics(self):
        """Last statistical pass: (per-point mean distances float32 [n], {mean, stddev, threshold, n})."""
        n = C.c_int64(0)
        self._check(self._lib.dgs_prefilter_get_statistics(self._h, None, 0, None, C.byref(n)))
        d = np.empty(n.value, np.float32)
        s = np.zeros(4, np.float64)
        self._check(self._lib.dgs_prefilter_get_statistics(self._h, d.ctypes.data_as(C.c_void_p), n.value, s.ctypes.data_as(C.c_void_p), C.byref(n)))
        return d, dict(mean=s[0], stddev=s[1], threshold=s[2], n=int(s[3]))

    def normals(self):
        """Last normal pass: (normals float32 [n,4] normalised and flipped, covariances float32 [n,9] row-major)."""
        n = C.c_int64(0)
        self._check(self._lib.dgs_prefilter_get_normals(self._h, None, None, 0, C.byref(n)))
        nv = np.empty((n.value, 4), np.float32)
        cv = np.empty((n.value, 9), np.float32)
        self._check(self._lib.dgs_prefilter_get_normals(self._h, nv.ctypes.data_as(C.c_void_p), cv.ctypes.data_as(C.c_void_p), n.value, C.byref(n)))
        return nv, cv


def _is_device(x) -> bool:
    return torch is not None and isinstance(x, torch.Tensor) and x.is_cuda
