"""Host-side mirror of the reference's registration objects, over the C ABI (include/dgs_reg.h).

`Registration` keeps the pcl::Registration<PointXYZ,PointXYZ> method names the reference calls
(/root/reference/apps/scan_matching_odometry_nodelet.cpp:180,185,218,222,228,318,327 and
/root/reference/include/hdl_graph_slam/loop_detector.hpp:124,138,145,148,149,155), and
`select_registration_method` mirrors the factory /root/reference/src/hdl_graph_slam/registrations.cpp:22-124
(same `registration_method` strings, same `reg_*` parameter names and defaults).

Clouds are float32 [N,4] arrays (numpy on the host, or torch tensors already resident in HBM); transforms
are 4x4 float32 numpy arrays in ordinary row/column indexing (converted to Eigen's column-major at the ABI).
There is no CPU fallback: constructing a Registration without the HIP library / a gfx950 device raises.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import _lib as L

try:  # torch is plumbing only: device memory + streams
    import torch
except Exception:  # pragma: no cover
    torch = None

__all__ = ["Registration", "RegistrationGroup", "DeviceCloud", "GroupCloud", "select_registration_method", "DgsError"]
DgsError = L.DgsError


def _is_tensor(x) -> bool:
    return torch is not None and isinstance(x, torch.Tensor)


def _cloud_ptr(cloud, sync: bool = True):
    """-> (pointer, n, on_device, keepalive).  sync=False: the caller orders torch's stream itself (once for a whole batch)."""
    if _is_tensor(cloud):
        if cloud.dtype != torch.float32 or cloud.dim() != 2 or cloud.shape[1] != 4:
            raise ValueError("cloud tensors must be float32 [N,4]")
        t = cloud.contiguous()
        if t.is_cuda:
            # the handle works on a stream of its own: whatever produced this tensor on torch's current stream must have finished
            # (include/dgs_reg.h, ordering contract for device pointers); the library is done with the buffer when its call returns
            if sync:
                torch.cuda.current_stream(t.device).synchronize()
            return C.c_void_p(t.data_ptr()), t.shape[0], 1, t
        a = t.numpy()
        return a.ctypes.data_as(C.c_void_p), a.shape[0], 0, a
    a = np.ascontiguousarray(cloud, dtype=np.float32)
    if a.ndim != 2 or a.shape[1] != 4:
        raise ValueError("clouds must be float32 [N,4] (x, y, z, pad)")
    return a.ctypes.data_as(C.c_void_p), a.shape[0], 0, a


def _col16(T) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(T, dtype=np.float32).T.reshape(16))


def _from_col16(t16) -> np.ndarray:
    return np.array(t16, dtype=np.float32).reshape(4, 4).T.copy()


# numpy view of dgs_result (include/dgs_reg.h)
_RESULT_DTYPE = np.dtype([("T", np.float32, (16,)), ("converged", np.int32), ("iterations", np.int32), ("evaluations", np.int32),
                          ("status", np.int32), ("score", np.float64), ("fitness", np.float64)])
assert _RESULT_DTYPE.itemsize == C.sizeof(L.Result)


_ICP_KEYS = {"icp_use_reciprocal_correspondences": "use_reciprocal_correspondences",
             "icp_euclidean_fitness_epsilon": "euclidean_fitness_epsilon", "icp_rotation_epsilon": "rotation_epsilon"}


_PG_KEYS = {"gicp_max_optimizer_iterations": "max_optimizer_iterations", "gicp_rotation_epsilon": "rotation_epsilon",
            "gicp_epsilon": "gicp_epsilon", "gicp_use_reciprocal_correspondences": "use_reciprocal_correspondences"}
_PG_METHODS = ("GICP_HIP", "GICP_OMP_HIP")


def _pcl_gicp_options(lib, method, params):
    """Split the GICP_HIP keywords off `params` into a dgs_pcl_gicp_options (None for another method).  gicp_rotation_epsilon keeps
    its dgs_params meaning (FAST_GICP's) on the other methods."""
    if method not in _PG_METHODS:
        picked = [k for k in params if k in _PG_KEYS and k != "gicp_rotation_epsilon"]
        if picked:
            raise TypeError(f"{sorted(picked)} apply to GICP_HIP / GICP_OMP_HIP only")
        return None
    picked = {k: params.pop(k) for k in list(params) if k in _PG_KEYS}
    o = L.PclGicpOptions()
    rc = lib.dgs_pcl_gicp_options_init(C.byref(o))
    if rc:
        raise DgsError(rc, "dgs_pcl_gicp_options_init")
    for k, v in picked.items():
        f = _PG_KEYS[k]
        setattr(o, f, int(v) if f == "max_optimizer_iterations" else int(bool(v)) if f == "use_reciprocal_correspondences" else float(v))
    return o


def _icp_options(lib, method, params):
    """Split the icp_* keywords off `params` into a dgs_icp_options (None for a method other than ICP_HIP)."""
    picked = {k: params.pop(k) for k in list(params) if k in _ICP_KEYS}
    if method != "ICP_HIP":
        if picked:
            raise TypeError(f"{sorted(picked)} apply to ICP_HIP only")
        return None
    o = L.IcpOptions()
    rc = lib.dgs_icp_options_init(C.byref(o))
    if rc:
        raise DgsError(rc, "dgs_icp_options_init")
    for k, v in picked.items():
        setattr(o, _ICP_KEYS[k], int(bool(v)) if k == "icp_use_reciprocal_correspondences" else float(v))
    return o


class DeviceCloud:
    """A cloud resident in HBM (dgs_cloud): KeyFrame::cloud of the loop detector kept on the device together with its
    NN index / GICP covariances, so a keyframe that is a loop candidate tick after tick is uploaded and indexed once."""

    def __init__(self, registration: "Registration", cloud):
        ptr, n, dev, keep = _cloud_ptr(cloud)
        self._lib = registration._lib
        self._c = C.c_void_p()
        registration._check(self._lib.dgs_cloud_create(registration._h, ptr, n, dev, C.byref(self._c)))
        self.n = n

    def __len__(self):
        return self.n

    def read(self, registration: "Registration") -> np.ndarray:
        """The cloud's points as it holds them now ([n, 4] float32, dgs_cloud_read)."""
        out = np.empty((max(self.n, 1), 4), dtype=np.float32)
        m = C.c_int64(0)
        registration._check(self._lib.dgs_cloud_read(registration._h, self._c, out.ctypes.data_as(C.c_void_p), self.n, 0, C.byref(m)))
        return out[:m.value].copy()

    def close(self):
        if getattr(self, "_c", None) is not None and self._c.value:
            self._lib.dgs_cloud_destroy(self._c)
            self._c = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Registration:
    """pcl::Registration-shaped object backed by one dgs_handle (HIP, gfx950)."""

    def __init__(self, method: str = "NDT_OMP", device: int | None = None, _borrow=None, lib_path: str | None = None, **params):
        lib = L.load(lib_path)   # lib_path: another build of the library (tests of the experiments build)
        self._lib = lib
        self._owns = _borrow is None
        if _borrow is not None:   # a dgs_group member's handle (RegistrationGroup.member): the group owns and destroys it
            self.method, self.params, self._h = method, None, C.c_void_p(_borrow)
            self._converged, self._final, self.last_result, self._keep = False, np.eye(4, dtype=np.float32), None, {}
            return
        exact = {"NDT_OMP": L.METHOD_NDT, "NDT_HIP": L.METHOD_NDT, "FAST_GICP": L.METHOD_GICP, "FAST_GICP_HIP": L.METHOD_GICP,
                 "FAST_VGICP": L.METHOD_VGICP, "FAST_VGICP_HIP": L.METHOD_VGICP, "ICP_HIP": L.METHOD_ICP,
                 "GICP_HIP": L.METHOD_PCL_GICP, "GICP_OMP_HIP": L.METHOD_PCL_GICP, "PCL_NDT_HIP": L.METHOD_PCL_NDT}
        if method not in exact:   # the reference's own "ICP" / "GICP" / "NDT" strings, pclomp::GICP, FAST_VGICP_CUDA: not served under those names
            raise NotImplementedError(f"registration_method {method!r} is not served by the HIP back-ends (served: {sorted(exact)})")
        m = exact[method]
        params = dict(params)
        batch_independent = bool(params.pop("batch_independent", False))   # a switch of the handle, not a dgs_params field
        icp_opt = _icp_options(lib, method, params)
        pg_opt = _pcl_gicp_options(lib, method, params)
        p = L.Params()
        rc = lib.dgs_params_init(C.byref(p), m)
        if rc:
            raise DgsError(rc, "dgs_params_init")
        if device is not None:
            p.device = int(device)
        for k, v in params.items():
            if not hasattr(p, k):
                raise TypeError(f"unknown registration parameter {k!r}")
            setattr(p, k, v)
        self.params = p
        self.method = method
        self._h = C.c_void_p()
        rc = lib.dgs_create(C.byref(p), C.byref(self._h))
        if rc:
            raise DgsError(rc, "dgs_create failed (this package has no CPU fallback): " + (lib.dgs_last_error(None) or b"").decode())
        self.icp_options = icp_opt
        if icp_opt is not None:
            self._check(lib.dgs_set_icp_options(self._h, C.byref(icp_opt)))
        self.pcl_gicp_options = pg_opt
        if pg_opt is not None:
            self._check(lib.dgs_set_pcl_gicp_options(self._h, C.byref(pg_opt)))
        self._converged = False
        self._final = np.eye(4, dtype=np.float32)
        self.last_result = None
        self._keep = {}
        if batch_independent:
            try:
                self.set_batch_independent(True)
            except DgsError:   # a method that refuses the switch: no half-made object is left behind
                self.close()
                raise

    # -- batch-independent results (dgs_set_batch_independent) -------------------------------
    def set_batch_independent(self, on: bool = True):
        """While on, every field of a pair's result, and every fitness, is a function of (parameters, target, source, guess) alone:
        align, align_batch, align_pairs and a RegistrationGroup member give the same bits for the same pair.  FAST_GICP / FAST_VGICP:
        the bits of a single align with the switch off.  NDT_OMP in the re-associated fast order raises DgsError (status 6)."""
        self._check(self._lib.dgs_set_batch_independent(self._h, 1 if on else 0))

    @property
    def batch_independent(self) -> bool:
        on = C.c_int32(0)
        self._check(self._lib.dgs_get_batch_independent(self._h, C.byref(on)))
        return bool(on.value)

    @batch_independent.setter
    def batch_independent(self, on: bool):
        self.set_batch_independent(on)

    # -- lifetime ---------------------------------------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            if getattr(self, "_owns", True):
                self._lib.dgs_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc: int):
        if rc:
            raise DgsError(rc, (self._lib.dgs_last_error(self._h) or b"").decode())

    def set_stream(self, stream=None):
        """Run on a torch.cuda.Stream (or the handle's own stream when None)."""
        ptr = None if stream is None else C.c_void_p(stream.cuda_stream)
        self._check(self._lib.dgs_set_stream(self._h, ptr))

    def synchronize(self):
        self._check(self._lib.dgs_synchronize(self._h))

    # -- pcl::Registration surface ------------------------------------------------------------------------
    def make_cloud(self, cloud) -> DeviceCloud:
        return DeviceCloud(self, cloud)

    def setInputTarget(self, cloud):
        if isinstance(cloud, DeviceCloud):
            self._keep["target"] = cloud
            self._check(self._lib.dgs_set_input_target_cloud(self._h, cloud._c))
            return
        ptr, n, dev, keep = _cloud_ptr(cloud)
        self._check(self._lib.dgs_set_input_target(self._h, ptr, n, dev))

    def setInputSource(self, cloud):
        if isinstance(cloud, DeviceCloud):
            self._keep["source"] = cloud
            self._n_source = cloud.n
            self._check(self._lib.dgs_set_input_source_cloud(self._h, cloud._c))
            return
        ptr, n, dev, keep = _cloud_ptr(cloud)
        self._n_source = n
        self._check(self._lib.dgs_set_input_source(self._h, ptr, n, dev))

    def align(self, guess=None, want_aligned: bool = False):
        """align(*aligned, guess).  Returns the aligned cloud ([N,4] float32) when want_aligned, else None.
        A failed registration never raises for numerical reasons: hasConverged() is False and the final
        transformation is the guess (the contract at scan_matching_odometry_nodelet.cpp:222-226)."""
        g = None if guess is None else _col16(guess)
        gp = None if g is None else g.ctypes.data_as(C.c_void_p)
        res = L.Result()
        out = None
        outp = None
        if want_aligned:
            out = np.empty((self._n_source, 4), dtype=np.float32)
            outp = out.ctypes.data_as(C.c_void_p)
        rc = self._lib.dgs_align(self._h, gp, C.byref(res), outp, 0)
        self.last_result = res
        self._converged = bool(res.converged)
        self._final = _from_col16(res.final_transformation)
        if rc in (L.DGS_OK,):
            return out
        if rc in (3, 4):  # PCL prints an error and returns; converged stays false
            return None
        self._check(rc)
        return out

    def hasConverged(self) -> bool:
        return self._converged

    def getFinalTransformation(self) -> np.ndarray:
        return self._final.copy()

    def getFitnessScore(self, max_range: float = 1.7976931348623157e308) -> float:
        s = C.c_double(0)
        self._check(self._lib.dgs_get_fitness_score(self._h, max_range, C.byref(s)))
        return s.value

    def getInlierFraction(self, max_sq_dist: float = 0.25) -> float:
        """The nearestKSearch loop of publish_scan_matching_status (scan_matching_odometry_nodelet.cpp:321-332)."""
        f = C.c_double(0)
        self._check(self._lib.dgs_get_inlier_fraction(self._h, max_sq_dist, C.byref(f)))
        return f.value

    def nearestKSearch(self, queries):
        """getSearchMethodTarget()->nearestKSearch(pt, 1, ...) for a batch of points -> (indices, sq_dists)."""
        ptr, m, dev, keep = _cloud_ptr(queries)
        if dev:
            raise ValueError("host queries only in the Python mirror")
        idx = np.empty(m, dtype=np.int32)
        sq = np.empty(m, dtype=np.float32)
        self._check(self._lib.dgs_nearest_search_target(self._h, ptr, m, 0, idx.ctypes.data_as(C.c_void_p), sq.ctypes.data_as(C.c_void_p)))
        return idx, sq

    def nn_fitness_distances(self, queries):
        """Test hook: squared 1-NN distances through the fitness pass's grid index (must equal nearestKSearch's)."""
        ptr, m, dev, keep = _cloud_ptr(queries)
        if dev:
            raise ValueError("host queries only in the Python mirror")
        sq = np.empty(m, dtype=np.float32)
        self._check(self._lib.dgs_nn_fitness_distances(self._h, ptr, m, 0, sq.ctypes.data_as(C.c_void_p)))
        return sq

    def find_loop_candidates(self, accum_distance, xy, new_accum_distance: float, new_xy, accum_distance_thresh: float, distance_thresh: float) -> np.ndarray:
        """LoopDetector::find_candidates (loop_detector.hpp:83-111) on the device: indices of the candidate keyframes, in keyframe order."""
        acc = np.ascontiguousarray(accum_distance, dtype=np.float64)
        p = np.ascontiguousarray(xy, dtype=np.float64).reshape(-1, 2)
        q = np.ascontiguousarray(new_xy, dtype=np.float64)
        n = acc.shape[0]
        out = np.empty(max(n, 1), dtype=np.int32)
        m = C.c_int64(0)
        self._check(self._lib.dgs_find_loop_candidates(self._h, acc.ctypes.data_as(C.c_void_p), p.ctypes.data_as(C.c_void_p), n, 0, float(new_accum_distance),
                                                       q.ctypes.data_as(C.c_void_p), float(accum_distance_thresh), float(distance_thresh),
                                                       out.ctypes.data_as(C.c_void_p), n, C.byref(m)))
        return out[:m.value].copy()

    def calc_fitness_score(self, cloud1, cloud2, relpose=None, max_range: float = 1.7976931348623157e308) -> float:
        """InformationMatrixCalculator::calc_fitness_score (information_matrix_calculator.cpp:77-108) on the device."""
        p1, n1, d1, k1 = _cloud_ptr(cloud1)
        p2, n2, d2, k2 = _cloud_ptr(cloud2)
        if n1 and n2 and d1 != d2:
            raise ValueError("both clouds must live on the same side (host arrays or device tensors)")
        t = None if relpose is None else _col16(relpose)
        s = C.c_double(0)
        self._check(self._lib.dgs_calc_fitness_score(self._h, p1, n1, p2, n2, d1 if n1 else d2, None if t is None else t.ctypes.data_as(C.c_void_p),
                                                      max_range, C.byref(s)))
        return s.value

    def _cloud_array(self, clouds):
        """-> (void* array of dgs_cloud, the DeviceClouds behind it); arrays and tensors become temporary DeviceClouds, one per object."""
        made = {}
        objs = []
        for c in clouds:
            if not isinstance(c, DeviceCloud):
                if id(c) not in made:
                    made[id(c)] = DeviceCloud(self, c)
                c = made[id(c)]
            objs.append(c)
        arr = (C.c_void_p * max(len(objs), 1))(*[o._c.value for o in objs])
        return arr, objs, list(made.values())

    def calc_fitness_score_batch(self, cloud1s, cloud2s, relposes=None, max_range: float = 1.7976931348623157e308, return_used: bool = False):
        """calc_fitness_score for every edge (cloud1s[e], cloud2s[e], relposes[e]) in one call (dgs_calc_fitness_score_batch_clouds): the
        index over each cloud1 is the one its DeviceCloud keeps, all edges are walked by one launch.  -> float64 [E] (and int64 [E] with
        return_used: the points within max_range).  numpy arrays and device tensors are wrapped in DeviceClouds for the call."""
        cloud1s, cloud2s = list(cloud1s), list(cloud2s)
        n = len(cloud1s)
        if len(cloud2s) != n:
            raise ValueError("cloud1s and cloud2s differ in length")
        arr, objs, temps = self._cloud_array(cloud1s + cloud2s)
        a1 = (C.c_void_p * max(n, 1))(*arr[:n])
        a2 = (C.c_void_p * max(n, 1))(*arr[n:2 * n])
        t = None
        if relposes is not None:
            if len(relposes) != n:
                raise ValueError("relposes and the clouds differ in length")
            t = np.ascontiguousarray(np.stack([_col16(r) for r in relposes]) if n else np.zeros((0, 16), np.float32), dtype=np.float32)
        scores = np.empty(n, dtype=np.float64)
        used = np.zeros(n, dtype=np.int64)
        try:
            self._check(self._lib.dgs_calc_fitness_score_batch_clouds(self._h, n, C.cast(a1, C.c_void_p), C.cast(a2, C.c_void_p),
                                                                      None if t is None else t.ctypes.data_as(C.c_void_p), float(max_range),
                                                                      scores.ctypes.data_as(C.c_void_p), used.ctypes.data_as(C.c_void_p)))
        finally:
            for c in temps:
                c.close()
        return (scores, used) if return_used else scores

    def calc_inlier_fraction_batch(self, cloud1s, cloud2s, relposes=None, max_sq_dist: float = 0.25, return_counts: bool = False):
        """getInlierFraction for every edge (cloud1s[e] indexed, cloud2s[e] moved by relposes[e]) in one call
        (dgs_calc_inlier_fraction_batch_clouds): the count of an edge is getInlierFraction's of the same pair exactly.  -> float64 [E]
        (NaN where a cloud is empty), and int64 [E] with return_counts."""
        cloud1s, cloud2s = list(cloud1s), list(cloud2s)
        n = len(cloud1s)
        if len(cloud2s) != n:
            raise ValueError("cloud1s and cloud2s differ in length")
        arr, objs, temps = self._cloud_array(cloud1s + cloud2s)
        a1 = (C.c_void_p * max(n, 1))(*arr[:n])
        a2 = (C.c_void_p * max(n, 1))(*arr[n:2 * n])
        t = None
        if relposes is not None:
            if len(relposes) != n:
                raise ValueError("relposes and the clouds differ in length")
            t = np.ascontiguousarray(np.stack([_col16(r) for r in relposes]) if n else np.zeros((0, 16), np.float32), dtype=np.float32)
        fractions = np.empty(n, dtype=np.float64)
        counts = np.zeros(n, dtype=np.int64)
        try:
            self._check(self._lib.dgs_calc_inlier_fraction_batch_clouds(self._h, n, C.cast(a1, C.c_void_p), C.cast(a2, C.c_void_p),
                                                                        None if t is None else t.ctypes.data_as(C.c_void_p), float(max_sq_dist),
                                                                        fractions.ctypes.data_as(C.c_void_p), counts.ctypes.data_as(C.c_void_p)))
        finally:
            for c in temps:
                c.close()
        return (fractions, counts) if return_counts else fractions

    _FILTERS = {"NONE": 0, "VOXELGRID": 1, "APPROX_VOXELGRID": 2}

    def assign_batch(self, clouds, inputs, downsample_method: str = "NONE", leaf_size: float = 0.1) -> np.ndarray:
        """dgs_cloud_assign_batch: DeviceCloud clouds[i] is refilled with inputs[i] (numpy arrays, or device tensors) passed through
        downsample_method -- one chain of launches and two host waits for the whole batch under VOXELGRID, each cloud receiving the
        bits of voxel_grid_filter(inputs[i], leaf_size).  Index and covariances of the clouds are dropped, registrations that borrowed
        one lose it.  -> the new sizes, int64 [n]."""
        clouds, inputs = list(clouds), list(inputs)
        n = len(clouds)
        if len(inputs) != n:
            raise ValueError("clouds and inputs differ in length")
        if not all(isinstance(c, DeviceCloud) for c in clouds):
            raise TypeError("assign_batch refills DeviceClouds")
        if downsample_method not in self._FILTERS:
            raise ValueError(f"downsample_method {downsample_method!r} is none of {sorted(self._FILTERS)}")
        ptrs = (C.c_void_p * max(n, 1))()
        sizes = (C.c_int64 * max(n, 1))()
        keep, devs, cuda_devs = [], set(), set()
        for i, a in enumerate(inputs):
            ptr, m, dev, k = _cloud_ptr(a, sync=False)
            ptrs[i] = ptr.value if ptr.value else 0
            sizes[i] = m
            keep.append(k)
            if m:
                devs.add(dev)
            if dev:
                cuda_devs.add(k.device)
        if len(devs) > 1:
            raise ValueError("inputs must be all host arrays or all device tensors")
        for d in cuda_devs:   # one ordering point for the whole batch (the device-pointer contract of include/dgs_reg.h)
            torch.cuda.current_stream(d).synchronize()
        arr = (C.c_void_p * max(n, 1))(*[c._c.value for c in clouds])
        out = np.zeros(max(n, 1), dtype=np.int64)
        rc = self._lib.dgs_cloud_assign_batch(self._h, n, C.cast(ptrs, C.c_void_p), C.cast(sizes, C.c_void_p), devs.pop() if devs else 0,
                                              self._FILTERS[downsample_method], float(leaf_size), C.cast(arr, C.c_void_p), out.ctypes.data_as(C.c_void_p))
        if rc != 5:   # DGS_ERR_GRID_TOO_LARGE leaves every cloud as it was; anything else that ran has resized them
            for c, m in zip(clouds, out):
                c.n = int(self._lib.dgs_cloud_size(c._c))
        self._check(rc)
        return out[:n].copy()

    def cloud_assign_counts(self) -> dict:
        """Of the last assign_batch: kernel launches, host waits, clouds."""
        c = (C.c_int64 * 8)()
        self._check(self._lib.dgs_cloud_assign_get_counts(self._h, C.cast(c, C.c_void_p)))
        return {"launches": c[0], "host_waits": c[1], "clouds": c[2]}

    def build_indices(self, clouds):
        """dgs_cloud_build_indices: the Hilbert-ordered NN index of every listed DeviceCloud that has none, in one batched build."""
        clouds = list(clouds)
        if not all(isinstance(c, DeviceCloud) for c in clouds):
            raise TypeError("build_indices takes DeviceClouds")
        arr = (C.c_void_p * max(len(clouds), 1))(*[c._c.value for c in clouds])
        self._check(self._lib.dgs_cloud_build_indices(self._h, len(clouds), C.cast(arr, C.c_void_p)))

    def fitness_batch_counts(self) -> dict:
        """Of the last calc_fitness_score_batch / build_indices: kernel launches, host waits, edges, indices built, partial rows; and
        single_builds: the single-cloud index builds this handle made by any other path since it was created."""
        c = (C.c_int64 * 8)()
        self._check(self._lib.dgs_fitness_batch_get_counts(self._h, C.cast(c, C.c_void_p)))
        return {"launches": c[0], "host_waits": c[1], "edges": c[2], "indices_built": c[3], "rows": c[4], "single_builds": c[5]}

    def build_covariances(self, clouds):
        """dgs_cloud_build_covariances: the missing NN indices, then the k-NN covariances this handle's method and parameters would make
        of every listed DeviceCloud on first use, for all of them in one search and one covariance launch per chunk.  Kept on the clouds;
        bit for bit what setInputSource(cloud) + align would have made.  FAST_GICP, FAST_VGICP, GICP_HIP / GICP_OMP_HIP."""
        clouds = list(clouds)
        if not all(isinstance(c, DeviceCloud) for c in clouds):
            raise TypeError("build_covariances takes DeviceClouds")
        arr = (C.c_void_p * max(len(clouds), 1))(*[c._c.value for c in clouds])
        self._check(self._lib.dgs_cloud_build_covariances(self._h, len(clouds), C.cast(arr, C.c_void_p)))

    def covariance_batch_counts(self) -> dict:
        """Of the last batched covariance pass (build_covariances, align_pairs, an align_batch of two or more sources): kernel launches,
        host waits, clouds listed / covered / already cached, chunks, clouds served one at a time by a fallback, indices built."""
        c = (C.c_int64 * 8)()
        self._check(self._lib.dgs_cloud_covariances_get_counts(self._h, C.cast(c, C.c_void_p)))
        return {"launches": c[0], "host_waits": c[1], "listed": c[2], "covered": c[3], "cached": c[4], "chunks": c[5], "fallback": c[6],
                "indices_built": c[7]}

    def voxel_grid_filter(self, cloud, leaf_size: float, approximate: bool = False):
        """pcl::VoxelGrid centroid filter (scan_matching_odometry_nodelet.cpp:83-89,155-165) -- or, with approximate=True,
        pcl::ApproximateVoxelGrid (:90-96) -- on the device.
        numpy in -> numpy out; device tensor in -> device tensor out (no host round trip of the points)."""
        fn = self._lib.dgs_approx_voxel_grid_filter if approximate else self._lib.dgs_voxel_grid_filter
        ptr, n, dev, keep = _cloud_ptr(cloud)
        m = C.c_int64(0)
        if dev:
            out = torch.empty((max(n, 1), 4), dtype=torch.float32, device=cloud.device)
            self._check(fn(self._h, ptr, n, 1, leaf_size, C.c_void_p(out.data_ptr()), n, 1, C.byref(m)))
            return out[:m.value]
        out = np.empty((max(n, 1), 4), dtype=np.float32)
        self._check(fn(self._h, ptr, n, 0, leaf_size, out.ctypes.data_as(C.c_void_p), n, 0, C.byref(m)))
        return out[:m.value].copy()

    # -- batched candidates (loop_detector.hpp:137-156) ----------------------------------------------------
    def _align_batch_raw(self, sources, guesses, compute_fitness, fitness_max_range):
        """-> ctypes array of dgs_result, one per source"""
        n = len(sources)
        g = None
        gp = None
        if guesses is not None:
            ga = np.asarray(guesses, dtype=np.float32)
            if ga.ndim == 3:   # [n,4,4] row-major -> n x column-major float[16]
                g = np.ascontiguousarray(ga.transpose(0, 2, 1).reshape(n, 16))
            else:
                g = np.ascontiguousarray(np.stack([_col16(G) for G in guesses]))
            gp = g.ctypes.data_as(C.c_void_p)
        res = (L.Result * n)()
        if all(isinstance(s_, DeviceCloud) for s_ in sources):
            cl = (C.c_void_p * n)(*[s_._c.value for s_ in sources])
            self._check(self._lib.dgs_align_batch_clouds(self._h, n, cl, gp, 1 if compute_fitness else 0, fitness_max_range, res))
            return res
        ptrs = (C.c_void_p * n)()
        sizes = (C.c_int64 * n)()
        keep = []
        devs = set()
        cuda_devs = set()
        for i, s in enumerate(sources):
            ptr, m, dev, k = _cloud_ptr(s, sync=False)
            ptrs[i] = ptr.value if ptr.value else 0
            sizes[i] = m
            keep.append(k)
            if m:
                devs.add(dev)
            if dev:
                cuda_devs.add(k.device)
        if len(devs) > 1:
            raise ValueError("sources must be all host arrays or all device tensors")
        on_device = devs.pop() if devs else 0
        for d in cuda_devs:   # one ordering point for the whole batch (the device-pointer contract of include/dgs_reg.h)
            torch.cuda.current_stream(d).synchronize()
        self._check(self._lib.dgs_align_batch(self._h, n, ptrs, sizes, on_device, gp, 1 if compute_fitness else 0, fitness_max_range, res))
        return res

    def align_batch(self, sources, guesses=None, compute_fitness: bool = True, fitness_max_range: float = 1.7976931348623157e308):
        if len(sources) == 0:
            return []
        res = self._align_batch_raw(sources, guesses, compute_fitness, fitness_max_range)
        return [dict(T=_from_col16(r.final_transformation), converged=bool(r.converged), iterations=r.iterations,
                     evaluations=r.evaluations, status=r.status, score=r.score, fitness=r.fitness) for r in res]

    def align_batch_records(self, sources, guesses=None, compute_fitness: bool = True, fitness_max_range: float = 1.7976931348623157e308):
        """align_batch as the loop detector's exchange records: float64 [n, 20] = (-1, converged, fitness, status, T row-major),
        filled from the C ABI's result array in one numpy pass (column 0 is left for the caller's candidate index)."""
        n = len(sources)
        out = np.full((n, 20), -1.0, dtype=np.float64)
        if n == 0:
            return out
        res = self._align_batch_raw(sources, guesses, compute_fitness, fitness_max_range)
        a = np.frombuffer(res, dtype=_RESULT_DTYPE, count=n)
        out[:, 1] = a["converged"] != 0
        out[:, 2] = a["fitness"]
        out[:, 3] = a["status"]
        out[:, 4:20] = a["T"].reshape(n, 4, 4).transpose(0, 2, 1).reshape(n, 16)   # column-major -> row-major
        return out

    # -- pairs that each name their own target (a tick of the loop detector: every new keyframe is a target) ---------------
    def _align_pairs_raw(self, targets, sources, guesses, compute_fitness, fitness_max_range):
        """-> ctypes array of dgs_result, one per pair (dgs_align_pairs_clouds); arrays and tensors are resident for the call only"""
        targets, sources = list(targets), list(sources)
        n = len(targets)
        if len(sources) != n:
            raise ValueError("targets and sources differ in length")
        if n == 0:   # nothing to register, whatever shape an empty `guesses` has
            return (L.Result * 1)()
        gp = None
        if guesses is not None:
            if len(guesses) != n:
                raise ValueError("guesses and the clouds differ in length")
            ga = np.asarray(guesses, dtype=np.float32)
            g = np.ascontiguousarray(ga.transpose(0, 2, 1).reshape(n, 16)) if ga.ndim == 3 else np.ascontiguousarray(np.stack([_col16(G) for G in guesses]))
            gp = g.ctypes.data_as(C.c_void_p)
        arr, objs, temps = self._cloud_array(targets + sources)
        at = (C.c_void_p * max(n, 1))(*arr[:n])
        as_ = (C.c_void_p * max(n, 1))(*arr[n:2 * n])
        res = (L.Result * max(n, 1))()
        try:
            self._check(self._lib.dgs_align_pairs_clouds(self._h, n, C.cast(at, C.c_void_p), C.cast(as_, C.c_void_p), gp, 1 if compute_fitness else 0,
                                                         float(fitness_max_range), res))
        finally:
            for c in temps:
                c.close()
        return res

    def align_pairs(self, targets, sources, guesses=None, compute_fitness: bool = True, fitness_max_range: float = 1.7976931348623157e308):
        """Pair i registers sources[i] against targets[i] from guesses[i]; all pairs advance together in one chain of launches
        (dgs_align_pairs_clouds; FAST_GICP and GICP_HIP / GICP_OMP_HIP).  -> one dict per pair, as align_batch gives.  The registration's own target, source,
        last result and counts() are untouched.  DeviceClouds are used as they are (and keep the index and covariances made here).
        GICP_HIP: a cloud of fewer than k points fails the pairs that name it (status 1), not the call; pcl_gicp_trajectory(i) answers
        for pair i of this call afterwards."""
        n = len(targets)
        res = self._align_pairs_raw(targets, sources, guesses, compute_fitness, fitness_max_range)
        return [dict(T=_from_col16(r.final_transformation), converged=bool(r.converged), iterations=r.iterations,
                     evaluations=r.evaluations, status=r.status, score=r.score, fitness=r.fitness) for r in res[:n]]

    def align_pairs_records(self, targets, sources, guesses=None, compute_fitness: bool = True, fitness_max_range: float = 1.7976931348623157e308):
        """align_pairs as the loop detector's exchange records: float64 [n, 20], laid out as align_batch_records'."""
        n = len(targets)
        out = np.full((n, 20), -1.0, dtype=np.float64)
        res = self._align_pairs_raw(targets, sources, guesses, compute_fitness, fitness_max_range)
        if n == 0:
            return out
        a = np.frombuffer(res, dtype=_RESULT_DTYPE, count=n)
        out[:, 1] = a["converged"] != 0
        out[:, 2] = a["fitness"]
        out[:, 3] = a["status"]
        out[:, 4:20] = a["T"].reshape(n, 4, 4).transpose(0, 2, 1).reshape(n, 16)   # column-major -> row-major
        return out

    # -- pcl::IterativeClosestPoint setters (ICP_HIP) ----------------------------------------------------------
    def _set_icp(self, field, value):
        if self.method != "ICP_HIP":
            raise NotImplementedError(f"{field} is an ICP_HIP setting")
        setattr(self.icp_options, field, value)
        self._check(self._lib.dgs_set_icp_options(self._h, C.byref(self.icp_options)))

    def setUseReciprocalCorrespondences(self, on: bool):   # ICP_HIP: reciprocal mode; GICP_HIP: accepted, without effect (as upstream)
        if self.method in _PG_METHODS:
            self._set_pg("use_reciprocal_correspondences", 1 if on else 0)
        else:
            self._set_icp("use_reciprocal_correspondences", 1 if on else 0)

    def setEuclideanFitnessEpsilon(self, eps: float):
        self._set_icp("euclidean_fitness_epsilon", float(eps))

    def setTransformationRotationEpsilon(self, eps: float):
        self._set_icp("rotation_epsilon", float(eps))

    def icp_trajectory(self, pair: int = 0):
        """ICP_HIP test hook: per iteration of pair `pair` of the last align / batch -> (T_k [m,4,4] float32, mse [m], kept pairs [m])."""
        cap = max(1, int(self.params.maximum_iterations)) if self.params is not None else 1024
        T = np.zeros((cap, 16), np.float32)
        mse = np.zeros(cap, np.float64)
        nc = np.zeros(cap, np.int32)
        ln = C.c_int32(0)
        self._check(self._lib.dgs_icp_get_trajectory(self._h, pair, T.ctypes.data_as(C.c_void_p), mse.ctypes.data_as(C.c_void_p),
                                                     nc.ctypes.data_as(C.c_void_p), cap, C.byref(ln)))
        m = min(ln.value, cap)
        return T[:m].reshape(m, 4, 4).transpose(0, 2, 1).copy(), mse[:m].copy(), nc[:m].copy()

    # -- pcl::GeneralizedIterativeClosestPoint setters (GICP_HIP / GICP_OMP_HIP) -------------------------------------
    def _set_pg(self, field, value):
        if self.method not in _PG_METHODS:
            raise NotImplementedError(f"{field} is a GICP_HIP setting")
        setattr(self.pcl_gicp_options, field, value)
        self._check(self._lib.dgs_set_pcl_gicp_options(self._h, C.byref(self.pcl_gicp_options)))

    def setMaximumOptimizerIterations(self, n: int):
        self._set_pg("max_optimizer_iterations", int(n))

    def setRotationEpsilon(self, eps: float):
        self._set_pg("rotation_epsilon", float(eps))

    def setCorrespondenceRandomness(self, k: int):
        """k_correspondences_ of a GICP_HIP handle: the covariances are recomputed at the next align."""
        if self.method not in _PG_METHODS:
            raise NotImplementedError("setCorrespondenceRandomness on a live handle is a GICP_HIP setting")
        self._check(self._lib.dgs_pcl_gicp_set_correspondence_randomness(self._h, int(k)))
        self.params.gicp_correspondence_randomness = int(k)

    def pcl_gicp_trajectory(self, pair: int = 0):
        """GICP_HIP test hook: per outer iteration of pair `pair` of the last align / batch -> dict of transformation_ [m,4,4] float32,
        kept pairs, BFGS inner iterations, evaluation passes [m] and the last f [m]."""
        cap = max(1, int(self.params.maximum_iterations)) if self.params is not None else 1024
        T = np.zeros((cap, 16), np.float32)
        nc, inner, passes = (np.zeros(cap, np.int32) for _ in range(3))
        f = np.zeros(cap, np.float64)
        ln = C.c_int32(0)
        self._check(self._lib.dgs_pcl_gicp_get_trajectory(self._h, pair, T.ctypes.data_as(C.c_void_p), nc.ctypes.data_as(C.c_void_p),
                                                          inner.ctypes.data_as(C.c_void_p), passes.ctypes.data_as(C.c_void_p),
                                                          f.ctypes.data_as(C.c_void_p), cap, C.byref(ln)))
        m = min(ln.value, cap)
        return dict(T=T[:m].reshape(m, 4, 4).transpose(0, 2, 1).copy(), n=nc[:m].copy(), inner=inner[:m].copy(), passes=passes[:m].copy(),
                    f=f[:m].copy())

    def pcl_gicp_evaluate(self, x, transformation=None, guess=None):
        """GICP_HIP test hook: one correspondence pass at (transformation_, guess) over the current source and target, then
        (kept pairs m, f, gradient [6]) at state x = (tx, ty, tz, roll, pitch, yaw)."""
        def colmajor(T):
            return None if T is None else np.ascontiguousarray(np.asarray(T, np.float32).T)
        Tc, Gc = colmajor(transformation), colmajor(guess)
        self._check(self._lib.dgs_pcl_gicp_set_probe(self._h, None if Tc is None else Tc.ctypes.data_as(C.c_void_p),
                                                     None if Gc is None else Gc.ctypes.data_as(C.c_void_p)))
        x = np.ascontiguousarray(x, np.float64)
        m = C.c_int32(0)
        f = C.c_double(0)
        g = np.zeros(6)
        self._check(self._lib.dgs_pcl_gicp_evaluate(self._h, x.ctypes.data_as(C.c_void_p), C.byref(m), C.byref(f), g.ctypes.data_as(C.c_void_p)))
        return int(m.value), float(f.value), g

    # -- measurement / test hooks ---------------------------------------------------------------------------
    def profile_enable(self, on: bool = True):
        self._check(self._lib.dgs_profile_enable(self._h, 1 if on else 0))

    def profile_reset(self):
        self._check(self._lib.dgs_profile_reset(self._h))

    def profile_get(self, kernel_id: int):
        ms = C.c_double(0)
        n = C.c_int64(0)
        self._check(self._lib.dgs_profile_get(self._h, kernel_id, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def counts(self):
        out = (C.c_int64 * 8)()
        self._check(self._lib.dgs_get_counts(self._h, out))
        return dict(target_points=out[0], source_points=out[1], valid_voxels=out[2], occupied_voxels=out[3],
                    grid_cells=out[4], evaluations=out[5], evaluations_reused=out[6])

    def vgicp_voxels(self):
        """FAST_VGICP target voxel map -> (coords [V,3], counts [V], means [V,3], covs [V,3,3]) in ascending (z, y, x) order"""
        n = C.c_int64(0)
        self._check(self._lib.dgs_vgicp_get_voxels(self._h, 0, None, None, None, None, C.byref(n)))
        coords = np.zeros((n.value, 3), np.int32)
        counts = np.zeros(n.value, np.int32)
        means = np.zeros((n.value, 3))
        covs = np.zeros((n.value, 3, 3))
        self._check(self._lib.dgs_vgicp_get_voxels(self._h, n.value, coords.ctypes.data_as(C.c_void_p), counts.ctypes.data_as(C.c_void_p),
                                                   means.ctypes.data_as(C.c_void_p), covs.ctypes.data_as(C.c_void_p), C.byref(n)))
        return coords, counts, means, covs

    def ndt_derivatives(self, p, T=None, hessian: bool = True):
        """One computeDerivatives evaluation at pose p (cloud transformed by T when given).  hessian=False (PCL_NDT_HIP only): the
        score + gradient evaluation of a More-Thuente trial; the Hessian comes back as zeros."""
        p = np.ascontiguousarray(p, dtype=np.float64)
        t16 = None if T is None else _col16(T)
        s = C.c_double(0)
        g = np.zeros(6)
        H = np.zeros((6, 6))
        self._check(self._lib.dgs_ndt_derivatives(self._h, p.ctypes.data_as(C.c_void_p), None if t16 is None else t16.ctypes.data_as(C.c_void_p),
                                                   C.byref(s), g.ctypes.data_as(C.c_void_p), H.ctypes.data_as(C.c_void_p) if hessian else None))
        return s.value, g, H

    def pcl_ndt_neighbours(self, queries):
        """PCL_NDT_HIP test hook (dgs_pcl_ndt_neighbours): per query point, taken as it is, the number of valid voxels whose float
        centroid lies within the resolution, and their numbers (rows of the device's voxel table) ascending, -1 padded: (m,), (m, 27)."""
        ptr, m, dev, keep = _cloud_ptr(queries)
        counts = np.zeros(m, np.int32)
        ids = np.full((m, 27), -1, np.int32)
        self._check(self._lib.dgs_pcl_ndt_neighbours(self._h, ptr, m, dev, counts.ctypes.data_as(C.c_void_p), ids.ctypes.data_as(C.c_void_p)))
        return counts, ids

    def ndt_hessian_double(self, p):
        """computeHessian in PCL's double form at pose p (dgs_ndt_hessian_double; upstream evaluation orders only)."""
        p = np.ascontiguousarray(p, dtype=np.float64)
        H = np.zeros((6, 6))
        self._check(self._lib.dgs_ndt_hessian_double(self._h, p.ctypes.data_as(C.c_void_p), H.ctypes.data_as(C.c_void_p)))
        return H

    def ndt_score_gradient(self, p):
        """The score + gradient evaluation of a More-Thuente trial at pose p (dgs_ndt_score_gradient; upstream evaluation orders only)."""
        p = np.ascontiguousarray(p, dtype=np.float64)
        s = C.c_double(0)
        g = np.zeros(6)
        self._check(self._lib.dgs_ndt_score_gradient(self._h, p.ctypes.data_as(C.c_void_p), C.byref(s), g.ctypes.data_as(C.c_void_p)))
        return s.value, g

    def gicp_covariances(self, which: str = "source", n: int | None = None):
        c = self.counts()   # the library writes one 3x3 per point of the cloud it holds: size the buffer from ITS count
        n = int(c["source_points"] if which == "source" else c["target_points"])
        out = np.zeros((n, 3, 3))
        self._check(self._lib.dgs_gicp_get_covariances(self._h, 0 if which == "source" else 1, out.ctypes.data_as(C.c_void_p)))
        return out

    def gicp_linearize(self, T, error_only: bool = False):
        T = np.ascontiguousarray(T, dtype=np.float64)
        e = C.c_double(0)
        H = np.zeros((6, 6))
        b = np.zeros(6)
        self._check(self._lib.dgs_gicp_linearize(self._h, T.ctypes.data_as(C.c_void_p), 1 if error_only else 0, C.byref(e),
                                                  H.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p)))
        return (e.value,) if error_only else (e.value, H, b)

    def ndt_trajectory(self, pair: int = 0):
        buf = np.zeros((72, 6))
        n = C.c_int32(0)
        self._check(self._lib.dgs_ndt_get_trajectory(self._h, pair, buf.ctypes.data_as(C.c_void_p), C.byref(n)))
        return buf[:n.value].copy()

    def ndt_voxels(self, raw: bool = False):
        """The target's voxel table ordered by cell key; raw=True: in the device's own row order (the voxel numbers of pcl_ndt_neighbours),
        the row of non-finite points (key -1) included."""
        n = C.c_int64(0)
        self._check(self._lib.dgs_ndt_get_voxels(self._h, C.byref(n), None, None, None, None, None))
        nv = n.value
        keys = np.zeros(nv, np.int64)
        counts = np.zeros(nv, np.int32)
        valid = np.zeros(nv, np.int32)
        mean = np.zeros((nv, 3))
        icov = np.zeros((nv, 3, 3))
        if nv:
            self._check(self._lib.dgs_ndt_get_voxels(self._h, C.byref(n), keys.ctypes.data_as(C.c_void_p), counts.ctypes.data_as(C.c_void_p),
                                                      valid.ctypes.data_as(C.c_void_p), mean.ctypes.data_as(C.c_void_p),
                                                      icov.ctypes.data_as(C.c_void_p)))
        if raw:
            return dict(keys=keys, counts=counts, valid=valid.astype(bool), mean=mean, icov=icov)
        keep = keys >= 0
        o = np.argsort(keys[keep])
        return dict(keys=keys[keep][o], counts=counts[keep][o], valid=valid[keep][o].astype(bool), mean=mean[keep][o], icov=icov[keep][o])


class GroupCloud:
    """dgs_group_cloud: KeyFrame::cloud (keyframe.hpp:51) resident on a group's devices -- on one member (`owner` >= 0: member
    owner mod G) or on every member (`owner` None / -1: the new keyframe, every member's target)."""

    def __init__(self, group: "RegistrationGroup", cloud, owner=None):
        ptr, n, dev, keep = _cloud_ptr(cloud)
        if dev:
            raise ValueError("a group cloud is uploaded from the host (KeyFrame::cloud)")
        self._lib = group._lib
        self._group = group
        self._c = C.c_void_p()
        group._check(self._lib.dgs_group_cloud_create(group._g, ptr, n, -1 if owner is None or owner < 0 else int(owner), C.byref(self._c)))
        self.n = n

    def __len__(self):
        return self.n

    @property
    def copies(self) -> int:
        return int(self._lib.dgs_group_cloud_copies(self._c))

    def trim(self, owner: int = -1):
        """dgs_group_cloud_trim: keep the copy on member owner mod G (or the first holder's), drop the others -- a keyframe that was every
        member's target for a tick goes back to one copy on its owner."""
        self._group._check(self._lib.dgs_group_cloud_trim(self._group._g, self._c, int(owner)))

    def close(self):
        if getattr(self, "_c", None) is not None and self._c.value:
            self._lib.dgs_group_cloud_destroy(self._c)
            self._c = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class RegistrationGroup:
    """dgs_group (include/dgs_reg.h): the candidate loop of LoopDetector::matching (loop_detector.hpp:137-156) sharded over
    several GPUs of ONE process -- candidate c goes to device c mod G, the result records come back through an RCCL all-gather
    in original candidate order.  Offers the batch surface LoopDetector drives (setInputTarget / align_batch[_records]), so a
    LoopDetector(registration=RegistrationGroup(...)) is the single-process counterpart of the one-process-per-GPU sharding."""

    def __init__(self, method: str = "NDT_OMP", devices=(0,), **params):
        lib = L.load()
        self._lib = lib
        exact = {"NDT_OMP": L.METHOD_NDT, "NDT_HIP": L.METHOD_NDT, "FAST_GICP": L.METHOD_GICP, "FAST_GICP_HIP": L.METHOD_GICP,
                 "FAST_VGICP": L.METHOD_VGICP, "FAST_VGICP_HIP": L.METHOD_VGICP, "ICP_HIP": L.METHOD_ICP,
                 "GICP_HIP": L.METHOD_PCL_GICP, "GICP_OMP_HIP": L.METHOD_PCL_GICP, "PCL_NDT_HIP": L.METHOD_PCL_NDT}
        if method not in exact:
            raise NotImplementedError(f"registration_method {method!r} is not served by the HIP back-ends")
        params = dict(params)
        batch_independent = bool(params.pop("batch_independent", False))   # a switch of the members' handles, not a dgs_params field
        icp_opt = _icp_options(lib, method, params)
        pg_opt = _pcl_gicp_options(lib, method, params)
        p = L.Params()
        rc = lib.dgs_params_init(C.byref(p), exact[method])
        if rc:
            raise DgsError(rc, "dgs_params_init")
        for k, v in params.items():
            if not hasattr(p, k):
                raise TypeError(f"unknown registration parameter {k!r}")
            setattr(p, k, v)
        self.devices = [int(d) for d in devices]
        self.method = method
        dv = (C.c_int32 * len(self.devices))(*self.devices)
        self._g = C.c_void_p()
        rc = lib.dgs_group_create(C.byref(p), dv, len(self.devices), C.byref(self._g))
        if rc:
            raise DgsError(rc, "dgs_group_create failed (this package has no CPU fallback): " + (lib.dgs_last_error(None) or b"").decode())
        self.icp_options = icp_opt
        if icp_opt is not None:
            self._check(lib.dgs_group_set_icp_options(self._g, C.byref(icp_opt)))
        self.pcl_gicp_options = pg_opt
        if pg_opt is not None:
            self._check(lib.dgs_group_set_pcl_gicp_options(self._g, C.byref(pg_opt)))
        self.best_index = -1
        self.best_score = float("inf")
        self._batch_independent = False
        if batch_independent:
            try:
                self.set_batch_independent(True)
            except DgsError:
                self.close()
                raise

    def set_batch_independent(self, on: bool = True):
        """Registration.set_batch_independent on every member: a candidate's record is the same whichever member registers it,
        and whatever the number of members."""
        self._check(self._lib.dgs_group_set_batch_independent(self._g, 1 if on else 0))
        self._batch_independent = bool(on)

    @property
    def batch_independent(self) -> bool:
        return self._batch_independent

    @batch_independent.setter
    def batch_independent(self, on: bool):
        self.set_batch_independent(on)

    def close(self):
        if getattr(self, "_g", None) is not None and self._g.value:
            self._lib.dgs_group_destroy(self._g)
            self._g = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc: int):
        if rc:
            raise DgsError(rc, (self._lib.dgs_group_last_error(self._g) or b"").decode())

    # -- pcl::IterativeClosestPoint setters (ICP_HIP), applied to every member ----------------------------------------------
    def _set_icp(self, field, value):
        if self.method != "ICP_HIP":
            raise NotImplementedError(f"{field} is an ICP_HIP setting")
        setattr(self.icp_options, field, value)
        self._check(self._lib.dgs_group_set_icp_options(self._g, C.byref(self.icp_options)))

    def setUseReciprocalCorrespondences(self, on: bool):   # ICP_HIP: reciprocal mode; GICP_HIP: accepted, without effect (as upstream)
        if self.method in _PG_METHODS:
            self._set_pg("use_reciprocal_correspondences", 1 if on else 0)
        else:
            self._set_icp("use_reciprocal_correspondences", 1 if on else 0)

    def setEuclideanFitnessEpsilon(self, eps: float):
        self._set_icp("euclidean_fitness_epsilon", float(eps))

    def setTransformationRotationEpsilon(self, eps: float):
        self._set_icp("rotation_epsilon", float(eps))

    # -- pcl::GeneralizedIterativeClosestPoint setters (GICP_HIP / GICP_OMP_HIP), applied to every member ---------------------------------
    def _set_pg(self, field, value):
        if self.method not in _PG_METHODS:
            raise NotImplementedError(f"{field} is a GICP_HIP setting")
        setattr(self.pcl_gicp_options, field, value)
        self._check(self._lib.dgs_group_set_pcl_gicp_options(self._g, C.byref(self.pcl_gicp_options)))

    def setMaximumOptimizerIterations(self, n: int):
        self._set_pg("max_optimizer_iterations", int(n))

    def setRotationEpsilon(self, eps: float):
        self._set_pg("rotation_epsilon", float(eps))

    @property
    def uses_rccl(self) -> bool:
        return bool(self._lib.dgs_group_uses_rccl(self._g))

    @property
    def rccl_ranks(self) -> int:
        """ncclCommCount of the group's communicator (0 without RCCL)."""
        return int(self._lib.dgs_group_rccl_ranks(self._g))

    @property
    def last_gather_used_rccl(self) -> bool:
        return bool(self._lib.dgs_group_last_gather_used_rccl(self._g))

    def member(self, k: int) -> "Registration":
        """Member k's handle as a (borrowed) Registration: measurement hooks (profile_*, counts) of one device of the group."""
        h = self._lib.dgs_group_member(self._g, int(k))
        if not h:
            raise IndexError(k)
        return Registration(self.method, _borrow=h)

    def make_cloud(self, cloud, owner=None) -> GroupCloud:
        return GroupCloud(self, cloud, owner)

    def setInputTarget(self, cloud):
        if isinstance(cloud, GroupCloud):
            self._keep_target = cloud
            self._check(self._lib.dgs_group_set_input_target_cloud(self._g, cloud._c))
            return
        ptr, n, dev, keep = _cloud_ptr(cloud)
        if dev:
            raise ValueError("a group takes host clouds (KeyFrame::cloud) or GroupCloud objects; each member holds its own copy")
        self._check(self._lib.dgs_group_set_input_target(self._g, ptr, n))

    def _raw(self, sources, guesses, compute_fitness, fitness_max_range):
        n = len(sources)
        g = gp = None
        if guesses is not None:
            ga = np.asarray(guesses, dtype=np.float32)
            g = np.ascontiguousarray(ga.transpose(0, 2, 1).reshape(n, 16)) if ga.ndim == 3 else np.ascontiguousarray(np.stack([_col16(G) for G in guesses]))
            gp = g.ctypes.data_as(C.c_void_p)
        temps = []
        if n and any(isinstance(s_, GroupCloud) for s_ in sources) and not all(isinstance(s_, GroupCloud) for s_ in sources):
            # a mixed list (a keyframe without an id among cached ones): the raw clouds are uploaded for this call, candidate c to member c mod G
            sources = list(sources)
            for i, s_ in enumerate(sources):
                if not isinstance(s_, GroupCloud):
                    sources[i] = GroupCloud(self, s_, owner=i)
                    temps.append(sources[i])
        if n and all(isinstance(s_, GroupCloud) for s_ in sources):   # resident keyframes: nothing is uploaded
            cl = (C.c_void_p * n)(*[s_._c.value for s_ in sources])
            res = (L.Result * n)()
            bi = C.c_int32(-1)
            bs = C.c_double(0)
            try:
                self._check(self._lib.dgs_group_align_batch_clouds(self._g, n, cl, gp, 1 if compute_fitness else 0, fitness_max_range, res, C.byref(bi), C.byref(bs)))
            finally:
                for t in temps:
                    t.close()
            self.best_index, self.best_score = bi.value, bs.value
            return res
        ptrs = (C.c_void_p * n)()
        sizes = (C.c_int64 * n)()
        keep = []
        for i, s_ in enumerate(sources):
            ptr, m, dev, k = _cloud_ptr(s_)
            if dev:
                raise ValueError("a group takes host clouds")
            ptrs[i] = ptr.value if ptr.value else 0
            sizes[i] = m
            keep.append(k)
        res = (L.Result * n)()
        bi = C.c_int32(-1)
        bs = C.c_double(0)
        self._check(self._lib.dgs_group_align_batch(self._g, n, ptrs, sizes, gp, 1 if compute_fitness else 0, fitness_max_range, res, C.byref(bi), C.byref(bs)))
        self.best_index, self.best_score = bi.value, bs.value
        return res

    def align_batch(self, sources, guesses=None, compute_fitness: bool = True, fitness_max_range: float = 1.7976931348623157e308):
        if len(sources) == 0:
            return []
        res = self._raw(sources, guesses, compute_fitness, fitness_max_range)
        return [dict(T=_from_col16(r.final_transformation), converged=bool(r.converged), iterations=r.iterations, evaluations=r.evaluations,
                     status=r.status, score=r.score, fitness=r.fitness) for r in res]

    def align_batch_records(self, sources, guesses=None, compute_fitness: bool = True, fitness_max_range: float = 1.7976931348623157e308):
        n = len(sources)
        out = np.full((n, 20), -1.0, dtype=np.float64)
        if n == 0:
            return out
        res = self._raw(sources, guesses, compute_fitness, fitness_max_range)
        a = np.frombuffer(res, dtype=_RESULT_DTYPE, count=n)
        out[:, 1] = a["converged"] != 0
        out[:, 2] = a["fitness"]
        out[:, 3] = a["status"]
        out[:, 4:20] = a["T"].reshape(n, 4, 4).transpose(0, 2, 1).reshape(n, 16)
        return out


    def align_pairs(self, *args, **kwargs):
        raise NotImplementedError("align_pairs (per-pair targets) is served by a single-device Registration; the multi-GPU forms are not built")

    align_pairs_records = align_pairs


def select_registration_method(params: dict | None = None, device: int | None = None) -> Registration:
    """Mirror of hdl_graph_slam::select_registration_method (registrations.cpp:22-124) for the HIP back-ends.

    `params` plays the role of the private NodeHandle: keys are the reference's rosparam names
    (registration_method, reg_num_threads, reg_transformation_epsilon, reg_maximum_iterations,
    reg_max_correspondence_distance, reg_correspondence_randomness, reg_resolution, reg_nn_search_method).
    "NDT_HIP" selects the HIP NDT; "ICP_HIP" the HIP pcl::IterativeClosestPoint (:59-64, + reg_use_reciprocal_correspondences); "GICP_HIP" / "GICP_OMP_HIP" the HIP
    pcl::GeneralizedIterativeClosestPoint (:65-87, + reg_max_optimizer_iterations); "FAST_GICP_HIP" / "FAST_GICP" select GICP (:27-36); "FAST_VGICP_HIP" / "FAST_VGICP" the voxelised
    GICP (:48-56).  Every other name goes through the reference's own chain of tests, in its order: "ICP" (:59-64) and any name
    containing "GICP" (:66-87: pcl::GICP, or pclomp::GICP when it also contains "OMP") are different algorithms -> NotImplementedError;
    what is left is the NDT branch (:88-123): a name without "NDT" warns "unknown registration type ... use NDT" (:89-92), and then
    a name without "OMP" -- plain "NDT" as well as an unknown name such as "FOO" -- is pcl::NormalDistributionsTransform (:94-100),
    another algorithm -> NotImplementedError, while a name containing "OMP" ("NDT_OMP", and e.g. "FOO_OMP" after the warning) is
    pclomp::NormalDistributionsTransform (:101-120), which this library serves.  "PCL_NDT_HIP" (tested before that chain) is the HIP
    pcl::NormalDistributionsTransform of :94-100 with its three rosparams: reg_resolution, reg_transformation_epsilon, reg_maximum_iterations.
    dgs_batch_independent (default false; not a key of the reference) turns on Registration.set_batch_independent.
    """
    pr = dict(params or {})
    reg = _select_registration_method(pr, device)
    if bool(pr.get("dgs_batch_independent", False)):   # this library's own key: batch-independent results (Registration.set_batch_independent)
        try:
            reg.set_batch_independent(True)
        except DgsError:
            reg.close()
            raise
    return reg


def _select_registration_method(pr: dict, device) -> Registration:
    method = pr.get("registration_method", "NDT_OMP")
    common = dict(num_threads=int(pr.get("reg_num_threads", 0)),
                  transformation_epsilon=float(pr.get("reg_transformation_epsilon", 0.01)),
                  maximum_iterations=int(pr.get("reg_maximum_iterations", 64)))
    if method in ("FAST_GICP", "FAST_GICP_HIP"):
        return Registration("FAST_GICP", device=device,
                            gicp_max_correspondence_distance=float(pr.get("reg_max_correspondence_distance", 2.5)),
                            gicp_correspondence_randomness=int(pr.get("reg_correspondence_randomness", 20)), **common)
    if method in ("FAST_VGICP", "FAST_VGICP_HIP"):      # registrations.cpp:48-56
        return Registration("FAST_VGICP", device=device, vgicp_resolution=float(pr.get("reg_resolution", 1.0)),
                            gicp_correspondence_randomness=int(pr.get("reg_correspondence_randomness", 20)), **common)
    if method == "ICP_HIP":                             # :59-64 on the GPU: pcl::IterativeClosestPoint (before the "GICP" test below)
        return Registration("ICP_HIP", device=device,
                            gicp_max_correspondence_distance=float(pr.get("reg_max_correspondence_distance", 2.5)),
                            icp_use_reciprocal_correspondences=bool(pr.get("reg_use_reciprocal_correspondences", False)), **common)
    if method in ("GICP_HIP", "GICP_OMP_HIP"):         # :65-87 on the GPU: pcl::GeneralizedIterativeClosestPoint (before the "GICP" test)
        return Registration(method, device=device,
                            gicp_max_correspondence_distance=float(pr.get("reg_max_correspondence_distance", 2.5)),
                            gicp_correspondence_randomness=int(pr.get("reg_correspondence_randomness", 20)),
                            gicp_max_optimizer_iterations=int(pr.get("reg_max_optimizer_iterations", 20)),
                            gicp_use_reciprocal_correspondences=bool(pr.get("reg_use_reciprocal_correspondences", False)), **common)
    if method == "PCL_NDT_HIP":                         # :94-100 on the GPU: pcl::NormalDistributionsTransform, its three rosparams (before the reference's chain)
        return Registration("PCL_NDT_HIP", device=device, ndt_resolution=float(pr.get("reg_resolution", 0.5)),
                            transformation_epsilon=float(pr.get("reg_transformation_epsilon", 0.01)),
                            maximum_iterations=int(pr.get("reg_maximum_iterations", 64)))
    if method == "ICP" or "GICP" in method:             # :59-64, :66-87 (FAST_VGICP_CUDA lands here too when the reference is built without CUDA)
        raise NotImplementedError(f"registration_method {method!r} is served by the reference's own factory branch, not by the HIP back-ends")
    if method != "NDT_HIP":
        if "NDT" not in method:                         # :89-92
            import sys
            print(f"warning: unknown registration type({method})\n       : use NDT", file=sys.stderr)
        if "OMP" not in method:                         # :94-100 pcl::NormalDistributionsTransform
            raise NotImplementedError(f"registration_method {method!r} selects pcl::NormalDistributionsTransform in the reference "
                                      "(registrations.cpp:94-100), a different algorithm from NDT_OMP: not served by the HIP back-ends")
    nn = pr.get("reg_nn_search_method", "DIRECT7")
    search = L.NDT_SEARCH["KDTREE"] if nn == "KDTREE" else L.NDT_SEARCH["DIRECT1"] if nn == "DIRECT1" else L.NDT_SEARCH["DIRECT7"]
    return Registration("NDT_OMP", device=device, ndt_resolution=float(pr.get("reg_resolution", 0.5)), ndt_search_method=search, **common)
