"""FloorDetectionNodelet::detect on the device (upstream apps/floor_detection_nodelet.cpp:110-238; dgs_floor_detection in
include/dgs_reg.h).

`FloorDetector(params)` takes the nodelet's seven parameter names (:57-63) with its defaults, plus the RANSAC's and the recalled-detail
switches of dgs_floor_detection_params.  `detect(cloud)` takes /filtered_points as float32 [N,4], a numpy array or a device tensor --
what `Prefilter.filter_scan` returns as its 3-D output goes in without a copy -- and returns the four plane coefficients, or None where
upstream returns boost::none (`.status` says why).  Like the Prefilter, a detector may share a Registration's handle: it works in
buffers of its own, so the registration's target, source and results, the prefilter's scratch, the map and the line code's state are
untouched.

`detect_batch(clouds)` runs detect over many scans -- the frames of several streams -- in one device call (dgs_floor_detection_batch):
scan i receives the bits detect gives it alone, `.statuses[i]` says why a scan has no floor, and `batch_filtered(i)`,
`batch_inliers(i)`, `batch_trace(i)`, `batch_clipped(i)` read scan i of the last batch.  The 3-D outputs of
`Prefilter.filter_scan_batch` go in as they are.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np

from . import _lib as L
from .registration import Registration, _cloud_ptr

__all__ = ["FloorDetector", "params_from_dict", "tilt_matrices"]

_NODELET = ("tilt_deg", "sensor_height", "height_clip_range", "floor_pts_thresh", "floor_normal_thresh", "use_normal_filtering",
            "normal_filter_thresh")
_EXTRA = ("distance_threshold", "max_iterations", "probability", "max_sample_checks", "transform_order", "plane_dot_order", "hyp_chunk_first",
          "hyp_chunk")


def params_from_dict(params: Optional[dict] = None) -> L.FloorDetectionParams:
    """The nodelet's defaults (:57-63) and PCL's (RandomSampleConsensus, SampleConsensusModel) overridden by `params`."""
    p = L.FloorDetectionParams()
    rc = L.load().dgs_floor_detection_params_init(C.byref(p))
    if rc:
        raise L.DgsError(rc, "dgs_floor_detection_params_init")
    kinds = dict(p._fields_)
    for k, v in dict(params or {}).items():
        if k not in _NODELET and k not in _EXTRA:
            raise KeyError(f"unknown floor detection parameter {k!r}")
        setattr(p, k, float(v) if kinds[k] is C.c_double else int(v))
    return p


def tilt_matrices(tilt_deg: float):
    """-> (tilt, tilt_inv) float32 [4,4]: Eigen::AngleAxisf((float)(tilt_deg * M_PI / 180.0f), UnitY).toRotationMatrix() in the top left
    corner of an identity (:112-113), and its float32 numpy.linalg.inv.  Both are the exact identity for tilt_deg = 0."""
    F = np.float32
    angle = F(float(tilt_deg) * np.pi / float(F(180.0)))
    s, c = F(np.sin(angle)), F(np.cos(angle))
    one_c = F(F(1) - c)
    t = np.eye(4, dtype=F)
    t[0, 0] = F(F(0) + c)
    t[1, 1] = F(F(one_c * F(1)) + c)
    t[2, 2] = F(F(0) + c)
    t[0, 2] = F(F(0) + s)
    t[2, 0] = F(F(0) - s)
    inv = np.linalg.inv(t).astype(F)
    return t, inv


class FloorDetector:
    def __init__(self, params: Optional[dict] = None, registration: Optional[Registration] = None, device: Optional[int] = None):
        self.params = params_from_dict(params)
        if registration is None:
            registration = Registration("NDT_OMP", device=device)   # any handle: only its stream and the detector's own buffers are used
        self.registration = registration
        self._lib = registration._lib
        self.status = "TOO_FEW_POINTS"       # L.FD_STATUS of the last detect
        self.statuses = []                   # L.FD_STATUS per scan of the last detect_batch

    @property
    def _h(self):
        return self.registration._h

    def detect(self, cloud, rng_raw=None, tilt=None, tilt_inv=None) -> Optional[np.ndarray]:
        """rng_raw: optional uint32 values that stand in for boost::mt19937(12345)() >> 1, three per draw.  tilt / tilt_inv: the two
        4 x 4 matrices of detect(); by default tilt_matrices(params.tilt_deg)."""
        ptr, n, dev, keep = _cloud_ptr(cloud)
        t16, ti16 = self._tilts(tilt, tilt_inv)
        raw = None if rng_raw is None else np.ascontiguousarray(rng_raw, dtype=np.uint32)
        coeffs = np.zeros(4, np.float32)
        st = C.c_int32(0)
        self.registration._check(self._lib.dgs_floor_detection(
            self._h, C.byref(self.params), t16.ctypes.data_as(C.c_void_p), ti16.ctypes.data_as(C.c_void_p), ptr, n, dev,
            None if raw is None else raw.ctypes.data_as(C.c_void_p), 0 if raw is None else raw.size, coeffs.ctypes.data_as(C.c_void_p), C.byref(st)))
        self.status = L.FD_STATUS[st.value]
        return coeffs if self.status == "DETECTED" else None

    def _tilts(self, tilt, tilt_inv):
        if tilt is None or tilt_inv is None:
            t, ti = tilt_matrices(self.params.tilt_deg)
            tilt = t if tilt is None else tilt
            tilt_inv = ti if tilt_inv is None else tilt_inv
        return (np.ascontiguousarray(np.asarray(tilt, np.float32).T.reshape(16)),      # column-major
                np.ascontiguousarray(np.asarray(tilt_inv, np.float32).T.reshape(16)))

    def detect_batch(self, clouds, rng_raws=None, tilt=None, tilt_inv=None):
        """detect over many scans in one device call.  clouds: all numpy arrays or all device tensors, float32 [N_i,4].  rng_raws: one
        entry per scan (None entries allowed: mt19937(12345)), or None for all.  One parameter set and one tilt / tilt_inv pair serve
        every scan.  -> [coefficients float32 [4], or None where upstream returns boost::none] per scan; `.statuses` says why."""
        clouds = list(clouds)
        n = len(clouds)
        raws = list(rng_raws) if rng_raws is not None else [None] * n
        if len(raws) != n:
            raise ValueError("rng_raws needs one entry per scan")
        if n and any(_is_device(c) != _is_device(clouds[0]) for c in clouds):
            raise ValueError("detect_batch takes all numpy arrays or all device tensors")
        t16, ti16 = self._tilts(tilt, tilt_inv)
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        if n == 0:
            self.registration._check(self._lib.dgs_floor_detection_batch(self._h, C.byref(self.params), vp(t16), vp(ti16), 0, None, None, 0, None, None, None, None))
            self.statuses = []
            return []
        dev = _is_device(clouds[0])
        ptrs = [_cloud_ptr(c, sync=False) for c in clouds]
        if dev:
            import torch
            torch.cuda.current_stream(clouds[0].device).synchronize()   # once for the whole batch
        sizes = np.array([q[1] for q in ptrs], np.int64)
        in_p = (C.c_void_p * n)(*[q[0] for q in ptrs])
        raws = [None if r is None else np.ascontiguousarray(r, dtype=np.uint32) for r in raws]
        raw_p = (C.c_void_p * n)(*[None if r is None or r.size == 0 else r.ctypes.data for r in raws])
        raw_n = np.array([0 if r is None else r.size for r in raws], np.int64)
        coeffs = np.zeros((n, 4), np.float32)
        st = np.zeros(n, np.int32)
        self.registration._check(self._lib.dgs_floor_detection_batch(self._h, C.byref(self.params), vp(t16), vp(ti16), n, in_p, vp(sizes), 1 if dev else 0,
                                                                     raw_p, vp(raw_n), vp(coeffs), vp(st)))
        self.statuses = [L.FD_STATUS[int(v)] for v in st]
        return [coeffs[i].copy() if self.statuses[i] == "DETECTED" else None for i in range(n)]

    def batch_filtered(self, i: int, device_like=None):
        """The filtered cloud of scan i of the last detect_batch: float32 [m,4]; a device tensor when `device_like` is one."""
        n = C.c_int64(0)
        self.registration._check(self._lib.dgs_floor_detection_batch_get_filtered(self._h, i, None, 0, 0, C.byref(n)))
        if device_like is not None and getattr(device_like, "is_cuda", False):
            import torch
            out = torch.empty((n.value, 4), dtype=torch.float32, device=device_like.device)
            if n.value:
                self.registration._check(self._lib.dgs_floor_detection_batch_get_filtered(self._h, i, C.c_void_p(out.data_ptr()), n.value, 1, C.byref(n)))
            return out
        out = np.empty((n.value, 4), np.float32)
        if n.value:
            self.registration._check(self._lib.dgs_floor_detection_batch_get_filtered(self._h, i, out.ctypes.data_as(C.c_void_p), n.value, 0, C.byref(n)))
        return out

    def batch_inliers(self, i: int):
        """-> (indices into scan i's filtered cloud int32 [m] ascending, the points float32 [m,4]); computed when asked for."""
        n = C.c_int64(0)
        self.registration._check(self._lib.dgs_floor_detection_batch_get_inliers(self._h, i, None, None, 0, C.byref(n)))
        idx, pts = np.empty(n.value, np.int32), np.empty((n.value, 4), np.float32)
        if n.value:
            self.registration._check(self._lib.dgs_floor_detection_batch_get_inliers(self._h, i, idx.ctypes.data_as(C.c_void_p),
                                                                                     pts.ctypes.data_as(C.c_void_p), n.value, C.byref(n)))
        return idx, pts

    def batch_trace(self, i: int) -> dict:
        """trace() of scan i.  hypotheses_scored and chunks_launched say how far that scan's own scoring went in the batch's rounds."""
        t = L.FloorDetectionTrace()
        self.registration._check(self._lib.dgs_floor_detection_batch_get_trace(self._h, i, C.byref(t)))
        return _trace_dict(t)

    def batch_clipped(self, i: int):
        """-> (the clipped cloud float32 [m,4], its normals float32 [m,4] or None without the normal filter) of scan i."""
        n = C.c_int64(0)
        self.registration._check(self._lib.dgs_floor_detection_batch_get_clipped(self._h, i, None, None, 0, C.byref(n)))
        c = np.empty((n.value, 4), np.float32)
        nv = np.full((n.value, 4), np.nan, np.float32) if self.params.use_normal_filtering else None
        if n.value:
            self.registration._check(self._lib.dgs_floor_detection_batch_get_clipped(
                self._h, i, c.ctypes.data_as(C.c_void_p), None if nv is None else nv.ctypes.data_as(C.c_void_p), n.value, C.byref(n)))
        return c, nv

    def batch_counts(self) -> np.ndarray:
        """counts8 of the last detect_batch: [0] kernel launches, [1] host waits, [2] scans listed, [3] scans that reached the RANSAC,
        [4] scans served by a per-scan fallback, [5] chunks, [6] indices built, [7] RANSAC rounds."""
        c = np.zeros(8, np.int64)
        self.registration._check(self._lib.dgs_floor_detection_batch_get_counts(self._h, c.ctypes.data_as(C.c_void_p)))
        return c

    def filtered(self, device_like=None):
        """The filtered cloud of the last detect (/floor_detection/floor_filtered_points): float32 [m,4]; a device tensor when
        `device_like` is one."""
        n = C.c_int64(0)
        self.registration._check(self._lib.dgs_floor_detection_get_filtered(self._h, None, 0, 0, C.byref(n)))
        if device_like is not None and getattr(device_like, "is_cuda", False):
            import torch
            out = torch.empty((n.value, 4), dtype=torch.float32, device=device_like.device)
            if n.value:
                self.registration._check(self._lib.dgs_floor_detection_get_filtered(self._h, C.c_void_p(out.data_ptr()), n.value, 1, C.byref(n)))
            return out
        out = np.empty((n.value, 4), np.float32)
        if n.value:
            self.registration._check(self._lib.dgs_floor_detection_get_filtered(self._h, out.ctypes.data_as(C.c_void_p), n.value, 0, C.byref(n)))
        return out

    def inliers(self):
        """-> (indices into the filtered cloud int32 [m] ascending, the points float32 [m,4]: /floor_detection/floor_points)."""
        n = C.c_int64(0)
        self.registration._check(self._lib.dgs_floor_detection_get_inliers(self._h, None, None, 0, C.byref(n)))
        idx, pts = np.empty(n.value, np.int32), np.empty((n.value, 4), np.float32)
        if n.value:
            self.registration._check(self._lib.dgs_floor_detection_get_inliers(self._h, idx.ctypes.data_as(C.c_void_p), pts.ctypes.data_as(C.c_void_p),
                                                                               n.value, C.byref(n)))
        return idx, pts

    def trace(self) -> dict:
        t = L.FloorDetectionTrace()
        self.registration._check(self._lib.dgs_floor_detection_get_trace(self._h, C.byref(t)))
        return _trace_dict(t)

    # -- test hook -----------------------------------------------------------------------------------------------------------
    def clipped(self):
        """-> (the clipped cloud float32 [m,4], its normals float32 [m,4] or None without the normal filter) of the last detect."""
        n = C.c_int64(0)
        self.registration._check(self._lib.dgs_floor_detection_get_clipped(self._h, None, None, 0, C.byref(n)))
        c = np.empty((n.value, 4), np.float32)
        nv = np.full((n.value, 4), np.nan, np.float32) if self.params.use_normal_filtering else None
        if n.value:
            self.registration._check(self._lib.dgs_floor_detection_get_clipped(
                self._h, c.ctypes.data_as(C.c_void_p), None if nv is None else nv.ctypes.data_as(C.c_void_p), n.value, C.byref(n)))
        return c, nv


def _is_device(x) -> bool:
    return bool(getattr(x, "is_cuda", False))


def _trace_dict(t) -> dict:
    return dict(n_clipped=t.n_clipped, n_filtered=t.n_filtered, draws=t.draws, hypotheses_scored=t.hypotheses_scored, iterations=t.iterations,
                chunks_launched=t.chunks_launched, winner_rank=t.winner_rank, sample=tuple(t.sample[:]), count=t.count,
                ransac_failed=t.ransac_failed, raw_coeffs=np.array(t.raw_coeffs[:], np.float32), dot=np.float32(t.dot))


def host_draws(n: int, n_draws: int, rng_raw=None) -> np.ndarray:
    """The library's draw list builder (host code, no device): int32 [n_draws, 3]."""
    raw = None if rng_raw is None else np.ascontiguousarray(rng_raw, dtype=np.uint32)
    if raw is not None and raw.size < 3 * n_draws:
        raise ValueError("rng_raw holds fewer than three values per draw")
    out = np.zeros((max(n_draws, 1), 3), np.int32)
    rc = L.load().dgs_floor_detection_draws(n, None if raw is None else raw.ctypes.data_as(C.c_void_p), n_draws, out.ctypes.data_as(C.c_void_p))
    if rc:
        raise L.DgsError(rc, "dgs_floor_detection_draws")
    return out[:n_draws]


def host_walk(counts, n: int, max_iterations: int = 1000, probability: float = 0.99):
    """The library's walk over inlier counts (host code, no device) -> (winner, iterations, still open past the counts)."""
    c = np.ascontiguousarray(counts, dtype=np.int32)
    w, it, op = C.c_int32(0), C.c_int32(0), C.c_int32(0)
    rc = L.load().dgs_floor_detection_walk(n, max_iterations, probability, c.ctypes.data_as(C.c_void_p), c.size, C.byref(w), C.byref(it), C.byref(op))
    if rc:
        raise L.DgsError(rc, "dgs_floor_detection_walk")
    return w.value, it.value, bool(op.value)
