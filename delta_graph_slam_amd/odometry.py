"""Frame-to-keyframe scan-matching odometry: the call sequence of ScanMatchingOdometryNodelet::matching over the HIP
registration, without the ROS shell.

Mirrors /root/reference/apps/scan_matching_odometry_nodelet.cpp:
  initialize_params   :64-106   keyframe_delta_trans / _angle / _time, transform_thresholding, max_acceptable_*
  matching            :173-270  first frame -> keyframe + setInputTarget; else setInputSource, align(prev_trans * msf_delta),
                                reject on !hasConverged (:222-226) or implausible jump (:231-241), keyframe switch (:249-260)
  publish_scan_matching_status :309-346  matching_error = getFitnessScore(), inlier_fraction (d^2 < 0.25)
Down-sampling (:83-103,155-165): VOXELGRID runs on the device (pcl::VoxelGrid centroid filter) so a raw scan
uploaded once stays in HBM through align; APPROX_VOXELGRID (pcl::ApproximateVoxelGrid, :90-96) likewise; NONE passes the cloud through.

The frame loop is inherently sequential (frame t's guess is frame t-1's result), so ONE stream does not shard ("replicas only" across
GPUs).  Several robots or bags share one card through the fleet:

ScanMatchingOdometryFleet advances several independent streams by one frame each in one chain of device calls: the
frames are down-sampled into resident clouds together, registered together as pairs that each name their own keyframe, and the
host decisions of `matching` (matching_decision, shared with ScanMatchingOdometry) are taken per stream.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Any, Optional

import numpy as np

__all__ = ["ScanMatchingOdometry", "ScanMatchingOdometryFleet", "ScanMatchingStatus", "matching_decision"]


@dataclass
class ScanMatchingStatus:
    """msg/ScanMatchingStatus.msg:1-8 (the fields the registration feeds)"""
    has_converged: bool
    matching_error: float
    inlier_fraction: float
    relative_pose: np.ndarray


def _quat_w(R: np.ndarray) -> float:
    """w of Eigen::Quaternionf(R) (positive branch used for small rotations; general Shepperd form)."""
    t = float(np.trace(R))
    if t > 0:
        return 0.5 * float(np.sqrt(t + 1.0))
    i = int(np.argmax(np.diag(R)))
    j, k = (i + 1) % 3, (i + 2) % 3
    s = float(np.sqrt(R[i, i] - R[j, j] - R[k, k] + 1.0))
    return float((R[k, j] - R[j, k]) * 0.5 / s)


def _read_thresholds(s, pr: dict):
    """initialize_params (:64-106): the keyframe and plausibility thresholds of one stream, onto `s`"""
    s.keyframe_delta_trans = float(pr.get("keyframe_delta_trans", 0.25))
    s.keyframe_delta_angle = float(pr.get("keyframe_delta_angle", 0.15))
    s.keyframe_delta_time = float(pr.get("keyframe_delta_time", 1.0))
    s.transform_thresholding = bool(pr.get("transform_thresholding", False))
    s.max_acceptable_trans = float(pr.get("max_acceptable_trans", 1.0))
    s.max_acceptable_angle = float(pr.get("max_acceptable_angle", 1.0))


def _first_frame(s, stamp: float):
    """matching :174-183: the pose state of a stream whose first frame becomes its keyframe"""
    s.prev_time = None
    s.prev_trans = np.eye(4, dtype=np.float32)
    s.keyframe_pose = np.eye(4, dtype=np.float32)
    s.keyframe_stamp = stamp


def matching_decision(s, stamp: float, converged: bool, trans: np.ndarray, on_keyframe_switch) -> np.ndarray:
    """The host decisions of matching (:222-260) for one registered frame of one stream.  `s` carries the stream's thresholds and pose
    state (keyframe_pose, keyframe_stamp, prev_time, prev_trans, n_keyframes) and is updated; `trans` is the registration's final
    transformation; on_keyframe_switch() is called where the frame becomes the new keyframe.  -> odom (4x4 float32)."""
    if not converged:
        return (s.keyframe_pose @ s.prev_trans).astype(np.float32)       # "ignore this frame"

    odom = (s.keyframe_pose @ trans).astype(np.float32)

    if s.transform_thresholding:
        d = np.linalg.inv(s.prev_trans) @ trans
        dx = float(np.linalg.norm(d[:3, 3]))
        da = float(np.arccos(np.clip(_quat_w(d[:3, :3]), -1.0, 1.0)))
        if dx > s.max_acceptable_trans or da > s.max_acceptable_angle:
            return (s.keyframe_pose @ s.prev_trans).astype(np.float32)   # "too large transform"

    s.prev_time = stamp
    s.prev_trans = trans

    delta_trans = float(np.linalg.norm(trans[:3, 3]))
    delta_angle = float(np.arccos(np.clip(_quat_w(trans[:3, :3]), -1.0, 1.0)))
    delta_time = stamp - s.keyframe_stamp
    if delta_trans > s.keyframe_delta_trans or delta_angle > s.keyframe_delta_angle or delta_time > s.keyframe_delta_time:
        on_keyframe_switch()
        s.keyframe_pose = odom
        s.keyframe_stamp = stamp
        s.prev_time = stamp
        s.prev_trans = np.eye(4, dtype=np.float32)
        s.n_keyframes += 1
    return odom


class ScanMatchingOdometry:
    def __init__(self, registration=None, params: Optional[dict] = None, device: Optional[int] = None):
        pr = dict(params or {})
        _read_thresholds(self, pr)
        # the reference defaults to VOXELGRID 0.1 m (:83-84); the mirror defaults to NONE so callers that already filtered are not
        # filtered twice -- pass downsample_method explicitly to reproduce the nodelet
        self.downsample_method = str(pr.get("downsample_method", "NONE"))
        self.downsample_resolution = float(pr.get("downsample_resolution", 0.1))
        if registration is None:
            from .registration import select_registration_method
            registration = select_registration_method(pr, device=device)
        self.registration = registration
        self.keyframe: Any = None
        self.keyframe_pose = np.eye(4, dtype=np.float32)
        self.keyframe_stamp = 0.0
        self.prev_time: Optional[float] = None
        self.prev_trans = np.eye(4, dtype=np.float32)
        self.last_status: Optional[ScanMatchingStatus] = None
        self.n_keyframes = 0

    def downsample(self, cloud):
        """scan_matching_odometry_nodelet.cpp:155-165"""
        if self.downsample_method == "VOXELGRID":
            return self.registration.voxel_grid_filter(cloud, self.downsample_resolution)
        if self.downsample_method == "APPROX_VOXELGRID":
            return self.registration.voxel_grid_filter(cloud, self.downsample_resolution, approximate=True)
        return cloud

    def matching(self, stamp: float, cloud, msf_delta: Optional[np.ndarray] = None, want_status: bool = False) -> np.ndarray:
        """Returns odom (4x4 float32): the pose of this frame in the odometry frame."""
        reg = self.registration
        if self.keyframe is None:
            _first_frame(self, stamp)
            self.keyframe = self.downsample(cloud)
            reg.setInputTarget(self.keyframe)
            self.n_keyframes = 1
            return np.eye(4, dtype=np.float32)

        filtered = self.downsample(cloud)
        reg.setInputSource(filtered)
        delta = np.eye(4, dtype=np.float32) if msf_delta is None else np.asarray(msf_delta, np.float32)
        reg.align((self.prev_trans @ delta).astype(np.float32))

        if want_status:  # publish_scan_matching_status, only when someone listens (:310)
            self.last_status = ScanMatchingStatus(reg.hasConverged(), reg.getFitnessScore(), reg.getInlierFraction(0.5 * 0.5),
                                                  reg.getFinalTransformation())

        def switch():
            self.keyframe = filtered
            reg.setInputTarget(filtered)

        return matching_decision(self, stamp, reg.hasConverged(), reg.getFinalTransformation(), switch)


_PAIR_METHODS = ("FAST_GICP", "FAST_GICP_HIP", "GICP_HIP", "GICP_OMP_HIP")   # the methods Registration.align_pairs serves


class _Stream:
    """One stream of the fleet: its thresholds and pose state (what matching_decision reads and writes) and its two resident clouds."""

    def __init__(self, registration, pr: dict):
        _read_thresholds(self, pr)
        self.key = registration.make_cloud(np.zeros((0, 4), np.float32))     # the keyframe
        self.frame = registration.make_cloud(np.zeros((0, 4), np.float32))   # the frame being registered
        self.has_keyframe = False
        self.keyframe_pose = np.eye(4, dtype=np.float32)
        self.keyframe_stamp = 0.0
        self.prev_time: Optional[float] = None
        self.prev_trans = np.eye(4, dtype=np.float32)
        self.n_keyframes = 0
        self.odom = np.eye(4, dtype=np.float32)
        self.last_status: Optional[ScanMatchingStatus] = None

    def swap(self):
        self.key, self.frame = self.frame, self.key


class ScanMatchingOdometryFleet:
    """n_streams independent ScanMatchingOdometry streams advanced together: one step() takes one frame per stream and costs one batched
    down-sampling, one align_pairs and (with want_status) one batched inlier count, whatever n_streams is.  Every stream owns two resident
    clouds, keyframe and frame; at a keyframe switch they are swapped, so the new keyframe keeps the index and covariances it made as a
    source.  `params`: one dict, or one per stream (the keyframe and plausibility thresholds are read per stream; downsample_method /
    downsample_resolution and the registration come from the first).  With n_streams > 1 the registration must be one align_pairs serves
    (FAST_GICP, GICP_HIP / GICP_OMP_HIP); a single stream is served for every method through the registration's own target and source.
    With a batch_independent FAST_GICP registration, and with GICP_HIP as it is, every stream's odometry is bitwise what a
    ScanMatchingOdometry over that stream alone returns."""

    def __init__(self, registration=None, n_streams: int = 1, params=None, device: Optional[int] = None):
        n_streams = int(n_streams)
        if n_streams < 1:
            raise ValueError("n_streams must be at least 1")
        if isinstance(params, (list, tuple)):
            if len(params) != n_streams:
                raise ValueError("one params dict per stream, or one for all")
            prs = [dict(p or {}) for p in params]
        else:
            prs = [dict(params or {}) for _ in range(n_streams)]
        self.downsample_method = str(prs[0].get("downsample_method", "NONE"))
        self.downsample_resolution = float(prs[0].get("downsample_resolution", 0.1))
        if registration is None:
            from .registration import select_registration_method
            registration = select_registration_method(prs[0], device=device)
        if n_streams > 1 and registration.method not in _PAIR_METHODS:
            raise NotImplementedError(f"ScanMatchingOdometryFleet with {n_streams} streams needs a registration that align_pairs serves "
                                      f"({', '.join(_PAIR_METHODS)}); this one is {registration.method} (one stream is served for every method)")
        self.registration = registration
        self.n_streams = n_streams
        self.streams = [_Stream(registration, pr) for pr in prs]
        self._target = None   # one stream: the cloud the registration holds as its target

    @property
    def n_keyframes(self):
        return [s.n_keyframes for s in self.streams]

    @property
    def last_status(self):
        return [s.last_status for s in self.streams]

    def step(self, stamps, clouds, msf_deltas=None, want_status: bool = False) -> np.ndarray:
        """One frame per stream: clouds[i] (None: stream i is not touched) stamped stamps[i], with the optional motion prior
        msf_deltas[i].  -> [n_streams, 4, 4] float32, row i the odometry of stream i's frame (its last one for an untouched stream)."""
        reg = self.registration
        if len(clouds) != self.n_streams or len(stamps) != self.n_streams or (msf_deltas is not None and len(msf_deltas) != self.n_streams):
            raise ValueError("one stamp, cloud and delta per stream")
        live = [i for i in range(self.n_streams) if clouds[i] is not None]
        if live:
            # 1. every live frame into its stream's frame cloud
            reg.assign_batch([self.streams[i].frame for i in live], [clouds[i] for i in live], self.downsample_method, self.downsample_resolution)
        # 2. first frames become keyframes
        rest = []
        for i in live:
            s = self.streams[i]
            if not s.has_keyframe:
                s.swap()
                s.has_keyframe = True
                _first_frame(s, stamps[i])
                s.n_keyframes = 1
                s.odom = np.eye(4, dtype=np.float32)
            else:
                rest.append(i)
        if rest:
            guesses = []
            for i in rest:
                s = self.streams[i]
                delta = np.eye(4, dtype=np.float32) if msf_deltas is None or msf_deltas[i] is None else np.asarray(msf_deltas[i], np.float32)
                guesses.append((s.prev_trans @ delta).astype(np.float32))
            # 3. / 4. one registration of all pairs (keyframe i, frame i), the status figures with it
            if self.n_streams == 1:
                conv, trans, fit, inl = self._register_one(self.streams[0], guesses[0], want_status)
            else:
                keys, frames = [self.streams[i].key for i in rest], [self.streams[i].frame for i in rest]
                rec = reg.align_pairs_records(keys, frames, np.stack(guesses), compute_fitness=want_status)
                conv = [bool(r[1] != 0.0) for r in rec]
                trans = [r[4:20].reshape(4, 4).astype(np.float32) for r in rec]   # float32 values carried in float64: exact
                fit = rec[:, 2]
                inl = reg.calc_inlier_fraction_batch(keys, frames, trans, 0.5 * 0.5) if want_status else None
            # 5. / 6. the decisions of matching per stream; a switch swaps the stream's two clouds
            for k, i in enumerate(rest):
                s = self.streams[i]
                if want_status:   # publish_scan_matching_status, only when someone listens (:310)
                    s.last_status = ScanMatchingStatus(conv[k], float(fit[k]), float(inl[k]), trans[k].copy())
                s.odom = matching_decision(s, stamps[i], conv[k], trans[k], s.swap)
            if self.n_streams == 1 and self._target is not self.streams[0].key:
                self._set_target(self.streams[0])
        elif live and self.n_streams == 1:
            self._set_target(self.streams[0])
        return np.stack([s.odom for s in self.streams])

    # -- one stream: every method, through the registration's own target and source ---------------------------------------------
    def _set_target(self, s):
        self.registration.setInputTarget(s.key)
        self._target = s.key

    def _register_one(self, s, guess, want_status):
        reg = self.registration
        reg.setInputSource(s.frame)   # bound again every frame: refilling a cloud detaches whoever borrowed it
        reg.align(guess)
        fit = inl = [float("nan")]
        if want_status:
            fit, inl = [reg.getFitnessScore()], [reg.getInlierFraction(0.5 * 0.5)]
        return [reg.hasConverged()], [reg.getFinalTransformation()], fit, inl
