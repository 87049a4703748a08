"""-m gpu tests of ScanMatchingOdometryFleet (delta_graph_slam_amd/odometry.py): several scan-matching odometry streams advanced
by one frame each per step.  The streams are cut from one synth.vlp16_stream(n_frames=24) -- the stream itself, the stream reversed, every
second frame, a rigidly moved copy that ends 8 frames early -- with different keyframe thresholds, so they switch keyframes at different
steps.  Frames are down-sampled with VOXELGRID 0.4 m (a few thousand points a frame: the paths are the 0.1 m ones, the test is quick)."""
import json
import os
import struct
import subprocess
import types

import numpy as np
import pytest

from delta_graph_slam_amd import synth
from tests import align_pairs_scenes as S

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEAF = 0.4
DOWN = {"downsample_method": "VOXELGRID", "downsample_resolution": LEAF}
THRESHOLDS = [dict(keyframe_delta_trans=1.0, keyframe_delta_angle=1.0, keyframe_delta_time=1e9),     # the stream: switches by distance, most frames
              dict(keyframe_delta_trans=2.5, keyframe_delta_angle=1.0, keyframe_delta_time=1e9),     # reversed: every second or third frame
              dict(keyframe_delta_trans=1e9, keyframe_delta_angle=1.0, keyframe_delta_time=0.35),    # every second frame: by time, every fourth step
              dict(keyframe_delta_trans=0.25, keyframe_delta_angle=0.15, keyframe_delta_time=1.0)]   # the moved copy: the nodelet's defaults
_CACHE = {}


def streams():
    """-> 4 lists of 24 entries (cloud or None), one stamp list"""
    if "streams" not in _CACHE:
        base, _ = synth.vlp16_stream(n_frames=24)
        moved = synth.make_transform((3.0, -2.0, 0.5), (0.02, -0.01, 0.7))
        second = base[::2] + [None] * 12
        copy = [synth.apply_transform(moved, c) for c in base[:16]] + [None] * 8
        _CACHE["streams"] = ([base, base[::-1], second, copy], [0.1 * k for k in range(24)])
    return _CACHE["streams"]


def _registration(method, **kw):
    from delta_graph_slam_amd.registration import Registration
    if method == "FAST_GICP":
        return Registration("FAST_GICP", gicp_max_correspondence_distance=2.0, transformation_epsilon=0.1, **kw)
    if method == "GICP_HIP":
        return Registration("GICP_HIP", gicp_max_correspondence_distance=2.0, **kw)
    if method == "ICP_HIP":
        return Registration("ICP_HIP", gicp_max_correspondence_distance=2.0, **kw)
    return Registration(method, ndt_resolution=1.0, **kw)


def _solo(method, which, n_frames=24, **kw):
    """ScanMatchingOdometry over each of the streams `which` alone -> per stream a list of (odom, keyframes, status) per step (None: no frame)"""
    from delta_graph_slam_amd.odometry import ScanMatchingOdometry
    key = (method, tuple(which), n_frames, tuple(sorted(kw.items())))
    if key in _CACHE:
        return _CACHE[key]
    clouds, stamps = streams()
    out = []
    for i in which:
        reg = _registration(method, **kw)
        odo = ScanMatchingOdometry(reg, dict(THRESHOLDS[i], **DOWN))
        rows = []
        for k in range(n_frames):
            if clouds[i][k] is None:
                rows.append(None)
                continue
            odom = odo.matching(stamps[k], clouds[i][k], want_status=True)
            rows.append((odom, odo.n_keyframes, odo.last_status if k > 0 else None))
        out.append(rows)
        reg.close()
    _CACHE[key] = out
    return out


def _fleet(method, which, n_frames=24, **kw):
    from delta_graph_slam_amd.odometry import ScanMatchingOdometryFleet
    key = ("fleet", method, tuple(which), n_frames, tuple(sorted(kw.items())))
    if key in _CACHE:
        return _CACHE[key]
    clouds, stamps = streams()
    reg = _registration(method, **kw)
    fleet = ScanMatchingOdometryFleet(reg, len(which), [dict(THRESHOLDS[i], **DOWN) for i in which])
    out = [[] for _ in which]
    last = np.stack([np.eye(4, dtype=np.float32)] * len(which))
    for k in range(n_frames):
        frame = [clouds[i][k] for i in which]
        odoms = fleet.step([stamps[k]] * len(which), frame, want_status=True)
        assert odoms.shape == (len(which), 4, 4) and odoms.dtype == np.float32
        for j, c in enumerate(frame):
            if c is None:
                assert np.array_equal(odoms[j], last[j])   # a stream without a frame is not touched: its row is its last odom
                out[j].append(None)
            else:
                out[j].append((odoms[j].copy(), fleet.n_keyframes[j], fleet.last_status[j] if k > 0 else None))
        last = odoms
    reg.close()
    _CACHE[key] = out
    return out


def _bits(x):
    return np.float64(x).view(np.uint64)


def _same_stream(a, b, what, fitness=True):
    """every frame's odom, keyframe count, inlier fraction (and matching_error) bit for bit"""
    assert len(a) == len(b)
    for k, (x, y) in enumerate(zip(a, b)):
        assert (x is None) == (y is None), (what, k)
        if x is None:
            continue
        assert np.array_equal(x[0], y[0]), (what, k, x[0], y[0])
        assert x[1] == y[1], (what, k, x[1], y[1])
        if x[2] is not None:
            assert x[2].has_converged == y[2].has_converged and np.array_equal(x[2].relative_pose, y[2].relative_pose), (what, k)
            assert _bits(x[2].inlier_fraction) == _bits(y[2].inlier_fraction), (what, k, x[2].inlier_fraction, y[2].inlier_fraction)
            if fitness:
                assert _bits(x[2].matching_error) == _bits(y[2].matching_error), (what, k, x[2].matching_error, y[2].matching_error)


# ------------------------------------------------------------------------------------------------------ (a) bitwise, batch-independent
def test_batch_independent_fast_gicp_fleet_is_bitwise_the_solo_streams():
    solo, fleet = _solo("FAST_GICP", (0, 1, 2, 3), batch_independent=True), _fleet("FAST_GICP", (0, 1, 2, 3), batch_independent=True)
    for i in range(4):
        _same_stream(fleet[i], solo[i], f"stream {i}")
    keyframes = [[r[1] for r in rows if r is not None][-1] for rows in fleet]
    print("keyframes per stream:", keyframes)
    assert len(set(keyframes)) > 1 and min(keyframes) >= 3   # the streams did switch, and not in step


def test_gicp_hip_fleet_is_bitwise_the_solo_streams():
    """GICP_HIP as it is: the pair's sums run over fixed slices, so odometry, keyframes and inlier fractions are the solo bits."""
    solo, fleet = _solo("GICP_HIP", (0, 3), 10), _fleet("GICP_HIP", (0, 3), 10)
    for i in range(2):
        _same_stream(fleet[i], solo[i], f"GICP_HIP stream {i}", fitness=False)


def test_gicp_hip_fleet_matching_error_is_bitwise_the_solo_streams():
    solo, fleet = _solo("GICP_HIP", (0, 3), 10), _fleet("GICP_HIP", (0, 3), 10)
    for i in range(2):
        _same_stream(fleet[i], solo[i], f"GICP_HIP stream {i}", fitness=True)


# ------------------------------------------------------------------------------------------------------ (b) default FAST_GICP, per step
def test_default_fast_gicp_fleet_matches_a_lone_registration_step_by_step():
    """After every step each stream's record is compared with a lone registration of the fleet's own (keyframe, frame, guess) of that step --
    per step, so a last-bit difference cannot cascade through the keyframe decisions.  Tolerances: the project's figures for exactly this
    comparison (align_pairs_scenes.POSE_TOL, FIT_RTOL); flags and the keyframe count the decisions give must be equal."""
    from delta_graph_slam_amd.odometry import ScanMatchingOdometryFleet, matching_decision
    from tests.helpers import pose_error
    clouds, stamps = streams()
    which = (0, 1, 3)
    reg, lone = _registration("FAST_GICP"), _registration("FAST_GICP")
    fleet = ScanMatchingOdometryFleet(reg, 3, [dict(THRESHOLDS[i], **DOWN) for i in which])
    worst = np.zeros(3)
    for k in range(10):
        before = []
        for s in fleet.streams:
            shadow = types.SimpleNamespace(**{a: getattr(s, a) for a in ("keyframe_delta_trans", "keyframe_delta_angle", "keyframe_delta_time", "transform_thresholding",
                                                                        "max_acceptable_trans", "max_acceptable_angle", "keyframe_pose", "keyframe_stamp", "prev_time",
                                                                        "prev_trans", "n_keyframes")})
            before.append((s.key.read(reg) if s.has_keyframe else None, shadow))
        fleet.step([stamps[k]] * 3, [clouds[i][k] for i in which], want_status=True)
        for j, i in enumerate(which):
            key, shadow = before[j]
            if key is None:
                continue
            lone.setInputTarget(key)
            lone.setInputSource(lone.voxel_grid_filter(clouds[i][k], LEAF))
            lone.align(shadow.prev_trans)
            st = fleet.last_status[j]
            assert st.has_converged == lone.hasConverged(), (k, j)
            dt, dr = pose_error(st.relative_pose, lone.getFinalTransformation())
            fit = lone.getFitnessScore()
            df = abs(st.matching_error - fit) / abs(fit)
            worst = np.maximum(worst, (dt, dr, df))
            assert dt <= S.POSE_TOL[0] and dr <= S.POSE_TOL[1] and df <= S.FIT_RTOL, (k, j, dt, dr, df)
            matching_decision(shadow, stamps[k], lone.hasConverged(), lone.getFinalTransformation(), lambda: None)
            assert shadow.n_keyframes == fleet.n_keyframes[j], (k, j)
    print(f"default FAST_GICP fleet against lone registrations: worst {worst[0]:.3e} m, {worst[1]:.3e} rad, fitness {worst[2]:.3e} relative")
    reg.close()
    lone.close()


# ------------------------------------------------------------------------------------------------------ (c) one stream, any method
@pytest.mark.parametrize("method", ["FAST_GICP", "NDT_OMP", "ICP_HIP"])
def test_one_stream_fleet_is_bitwise_the_solo_class(method):
    solo, fleet = _solo(method, (3,), 8), _fleet(method, (3,), 8)   # the nodelet's default thresholds: a switch at nearly every frame
    _same_stream(fleet[0], solo[0], method)
    print(method, "converged", [r[2].has_converged for r in fleet[0][1:]], "keyframes", [r[1] for r in fleet[0]])
    assert fleet[0][-1][1] >= 2   # at least one switch: the swapped cloud became the registration's target (NDT 1.0 m tracks these sparse frames poorly: it switches once)


# ------------------------------------------------------------------------------------------------------ (d) keyframe switch
def test_a_keyframe_switch_builds_no_index_and_no_covariances():
    """The new keyframe was the source one call earlier and keeps what it made then: a step registers B frames and makes B indices and B
    covariance passes, the frames', whether or not keyframes switched before it.  Only the step after the first frames makes both sides."""
    from delta_graph_slam_amd import _lib as L
    from delta_graph_slam_amd.odometry import ScanMatchingOdometryFleet
    clouds, stamps = streams()
    which = (0, 1, 3)
    reg = _registration("FAST_GICP")
    fleet = ScanMatchingOdometryFleet(reg, 3, [dict(THRESHOLDS[i], **DOWN) for i in which])
    reg.profile_enable(True)
    switches = 0
    for k in range(8):
        reg.profile_reset()
        single_before = reg.fitness_batch_counts()["single_builds"]
        kf_before = list(fleet.n_keyframes)
        fleet.step([stamps[k]] * 3, [clouds[i][k] for i in which])
        cov = reg.profile_get(L.K_GICP_COVARIANCE)[1]
        counts = reg.fitness_batch_counts()
        print(f"step {k}: covariance passes {cov}, indices built {counts['indices_built']}, keyframes {fleet.n_keyframes}")
        assert counts["single_builds"] == single_before
        if k == 0:
            assert cov == 0
        elif k == 1:
            assert cov == 6 and counts["indices_built"] == 6
        else:
            assert cov == 3 and counts["indices_built"] == 3, (k, cov, counts)
            switches += sum(a != b for a, b in zip(kf_before, fleet.n_keyframes))   # switches the PREVIOUS steps made were free in this one
    assert switches >= 4
    reg.close()


# ------------------------------------------------------------------------------------------------------ (e) non-convergence
@pytest.mark.parametrize("kind", ["moved 100 m", "no finite point"])
def test_a_frame_that_does_not_converge_is_ignored_in_its_stream_only(kind):
    """Frame 5 of the second stream is replaced.  "moved 100 m": FAST_GICP finds almost no correspondence, its step is below the
    epsilons and -- as fast_gicp does -- it reports convergence at the guess (measured here: converged, inlier fraction 0.005), so the
    stream does what the solo class does with that frame, whichever branch that is.  "no finite point": the frame filters to nothing,
    the pair fails with "no source", and the stream takes the "ignore this frame" branch.  Either way the first stream never notices,
    and the second is bitwise a solo ScanMatchingOdometry over the same frames."""
    from delta_graph_slam_amd.odometry import ScanMatchingOdometry, ScanMatchingOdometryFleet
    clouds, stamps = streams()
    which = (0, 1)
    status = kind == "moved 100 m"   # the solo class cannot report a status without a source
    good = _fleet("FAST_GICP", which, 7, batch_independent=True)
    bad = synth.apply_transform(synth.make_transform((100.0, 0.0, 0.0), (0.0, 0.0, 0.0)), clouds[1][5]) if status else np.full((500, 4), np.nan, np.float32)
    frames1 = [bad if k == 5 else clouds[1][k] for k in range(7)]
    solo_reg = _registration("FAST_GICP", batch_independent=True)
    solo = ScanMatchingOdometry(solo_reg, dict(THRESHOLDS[1], **DOWN))
    reg = _registration("FAST_GICP", batch_independent=True)
    fleet = ScanMatchingOdometryFleet(reg, 2, [dict(THRESHOLDS[i], **DOWN) for i in which])
    for k in range(7):
        kf, prev, pose = fleet.n_keyframes[1], fleet.streams[1].prev_trans.copy(), fleet.streams[1].keyframe_pose.copy()
        odoms = fleet.step([stamps[k]] * 2, [clouds[0][k], frames1[k]], want_status=status)
        ref = solo.matching(stamps[k], frames1[k], want_status=status)
        assert np.array_equal(odoms[0], good[0][k][0]) and fleet.n_keyframes[0] == good[0][k][1]   # the other stream never notices
        assert np.array_equal(odoms[1], ref) and fleet.n_keyframes[1] == solo.n_keyframes, k
        if status and k > 0:
            a, b = fleet.last_status[1], solo.last_status
            assert a.has_converged == b.has_converged and _bits(a.inlier_fraction) == _bits(b.inlier_fraction) and _bits(a.matching_error) == _bits(b.matching_error), k
        if k == 5 and status:
            print("the moved frame: converged", fleet.last_status[1].has_converged, "inlier fraction", fleet.last_status[1].inlier_fraction)
            assert fleet.last_status[1].inlier_fraction < 0.05
        if k == 5 and not status:
            assert np.array_equal(odoms[1], (pose @ prev).astype(np.float32))                      # "ignore this frame"
            assert fleet.n_keyframes[1] == kf and np.array_equal(fleet.streams[1].prev_trans, prev)
    assert np.array_equal(fleet.streams[1].prev_trans, solo.prev_trans)   # the stream goes on from its keyframe with the next frame
    reg.close()
    solo_reg.close()


def test_gicp_hip_frame_of_fewer_than_k_points_is_not_converged():
    """GICP_HIP: a cloud of fewer than k = 20 points fails its pair (align_pairs documents it); the stream treats it as "not converged"."""
    from delta_graph_slam_amd.odometry import ScanMatchingOdometryFleet
    clouds, stamps = streams()
    good = _fleet("GICP_HIP", (0, 3), 10)
    reg = _registration("GICP_HIP")
    fleet = ScanMatchingOdometryFleet(reg, 2, [dict(THRESHOLDS[i], **DOWN) for i in (0, 3)])
    for k in range(4):
        kf, prev, pose = fleet.n_keyframes[1], fleet.streams[1].prev_trans.copy(), fleet.streams[1].keyframe_pose.copy()
        odoms = fleet.step([stamps[k]] * 2, [clouds[0][k], clouds[3][k][:12] if k == 2 else clouds[3][k]])
        assert np.array_equal(odoms[0], good[0][k][0])
        if k == 2:
            assert np.array_equal(odoms[1], (pose @ prev).astype(np.float32)) and fleet.n_keyframes[1] == kf
    reg.close()


# ------------------------------------------------------------------------------------------------------ (f) the C++ adapter
def test_cpp_fleet_reproduces_the_python_fleet_frame_by_frame(tmp_path):
    """dgs::HipOdometryFleet through tests/cpp/odometry_fleet_driver.cpp on the streams of (a).  What the device computes -- every frame's
    relative pose, convergence flag, matching error, inlier fraction -- and the keyframe counts the decisions give are the Python fleet's
    bit for bit.  The odometry is a product of up to 24 float 4 x 4 matrices formed on the host, by numpy there and by the adapter's own
    loop here: each product rounds its entries once more (relative 2^-24 of sums of at most 4 terms of magnitude <= |t|), so over a chain
    of 24 with translations below 64 m the entries agree to 24 x 4 x 2^-24 x 64 m < 4e-4 m; the figure is printed."""
    exe = str(tmp_path / "odometry_fleet_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "tests", "stub_pcl"), "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "odometry_fleet_driver.cpp"), "-o", exe, os.path.join(ROOT, "delta_graph_slam_amd", "libdgs_reg.so"),
                           "-Wl,-rpath," + os.path.join(ROOT, "delta_graph_slam_amd"), "-Wl,-rpath,/opt/rocm/lib"])
    clouds, stamps = streams()
    fleet = _fleet("FAST_GICP", (0, 1, 2, 3), batch_independent=True)
    pin, pout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(pin, "wb") as f:
        f.write(struct.pack("<q", 4))
        for t in THRESHOLDS:
            f.write(struct.pack("<6d", t["keyframe_delta_trans"], t["keyframe_delta_angle"], t["keyframe_delta_time"], 0.0, 1.0, 1.0))
        f.write(struct.pack("<q", 24))
        for k in range(24):
            for i in range(4):
                c = clouds[i][k]
                f.write(struct.pack("<qd", -1 if c is None else c.shape[0], stamps[k]))
                if c is not None:
                    f.write(np.ascontiguousarray(c, np.float32).tobytes())
    info = json.loads(subprocess.check_output([exe, "FAST_GICP", pin, pout, "1", "2.0", str(LEAF), "0.1"]).decode().strip().splitlines()[-1])
    assert info["ok"] is True and info["frames"] == 24, info
    rec = np.fromfile(pout, dtype=np.dtype([("odom", np.float32, (16,)), ("rel", np.float32, (16,)), ("converged", np.int32), ("keyframes", np.int32),
                                            ("error", np.float64), ("inliers", np.float64)])).reshape(24, 4)
    worst = 0.0
    for k in range(24):
        for i in range(4):
            row = fleet[i][k]
            if row is None:
                continue
            assert rec["keyframes"][k, i] == row[1], (k, i)
            if row[2] is not None:
                assert np.array_equal(rec["rel"][k, i].reshape(4, 4).T, row[2].relative_pose) and bool(rec["converged"][k, i]) == row[2].has_converged, (k, i)
                assert _bits(rec["error"][k, i]) == _bits(row[2].matching_error) and _bits(rec["inliers"][k, i]) == _bits(row[2].inlier_fraction), (k, i)
            worst = max(worst, float(np.abs(rec["odom"][k, i].reshape(4, 4).T - row[0]).max()))
    print(f"C++ fleet against the Python fleet: largest odometry entry difference {worst:.3e}")
    assert worst < 4e-4
