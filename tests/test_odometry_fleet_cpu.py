"""CPU tests of the odometry fleet: the C++ adapter compiles against the stubs, the Python class refuses what it cannot serve
before it touches a device, the new C calls reject bad arguments without one, and matching_decision -- the host decisions factored out of
ScanMatchingOdometry.matching -- gives what `matching` gave before the split (tests/golden/odometry_decisions_parent.npz: the inputs a
scripted registration fed the class as it stood, and what it returned and kept, frame by frame)."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "odometry_decisions_parent.npz")


def test_header_compiles_with_wall_and_the_driver_fails_soft_without_a_gpu(tmp_path):
    import torch
    exe = str(tmp_path / "odometry_fleet_driver")
    p = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "tests", "stub_pcl"), "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "cpp", "odometry_fleet_driver.cpp"), "-o", exe, os.path.join(ROOT, "delta_graph_slam_amd", "libdgs_reg.so"),
                        "-Wl,-rpath," + os.path.join(ROOT, "delta_graph_slam_amd"), "-Wl,-rpath,/opt/rocm/lib"], capture_output=True, text=True)
    assert p.returncode == 0 and "warning" not in p.stderr, p.stderr
    pin, pout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    rng = np.random.default_rng(1)
    with open(pin, "wb") as f:
        f.write(np.int64(2).tobytes())
        for _ in range(2):
            f.write(np.array([0.25, 0.15, 1.0, 0.0, 1.0, 1.0], np.float64).tobytes())
        f.write(np.int64(1).tobytes())
        for _ in range(2):
            f.write(np.int64(64).tobytes() + np.float64(0.0).tobytes() + rng.uniform(-1, 1, (64, 4)).astype(np.float32).tobytes())
    out = subprocess.check_output([exe, "FAST_GICP", pin, pout, "0", "2.0", "0.1", "0.01"]).decode()
    info = json.loads(out.strip().splitlines()[-1])
    if not torch.cuda.is_available():   # no device: never throws, no frame advanced, the reason is there
        assert info["ok"] is False and info["frames"] == 0 and info["error"]
    else:
        assert info["ok"] is True and info["frames"] == 1
    assert subprocess.call([exe, "BOGUS", pin, pout, "0", "2.0", "0.1", "0.01"], stdout=subprocess.DEVNULL) == 3


class _Stub:
    """a registration that is never asked for a device"""

    def __init__(self, method):
        self.method = method

    def make_cloud(self, cloud):
        raise AssertionError("the fleet reached for the device before it checked the method")


def test_more_than_one_stream_needs_a_method_that_align_pairs_serves():
    from delta_graph_slam_amd.odometry import ScanMatchingOdometryFleet
    for method in ("NDT_OMP", "ICP_HIP", "FAST_VGICP"):
        with pytest.raises(NotImplementedError) as e:
            ScanMatchingOdometryFleet(_Stub(method), 2, {})
        assert method in str(e.value)
    with pytest.raises(ValueError):
        ScanMatchingOdometryFleet(_Stub("FAST_GICP"), 0, {})
    with pytest.raises(ValueError):
        ScanMatchingOdometryFleet(_Stub("FAST_GICP"), 3, [{}, {}])


def test_the_new_calls_reject_bad_arguments_without_a_device():
    from delta_graph_slam_amd import _lib as L
    lib = L.load()
    n = C.c_int64(0)
    assert lib.dgs_cloud_assign_batch(None, 1, None, None, 0, 1, 0.1, None, None) == 1          # DGS_ERR_INVALID_ARGUMENT
    assert lib.dgs_calc_inlier_fraction_batch_clouds(None, 1, None, None, None, 0.25, None, None) == 1
    assert lib.dgs_cloud_assign_get_counts(None, None) == 1
    assert lib.dgs_cloud_read(None, None, None, 0, 0, C.byref(n)) == 1
    for s in ("dgs_cloud_assign_batch", "dgs_calc_inlier_fraction_batch_clouds"):
        assert s in L.SYMBOLS
    assert lib.dgs_abi_version() == 5


@pytest.mark.parametrize("name", ["default", "fails", "thresholding"])
def test_matching_decision_gives_what_matching_gave(name):
    from delta_graph_slam_amd.odometry import ScanMatchingOdometry, matching_decision
    g = np.load(GOLDEN)
    params = json.loads(bytes(g[f"{name}_params"]).decode())
    stamps, conv, trans, odom, state = (g[f"{name}_{k}"] for k in ("stamps", "converged", "trans", "odom", "state"))

    class Scripted:
        method = "SCRIPTED"
        k = -1

        def setInputTarget(self, c): pass
        def setInputSource(self, c): pass
        def align(self, guess): self.k += 1
        def hasConverged(self): return bool(conv[self.k])
        def getFinalTransformation(self): return trans[self.k].copy()

    # the class as it stands now, through `matching`
    odo = ScanMatchingOdometry(Scripted(), params)
    cloud = np.zeros((4, 4), np.float32)
    assert np.array_equal(odo.matching(float(stamps[0]), cloud), odom[0])
    # ... and the function alone on a bare state object
    bare = ScanMatchingOdometry(Scripted(), params)
    bare.matching(float(stamps[0]), cloud)
    switches = []
    for k in range(conv.shape[0]):
        a = odo.matching(float(stamps[k + 1]), cloud)
        b = matching_decision(bare, float(stamps[k + 1]), bool(conv[k]), trans[k].copy(), lambda: switches.append(k))
        for got, who in ((a, odo), (b, bare)):
            assert got.dtype == np.float32 and np.array_equal(got, odom[k + 1]), (name, k)
            kept = np.concatenate([who.keyframe_pose.reshape(-1), who.prev_trans.reshape(-1),
                                   [who.keyframe_stamp, -1.0 if who.prev_time is None else who.prev_time, who.n_keyframes]])
            assert np.array_equal(kept, state[k]), (name, k)
    assert len(switches) == int(state[-1, -1]) - 1 and len(switches) >= 2
    if name != "default":
        assert int((conv == 0).sum()) >= 1
