"""dgs_floor_detection_batch without a GPU: the symbols and their declarations, the argument checks that come before
any device is touched, the wrapper's list checks, the host plan against hand-written expectations, and the C++ driver against the
stubs."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("dgs_floor_detection_batch", "dgs_floor_detection_batch_get_filtered", "dgs_floor_detection_batch_get_inliers",
               "dgs_floor_detection_batch_get_trace", "dgs_floor_detection_batch_get_clipped", "dgs_floor_detection_batch_get_counts")


def test_the_library_exports_the_new_symbols():
    from delta_graph_slam_amd import _lib as L
    lib = L.load()
    for s in NEW_SYMBOLS:
        assert s in L.SYMBOLS and hasattr(lib, s)
    assert lib.dgs_abi_version() == 5                                # additions only


def test_the_header_declares_what_the_library_exports():
    with open(os.path.join(ROOT, "include", "dgs_reg.h")) as f:
        header = f.read()
    assert "int dgs_floor_detection_batch(dgs_handle* h, const dgs_floor_detection_params* params, const float* tilt16, const float* tilt_inv16," in header
    for s in NEW_SYMBOLS[1:]:
        assert f"int {s}(dgs_handle* h, " in header
    assert "#define DGS_ABI_VERSION 5" in header


def test_the_new_calls_check_their_arguments_without_touching_a_device():
    from delta_graph_slam_amd import _lib as L
    lib = L.load()
    p = L.FloorDetectionParams()
    assert lib.dgs_floor_detection_params_init(C.byref(p)) == 0
    eye = np.eye(4, dtype=np.float32).reshape(16)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    n = 2
    sizes = np.zeros(n, np.int64)
    ptrs = (C.c_void_p * n)(None, None)
    co, st = np.full((n, 4), 7.0, np.float32), np.full(n, 7, np.int32)

    def call(h=None, params=p, n_scans=n, sizes=sizes):
        return lib.dgs_floor_detection_batch(h, C.byref(params), vp(eye), vp(eye), n_scans, ptrs, vp(sizes), 0, None, None, vp(co), vp(st))

    assert call() == 1                                               # NULL handle
    assert call(n_scans=0) == 1
    wrong = L.FloorDetectionParams.from_buffer_copy(p)
    wrong.struct_size = p.struct_size - 4
    assert call(params=wrong) == 1                                   # refused before the handle is looked at
    assert call(n_scans=-1) == 1
    assert call(sizes=np.array([0, -1], np.int64)) == 1
    assert np.all(co == 7.0) and np.all(st == 7)                     # nothing written
    k = C.c_int64(-1)
    t = L.FloorDetectionTrace()
    counts = (C.c_int64 * 8)()
    assert lib.dgs_floor_detection_batch_get_filtered(None, 0, None, 0, 0, C.byref(k)) == 1 and k.value == -1
    assert lib.dgs_floor_detection_batch_get_inliers(None, 0, None, None, 0, C.byref(k)) == 1 and k.value == -1
    assert lib.dgs_floor_detection_batch_get_clipped(None, 0, None, None, 0, C.byref(k)) == 1 and k.value == -1
    assert lib.dgs_floor_detection_batch_get_trace(None, 0, C.byref(t)) == 1
    assert lib.dgs_floor_detection_batch_get_counts(None, counts) == 1


def test_the_python_wrapper_validates_its_lists_before_the_library_is_called():
    from delta_graph_slam_amd.floor_detection import FloorDetector, params_from_dict
    det = FloorDetector.__new__(FloorDetector)                       # no handle: the checks come first
    det.params = params_from_dict({})
    clouds = [np.zeros((3, 4), np.float32), np.zeros((2, 4), np.float32)]
    with pytest.raises(ValueError):
        det.detect_batch(clouds, rng_raws=[None])
    with pytest.raises(ValueError):
        det.detect_batch([np.zeros((3, 3), np.float32)])             # not [N,4]

    class FakeDevice:
        is_cuda = True

    with pytest.raises(ValueError):
        det.detect_batch([clouds[0], FakeDevice()])                  # numpy and device tensors mixed


def test_the_host_plan_against_hand_written_expectations(tmp_path):
    """floor_detection_plan.h has no HIP in it: a plain g++ program includes it and checks the first-workgroup tables at 0 / 1 /
    256 / 257 / 1,023 / 1,024 / 1,025 points, dead scans between live ones, chunk boundaries, round tables where scans close in different
    rounds, the y extent of a round, the status mapping and the verdict (status, dot product, coefficients at its edges); built with the host sanitizers and run directly"""
    exe = str(tmp_path / "floor_detection_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "delta_graph_slam_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "floor_detection_plan_check.cpp"),
                           "-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 0 and p.stdout.strip().splitlines()[-1] == "ok", p.stdout + p.stderr


def test_cpp_driver_compiles_and_links_against_the_stubs(tmp_path):
    exe = str(tmp_path / "floor_detection_batch_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "tests", "stub_eigen"), "-I", os.path.join(ROOT, "tests", "stub_pcl"),
                           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "floor_detection_batch_driver.cpp"), "-o", exe,
                           os.path.join(ROOT, "delta_graph_slam_amd", "libdgs_reg.so"), "-Wl,-rpath," + os.path.join(ROOT, "delta_graph_slam_amd"),
                           "-Wl,-rpath,/opt/rocm/lib"])
    assert subprocess.run([exe], capture_output=True).returncode == 2   # usage: no device touched
