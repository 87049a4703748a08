"""dgs_prefilter_scan_batch without a GPU: the symbols and their declarations, the argument checks that come before any
device is touched, the host plan against hand-written expectations, and the C++ driver against the stubs."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("dgs_prefilter_scan_batch", "dgs_prefilter_batch_get_counts", "dgs_prefilter_batch_get_statistics")


def test_the_library_exports_the_new_symbols():
    from delta_graph_slam_amd import _lib as L
    lib = L.load()
    for s in NEW_SYMBOLS:
        assert s in L.SYMBOLS and hasattr(lib, s)
    assert lib.dgs_abi_version() == 5                                # additions only


def test_the_header_declares_what_the_library_exports():
    with open(os.path.join(ROOT, "include", "dgs_reg.h")) as f:
        header = f.read()
    assert "int dgs_prefilter_scan_batch(dgs_handle* h, const dgs_prefilter_params* chain_params, int32_t n_scans," in header
    assert "int dgs_prefilter_batch_get_counts(dgs_handle* h, int64_t* counts8);" in header
    assert "int dgs_prefilter_batch_get_statistics(dgs_handle* h, double* stats4_per_scan, int64_t capacity_scans, int64_t* n_scans);" in header
    assert "#define DGS_ABI_VERSION 5" in header


def test_the_new_calls_reject_a_null_handle_without_touching_a_device():
    from delta_graph_slam_amd import _lib as L
    lib = L.load()
    cp = L.PrefilterParams()
    assert lib.dgs_prefilter_params_init(C.byref(cp)) == 0
    n = 2
    sizes = (C.c_int64 * n)(0, 0)
    ptrs = (C.c_void_p * n)(None, None)
    m3, m2, st = (C.c_int64 * n)(), (C.c_int64 * n)(), (C.c_int32 * n)(7, 7)
    assert lib.dgs_prefilter_scan_batch(None, C.byref(cp), n, None, ptrs, sizes, 0, ptrs, sizes, ptrs, sizes, 0, m3, m2, None, st) == 1
    assert list(st) == [7, 7]                                        # nothing written
    assert lib.dgs_prefilter_scan_batch(None, C.byref(cp), 0, None, None, None, 0, None, None, None, None, 0, None, None, None, None) == 1
    counts = (C.c_int64 * 8)()
    assert lib.dgs_prefilter_batch_get_counts(None, counts) == 1
    k = C.c_int64(-1)
    assert lib.dgs_prefilter_batch_get_statistics(None, None, 0, C.byref(k)) == 1 and k.value == -1


def test_the_python_wrapper_validates_its_lists_before_the_library_is_called():
    import numpy as np
    from delta_graph_slam_amd.prefilter import Prefilter
    pf = Prefilter.__new__(Prefilter)                                # no handle: the checks come first
    clouds = [np.zeros((3, 4), np.float32), np.zeros((2, 4), np.float32)]
    with pytest.raises(ValueError):
        pf.filter_scan_batch(clouds, angular_velocities=[None])
    with pytest.raises(ValueError):
        pf.filter_scan_batch(clouds, base_link_transforms=[None, None, None])


def test_the_host_plan_against_hand_written_expectations(tmp_path):
    """prefilter_batch_plan.h has no HIP in it: a plain g++ program includes it and checks the first-workgroup tables at 0 / 1 / 256 / 257
    points, dead scans between live ones, chunk boundaries and the status mapping; built with the host sanitizers and run directly"""
    exe = str(tmp_path / "prefilter_batch_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "delta_graph_slam_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "prefilter_batch_plan_check.cpp"), "-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 0 and p.stdout.strip().splitlines()[-1] == "ok", p.stdout + p.stderr


def test_the_table_layouts_against_hand_written_offsets(tmp_path):
    """seg_table.h has no HIP in it either: the offsets of the stage block (entries | heads | firsts | search firsts | totals | statistics)
    and of the covariance pass's chunk sections for 0, 1 and 3 entries, and the first-workgroup array around an empty item, against values
    written out by hand; built with the host sanitizers and run directly"""
    exe = str(tmp_path / "seg_table_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "delta_graph_slam_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "seg_table_check.cpp"), "-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 0 and p.stdout.strip().splitlines()[-1] == "ok", p.stdout + p.stderr


def test_cpp_driver_compiles_and_links_against_the_stubs(tmp_path):
    exe = str(tmp_path / "prefilter_batch_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "tests", "stub_pcl"), "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "prefilter_batch_driver.cpp"), "-o", exe,
                           os.path.join(ROOT, "delta_graph_slam_amd", "libdgs_reg.so"), "-Wl,-rpath," + os.path.join(ROOT, "delta_graph_slam_amd"),
                           "-Wl,-rpath,/opt/rocm/lib"])
    assert subprocess.run([exe], capture_output=True).returncode == 2   # usage: no device touched
