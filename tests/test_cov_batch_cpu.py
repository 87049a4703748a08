"""The batched k-NN covariance pass where no GPU is needed: the library's new symbols, the Python wrappers' argument checks,
dgs::HipRegistration::buildCovariances through tests/cpp/build_covariances_driver.cpp (compiles against the PCL-shape stubs, links, fails
soft without a device), and the host plan header delta_graph_slam_amd/csrc/cov_batch_plan.h checked on its own by a stand-alone program
under AddressSanitizer and UBSan."""
import ctypes as C
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("dgs_cloud_build_covariances", "dgs_cloud_covariances_get_counts")


def test_the_library_exports_the_new_symbols():
    from delta_graph_slam_amd import _lib as L
    lib = L.load()
    for s in NEW_SYMBOLS:
        assert s in L.SYMBOLS and hasattr(lib, s), s
    # no handle: refused before anything is touched
    ptrs = (C.c_void_p * 1)()
    assert lib.dgs_cloud_build_covariances(None, 1, C.cast(ptrs, C.c_void_p)) == 1
    assert lib.dgs_cloud_covariances_get_counts(None, None) == 1


def test_the_header_declares_what_the_library_exports():
    with open(os.path.join(ROOT, "include", "dgs_reg.h")) as f:
        header = f.read()
    assert "int dgs_cloud_build_covariances(dgs_handle* h, int32_t n, dgs_cloud* const* clouds);" in header
    assert "int dgs_cloud_covariances_get_counts(dgs_handle* h, int64_t* counts8);" in header


def test_the_python_wrappers_validate_their_arguments():
    """build_covariances takes DeviceClouds and nothing else; the check comes before the library is called, so a stand-in object without
    a handle shows it"""
    from delta_graph_slam_amd.registration import Registration
    reg = Registration.__new__(Registration)   # no handle, no device: the wrappers must refuse before they would need one
    for bad in ([None], [object()], ["cloud"], [1.5]):
        with pytest.raises(TypeError):
            Registration.build_covariances(reg, bad)
    with pytest.raises(TypeError):
        Registration.build_covariances(reg, None)   # not a list of clouds at all
    assert callable(Registration.covariance_batch_counts)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("build_covariances") / "build_covariances_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "tests", "stub_pcl"), "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "build_covariances_driver.cpp"), "-o", out,
                           os.path.join(ROOT, "delta_graph_slam_amd", "libdgs_reg.so"), "-Wl,-rpath," + os.path.join(ROOT, "delta_graph_slam_amd"),
                           "-Wl,-rpath,/opt/rocm/lib"])
    return out


def test_cpp_driver_compiles_links_and_fails_soft_without_a_gpu(driver):
    import torch
    info = json.loads(subprocess.check_output([driver, "FAST_GICP_HIP", "3", "400"]).decode().strip().splitlines()[-1])
    assert info["clouds"] == 3
    if torch.cuda.is_available():
        assert info["ok"] is True and info["error"] == ""
        launches, waits, listed, covered, cached, chunks, fallback, built = info["counts"]
        assert (launches, waits, listed, covered, cached, chunks, fallback, built) == (2, 0, 4, 3, 0, 1, 0, 3), info   # the first cloud is listed twice
        other = json.loads(subprocess.check_output([driver, "NDT_HIP", "2", "400"]).decode().strip().splitlines()[-1])
        assert other["ok"] is False and "NDT" in other["error"]
    else:   # no device: never throws, nothing built
        assert info["ok"] is False and info["counts"] == [0] * 8
    assert subprocess.call([driver, "BOGUS", "1", "10"], stdout=subprocess.DEVNULL) == 3


def test_the_host_plan_against_hand_written_expectations(tmp_path):
    """cov_batch_plan.h has no HIP in it: a plain g++ program includes it and checks cache filtering by key, de-duplication, chunking
    (a budget of 300, an over-budget cloud, an empty list), the workgroup prefixes of both launches and `parts` per size"""
    exe = str(tmp_path / "cov_batch_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "delta_graph_slam_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "cov_batch_plan_check.cpp"), "-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 0 and p.stdout.strip().splitlines()[-1] == "ok", p.stdout + p.stderr
