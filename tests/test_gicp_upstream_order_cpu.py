"""CPU tests of the third value of dgs_params.gicp_cov_jacobi_svd (2 = DGS_GICP_COV_UPSTREAM_ORDER): the default is untouched, dgs_create takes the
value, the Python name table and the C++ adapter (setter and factory parameter) carry it."""
import ctypes as C
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_default_stays_0_and_the_names_match_the_header():
    from delta_graph_slam_amd import _lib as L
    lib = L.load()
    for method in (L.METHOD_GICP, L.METHOD_VGICP):
        p = L.Params()
        assert lib.dgs_params_init(C.byref(p), method) == 0
        assert p.gicp_cov_jacobi_svd == 0
    assert L.GICP_COV == {"SYM_EIG": 0, "JACOBI_SVD": 1, "UPSTREAM_ORDER": 2}
    header = open(os.path.join(ROOT, "include", "dgs_reg.h")).read()
    for name, value in L.GICP_COV.items():
        assert f"DGS_GICP_COV_{name} = {value}" in header
    assert lib.dgs_abi_version() == 5      # same struct, same ABI: the field only gained a value


def test_create_takes_the_value_2_like_the_value_0():
    """dgs_create does not reject the new value: with a GPU the handle is made (status 0); without one the status is the missing device's
    (DGS_ERR_HIP), as for the default value -- never DGS_ERR_INVALID_ARGUMENT or DGS_ERR_UNSUPPORTED."""
    from delta_graph_slam_amd import _lib as L
    lib = L.load()
    status = {}
    for mode in (0, 2):
        p = L.Params()
        assert lib.dgs_params_init(C.byref(p), L.METHOD_GICP) == 0
        p.gicp_cov_jacobi_svd = mode
        h = C.c_void_p()
        status[mode] = lib.dgs_create(C.byref(p), C.byref(h))
        if status[mode] == 0:
            assert not lib.dgs_last_error(h)
            lib.dgs_destroy(h)
    assert status[2] == status[0] and status[2] in (0, 2)


@pytest.mark.parametrize("name,method", [("FAST_GICP_HIP", 1), ("FAST_VGICP_HIP", 2)])
def test_cpp_adapter_setter_and_factory_parameter(tmp_path, name, method):
    out = str(tmp_path / "gicp_cov_mode_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "tests", "stub_pcl"), "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "gicp_cov_mode_driver.cpp"), "-o", out,
                           os.path.join(ROOT, "delta_graph_slam_amd", "libdgs_reg.so"), "-Wl,-rpath," + os.path.join(ROOT, "delta_graph_slam_amd"),
                           "-Wl,-rpath,/opt/rocm/lib"])
    res = json.loads(subprocess.check_output([out, name]).decode().strip().splitlines()[-1])
    assert res["method"] == method and res["k"] == 15
    assert res["default"] == 0 and res["parameter_false"] == 0 and res["with_parameter"] == 2
    assert (res["set_1"], res["set_2"], res["set_0"]) == (1, 2, 0)
    assert res["enum"] == [0, 1, 2]
