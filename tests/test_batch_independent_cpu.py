"""CPU tests of the batch-independent switch (dgs_set_batch_independent): the three calls are declared, exported and listed,
refuse bad arguments before any device call, the Python keyword reaches dgs_create (which fails with DGS_ERR_HIP on a box without a GPU,
never with TypeError), and the C++ adapter's setter and factory parameter compile against the PCL-shape stubs."""
import ctypes as C
import json
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "dgs_reg.h")
NEW = ("dgs_set_batch_independent", "dgs_get_batch_independent", "dgs_group_set_batch_independent")


def test_the_three_calls_are_declared_exported_and_listed():
    from delta_graph_slam_amd import _lib as L
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    lib = L.load()
    for name in NEW:
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), f"{name} is not declared in dgs_reg.h"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in L.SYMBOLS
    assert re.search(r"int\s+dgs_set_batch_independent\s*\(\s*dgs_handle\s*\*\s*\w*\s*,\s*int32_t\s+\w+\s*\)", text)
    assert re.search(r"int\s+dgs_get_batch_independent\s*\(\s*const\s+dgs_handle\s*\*\s*\w*\s*,\s*int32_t\s*\*\s*\w+\s*\)", text)
    assert re.search(r"int\s+dgs_group_set_batch_independent\s*\(\s*dgs_group\s*\*\s*\w*\s*,\s*int32_t\s+\w+\s*\)", text)
    assert lib.dgs_abi_version() == 5     # additions only


def test_argument_errors_return_before_any_device_call():
    from delta_graph_slam_amd import _lib as L
    lib = L.load()
    on = C.c_int32(7)
    assert lib.dgs_set_batch_independent(None, 1) == 1            # DGS_ERR_INVALID_ARGUMENT
    assert lib.dgs_set_batch_independent(None, 0) == 1
    assert lib.dgs_get_batch_independent(None, C.byref(on)) == 1 and on.value == 7
    assert lib.dgs_get_batch_independent(None, None) == 1
    assert lib.dgs_group_set_batch_independent(None, 1) == 1
    assert lib.dgs_last_error(None) is not None


def test_the_keyword_is_not_a_dgs_params_field():
    """Registration pops batch_independent before the dgs_params loop, as it does the icp_* options: an unknown keyword is still refused."""
    from delta_graph_slam_amd import _lib as L
    from delta_graph_slam_amd.registration import DgsError, Registration
    assert not hasattr(L.Params(), "batch_independent")
    with pytest.raises((TypeError, DgsError)) as e:
        Registration("FAST_GICP", batch_independent=True, no_such_parameter=1)
    assert e.type is TypeError and "no_such_parameter" in str(e.value) and "batch_independent" not in str(e.value)


def test_no_gpu_gives_dgs_err_hip_not_type_error():
    import torch
    from delta_graph_slam_amd.registration import DgsError, Registration, RegistrationGroup, select_registration_method
    if torch.cuda.is_available():
        r = Registration("FAST_GICP", batch_independent=True)       # with a device the keyword simply works
        assert r.batch_independent is True
        r.close()
        return
    for make in (lambda: Registration("FAST_GICP", batch_independent=True), lambda: Registration("NDT_OMP", batch_independent=True),
                 lambda: RegistrationGroup("FAST_GICP", devices=(0,), batch_independent=True),
                 lambda: select_registration_method({"registration_method": "FAST_GICP", "dgs_batch_independent": True})):
        with pytest.raises(DgsError) as e:
            make()
        assert e.value.status == 2          # DGS_ERR_HIP: dgs_create was reached


def test_surface_of_the_python_classes():
    from delta_graph_slam_amd.registration import Registration, RegistrationGroup
    for cls in (Registration, RegistrationGroup):
        assert callable(getattr(cls, "set_batch_independent"))
        assert isinstance(getattr(cls, "batch_independent"), property) and cls.batch_independent.fset is not None


def test_adapter_setter_and_factory_parameter_compile_against_the_stubs(tmp_path):
    import torch
    out = str(tmp_path / "batch_independent_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "tests", "stub_pcl"), "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "batch_independent_driver.cpp"), "-o", out,
                           os.path.join(ROOT, "delta_graph_slam_amd", "libdgs_reg.so"), "-Wl,-rpath," + os.path.join(ROOT, "delta_graph_slam_amd"),
                           "-Wl,-rpath,/opt/rocm/lib"])
    res = json.loads(subprocess.check_output([out]).decode().strip().splitlines()[-1])
    assert res["served"] == 6 and res["factory_on"] == 6 and res["factory_default_off"] == 6 and res["unserved_is_null"] == 1
    assert (res["initial"], res["after_on"], res["after_align"], res["after_off"]) == (0, 1, 1, 0)
    if torch.cuda.is_available():           # a handle exists after the align: the switch was applied to it, and taken back in place
        assert (res["has_handle"], res["handle_on"], res["handle_off"]) == (1, 1, 0)
    else:
        assert res["has_handle"] == 0
