"""InformationMatrixCalculator without a device: the Python mirror's weights and matrices against a float64 restatement of the
reference (tests/information_matrix_reference.py), the new C ABI symbols, the C++ adapter's driver against tests/stub_pcl, and the
facts about the GPU tests' scene that those tests rely on."""
import ctypes as C
import inspect
import json
import math
import os
import re
import subprocess

import numpy as np
import pytest

import information_matrix_reference as R

ROOT = R.ROOT
NEW_SYMBOLS = ("dgs_calc_fitness_score_batch_clouds", "dgs_cloud_build_indices", "dgs_fitness_batch_get_counts")

PARAM_SETS = [
    {},
    {"var_gain_a": 5.0, "min_stddev_x": 0.2, "max_stddev_x": 3.0, "min_stddev_q": 0.01, "max_stddev_q": 0.5, "fitness_score_thresh": 2.5},
    {"use_const_inf_matrix": True, "const_stddev_x": 0.25, "const_stddev_q": 0.3},
    {"delta_var_gain_a": 8.0, "delta_min_stddev_x": 0.3, "delta_max_stddev_x": 2.0, "delta_min_stddev_q": 0.02, "delta_max_stddev_q": 0.4,
     "delta_avg_fitness_score": 0.8, "delta_importance_ratio_global": 2.5, "delta_importance_ratio_local": 3.0},
    {"use_const_inf_matrix": True, "delta_importance_ratio_global": 4.0, "delta_importance_ratio_local": 0.5},
]
FITNESS = [0.0, 1e-9, 0.0137, 0.25, 0.5, 0.7, 2.5, 40.0, 1e6, R.DBL_MAX]


def calculator(params):
    from delta_graph_slam_amd.information_matrix import InformationMatrixCalculator
    return InformationMatrixCalculator(params, registration=object())   # no handle: host arithmetic only


class _FixedFitness:
    """stands in for the registration: calc_fitness_score(_batch) return what the test sets"""
    def __init__(self, values):
        self.values = list(values)

    def calc_fitness_score(self, c1, c2, relpose=None, max_range=R.DBL_MAX):
        return self.values[0]

    def calc_fitness_score_batch(self, c1s, c2s, relposes=None, max_range=R.DBL_MAX, return_used=False):
        assert len(c1s) == len(c2s) == len(relposes) == len(self.values)
        assert all(np.asarray(r).dtype == np.float32 for r in relposes)   # relpose.cast<float>()
        return np.array(self.values, np.float64)


@pytest.mark.parametrize("p", range(len(PARAM_SETS)))
def test_information_matrix_equals_the_restatement(p):
    from delta_graph_slam_amd.information_matrix import InformationMatrixCalculator
    prm = PARAM_SETS[p]
    cloud = np.zeros((1, 4), np.float32)
    for f in FITNESS:
        calc = InformationMatrixCalculator(prm, registration=_FixedFitness([f]))
        want = R.information_matrix(prm, f)
        got = calc.calc_information_matrix(cloud, cloud, np.eye(4))
        assert got.shape == (3, 3) and got.dtype == np.float64
        assert np.array_equal(got, want), (prm, f, got, want)
        assert np.array_equal(calc.calc_information_matrix_buildings_global(f), R.information_matrix_buildings_global(prm, f))
    calc = InformationMatrixCalculator(prm, registration=_FixedFitness(FITNESS))
    many = calc.calc_information_matrices([(cloud, cloud, np.eye(4))] * len(FITNESS))
    assert many.shape == (len(FITNESS), 3, 3)
    assert np.array_equal(many, np.stack([R.information_matrix(prm, f) for f in FITNESS]))
    assert calc.calc_information_matrices([]).shape == (0, 3, 3)


def test_the_weights_pass_through_float():
    """fitness 0 gives min_var, fitness = thresh gives max_var, each cast to float before the division (.cpp:68-73)"""
    calc = calculator({})
    assert calc.fitness_score_thresh == 0.5   # the reference constructor's default (.cpp:38), not the 2.5 of its `load` template (.hpp:35)
    m0 = calc._from_fitness(0.0)
    assert m0[0, 0] == m0[1, 1] == 1.0 / float(np.float32(0.1 ** 2)) and m0[2, 2] == 1.0 / float(np.float32(0.05 ** 2))
    assert m0[0, 0] != 1.0 / (0.1 ** 2)       # the cast shows
    m1 = calc._from_fitness(0.5)
    assert m1[0, 0] == 1.0 / float(np.float32(5.0 ** 2)) and m1[2, 2] == 1.0 / float(np.float32(0.2 ** 2))
    assert np.count_nonzero(m0) == 3 and np.count_nonzero(m1) == 3
    # DBL_MAX ("no point qualified"): exp(-inf) = 0, the weight goes past max_var by the factor 1 / (1 - exp(-a thresh))
    mx = calc._from_fitness(R.DBL_MAX)
    assert mx[0, 0] == 1.0 / float(np.float32(0.01 + (25.0 - 0.01) / (1.0 - math.exp(-10.0))))


@pytest.mark.parametrize("p", range(len(PARAM_SETS)))
def test_buildings_local_equals_the_restatement(p):
    prm = PARAM_SETS[p]
    calc = calculator(prm)
    for avg in (0.0, 0.05, 0.5, 0.8, 3.0, 30.0):
        for cov in (0.0, 37.5, 100.0):
            for edge in (False, True):
                want = R.information_matrix_buildings_local(prm, avg, cov, edge)
                got = calc.calc_information_matrix_buildings_local(R.alignment(avg, cov, edge))
                assert np.array_equal(got, want), (prm, avg, cov, edge)
    # use_const_inf_matrix has no say here (.cpp:134-157), isEdgeAligned and the coverage factor do
    a = calc.calc_information_matrix_buildings_local(R.alignment(0.5, 50.0, False))
    b = calc.calc_information_matrix_buildings_local(R.alignment(0.5, 50.0, True))
    ratio = {**R.DEFAULTS, **prm}["delta_importance_ratio_local"]
    assert np.allclose(b, a * ratio, rtol=1e-15)
    assert np.array_equal(calc.calc_information_matrix_buildings_local(R.alignment(0.5, 100.0, False)) * 0.5, a)


def test_b_weight_is_the_logistic_curve():
    from delta_graph_slam_amd.information_matrix import InformationMatrixCalculator as IMC
    assert IMC.b_weight(20.0, 0.5, 1.0, 3.0, 0.5) == 2.0
    assert IMC.b_weight(20.0, 0.5, 1.0, 3.0, -1e9) == 1.0
    for x in (0.0, 0.3, 0.6, 1.2):
        assert IMC.b_weight(7.0, 0.4, 0.2, 0.9, x) == R.b_weight(7.0, 0.4, 0.2, 0.9, x)
    assert np.isnan(IMC.b_weight(20.0, 0.5, 1.0, 3.0, 1e9))   # inf / inf, as std::exp gives upstream


def test_new_symbols_are_declared_exported_and_bound():
    from delta_graph_slam_amd import _lib as L
    from delta_graph_slam_amd.information_matrix import InformationMatrixCalculator as IMC
    from delta_graph_slam_amd.registration import Registration
    lib = L.load()
    header = open(os.path.join(ROOT, "include", "dgs_reg.h")).read()
    for s in NEW_SYMBOLS:
        assert re.search(r"\bint\s+" + s + r"\s*\(", header), s
        assert s in L.SYMBOLS and hasattr(lib, s) and getattr(lib, s).argtypes, s
    assert lib.dgs_abi_version() == 5
    for m in ("calc_fitness_score_batch", "build_indices", "fitness_batch_counts"):
        assert callable(getattr(Registration, m))
    assert list(inspect.signature(Registration.calc_fitness_score_batch).parameters)[1:] == ["cloud1s", "cloud2s", "relposes", "max_range", "return_used"]
    for m in ("calc_information_matrices", "calc_information_matrix_buildings_global", "calc_information_matrix_buildings_local", "b_weight"):
        assert callable(getattr(IMC, m))
    assert os.path.exists(os.path.join(ROOT, "include", "dgs", "information_matrix_hip.hpp"))


def test_invalid_arguments_are_rejected_without_touching_a_device():
    from delta_graph_slam_amd import _lib as L
    lib = L.load()
    out = (C.c_double * 1)()
    ptrs = (C.c_void_p * 1)()
    assert lib.dgs_calc_fitness_score_batch_clouds(None, 1, C.cast(ptrs, C.c_void_p), C.cast(ptrs, C.c_void_p), None, 1.0, C.cast(out, C.c_void_p), None) == 1
    assert lib.dgs_cloud_build_indices(None, 1, C.cast(ptrs, C.c_void_p)) == 1
    assert lib.dgs_fitness_batch_get_counts(None, None) == 1


def test_the_scene_is_what_the_gpu_tests_assume():
    clouds, poses = R.scene()
    sizes = [clouds[f"k{i}"].shape[0] for i in range(6)]
    assert all(3500 <= n <= 4096 for n in sizes), sizes          # a few thousand points: index depth 3
    assert [R.index_depth(n) for n in sizes] == [3] * 6
    assert [R.index_depth(n) for n in R.SUB_SIZES] == [1, 1, 1, 1, 2, 2, 3]
    assert clouds["big"].shape[0] > 4096 and R.index_depth(clouds["big"].shape[0]) == 4
    assert [R.index_depth(clouds[t].shape[0]) for t in R.DEPTH_TARGETS] == [1, 2, 3, 4]
    assert np.allclose([np.linalg.norm(poses[i][:3, 3] - poses[i - 1][:3, 3]) for i in range(1, 6)], 2.0)
    assert len(R.main_edges()) == 16 and len(R.size_edges()) == 44
    assert R.main_edges()[5][0] == R.main_edges()[6][0] == "k5"     # the two loop edges share key1
    assert R.main_edges()[R.SELF_EDGE][0] == R.main_edges()[R.SELF_EDGE][1]
    assert np.isnan(clouds["nonfinite"]).sum() == 1 and np.isinf(clouds["nonfinite"]).sum() == 1


def test_the_oracle_on_the_scene():
    """max_range = 0.05 keeps a part of every odometry edge's points (neither none nor all), 1e-7 and -1 keep none"""
    clouds, _ = R.scene()
    full = R.oracle_edges("main", R.DBL_MAX)
    part = R.oracle_edges("main", 0.05)
    for e in range(R.N_ODOMETRY):
        n2 = clouds[R.main_edges()[e][1]].shape[0]
        print("odometry edge", e, "points", n2, "within 0.05:", part[e][1], "scores", full[e][0], part[e][0])
        assert full[e][1] == n2 and 0.25 * n2 < part[e][1] < 0.75 * n2
        assert part[e][0] < 0.05 < full[e][0]
    assert full[R.SELF_EDGE] == (0.0, clouds["k2"].shape[0])
    for mr in (1e-7, -1.0):
        o = R.oracle_edges("main", mr)
        assert all(o[e] == (R.DBL_MAX, 0) for e in range(len(o)) if e != R.SELF_EDGE)
    assert R.oracle_edges("main", -1.0)[R.SELF_EDGE] == (R.DBL_MAX, 0)
    # the size edges: used = n2 for every finite cloud2, DBL_MAX for the empty one
    for (t, c2, _), (s, used) in zip(R.size_edges(), R.oracle_edges("size", R.DBL_MAX)):
        assert used == clouds[c2].shape[0] and (s == R.DBL_MAX) == (used == 0)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return R.build_driver(tmp_path_factory.mktemp("imdrv"))


@pytest.mark.parametrize("p", [0, 3, 4])
def test_adapter_driver_host_forms_and_soft_failure(driver, tmp_path, p):
    """The driver compiles against tests/stub_pcl.  The two building forms are host arithmetic and equal the restatement with or
    without a device; without a GPU the device calls fail soft: ok = false, a message, exit code 0."""
    prm = PARAM_SETS[p]
    clouds, _ = R.scene()
    ip, op = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    tail = (0.137, 0.42, 63.0, 1.0)
    R.write_driver_input(ip, [clouds["sub65"], clouds["e33"]], [(0, 1, R.relpose(0, 1)), (0, 0, np.eye(4))], tail)
    args = [f"{k}={int(v) if isinstance(v, bool) else v}" for k, v in prm.items()]
    res = json.loads(subprocess.check_output([driver, ip, op] + args, timeout=120).decode().splitlines()[-1])
    m = R.read_driver_output(op)
    assert np.array_equal(m[0], R.information_matrix_buildings_global(prm, tail[0]))
    assert np.array_equal(m[1], R.information_matrix_buildings_local(prm, tail[1], tail[2], True))
    try:
        import torch
        gpu = torch.cuda.is_available()
    except Exception:
        gpu = False
    if prm.get("use_const_inf_matrix"):
        assert res["ok"] and m.shape[0] == 2 + 3 * 2      # the constant matrix needs no device
        assert all(np.array_equal(x, R.information_matrix(prm, 0.0)) for x in m[2:])
    elif not gpu:
        assert res["ok"] is False and res["error"] and m.shape[0] == 2
    else:
        assert res["ok"] and m.shape[0] == 2 + 3 * 2
