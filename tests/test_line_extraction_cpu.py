"""CPU tests of the line extraction: the numpy restatement on its own (generator, draw stream, walk, planted scenes, tolerance spread,
threshold margins) and the C boundary without a device (struct layout, defaults, rejections)."""
import ctypes as C
import json
import os
import subprocess
import tempfile

import numpy as np
import pytest

import line_extraction_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# Largest difference of any A / B coordinate or statistic between the restatement with numpy's float32 trigonometry and with the
# trigonometry evaluated in float64 and rounded, over every scene of the GPU tests (test_tolerance_spread measures it again).  The
# two differ in 10 of 34 calls on the non-flat scenes, but the largest root moves by at most an ulp and the eigenvector's x and y come
# out the same floats: the measured spread is 0, so the doubles are compared exactly.
SPREAD = 0.0
TOL = 4.0 * SPREAD


def all_scenes():
    yield "nonflat", R.nonflat_scene()
    for n in R.SIZES:
        for it in R.ITERATIONS:
            yield f"n{n}_it{it}", R.size_scene(n, it)


def test_mt19937_check_value():
    g = R.MT19937()
    for _ in range(9999):
        g()
    assert g() == 4123659995
    g = R.MT19937(12345)
    assert R.mt_raw(3) == [g() >> 1 for _ in range(3)]


def test_draw_stream_against_a_hand_written_swap_trace():
    # n = 5, s = [0 1 2 3 4]
    # draw 1: 7 % 5 = 2 -> swap s0, s2: [2 1 0 3 4]; 1 + 2 % 4 = 3 -> swap s1, s3: [2 3 0 1 4] -> (2, 3)
    # draw 2: 0 % 5 = 0 and 1 + 0 % 4 = 1: nothing moves                                      -> (2, 3)
    # draw 3: 4 % 5 = 4 -> swap s0, s4: [4 3 0 1 2]; 1 + 3 % 4 = 4 -> swap s1, s4: [4 2 0 1 3] -> (4, 2)
    st = R.draw_stream(5, [7, 2, 0, 0, 4, 3])
    assert [next(st) for _ in range(3)] == [(2, 3), (2, 3), (4, 2)]
    with pytest.raises(R.StreamEnd):
        next(st)
    # n = 2: the second swap has one choice
    st = R.draw_stream(2, [1, 9, 1, 9])
    assert [next(st) for _ in range(2)] == [(1, 0), (0, 1)]


def test_walk_early_stop_bound_and_takeover():
    # 90 of 100 inliers: k = log(0.01) / log(1 - 0.81) = 2.77 -> three iterations
    assert R.walk([90] * 600, 100, 500) == (0, 3)
    # 10 of 100: k = 458.2 -> 459 iterations; an equal count does not take over, a greater one does
    assert R.walk([10] * 600, 100, 500) == (0, 459)
    assert R.walk([10, 10, 20] + [0] * 600, 100, 500)[0] == 2
    assert R.walk([10, 10] + [0] * 600, 100, 500)[0] == 0
    # the bound: at most max_iterations + 1 hypotheses
    assert R.walk([1] * 600, 100, 4) == (0, 5)
    assert R.walk([1] * 600, 100, 0) == (0, 1)
    assert R.walk([0] * 600, 100, 7) == (0, 8)      # no inlier at all: k is huge, the bound ends the walk


def test_restatement_finds_the_planted_segments():
    cloud, prm = R.size_scene(1500, 100)
    lines, rounds, status = R.cached("n1500_it100", cloud, prm)
    assert len(lines) == 2 and status == "MAX_ROUNDS" and len(rounds) == 12
    for l in lines:
        length = np.linalg.norm(l["A"] - l["B"])     # inliers lie within 0.1 of the sample's line; the refit line may sit up to as far again
        assert 7.0 < length < 8.5 and l["mean"] < 0.06 and l["min"] <= l["mean"] <= l["max"] < 0.2 and l["A"][2] == 0 and l["B"][2] == 0
    assert rounds[0]["inliers"] >= rounds[0]["cluster"] > 400
    assert np.all(np.diff(rounds[0]["cluster_idx"]) > 0) and set(rounds[0]["cluster_idx"]) <= set(rounds[0]["inlier_idx"])
    # below min_cluster_size nothing runs; at it, one round
    assert R.cached("n24_it100", *R.size_scene(24, 100))[1] == []
    assert len(R.cached("n25_it100", *R.size_scene(25, 100))[1]) == 1


def test_and_rule_never_accepts_a_flattened_sample():
    cloud, prm = R.size_scene(64, 1)
    lines, rounds, status = R.line_extraction(cloud, dict(prm, sample_good_any_axis=0))
    assert status == "RANSAC_FAILED" and rounds[0]["draws"] == 1000 and rounds[0]["iterations"] == 0 and not lines


def test_tolerance_spread():
    spread = 0.0
    for name, (cloud, prm) in all_scenes():
        a = R.cached(name, cloud, prm)
        b = R.cached(name, cloud, prm, trig="f64")
        assert len(a[0]) == len(b[0])
        for x, y in zip(a[0], b[0]):
            for k in x:
                spread = max(spread, float(np.max(np.abs(np.asarray(x[k]) - np.asarray(y[k])))))
    print("spread", spread)
    assert spread <= SPREAD and TOL < 1e-4


def test_thresholds_are_farther_than_the_tolerance_in_every_round():
    for name, (cloud, prm) in all_scenes():
        p = dict(R.DEFAULTS, **prm)
        for r in R.cached(name, cloud, prm)[1]:
            if "mean" in r:
                assert abs(r["mean"] - p["merror_threshold"]) > TOL and abs(r["length"] - p["line_length_threshold"]) > TOL, (name, r)


def test_struct_layouts_match_the_header():
    from delta_graph_slam_amd import _lib as L
    src = r'''
#include <stdio.h>
#include <stddef.h>
#include "dgs_reg.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(dgs_line_extraction_params), offsetof(dgs_line_extraction_params, cluster_tolerance),
         offsetof(dgs_line_extraction_params, merror_threshold), offsetof(dgs_line_extraction_params, sac_method_type),
         offsetof(dgs_line_extraction_params, record_lists), sizeof(dgs_line_feature), offsetof(dgs_line_feature, mean_error),
         sizeof(dgs_line_extraction_round), offsetof(dgs_line_extraction_round, emitted));
  return 0;
}'''
    with tempfile.TemporaryDirectory() as d:
        cfile = os.path.join(d, "t.c")
        open(cfile, "w").write(src)
        exe = os.path.join(d, "t")
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), cfile, "-o", exe])   # the header is plain C
        vals = [int(x) for x in subprocess.check_output([exe]).split()]
    P, F, Rd = L.LineExtractionParams, L.LineFeatureC, L.LineExtractionRound
    assert vals == [C.sizeof(P), P.cluster_tolerance.offset, P.merror_threshold.offset, P.sac_method_type.offset, P.record_lists.offset,
                    C.sizeof(F), F.mean_error.offset, C.sizeof(Rd), Rd.emitted.offset]


def test_defaults_are_the_constructor_defaults():
    """line_based_scanmatcher.hpp:80-89."""
    from delta_graph_slam_amd.line_extraction import params_from_dict
    p = params_from_dict()
    assert p.struct_size == C.sizeof(type(p))
    assert (p.min_cluster_size, p.max_cluster_size, p.max_iterations, p.sac_method_type) == (25, 25000, 500, 0)
    assert p.cluster_tolerance == 1.0 and p.sac_distance_threshold == np.float32(0.1) and p.merror_threshold == 150.0 and p.line_length_threshold == 1.0
    assert (p.sample_good_any_axis, p.sqnorm_order, p.cluster_inclusive, p.record_lists) == (1, 0, 1, 0) and p.max_rounds > 0
    for k, v in R.DEFAULTS.items():
        assert getattr(p, k) == (np.float32(v) if isinstance(v, float) else v), k
    q = params_from_dict({"delta_MinClusterSize": 40, "delta_ClusterTolerance": 1.5, "delta_Max_iterations": 100, "delta_Merror_threshold": 0.1,
                          "delta_lenght_threshold": 1.5, "delta_SACMethodType": "SAC_MSAC"})
    assert (q.min_cluster_size, q.max_iterations, q.sac_method_type) == (40, 100, 2) and q.cluster_tolerance == 1.5
    assert params_from_dict({"delta_SACMethodType": "NO_SUCH"}).sac_method_type == 0
    with pytest.raises(KeyError):
        params_from_dict({"min_cluster": 3})


def test_other_sac_methods_and_bad_struct_size_are_rejected_without_a_device():
    from delta_graph_slam_amd import _lib as L
    from delta_graph_slam_amd.line_extraction import params_from_dict
    lib = L.load()
    pts = np.zeros((30, 4), np.float32)
    out = (L.LineFeatureC * 4)()
    m, st = C.c_int64(0), C.c_int32(0)

    def call(p):
        return lib.dgs_line_extraction(None, C.byref(p), pts.ctypes.data_as(C.c_void_p), 30, 0, None, 0, C.cast(out, C.c_void_p), 4, C.byref(m), C.byref(st))

    for method in range(1, 7):
        assert call(params_from_dict({"sac_method_type": method})) == 1
    p = params_from_dict()
    p.struct_size = 12
    assert call(p) == 1
    assert call(params_from_dict({"sqnorm_order": 3})) == 1
    assert call(params_from_dict()) == 1                      # a NULL handle, with good parameters
    assert lib.dgs_line_extraction_params_init(None) == 1
    n = C.c_int64(0)
    assert lib.dgs_line_extraction_get_rounds(None, None, 0, C.byref(n), -1, None, None, None) == 1


def test_adapter_driver_reads_the_nodelet_parameters(tmp_path):
    exe = str(tmp_path / "line_extraction_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "tests", "stub_pcl"), "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "line_extraction_driver.cpp"), "-o", exe,
                           os.path.join(ROOT, "delta_graph_slam_amd", "libdgs_reg.so"), "-Wl,-rpath," + os.path.join(ROOT, "delta_graph_slam_amd"),
                           "-Wl,-rpath,/opt/rocm/lib"])
    d = json.loads(subprocess.check_output([exe, "params"]).decode())
    d["sac_distance_threshold"] = float(np.float32(d["sac_distance_threshold"]))     # printed with 9 digits: the float it names
    assert d == dict(min_cluster_size=25, max_cluster_size=25000, cluster_tolerance=1.0, sac_distance_threshold=float(np.float32(0.1)),
                     max_iterations=500, merror_threshold=150.0, line_length_threshold=1.0, sac_method_type=0)
    d = json.loads(subprocess.check_output([exe, "params", "delta_MinClusterSize=40", "delta_ClusterTolerance=1.5", "delta_Max_iterations=100",
                                            "delta_Merror_threshold=0.1", "delta_lenght_threshold=1.5", "delta_SACMethodType=SAC_LMEDS"]).decode())
    assert (d["min_cluster_size"], d["max_iterations"], d["sac_method_type"], d["cluster_tolerance"]) == (40, 100, 1, 1.5)
