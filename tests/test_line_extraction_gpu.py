"""dgs_line_extraction on the device against the numpy restatement (tests/line_extraction_reference.py): the round trace and the inlier
and cluster index lists of every round exactly, the emitted lines' doubles within TOL (test_line_extraction_cpu.py: 4 x the measured
spread of the restatement's own trigonometry, which is 0 on these scenes -- the doubles are compared exactly)."""
import json
import os
import subprocess

import numpy as np
import pytest

import line_extraction_reference as R
from test_line_extraction_cpu import TOL

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def reg():
    from delta_graph_slam_amd.registration import Registration
    return Registration("NDT_OMP", device=0)


def _extract(reg, cloud, prm, raw=None):
    from delta_graph_slam_amd.line_extraction import LineExtractor
    ex = LineExtractor(dict(prm, record_lists=1), registration=reg)
    lines = ex.extract(cloud, rng_raw=raw)
    return ex, lines


def _compare(ex, lines, ref):
    rlines, rrounds, rstatus = ref
    rounds = ex.rounds()
    print("device", ex.status, [(r["n_before"], r["draws"], r["iterations"], r["sample"], r["inliers"], r["cluster"], r["emitted"]) for r in rounds])
    print("restatement", rstatus, [(r["n_before"], r["draws"], r["iterations"], r["sample"], r["inliers"], r["cluster"], r["emitted"]) for r in rrounds])
    assert ex.status == rstatus
    assert len(rounds) == len(rrounds)
    for k, (a, b) in enumerate(zip(rounds, rrounds)):
        assert a == {key: b[key] for key in a}, (k, a)
        if b["sample"][0] >= 0:
            il, cl = ex.round_lists(k, a["inliers"], a["cluster"])
            assert np.array_equal(il, b["inlier_idx"]) and np.array_equal(cl, b["cluster_idx"]), k
    assert len(lines) == len(rlines)
    for a, b in zip(lines, rlines):
        got = np.concatenate([a.pointA, a.pointB, [a.mean_error, a.std_sigma, a.max_error, a.min_error]])
        want = np.concatenate([b["A"], b["B"], [b["mean"], b["sigma"], b["max"], b["min"]]])
        print("max |difference|", float(np.abs(got - want).max()))
        assert np.all(np.abs(got - want) <= TOL), (got, want)


@pytest.mark.parametrize("max_iterations", R.ITERATIONS)
@pytest.mark.parametrize("n", R.SIZES)
def test_sizes_and_iterations(reg, n, max_iterations):
    cloud, prm = R.size_scene(n, max_iterations)
    ex, lines = _extract(reg, cloud, prm)
    _compare(ex, lines, R.cached(f"n{n}_it{max_iterations}", cloud, prm))
    c = ex.counts()
    assert c["rounds_launched"] == len(ex.rounds())       # no round needed a longer draw list


@pytest.mark.parametrize("order", [0, 1, 2])
def test_nonflat_input_under_each_norm_order(reg, order):
    cloud, prm = R.nonflat_scene()
    prm = dict(prm, sqnorm_order=order)
    ex, lines = _extract(reg, cloud, prm)
    assert len(lines) >= 3
    _compare(ex, lines, R.cached(f"nonflat{order}" if order else "nonflat", cloud, prm))


def _dup_cloud():
    cloud = R.scene(200, segments=1, seed=3, clutter=0.2)
    cloud[::2] = cloud[0]                                    # every second point is one and the same point
    return cloud


def test_caller_stream_with_repeated_and_bad_samples(reg):
    cloud = _dup_cloud()
    raw = np.random.default_rng(5).integers(0, 2**31, 4000, dtype=np.uint32)
    raw[:8] = 0                                              # four times the sample (0, 1)
    prm = dict(max_iterations=20, max_rounds=3, min_cluster_size=10)
    ex, lines = _extract(reg, cloud, prm, raw)
    ref = R.line_extraction(cloud, prm, raw)
    assert ref[1][0]["draws"] > ref[1][0]["iterations"] > 4  # bad samples were skipped
    _compare(ex, lines, ref)


def test_caller_stream_that_runs_out(reg):
    cloud = _dup_cloud()
    raw = np.zeros(6, np.uint32)                             # three draws of (0, 1) for up to 101 hypotheses
    prm = dict(max_iterations=100)
    ex, lines = _extract(reg, cloud, prm, raw)
    assert ex.status == "RNG_EXHAUSTED" and not lines
    _compare(ex, lines, R.line_extraction(cloud, prm, raw))


def test_thousand_bad_draws_fail_the_round(reg):
    cloud = np.tile(np.array([[1.5, -2.0, 0.0, 1.0]], np.float32), (40, 1))
    raw = np.random.default_rng(6).integers(0, 2**31, 2400, dtype=np.uint32)
    for r, prm in ((raw, dict(max_iterations=10)), (None, dict(max_iterations=10))):
        ex, lines = _extract(reg, cloud, prm, r)
        assert ex.status == "RANSAC_FAILED" and not lines
        assert ex.rounds() == [dict(n_before=40, draws=1000, iterations=0, sample=(-1, -1), inliers=0, cluster=0, emitted=0)]
        _compare(ex, lines, R.line_extraction(cloud, prm, r))
    # the recalled PCL 1.10 rule never accepts a sample of a flattened cloud
    cloud, prm = R.size_scene(64, 1)
    ex, lines = _extract(reg, cloud, dict(prm, sample_good_any_axis=0))
    assert ex.status == "RANSAC_FAILED" and ex.rounds()[0]["draws"] == 1000


def _two_runs_on_a_line():
    x = np.concatenate([np.arange(30) * 0.1, 10.0 + np.arange(30) * 0.1])
    cloud = np.zeros((60, 4), np.float32)
    cloud[:, 0] = x
    cloud[:, 3] = 1
    cloud[[0, 45]] = cloud[[45, 0]]                          # the lowest position belongs to the second run
    return cloud


def test_equal_top_clusters_go_to_the_lowest_position(reg):
    cloud = _two_runs_on_a_line()
    prm = dict(max_iterations=5, max_rounds=2)
    ex, lines = _extract(reg, cloud, prm)
    r0 = ex.rounds()[0]
    assert r0["inliers"] == 60 and r0["cluster"] == 30
    il, cl = ex.round_lists(0, 60, 30)
    assert cl[0] == 0 and np.all(cloud[cl, 0] >= 3.0 - 1e-6)
    _compare(ex, lines, R.line_extraction(cloud, prm))


def test_oversized_clusters_stall(reg):
    cloud = _two_runs_on_a_line()
    prm = dict(max_iterations=5, max_cluster_size=20)
    ex, lines = _extract(reg, cloud, prm)
    assert ex.status == "STALL" and not lines and len(ex.rounds()) == 1 and ex.rounds()[0]["cluster"] == 0
    _compare(ex, lines, R.line_extraction(cloud, prm))


@pytest.fixture(scope="module")
def flat(reg):
    import torch
    from delta_graph_slam_amd import synth
    from delta_graph_slam_amd.prefilter import Prefilter
    import prefilter_reference as PR
    xyz, _ = synth.street_scan((-30.0, 1.0, 0.1), 16, (15.0, -15.0), 1875, 21)
    scan = np.concatenate([xyz, np.ones((xyz.shape[0], 1))], 1).astype(np.float32)
    _, f2, _ = Prefilter(PR.LAUNCH, registration=reg).filter_scan(torch.from_numpy(scan).cuda())
    return f2


def test_device_tensor_straight_from_the_prefilter(reg, flat):
    assert flat.is_cuda and flat.shape[0] > 500
    prm = dict(R.LAUNCH, max_rounds=6)
    before = flat.clone()
    ex, lines = _extract(reg, flat, prm)
    rounds_dev = ex.rounds()
    host = flat.cpu().numpy()
    assert np.array_equal(before.cpu().numpy(), host)        # the input is not modified
    ex2, lines2 = _extract(reg, host, prm)
    assert rounds_dev == ex2.rounds() and len(lines) == len(lines2)
    for a, b in zip(lines, lines2):
        assert np.array_equal(a.pointA, b.pointA) and np.array_equal(a.pointB, b.pointB) and a.mean_error == b.mean_error
    _compare(ex, lines, R.line_extraction(host, prm))


def test_registration_on_the_same_handle_is_untouched():
    import torch
    from delta_graph_slam_amd import synth
    from delta_graph_slam_amd.line_extraction import LineExtractor
    from delta_graph_slam_amd.registration import Registration
    tgt, src, _ = synth.planar_pair(n=4096)

    def run(with_extraction):
        reg = Registration("NDT_OMP", device=0, ndt_resolution=1.0)
        reg.setInputTarget(torch.from_numpy(tgt).cuda())
        reg.setInputSource(torch.from_numpy(src).cuda())
        if with_extraction:
            LineExtractor(dict(max_iterations=20, max_rounds=3), registration=reg).extract(R.size_scene(1500, 100)[0])
        reg.align()
        T = reg.getFinalTransformation().copy()
        fit = reg.getFitnessScore()
        if with_extraction:
            LineExtractor(dict(max_iterations=20, max_rounds=3), registration=reg).extract(R.size_scene(257, 100)[0])
            assert np.array_equal(T, reg.getFinalTransformation()) and fit == reg.getFitnessScore()
        return T, fit, reg.last_result.iterations

    a, b = run(False), run(True)
    assert np.array_equal(a[0], b[0]) and a[1] == b[1] and a[2] == b[2]


def test_cpp_driver_on_a_dumped_scene(reg, tmp_path):
    exe = str(tmp_path / "line_extraction_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "tests", "stub_pcl"), "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "line_extraction_driver.cpp"), "-o", exe,
                           os.path.join(ROOT, "delta_graph_slam_amd", "libdgs_reg.so"), "-Wl,-rpath," + os.path.join(ROOT, "delta_graph_slam_amd"),
                           "-Wl,-rpath,/opt/rocm/lib"])
    cloud, _ = R.size_scene(1500, 100)
    inp, out = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    cloud.tofile(inp)
    res = json.loads(subprocess.check_output([exe, "run", inp, out, "delta_Max_iterations=100", "delta_MinClusterSize=300"], timeout=120).decode().splitlines()[-1])
    prm = dict(max_iterations=100, min_cluster_size=300)
    ex, lines = _extract(reg, cloud, prm)
    got = np.fromfile(out, np.float64).reshape(-1, 10)
    assert res["lines"] == len(lines) == got.shape[0] == 2 and res["status"] == 0 and ex.status == "DONE"
    for g, l in zip(got, lines):
        assert np.array_equal(g, np.concatenate([l.pointA, l.pointB, [l.mean_error, l.std_sigma, l.max_error, l.min_error]]))
    # an unserved method: an empty vector and a reason, for the caller to fall back on
    res = json.loads(subprocess.check_output([exe, "run", inp, out, "delta_SACMethodType=SAC_MSAC"], timeout=120).decode().splitlines()[-1])
    assert res["lines"] == 0 and "SAC_RANSAC" in res["error"]
