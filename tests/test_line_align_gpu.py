"""dgs_line_align_global on the device against the numpy restatement (tests/line_align_reference.py): gate codes and the survivor order
exactly, per-hypothesis fitness and scores and the final record within TOL (test_line_align_cpu.py: 4 x the measured spread of the
restatement under a +-1 ulp nudge of its trigonometry).  Hypotheses whose decisions change under that nudge may be left out of the exact
comparison (at most 2 % of a scene, never the winner; no scene has one)."""
import json
import os
import subprocess

import numpy as np
import pytest

import line_align_reference as R
from test_line_align_cpu import NUDGE_SEED, TOL, UNSTABLE_CAP, _arr, _lines

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def reg():
    from delta_graph_slam_amd.registration import Registration
    return Registration("NDT_OMP", device=0)


def _close(got, want, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    same = (got == want) | (np.isnan(got) & np.isnan(want))
    with np.errstate(all="ignore"):
        err = np.where(same, 0.0, np.abs(got - want))
    print(what, "max |difference|", float(np.max(err, initial=0.0)))
    assert np.all(err <= TOL), (what, got[err > TOL][:4], want[err > TOL][:4])


def _run(reg, name):
    from delta_graph_slam_amd.line_align import LineScanMatcher
    src, trg, kw = R.scenes()[name]
    m = LineScanMatcher(kw.get("params"), registration=reg)
    res = m.align_global(_lines(src), _lines(trg), kw.get("constrain_angle", False), kw.get("max_range", np.inf))
    return m, res


def _compare(m, res, name):
    ref, ref2 = R.scene_result(name), R.scene_result(name, NUDGE_SEED)
    unstable = R.compare_runs(ref, ref2)[0]
    H = ref["gate"].size
    assert unstable.size <= UNSTABLE_CAP * H and ref["winner"] not in unstable
    stable = np.ones(H, bool)
    stable[unstable] = False
    c = m.counts()
    print(name, "hypotheses", c["hypotheses"], "survivors", c["survivors"], "launches", c["launches"], "host waits", c["host_waits"],
          "winner", res.winner, ref["winner"], "refine", res.refine_steps, ref["refine_steps"], "status", res.status)
    assert c["hypotheses"] == H == res.counts["hypotheses"] and c["host_waits"] == 1
    assert res.counts["edges_source"] == ref["edges_source"].shape[0] and res.counts["edges_target"] == ref["edges_target"].shape[0]
    assert res.counts["lines_target"] == ref["lines_target"].shape[0]
    if H:
        hy = m.hypotheses()
        assert np.array_equal(hy["gate"][stable], ref["gate"][stable])
        if not unstable.size:
            assert c["survivors"] == ref["survivors"].size
            want_slot = np.full(H, -1)
            want_slot[ref["survivors"]] = np.arange(ref["survivors"].size)
            assert np.array_equal(hy["slot"], want_slot)                    # the survivors, compacted in h order
        ok = stable & (ref["gate"] == R.GATE_PASS)
        assert np.array_equal(np.diff(hy["slot"][hy["slot"] >= 0]) > 0, np.ones(max(c["survivors"] - 1, 0), bool))
        _close(hy["rotation"][stable], ref["rotation"][stable], "rotation")
        _close(hy["translation"][stable], ref["translation"][stable], "translation")
        _close(hy["fitness"][ok], ref["fitness"][ok], "fitness")
        _close(hy["score"][ok], ref["score"][ok], "score")
        assert np.all(hy["score"][hy["gate"] != 0] == 0.0)
        if res.winner >= 0:
            assert not np.isnan(hy["score"][res.winner]) and hy["score"][res.winner] > ref["base_score"] - TOL
            best = np.nanmax(hy["score"][hy["gate"] == 0])
            assert hy["score"][res.winner] == best and res.winner == np.nonzero((hy["gate"] == 0) & (hy["score"] == best))[0][0]
    if R.winner_margin(ref) > TOL and (ref["winner"] >= 0 or not H or ref["survivors"].size == 0
                                        or np.nanmax(ref["score"][ref["survivors"]]) < ref["base_score"] - TOL):
        assert res.winner == ref["winner"]
    assert res.refine_steps == ref["refine_steps"]
    _close(res.transformation, ref["transformation"], "final transformation")
    f = res.fitness_score
    _close([f.real_avg_distance, f.avg_distance, f.coverage, f.coverage_percentage], ref["fitness_final"], "final fitness")
    _close(res.score, ref["score_final"], "final score")
    _close(_arr(res.aligned_lines), ref["aligned_lines"], "aligned lines")
    assert np.array_equal(_arr(res.not_aligned_lines), R.scenes()[name][0])
    for a, b in zip(res.aligned_lines, res.not_aligned_lines):
        assert (a.mean_error, a.std_sigma, a.max_error, a.min_error) == (b.mean_error, b.std_sigma, b.max_error, b.min_error)
    return ref


@pytest.mark.parametrize("name", list(R.scenes()))
def test_scene_against_the_restatement(reg, name):
    m, res = _run(reg, name)
    ref = _compare(m, res, name)
    want = ("ALIGNED" if res.winner >= 0 else "NO_HYPOTHESES" if not ref["gate"].size else "ALL_GATED" if not ref["survivors"].size
            else "NONE_BETTER")
    assert res.status == want


def test_statuses_and_identity_results(reg):
    for name, status in (("lt1", "NO_HYPOTHESES"), ("ls0", "NO_HYPOTHESES"), ("all_gated", "ALL_GATED"), ("in_place", "NONE_BETTER")):
        m, res = _run(reg, name)
        assert res.status == status and res.winner == -1
        if name != "lt1":
            assert res.refine_steps == 0 and np.array_equal(res.transformation, np.eye(4))
            assert np.array_equal(_arr(res.aligned_lines), R.scenes()[name][0])
    m, res = _run(reg, "short_range")                        # no line of the unaligned source counts: the baseline item's record
    hy = m.hypotheses()
    none_counted = R.scene_result("short_range")["fitness"][:, 0] == R.DBL_MAX
    assert none_counted.any() and np.all(hy["fitness"][none_counted, 0] == R.DBL_MAX)


def test_equal_scores_go_to_the_lower_hypothesis(reg):
    m, res = _run(reg, "ties")
    hy = m.hypotheses()
    w = res.winner
    twins = [h for h in range(hy["gate"].size) if h != w and hy["gate"][h] == 0 and np.array_equal(hy["rotation"][h], hy["rotation"][w])
             and np.array_equal(hy["translation"][h], hy["translation"][w]) and hy["score"][h] == hy["score"][w]]
    assert w >= 0 and twins and min(twins) > w


def test_tie_rule_changes_the_record_on_the_device_and_in_the_refinement(reg):
    """At the exactly aligned hypothesis of `ties` one source line is equally far from two target lines with different records."""
    lo, hi = R.scene_result("ties"), R.scene_result("ties_high")
    w = lo["winner"]
    m, res = _run(reg, "ties")
    a = m.hypotheses()
    m2, res2 = _run(reg, "ties_high")
    b = m2.hypotheses()
    assert np.array_equal(a["rotation"][w], [1.0, 0.0, 0.0, 1.0]) and np.array_equal(a["translation"][w], [1.5, 0.75, 0.0])   # exact: no rounding in it
    assert np.array_equal(a["fitness"][w], lo["fitness"][w]) and np.array_equal(b["fitness"][w], hi["fitness"][w])
    assert not np.array_equal(a["fitness"][w], b["fitness"][w])
    _compare(m2, res2, "ties_high")
    f, g = res.fitness_score, res2.fitness_score
    assert (f != g or not np.array_equal(res.transformation, res2.transformation)) == \
        (not np.array_equal(lo["fitness_final"], hi["fitness_final"]) or not np.array_equal(lo["transformation"], hi["transformation"]))


def test_nan_scores_never_win_and_a_nan_baseline_is_never_beaten(reg):
    m, res = _run(reg, "nan_scores")
    hy = m.hypotheses()
    ref = R.scene_result("nan_scores")
    s = ref["survivors"]
    assert np.array_equal(np.isnan(hy["score"][s]), np.isnan(ref["score"][s])) and np.isnan(hy["score"][s]).any()
    assert res.winner == -1 and res.status == "NONE_BETTER" and res.score == -np.inf
    m, res = _run(reg, "nan_baseline")
    hy = m.hypotheses()
    assert (hy["score"][hy["gate"] == 0] == np.inf).any()
    assert res.winner == -1 and res.status == "NONE_BETTER" and np.isnan(res.score)


def test_limits_are_errors_not_truncations(reg):
    from delta_graph_slam_amd import _lib as L
    from delta_graph_slam_amd.line_align import LineScanMatcher
    m = LineScanMatcher(registration=reg)
    many = np.array([R.seg(0.0, 3.0 * k, 5.0, 3.0 * k) for k in range(257)])
    with pytest.raises(L.DgsError, match="DGS_LA_MAX_LINES_SOURCE"):
        m.align_global(_lines(many), _lines(many[:4]))
    many = np.array([R.seg(0.0, 3.0 * k, 5.0, 3.0 * k) for k in range(513)])
    with pytest.raises(L.DgsError, match="DGS_LA_MAX_LINES_TARGET"):
        m.align_global(_lines(many[:4]), _lines(many))
    bad = many[:4].copy()
    bad[1, 0, 0] = np.inf
    with pytest.raises(L.DgsError, match="finite"):
        m.align_global(_lines(bad), _lines(many[:4]))
    with pytest.raises(L.DgsError, match="DGS_LA_MAX_HYPOTHESES"):
        m.align_global(_lines(R.grid(16, 16, seed=1)), _lines(R.grid(100, 100, seed=2)))


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


def test_cloud_in_and_line_list_in_give_the_same_record(reg, flat):
    import line_extraction_reference as LR
    from delta_graph_slam_amd.line_align import LineScanMatcher
    from delta_graph_slam_amd.line_extraction import LineExtractor
    prm = dict(LR.LAUNCH, max_rounds=8)
    lines = LineExtractor(prm, registration=reg).extract(flat)
    assert len(lines) >= 2
    trg = _lines(R.move(_arr(lines), 0.3, -0.2, np.deg2rad(2.0))) + _lines(R.ring(8, seed=2))
    m = LineScanMatcher(dict(prm, delta_global_coverage_weight=1.0), registration=reg)
    a = m.align_global(flat, trg)
    b = m.align_global(lines, trg)
    c = m.align_global(flat.cpu().numpy(), trg)
    for x in (b, c):
        assert np.array_equal(a.transformation, x.transformation) and a.fitness_score == x.fitness_score and a.winner == x.winner
        assert np.array_equal(_arr(a.aligned_lines), _arr(x.aligned_lines)) and np.array_equal(_arr(a.not_aligned_lines), _arr(x.not_aligned_lines))
    ref = R.align_global(_arr(lines), _arr(trg))
    _close(a.transformation, ref["transformation"], "transformation from a cloud")
    # no lines come out of an empty cloud: the identity with the empty score, as upstream falls through
    e = m.align_global(np.zeros((0, 4), np.float32), trg)
    assert e.status == "NO_HYPOTHESES" and not e.aligned_lines and e.fitness_score.real_avg_distance == R.DBL_MAX


def test_registration_and_line_extraction_on_the_same_handle_are_untouched():
    import torch
    import line_extraction_reference as LR
    from delta_graph_slam_amd import synth
    from delta_graph_slam_amd.line_align import LineScanMatcher
    from delta_graph_slam_amd.line_extraction import LineExtractor
    from delta_graph_slam_amd.registration import Registration
    tgt, src, _ = synth.planar_pair(n=4096)
    ssrc, strg, _ = R.scenes()["lt65"]

    def run(with_align):
        reg = Registration("NDT_OMP", device=0, ndt_resolution=1.0)
        reg.setInputTarget(torch.from_numpy(tgt).cuda())
        reg.setInputSource(torch.from_numpy(src).cuda())
        ex = LineExtractor(dict(max_iterations=20, max_rounds=3), registration=reg)
        ex.extract(LR.size_scene(1500, 100)[0])
        rounds = ex.rounds()
        if with_align:
            LineScanMatcher(registration=reg).align_global(_lines(ssrc), _lines(strg))
            assert ex.rounds() == rounds
        reg.align()
        T = reg.getFinalTransformation().copy()
        fit = reg.getFitnessScore()
        if with_align:
            LineScanMatcher(registration=reg).align_global(_lines(ssrc), _lines(strg))
            assert np.array_equal(T, reg.getFinalTransformation()) and fit == reg.getFitnessScore() and ex.rounds() == rounds
        return T, fit, reg.last_result.iterations

    a, b = run(False), run(True)
    assert np.array_equal(a[0], b[0]) and a[1] == b[1] and a[2] == b[2]


def test_cpp_driver_equals_the_python_call(reg, tmp_path):
    from delta_graph_slam_amd.line_align import LineScanMatcher
    exe = str(tmp_path / "line_align_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "line_align_driver.cpp"),
                           "-o", exe, os.path.join(ROOT, "delta_graph_slam_amd", "libdgs_reg.so"),
                           "-Wl,-rpath," + os.path.join(ROOT, "delta_graph_slam_amd"), "-Wl,-rpath,/opt/rocm/lib"])
    out = json.loads(subprocess.check_output([exe, "params", "delta_global_transform_weight=0.25"], timeout=60).decode().splitlines()[-1])
    assert out["g_transform_weight"] == 0.25 and out["g_avg_distance_weight"] == 1.5 and out["g_max_score_distance"] == 3.5   # the nodelet's defaults
    src, trg, _ = R.scenes()["angle_off"]
    sp, tp, op = (str(tmp_path / n) for n in ("src.bin", "trg.bin", "out.bin"))
    src.tofile(sp)
    trg.tofile(tp)
    nodelet = dict(g_avg_distance_weight=1.5, g_coverage_weight=0.5, g_transform_weight=0.5, g_max_score_distance=3.5, g_max_score_translation=3.5)
    for constrain in (0, 1):
        res = json.loads(subprocess.check_output([exe, "run", sp, tp, op, str(constrain), "inf"], timeout=120).decode().splitlines()[-1])
        py = LineScanMatcher(nodelet, registration=reg).align_global(_lines(src), _lines(trg), bool(constrain))
        got = np.fromfile(op, np.float64)
        f = py.fitness_score
        want = np.concatenate([py.transformation.ravel(), [f.real_avg_distance, f.avg_distance, f.coverage, f.coverage_percentage],
                               _arr(py.aligned_lines).ravel()])
        assert res["ok"] and res["winner"] == py.winner and res["refine_steps"] == py.refine_steps and res["hypotheses"] == py.counts["hypotheses"]
        assert np.array_equal(got, want)                     # bit for bit
    # a failure the caller can fall back on: too many source lines
    np.array([R.seg(0.0, 3.0 * k, 5.0, 3.0 * k) for k in range(300)]).tofile(sp)
    res = json.loads(subprocess.check_output([exe, "run", sp, tp, op, "0", "inf"], timeout=120).decode().splitlines()[-1])
    assert not res["ok"] and "DGS_LA_MAX_LINES_SOURCE" in res["error"]
