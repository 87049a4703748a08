"""dgs_line_align_local_batch on the device against the numpy restatement (tests/line_align_local_reference.py): gate codes and neighbour
ranks exactly, per-hypothesis fitness and scores of both phases and the final record within TOL_LOCAL (test_line_align_local_cpu.py: 4 x
the measured spread of the restatement under a +-1 ulp nudge of its trigonometry), winners wherever the restatement's margin exceeds
TOL_LOCAL.  Hypotheses whose decisions change under that nudge may be left out of the exact comparison (at most 2 % of a scene, never a
winner; no scene has one).  Every item of the 33-item batch equals the same item run alone bit for bit."""
import numpy as np
import pytest

import line_align_local_reference as LR
import line_align_reference as R
from test_line_align_cpu import _arr
from test_line_align_local_cpu import NUDGE_SEED, TOL_LOCAL, UNSTABLE_CAP

pytestmark = pytest.mark.gpu
_lines = LR.feature_lines


@pytest.fixture(scope="module")
def reg():
    from delta_graph_slam_amd.registration import Registration
    return Registration("NDT_OMP", device=0)


def _matcher(reg, params=None):
    from delta_graph_slam_amd.line_align import LineScanMatcher
    return LineScanMatcher(params, registration=reg)


def _close(got, want, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    same = (got == want) | (np.isnan(got) & np.isnan(want))
    with np.errstate(all="ignore"):
        err = np.where(same, 0.0, np.abs(got - want))
    print(what, "max |difference|", float(np.max(err, initial=0.0)))
    assert np.all(err <= TOL_LOCAL), (what, got[err > TOL_LOCAL][:4], want[err > TOL_LOCAL][:4])


def _fit(f):
    return [f.real_avg_distance, f.avg_distance, f.coverage, f.coverage_percentage]


def _compare(m, item, res, src, ref, ref2):
    """One item of the last call against the restatement."""
    un1, un2 = LR.compare_runs(ref, ref2)[:2]
    H1, H2 = ref["gate1"].size, ref["gate2"].size
    assert un1.size <= UNSTABLE_CAP * H1 and un2.size <= UNSTABLE_CAP * H2
    assert ref["winner_edge"] not in un1 and ref["winner_line"] not in un2
    c = res.counts
    print("item", item, "edge pairs", H1, "survivors", c["survivors_edge"], "winner", res.winner, ref["winner_edge"], "line pairs", H2, "survivors",
          c["survivors_line"], "winner", res.winner_line, ref["winner_line"], "status", res.status)
    assert (c["hypotheses_edge"], c["hypotheses_line"]) == (H1, H2)
    assert (c["edges_source"], c["edges_target"]) == (ref["edges_source"].shape[0], ref["edges_target"].shape[0])
    _close(_fit(res.baseline_fitness_score), ref["base_fitness"], "baseline fitness")
    _close(res.baseline_score, ref["base_score"], "baseline score")
    for phase, H, un, sfx in ((0, H1, un1, "1"), (1, H2, un2, "2")):
        if not H:
            continue
        hy = m.local_hypotheses(item, phase, 0, H)
        stable = np.ones(H, bool)
        stable[un] = False
        gate = ref["gate" + sfx]
        assert np.array_equal(hy["gate"][stable], gate[stable])
        if phase == 1:
            assert np.array_equal(hy["target"][stable], ref["target2"][stable])           # the neighbour ranks
            assert np.array_equal(np.sort(hy["target"].reshape(-1, H // src.shape[0]), axis=1),
                                  np.tile(np.arange(H // src.shape[0]), (src.shape[0], 1)))   # a permutation per line
        else:
            assert np.all(hy["target"] == -1)
        if not un.size:
            assert c["survivors_edge" if phase == 0 else "survivors_line"] == ref["survivors" + sfx].size
        moved = stable & ~np.isin(gate, (LR.GATE_LINE_DIRECTION, LR.GATE_RANK))
        _close(hy["rotation"][moved], ref["rotation" + sfx][moved], "rotation")
        _close(hy["translation"][moved], ref["translation" + sfx][moved], "translation")
        ok = stable & (gate == LR.GATE_PASS)
        _close(hy["fitness"][ok], ref["fitness" + sfx][ok], "fitness")
        _close(hy["score"][ok], ref["score" + sfx][ok], "score")
        assert np.all(hy["score"][hy["gate"] != 0] == 0.0) and np.all(hy["fitness"][hy["gate"] != 0] == 0.0)
        w, start = (res.winner, res.baseline_score) if phase == 0 else (res.winner_line, res.edge_score)
        if w >= 0:                                          # the device's own arg-max: strict, lowest index among the maxima
            best = np.nanmax(hy["score"][hy["gate"] == 0])
            assert hy["score"][w] == best > start and w == np.nonzero((hy["gate"] == 0) & (hy["score"] == best))[0][0]
        else:
            assert not np.any(hy["score"][hy["gate"] == 0] > start)
    m1, m2 = LR.margins(ref)
    if m1 > TOL_LOCAL:
        assert res.winner == ref["winner_edge"]
        if m2 > TOL_LOCAL:
            assert res.winner_line == ref["winner_line"]
    assert res.isEdgeAligned == (res.winner >= 0)
    _close(res.edge_transformation, ref["edge_transformation"], "edge transformation")
    _close(_fit(res.edge_fitness_score), ref["edge_fitness"], "edge fitness")
    _close(res.edge_score, ref["edge_score"], "edge score")
    _close(res.transformation, ref["transformation"], "final transformation")
    _close(_fit(res.fitness_score), ref["fitness_final"], "final fitness")
    _close(res.score, ref["score_final"], "final score")
    _close(_arr(res.aligned_lines), ref["aligned_lines"], "aligned lines")
    assert np.array_equal(_arr(res.not_aligned_lines), src)
    for a, b in zip(res.aligned_lines, res.not_aligned_lines):
        assert (a.mean_error, a.std_sigma, a.max_error, a.min_error) == (b.mean_error, b.std_sigma, b.max_error, b.min_error)
    want = ("ALIGNED" if res.winner >= 0 else "LINE_ALIGNED" if res.winner_line >= 0 else "NO_HYPOTHESES" if H1 + H2 == 0
            else "ALL_GATED" if c["survivors_edge"] + c["survivors_line"] == 0 else "NONE_BETTER")
    assert res.status == want


def _run(reg, name):
    src, trg, kw = LR.scenes()[name]
    m = _matcher(reg, kw.get("params"))
    res = m.align_local(_lines(src), _lines(trg), kw.get("max_range", 0.5))
    c = m.local_counts()
    assert c["host_waits"] == 1 and c["items"] == 1
    return m, res, c


@pytest.mark.parametrize("name", list(LR.scenes()))
def test_scene_against_the_restatement(reg, name):
    m, res, c = _run(reg, name)
    _compare(m, 0, res, LR.scenes()[name][0], LR.scene_result(name), LR.scene_result(name, NUDGE_SEED))


def test_scene_properties_on_the_device(reg):
    _, res, _ = _run(reg, "empty_source")
    assert res.status == "NO_HYPOTHESES" and not res.aligned_lines and np.array_equal(res.transformation, np.eye(4))
    assert res.fitness_score.avg_distance == R.DBL_MAX and res.fitness_score.coverage_percentage == 0.0
    _, res, _ = _run(reg, "one_line_each")
    assert res.counts["hypotheses_edge"] == 0 and res.counts["hypotheses_line"] == 1
    _, res, _ = _run(reg, "corner")
    assert res.isEdgeAligned and res.status == "ALIGNED"
    _, res, _ = _run(reg, "angular_dist")
    assert res.counts["edges_source"] == 0 and res.counts["edges_target"] == 4
    _, res, _ = _run(reg, "case4_crossing")
    assert res.counts["edges_source"] == 4 and res.counts["edges_target"] == 4
    _, res, _ = _run(reg, "refine_only")
    assert res.counts["survivors_edge"] == 0 and res.winner_line >= 0 and res.status == "LINE_ALIGNED" and not res.isEdgeAligned
    _, res, _ = _run(reg, "refine_rank")
    assert res.winner_line % res.counts["hypotheses_line"] >= 1 and res.winner_line == 1
    m, res, _ = _run(reg, "refine_on_winner")
    assert res.winner >= 0 and res.winner_line >= 0 and res.score > res.edge_score
    step = m.local_hypotheses(0, 1, res.winner_line, 1)
    T2 = R._mat(step["rotation"][0], step["translation"][0])
    assert np.array_equal(res.transformation, R._compose(res.edge_transformation, T2))      # best_trans * transform, the same operations
    src = LR.scenes()["refine_on_winner"][0]
    te = res.edge_transformation
    snap = R.transform_lines(src, te[None, :2, :2].reshape(1, 4), te[None, :3, 3])[0]
    assert np.array_equal(_arr(res.aligned_lines), R.transform_lines(snap, step["rotation"], step["translation"])[0])
    for name in ("nan_scores", "nan_baseline"):
        _, res, _ = _run(reg, name)
        assert res.winner == -1 and res.winner_line == -1 and res.status == "NONE_BETTER" and res.counts["survivors_line"] > 0
    assert np.isnan(res.score)


def test_three_nearest_switch_and_the_boundary_of_three(reg):
    for name, lt, skipped in (("two_targets", 2, 0), ("three_targets", 3, 0), ("five_targets", 5, 4)):
        ma, a, _ = _run(reg, name)
        ga = ma.local_hypotheses(0, 1, 0, 2 * lt)             # the hook reads the handle's last call: before the next one
        mb, b, _ = _run(reg, name + "_three")
        gb = mb.local_hypotheses(0, 1, 0, 2 * lt)
        rank = np.tile(np.arange(lt), 2)
        assert a.counts["hypotheses_line"] == b.counts["hypotheses_line"] == 2 * lt
        assert not np.any(ga["gate"] == LR.GATE_RANK) and np.count_nonzero(gb["gate"] == LR.GATE_RANK) == skipped
        assert np.all(gb["gate"][rank >= 3] == LR.GATE_RANK) and np.array_equal(ga["gate"][rank < 3], gb["gate"][rank < 3])
        assert np.array_equal(ga["target"], gb["target"]) and np.array_equal(ga["score"][rank < 3], gb["score"][rank < 3])


def test_rank_ties_follow_the_switch(reg):
    lo, hi = LR.scene_result("rank_ties"), LR.scene_result("rank_ties_high")
    differ = np.nonzero(lo["target2"] != hi["target2"])[0]
    assert differ.size
    H = lo["gate2"].size
    ma, _, _ = _run(reg, "rank_ties")
    a = ma.local_hypotheses(0, 1, 0, H)
    mb, _, _ = _run(reg, "rank_ties_high")
    b = mb.local_hypotheses(0, 1, 0, H)
    assert np.array_equal(a["target"], lo["target2"]) and np.array_equal(b["target"], hi["target2"])
    assert np.array_equal(np.nonzero(a["target"] != b["target"])[0], differ)


def _alone_equals(a, b):
    assert np.array_equal(a.transformation, b.transformation) and np.array_equal(a.edge_transformation, b.edge_transformation)
    for x, y in ((a.fitness_score, b.fitness_score), (a.edge_fitness_score, b.edge_fitness_score), (a.baseline_fitness_score, b.baseline_fitness_score)):
        assert np.array_equal(_fit(x), _fit(y), equal_nan=True)
    assert np.array_equal([a.score, a.edge_score, a.baseline_score], [b.score, b.edge_score, b.baseline_score], equal_nan=True)
    assert (a.winner, a.winner_line, a.status, a.isEdgeAligned, a.counts) == (b.winner, b.winner_line, b.status, b.isEdgeAligned, b.counts)
    assert np.array_equal(_arr(a.aligned_lines), _arr(b.aligned_lines))


def test_batch_mixed_against_the_restatement_and_against_single_calls(reg):
    items = LR.batch_mixed()
    m = _matcher(reg)
    batch = m.align_local_batch([(_lines(s), _lines(t)) for s, t in items], 0.5)
    cb = m.local_counts()
    assert cb["host_waits"] == 1 and cb["items"] == 33
    assert cb["hypotheses_edge"] == sum(LR.batch_result(b)["gate1"].size for b in range(33))
    assert cb["hypotheses_line"] == sum(s.shape[0] * t.shape[0] for s, t in items)
    hyps = []
    for b, (s, t) in enumerate(items):
        _compare(m, b, batch[b], s, LR.batch_result(b), LR.batch_result(b, NUDGE_SEED))
        hyps.append([m.local_hypotheses(b, ph, 0, n) for ph, n in ((0, batch[b].counts["hypotheses_edge"]), (1, batch[b].counts["hypotheses_line"])) if n])
    m1 = _matcher(reg)
    for b, (s, t) in enumerate(items):                       # device against device: exact
        one = m1.align_local(_lines(s), _lines(t), 0.5)
        c1 = m1.local_counts()
        assert c1["launches"] == cb["launches"] and c1["host_waits"] == 1      # launches do not depend on the number of items
        _alone_equals(batch[b], one)
        alone = [m1.local_hypotheses(0, ph, 0, n) for ph, n in ((0, one.counts["hypotheses_edge"]), (1, one.counts["hypotheses_line"])) if n]
        for x, y in zip(hyps[b], alone):
            for k in x:
                assert np.array_equal(x[k], y[k], equal_nan=True), (b, k)


def test_limits_are_errors_not_truncations(reg):
    from delta_graph_slam_amd import _lib as L
    m = _matcher(reg)
    line = lambda k: R.seg(0.0, 3.0 * k, 5.0, 3.0 * k)
    few = _lines(np.array([line(k) for k in range(3)]))
    with pytest.raises(L.DgsError, match="DGS_LA_MAX_LINES_SOURCE"):
        m.align_local(_lines(np.array([line(k) for k in range(257)])), few)
    with pytest.raises(L.DgsError, match="DGS_LA_MAX_LINES_TARGET"):
        m.align_local(few, _lines(np.array([line(k) for k in range(513)])))
    with pytest.raises(L.DgsError, match="DGS_LA_MAX_ITEMS"):
        m.align_local_batch([([], [])] * 4097)
    big = (_lines(np.array([line(k) for k in range(256)])), _lines(np.array([line(k) for k in range(512)])))
    with pytest.raises(L.DgsError, match="DGS_LA_MAX_HYPOTHESES"):
        m.align_local_batch([big] * 17)                      # 17 x 256 x 512 line pairs
    bad = np.array([line(k) for k in range(3)])
    bad[1, 0, 0] = np.inf
    with pytest.raises(L.DgsError, match="finite"):
        m.align_local(_lines(bad), few)
    bad[1, 0, 0] = np.nan
    with pytest.raises(L.DgsError, match="finite"):
        m.align_local_batch([(few, few), (few, _lines(bad))])
    with pytest.raises(L.DgsError, match="max_range"):
        m.align_local(few, few, np.nan)


def test_align_global_on_the_same_handle_is_untouched(reg):
    src, trg, kw = R.scenes()["rectangle"]
    before = _matcher(reg).align_global(_lines(src), _lines(trg))
    m = _matcher(reg)
    m.align_local_batch([(_lines(s), _lines(t)) for s, t in LR.batch_mixed()], 0.5)
    after = m.align_global(_lines(src), _lines(trg))
    hy = m.hypotheses()
    assert np.array_equal(before.transformation, after.transformation) and before.fitness_score == after.fitness_score
    assert (before.winner, before.refine_steps, before.status, before.counts) == (after.winner, after.refine_steps, after.status, after.counts)
    assert np.array_equal(_arr(before.aligned_lines), _arr(after.aligned_lines))
    ref = R.scene_result("rectangle")
    assert after.winner == ref["winner"] and np.array_equal(hy["gate"], ref["gate"])
    assert np.abs(after.transformation - ref["transformation"]).max() <= 9.7e-13   # 6f's TOL


def test_cpp_driver_equals_the_python_call(reg, tmp_path):
    import json
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "line_align_local_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-I", os.path.join(root, "include"),
                           os.path.join(root, "tests", "cpp", "line_align_local_driver.cpp"), "-o", exe,
                           os.path.join(root, "delta_graph_slam_amd", "libdgs_reg.so"), "-Wl,-rpath," + os.path.join(root, "delta_graph_slam_amd"),
                           "-Wl,-rpath,/opt/rocm/lib"])
    items = LR.batch_mixed()
    ip, op = str(tmp_path / "items.bin"), str(tmp_path / "out.bin")
    LR.write_items(ip, items)
    res = json.loads(subprocess.check_output([exe, "run", ip, op, "0.5", "delta_local_transform_weight=0.15"], timeout=120).decode().splitlines()[-1])
    assert res["ok"] and res["items"] == 33, res
    nodelet = dict(l_coverage_weight=1.5, l_transform_weight=0.15, l_max_score_distance=1.0, l_max_score_translation=3.5)   # the nodelet's defaults
    py = _matcher(reg, nodelet).align_local_batch([(_lines(s), _lines(t)) for s, t in items], 0.5)
    want = np.concatenate([np.concatenate([r.transformation.ravel(), _fit(r.fitness_score), [r.score], _arr(r.aligned_lines).ravel()]) for r in py])
    assert np.array_equal(np.fromfile(op, np.float64), want)              # bit for bit
    # a failure the caller can fall back on
    many = np.array([R.seg(0.0, 3.0 * k, 5.0, 3.0 * k) for k in range(300)])
    LR.write_items(ip, [(many, many[:3])])
    res = json.loads(subprocess.check_output([exe, "run", ip, op, "0.5"], timeout=120).decode().splitlines()[-1])
    assert not res["ok"] and "DGS_LA_MAX_LINES_SOURCE" in res["error"]


def test_struct_size_guard(reg):
    """A params struct that ends at `reserved` (before align_local's members) is accepted and gets upstream's defaults: whatever sits
    behind its end is not read.  Any other size is refused with a message."""
    import ctypes as C
    from delta_graph_slam_amd import _lib as L
    src, trg, _ = LR.scenes()["refine_on_winner"]
    want = _matcher(reg).align_local(_lines(src), _lines(trg), 0.5)
    m = _matcher(reg, dict(l_coverage_weight=0.25, l_max_distance=0.1, refine_three_nearest=1))
    changed = m.align_local(_lines(src), _lines(trg), 0.5)
    assert changed.score != want.score                      # the tail matters when it is read
    old = L.LineAlignParams.l_avg_distance_weight.offset
    assert old == 72
    m.params.struct_size = old                              # the same bytes, declared to end before the tail
    _alone_equals(m.align_local(_lines(src), _lines(trg), 0.5), want)
    m.params.l_coverage_weight = -1.0                       # refused when read ...
    _alone_equals(m.align_local(_lines(src), _lines(trg), 0.5), want)
    m.params.struct_size = C.sizeof(L.LineAlignParams)
    with pytest.raises(L.DgsError, match="weight"):        # ... and read with the whole struct
        m.align_local(_lines(src), _lines(trg), 0.5)
    for size in (0, 12, old - 8, old + 8, C.sizeof(L.LineAlignParams) + 8):
        m.params.struct_size = size
        with pytest.raises(L.DgsError, match="struct_size"):
            m.align_local(_lines(src), _lines(trg), 0.5)
    m.params.struct_size = old                              # align_global takes the short struct as before
    g = m.align_global(_lines(src), _lines(trg))
    assert g.status in L.LA_STATUS.values()


def test_local_hypotheses_default_count(reg):
    m = _matcher(reg)
    res = m.align_local_batch([(_lines(s), _lines(t)) for s, t in LR.batch_mixed()[:4]], 0.5)
    for b, r in enumerate(res):
        for phase, n in ((0, r.counts["hypotheses_edge"]), (1, r.counts["hypotheses_line"])):
            assert m.local_hypotheses(b, phase)["gate"].size == n
            if n > 1:
                assert np.array_equal(m.local_hypotheses(b, phase, 1)["score"], m.local_hypotheses(b, phase, 0, n)["score"][1:])
