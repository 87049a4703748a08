"""-m gpu: dgs_line_extraction (delta_graph_slam_amd/csrc/line_extraction.hip) at the edges of its kernels, against the numpy restatement
tests/line_extraction_reference.py.  The scenes and the kernel line each one aims at: tests/line_extraction_edge_cases.py (proved on the
CPU by tests/test_line_extraction_edge_cases_cpu.py).

  * every case: status, round trace and the inlier and cluster index lists of every round equal, the lines' doubles within EDGE_TOL
    (4 x the measured spread of the restatement's own trigonometry over the cases, which is 0: they are compared exactly);
  * draw lists: the number of relaunched rounds is the planned one -- two for `regrow_twice`, none where no list should grow;
  * history: one handle after large, small and large clouds gives each the bits of a fresh handle."""
import numpy as np
import pytest

import line_extraction_edge_cases as E
import line_extraction_reference as R
import test_line_extraction_gpu as G
from test_line_extraction_edge_cases_cpu import EDGE_TOL

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def reg():
    from delta_graph_slam_amd.registration import Registration
    return Registration("NDT_OMP", device=0)


def _compare(ex, lines, ref, monkeypatch):
    monkeypatch.setattr(G, "TOL", EDGE_TOL)                  # the comparison of test_line_extraction_gpu with this file's tolerance
    G._compare(ex, lines, ref)


@pytest.mark.parametrize("name", E.NAMES)
def test_edge_case(reg, name, monkeypatch):
    c = E.case(name)
    print(name, "--", c.aims)
    ex, lines = G._extract(reg, c.cloud, c.params, c.raw)
    ref = E.reference(name)
    _compare(ex, lines, ref, monkeypatch)
    if not lines:
        print("max |difference| -- (no line emitted)")
    launched, rounds = ex.counts()["rounds_launched"], len(ex.rounds())
    print("rounds", rounds, "launched", launched)
    if name == "regrow_twice":
        assert launched >= rounds + 2
    assert launched == c.plan.get("launched", rounds + c.plan.get("relaunches", 0))


def _result(ex, lines):
    rounds = ex.rounds()
    lists = [ex.round_lists(k, r["inliers"], r["cluster"]) for k, r in enumerate(rounds) if r["sample"][0] >= 0]
    doubles = [np.concatenate([l.pointA, l.pointB, [l.mean_error, l.std_sigma, l.max_error, l.min_error]]) for l in lines]
    return ex.status, rounds, lists, doubles


def _same_result(a, b):
    return (a[0] == b[0] and a[1] == b[1] and len(a[2]) == len(b[2]) and len(a[3]) == len(b[3])
            and all(np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) for x, y in zip(a[2], b[2]))
            and all(np.array_equal(x.view(np.uint64), y.view(np.uint64)) for x, y in zip(a[3], b[3])))


def test_a_used_handle_gives_the_bits_of_a_fresh_one(monkeypatch):
    from delta_graph_slam_amd.line_extraction import LineExtractor
    from delta_graph_slam_amd.registration import Registration
    big, small = E.case("chunk_and_tile"), E.case("n2_min2")
    lib_cloud, lib_prm = R.size_scene(4099, 100)
    jobs = [("chunk_and_tile", big.cloud, big.params, big.raw), ("n2_min2", small.cloud, small.params, small.raw),
            ("n4099_it100", lib_cloud, lib_prm, None), ("chunk_and_tile again", big.cloud, big.params, big.raw)]
    used = Registration("NDT_OMP", device=0)
    for what, cloud, prm, raw in jobs:
        ex = LineExtractor(dict(prm, record_lists=1), registration=used)      # ln.sac.perm, mt_raw and every buffer are the handle's
        got = _result(ex, ex.extract(cloud, rng_raw=raw))
        fresh, lines = G._extract(Registration("NDT_OMP", device=0), cloud, prm, raw)
        assert _same_result(got, _result(fresh, lines)), what
        assert len(got[1]) > 0 and got[0] in ("DONE", "MAX_ROUNDS"), what
    # and the last one is still the restatement's
    _compare(ex, ex.extract(big.cloud, rng_raw=big.raw), E.reference("chunk_and_tile"), monkeypatch)
