"""-m gpu: dgs_building_overlap_pairs and dgs_line_align_overlapped_batch (delta_graph_slam_amd/csrc/building_overlap.hip) at the edges of
their launch shapes, against the numpy restatement tests/building_overlap_reference.py.  The inputs and the edge each one hits:
tests/building_overlap_edge_cases.py, proved on the CPU by tests/test_building_overlap_edge_cases_cpu.py.

  * pair search, exactly and in order: rows of 66 words with pairs past a wave's first 64 (the count loop's second trip, the emit loop's
    second step and its carried base); a clique of 130 (a full word, a row over three words, 8385 pairs through the wrapper's second
    call, capacities that end mid-row and mid-word); planted pairs at rows 62 .. 65 and columns 127 .. 129 with B = 128, 129, 130; the
    scan at B = 255 .. 513, 4097 (17 rows a thread) and 2^14 (64 rows a thread); the last line pair of 512 x 512, no line pair at all,
    and tiles whose two rows hold 512 and 3 lines;
  * alignment, with test_building_overlap_cpu.check_alignment and TOL_OVERLAP as they stand: twins of bit-equal norm one arg-min trip
    apart and in different waves (the winner exactly), overlap decided by target lines 256 and up, 256 source lines, every unit-table
    size around 16 with empty items first, last and back to back (each item equal to the item alone bit for bit), 4096 items, and the
    item and hypothesis limits."""
import json
import os
import subprocess

import numpy as np
import pytest

import building_overlap_edge_cases as E
import building_overlap_reference as BR
from test_building_overlap_cpu import NUDGE_SEED, ROOT, check_alignment, read_align
from test_building_overlap_gpu import _features, _got, _status

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def reg():
    from delta_graph_slam_amd.registration import Registration
    return Registration("NDT_OMP", device=0)


@pytest.fixture(scope="module")
def overlap(reg):
    from delta_graph_slam_amd.building_overlap import BuildingOverlap
    return BuildingOverlap(registration=reg)


@pytest.fixture(scope="module")
def matcher(reg):
    from delta_graph_slam_amd.line_align import LineScanMatcher
    return LineScanMatcher(None, registration=reg)


def _same(a, b, what):
    """two records in _got's shape, bit for bit"""
    for k, v in a.items():
        if isinstance(v, np.ndarray):
            assert v.tobytes() == b[k].tobytes(), (what, k)
        else:
            assert v == b[k], (what, k)


# ---- pair search ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", E.PAIR_NAMES)
def test_pair_list_equals_the_restatement(overlap, name):
    bl, ce = E.pair_scenes()[name]
    ref = E.pair_result(name)
    got = overlap.overlapped_pairs(bl, ce, capacity=max(ref.shape[0], 1))
    c = overlap.counts()
    print(name, "buildings", len(bl), "pairs", got.shape[0], ref.shape[0], c)
    assert got.dtype == np.int32 and np.array_equal(got, ref)                       # exactly, order included
    assert (c["launches"], c["host_waits"], c["buildings"], c["pairs"]) == (5, 1, len(bl), ref.shape[0])


def test_dense_rows_at_every_capacity(overlap):
    from delta_graph_slam_amd._lib import DGS_ERR_CAPACITY, DgsError
    bl, ce = E.pair_scenes()["clique130"]
    ref = E.pair_result("clique130")
    assert np.array_equal(overlap.overlapped_pairs(bl, ce), ref)                    # 4 a building is too few: the wrapper's second call
    assert overlap.last_count == ref.shape[0] == 8385
    for cap in (ref.shape[0] - 1, E.position(ref, 0, 70), E.position(ref, 1, 64), E.position(ref, 1, 64) + 1):
        with pytest.raises(DgsError) as e:
            overlap.overlapped_pairs(bl, ce, capacity=cap)
        assert e.value.status == DGS_ERR_CAPACITY
        assert overlap.last_count == ref.shape[0] and np.array_equal(overlap.last_pairs, ref[:cap])   # the full count, the first `capacity` pairs
        assert overlap.counts()["pairs"] == ref.shape[0]


def test_appended_clique_leaves_the_planted_list(overlap):
    bl, ce = E.pair_scenes()["rows130"]
    more, mce = E.far(E.pair_scenes()["clique130"])
    got = overlap.overlapped_pairs(bl + more + [E.NONE], np.concatenate([ce, mce, [[0.0, 0.0, 0.0]]]))
    assert np.array_equal(got[np.all(got < 130, axis=1)], E.pair_result("rows130"))
    assert np.array_equal(got[np.all(got >= 130, axis=1)] - 130, E.pair_result("clique130"))
    assert not np.any((got[:, 0] < 130) & (got[:, 1] >= 130))


# ---- alignment ----------------------------------------------------------------------------------------------------------------------------
SCENES = {n: (lambda n=n: E.twin_item(n)) for n in E.TWIN_CASES}
SCENES.update({"past_255_Lt%d" % Lt: (lambda Lt=Lt: E.past_255(Lt)) for Lt in E.PAST_255})
SCENES.update({"source_limit_Lt%d" % Lt: (lambda Lt=Lt: E.source_limit(Lt)) for Lt in (1, 2, 257)})


@pytest.mark.parametrize("name", list(SCENES))
def test_alignment_equals_the_restatement_on_scenes(matcher, name):
    item = SCENES[name]()
    ref = E.restated(item)
    res = matcher.align_overlapped(*_features(item))
    got = _got(matcher, 0, res)
    print(name, "hypotheses", got["gate"].size, "angle passed", got["n_angle_passed"], "not overlapped", got["n_not_overlapped"], "winner", res.winner,
          ref["winner"], "norm", res.translation_norm, "status", res.status)
    check_alignment(got, ref, E.restated(item, NUDGE_SEED))
    assert res.status == _status(ref)
    c = matcher.overlapped_counts()
    assert (c["launches"], c["host_waits"], c["items"], c["hypotheses"]) == (3, 1, 1, ref["gate"].size)
    if name in E.TWIN_CASES:
        lo, hi = E.TWIN_CASES[name][2]
        assert res.winner == lo and got["tn"][lo].tobytes() == got["tn"][hi].tobytes()    # the device's twins are bit-equal too: the lower h


@pytest.fixture(scope="module")
def units(matcher):
    items = E.batch_units()
    res = matcher.align_overlapped_batch([_features(it) for it in items])
    counts = matcher.overlapped_counts()
    return items, res, [_got(matcher, b, r) for b, r in enumerate(res)], counts


def test_unit_table_batch_equals_the_restatement(units):
    items, res, got, counts = units
    assert (counts["launches"], counts["host_waits"], counts["items"], counts["hypotheses"]) == (3, 1, len(items), sum(E.UNIT_H))
    assert [g["gate"].size for g in got] == list(E.UNIT_H)
    for it, r, g in zip(items, res, got):
        ref = E.restated(it)
        check_alignment(g, ref, E.restated(it, NUDGE_SEED))
        assert r.status == _status(ref) and r.winner == ref["winner"]
    for b, h in enumerate(E.UNIT_H):
        if h == 0:
            assert res[b].status == "NO_HYPOTHESES" and res[b].is_identity and res[b].winner == -1


def test_every_unit_table_item_equals_the_item_alone_bit_for_bit(matcher, units):
    items, res, got, _ = units
    alone = []
    for b, it in enumerate(items):
        one = matcher.align_overlapped(*_features(it))
        alone.append(_got(matcher, 0, one))
        assert one.status == res[b].status
        _same(got[b], alone[b], b)
    again = matcher.align_overlapped_batch([_features(it) for it in items])
    for b in range(len(items)):                                              # each item's own records, by item
        hy = matcher.overlapped_hypotheses(b)
        for k in ("gate", "rotation", "translation", "tn"):
            assert hy[k].shape[0] == E.UNIT_H[b] and hy[k].tobytes() == alone[b][k].astype(hy[k].dtype).tobytes(), (b, k)
        if E.UNIT_H[b] > 1:
            tail = matcher.overlapped_hypotheses(b, E.UNIT_H[b] - 1, 1)
            assert tail["tn"].tobytes() == alone[b]["tn"][-1:].tobytes()
        assert again[b].winner == res[b].winner


def test_item_limit(matcher):
    from delta_graph_slam_amd._lib import DgsError
    protos = E.prototypes()
    feats = [_features(it) for it in protos]
    alone = []
    for it, f in zip(protos, feats):
        alone.append(_got(matcher, 0, matcher.align_overlapped(*f)))
        check_alignment(alone[-1], E.restated(it), E.restated(it, NUDGE_SEED))
    n = E.MAX_ITEMS
    res = matcher.align_overlapped_batch([feats[b % 8] for b in range(n)])
    c = matcher.overlapped_counts()
    assert len(res) == n and (c["launches"], c["host_waits"], c["items"]) == (3, 1, n)
    assert c["hypotheses"] == (n // 8) * sum(a["gate"].size for a in alone)
    for b, r in enumerate(res):
        g = _got(matcher, b, r)
        _same(g, alone[b % 8], b)
        check_alignment(g, E.restated(protos[b % 8]), E.restated(protos[b % 8], NUDGE_SEED))
    with pytest.raises(DgsError) as e:
        matcher.align_overlapped_batch([feats[b % 8] for b in range(n + 1)])
    assert e.value.status == 1 and "DGS_LA_MAX_ITEMS" in str(e.value)


def test_hypothesis_limit(matcher):
    from delta_graph_slam_amd._lib import DgsError
    from delta_graph_slam_amd.line_align import LineScanMatcher
    from delta_graph_slam_amd.registration import Registration
    f = _features(E.over_the_hypothesis_limit()[0])
    with pytest.raises(DgsError) as e:
        matcher.align_overlapped_batch([f] * 17)
    assert e.value.status == 1 and "DGS_LA_MAX_HYPOTHESES" in str(e.value)
    assert matcher.overlapped_counts() == dict(launches=0, host_waits=0, items=0, hypotheses=0)     # refused before any launch
    with pytest.raises(DgsError):
        matcher.overlapped_hypotheses(0, 0, 1)
    item = _features(E.twin_item("trip_lane0"))
    after = _got(matcher, 0, matcher.align_overlapped(*item))
    fresh_matcher = LineScanMatcher(None, registration=Registration("NDT_OMP", device=0))
    _same(after, _got(fresh_matcher, 0, fresh_matcher.align_overlapped(*item)), "after the refusal")
    assert after["winner"] == 0


# ---- the C++ wrappers -----------------------------------------------------------------------------------------------------------------------
def test_cpp_wrappers_equal_the_python_path(tmp_path, overlap, units):
    exe = str(tmp_path / "building_overlap_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "building_overlap_driver.cpp"), "-o", exe,
                           os.path.join(ROOT, "delta_graph_slam_amd", "libdgs_reg.so"), "-Wl,-rpath," + os.path.join(ROOT, "delta_graph_slam_amd"),
                           "-Wl,-rpath,/opt/rocm/lib"])
    run = lambda *a: json.loads(subprocess.check_output([exe] + list(a), timeout=120).decode().splitlines()[-1])
    bl, ce = E.pair_scenes()["words66"]
    ip, op = str(tmp_path / "b.bin"), str(tmp_path / "p.bin")
    BR.write_buildings(ip, bl, ce)
    res = run("device", "pairs", ip, op)
    assert res["ok"] and res["n"] == len(bl), res
    assert np.fromfile(op, np.int32).tobytes() == overlap.overlapped_pairs(bl, ce).tobytes() == E.pair_result("words66").tobytes()
    items, _, got, _ = units
    ip, op = str(tmp_path / "i.bin"), str(tmp_path / "o.bin")
    BR.write_items(ip, items)
    res = run("device", "align", ip, op)
    assert res["ok"] and res["n"] == len(items) and res["count"] == sum(E.UNIT_H), res
    for b, d in enumerate(read_align(op, items)):
        for k, v in d.items():
            assert np.array_equal(np.asarray(v, np.float64), np.asarray(got[b][k], np.float64)), (b, k)   # bit for bit: the same library calls
