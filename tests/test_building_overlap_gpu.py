"""dgs_building_overlap_pairs and dgs_line_align_overlapped_batch on the device against the numpy restatement
(tests/building_overlap_reference.py).  The pair search has no libm call: its list equals the restatement's exactly, order included, on
every scene, and does not change when unrelated buildings are appended.  Alignment: gate codes exactly, norms, transforms and aligned
lines within TOL_OVERLAP (test_building_overlap_cpu.py: 4 x the measured spread of the restatement under a +-1 ulp nudge of its
trigonometry), winners wherever the restatement's margin exceeds TOL_OVERLAP, and in every case the device's winner obeys its own rule on
its own hypothesis records.  Hypotheses whose gate changes under that nudge may be left out of the exact comparison (at most 2 % of a scene,
never the winner; no scene has one).  Every item of the 33-item batch equals the same item run alone bit for bit."""
import json
import os
import subprocess

import numpy as np
import pytest

import building_overlap_reference as BR
from line_align_local_reference import feature_lines
from test_building_overlap_cpu import NUDGE_SEED, OWN_RULE_ONLY, ROOT, check_alignment, read_align

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


# ---- pair search ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(BR.pair_scenes()))
def test_pair_list_equals_the_restatement(overlap, name):
    bl, ce = BR.pair_scenes()[name]
    got = overlap.overlapped_pairs(bl, ce)
    ref = BR.pair_result(name)
    print(name, "buildings", len(bl), "pairs", got.shape[0], ref.shape[0], overlap.counts())
    assert got.dtype == np.int32 and np.array_equal(got, ref)                       # exactly, order included
    c = overlap.counts()
    if len(bl) >= 2:
        assert (c["launches"], c["host_waits"], c["buildings"], c["pairs"]) == (5, 1, len(bl), ref.shape[0])
    else:
        assert (c["launches"], c["host_waits"]) == (0, 0)


def test_line_features_are_taken_like_arrays(overlap):
    bl, ce = BR.pair_scenes()["grid65"]
    assert np.array_equal(overlap.overlapped_pairs([feature_lines(b) for b in bl], ce), BR.pair_result("grid65"))


@pytest.mark.parametrize("name", ["clique24", "random300"])
def test_capacity_one_below_the_count(overlap, name):
    from delta_graph_slam_amd._lib import DGS_ERR_CAPACITY, DgsError
    bl, ce = BR.pair_scenes()[name]
    ref = BR.pair_result(name)
    with pytest.raises(DgsError) as e:
        overlap.overlapped_pairs(bl, ce, capacity=ref.shape[0] - 1)
    assert e.value.status == DGS_ERR_CAPACITY and "capacity" in str(e.value)
    assert overlap.last_count == ref.shape[0] and np.array_equal(overlap.last_pairs, ref[:-1])     # the full count, the first `capacity` pairs
    assert np.array_equal(overlap.overlapped_pairs(bl, ce, capacity=ref.shape[0]), ref)
    with pytest.raises(DgsError):
        overlap.overlapped_pairs(bl, ce, capacity=0)
    assert overlap.last_count == ref.shape[0] and overlap.last_pairs.shape == (0, 2)
    small = overlap.overlapped_pairs(bl[:3], ce[:3], capacity=10 ** 6)                              # more room than pairs can exist
    assert np.array_equal(small, BR.overlapped_pairs(bl[:3], ce[:3]))


@pytest.mark.parametrize("name", ["grid65", "grid129"])
def test_appended_buildings_do_not_change_a_pair_list(overlap, name):
    bl, ce = BR.pair_scenes()[name]
    more, mce = BR.pair_scenes()["clique24"]
    B, far = len(bl), np.array([500.0, 500.0, 0.0])                       # the clique, lines and centres, 500 m away
    got = overlap.overlapped_pairs(bl + [m + far for m in more] + [BR.NONE], np.concatenate([ce, mce + far, [[0.0, 0.0, 0.0]]]))
    assert np.array_equal(got[np.all(got < B, axis=1)], BR.pair_result(name))
    assert np.array_equal(got[np.all(got >= B, axis=1)] - B, BR.pair_result("clique24"))
    assert not np.any((got[:, 0] < B) & (got[:, 1] >= B))


def test_pair_search_limits(overlap):
    from delta_graph_slam_amd._lib import BO_MAX_BUILDINGS, DgsError
    box = BR.rectangle(0, 0, 10, 6)
    for bl, ce, word in (([BR.NONE] * (BO_MAX_BUILDINGS + 1), np.zeros((BO_MAX_BUILDINGS + 1, 3)), "DGS_BO_MAX_BUILDINGS"),
                         ([np.concatenate([box] * 129), box], np.zeros((2, 3)), "DGS_LA_MAX_LINES_TARGET"),
                         ([box * np.array([np.nan, 1, 1]), box], np.zeros((2, 3)), "finite"),
                         ([box, box], np.array([[0, np.inf, 0], [0, 0, 0.0]]), "finite")):
        with pytest.raises(DgsError) as e:
            overlap.overlapped_pairs(bl, ce)
        assert e.value.status == 1 and word in str(e.value)
    assert overlap.overlapped_pairs([BR.NONE] * BO_MAX_BUILDINGS, np.zeros((BO_MAX_BUILDINGS, 3))).shape == (0, 2)   # the limit itself is served
    assert np.array_equal(overlap.overlapped_pairs([np.concatenate([box] * 128), BR.rectangle(3, 2, 4, 12)], np.array([[0, 0, 0], [3, 2, 0.0]])), [[0, 1]])


# ---- alignment ----------------------------------------------------------------------------------------------------------------------------
def _features(item):
    return (feature_lines(item[0]), feature_lines(item[1]), item[2], item[3])


def _got(m, item, res):
    """One item of the last call in the shape test_building_overlap_cpu.check_alignment takes."""
    c = res.counts
    hy = m.overlapped_hypotheses(item)
    d = dict(transformation=res.transformation, translation_norm=res.translation_norm, winner=res.winner, n_edge=c["hypotheses_edge"],
             n_line=c["hypotheses_line"], n_angle_passed=c["angle_passed"], n_not_overlapped=c["not_overlapped"], Es=c["edges_source"], Et=c["edges_target"],
             is_identity=int(res.is_identity), aligned_lines=np.array([[l.pointA, l.pointB] for l in res.aligned_lines], np.float64).reshape(-1, 2, 3))
    d.update(gate=hy["gate"].astype(np.int64), rotation=hy["rotation"], translation=hy["translation"], tn=hy["tn"])
    return d


def _status(ref):
    return "ALIGNED" if ref["winner"] >= 0 else "NO_HYPOTHESES" if ref["gate"].size == 0 else "ALL_GATED" if ref["n_not_overlapped"] == 0 else "NONE_BETTER"


@pytest.mark.parametrize("name", list(BR.align_scenes()))
def test_alignment_equals_the_restatement_on_scenes(matcher, name):
    item = BR.align_scenes()[name]
    res = matcher.align_overlapped(*_features(item))
    ref = BR.scene_result(name)
    got = _got(matcher, 0, res)
    print(name, "hypotheses", got["gate"].size, "angle passed", got["n_angle_passed"], "not overlapped", got["n_not_overlapped"], "winner", res.winner,
          ref["winner"], "norm", res.translation_norm, "status", res.status, matcher.overlapped_counts())
    check_alignment(got, ref, BR.scene_result(name, NUDGE_SEED), name in OWN_RULE_ONLY)
    assert res.status == _status(ref)
    c = matcher.overlapped_counts()
    assert (c["launches"], c["host_waits"], c["items"], c["hypotheses"]) == (3, 1, 1, ref["gate"].size)
    src = _features(item)[0]
    assert [l.mean_error for l in res.aligned_lines] == [l.mean_error for l in src]      # the statistics are carried through


def test_double_angle_chain(matcher):
    """angle_gate_float_chain = 0 comes from dgs_line_align_params: atan2(r10, r00) in double"""
    from delta_graph_slam_amd.line_align import LineScanMatcher
    item = BR.align_scenes()["l_shape"]
    m = LineScanMatcher(dict(angle_gate_float_chain=0), registration=matcher.registration)
    res = m.align_overlapped(*_features(item))
    check_alignment(_got(m, 0, res), BR.align_overlapped(*item, float_chain=0), BR.align_overlapped(*item, float_chain=0, seed=NUDGE_SEED))


@pytest.fixture(scope="module")
def batch(matcher):
    items = BR.batch_mixed()
    res = matcher.align_overlapped_batch([_features(it) for it in items])
    counts = matcher.overlapped_counts()
    return items, res, [_got(matcher, b, r) for b, r in enumerate(res)], counts


def test_batch_equals_the_restatement(batch):
    items, res, got, counts = batch
    assert len(res) == 33 and (counts["launches"], counts["host_waits"], counts["items"]) == (3, 1, 33)
    assert counts["hypotheses"] == sum(BR.batch_result(b)["gate"].size for b in range(33))
    own = [list(BR.align_scenes()).index(n) for n in OWN_RULE_ONLY]
    for b in range(33):
        check_alignment(got[b], BR.batch_result(b), BR.batch_result(b, NUDGE_SEED), b in own)
        assert res[b].status == _status(BR.batch_result(b))
    assert res[16].status == "NO_HYPOTHESES" and res[16].is_identity and res[20].counts["edges_source"] == 0


def test_every_batch_item_equals_the_item_alone_bit_for_bit(matcher, batch):
    items, res, got, _ = batch
    for b, it in enumerate(items):
        one = matcher.align_overlapped(*_features(it))
        alone = _got(matcher, 0, one)
        assert one.status == res[b].status
        for k, v in got[b].items():
            if isinstance(v, np.ndarray):
                assert v.tobytes() == alone[k].tobytes(), (b, k)
            else:
                assert v == alone[k], (b, k)


def test_alignment_limits(matcher):
    from delta_graph_slam_amd._lib import DgsError
    box, other = feature_lines(BR.rectangle(0, 0, 10, 6)), feature_lines(BR.rectangle(6, 2, 9, 7, 0.2))
    for item, word in (((box * 65, other, np.zeros(3), np.zeros(3)), "DGS_LA_MAX_LINES_SOURCE"),
                       ((box, other * 129, np.zeros(3), np.zeros(3)), "DGS_LA_MAX_LINES_TARGET"),
                       ((box, other, np.array([0, np.nan, 0]), np.zeros(3)), "finite")):
        with pytest.raises(DgsError) as e:
            matcher.align_overlapped(*item)
        assert e.value.status == 1 and word in str(e.value)
    assert matcher.align_overlapped_batch([]) == []
    with pytest.raises(DgsError):
        matcher.overlapped_hypotheses(0, 0, 1)                              # nothing is left to read after an empty call


# ---- the C++ wrappers -----------------------------------------------------------------------------------------------------------------------
def test_cpp_wrappers_equal_the_python_path(tmp_path, overlap, batch):
    exe = str(tmp_path / "building_overlap_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "building_overlap_driver.cpp"), "-o", exe,
                           os.path.join(ROOT, "delta_graph_slam_amd", "libdgs_reg.so"), "-Wl,-rpath," + os.path.join(ROOT, "delta_graph_slam_amd"),
                           "-Wl,-rpath,/opt/rocm/lib"])
    run = lambda *a: json.loads(subprocess.check_output([exe] + list(a), timeout=120).decode().splitlines()[-1])
    bl, ce = BR.pair_scenes()["random300"]                                   # 104 pairs: the wrapper's first capacity holds them
    ip, op = str(tmp_path / "b.bin"), str(tmp_path / "p.bin")
    BR.write_buildings(ip, bl, ce)
    res = run("device", "pairs", ip, op)
    assert res["ok"], res
    assert np.array_equal(np.fromfile(op, np.int32).reshape(-1, 2), BR.pair_result("random300"))
    bl, ce = BR.pair_scenes()["clique24"]                                    # 276 pairs: past it, so the wrapper calls a second time
    BR.write_buildings(ip, bl, ce)
    assert run("device", "pairs", ip, op)["ok"]
    assert np.array_equal(np.fromfile(op, np.int32).reshape(-1, 2), BR.pair_result("clique24"))
    items, _, got, _ = batch
    ip, op = str(tmp_path / "i.bin"), str(tmp_path / "o.bin")
    BR.write_items(ip, items)
    res = run("device", "align", ip, op)
    assert res["ok"] and res["n"] == 33, res
    for b, d in enumerate(read_align(op, items)):
        for k, v in d.items():
            assert np.array_equal(np.asarray(v, np.float64), np.asarray(got[b][k], np.float64)), (b, k)   # bit for bit: the same library calls
