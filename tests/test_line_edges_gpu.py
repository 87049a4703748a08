"""dgs_line_edge_extraction_batch on the device against the host's dgs_line_edges_angular, by bytes: the edges, their order and the edge
offsets of every scene of tests/line_edges_scenes.py in the three modes the aligners use, and dgs_line_align_global /
dgs_line_align_local_batch with edges_on_device 0 and 1 on the scenes of the existing line-align GPU tests and on the benchmark's `crossing`
scene: records, aligned lines and per-hypothesis records identical, one more host wait, a launch count that does not grow with the batch.
No tolerance anywhere: la::edge_pair is + - * /, sqrt, comparisons, fmin and fmax without contraction."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import line_align_local_reference as LR
import line_align_reference as R
import line_edges_scenes as S
from test_line_align_cpu import _arr

pytestmark = pytest.mark.gpu
_lines = LR.feature_lines
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_HOST = {}


@pytest.fixture(scope="module")
def reg():
    from delta_graph_slam_amd.registration import Registration
    return Registration("NDT_OMP", device=0)


def _matcher(reg, params=None):
    from delta_graph_slam_amd.line_align import LineScanMatcher
    return LineScanMatcher(params, registration=reg)


def _host(name, mode):
    """The host function's edges and offsets of a scene, computed once and left unchanged."""
    if (name, mode) not in _HOST:
        _HOST[(name, mode)] = S.host_batch(S.scenes()[name], *mode)
    return _HOST[(name, mode)]


def _device(reg, segments, modes, **kw):
    return S.device_batch_raw(reg._lib, reg._h, segments, modes, **kw)


def _same(got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    return got.shape == want.shape and got.dtype == want.dtype and got.tobytes() == want.tobytes()


@pytest.mark.parametrize("mode", S.MODES, ids=["global", "local_target", "local_source"])
@pytest.mark.parametrize("name", list(S.scenes()))
def test_scene_equals_the_host_function(reg, name, mode):
    segments = S.scenes()[name]
    want, want_off = _host(name, mode)
    rc, got, off, n = _device(reg, segments, [mode] * len(segments))
    c = _matcher(reg).edge_counts()
    print(name, mode, "segments", len(segments), "slots", S.slots(segments), "edges", n, want.shape[0], "counts", c)
    assert rc == 0 and n == want.shape[0]
    assert _same(off, want_off)
    assert _same(got, want)
    assert c["pairs"] == sum(len(s) * (len(s) - 1) // 2 for s in segments) and c["edges"] == n
    # count, scan, offsets, one wait; emit and the download's wait when there are edges; nothing at all without a pair slot
    assert (c["launches"], c["host_waits"]) == ((0, 0) if not S.slots(segments) else (4, 2) if n else (3, 1))


def test_segments_with_their_own_modes(reg):
    """align_local's call: every source segment with (true, 0.01), every target segment with (true, 7.0), in one batch."""
    names = ("case1_both_same", "case2_same1_only", "case3_same2_only", "case4_neither", "case1_far", "gate60", "tri24")
    segments = [S.scenes()[n][0] for n in names]
    src, trg = S.MODES[2], S.MODES[1]
    rc, got, off, n = _device(reg, segments + segments, [src] * len(names) + [trg] * len(names))
    want = [_host(n, src)[0] for n in names] + [_host(n, trg)[0] for n in names]
    assert rc == 0 and _same(off, np.cumsum([0] + [len(w) for w in want]).astype(np.int64))
    assert _same(got, np.concatenate(want))
    assert sum(len(_host(n, src)[0]) for n in names) < sum(len(_host(n, trg)[0]) for n in names)      # the two modes differ on these


def test_batch_order(reg):
    """The same segments in two orders: every segment's edges are unchanged and the offsets follow the order."""
    names = ("tri23", "n0", "star", "case3_other_end", "n1", "wg_exact", "gate60", "n3")
    mode = S.MODES[0]
    rng = np.random.default_rng(5)
    for order in (list(range(len(names))), list(rng.permutation(len(names))), list(range(len(names)))[::-1]):
        segments = [S.scenes()[names[k]][0] for k in order]
        rc, got, off, n = _device(reg, segments, [mode] * len(segments))
        assert rc == 0 and off[0] == 0 and off[-1] == n and np.all(np.diff(off) >= 0)
        for pos, k in enumerate(order):
            assert _same(got[off[pos]:off[pos + 1]], _host(names[k], mode)[0]), (order, pos)


def test_a_table_that_outgrows_its_pinned_block_between_calls():
    """One segment, then 64 segments of at most 64 lines -- their table and packed lines are more than the bytes + bytes / 4 + 4 KiB the
    first call left the pinned block with -- then the one segment again, all on one handle: edges, offsets and counts of a fresh handle"""
    from delta_graph_slam_amd.registration import Registration
    names = ("tri23", "n0", "star", "case3_other_end", "n1", "wg_exact", "gate60", "n3")
    mode = S.MODES[0]
    one, many = [S.scenes()["tri23"][0]], [S.scenes()[names[i % 8]][0] for i in range(64)]
    block = lambda segs: 32 * len(segs) + 8 * ((len(segs) + 2) // 2) + 48 * sum(len(s) for s in segs)   # segment table | offsets | lines
    assert max(len(s) for s in many) <= 64 and block(many) > block(one) + block(one) // 4 + 4096
    used = Registration("NDT_OMP", device=0)
    for segments in (one, many, one):
        fresh = Registration("NDT_OMP", device=0)
        a, b = _device(used, segments, [mode] * len(segments)), _device(fresh, segments, [mode] * len(segments))
        assert a[0] == b[0] == 0 and a[3] == b[3] and _same(a[1], b[1]) and _same(a[2], b[2])
        assert _matcher(used).edge_counts() == _matcher(fresh).edge_counts() and _matcher(used).edge_counts()["edges"] == a[3]
        assert len(segments) == 1 or a[3] > 64
        fresh.close()
    used.close()


def test_capacity_rule_is_dgs_line_edges_s(reg):
    from delta_graph_slam_amd import _lib as L
    segments = S.scenes()["mixed_sizes"]
    mode = S.MODES[0]
    want, want_off = _host("mixed_sizes", mode)
    total = want.shape[0]
    assert total == 8 + 4 + 8
    rc, got, off, n = _device(reg, segments, [mode] * len(segments), capacity=0)          # the count and the offsets alone
    assert rc == 1 and n == total and got.shape[0] == 0 and _same(off, want_off)
    assert _matcher(reg).edge_counts()["launches"] == 3                                   # nothing was emitted
    rc, got, off, n = _device(reg, segments, [mode] * len(segments), capacity=total - 1)
    assert rc == 1 and n == total and "capacity" in (reg._lib.dgs_last_error(reg._h) or b"").decode()
    rc, got, off, n = _device(reg, segments, [mode] * len(segments), capacity=total, want_offsets=False)
    assert rc == 0 and n == total and _same(got, want)
    rc, got, off, n = _device(reg, S.scenes()["n1"], [mode], capacity=0)                   # no edges: nothing is missing
    assert rc == 0 and n == 0 and _same(off, np.zeros(2, np.int64))
    rc, got, off, n = _device(reg, [], [], capacity=0)
    assert rc == 0 and n == 0 and _same(off, np.zeros(1, np.int64))
    # the single-segment entry point
    lines = S.scenes()["star"][0]
    f = S.features(lines)
    out = np.zeros((4 * 5 * 7, 3, 3))
    ne = C.c_int64(-1)
    assert reg._lib.dgs_line_edge_extraction(reg._h, f.ctypes.data, len(lines), 0, 7.0, out.ctypes.data, out.shape[0], C.byref(ne)) == 0
    assert ne.value == out.shape[0] and _same(out, _host("star", mode)[0])
    with pytest.raises(L.DgsError, match="DGS_LA_MAX_LINES_TARGET"):
        _matcher(reg).edge_extraction(_lines(np.array([R.seg(0.0, 3.0 * k, 5.0, 3.0 * k) for k in range(513)])))
    with pytest.raises(L.DgsError, match="finite"):
        bad = S.CASES["case4_neither"].copy()
        bad[0, 1, 0] = np.inf
        _matcher(reg).edge_extraction_batch([(_lines(S.CASES["case4_neither"]), True, 7.0), (_lines(bad), True, 7.0)])


def test_python_methods_return_the_host_function_s_objects(reg):
    from delta_graph_slam_amd.line_align import edge_extraction
    m = _matcher(reg)
    flat = lambda es: np.array([[e.edgePoint, e.pointA, e.pointB] for e in es], np.float64).reshape(-1, 3, 3)
    for name in ("gate60", "star", "n1", "case3_other_end"):
        lines = _lines(S.scenes()[name][0])
        assert _same(flat(m.edge_extraction(lines)), flat(edge_extraction(lines)))
        for only, dist in S.MODES[1:]:
            got = m.edge_extraction(lines, only, dist)
            want = edge_extraction(lines, only, dist)
            assert type(got) is list and all(type(a) is type(b) for a, b in zip(got, want)) and _same(flat(got), flat(want))
    items = [(_lines(s), only, dist) for s in S.scenes()["mixed_sizes"] for only, dist in S.MODES]
    got = m.edge_extraction_batch(items)
    assert len(got) == len(items)
    for g, (lines, only, dist) in zip(got, items):
        assert _same(flat(g), flat(edge_extraction(lines, only, dist)))
    assert m.edge_extraction_batch([]) == []


def test_cpp_driver_equals_the_host_function(reg, tmp_path):
    exe = str(tmp_path / "line_edges_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "line_edges_driver.cpp"),
                           "-o", exe, os.path.join(ROOT, "delta_graph_slam_amd", "libdgs_reg.so"), "-Wl,-rpath," + os.path.join(ROOT, "delta_graph_slam_amd"),
                           "-Wl,-rpath,/opt/rocm/lib"])
    names = ("star", "n0", "case2_same1_only", "tri24", "n1")
    modes = [S.MODES[k % 3] for k in range(len(names))]
    segments = [S.scenes()[n][0] for n in names]
    ip, op = str(tmp_path / "segments.bin"), str(tmp_path / "out.bin")
    with open(ip, "wb") as f:
        np.array([len(names)], np.int64).tofile(f)
        np.cumsum([0] + [len(s) for s in segments]).astype(np.int64).tofile(f)
        np.array([1 if m[0] else 0 for m in modes], np.int64).tofile(f)
        np.array([m[1] for m in modes], np.float64).tofile(f)
        np.concatenate(segments).tofile(f)
    res = json.loads(subprocess.check_output([exe, ip, op], timeout=120).decode().splitlines()[-1])
    want = [_host(n, m)[0] for n, m in zip(names, modes)]
    assert res["ok"] and res["segments"] == len(names) and res["edges"] == sum(len(w) for w in want), res
    out = np.fromfile(op, np.float64)
    assert np.array_equal(out[:len(names) + 1], np.cumsum([0] + [len(w) for w in want]))
    assert _same(out[len(names) + 1:], np.concatenate(want + [want[0]]).ravel())        # the batch, then segment 0 from the single call


# ---- the aligners with edges_on_device ---------------------------------------------------------------------------------------------------
def _fit(f):
    return [f.real_avg_distance, f.avg_distance, f.coverage, f.coverage_percentage]


def _global_scenes():
    sc = dict(R.scenes())
    sc["crossing"] = (*S.crossing(16), {})
    return sc


def _run_global(reg, scene, on):
    src, trg, kw = scene
    m = _matcher(reg, dict(kw.get("params") or {}, edges_on_device=on))
    res = m.align_global(_lines(src), _lines(trg), kw.get("constrain_angle", False), kw.get("max_range", np.inf))
    c = m.counts()
    hy = m.hypotheses() if c["hypotheses"] else {}
    return res, c, hy, (m.edge_counts() if on else None)


@pytest.mark.parametrize("name", list(_global_scenes()))
def test_align_global_is_identical_with_device_edges(reg, name):
    scene = _global_scenes()[name]
    a, ca, ha, _ = _run_global(reg, scene, 0)
    b, cb, hb, ce = _run_global(reg, scene, 1)
    print(name, "counts", a.counts, "host path", ca, "device edges", cb, ce)
    assert _same(a.transformation, b.transformation) and _same(np.array(_fit(a.fitness_score)), np.array(_fit(b.fitness_score)))
    assert _same(np.float64(a.score), np.float64(b.score))
    assert (a.winner, a.refine_steps, a.status, a.counts) == (b.winner, b.refine_steps, b.status, b.counts)
    assert _same(_arr(a.aligned_lines), _arr(b.aligned_lines)) and _same(_arr(a.not_aligned_lines), _arr(b.not_aligned_lines))
    assert set(ha) == set(hb)
    for k in ha:
        assert _same(ha[k], hb[k]), k
    # the extra wait for the two edge counts, and the extraction's launches on top of the search's
    assert (ca["hypotheses"], ca["survivors"]) == (cb["hypotheses"], cb["survivors"])
    some_line = len(scene[0]) + a.counts["lines_target"] > 0
    assert ca["host_waits"] == 1 and cb["host_waits"] == 1 + ce["host_waits"] and ce["host_waits"] == (1 if some_line else 0)
    assert cb["launches"] == ca["launches"] + ce["launches"] and ce["launches"] == (0 if not some_line else 4 if ce["edges"] else 3)
    assert ce["edges"] == a.counts["edges_source"] + a.counts["edges_target"]
    if name == "crossing":
        assert a.counts["edges_source"] > 0 and a.counts["hypotheses"] > 0 and ce["launches"] == 4 and cb["host_waits"] == 2


def _local_items():
    items = {name: (src, trg, kw) for name, (src, trg, kw) in LR.scenes().items()}
    items["crossing"] = (*S.crossing(16), {})
    return items


def _local_equal(a, b):
    assert _same(a.transformation, b.transformation) and _same(a.edge_transformation, b.edge_transformation)
    for x, y in ((a.fitness_score, b.fitness_score), (a.edge_fitness_score, b.edge_fitness_score), (a.baseline_fitness_score, b.baseline_fitness_score)):
        assert _same(np.array(_fit(x)), np.array(_fit(y)))
    assert _same(np.array([a.score, a.edge_score, a.baseline_score]), np.array([b.score, b.edge_score, b.baseline_score]))
    assert (a.winner, a.winner_line, a.status, a.isEdgeAligned, a.counts) == (b.winner, b.winner_line, b.status, b.isEdgeAligned, b.counts)
    assert _same(_arr(a.aligned_lines), _arr(b.aligned_lines))


def _run_local(reg, items, params, max_range, on):
    m = _matcher(reg, dict(params or {}, edges_on_device=on))
    res = m.align_local_batch([(_lines(s), _lines(t)) for s, t in items], max_range)
    c = m.local_counts()
    hy = [[m.local_hypotheses(b, ph, 0, n) for ph, n in ((0, r.counts["hypotheses_edge"]), (1, r.counts["hypotheses_line"])) if n] for b, r in enumerate(res)]
    return res, c, hy, (m.edge_counts() if on else None)


def _compare_local(reg, items, params, max_range):
    a, ca, ha, _ = _run_local(reg, items, params, max_range, 0)
    b, cb, hb, ce = _run_local(reg, items, params, max_range, 1)
    print("items", len(items), "host path", ca, "device edges", cb, ce)
    for x, y in zip(a, b):
        _local_equal(x, y)
    for x, y in zip(ha, hb):
        assert len(x) == len(y)
        for p, q in zip(x, y):
            for k in p:
                assert _same(p[k], q[k]), k
    assert {k: v for k, v in ca.items() if k not in ("launches", "host_waits")} == {k: v for k, v in cb.items() if k not in ("launches", "host_waits")}
    assert ca["host_waits"] == 1 and cb["host_waits"] == 1 + ce["host_waits"] and cb["launches"] == ca["launches"] + ce["launches"]
    assert ce["edges"] == sum(r.counts["edges_source"] + r.counts["edges_target"] for r in a)
    return ca, cb, ce


@pytest.mark.parametrize("name", list(_local_items()))
def test_align_local_is_identical_with_device_edges(reg, name):
    src, trg, kw = _local_items()[name]
    _compare_local(reg, [(src, trg)], kw.get("params"), kw.get("max_range", 0.5))


def test_align_local_batch_is_identical_and_its_launches_do_not_grow(reg):
    items = LR.batch_mixed()
    ca, cb, ce = _compare_local(reg, items, None, 0.5)
    assert len(items) == 33 and cb["items"] == 33 and ce["pairs"] == sum(len(s) * (len(s) - 1) // 2 + len(t) * (len(t) - 1) // 2 for s, t in items)
    assert (ce["launches"], ce["host_waits"], cb["host_waits"]) == (4, 1, 2)
    one = next((s, t) for s, t in items if len(S.host_edges(s, True, 0.01)) + len(S.host_edges(t, True, 7.0)))
    _, c1, e1 = _compare_local(reg, [one], None, 0.5)
    assert c1["launches"] == cb["launches"] and e1["launches"] == 4                   # one item or 33: the same launches
    _, c2, _ = _compare_local(reg, items + items[::-1], None, 0.5)
    assert c2["launches"] == cb["launches"] and c2["host_waits"] == 2


def test_struct_sizes_on_the_device(reg):
    """The short struct takes the host path whatever lies behind its end; the whole struct reads edges_on_device; sizes in between are
    refused by name."""
    from delta_graph_slam_amd import _lib as L
    src, trg = S.crossing(8)
    want = _matcher(reg).align_global(_lines(src), _lines(trg))
    m = _matcher(reg, dict(edges_on_device=1))
    P = L.LineAlignParams
    for size, waits in ((P.l_avg_distance_weight.offset, 1), (C.sizeof(P), 2)):
        m.params.struct_size = size
        got = m.align_global(_lines(src), _lines(trg))
        assert m.counts()["host_waits"] == waits
        assert _same(got.transformation, want.transformation) and (got.winner, got.counts) == (want.winner, want.counts)
        loc = m.align_local(_lines(src), _lines(trg), 0.5)
        assert m.local_counts()["host_waits"] == waits and loc.status in L.LA_STATUS.values()
    for size in (0, 12, 80, 128, P.edges_on_device.offset, C.sizeof(P) + 8):
        m.params.struct_size = size
        with pytest.raises(L.DgsError, match="struct_size"):
            m.align_global(_lines(src), _lines(trg))
        with pytest.raises(L.DgsError, match="struct_size"):
            m.align_local(_lines(src), _lines(trg), 0.5)


def test_pair_cap_of_the_local_batch_is_an_error_not_a_truncation(reg):
    from delta_graph_slam_amd import _lib as L
    wall = np.array([R.seg(0.0, 3.0 * k, 5.0, 3.0 * k) for k in range(512)])
    items = [(_lines(wall[:1]), _lines(wall))] * 64           # 64 x (1 + 512 * 512) pair slots; 64 x 512 line pairs
    m = _matcher(reg, dict(edges_on_device=1))
    with pytest.raises(L.DgsError, match="DGS_LA_MAX_EDGE_PAIRS"):
        m.align_local_batch(items, 0.5)
    res = _matcher(reg).align_local_batch(items[:2], 0.5)      # the host path has no such cap
    assert len(res) == 2
    # align_global's hypothesis cap is checked on the counts read back from the device, with the host path's message
    for on in (0, 1):
        with pytest.raises(L.DgsError, match="DGS_LA_MAX_HYPOTHESES"):
            _matcher(reg, dict(edges_on_device=on)).align_global(_lines(R.grid(16, 16, seed=1)), _lines(R.grid(100, 100, seed=2)))
