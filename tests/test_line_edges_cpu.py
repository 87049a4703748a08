"""The edge extraction's host side without a GPU: the refactored host path (la::edge_pair behind dgs_line_edges_angular) against the numpy
restatement byte for byte on every scene of the GPU tests, the scenes' stated properties, the edges_on_device member (in the place of
reserved2: the struct keeps its size) and the two accepted struct sizes, and the new entry points' argument checks, which run before the handle is looked at (the message of a call
without a handle is dgs_last_error(NULL)'s)."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

import line_align_local_reference as LR
import line_edges_scenes as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("dgs_line_edge_extraction_batch", "dgs_line_edge_extraction", "dgs_line_edges_get_counts")
# the restatement is scalar Python: the two scenes of 512 lines (130,816 pairs each) are compared once, in the mode that drops the most
# pairs late (align_local's target call); every other scene in all three modes
BIG = ("max512", "scan_over")
_WANT = {}
SCENE_MODES = [(n, m) for n in S.scenes() for m in S.MODES if n not in BIG or m == (True, 7.0)]


@pytest.mark.parametrize("name,mode", SCENE_MODES, ids=[f"{n}-{int(m[0])}-{m[1]}" for n, m in SCENE_MODES])
def test_host_path_equals_the_restatement(name, mode):
    for k, seg in enumerate(S.scenes()[name]):
        key = (seg.tobytes(), mode)
        if key not in _WANT:                                 # computed once and left unchanged: scan_over repeats max512's segment
            _WANT[key] = np.asarray(LR.edge_extraction(seg, *mode), np.float64).reshape(-1, 3, 3)
        want = _WANT[key]
        got = S.host_edges(seg, *mode)
        assert got.shape == want.shape and got.tobytes() == want.tobytes(), (name, k)


def _cases(lines):
    cases = []
    LR.edge_extraction(lines, False, 7.0, cases)             # (case, edges) per pair
    return [c for c, _ in cases]


def test_scenes_have_their_stated_properties():
    sc = S.scenes()
    assert [len(s) for s in sc["mixed_sizes"]] == [0, 3, 0, 0, 2, 1, 3, 0]
    assert [sum(len(s) for s in sc[n]) for n in ("n0", "n1", "n2", "n3")] == [0, 1, 2, 3]
    for n in ("n0", "n1"):
        assert S.host_edges(sc[n][0], False, 7.0).shape[0] == 0
    assert S.host_edges(sc["n2"][0], False, 7.0).shape[0] == 4 and S.host_edges(sc["n3"][0], False, 7.0).shape[0] == 8
    # one scene per case, and what the angular distance does to it: off / on with 7.0 / on with 0.01
    want = dict(case1_both_same=(1, [1, 1, 0]), case1_far=(1, [1, 0, 0]), case2_same1_only=(2, [2, 2, 0]), case2_far=(2, [2, 0, 0]),
                case3_same2_only=(3, [2, 2, 0]), case3_other_end=(3, [2, 2, 0]), case3_far=(3, [2, 0, 0]), case4_neither=(4, [4, 4, 4]),
                case4_short_arms=(4, [1, 1, 1]))
    assert set(want) == set(S.CASES)
    for name, (case, counts) in want.items():
        assert _cases(S.CASES[name]) == [case], name
        assert [S.host_edges(S.CASES[name], *m).shape[0] for m in S.MODES] == counts, name
    # same2 only: point_a comes from line 2, chosen by comparing line 1's sides
    e = S.host_edges(S.CASES["case3_other_end"], False, 7.0)
    assert np.array_equal(e[0, 1], S.CASES["case3_other_end"][1][0]) and np.array_equal(e[0, 2], S.CASES["case3_other_end"][0][0])
    # star: every pair is gated or emits exactly four edges, in the order of the fourth case
    lines = sc["star"][0]
    cases = _cases(lines)
    assert set(cases) == {0, 4} and cases.count(4) == 5 * 7
    e = S.host_edges(lines, False, 7.0)
    assert e.shape[0] == 4 * 5 * 7
    first = e[:4]
    assert np.array_equal(first[:, 1], [lines[0][0], lines[0][0], lines[0][1], lines[0][1]])
    assert np.array_equal(first[:, 2], [lines[5][0], lines[5][1], lines[5][0], lines[5][1]])
    # the gate: the wall against the 16 others: parallel and just inside 60 degrees gated, just beyond not; the lines at 60 and 120 degrees
    # as computed fall where their rounding puts them
    lines = sc["gate60"][0]
    gated = [not S.host_edges(np.array([lines[0], l]), False, 7.0).shape[0] for l in lines[1:]]
    assert gated[:3] == [True, True, True] and gated[4:9] == [False] * 5 and gated[10:13] == [True, True, True]
    assert len(set(gated[13:])) == 2                          # sqrt(3) / 2 and its neighbours fall on both sides
    # the boundaries of the chosen index
    assert [S.slots(sc[n]) for n in ("wg_short", "wg_exact", "wg_over", "wg_over_emits")] == [255, 256, 257, 259]
    assert S.slots(sc["max512"]) == S.SCAN_CHUNK and S.slots(sc["scan_over"]) == S.SCAN_CHUNK + 1 + 9
    assert S.WORKGROUP == 256 and [len(sc[n][0]) for n in ("tri23", "tri24", "max512")] == [23, 24, 512]
    assert S.host_edges(sc["wg_over_emits"][-1], False, 7.0).shape[0] == 4          # slot 256 emits
    assert S.host_edges(sc["max512"][0][510:], False, 7.0).shape[0] == 4            # the last pair emits
    for n in ("wg_short", "wg_exact", "tri23", "tri24", "max512"):
        assert S.host_batch(sc[n], False, 7.0)[0].shape[0] > 0
    # the benchmark's crossing scene has source edges, the street scene of DESIGN.md 6f (parallel walls) has none
    src, trg = S.crossing(8)
    assert S.host_edges(src, False, 7.0).shape[0] > 0 and S.host_edges(trg, False, 7.0).shape[0] > 0


def test_symbols_mirrors_and_defaults():
    from delta_graph_slam_amd import _lib as L
    from delta_graph_slam_amd.line_align import LineScanMatcher, params_from_dict
    lib = L.load()
    header = open(os.path.join(ROOT, "include", "dgs_reg.h")).read()
    for s in NEW_SYMBOLS:
        assert re.search(r"\bint\s+" + s + r"\s*\(", header), s
        assert s in L.SYMBOLS and hasattr(lib, s) and getattr(lib, s).argtypes, s
    assert lib.dgs_abi_version() == 5
    for m in ("edge_extraction", "edge_extraction_batch", "edge_counts"):
        assert callable(getattr(LineScanMatcher, m))
    for name, value in (("DGS_LA_MAX_ITEMS", L.LA_MAX_ITEMS), ("DGS_LA_MAX_LINES_TARGET", L.LA_MAX_LINES_TARGET)):
        assert int(re.search(r"#define\s+" + name + r"\s+(\d+)", header).group(1)) == value
    assert re.search(r"#define\s+DGS_LA_MAX_EDGE_PAIRS\s+\(1 << 24\)", header) and L.LA_MAX_EDGE_PAIRS == 1 << 24
    P = L.LineAlignParams
    p, _ = params_from_dict()
    assert p.edges_on_device == 0 and p.struct_size == C.sizeof(P) == 136                 # the member took reserved2's place: the size stays
    assert (P.l_avg_distance_weight.offset, P.edges_on_device.offset) == (72, 132) and not hasattr(p, "reserved2")
    q, rest = params_from_dict(dict(edges_on_device=1))
    assert q.edges_on_device == 1 and not rest
    text = open(os.path.join(ROOT, "include", "dgs", "line_align_hip.hpp")).read()
    assert "edgeExtractionBatch" in text and "edgeExtraction(" in text


def test_both_struct_sizes_are_accepted_and_others_refused():
    """The guard runs before the handle is looked at, and a call without a handle leaves its message in dgs_last_error(NULL): a refused
    struct is reported by name, an accepted one gets as far as the missing handle."""
    from delta_graph_slam_amd import _lib as L
    from delta_graph_slam_amd.line_align import params_from_dict
    lib = L.load()
    lines = S.features(S.CASES["case4_neither"])
    out = np.zeros((2, 10))
    al = L.LineAlignment()
    lal = L.LineLocalAlignment()
    off = (C.c_int64 * 2)(0, 2)

    def calls(p):
        g = lib.dgs_line_align_global(None, C.byref(p), lines.ctypes.data, 2, lines.ctypes.data, 2, 0, 1.0, out.ctypes.data, C.byref(al))
        mg = _err(lib)
        l = lib.dgs_line_align_local_batch(None, C.byref(p), 1, lines.ctypes.data, C.cast(off, C.c_void_p), lines.ctypes.data, C.cast(off, C.c_void_p),
                                           0.5, out.ctypes.data, C.cast(C.pointer(lal), C.c_void_p))
        assert (g, l) == (1, 1)
        return mg, _err(lib)

    p, _ = params_from_dict()
    P = L.LineAlignParams
    sizes = (P.l_avg_distance_weight.offset, C.sizeof(P))    # the struct before align_local's members, and the whole of it
    assert sizes == (72, 136)
    p.edges_on_device = 1
    for size in sizes:
        p.struct_size = size
        assert calls(p) == ("line align: the handle is NULL",) * 2
    # what lies behind a short struct's end is not read: a negative l_* weight is refused only by a struct that declares the member
    p.l_coverage_weight = -1.0
    for size in sizes:
        p.struct_size = size
        mg, ml = calls(p)
        assert mg == "line align: the handle is NULL" and ("weight" in ml) == (size > 72)
    p.l_coverage_weight = 1.0
    for size in (0, 12, 64, 80, 128, 132, 140, 144):              # in between and beyond
        p.struct_size = size
        mg, ml = calls(p)
        assert "struct_size" in mg and "struct_size" in ml


def _err(lib):
    lib.dgs_last_error.restype = C.c_char_p
    lib.dgs_last_error.argtypes = [C.c_void_p]
    return lib.dgs_last_error(None).decode()


def test_limits_are_refused_with_a_message_before_any_device_is_touched():
    from delta_graph_slam_amd import _lib as L
    lib = L.load()
    two = S.CASES["case4_neither"]
    wall = lambda k: np.array(S.R.seg(0.0, 3.0 * k, 5.0, 3.0 * k))
    ne = C.c_int64(0)

    def batch(segments, modes=None, offsets=None):
        n = len(segments)
        f = S.features(np.concatenate(list(segments) + [np.zeros((0, 2, 3))]))
        off = np.cumsum([0] + [len(s) for s in segments]).astype(np.int64) if offsets is None else np.asarray(offsets, np.int64)
        only = np.zeros(n + 1, np.int32)
        dist = np.array([m for m in (modes or [7.0] * n)] + [0.0], np.float64)
        rc = lib.dgs_line_edge_extraction_batch(None, f.ctypes.data, off.ctypes.data, n, only.ctypes.data, dist.ctypes.data, None, 0, None, C.byref(ne))
        return rc, _err(lib)

    def single(lines, dist=7.0):
        f = S.features(lines)
        rc = lib.dgs_line_edge_extraction(None, f.ctypes.data, len(lines), 0, dist, None, 0, C.byref(ne))
        return rc, _err(lib)

    bad = two.copy()
    for v in (np.inf, -np.inf, np.nan):
        bad[1, 0, 1] = v
        for rc, msg in (batch([two, bad]), single(bad)):
            assert rc == 1 and "finite" in msg
    rc, msg = batch([two, two], offsets=[0, 3, 2])
    assert rc == 1 and "ascending" in msg
    rc, msg = batch([two], offsets=[1, 2])
    assert rc == 1 and "first offset" in msg
    many = np.array([wall(k) for k in range(L.LA_MAX_LINES_TARGET + 1)])
    for rc, msg in (batch([two, many]), single(many)):
        assert rc == 1 and "DGS_LA_MAX_LINES_TARGET" in msg
    rc, msg = batch([two[:0]] * (L.LA_MAX_ITEMS + 1))
    assert rc == 1 and "DGS_LA_MAX_ITEMS" in msg
    full = many[:L.LA_MAX_LINES_TARGET]
    assert 64 * len(full) ** 2 == L.LA_MAX_EDGE_PAIRS
    rc, msg = batch([full] * 64 + [two[:1]])                 # one pair slot over the cap
    assert rc == 1 and "DGS_LA_MAX_EDGE_PAIRS" in msg
    rc, msg = batch([two], modes=[np.nan])
    assert rc == 1 and "NaN" in msg
    # arguments that are in order get as far as the handle: 4096 segments, 512 lines, exactly the pair cap
    for rc, msg in (batch([two[:0]] * L.LA_MAX_ITEMS), single(full), batch([full] * 64), single(two)):
        assert rc == 1 and "handle is NULL" in msg
    assert lib.dgs_line_edges_get_counts(None, None) == 1


def test_cpp_adapter_compiles_and_fails_softly_without_a_device(tmp_path):
    """dgs::HipLineAligner::edgeExtractionBatch never throws: without a device it returns false and the caller keeps its host loop."""
    exe = str(tmp_path / "line_edges_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "line_edges_driver.cpp"),
                           "-o", exe, os.path.join(ROOT, "delta_graph_slam_amd", "libdgs_reg.so"), "-Wl,-rpath," + os.path.join(ROOT, "delta_graph_slam_amd"),
                           "-Wl,-rpath,/opt/rocm/lib"])
    ip, op = str(tmp_path / "segments.bin"), str(tmp_path / "out.bin")
    seg = S.CASES["case4_neither"]
    with open(ip, "wb") as f:
        np.array([1, 0, 2, 0], np.int64).tofile(f)
        np.array([7.0], np.float64).tofile(f)
        seg.tofile(f)
    res = json.loads(subprocess.check_output([exe, ip, op], timeout=120).decode().splitlines()[-1])
    assert res["segments"] == 1
    if res["ok"]:                                            # a device is present: the host function's four edges, twice
        out = np.fromfile(op, np.float64)
        assert res["edges"] == 4 and np.array_equal(out[:2], [0, 4])
        assert out[2:].tobytes() == np.concatenate([S.host_edges(seg, False, 7.0)] * 2).tobytes()
    else:
        assert res["edges"] == 0 and not os.path.exists(op)
