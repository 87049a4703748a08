"""Building overlap without a GPU: the numpy restatement (tests/building_overlap_reference.py) on its scenes, the measurement of the tolerance
the GPU tests use, the shared header compiled for the host (tests/cpp/building_overlap_driver.cpp, mode `host`) against the restatement,
and the new symbols, ctypes mirrors and struct sizes.

TOL_OVERLAP.  The restatement runs every alignment scene and every item of batch_mixed twice: with numpy's arctan2 / sin / cos, and with
every trigonometric result nudged by a seeded +-1 ulp (DESIGN.md 6f's method).  Largest spreads measured over all of them:
    per hypothesis past the angle gate (norm, rotation, translation) 2.85e-14, final record (transformation, norm, aligned lines) 6.3e-15
TOL_OVERLAP = 4 x the largest spread = 1.14e-13 covers a device libm that is one ulp off in either direction.  No scene and no batch item has
an unstable hypothesis (gate outcome, or rot1 / rot2 choice past the angle gate) under the nudge; the cap the GPU test may exclude is 2 % of
a scene's hypotheses and never the winner.  The pair search has no libm call: its list is compared exactly."""
import ctypes as C
import json
import os
import subprocess
import tempfile

import numpy as np
import pytest

import building_overlap_reference as BR

SPREAD = 2.85e-14
TOL_OVERLAP = 4 * SPREAD
UNSTABLE_CAP = 0.02
NUDGE_SEED = 11
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [("scene", n) for n in BR.align_scenes()] + [("batch", b) for b in range(33)]
OWN_RULE_ONLY = ("symmetric_squares",)


def case_result(kind, key, seed=None):
    return BR.scene_result(key, seed) if kind == "scene" else BR.batch_result(key, seed)


# ---- the restatement's own facts ----------------------------------------------------------------------------------------------------------
def test_pair_scenes_are_what_the_issue_lists():
    s = BR.pair_scenes()
    r = {n: BR.pair_result(n) for n in s}
    assert [len(s[n][0]) for n in ("b0", "b1", "b2")] == [0, 1, 2]
    assert r["b0"].shape == (0, 2) and r["b1"].shape == (0, 2) and r["b2"].tolist() == [[0, 1]]
    odd = s["odd_sizes"][0]
    assert [b.shape[0] for b in odd] == [0, 1, 65, 3, 4, 0] and r["odd_sizes"].tolist() == [[1, 4], [2, 3]]
    gon, tri = BR.shrink(odd[2], s["odd_sizes"][1][2]), BR.shrink(odd[3], s["odd_sizes"][1][3])
    first = np.nonzero(BR.lines_intersected(gon[:, None], tri[None, :]).reshape(-1))[0][0]
    assert first >= 64                                                   # the first intersecting line pair p = a * Lb + b is past lane 63
    assert r["shared_wall"].size == 0 and r["crossing"].tolist() == [[0, 1]]
    assert r["inside"].size == 0                                         # containment is not overlap: no wall crosses a wall
    assert r["collinear"].size == 0                                      # det == 0 never intersects
    assert r["axis_aligned"].tolist() == [[0, 1]]                        # the plus crosses; the bar ends short of the third stem
    assert r["clique24"].shape[0] == 24 * 23 // 2 > 256
    assert np.array_equal(r["clique24"], np.array([(i, j) for i in range(24) for j in range(i + 1, 24)], np.int32))
    for n, B in (("grid65", 65), ("grid129", 129), ("random300", 300)):
        assert len(s[n][0]) == B
        frac = np.unique(r[n]).size / B
        print(n, "pairs", r[n].shape[0], "buildings in a pair", frac)
        assert 0.05 < frac < 0.7 and r[n].shape[0] >= 8
        assert np.all(r[n][:, 0] < r[n][:, 1]) and np.array_equal(r[n], r[n][np.lexsort((r[n][:, 1], r[n][:, 0]))])
    assert np.any(r["grid129"][:, 0] >= 64) and [63, 128] in r["grid129"].tolist()      # rows past the first chunk, a j in the third


def test_pair_search_equals_the_scalar_double_loop():
    """the vectorised restatement against are_buildings_overlapped called pair by pair, as getOverlappedBuildings does"""
    for n in ("odd_sizes", "axis_aligned", "clique24", "grid65"):
        bl, ce = BR.pair_scenes()[n]
        want = [(i, j) for i in range(len(bl)) for j in range(i + 1, len(bl)) if BR.buildings_overlapped(bl[i], ce[i], bl[j], ce[j])]
        assert BR.pair_result(n).tolist() == [list(p) for p in want]


def test_appended_buildings_do_not_change_a_pair_list():
    bl, ce = BR.pair_scenes()["grid65"]
    more, mce = BR.pair_scenes()["clique24"]
    far = np.array([500.0, 500.0, 0.0])
    got = BR.overlapped_pairs(bl + [m + far for m in more], np.concatenate([ce, mce + far]))
    assert np.array_equal(got[np.all(got < 65, axis=1)], BR.pair_result("grid65")) and not np.any((got[:, 0] < 65) & (got[:, 1] >= 65))


@pytest.mark.parametrize("kind,key", CASES)
def test_spread_and_unstable_hypotheses(kind, key):
    a, b = case_result(kind, key), case_result(kind, key, NUDGE_SEED)
    un, s_hyp, s_final = BR.compare_runs(a, b)
    print(kind, key, "hypotheses", a["gate"].size, "edge pairs", a["n_edge"], "unstable", un.size, "spreads", s_hyp, s_final, "winner", a["winner"],
          "margin", BR.margin(a))
    assert max(s_hyp, s_final) <= SPREAD
    assert un.size == 0
    assert np.array_equal(a["edges_source"], b["edges_source"]) and np.array_equal(a["edges_target"], b["edges_target"])   # no trigonometry there


def test_align_scenes_cover_what_the_issue_lists():
    s = BR.align_scenes()
    r = {n: BR.scene_result(n) for n in s}
    o = r["offset_rects"]
    assert o["winner"] >= o["n_edge"] > 0 and abs(o["translation_norm"] - 1.0) < 1e-12 and BR.margin(o) > 1.0    # unique: 1 m, the next 2.5 m
    src, trg, cs, ct = s["offset_rects"]
    step = o["translation"][o["winner"]] * [1, 1, 0]                      # the winner turns by less than 1e-15 rad: its move is this shift
    assert BR.buildings_overlapped(src, cs, trg, ct) and not BR.buildings_overlapped(o["aligned_lines"], cs, trg, ct)
    assert BR.buildings_overlapped(src + 0.9 * step, cs, trg, ct)        # 10 cm short of the move: still overlapped (the depth is 1 m)
    assert not BR.buildings_overlapped(src + 0.95 * step, cs, trg, ct)   # 5 cm short: already apart, so the clearance is centimetres
    l = r["l_shape"]
    past = l["gate"][:l["n_edge"]] != BR.GATE_ANGLE
    assert l["rot1"][past].any() and not l["rot1"][past].all()           # both rotations are taken
    e = r["edge_pair_winner"]
    assert 0 <= e["winner"] < e["n_edge"] and BR.margin(e) > 0.1
    assert r["one_line_source"]["n_edge"] == 0 and r["one_line_source"]["n_line"] == 4 and r["one_line_source"]["winner"] >= 0
    for n in ("empty_source", "empty_target"):
        assert r[n]["gate"].size == 0 and r[n]["winner"] == -1 and r[n]["is_identity"] and np.array_equal(r[n]["aligned_lines"], s[n][0])
    g = r["all_angle_gated"]
    assert g["gate"].size == 4 and np.all(g["gate"] == BR.GATE_ANGLE) and g["is_identity"]
    v = r["all_overlapped"]
    assert v["n_angle_passed"] >= 32 and v["n_not_overlapped"] == 0 and v["winner"] == -1 and v["is_identity"]
    w = r["line_pair_winner"]
    assert w["n_edge"] == 16 and w["winner"] >= 16 and BR.margin(w) > 1.0
    f = r["fences65"]
    assert s["fences65"][0].shape[0] == s["fences65"][1].shape[0] == 65 and f["n_line"] == 4225 and f["winner"] >= 0 and BR.margin(f) > 1e-3
    q = r["symmetric_squares"]
    ok = q["gate"] == BR.GATE_PASS
    twins = np.nonzero(ok & (q["tn"] == q["tn"][q["winner"]]))[0]
    assert twins.size >= 2 and twins[0] == q["winner"]                  # bit-equal norms: the lowest h wins
    assert BR.margin(q) <= TOL_OVERLAP                                    # and a rival that moves differently within the tolerance
    for x in r.values():
        assert x["winner"] == BR.own_rule_winner(x["gate"], x["tn"])


def test_batch_mixed_is_what_the_issue_asks_for():
    items = BR.batch_mixed()
    assert len(items) == 33
    h = [BR.batch_result(b)["gate"].size for b in range(33)]
    assert items[16][0].shape[0] == 0 and h[16] == 0                      # an empty item
    assert BR.batch_result(20)["n_edge"] == 0 and h[20] == 1              # a no-edge item
    off = np.cumsum([0] + h)
    inner = [int(o) for o in off[1:-1] if 0 < o < off[-1]]
    assert any(o % 64 for o in inner) and any(o % 256 for o in inner)     # items begin inside a wave and inside a workgroup


# ---- symbols, mirrors, struct sizes ------------------------------------------------------------------------------------------------------
NEW_SYMBOLS = ["dgs_building_overlap_pairs", "dgs_line_align_overlapped_batch", "dgs_line_align_overlapped",
               "dgs_line_align_overlapped_get_hypotheses", "dgs_building_overlap_get_counts"]


def test_new_symbols_are_declared_exported_and_bound():
    from delta_graph_slam_amd import _lib as L
    lib = L.load()
    header = open(os.path.join(ROOT, "include", "dgs_reg.h")).read()
    for name in NEW_SYMBOLS:
        assert name + "(" in header and name in L.SYMBOLS and hasattr(lib, name) and getattr(lib, name).argtypes
    assert lib.dgs_abi_version() == 5
    assert L.LA_GATE[7] == "OVERLAP" and L.STATUS[7] == "DGS_ERR_CAPACITY" and L.BO_MAX_BUILDINGS == 1 << 14


def test_struct_layouts_match_the_header():
    from delta_graph_slam_amd import _lib as L
    src = r'''
#include <stdio.h>
#include <stddef.h>
#include "dgs_reg.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu %zu %zu %d %d %d %.17g\n", sizeof(dgs_line_overlap_alignment), offsetof(dgs_line_overlap_alignment, translation_norm),
         offsetof(dgs_line_overlap_alignment, winner), offsetof(dgs_line_overlap_alignment, n_not_overlapped),
         offsetof(dgs_line_overlap_alignment, is_identity), offsetof(dgs_line_overlap_alignment, status),
         sizeof(dgs_line_align_overlapped_hypothesis), offsetof(dgs_line_align_overlapped_hypothesis, translation_norm),
         (int)DGS_LA_GATE_OVERLAP, (int)DGS_ERR_CAPACITY, (int)DGS_BO_MAX_BUILDINGS, DGS_LA_OVERLAP_MAX_ANGLE);
  return 0;
}'''
    with tempfile.TemporaryDirectory() as d:
        cfile = os.path.join(d, "t.c")
        open(cfile, "w").write(src)
        exe = os.path.join(d, "t")
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), cfile, "-o", exe])   # the header is plain C
        vals = subprocess.check_output([exe]).split()
    A, H = L.LineOverlapAlignment, L.LineAlignOverlappedHypothesis
    assert [int(x) for x in vals[:11]] == [C.sizeof(A), A.translation_norm.offset, A.winner.offset, A.n_not_overlapped.offset, A.is_identity.offset,
                                           A.status.offset, C.sizeof(H), H.translation_norm.offset, 7, 7, L.BO_MAX_BUILDINGS]
    assert float(vals[11]) == np.pi / 3.0 == BR.MAX_ANGLE
    assert C.sizeof(L.LineAlignParams) == 136                             # no member was added: pi / 3 is a constant


def test_invalid_arguments_are_rejected_without_touching_a_device():
    from delta_graph_slam_amd import _lib as L
    lib = L.load()
    n = C.c_int64(0)
    assert lib.dgs_building_overlap_pairs(None, None, None, None, 0, None, 0, C.byref(n)) == 1
    assert lib.dgs_line_align_overlapped_batch(None, None, 0, None, None, None, None, None, None, None, None) == 1
    assert lib.dgs_line_align_overlapped_get_hypotheses(None, 0, 0, 0, None) == 1
    assert lib.dgs_building_overlap_get_counts(None, None) == 1


# ---- the shared header compiled for the host ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("bo") / "building_overlap_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "building_overlap_driver.cpp"), "-o", exe,
                           os.path.join(ROOT, "delta_graph_slam_amd", "libdgs_reg.so"), "-Wl,-rpath," + os.path.join(ROOT, "delta_graph_slam_amd"),
                           "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def run_driver(driver, mode, what, ip, op, *args):
    return json.loads(subprocess.check_output([driver, mode, what, ip, op] + list(args), timeout=120).decode().splitlines()[-1])


def read_align(path, items):
    """-> one dict per item from the driver's `align` output"""
    v = np.fromfile(path, np.float64)
    out, at = [], 0
    for it in items:
        d = dict(transformation=v[at:at + 16].reshape(4, 4), translation_norm=v[at + 16])
        (d["winner"], d["n_edge"], d["n_line"], d["n_angle_passed"], d["n_not_overlapped"], d["Es"], d["Et"], d["is_identity"]) = (int(x) for x in v[at + 17:at + 25])
        at += 25
        d["aligned_lines"] = v[at:at + 6 * it[0].shape[0]].reshape(-1, 2, 3)
        at += 6 * it[0].shape[0]
        h = d["n_edge"] + d["n_line"]
        rec = v[at:at + 9 * h].reshape(-1, 9)
        at += 9 * h
        d["gate"], d["rotation"], d["translation"], d["tn"] = rec[:, 0].astype(np.int64), rec[:, 1:5], rec[:, 5:8], rec[:, 8]
        out.append(d)
    assert at == v.size
    return out


def close(got, want, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    same = (got == want) | (np.isnan(got) & np.isnan(want))
    with np.errstate(all="ignore"):
        err = np.where(same, 0.0, np.abs(got - want))
    print(what, "largest difference", float(err.max(initial=0.0)))
    assert np.all(err <= TOL_OVERLAP), (what, float(err.max()))


def check_alignment(got, ref, nudged, own_rule_only=False):
    """`got`: gate, rotation, translation, tn per hypothesis and the record (winner, transformation, translation_norm, aligned_lines, counts,
    Es, Et, is_identity), from the host header or the device; `ref`, `nudged`: the restatement's plain and nudged runs."""
    assert (got["Es"], got["Et"]) == (ref["edges_source"].shape[0], ref["edges_target"].shape[0])
    assert (got["n_edge"], got["n_line"]) == (ref["n_edge"], ref["n_line"]) and got["gate"].size == ref["gate"].size
    un = BR.compare_runs(ref, nudged)[0]
    assert un.size <= UNSTABLE_CAP * max(ref["gate"].size, 1) and ref["winner"] not in un
    stable = np.ones(ref["gate"].size, bool)
    stable[un] = False
    assert np.array_equal(got["gate"][stable], ref["gate"][stable])                       # gate codes, exactly
    past = stable & (ref["gate"] != BR.GATE_ANGLE)                                        # behind the gate a transform may sit on the pi / 2 wrap
    for k in ("tn", "rotation", "translation"):
        close(got[k][past], ref[k][past], k)
    if un.size == 0:
        assert (got["n_angle_passed"], got["n_not_overlapped"]) == (ref["n_angle_passed"], ref["n_not_overlapped"])
    assert got["winner"] == BR.own_rule_winner(got["gate"], got["tn"])                    # its own rule on its own records
    assert (got["winner"] >= 0) == (ref["winner"] >= 0)
    assert got["is_identity"] == int(np.array_equal(got["transformation"], np.eye(4)))
    if got["winner"] >= 0:
        w = got["winner"]
        assert np.array_equal(got["transformation"], BR.R._mat(got["rotation"][w], got["translation"][w])) and got["translation_norm"] == got["tn"][w]
    else:
        assert got["translation_norm"] == BR.DBL_MAX and np.array_equal(got["aligned_lines"], ref["aligned_lines"])   # the source lines as they are
    if own_rule_only:
        return
    if BR.margin(ref) > TOL_OVERLAP:
        assert got["winner"] == ref["winner"]
    for k in ("translation_norm", "transformation", "aligned_lines"):
        close(got[k], ref[k], k)


@pytest.mark.parametrize("name", list(BR.pair_scenes()))
def test_host_header_pair_search_equals_the_restatement(driver, tmp_path, name):
    bl, ce = BR.pair_scenes()[name]
    ip, op = str(tmp_path / "b.bin"), str(tmp_path / "p.bin")
    BR.write_buildings(ip, bl, ce)
    res = run_driver(driver, "host", "pairs", ip, op)
    assert res["ok"] and res["n"] == len(bl)
    assert np.array_equal(np.fromfile(op, np.int32).reshape(-1, 2), BR.pair_result(name))     # exactly, order included


@pytest.mark.parametrize("name", list(BR.align_scenes()))
def test_host_header_alignment_equals_the_restatement_on_scenes(driver, tmp_path, name):
    item = BR.align_scenes()[name]
    ip, op = str(tmp_path / "i.bin"), str(tmp_path / "o.bin")
    BR.write_items(ip, [item])
    assert run_driver(driver, "host", "align", ip, op)["ok"]
    check_alignment(read_align(op, [item])[0], BR.scene_result(name), BR.scene_result(name, NUDGE_SEED), name in OWN_RULE_ONLY)


def test_host_header_alignment_equals_the_restatement_on_batch_mixed(driver, tmp_path):
    items = BR.batch_mixed()
    ip, op = str(tmp_path / "i.bin"), str(tmp_path / "o.bin")
    BR.write_items(ip, items)
    res = run_driver(driver, "host", "align", ip, op)
    assert res["ok"] and res["n"] == 33
    own = [list(BR.align_scenes()).index(n) for n in OWN_RULE_ONLY]
    for b, got in enumerate(read_align(op, items)):
        check_alignment(got, BR.batch_result(b), BR.batch_result(b, NUDGE_SEED), b in own)
