"""What every scene of tests/building_overlap_edge_cases.py claims, asserted on the numpy restatement (tests/building_overlap_reference.py)
without a GPU, and the shared header compiled for the host (tests/cpp/building_overlap_driver.cpp, mode `host`) on every one of them.

The conditions are stated against the launch shapes of delta_graph_slam_amd/csrc/building_overlap.hip: 64 flags a word, rows owned by
tiles of two, a wave's 64 words per step of the count and emit loops, `per = ceil(B / 256)` rows per thread of the scan, 64 line pairs
per step of a building pair, 256 target lines per LDS fill trip, 16 hypotheses per workgroup of the overlap test, and an arg-min that
strides 256 per lane before it merges four waves.  Alignment scenes: spreads under the +-1 ulp nudge within SPREAD and no unstable
hypothesis, so TOL_OVERLAP of test_building_overlap_cpu.py holds for them as it stands and nothing is left out of a comparison."""
import numpy as np
import pytest

import building_overlap_edge_cases as E
import building_overlap_reference as BR
from test_building_overlap_cpu import NUDGE_SEED, SPREAD, TOL_OVERLAP, check_alignment, driver, read_align, run_driver  # noqa: F401 (driver: a fixture)

W = lambda j: j // E.WAVE


def _rows(pairs, B):
    return np.bincount(pairs[:, 0], minlength=B)


def _sorted_i_then_j(p):
    return np.all(p[:, 0] < p[:, 1]) and np.array_equal(p, p[np.lexsort((p[:, 1], p[:, 0]))])


# ---- pair search ----------------------------------------------------------------------------------------------------------------------
def test_words_past_the_64th():
    bl, _ = E.pair_scenes()["words66"]
    p = E.pair_result("words66")
    B = len(bl)
    assert B == 4161 and (B + 63) // 64 == 66 and [k for k, b in enumerate(bl) if b.shape[0]] == list(E.WORDS66_AT)
    assert p.tolist() == [[i, j] for i in E.WORDS66_AT for j in E.WORDS66_AT if i < j] and p.shape[0] == 28
    assert p[:5].tolist() == [[0, 63], [0, 64], [0, 65], [0, 4095], [0, 4096]]
    words = {i: W(p[p[:, 0] == i, 1]) for i in np.unique(p[:, 0])}
    assert any(w.min() == 0 and w.max() >= 64 for w in words.values())       # one row: a pair in word 0 and one past a wave's first 64 words
    assert any(w[0] >= 64 for w in words.values())                           # a row whose first pair is in such a word
    assert any(w.min() - W(i + 1) < 64 <= w.max() - W(i + 1) for i, w in words.items())   # the emit loop carries a count into its second step
    assert p[-1].tolist() == [B - 2, B - 1]


def test_dense_rows():
    bl, _ = E.pair_scenes()["clique130"]
    p = E.pair_result("clique130")
    assert len(bl) == 130 and p.shape[0] == 8385 and p.tolist() == [[i, j] for i in range(130) for j in range(i + 1, 130)]
    row0 = p[p[:, 0] == 0, 1]
    per_word = np.bincount(W(row0))
    # 129 bits over three words.  Word 1 is full: lane 63 with every lower bit set.  Word 0 lacks only bit 0, which is the row itself
    assert row0.size == 129 and per_word.tolist() == [63, 64, 2]
    assert [int(np.count_nonzero(W(p[p[:, 0] == i, 1]) == 1)) for i in (0, 63, 64)] == [64, 64, 63]
    assert p[E.position(p, 0, 70)].tolist() == [0, 70] and E.position(p, 0, 70) == 69              # mid-row, mid-word
    assert E.position(p, 1, 64) == 129 + 62                                                          # the first bit of row 1's second word


@pytest.mark.parametrize("B", [130, 129, 128])
def test_rows_and_columns_at_word_and_tile_edges(B):
    bl, _ = E.pair_scenes()["rows%d" % B]
    p = E.pair_result("rows%d" % B)
    want = E.planted_alignment_pairs(B)
    assert len(bl) == B and p.tolist() == [list(x) for x in want]                                    # exactly these, nothing else
    assert len(want) == {130: 16, 129: 12, 128: 8}[B]
    if B == 130:
        assert want == [(62, 63), (62, 127), (62, 128), (62, 129), (63, 64), (63, 127), (63, 128), (63, 129), (64, 65), (64, 127), (64, 128),
                        (64, 129), (65, 66), (65, 127), (65, 128), (65, 129)]
    # rows 62 and 63 share a tile that starts in chunk 0 while row 63 reads from chunk 1; the last tile has one row or two
    assert ((62 + 1) // 64, (63 + 1) // 64) == (0, 1) and (B % E.TILE_ROWS == 1) == (B == 129)


@pytest.mark.parametrize("B", E.SCAN_SIZES)
def test_scan_ownership_scenes(B):
    bl, _ = E.pair_scenes()["scan%d" % B]
    p = E.pair_result("scan%d" % B)
    rows = _rows(p, B)
    frac = np.unique(p).size / B
    print(B, "pairs", p.shape[0], "buildings in a pair", frac, "row counts", np.bincount(rows).tolist())
    assert len(bl) == B and _sorted_i_then_j(p)
    assert 0.05 < frac < 0.7 and np.unique(rows).size >= 3                                           # non-uniform row counts
    assert [0, B - 1] in p.tolist() and p[-1].tolist() == [B - 2, B - 1] and p[0].tolist() == [0, B - 1]
    per = -(-B // E.BLOCK)
    owners = -(-B // per)
    assert per == {255: 1, 256: 1, 257: 2, 511: 2, 512: 2, 513: 3, 4097: 17}[B]
    assert (owners < E.BLOCK) == (B in (255, 257, 513, 4097)) and (B % per != 0) == (B in (257, 511))       # idle threads; a partly filled last owner
    assert rows[0] > 0 and rows[B - 2] > 0 and rows[B - 1] == 0             # counts in the first owner's range and in the last row that can have one


def test_the_fixture_pair_list_is_the_restatement():
    for name in E.GOLDEN:
        assert np.array_equal(E.pair_result(name), E.pair_result_fresh(name))


def test_scan_with_64_rows_per_thread():
    bl, _ = E.pair_scenes()["scan_sparse"]
    p = E.pair_result("scan_sparse")
    B = len(bl)
    assert B == 1 << 14 and -(-B // E.BLOCK) == 64 and 18 <= p.shape[0] <= 22
    assert p.tolist() == sorted(list(x) for x in E.SPARSE_PAIRS)
    assert sum(b.shape[0] for b in bl) < 64                                                          # otherwise empty
    owner = np.unique(p[:, 0] // 64)
    assert owner.size >= 8 and owner[0] == 0 and owner[-1] == E.BLOCK - 1                            # first and last thread own pairs
    assert {0, 63} <= set((p[:, 0] % 64).tolist())                                                   # an owner's first and last row


def test_line_pair_space():
    a, b, ca, cb = E.picket_pair()
    assert a.shape[0] == b.shape[0] == 512
    hit = BR.lines_intersected(BR.shrink(a, ca)[:, None], BR.shrink(b, cb)[None, :])
    assert hit.shape == (512, 512) and np.argwhere(hit).tolist() == [[511, 511]]                     # p = La * Lb - 1 alone
    a, b, ca, cb = E.picket_pair(parallel=True)
    assert not BR.lines_intersected(BR.shrink(a, ca)[:, None], BR.shrink(b, cb)[None, :]).any()
    s = E.pair_scenes()
    assert E.pair_result("last_line_pair").tolist() == [[0, 1]] and E.pair_result("no_line_pair").shape == (0, 2)
    assert [x.shape[0] for x in s["tile_512_3"][0]] == [512, 3, 512] and E.pair_result("tile_512_3").tolist() == [[0, 2], [1, 2]]
    assert [x.shape[0] for x in s["tile_none_512"][0]] == [0, 512, 3, 512] and E.pair_result("tile_none_512").tolist() == [[1, 3], [2, 3]]


def test_appended_clique_leaves_the_planted_list():
    bl, ce = E.pair_scenes()["rows130"]
    more, mce = E.far(E.pair_scenes()["clique130"])
    got = BR.overlapped_pairs(bl + more + [E.NONE], np.concatenate([ce, mce, [[0.0, 0.0, 0.0]]]))
    assert np.array_equal(got[np.all(got < 130, axis=1)], E.pair_result("rows130"))
    assert np.array_equal(got[np.all(got >= 130, axis=1)] - 130, E.pair_result("clique130"))
    assert not np.any((got[:, 0] < 130) & (got[:, 1] >= 130))


@pytest.mark.parametrize("name", E.PAIR_NAMES)
def test_host_header_pair_search_equals_the_restatement(driver, tmp_path, name):
    bl, ce = E.pair_scenes()[name]
    ip, op = str(tmp_path / "b.bin"), str(tmp_path / "p.bin")
    BR.write_buildings(ip, bl, ce)
    res = run_driver(driver, "host", "pairs", ip, op)
    assert res["ok"] and res["n"] == len(bl)
    assert np.array_equal(np.fromfile(op, np.int32).reshape(-1, 2), E.pair_result(name))            # exactly, order included


# ---- alignment ------------------------------------------------------------------------------------------------------------------------
def align_cases():
    """name -> item: every alignment item of the edge cases (the 4096-item batch repeats the prototypes)"""
    c = {n: E.twin_item(n) for n in E.TWIN_CASES}
    c.update({"past_255_Lt%d" % Lt: E.past_255(Lt) for Lt in E.PAST_255})
    c.update({"source_limit_Lt%d" % Lt: E.source_limit(Lt) for Lt in (1, 2, 257)})
    c.update({"unit%d" % k: it for k, it in enumerate(E.batch_units())})
    c.update({"prototype%d" % k: it for k, it in enumerate(E.prototypes())})
    return c


ALIGN_NAMES = (list(E.TWIN_CASES) + ["past_255_Lt%d" % Lt for Lt in E.PAST_255] + ["source_limit_Lt%d" % Lt for Lt in (1, 2, 257)] +
               ["unit%d" % k for k in range(13)] + ["prototype%d" % k for k in range(8)])


@pytest.mark.parametrize("name", ALIGN_NAMES)
def test_spread_and_unstable_hypotheses(name):
    item = align_cases()[name]
    a, b = E.restated(item), E.restated(item, NUDGE_SEED)
    un, s_hyp, s_final = BR.compare_runs(a, b)
    print(name, "hypotheses", a["gate"].size, "edge pairs", a["n_edge"], "unstable", un.size, "spreads", s_hyp, s_final, "winner", a["winner"],
          "margin", BR.margin(a))
    assert max(s_hyp, s_final) <= SPREAD
    assert un.size == 0                                                    # nothing is left out of a comparison
    assert a["winner"] == BR.own_rule_winner(a["gate"], a["tn"])
    assert max(np.abs(x).max(initial=0.0) for x in item[:2]) < 65.0        # coordinates as large as the scenes TOL_OVERLAP was measured on


@pytest.mark.parametrize("name", list(E.TWIN_CASES))
def test_twins(name):
    item = E.twin_item(name)
    lo, hi = E.TWIN_CASES[name][2]
    r = E.restated(item)
    assert item[0].shape[0] == 1 and r["n_edge"] == 0 and r["gate"].size == item[1].shape[0]      # one source line: h is the target line
    ok = r["gate"] == BR.GATE_PASS
    assert np.nonzero(ok & (r["tn"] == r["tn"][r["winner"]]))[0].tolist() == [lo, hi]              # bit-equal norms at exactly these
    assert np.array_equal(r["rotation"][lo], r["rotation"][hi]) and np.array_equal(r["translation"][lo], r["translation"][hi])
    assert r["winner"] == lo == BR.own_rule_winner(r["gate"], r["tn"]) and BR.margin(r) > 0.1     # the lower h wins, by the rule and by far
    lane, wave, trip = (lambda h: h % E.BLOCK % E.WAVE), (lambda h: h % E.BLOCK // E.WAVE), (lambda h: h // E.BLOCK)
    if name.startswith("trip"):
        assert hi == lo + E.BLOCK and (lane(lo), wave(lo)) == (lane(hi), wave(hi)) and trip(hi) == trip(lo) + 1
        assert (wave(lo), lane(lo)) == {"trip_lane0": (0, 0), "trip_wave3": (3, 8), "trip_last_lane": (3, 63)}[name]
    else:
        assert (wave(lo), wave(hi), trip(lo), trip(hi)) == {"waves_1_3": (1, 3, 0, 0), "waves_3_0": (3, 0, 0, 1)}[name]
    if name == "waves_3_0":
        assert r["tn"][hi % E.BLOCK] > r["tn"][hi]                         # the twin's lane held a larger norm from its first trip


@pytest.mark.parametrize("Lt", list(E.PAST_255))
def test_overlap_decided_past_line_255(Lt):
    item = E.past_255(Lt)
    Ls, bands = E.PAST_255[Lt]
    r = E.restated(item)
    assert (item[0].shape[0], item[1].shape[0]) == (Ls, Lt) and 1 <= Ls <= 3 and r["n_edge"] == 0 and r["gate"].size == Ls * Lt
    h = np.arange(r["gate"].size)
    for part in (h < 256, h >= 256):
        assert {BR.GATE_PASS, BR.GATE_OVERLAP} <= set(r["gate"][part].tolist())
    assert r["winner"] >= 0 and BR.margin(r) > TOL_OVERLAP
    if Lt > 256:                                                            # Lt = 256 fills LDS in exactly one trip: the control
        cut, whole = E.overlap_gates_without_lines_from(item, 256)
        only = (cut == BR.GATE_PASS) & (whole == BR.GATE_OVERLAP)           # overlapped only because of target lines 256 and up
        assert only.any() and np.array_equal(cut != whole, only)
        assert Lt - len(bands) >= 256                                       # every blocker is such a line


@pytest.mark.parametrize("Lt", [1, 2, 257])
def test_source_limit(Lt):
    item = E.source_limit(Lt)
    r = E.restated(item)
    assert (item[0].shape[0], item[1].shape[0]) == (256, Lt) and r["n_edge"] == 0 and r["gate"].size == 256 * Lt
    assert r["n_angle_passed"] == 256 and r["winner"] >= 0 and BR.margin(r) > TOL_OVERLAP
    assert r["winner"] // Lt > 160 and r["winner"] % Lt == 0                # a late source line onto target line 0
    if Lt >= 2:
        assert {BR.GATE_PASS, BR.GATE_OVERLAP, BR.GATE_ANGLE} == set(r["gate"].tolist())
    if Lt == 257:
        cut, whole = E.overlap_gates_without_lines_from(item, 256)
        only = (cut == BR.GATE_PASS) & (whole == BR.GATE_OVERLAP)
        assert r["gate"].size == 65792 and only.any() and np.array_equal(cut != whole, only) and not np.any(cut == BR.GATE_OVERLAP)


def test_unit_table_batch():
    items = E.batch_units()
    res = [E.restated(it) for it in items]
    H = [r["gate"].size for r in res]
    assert tuple(H) == E.UNIT_H == (0, 1, 15, 16, 17, 0, 0, 31, 32, 33, 16, 1, 0) and all(r["n_edge"] == 0 for r in res)
    assert [H[k] for k in (0, 5, 6, 12)] == [0, 0, 0, 0] and {(it[0].shape[0] == 0, it[1].shape[0] == 0) for it, h in zip(items, H) if h == 0} == \
        {(True, False), (False, True), (True, True)}                        # first, last, back to back; either side empty, or both
    assert {h % E.UNITS for h in H if h} == {0, 1, 15} and any(h % E.UNITS and H[k + 1] for k, h in enumerate(H[:-1]))   # a partly filled last workgroup, then an item
    for r in res:
        if r["gate"].size > E.UNITS and r["gate"].size % E.UNITS == 1:
            assert r["gate"][-1] == BR.GATE_OVERLAP                         # the last workgroup's only hypothesis: skipping it would show
    assert sum(1 for r in res if {BR.GATE_PASS, BR.GATE_OVERLAP, BR.GATE_ANGLE} <= set(r["gate"].tolist())) >= 4
    assert all((r["winner"] >= 0) == (r["gate"].size > 0) for r in res)


def test_item_limit_prototypes():
    protos = E.prototypes()
    res = [E.restated(it) for it in protos]
    assert len(protos) == 8 and E.MAX_ITEMS % 8 == 0
    assert any(r["gate"].size == 0 for r in res) and any(it[0].shape[0] == it[1].shape[0] == 1 for it in protos)
    assert sum(1 for r in res if r["n_edge"] > 0) >= 2                      # edge offsets move through the batch too
    assert sum(r["gate"].size for r in res) * (E.MAX_ITEMS // 8) < E.MAX_HYPOTHESES


def test_hypothesis_limit_batch():
    items = E.over_the_hypothesis_limit()
    src, trg = items[0][:2]
    assert len(items) == 17 and all(it is items[0] for it in items) and (src.shape[0], trg.shape[0]) == (256, 512)
    assert E._edges_once(src).shape[0] == 0 and E._edges_once(trg).shape[0] == 0                     # no edge pairs: H = 256 * 512 an item
    assert 16 * 256 * 512 == E.MAX_HYPOTHESES < 17 * 256 * 512


def _host(driver, tmp_path, items):
    ip, op = str(tmp_path / "i.bin"), str(tmp_path / "o.bin")
    BR.write_items(ip, items)
    res = run_driver(driver, "host", "align", ip, op)
    assert res["ok"] and res["n"] == len(items)
    return read_align(op, items)


@pytest.mark.parametrize("name", ALIGN_NAMES[:11])
def test_host_header_alignment_equals_the_restatement_on_scenes(driver, tmp_path, name):
    item = align_cases()[name]
    got = _host(driver, tmp_path, [item])[0]
    check_alignment(got, E.restated(item), E.restated(item, NUDGE_SEED))
    if name in E.TWIN_CASES:
        assert got["winner"] == E.TWIN_CASES[name][2][0]


@pytest.mark.parametrize("which", ["units", "prototypes"])
def test_host_header_alignment_equals_the_restatement_on_batches(driver, tmp_path, which):
    items = E.batch_units() if which == "units" else E.prototypes()
    for it, got in zip(items, _host(driver, tmp_path, items)):
        check_alignment(got, E.restated(it), E.restated(it, NUDGE_SEED))
