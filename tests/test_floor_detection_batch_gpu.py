"""dgs_floor_detection_batch on the MI355X: detect() over many scans in one device call against detect() scan by scan
on a second detector with the same parameters.  Same device, same bodies, same flags: every comparison is np.array_equal on the
float32 bits or equality of integers, no tolerance anywhere.  One parameter set and one tilt pair serve a batch, so the scenes of
tests/floor_detection_cases.py go in by cloud and draw stream under the batch's common parameters; what a scene is meant to provoke
(a status, a failed walk, a grown draw list) is asserted on the single call's answer before the batch is compared with it."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import floor_detection_cases as K
import floor_detection_reference as R

pytestmark = pytest.mark.gpu
F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the trace fields that do not describe launch shape
TRACE_KEYS = ("n_clipped", "n_filtered", "draws", "iterations", "winner_rank", "sample", "count", "ransac_failed")


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def _detector(params, registration=None):
    from delta_graph_slam_amd.floor_detection import FloorDetector
    return FloorDetector(dict(params), registration=registration)


def _single(det, cloud, raw, tilt, tilt_inv):
    """detect() alone -> everything the batch is compared with"""
    co = det.detect(cloud, raw, tilt, tilt_inv)
    clipped, nv = det.clipped()
    return dict(status=det.status, coeffs=co, clipped=clipped, normals=nv, filtered=det.filtered(), inliers=det.inliers(), trace=det.trace())


def _assert_scan_equal(bat, i, co, want, where=""):
    assert bat.statuses[i] == want["status"], (where, i, bat.statuses[i], want["status"])
    if want["coeffs"] is None:
        assert co is None, (where, i)
    else:
        assert co is not None and np.array_equal(_bits(co), _bits(want["coeffs"])), (where, i)
    clipped, nv = bat.batch_clipped(i)
    assert np.array_equal(_bits(clipped), _bits(want["clipped"])), (where, i)
    assert (nv is None) == (want["normals"] is None)
    if nv is not None:
        assert np.array_equal(_bits(nv), _bits(want["normals"])), (where, i)
    assert np.array_equal(_bits(bat.batch_filtered(i)), _bits(want["filtered"])), (where, i)
    t, wt = bat.batch_trace(i), want["trace"]
    assert {k: t[k] for k in TRACE_KEYS} == {k: wt[k] for k in TRACE_KEYS}, (where, i)
    assert np.array_equal(_bits(t["raw_coeffs"]), _bits(wt["raw_coeffs"])) and _bits(t["dot"]) == _bits(wt["dot"]), (where, i)
    idx, pts = bat.batch_inliers(i)
    assert np.array_equal(idx, want["inliers"][0]) and np.array_equal(_bits(pts), _bits(want["inliers"][1])), (where, i)
    if t["winner_rank"] >= 0 and bat.statuses[i] != "RNG_EXHAUSTED":
        assert len(idx) == t["count"], (where, i)          # the scored count IS the length of the inlier list: the decisions rest on it
    return t


def _compare(params, scans, tilt_deg=0.0, device=False, bat=None, one=None, singles=None, where=""):
    """scans: [(cloud, raw or None)].  -> (batch detector, single results, batch traces)"""
    bat = bat or _detector(params)
    one = one or _detector(params)
    tilt, tilt_inv = R.tilt_matrices(tilt_deg)
    if singles is None:
        singles = [_single(one, c, r, tilt, tilt_inv) for c, r in scans]
    clouds = [np.ascontiguousarray(c, F) for c, _ in scans]
    if device:
        import torch
        clouds = [torch.from_numpy(c).cuda() for c in clouds]
    cos = bat.detect_batch(clouds, [r for _, r in scans], tilt, tilt_inv)
    assert len(cos) == len(scans) == len(bat.statuses)
    traces = [_assert_scan_equal(bat, i, cos[i], singles[i], where) for i in range(len(scans))]
    return bat, singles, traces


def _dense(n, rank, seed):
    """60 % of n points on a plane, the rest clutter far from it; clutter triples at every rank but `rank`, which holds three plane
    points: the walk closes right behind it once it > 19"""
    rng = np.random.default_rng(seed)
    m = int(0.6 * n)
    pts = np.ones((n, 4), F)
    xy = rng.uniform(-10, 10, (m, 2))
    pts[:m, 0], pts[:m, 1], pts[:m, 2] = xy[:, 0], xy[:, 1], -2.0 + 0.01 * xy[:, 0]
    cl = rng.uniform(-10, 10, (n - m, 3))
    cl[:, 2] = rng.uniform(2.0, 10.0, n - m)
    pts[m:, :3] = cl
    pts = pts[rng.permutation(n)]
    on = np.nonzero(pts[:, 2] < 0)[0]
    off = np.nonzero(pts[:, 2] > 0)[0]
    tr = K._triples(rng, off, 1001)
    tr[rank] = tuple(int(v) for v in on[:3])
    return pts, R.raw_for_triples(n, tr)


# ---- 1. sizes side by side -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("device", [False, True])
def test_sizes_side_by_side(device):
    full = K.two_planes(2 * K.TILE + 1, seed=2)[0]
    sizes = (0, 1, 2, 3, 63, 64, 65, 255, 256, 257, K.TILE - 1, K.TILE, K.TILE + 1, 2 * K.TILE + 1)
    bat, singles, traces = _compare(dict(K.OPEN, floor_pts_thresh=1), [(full[:n], None) for n in sizes], device=device)
    assert singles[0]["status"] == "TOO_FEW_POINTS" and singles[1]["trace"]["ransac_failed"] == 1
    assert all(s["trace"]["iterations"] > 0 for s in singles[3:])                      # the RANSAC ran
    c = bat.batch_counts()
    assert c[2] == len(sizes) and c[3] == len(sizes) - 3 and c[5] == 1


# ---- 2. place independence -----------------------------------------------------------------------------------------------------
def test_a_scans_result_does_not_depend_on_its_place_or_its_neighbours():
    prm = dict(use_normal_filtering=1)
    a = (K.planted(5.0, True)["cloud"], None)
    others = [(K.planted(5.0, True, seed=s)["cloud"], None) for s in (21, 22, 23)] + [(K.planted_empty_band()["cloud"], None), (np.zeros((0, 4), F), None)]
    bat, one = _detector(prm), _detector(prm)
    want = _single(one, a[0], None, *R.tilt_matrices(5.0))
    assert want["status"] == "DETECTED"
    for order in ([a] + others[:3], others[:2] + [a] + others[2:], others[3:] + [a], [others[4], others[0], a], [a]):
        at = [i for i, s in enumerate(order) if s is a][0]
        _, singles, _ = _compare(prm, order, tilt_deg=5.0, bat=bat, one=one)
        for k in ("status",):
            assert singles[at][k] == want[k]
        assert np.array_equal(_bits(singles[at]["coeffs"]), _bits(want["coeffs"]))     # and the batch equals singles[at] (checked in _compare)


# ---- 3. compaction edges -------------------------------------------------------------------------------------------------------
def test_compaction_edges():
    prm = dict(use_normal_filtering=1)
    full_a, full_b = R.floor_scene(2600, 300, seed=31), R.floor_scene(2500, 400, seed=32)
    full_a[-1, :3] = (0.5, 0.5, -2.0)                                                  # kept last point ...
    full_b[0, :3] = (0.25, -0.5, -2.0)                                                 # ... next to a kept first point
    above = R.floor_scene(700, 0, seed=33)
    above[:, 2] += F(50.0)                                                             # the clip empties it
    rng = np.random.default_rng(34)
    wall = np.ones((900, 4), F)                                                        # horizontal normals: the normal rule empties it
    wall[:, 0] = 5.0
    wall[:, 1] = rng.uniform(-5, 5, 900)
    wall[:, 2] = rng.uniform(-2.9, -1.1, 900)
    bat, singles, _ = _compare(prm, [(full_a, None), (above, None), (full_a, None), (full_b, None), (wall, None), (full_b, None)])
    assert singles[1]["trace"]["n_clipped"] == 0 and singles[1]["status"] == "TOO_FEW_POINTS"
    assert singles[4]["trace"]["n_clipped"] == 900 and singles[4]["trace"]["n_filtered"] == 0
    assert singles[0]["status"] == singles[3]["status"] == "DETECTED"
    assert np.array_equal(singles[0]["clipped"][-1, :3], full_a[-1, :3]) and np.array_equal(singles[3]["clipped"][0, :3], full_b[0, :3])


def test_the_scan_kernels_second_chunk_begins_inside_a_scan():
    prm = dict(use_normal_filtering=1)
    scans = [(R.floor_scene(4700 + 7 * (i % 5), 300, seed=100 + i), None) for i in range(56)]
    assert sum((c.shape[0] + 255) // 256 for c, _ in scans) == 1120                    # workgroups of the first stage
    bat, singles, _ = _compare(prm, scans)
    assert all(s["status"] == "DETECTED" for s in singles)
    c = bat.batch_counts()
    assert c[1] == 3 and c[4] == 0 and c[6] == 56


# ---- 4. rounds -----------------------------------------------------------------------------------------------------------------
def _round_scans():
    scans = []
    for i, rank in enumerate(K.RANKS):
        c = K.rank_edge(K.SIZES[i % len(K.SIZES)], rank)
        scans.append((c["cloud"], c["raw"]))
    scans.insert(1, _dense(K.TILE + 1, 5, seed=41))                                    # closes in round 1
    scans.insert(4, _dense(2 * K.TILE + 1, 100, seed=42))                              # closes in round 2
    return scans


def test_scans_close_in_different_rounds_of_one_call():
    scans = _round_scans()
    bat, singles, traces = _compare(K.OPEN, scans)
    chunks = [s["trace"]["chunks_launched"] for s in singles]
    assert sorted(set(chunks)) == [1, 2, 3]
    assert [t["chunks_launched"] for t in traces] == chunks                            # how far each scan's own scoring went
    assert [t["winner_rank"] for t in traces] == [K.RANKS[0], 5, K.RANKS[1], K.RANKS[2], 100] + list(K.RANKS[3:])
    c = bat.batch_counts()
    assert c[7] == max(chunks) == 3 and c[4] == 0 and c[1] == 1 + 3                    # one wait for the clip, one per round
    # the same batch under other chunk sizes: identical results
    small = dict(K.OPEN, hyp_chunk_first=1, hyp_chunk=3)
    bat2, _, traces2 = _compare(small, scans, singles=singles)
    assert bat2.batch_counts()[7] == 1 + 334


# ---- 5. walk ends --------------------------------------------------------------------------------------------------------------
def test_walk_ends_in_one_batch():
    prm = dict(K.OPEN, max_iterations=40)
    b999, b1000, behind, quirk = K.bad_run(999), K.bad_run(1000), K.run_behind_the_stop(), K.quirk_cloud()
    stop = K.rank_edge(K.TILE + 1, 40, max_iterations=40)
    scans = [(b999["cloud"], b999["raw"]), (behind["cloud"], behind["raw"]), (b1000["cloud"], b1000["raw"]), (stop["cloud"], stop["raw"]),
             (b999["cloud"], np.zeros(2, np.uint32)),                                  # not one draw
             (quirk["cloud"], quirk["raw"]),
             (b999["cloud"], b999["raw"][:3 * 200]),                                   # runs out when the list has to grow
             (behind["cloud"], None)]
    bat, singles, traces = _compare(prm, scans)
    st = [s["status"] for s in singles]
    assert st[4] == st[6] == "RNG_EXHAUSTED" and st[5] == "NOT_VERTICAL" and st[1] == st[7] == "DETECTED"
    assert singles[0]["trace"]["ransac_failed"] == 0 and singles[0]["trace"]["draws"] == 30 + 999 + 11
    assert singles[2]["trace"]["ransac_failed"] == 1 and singles[2]["status"] == "DETECTED"
    assert singles[3]["trace"]["iterations"] == 41 and singles[3]["trace"]["winner_rank"] == 40
    assert bat.batch_counts()[4] >= 1                                                  # the grown draw lists went through the single routine


# ---- 6. thresholds and orders --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("transform_order", [0, 1])
@pytest.mark.parametrize("plane_dot_order", [0, 1, 2])
def test_thresholds_and_orders(plane_dot_order, transform_order):
    orders = dict(plane_dot_order=plane_dot_order, transform_order=transform_order)
    n = K.TILE + 1
    edge = K.rank_edge(n, K.CHUNK_FIRST - 1)
    m1 = edge["m"] + 1
    scans = [(edge["cloud"], edge["raw"])]
    for ang, flip in ((9.9, False), (10.1, False), (9.9, True)):
        c = K.tilted_plane(ang, flip=flip)
        scans.append((c["cloud"], c["raw"]))
    seen = []
    for thresh in (100, m1, m1 + 1, n, n + 1):
        _, singles, _ = _compare(dict(K.OPEN, floor_pts_thresh=thresh, **orders), scans, where=f"thresh {thresh}")
        seen.append([s["status"] for s in singles])
    assert seen[0] == ["DETECTED", "DETECTED", "NOT_VERTICAL", "DETECTED"]
    assert [s[0] for s in seen] == ["DETECTED", "DETECTED", "TOO_FEW_INLIERS", "TOO_FEW_INLIERS", "TOO_FEW_POINTS"]
    # end to end with the normal filter on, a tilted sensor
    planted = [(K.planted(5.0, True)["cloud"], None), (K.planted_empty_band()["cloud"], None)]
    _, singles, _ = _compare(dict(use_normal_filtering=1, **orders), planted, tilt_deg=5.0)
    assert [s["status"] for s in singles] == ["DETECTED", "DETECTED"]


# ---- 7. counts and refusals ----------------------------------------------------------------------------------------------------
def test_launches_and_host_waits_do_not_grow_with_the_batch():
    scene = K.planted(5.0, True)["cloud"]
    for normal, waits in ((1, 3), (0, 2)):
        counts = []
        for b in (2, 7):
            bat, singles, traces = _compare(dict(use_normal_filtering=normal), [(scene, None)] * b, tilt_deg=5.0)
            assert all(t["chunks_launched"] == 1 for t in traces)
            counts.append(bat.batch_counts())
        assert counts[0][0] == counts[1][0] and counts[0][1] == counts[1][1] == waits  # launches, host waits
        assert counts[0][4] == counts[1][4] == 0 and counts[1][2] == counts[1][3] == 7 and counts[0][7] == 1


def test_the_empty_batch_and_call_level_refusals():
    import ctypes as C
    from delta_graph_slam_amd import _lib as L
    prm = dict(use_normal_filtering=0)
    bat = _detector(prm)
    assert bat.detect_batch([]) == [] and bat.statuses == [] and bat.batch_counts().tolist() == [0] * 8
    scene = K.planted(0.0, False)["cloud"]
    want = _single(_detector(prm), scene, None, *R.tilt_matrices(0.0))
    lib, h = bat._lib, bat._h
    t16, ti16 = bat._tilts(None, None)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    sizes = np.array([scene.shape[0], scene.shape[0]], np.int64)
    ptrs = (C.c_void_p * 2)(scene.ctypes.data, scene.ctypes.data)
    raw_n = np.zeros(2, np.int64)
    raws = (C.c_void_p * 2)(None, None)

    def call(params=bat.params, n=2, ptrs=ptrs, sizes=sizes, raws=raws, raw_n=raw_n, out=True):
        co, st = np.full((2, 4), 7.0, F), np.full(2, 7, np.int32)
        rc = lib.dgs_floor_detection_batch(h, C.byref(params), vp(t16), vp(ti16), n, ptrs, None if sizes is None else vp(sizes), 0, raws,
                                           None if raw_n is None else vp(raw_n), vp(co) if out else None, vp(st))
        return rc, co, st

    bad = L.FloorDetectionParams.from_buffer_copy(bat.params)
    bad.floor_pts_thresh = -1
    wrong_size = L.FloorDetectionParams.from_buffer_copy(bat.params)
    wrong_size.struct_size = 8
    refusals = [dict(params=bad), dict(params=wrong_size), dict(n=-1), dict(ptrs=None), dict(sizes=None), dict(out=False),
                dict(sizes=np.array([5, -1], np.int64)), dict(ptrs=(C.c_void_p * 2)(scene.ctypes.data, None)),
                dict(sizes=np.array([5, 2 ** 31], np.int64)), dict(sizes=np.array([2 ** 31 - 1, 2 ** 31 - 1], np.int64)),
                dict(raw_n=np.array([0, -3], np.int64)), dict(raw_n=np.array([0, 6], np.int64))]
    for kw in refusals:
        rc, co, st = call(**kw)
        assert rc == 1 and np.all(co == 7.0) and np.all(st == 7), kw                   # nothing written
    rc, co, st = call()
    assert rc == 0 and st.tolist() == [0, 0] and np.array_equal(_bits(co[1]), _bits(want["coeffs"]))
    with pytest.raises(L.DgsError):
        bat.batch_trace(2)                                                             # scan numbers beyond the last batch
    with pytest.raises(ValueError):
        bat.detect_batch([scene], rng_raws=[None, None])


def test_a_large_batch_before_a_small_one():
    prm = dict(use_normal_filtering=1)
    bat, one = _detector(prm), _detector(prm)
    big = [(R.floor_scene(3000 + 11 * i, 300, seed=60 + i), None) for i in range(9)]
    small = [(R.floor_scene(400, 50, seed=70), None), (R.floor_scene(900, 80, seed=71), None)]
    _compare(prm, big, bat=bat, one=one)
    _compare(prm, small, bat=bat, one=one)
    with pytest.raises(Exception):
        bat.batch_trace(2)                                                             # the getters speak of the last batch only
    _compare(prm, big[:3], bat=bat, one=one)


_CHUNKED = r"""
import json, sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import floor_detection_reference as R
from delta_graph_slam_amd.floor_detection import FloorDetector
prm = dict(use_normal_filtering=1)
bat, one = FloorDetector(prm), FloorDetector(prm)
scans = [R.floor_scene(1500 + 100 * i, 200, seed=80 + i) for i in range(5)] + [np.zeros((0, 4), np.float32)]
cos = bat.detect_batch(scans)
ok = True
for i, c in enumerate(scans):
    co = one.detect(c)
    ok = ok and bat.statuses[i] == one.status and (co is None) == (cos[i] is None)
    ok = ok and (co is None or np.array_equal(co.view(np.uint32), cos[i].view(np.uint32)))
    ok = ok and np.array_equal(bat.batch_filtered(i).view(np.uint32), one.filtered().view(np.uint32))
    ok = ok and np.array_equal(bat.batch_inliers(i)[0], one.inliers()[0])
    ok = ok and np.array_equal(bat.batch_clipped(i)[1].view(np.uint32), one.clipped()[1].view(np.uint32))
print(json.dumps(dict(ok=bool(ok), counts=bat.batch_counts().tolist(), statuses=bat.statuses)))
"""


def test_a_small_point_budget_cuts_the_call_into_chunks(tmp_path):
    script = tmp_path / "chunked.py"
    script.write_text(_CHUNKED)
    env = dict(os.environ, DGS_FLOOR_BATCH_POINTS="3500")
    p = subprocess.run([sys.executable, str(script), ROOT], capture_output=True, text=True, env=env, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    res = json.loads(p.stdout.strip().splitlines()[-1])
    assert res["ok"] and res["counts"][5] == 4 and res["counts"][2] == 6               # 1700 + 1800 | 1900 | 2000 | 2100 + the empty scan
    assert res["statuses"][:5] == ["DETECTED"] * 5 and res["statuses"][5] == "TOO_FEW_POINTS"


# ---- 8. neighbours on the handle -----------------------------------------------------------------------------------------------
def test_single_detect_registration_and_prefilter_on_the_same_handle():
    from delta_graph_slam_amd import synth
    from delta_graph_slam_amd.prefilter import Prefilter
    from delta_graph_slam_amd.registration import Registration
    prm = dict(use_normal_filtering=1)
    c = K.planted(5.0, True)
    tilt, tilt_inv = c["tilt"], c["tilt_inv"]
    scan = K.raw_scan("vlp16")
    tgt, src, _ = synth.planar_pair(n=8192)
    ref = Registration("NDT_OMP", ndt_resolution=1.0)
    ref.setInputTarget(tgt)
    ref.setInputSource(src)
    ref.align()
    f3, f2 = Prefilter().cloud_callback(scan)
    want = _single(_detector(prm), c["cloud"], None, tilt, tilt_inv)

    r = Registration("NDT_OMP", ndt_resolution=1.0)
    det = _detector(prm, registration=r)
    r.setInputTarget(tgt)
    r.setInputSource(src)
    got = _single(det, c["cloud"], None, tilt, tilt_inv)
    others = [(K.planted(5.0, True, seed=s)["cloud"], None) for s in (51, 52)]
    _compare(prm, others + [(c["cloud"], None)], tilt_deg=5.0, bat=det, one=_detector(prm))
    # the single getters still speak of the single detect
    assert det.status == got["status"] and np.array_equal(_bits(det.filtered()), _bits(want["filtered"]))
    assert np.array_equal(det.inliers()[0], want["inliers"][0]) and det.trace()["count"] == want["trace"]["count"]
    assert np.array_equal(_bits(det.clipped()[1]), _bits(want["normals"]))
    g3, g2 = Prefilter(registration=r).cloud_callback(scan)
    assert np.array_equal(_bits(g3), _bits(f3)) and np.array_equal(_bits(g2), _bits(f2))
    r.align()
    assert np.array_equal(r.getFinalTransformation(), ref.getFinalTransformation())
    again = _single(det, c["cloud"], None, tilt, tilt_inv)                               # a single detect after the batch
    assert again["status"] == want["status"] and np.array_equal(_bits(again["coeffs"]), _bits(want["coeffs"]))
    assert np.array_equal(again["inliers"][0], want["inliers"][0])
    assert np.array_equal(_bits(det.batch_filtered(0)), _bits(_single(_detector(prm), others[0][0], None, tilt, tilt_inv)["filtered"]))


# ---- 9. pipeline ---------------------------------------------------------------------------------------------------------------
def test_two_streams_by_three_frames_through_the_batched_prefilter():
    import torch
    from delta_graph_slam_amd import synth
    from delta_graph_slam_amd.prefilter import Prefilter
    prm = dict(K.SCAN_PARAMS, use_normal_filtering=1)
    pf_b, pf_1 = Prefilter(), Prefilter()
    bat, one = _detector(prm), _detector(prm)
    for frame in range(3):
        raws = []
        for stream in range(2):
            xyz, _ = synth.street_scan((-30.0 + 0.4 * frame + 5.0 * stream, 1.0, 0.1), 16, (15.0, -15.0), 1875, 21 + stream)
            raws.append(torch.from_numpy(synth._xyz1(xyz)).cuda())
        outs, statuses = pf_b.filter_scan_batch(raws)
        assert statuses.tolist() == [0, 0]
        f3 = [o[0] for o in outs]
        assert all(t.is_cuda for t in f3)                                                # they go in as they are
        cos = bat.detect_batch(f3)
        for s in range(2):
            g3 = pf_1.filter_scan(raws[s])[0]
            want = _single(one, g3, None, *R.tilt_matrices(0.0))
            _assert_scan_equal(bat, s, cos[s], want, f"frame {frame}")
            assert want["status"] == "DETECTED"
        assert bat.batch_counts()[1] == 3


# ---- 10. the C++ driver --------------------------------------------------------------------------------------------------------
def test_cpp_driver_matches_the_python_path(tmp_path):
    exe = str(tmp_path / "floor_detection_batch_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "tests", "stub_eigen"), "-I", os.path.join(ROOT, "tests", "stub_pcl"),
                           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "floor_detection_batch_driver.cpp"), "-o", exe,
                           os.path.join(ROOT, "delta_graph_slam_amd", "libdgs_reg.so"), "-Wl,-rpath," + os.path.join(ROOT, "delta_graph_slam_amd"),
                           "-Wl,-rpath,/opt/rocm/lib"])
    prm = dict(use_normal_filtering=1, sensor_height=2.0)
    scans = [R.floor_scene(2600, 700, seed=11), R.floor_scene(300, 40, seed=12), np.zeros((0, 4), F), R.floor_scene(1800, 300, seed=13)]
    args = [exe, str(len(scans))]
    for i, c in enumerate(scans):
        c.astype(F).tofile(str(tmp_path / f"in{i}.bin"))
        args += [str(tmp_path / f"in{i}.bin"), str(tmp_path / f"filtered{i}.bin"), str(tmp_path / f"floor{i}.bin")]
    args += [f"{k}={v}" for k, v in prm.items()]
    p = subprocess.run(args, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    res = json.loads(p.stdout.strip().splitlines()[-1])
    bat = _detector(prm)
    cos = bat.detect_batch(scans)                                                       # tilt_deg = 0: both paths build the exact identity
    from delta_graph_slam_amd import _lib as L
    assert [L.FD_STATUS[s] for s in res["status"]] == bat.statuses
    for i in range(len(scans)):
        if cos[i] is None:
            assert res["coeffs"][i] is None
        else:
            assert np.array_equal(_bits(np.array(res["coeffs"][i], F)), _bits(cos[i]))
        filtered = np.fromfile(str(tmp_path / f"filtered{i}.bin"), F).reshape(-1, 4)
        floor = np.fromfile(str(tmp_path / f"floor{i}.bin"), F).reshape(-1, 4)
        assert np.array_equal(_bits(filtered[:, :3]), _bits(bat.batch_filtered(i)[:, :3]))
        assert np.array_equal(_bits(floor[:, :3]), _bits(bat.batch_inliers(i)[1][:, :3]))
