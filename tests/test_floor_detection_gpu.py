"""FloorDetectionNodelet::detect on the MI355X against the numpy restatement tests/floor_detection_reference.py.  The filter stage is
compared on prefiltered synthetic scans (clipped cloud bit for bit, normal decisions outside the band); everything from the filtered
cloud on -- trace, inlier list, coefficients -- is bit-equal, so those comparisons carry no tolerance.  The conditions on the scenes
(band sizes, walk decisions away from ties, planted counts) are asserted by tests/test_floor_detection_cpu.py."""
import math

import numpy as np
import pytest

import floor_detection_cases as K
import floor_detection_reference as R

pytestmark = pytest.mark.gpu
F = np.float32
TRACE_KEYS = ("draws", "iterations", "winner_rank", "sample", "count", "ransac_failed")


def _detector(params, registration=None):
    from delta_graph_slam_amd.floor_detection import FloorDetector
    return FloorDetector({k: v for k, v in params.items()}, registration=registration)


def _run(c, det=None, cloud=None, **over):
    det = det or _detector(dict(c["params"], **over))
    co = det.detect(c["cloud"] if cloud is None else cloud, c["raw"], c["tilt"], c["tilt_inv"])
    return det, co


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def _assert_ransac_equal(det, co, ref):
    """status, trace, inlier list and coefficient bits against a restatement result (R.detect's or R.finish's)."""
    assert det.status == ref["status"]
    t, rt = det.trace(), ref["trace"]
    if rt is not None and ref["status"] != "RNG_EXHAUSTED":
        got = {k: (tuple(t[k]) if k == "sample" else t[k]) for k in TRACE_KEYS}
        want = {k: (tuple(int(v) for v in rt[k]) if k == "sample" else rt[k]) for k in TRACE_KEYS}
        assert got == want
        assert np.array_equal(_bits(t["raw_coeffs"]), _bits(rt["coeffs"]))
        if "dot" in rt:
            assert _bits(t["dot"]) == _bits(rt["dot"])
    idx, pts = det.inliers()
    assert np.array_equal(idx, ref["inliers"])
    if ref["coeffs"] is None:
        assert co is None
    else:
        assert np.array_equal(_bits(co), _bits(ref["coeffs"]))
    return t, idx, pts


def _assert_end_to_end(c, key, **over):
    ref = K.reference(key, c) if not over else R.detect(c["cloud"], dict(c["params"], **over), c["raw"], c["tilt"], c["tilt_inv"])
    det, co = _run(c, **over)
    assert np.array_equal(_bits(det.filtered()), _bits(ref["filtered"]))
    t, idx, pts = _assert_ransac_equal(det, co, ref)
    assert t["n_clipped"] == ref["clipped"].shape[0] and t["n_filtered"] == ref["filtered"].shape[0]
    assert np.array_equal(_bits(pts), _bits(ref["filtered"][ref["inliers"]]))
    return det, t, ref


# ---- filter stage ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["hdl64", "vlp16"])
def test_filter_stage_on_prefiltered_scans(kind):
    import torch
    from delta_graph_slam_amd.prefilter import Prefilter
    f3_dev, _ = Prefilter().cloud_callback(torch.from_numpy(K.raw_scan(kind)).cuda())
    assert f3_dev.is_cuda                                           # /filtered_points goes in where it lies
    f3 = f3_dev.cpu().numpy()
    for normal in (1, 0):
        c = K.case(f3, dict(K.SCAN_PARAMS, use_normal_filtering=normal))
        ref = K.reference(("scan_gpu", kind, normal), c)
        det, co = _run(c, cloud=f3_dev)
        clipped, nv = det.clipped()
        assert np.array_equal(_bits(clipped), _bits(ref["clipped"]))                    # bit for bit, in order
        if normal:
            cos_thr = math.cos(20.0 * math.pi / 180.0)
            keep_gpu = np.abs(nv[:, 2]).astype(np.float64) > cos_thr
            assert int(ref["band"].sum()) <= clipped.shape[0] // 100
            assert not np.any((keep_gpu != ref["keep"]) & ~ref["band"] & ~ref["tie"])   # decisions may differ only inside the band
            want = R.transform(clipped[keep_gpu], c["tilt_inv"])
            print(f"{kind}: clipped {clipped.shape[0]}, band {int(ref['band'].sum())}, ties {int(ref['tie'].sum())}, "
                  f"decisions that differ {int((keep_gpu != ref['keep']).sum())}")
        else:
            assert nv is None
            want = ref["filtered"]
        filtered = det.filtered()
        assert np.array_equal(_bits(filtered), _bits(want))
        assert np.array_equal(_bits(det.filtered(f3_dev).cpu().numpy()), _bits(want))
        # the RANSAC stage from the filtered cloud the device returned: exact
        _assert_ransac_equal(det, co, R.finish(filtered, c["params"], None, c["tilt_inv"]))
        assert det.status == "DETECTED" and det.trace()["chunks_launched"] == 1


@pytest.mark.parametrize("transform_order", [0, 1])
@pytest.mark.parametrize("plane_dot_order", [0, 1, 2])
def test_ransac_stage_is_exact_under_every_order(plane_dot_order, transform_order):
    c = K.planted(5.0, normal=True, plane_dot_order=plane_dot_order, transform_order=transform_order)
    det, co = _run(c)
    filtered = det.filtered()
    assert filtered.shape[0] > 2000
    t, _, _ = _assert_ransac_equal(det, co, R.finish(filtered, c["params"], None, c["tilt_inv"]))
    assert det.status == "DETECTED" and t["chunks_launched"] == 1 and t["hypotheses_scored"] == K.CHUNK_FIRST


# ---- end to end ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tilt_deg", [0.0, 5.0])
def test_end_to_end_without_the_normal_filter(tilt_deg):
    det, t, ref = _assert_end_to_end(K.planted(tilt_deg, False), ("planted", tilt_deg, False))
    assert det.status == "DETECTED" and t["chunks_launched"] == 1      # the common case: one host wait for the RANSAC


def test_end_to_end_with_an_empty_normal_band():
    det, t, ref = _assert_end_to_end(K.planted_empty_band(), "empty_band")
    assert det.status == "DETECTED" and int(ref["band"].sum()) == 0 and t["n_filtered"] == 44 * 44


def test_upstream_quirks():
    det, t, _ = _assert_end_to_end(K.quirk_cloud(), "quirk")
    assert det.status == "NOT_VERTICAL" and t["count"] == 700
    det, t, _ = _assert_end_to_end(K.diagonal_cloud(), "diagonal")
    assert det.status == "TOO_FEW_INLIERS" and t["ransac_failed"] == 1 and t["draws"] == 1000


# ---- kernel edges ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", K.SIZES)
@pytest.mark.parametrize("rank", K.RANKS)
def test_winner_at_chunk_edges_leading_through_the_last_point(n, rank):
    c = K.rank_edge(n, rank)
    det, t, ref = _assert_end_to_end(c, ("rank", n, rank))
    assert t["winner_rank"] == rank and t["count"] == c["m"] + 1 and t["iterations"] == 1001
    assert t["chunks_launched"] == 3 and t["hypotheses_scored"] == 1001


@pytest.mark.parametrize("n,rank", [(K.TILE + 1, K.CHUNK_FIRST), (2 * K.TILE + 1, K.CHUNK_FIRST + K.CHUNK + 1)])
def test_result_does_not_depend_on_the_chunk_sizes(n, rank):
    c = K.rank_edge(n, rank)
    a, ta, _ = _assert_end_to_end(c, ("rank", n, rank))
    b, tb, _ = _assert_end_to_end(c, ("rank", n, rank, "chunks"), hyp_chunk_first=1, hyp_chunk=3)
    assert tb["chunks_launched"] == 1 + 334 and ta["chunks_launched"] == 3
    assert {k: ta[k] for k in TRACE_KEYS} == {k: tb[k] for k in TRACE_KEYS}
    assert np.array_equal(_bits(ta["raw_coeffs"]), _bits(tb["raw_coeffs"])) and np.array_equal(a.inliers()[0], b.inliers()[0])


def test_max_iterations_stop():
    det, t, _ = _assert_end_to_end(K.rank_edge(K.TILE + 1, 5, max_iterations=5), ("rank", K.TILE + 1, 5, "mi5"))
    assert t["iterations"] == 6 and t["winner_rank"] == 5 and t["chunks_launched"] == 1 and t["hypotheses_scored"] == 6


def test_draw_list_runs_of_bad_samples():
    det, t, _ = _assert_end_to_end(K.bad_run(999), ("bad_run", 999))
    assert t["ransac_failed"] == 0 and t["iterations"] == 41 and t["draws"] == 30 + 999 + 11
    det, t, _ = _assert_end_to_end(K.bad_run(1000), ("bad_run", 1000))
    assert t["ransac_failed"] == 1 and t["iterations"] == 30 and t["winner_rank"] == 3 and det.status == "DETECTED"
    det, t, _ = _assert_end_to_end(K.run_behind_the_stop(), "behind")
    assert t["ransac_failed"] == 0 and t["draws"] <= 5 and det.status == "DETECTED"


# ---- thresholds ------------------------------------------------------------------------------------------------------------------
def test_point_and_inlier_thresholds():
    n = K.TILE + 1
    c = K.rank_edge(n, K.CHUNK_FIRST - 1)
    m1 = c["m"] + 1
    for thresh, want in ((m1, "DETECTED"), (m1 + 1, "TOO_FEW_INLIERS"), (n, "TOO_FEW_INLIERS"), (n + 1, "TOO_FEW_POINTS")):
        det, t, _ = _assert_end_to_end(c, None, floor_pts_thresh=thresh)
        assert det.status == want
        assert (t["iterations"] == 0) == (want == "TOO_FEW_POINTS")


def test_verticality_threshold_and_downward_normal():
    for ang, want in ((9.9, "DETECTED"), (10.1, "NOT_VERTICAL")):
        det, t, _ = _assert_end_to_end(K.tilted_plane(ang), ("tilted", ang, False))
        assert det.status == want
    det, co = _run(K.tilted_plane(9.9, flip=True))
    _assert_ransac_equal(det, co, K.reference(("tilted", 9.9, True), K.tilted_plane(9.9, flip=True)))
    assert det.trace()["raw_coeffs"][2] < 0 and co[2] > 0 and np.array_equal(co, -det.trace()["raw_coeffs"])


# ---- host ------------------------------------------------------------------------------------------------------------------------
def test_tiny_clouds_and_bad_arguments():
    from delta_graph_slam_amd import _lib as L
    pts = R.floor_scene(3, 0, seed=1)
    for n in (0, 1, 2, 3):
        for thresh in (0, 512):
            c = K.case(pts[:n], dict(use_normal_filtering=0, floor_pts_thresh=thresh))
            det, t, ref = _assert_end_to_end(c, None, floor_pts_thresh=thresh)
            assert det.status == ref["status"] and det.filtered().shape == (n, 4)
    c = K.case(pts, dict(use_normal_filtering=1, floor_pts_thresh=0))      # three points through the normal pass
    _assert_end_to_end(c, None, floor_pts_thresh=0)
    with pytest.raises(L.DgsError) as ei:
        _run(K.case(pts, dict(floor_pts_thresh=-1)))
    assert ei.value.status == 1
    short = K.planted(0.0, False)
    short["raw"] = np.zeros(2, np.uint32)
    det, co = _run(short)
    assert det.status == "RNG_EXHAUSTED" and co is None


def test_device_input_and_handle_reuse_give_the_same_bits():
    import torch
    big, small = K.planted(5.0, True), K.rank_edge(K.TILE - 1, K.CHUNK_FIRST)
    fresh = {}
    for name, c in (("big", big), ("small", small)):
        det, co = _run(c)
        fresh[name] = (det.status, co, det.filtered(), det.inliers()[0], det.trace())
    det_d, co_d = _run(big, cloud=torch.from_numpy(big["cloud"]).cuda())
    assert np.array_equal(_bits(co_d), _bits(fresh["big"][1])) and np.array_equal(_bits(det_d.filtered()), _bits(fresh["big"][2]))
    from delta_graph_slam_amd.registration import Registration
    reg = Registration("NDT_OMP")
    for name, c in (("big", big), ("small", small), ("big", big)):
        det, co = _run(c, det=_detector(c["params"], registration=reg))
        st, co0, f0, i0, t0 = fresh[name]
        assert det.status == st and np.array_equal(_bits(co), _bits(co0)) and np.array_equal(_bits(det.filtered()), _bits(f0))
        assert np.array_equal(det.inliers()[0], i0)
        assert {k: det.trace()[k] for k in TRACE_KEYS} == {k: t0[k] for k in TRACE_KEYS}


def test_prefilter_line_extraction_and_align_interleaved_on_one_handle():
    from delta_graph_slam_amd import synth
    from delta_graph_slam_amd.line_extraction import LineExtractor
    from delta_graph_slam_amd.prefilter import Prefilter
    from delta_graph_slam_amd.registration import Registration
    scan = K.raw_scan("vlp16")
    tgt, src, _ = synth.planar_pair(n=8192)
    le_params = {"max_iterations": 100, "max_rounds": 4}
    c = K.planted(5.0, True)

    def lines_of(ls):
        return [(l.pointA.tolist(), l.pointB.tolist(), l.mean_error, l.std_sigma, l.max_error, l.min_error) for l in ls]

    # every piece on a handle of its own
    f3, f2 = Prefilter().cloud_callback(scan)
    lines = lines_of(LineExtractor(le_params).extract(f2))
    ref = Registration("NDT_OMP", ndt_resolution=1.0)
    ref.setInputTarget(tgt)
    ref.setInputSource(src)
    ref.align()
    det0, co0 = _run(c)
    want = (det0.status, _bits(co0).tolist(), _bits(det0.filtered()).tolist(), det0.inliers()[0].tolist())

    def detect_again(det):
        co = det.detect(c["cloud"], c["raw"], c["tilt"], c["tilt_inv"])
        assert (det.status, _bits(co).tolist(), _bits(det.filtered()).tolist(), det.inliers()[0].tolist()) == want

    # all of them on one handle, a detect between every two steps
    r = Registration("NDT_OMP", ndt_resolution=1.0)
    det = _detector(c["params"], registration=r)
    r.setInputTarget(tgt)
    r.setInputSource(src)
    detect_again(det)
    g3, g2 = Prefilter(registration=r).cloud_callback(scan)
    detect_again(det)
    assert np.array_equal(_bits(g3), _bits(f3)) and np.array_equal(_bits(g2), _bits(f2))
    assert lines_of(LineExtractor(le_params, registration=r).extract(g2)) == lines
    detect_again(det)
    r.align()
    assert np.array_equal(r.getFinalTransformation(), ref.getFinalTransformation())
    detect_again(det)
