"""FloorDetectionNodelet::detect without a device: the numpy restatement (tests/floor_detection_reference.py) on its own, the library's
host pieces (draw list, walk) against it, and the conditions the GPU tests rely on, checked with the restatement alone."""
import math

import numpy as np
import pytest

import floor_detection_cases as K
import floor_detection_reference as R
import prefilter_reference as PR
from line_extraction_reference import MT19937

F = np.float32
K_MARGIN = 1e-6      # every walk decision `it < k` sits farther than this from a tie, so libm's last bit cannot decide a trace


def _margin_ok(res):
    return res["trace"] is None or res["trace"]["k_margin"] > K_MARGIN


# ---- the restatement ---------------------------------------------------------------------------------------------------------
def test_tilt_zero_is_the_exact_identity():
    from delta_graph_slam_amd.floor_detection import tilt_matrices
    for fn in (R.tilt_matrices, tilt_matrices):
        t, ti = fn(0.0)
        assert np.array_equal(t.view(np.uint32), np.eye(4, dtype=F).view(np.uint32))
        assert np.array_equal(ti.view(np.uint32), np.eye(4, dtype=F).view(np.uint32))
    a, b = R.tilt_matrices(5.0), tilt_matrices(5.0)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert abs(float(a[0][0, 2]) - math.sin(math.radians(5.0))) < 1e-7 and a[0][2, 0] == -a[0][0, 2]
    assert np.max(np.abs(a[0] @ a[1] - np.eye(4))) < 1e-6


def test_identity_transform_turns_minus_zero_into_plus_zero_and_sets_w():
    c = np.array([[-0.0, 1.0, -2.0, 7.0], [np.nan, 0.0, -2.0, 1.0], [1.0, np.inf, -2.0, 1.0]], F)
    for order in (0, 1):
        out = R.transform(c, np.eye(4, dtype=F), order)
        assert not np.signbit(out[0, 0]) and out[0, 3] == 1.0 and out[0, 1] == 1.0 and out[0, 2] == -2.0
        assert np.isnan(out[1, 0]) and np.isnan(out[2, 0]) and np.isinf(out[2, 1])
    # 0 * inf = NaN reaches every coordinate; the clip's 0 * x term then drops the point
    assert R.clip(R.transform(c, np.eye(4, dtype=F)), 2.0, 1.0).shape[0] == 1


def test_height_clip_band_is_half_open():
    z = np.array([-3.0, np.nextafter(F(-3.0), F(-4.0)), -1.0, np.nextafter(F(-1.0), F(-2.0)), -2.0, np.nan, np.inf, -np.inf], F)
    c = np.ones((z.size, 4), F)
    c[:, 2] = z
    out = R.clip(c, 2.0, 1.0)
    assert out[:, 2].tolist() == [-3.0, float(np.nextafter(F(-1.0), F(-2.0))), -2.0]


def test_draw_stream_matches_a_literal_transcription():
    n = 1000
    g = MT19937(12345)
    s = list(range(n))
    want = []
    for _ in range(50):
        for i in range(3):
            j = i + (g() >> 1) % (n - i)
            s[i], s[j] = s[j], s[i]
        want.append((s[0], s[1], s[2]))
    st = R.draw_stream(n)
    assert [next(st) for _ in range(50)] == want
    assert MT19937(5489)() == 3499211612                          # the standard's first output of the default seed


def test_raw_for_triples_round_trips():
    rng = np.random.default_rng(0)
    for n in (3, 4, 17, 1000):
        tr = [tuple(int(v) for v in rng.choice(n, 3, replace=False)) for _ in range(200)]
        raw = R.raw_for_triples(n, tr)
        st = R.draw_stream(n, raw)
        assert [next(st) for _ in tr] == tr
        with pytest.raises(R.StreamEnd):
            next(st)


def test_library_draw_list_and_walk_agree_with_the_restatement():
    from delta_graph_slam_amd.floor_detection import host_draws, host_walk
    for n in (3, 5, 1024, 30011):
        st = R.draw_stream(n)
        assert host_draws(n, 300).tolist() == [list(next(st)) for _ in range(300)]
    raw = np.random.default_rng(1).integers(0, 2**31, 3 * 400, dtype=np.uint32)
    st = R.draw_stream(777, raw)
    assert host_draws(777, 400, raw).tolist() == [list(next(st)) for _ in range(400)]
    rng = np.random.default_rng(2)
    for trial in range(200):
        n = int(rng.integers(50, 5000))
        hi = int(rng.integers(1, n + 1))
        counts = rng.integers(0, hi + 1, 1200)
        mi = int(rng.choice([0, 1, 5, 1000]))
        win, it, margin, _ = R.walk(counts, n, mi)
        if margin <= K_MARGIN:
            continue
        assert host_walk(counts, n, mi) == (win, it, False)
    assert host_walk([3, 4], 1000, 1000) == (1, 2, True)          # ran past the counts with the loop still open


def test_planted_planes_are_recovered_with_an_upward_normal():
    for tilt_deg, normal in ((0.0, False), (5.0, False), (5.0, True)):
        c = K.planted(tilt_deg, normal)
        r = K.reference(("planted", tilt_deg, normal), c)
        assert r["status"] == "DETECTED" and _margin_ok(r)
        co = r["coeffs"]
        assert co[2] > 0.99 and abs(float(np.linalg.norm(co[:3])) - 1.0) < 1e-6
        # the plane in the sensor frame: floor_scene's z = -2 + 0.03 x - 0.02 y seen through tilt_inv
        f = r["filtered"][r["inliers"]]
        assert np.max(np.abs(f[:, :3] @ co[:3] + co[3])) < 0.1
        assert r["inliers"].size >= 2300 and r["trace"]["iterations"] <= 12


def test_every_status():
    c = K.planted(0.0, False)
    assert K.reference(("planted", 0.0, False), c)["status"] == "DETECTED"
    assert R.detect(c["cloud"], dict(c["params"], floor_pts_thresh=3301))["status"] == "TOO_FEW_POINTS"
    assert R.detect(c["cloud"], dict(c["params"], floor_pts_thresh=3000))["status"] == "TOO_FEW_INLIERS"
    assert R.detect(np.zeros((0, 4), F))["status"] == "TOO_FEW_POINTS"
    assert R.detect(c["cloud"], c["params"], raw=np.zeros(2, np.uint32))["status"] == "RNG_EXHAUSTED"
    with pytest.raises(ValueError):
        R.detect(c["cloud"], dict(floor_pts_thresh=-1))
    for ang, want in ((9.9, "DETECTED"), (10.1, "NOT_VERTICAL")):
        t = K.tilted_plane(ang)
        r = K.reference(("tilted", ang, False), t)
        assert r["status"] == want and _margin_ok(r) and r["trace"]["winner_rank"] == 0
        assert abs(abs(float(r["trace"]["dot"])) - math.cos(math.radians(ang))) < 1e-5      # off the threshold by 2.6e-4: far more than float rounding
    dn = K.reference(("tilted", 9.9, True), K.tilted_plane(9.9, flip=True))
    assert dn["status"] == "DETECTED" and dn["trace"]["coeffs"][2] < 0 and np.array_equal(dn["coeffs"], -dn["trace"]["coeffs"])


def test_duplicate_point_quirk_is_not_vertical_with_every_point_an_inlier():
    c = K.quirk_cloud()
    r = K.reference("quirk", c)
    assert r["status"] == "NOT_VERTICAL" and r["trace"]["count"] == c["cloud"].shape[0] and r["trace"]["iterations"] == 1
    assert not np.any(r["trace"]["coeffs"][:3]) and r["trace"]["dot"] == 0


def test_thousand_bad_draws_break_the_walk_with_empty_inliers():
    c = K.diagonal_cloud()
    r = K.reference("diagonal", c)
    assert r["status"] == "TOO_FEW_INLIERS" and r["inliers"].size == 0
    assert r["trace"]["ransac_failed"] == 1 and r["trace"]["draws"] == 1000 and r["trace"]["iterations"] == 0 and r["trace"]["winner_rank"] == -1


# ---- conditions of the GPU tests ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["hdl64", "vlp16"])
def test_scan_band_holds_at_most_one_percent_of_the_clipped_points(kind, oracle_lib):
    f3, _, _ = PR.cloud_callback(K.raw_scan(kind), PR.DEFAULTS, (0.0, 0.0, 0.0), oracle_lib)
    for normal in (1, 0):
        c = K.case(f3, dict(K.SCAN_PARAMS, use_normal_filtering=normal))
        r = K.reference(("scan", kind, normal), c)
        assert r["status"] == "DETECTED" and _margin_ok(r)
        assert r["clipped"].shape[0] >= 5000 and abs(float(r["coeffs"][3]) - K.SENSOR_Z) < 0.05
        if normal:
            assert int(r["band"].sum()) <= r["clipped"].shape[0] // 100
            print(f"{kind}: 3-D {f3.shape[0]}, clipped {r['clipped'].shape[0]}, filtered {r['filtered'].shape[0]}, band {int(r['band'].sum())}, "
                  f"ties {int(r['tie'].sum())}, iterations {r['trace']['iterations']}")


def test_end_to_end_scene_has_an_empty_band():
    c = K.planted_empty_band()
    r = K.reference("empty_band", c)
    assert r["status"] == "DETECTED" and _margin_ok(r)
    assert int(r["band"].sum()) == 0 and int(r["tie"].sum()) == 0
    assert r["filtered"].shape[0] == 44 * 44                       # every floor point kept, every wall point dropped


@pytest.mark.parametrize("n", K.SIZES)
def test_rank_edge_scenes_are_what_the_gpu_tests_assume(n):
    for rank in (K.RANKS[0], K.RANKS[-1]):
        c = K.rank_edge(n, rank)
        r = K.reference(("rank", n, rank), c)
        t = r["trace"]
        assert _margin_ok(r) and r["filtered"].shape[0] == n
        assert t["winner_rank"] == rank and t["count"] == c["m"] + 1 and t["iterations"] == 1001 and t["draws"] == 1001
        assert r["inliers"][-1] == n - 1                            # the winner leads through the last index only
        a_count = int(R.inlier_mask(r["filtered"], R.plane_model(*[r["filtered"][i] for i in _triple(c, 3)]), 0.1).sum())
        assert a_count == c["m"]


def _triple(c, rank):
    st = R.draw_stream(c["cloud"].shape[0], c["raw"])
    return [next(st) for _ in range(rank + 1)][rank]


def test_draw_list_scenes_are_what_the_gpu_tests_assume():
    r = K.reference(("bad_run", 999), K.bad_run(999))
    assert _margin_ok(r) and r["trace"]["ransac_failed"] == 0 and r["trace"]["iterations"] == 41 and r["trace"]["draws"] == 30 + 999 + 11
    r = K.reference(("bad_run", 1000), K.bad_run(1000))
    assert _margin_ok(r) and r["trace"]["ransac_failed"] == 1 and r["trace"]["iterations"] == 30 and r["trace"]["draws"] == 30 + 1000
    assert r["trace"]["winner_rank"] == 3 and r["status"] == "DETECTED"      # the best model so far is kept
    r = K.reference("behind", K.run_behind_the_stop())
    assert _margin_ok(r) and r["trace"]["ransac_failed"] == 0 and r["trace"]["draws"] <= 5 and r["status"] == "DETECTED"


def test_short_walk_scene():
    r = K.reference(("rank", K.TILE + 1, 5, "mi5"), K.rank_edge(K.TILE + 1, 5, max_iterations=5))
    assert _margin_ok(r) and r["trace"]["iterations"] == 6 and r["trace"]["winner_rank"] == 5
