"""CPU proof of what tests/prefilter_edge_cases.py claims and of every condition that concerns the numpy restatement alone
(tests/prefilter_reference.py): the mask cases compact to cloud[mask], the threshold searches found their points, the exact-tie
lattices sit on r * r and make radius_inclusive observable, the k-NN of the restatement is safe under ties, the eigen33 branches the
new normal inputs reach, the normal band cap, and the legitimacy of every statistical case."""
import numpy as np
import pytest

import prefilter_edge_cases as E
import prefilter_reference as R
from delta_graph_slam_amd import synth

F = np.float32


@pytest.fixture(scope="module")
def down(oracle_lib):
    xyz, _ = synth.street_scan((0.0, 0.0, 0.0), 64, (2.0, -24.8), 4096, 3)
    return oracle_lib.voxel_grid(R.distance_filter(synth._xyz1(xyz)), 0.1)


# ---------------------------------------------------------------------------------------------------- compaction masks
def test_mask_sizes_straddle_the_wave_the_workgroup_and_the_scan_chunk():
    assert E.EDGE == 262144 and 1023 * 256 + 255 == E.EDGE - 1
    for edge in (E.WAVE, E.BLOCK):
        assert {edge - 1, edge, edge + 1} <= set(E.SMALL_SIZES)
    assert {E.EDGE - 1, E.EDGE, E.EDGE + 1, E.EDGE + 257, 2 * E.EDGE + 1} <= set(E.LARGE_SIZES) and max(E.LARGE_SIZES) > 3 * E.EDGE
    ids = E.mask_case_ids()
    assert len(ids) == len(set(ids))
    for n in E.LARGE_SIZES:
        assert {m for k, m in ids if k == n} == set(E.MASKS)
    for n in E.SMALL_SIZES + E.LARGE_SIZES:
        assert {"all", "none", "random_50"} <= {m for k, m in ids if k == n}


@pytest.mark.parametrize("n", E.SMALL_SIZES + E.LARGE_SIZES)
def test_mask_cases_compact_to_the_masked_cloud(n):
    for k, name in E.mask_case_ids():
        if k != n:
            continue
        c, mask = E.mask_case(n, name)
        want = c[mask]
        assert c.shape == (n, 4) and np.array_equal(c[:, 3], np.arange(n))            # the index is exact in the pad lane
        assert np.array_equal(R.distance_filter(c), want), (n, name)
        assert np.all(np.diff(want[:, 3]) > 0), (n, name)                             # w strictly increasing: order is observable
        assert np.array_equal(want[:, 3].astype(np.int64), np.nonzero(mask)[0])
        assert E.first_difference(want, want) == "equal"
        if want.shape[0] > 1:
            swapped = want.copy()
            swapped[[0, -1]] = swapped[[-1, 0]]
            assert "index 0" in E.first_difference(swapped, want)


def test_masks_do_what_their_names_say():
    n = 3 * E.EDGE + 321
    m = {k: f(n) for k, f in E.MASKS.items()}
    assert m["all"].all() and not m["none"].any()
    assert np.nonzero(m["first"])[0].tolist() == [0] and np.nonzero(m["last"])[0].tolist() == [n - 1]
    assert np.all(np.nonzero(m["last_lane_of_every_wave"])[0] % 64 == 63) and m["last_lane_of_every_wave"].sum() == n // 64
    assert np.all(np.nonzero(m["first_lane_of_every_workgroup"])[0] % 256 == 0) and m["first_lane_of_every_workgroup"].sum() == n // 256 + 1
    for k, d in (("random_1", 0.01), ("random_50", 0.5), ("random_99", 0.99)):
        assert abs(m[k].mean() - d) < 0.005
    blocks = lambda mask: np.unique(np.nonzero(mask)[0] // 256)
    assert blocks(m["workgroups_1023_1024"]).tolist() == [1023, 1024] and m["workgroups_1023_1024"].sum() == 512
    assert blocks(m["chunk0_empty_chunk1_full"]).tolist() == list(range(1024, 2048)) and m["chunk0_empty_chunk1_full"].sum() == E.EDGE
    assert blocks(m["chunk0_full_chunk1_empty"]).tolist() == list(range(1024)) and m["chunk0_full_chunk1_empty"].sum() == E.EDGE
    assert np.array_equal(E.index_lane((1 << 24) + 2).view(np.uint32)[-2:], [1 << 24, (1 << 24) + 1])   # beyond 2^24: the bit pattern


# ---------------------------------------------------------------------------------------------------- predicate thresholds
@pytest.mark.parametrize("near,far", E.THRESHOLD_PAIRS)
def test_threshold_searches_found_their_points(near, far):
    c, found = E.threshold_cloud(near, far)
    for t, f in found.items():
        print(f"near {near} far {far}: threshold {t}: {f}")
        assert f["exact"] >= E.MIN_FOUND and f["parts"] >= E.MIN_FOUND and f["flips"] >= E.MIN_FOUND
        assert f["below"] + f["above"] >= E.MIN_FOUND      # just above a power of two the float is two steps of the search away
    assert set(found) == {t for t in (near, far) if 0 < t < 1e19}
    d = E.f32_norm(c[:, :3]).astype(np.float64)
    for t in found:
        ft = F(t)
        for v in (ft, np.nextafter(ft, F(-np.inf)), np.nextafter(ft, F(np.inf))):
            assert np.count_nonzero(d == float(v)) >= 6     # the axis points at least
    out = R.distance_filter(c, near, far)
    # NaN in w only: kept, and the payload survives
    assert np.array_equal(out[-len(E.NAN_PAYLOADS):, 3].view(np.uint32), np.asarray(E.NAN_PAYLOADS, np.uint32))
    assert np.all(np.isfinite(out[:, :3]))
    xyz = c[:, :3]
    big = np.any(np.abs(xyz) == F(2e19), 1)
    assert big.sum() == 6 and not np.isin(c[big, 3], out[:, 3]).any()                   # the square overflows: dropped even at far = 3.4e38
    sub = np.any((np.abs(xyz) > 0) & (np.abs(xyz) < R.FLT_MIN), 1)
    assert sub.sum() == 6 and not np.isin(c[sub, 3], out[:, 3]).any()                   # the square of a subnormal is 0: d = 0, not > near
    tiny = np.any(xyz == F(1e-20), 1)
    assert tiny.sum() == 3 and np.isin(c[tiny, 3], out[:, 3]).all() == (near == 0.0)    # subnormal square, d = 1e-20 > 0
    zero = ~np.any(xyz != 0, 1)
    assert zero.sum() == 3 and np.signbit(xyz[zero]).any() and not np.isin(c[zero, 3], out[:, 3]).any()
    assert (np.any(xyz == F(1.8e19), 1) & np.isin(c[:, 3], out[:, 3])).sum() == (3 if far > 1e30 else 0)


def test_threshold_flips_change_the_decision():
    """At the `flips` points a fused or double sum of squares gives the other answer: a kernel that contracts the sum fails there."""
    tp = E.threshold_points(1.0)
    d = E.f32_norm(tp["flips"])
    fused, dbl = E.other_norms(tp["flips"])
    assert np.all(((d > 1) != (fused > 1)) | ((d > 1) != (dbl > 1)) | ((d < 1) != (fused < 1)) | ((d < 1) != (dbl < 1)))
    # and at 0.1 the float and the double threshold part: d == float32(0.1) is > 0.1
    c, _ = E.threshold_cloud(0.1, 100.0)
    on = c[E.f32_norm(c[:, :3]) == F(0.1)]
    assert on.shape[0] >= E.MIN_FOUND and np.isin(on[:, 3], R.distance_filter(c, 0.1, 100.0)[:, 3]).all()


@pytest.mark.parametrize("lz", E.HEIGHT_LIDAR_Z)
def test_height_cloud_shows_the_height_decision_in_the_2d_output(lz):
    vals = E.height_test_values(lz)
    z = F(lz)
    assert {float(np.nextafter(z, F(-np.inf))), float(z), float(np.nextafter(z, F(np.inf)))} <= set(vals.tolist())
    assert vals.min() < lz < vals.max() or lz == 0                                # floats on both sides of the double value
    assert np.signbit(vals).any() and np.any((vals == 0) & ~np.signbit(vals))     # +0 and -0
    c = E.height_cloud(lz)
    f3, f2, info = R.cloud_callback(c, E.HEIGHT_PARAMS, (0.0, 0.0, lz), None)
    h = info["height"]
    assert np.array_equal(f3, c)                                                  # the distance filter keeps the wall
    assert np.array_equal(h, c[c[:, 2].astype(np.float64) > lz]) and 0 < c.shape[0] - h.shape[0] < c.shape[0] // 5 + 1
    assert int(info["normal_band"].sum()) == 0
    assert np.array_equal(f2, R.flatten(h))                                       # the normal filter keeps every point: f2 shows h
    if lz == 0:
        sub = c[(c[:, 2] > 0) & (c[:, 2] < R.FLT_MIN)]
        assert sub.shape[0] and np.isin(sub[:, 3], h[:, 3]).all()                 # a subnormal z is above 0


# ---------------------------------------------------------------------------------------------------- k-NN under ties
def test_brute_force_knn_equals_the_tree_path_on_a_tie_free_cloud():
    c = E.blob(3000, seed=7)
    for k in (1, 3, 10, 32):
        ib, db, tb = R.knn(c, k, brute=True)
        it, dt, tt = R.knn(c, k, brute=False)
        assert not tb.any() and not tt.any()
        assert np.array_equal(ib, it) and np.array_equal(db, dt)


def test_knn_is_exact_under_ties_on_both_paths():
    c = E.duplicates(distinct=50, fold=20)                      # 1,000 points, tie groups of 20
    p = c[:, :3]
    full = np.array([(np.square(p[i] - p, dtype=F)[:, 0] + np.square(p[i] - p, dtype=F)[:, 1]) + np.square(p[i] - p, dtype=F)[:, 2] for i in range(p.shape[0])])
    for k in (10, 21, 32):
        want = np.array([np.lexsort((np.arange(p.shape[0]), full[i]))[:k] for i in range(p.shape[0])])
        for brute in (True, False):
            idx, dd, tie = R.knn(c, k, brute=brute)
            assert np.array_equal(idx, want), (k, brute)
            assert np.array_equal(dd, np.take_along_axis(full, want, 1))
    idx, dd, tie = R.knn(c, 10)
    assert tie.all() and np.all(dd == 0) and np.all(idx[:, 0] == np.arange(1000) % 50)    # the ten lowest indices of the 20 copies
    # fewer points than k: the rest of the list is empty
    idx, dd, tie = R.knn(c[:3], 5)
    assert np.all(idx[:, 3:] == -1) and np.all(np.isinf(dd[:, 3:])) and not tie.any()


def test_exact_tie_lattices_sit_on_the_radius_and_make_the_switch_observable():
    assert E.exact_radius(0.5, 1) == 0.5 and E.exact_radius(0.25, 1) == 0.25
    r = np.sqrt(0.125)
    assert E.R_DIAG is None and all(v * v != 0.125 for v in (r, np.nextafter(r, 0), np.nextafter(r, 1)))   # why that lattice is dropped
    assert {name for name, _, _ in E.EXACT_TIE_RADIUS} == {"lattice_half", "lattice_plane"}
    for name, radius, min_nb in E.EXACT_TIE_RADIUS:
        assert (radius, min_nb) in E.TIE_CLOUDS[name][1]
        c = E.tie_cloud(name)
        _, dd, _ = R.knn(c, min_nb + 1)
        on = int(np.count_nonzero(dd[:, min_nb].astype(np.float64) == radius * radius))
        assert 4 * on >= c.shape[0], (name, on)
        inc, _ = R.radius_outlier_removal(c, radius, min_nb, True)
        exc, _ = R.radius_outlier_removal(c, radius, min_nb, False)
        assert inc.shape[0] - exc.shape[0] == on and on > 0
        print(f"{name} r {radius} min_neighbors {min_nb}: d_k^2 == r*r at {on} of {c.shape[0]}, kept {inc.shape[0]} inclusive, {exc.shape[0]} strict")


def test_tie_clouds_are_small_exact_and_tied(down):
    ties = {}
    for name in E.TIE_CLOUDS:
        c = E.tie_cloud(name, down)
        assert 0 < c.shape[0] <= R.KNN_BRUTE_MAX and np.array_equal(c[:, 3], np.arange(c.shape[0]))
        assert np.all(E.f32_norm(c[:, :3]) > 1.0) and np.all(E.f32_norm(c[:, :3]) < 100.0)
        ties[name] = int(R.knn(c, R.NORMAL_K)[2].sum())
    print("k-th distance ties at k = 10:", ties)
    assert ties["lattice_plane"] == 6400 and ties["lattice_half"] == 4096 and ties["duplicates"] == 4000
    assert ties["cubic_lattice"] > 3000 and ties["line"] > 200 and ties["quantised_crop"] > 0
    q = E.tie_cloud("quantised_crop", down)[:, :3].astype(np.float64) / 0.002
    assert np.abs(q - np.round(q)).max() < 1e-3                                  # on the 2 mm grid up to float32 rounding
    d = E.duplicates()
    assert np.unique(d[:, :3], axis=0).shape[0] == 200 and np.array_equal(d[:200, :3], d[200:400, :3])


# ---------------------------------------------------------------------------------------------------- normal inputs
def test_eigen33_census_and_band_cap_of_the_new_normal_inputs(down):
    total = {}
    inputs = [(name, E.tie_cloud(name, down)) for name in E.TIE_CLOUDS] + [(f"blob{n}", E.blob(n)) for n in E.NORMAL_LENGTHS]
    for name, c in inputs:
        census = {}
        nv, cov, keep, band, tie = R.normals(c, census=census)
        counts = {k: int(v.sum()) for k, v in census.items()}
        counts["nan"] = int(np.isnan(nv).any(1).sum())
        print(f"{name}: n {c.shape[0]}, band {int(band.sum())}, ties {int(tie.sum())}, {counts}")
        assert int(band.sum()) <= max(5, c.shape[0] // 1000)                      # the existing cap of the chain test
        if c.shape[0] >= 3:
            assert counts["pick1"] + counts["pick2"] + counts["pick3"] == c.shape[0]
        for k, v in counts.items():
            total[k] = total.get(k, 0) + v
        if name in ("duplicates", "line"):
            assert counts["nan"] == c.shape[0]                                    # zero covariance / zero cross products: NaN normals
        if name == "duplicates":
            assert counts["scale_tiny"] == c.shape[0]                             # the branch scale <= FLT_MIN
    for branch in ("scale_tiny", "c0_small", "pick1", "pick2", "pick3", "nan"):
        assert total[branch] > 0, branch
    # blobs of one and two points: NaN normals and NaN covariances (fewer than 3 neighbours)
    for n in (1, 2):
        nv, cov, keep, _, _ = R.normals(E.blob(n))
        assert np.isnan(nv).all() and np.isnan(cov).all() and not keep.any()


# ---------------------------------------------------------------------------------------------------- statistical cases
def _legit(st):
    """The existing condition of the statistical test, on the reference alone: no point within 1e-9 relative of the threshold, and the
    variance not within 1e-9 (of the squared mean) of zero."""
    return int(np.count_nonzero(st["near"])) == 0 and st["stddev"] ** 2 > 1e-9 * st["mean"] ** 2


def test_every_statistical_case_is_legitimate_and_the_sqrt_switch_is_observable(down):
    seen = 0
    for name, (_, _, stat) in E.TIE_CLOUDS.items():
        for mean_k, mul in stat or []:
            c = E.tie_cloud(name, down)
            o1, s1 = R.statistical_outlier_removal(c, mean_k, mul, True)
            o0, s0 = R.statistical_outlier_removal(c, mean_k, mul, False)
            assert _legit(s1) and _legit(s0), (name, mean_k)
            differ = int(np.count_nonzero(s1["distances"] != s0["distances"]))
            assert differ > 0, (name, mean_k)                                     # sqrt in float or in double: different mean distances
            print(f"{name} mean_k {mean_k}: kept {o1.shape[0]} / {o0.shape[0]} of {c.shape[0]}, mean distances that differ {differ}")
            seen += 1
    assert seen >= 5
    for mean_k, n in E.STATISTICAL_LENGTHS:
        assert n > mean_k
        for sf in (True, False):
            _, st = R.statistical_outlier_removal(E.blob(n), mean_k, 1.0, sf)
            assert _legit(st), (mean_k, n, sf)
    assert {k for k, _ in E.STATISTICAL_LENGTHS} == {1, 2, 31} and {(1, 2), (2, 3), (31, 32), (1, 33), (2, 33), (31, 33), (1, 257), (2, 257), (31, 257)} <= set(E.STATISTICAL_LENGTHS)
    # the ring is left out for the reason the generator gives: a lattice in one dimension, the variance is rounding-sized
    _, st = R.statistical_outlier_removal(E.ring(), 5, 1.0)
    assert not _legit(st)


def test_radius_length_cases_and_the_switch_at_radius_zero():
    assert {k for k, _ in E.RADIUS_LENGTHS} == {0, 1, 31}
    for min_nb, n in E.RADIUS_LENGTHS:
        c = E.blob(n)
        inc, _ = R.radius_outlier_removal(c, 0.0, min_nb, True)
        exc, _ = R.radius_outlier_removal(c, 0.0, min_nb, False)
        assert exc.shape[0] == 0
        assert inc.shape[0] == (n if min_nb == 0 else 0)          # k = 1: the query itself at d^2 = 0 == r * r
        if n < min_nb + 1:
            assert R.radius_outlier_removal(c, 1.5, min_nb)[0].shape[0] == 0


# ---------------------------------------------------------------------------------------------------- voxel index overflow
def test_overflow_box_overflows_the_dense_voxel_index_inside_the_far_threshold(oracle_lib):
    b = E.overflow_box()
    assert np.array_equal(R.distance_filter(b), b)                                # every point inside near / far of the defaults
    ext = b[:, :3].max(0) - b[:, :3].min(0)
    assert np.array_equal(ext, [199.0, 199.0, 60.0])
    assert E.voxel_cells(b, 0.1) > np.iinfo(np.int32).max and b.shape[0] > 200
    assert E.voxel_cells(b[8:], 0.1) < np.iinfo(np.int32).max                     # without the spanning points the grid fits
    for ds in ("NONE", "APPROX_VOXELGRID"):
        f3, f2, info = R.cloud_callback(b, dict(downsample_method=ds), (0.0, 0.0, 0.0), oracle_lib)
        assert f3.shape[0] > 200 and info["statistical_near"] == 0 and int(info["normal_band"].sum()) <= 5
