"""-m gpu: the prefilter chain (delta_graph_slam_amd/csrc/prefilter.hip) at the edges of its kernels, against the numpy restatement
tests/prefilter_reference.py.  The inputs and the edge each one hits: tests/prefilter_edge_cases.py (proved on the CPU by
tests/test_prefilter_edge_cases_cpu.py).

  * compaction: every mask case through dgs_prefilter_distance, host arrays and device tensors, bit for bit and in order -- the cases
    above 262,144 points run the second and later chunks of pf_scan_kernel and its carry;
  * predicates: the distance thresholds (exact, one ulp either side, points where a fused or double sum of squares decides otherwise,
    overflow, subnormals, zeros, non-finite coordinates, NaN pad lanes) and the height threshold through the chain;
  * ties and switches: the radius, statistical and normal passes and the chain on clouds with equal distances, under both values of
    radius_inclusive and statistical_sqrt_float; the covariances of the normal pass bit-equal, which proves the tie order;
  * list lengths: k = 1, 2 and 32, clouds of k and k + 1 points, the normal pass below ten points;
  * history: one handle after a large cloud gives a small one the bits of a fresh handle;
  * output capacity and the voxel index overflow (DGS_ERR_GRID_TOO_LARGE, nothing published, the handle stays usable)."""
import ctypes as C

import numpy as np
import pytest

import prefilter_edge_cases as E
import prefilter_reference as R
from delta_graph_slam_amd import synth

pytestmark = pytest.mark.gpu
ORIGIN = (0.0, 0.0, 0.0)


def _pf(params=None):
    from delta_graph_slam_amd.prefilter import Prefilter
    return Prefilter(params)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(got, want):
    """Bit for bit, NaN payloads and signed zeros included."""
    return got.shape == want.shape and np.array_equal(_bits(got), _bits(want))


@pytest.fixture(scope="module")
def hdl64():
    xyz, _ = synth.street_scan((0.0, 0.0, 0.0), 64, (2.0, -24.8), 4096, 3)
    return synth._xyz1(xyz)


@pytest.fixture(scope="module")
def vlp16():
    xyz, _ = synth.street_scan((-30.0, 1.0, 0.1), 16, (15.0, -15.0), 1875, 21)
    return synth._xyz1(xyz)


@pytest.fixture(scope="module")
def down(hdl64, oracle_lib):
    return oracle_lib.voxel_grid(R.distance_filter(hdl64), 0.1)


@pytest.fixture(scope="module")
def pf_default():
    return _pf()


# ---------------------------------------------------------------------------------------------------- compaction
@pytest.mark.parametrize("n,mask_name", E.mask_case_ids())
def test_compaction_of_a_mask_case(pf_default, n, mask_name):
    c, mask = E.mask_case(n, mask_name)
    out = pf_default.distance_filter(c)
    want = c[mask]
    assert np.array_equal(out, want), f"n {n}, mask {mask_name}: {E.first_difference(out, want)}"


def test_compaction_of_every_mask_case_through_device_tensors(pf_default):
    import torch
    for n, mask_name in E.mask_case_ids():
        c, mask = E.mask_case(n, mask_name)
        out = pf_default.distance_filter(torch.from_numpy(c).cuda())
        assert out.is_cuda
        out, want = out.cpu().numpy(), c[mask]
        assert np.array_equal(out, want), f"n {n}, mask {mask_name}, device tensors: {E.first_difference(out, want)}"


# ---------------------------------------------------------------------------------------------------- predicates
@pytest.mark.parametrize("near,far", E.THRESHOLD_PAIRS)
def test_distance_predicate_at_its_thresholds(near, far):
    import torch
    c, found = E.threshold_cloud(near, far)
    pf = _pf({"distance_near_thresh": near, "distance_far_thresh": far})
    want = R.distance_filter(c, near, far)
    out = pf.distance_filter(c)
    assert _same(out, want), f"near {near} far {far}: {E.first_difference(out, want)}"
    dev = pf.distance_filter(torch.from_numpy(c).cuda()).cpu().numpy()
    assert _same(dev, want), f"near {near} far {far}, device tensors: {E.first_difference(dev, want)}"
    print(f"near {near} far {far}: {c.shape[0]} points, kept {out.shape[0]}, searches {found}")


@pytest.mark.parametrize("near,far", E.THRESHOLD_PAIRS[:2])
@pytest.mark.parametrize("lz", E.HEIGHT_LIDAR_Z)
def test_height_predicate_at_its_threshold(lz, near, far):
    c = E.height_cloud(lz)
    params = dict(E.HEIGHT_PARAMS, distance_near_thresh=near, distance_far_thresh=far)
    lidar = (0.0, 0.0, lz)
    pf = _pf(params)
    f3, f2 = pf.cloud_callback(c, lidar)
    r3, r2, info = R.cloud_callback(c, params, lidar, None)
    h = info["height"]
    assert _same(f3, r3)
    nv, _ = pf.normals()
    assert nv.shape[0] == h.shape[0], f"lidar z {lz!r}: the height filter kept {nv.shape[0]} points for {h.shape[0]}"
    assert int(info["normal_band"].sum()) == 0
    assert _same(f2, R.flatten(h)), f"lidar z {lz!r}: {E.first_difference(f2, R.flatten(h))}"    # the w lane names the points that passed


# ---------------------------------------------------------------------------------------------------- ties and switches
def _check_radius(c, radius, min_nb, what):
    ties = None
    for inclusive in E.SWITCHES:
        pf = _pf({"radius_radius": radius, "radius_min_neighbors": min_nb, "radius_inclusive": bool(inclusive)})
        out = pf.radius_outlier_removal(c)
        ref, tie = R.radius_outlier_removal(c, radius, min_nb, bool(inclusive))
        assert _same(out, ref), f"{what} r {radius} min_neighbors {min_nb} inclusive {inclusive}: {E.first_difference(out, ref)}"
        ties = (int(tie.sum()), out.shape[0]) if ties is None else ties + (out.shape[0],)
    return ties


def _check_statistical(c, mean_k, mul, what):
    for sqrt_float in E.SWITCHES:
        pf = _pf({"statistical_mean_k": mean_k, "statistical_stddev": mul, "statistical_sqrt_float": bool(sqrt_float)})
        out = pf.statistical_outlier_removal(c)
        ref, st = R.statistical_outlier_removal(c, mean_k, mul, bool(sqrt_float))
        dist, s = pf.statistics()
        assert s["n"] == c.shape[0]
        assert np.array_equal(dist, st["distances"]), (what, mean_k, sqrt_float)            # per-point mean distances bit-equal
        assert abs(s["threshold"] - st["threshold"]) <= 1e-12 * abs(st["threshold"]), (what, mean_k, sqrt_float)
        assert int(np.count_nonzero(st["near"])) == 0
        assert _same(out, ref), f"{what} mean_k {mean_k} sqrt_float {sqrt_float}: {E.first_difference(out, ref)}"


def _check_normals(pf, h, lidar, what):
    """The hooks of the last normal pass against the restatement on its input h -> (device keep mask, band count)."""
    nv, cov = pf.normals()
    assert nv.shape[0] == h.shape[0], what
    if h.shape[0] == 0:
        return np.zeros(0, bool), 0
    with np.errstate(invalid="ignore", divide="ignore"):
        rn, rcov, keep, band, tie = R.normals(h, lidar)
        assert np.array_equal(cov.view(np.uint32), rcov.view(np.uint32)), f"{what}: covariances differ (the neighbour sets or their order)"
        assert np.array_equal(np.isnan(nv[:, :3]), np.isnan(rn)), what
        ok = ~np.isnan(rn).any(1)
        assert ok.sum() == 0 or np.max(np.abs(np.abs(nv[ok, :3]) - np.abs(rn[ok]))) <= 1e-5, what
        keep_gpu = np.abs(nv[:, 2]) < np.float32(0.2)
    assert not np.any((keep_gpu != keep) & ~band), what
    assert int(band.sum()) <= max(5, h.shape[0] // 1000)
    return keep_gpu, int(band.sum())


def _check_chain(c, params, lidar, orc, what):
    pf = _pf(params)
    f3, f2 = pf.cloud_callback(c, lidar)
    r3, r2, info = R.cloud_callback(c, params, lidar, orc)
    assert _same(f3, r3), f"{what}: /filtered_points: {E.first_difference(f3, r3)}"
    h = info["height"]
    keep_gpu, band = _check_normals(pf, h, lidar, what)
    assert _same(f2, R.flatten(h[keep_gpu])), f"{what}: /flat_filtered_points"
    return f3.shape[0], f2.shape[0], band, info


@pytest.mark.parametrize("name", list(E.TIE_CLOUDS))
def test_radius_filter_on_a_tie_cloud_under_both_switch_values(down, name):
    c = E.tie_cloud(name, down)
    for radius, min_nb in E.TIE_CLOUDS[name][1]:
        ties, kept_inc, kept_exc = _check_radius(c, radius, min_nb, name)
        print(f"{name} r {radius} / {min_nb}: k-th distance ties {ties} of {c.shape[0]}, kept {kept_inc} inclusive / {kept_exc} strict")
        if (name, radius, min_nb) in E.EXACT_TIE_RADIUS:
            assert kept_inc > kept_exc


@pytest.mark.parametrize("name", [k for k, v in E.TIE_CLOUDS.items() if v[2]])
def test_statistical_filter_on_a_tie_cloud_under_both_switch_values(down, name):
    c = E.tie_cloud(name, down)
    for mean_k, mul in E.TIE_CLOUDS[name][2]:
        _check_statistical(c, mean_k, mul, name)


@pytest.mark.parametrize("name", list(E.TIE_CLOUDS))
def test_normal_pass_on_a_tie_cloud(down, name):
    c = E.tie_cloud(name, down)
    pf = _pf()
    out = pf.normal_filtering(c)
    keep_gpu, band = _check_normals(pf, c, ORIGIN, name)
    assert _same(out, c[keep_gpu])
    print(f"{name}: {c.shape[0]} points, kept {out.shape[0]}, band {band}")


@pytest.mark.parametrize("name", list(E.TIE_CLOUDS))
def test_chain_on_a_tie_cloud_under_both_switch_values(down, name):
    c = E.tie_cloud(name, down)
    for params in E.tie_chain_params(name):
        for sw in E.SWITCHES:
            p = dict(params, radius_inclusive=bool(sw), statistical_sqrt_float=bool(sw))
            n3, n2, band, info = _check_chain(c, p, ORIGIN, None, f"{name} {p['outlier_removal_method']} switches {sw}")
            print(f"{name} {p['outlier_removal_method']} switches {sw}: 3D {n3}, 2D {n2}, band {band}, radius ties {info.get('radius_ties')}, "
                  f"statistical near {info.get('statistical_near')}")


# ---------------------------------------------------------------------------------------------------- list lengths
@pytest.mark.parametrize("mean_k,n", E.STATISTICAL_LENGTHS)
def test_statistical_lists_at_their_limits(mean_k, n):
    _check_statistical(E.blob(n), mean_k, 1.0, f"blob {n}")


@pytest.mark.parametrize("min_nb,n", E.RADIUS_LENGTHS)
def test_radius_lists_at_their_limits(min_nb, n):
    for radius in E.RADIUS_LENGTH_RADII:
        _check_radius(E.blob(n), radius, min_nb, f"blob {n}")


@pytest.mark.parametrize("n", E.NORMAL_LENGTHS)
def test_normal_pass_below_and_at_ten_points(n):
    c = E.blob(n)
    pf = _pf()
    out = pf.normal_filtering(c)
    keep_gpu, _ = _check_normals(pf, c, ORIGIN, f"blob {n}")
    assert _same(out, c[keep_gpu])
    if n < 3:
        nv, cov = pf.normals()
        assert np.isnan(nv).all() and np.isnan(cov).all() and out.shape[0] == 0


def test_lists_beyond_the_cap_are_invalid_arguments():
    from delta_graph_slam_amd import _lib as L
    c = E.blob(257)
    with pytest.raises(L.DgsError) as ei:
        _pf({"statistical_mean_k": 32}).statistical_outlier_removal(c)
    assert ei.value.status == 1
    with pytest.raises(L.DgsError) as ei:
        _pf({"radius_min_neighbors": 32}).radius_outlier_removal(c)
    assert ei.value.status == 1
    with pytest.raises(L.DgsError) as ei:
        _pf({"statistical_mean_k": 31}).statistical_outlier_removal(c[:31])     # n == mean_k: one point short of the smallest legal cloud
    assert ei.value.status == 1


# ---------------------------------------------------------------------------------------------------- history
def test_a_used_handle_gives_the_bits_of_a_fresh_one(hdl64, down):
    from delta_graph_slam_amd.prefilter import Prefilter, params_from_dict
    pf = _pf()
    big, mask = E.mask_case(max(E.LARGE_SIZES), "random_50")
    out = pf.distance_filter(big)
    assert np.array_equal(out, big[mask]), E.first_difference(out, big[mask])
    jobs = [("hdl64 defaults", hdl64, R.DEFAULTS), ("hdl64 launch", hdl64, R.LAUNCH)]
    for name in E.TIE_CLOUDS:
        jobs += [(name, E.tie_cloud(name, down), p) for p in E.tie_chain_params(name)]
    small = E.blob(65)
    small_params = dict(downsample_method="NONE", statistical_mean_k=20)
    jobs.append(("blob 65", small, small_params))
    for what, c, params in jobs:
        pf.params = params_from_dict(params)
        f3, f2 = pf.cloud_callback(c)
        g3, g2 = Prefilter(params).cloud_callback(c)
        assert _same(f3, g3), f"{what}: /filtered_points differ from a fresh handle's: {E.first_difference(f3, g3)}"
        assert _same(f2, g2), f"{what}: /flat_filtered_points differ from a fresh handle's: {E.first_difference(f2, g2)}"
    # the hooks report the small run, not what the large ones left in the buffers
    r3, r2, info = R.cloud_callback(small, small_params, ORIGIN, None)
    assert _same(f3, r3) and info["statistical_near"] == 0
    dist, s = pf.statistics()
    assert s["n"] == 65 and dist.shape == (65,)
    assert np.array_equal(dist, R.statistical_mean_distances(small, 20)[0])
    keep_gpu, _ = _check_normals(pf, info["height"], ORIGIN, "blob 65 after the large clouds")
    assert pf.normals()[0].shape[0] == info["height"].shape[0] == f3.shape[0]           # every point of the blob is above the sensor
    assert _same(f2, R.flatten(info["height"][keep_gpu]))
    # single stages after the chain: the same
    for stage in ("radius_outlier_removal", "statistical_outlier_removal", "normal_filtering", "distance_filter"):
        assert _same(getattr(pf, stage)(small), getattr(Prefilter(small_params), stage)(small)), stage


# ---------------------------------------------------------------------------------------------------- output capacity
def test_an_output_buffer_one_point_short_is_refused_and_the_handle_goes_on():
    pf = _pf()
    lib, h = pf._lib, pf._h
    c, mask = E.mask_case(257, "random_50")
    m = int(mask.sum())
    out = np.full((257, 4), -1.0, np.float32)
    n_out = C.c_int64(-1)
    src, dst = c.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)
    assert lib.dgs_prefilter_distance(h, src, 257, 0, 1.0, 100.0, dst, m - 1, 0, C.byref(n_out)) == 1      # DGS_ERR_INVALID_ARGUMENT
    assert n_out.value == m                                                                                 # the size the caller needs
    assert np.all(out == -1.0)                                                                              # nothing was written
    assert lib.dgs_prefilter_distance(h, src, 257, 0, 1.0, 100.0, dst, m, 0, C.byref(n_out)) == 0
    assert n_out.value == m and np.array_equal(out[:m], c[mask]) and np.all(out[m:] == -1.0)
    b = E.blob(257)
    ref, _ = R.radius_outlier_removal(b, 0.4, 2)
    assert 1 < ref.shape[0] < 257
    src = b.ctypes.data_as(C.c_void_p)
    assert lib.dgs_prefilter_radius(h, src, 257, 0, 0.4, 2, 1, dst, ref.shape[0] - 1, 0, C.byref(n_out)) == 1
    assert n_out.value == ref.shape[0]
    assert lib.dgs_prefilter_radius(h, src, 257, 0, 0.4, 2, 1, dst, ref.shape[0], 0, C.byref(n_out)) == 0
    assert n_out.value == ref.shape[0] and np.array_equal(out[:ref.shape[0]], ref)
    assert np.array_equal(pf.distance_filter(c), c[mask])


# ---------------------------------------------------------------------------------------------------- voxel index overflow
def test_voxel_index_overflow_is_reported_and_nothing_is_published(vlp16, oracle_lib):
    from delta_graph_slam_amd import _lib as L
    assert L.STATUS[5] == "DGS_ERR_GRID_TOO_LARGE"
    box = E.overflow_box()
    pf = _pf()                                                       # the nodelet's defaults: VOXELGRID 0.1, far 100
    with pytest.raises(L.DgsError) as ei:
        pf.cloud_callback(box)
    assert ei.value.status == 5
    n = box.shape[0]
    o3, o2 = np.full((n, 4), -1.0, np.float32), np.full((n, 4), -1.0, np.float32)
    m3, m2 = C.c_int64(-1), C.c_int64(-1)
    rc = pf._lib.dgs_prefilter(pf._h, C.byref(pf.params), box.ctypes.data_as(C.c_void_p), n, 0, (C.c_double * 3)(0.0, 0.0, 0.0),
                               o3.ctypes.data_as(C.c_void_p), n, o2.ctypes.data_as(C.c_void_p), n, 0, C.byref(m3), C.byref(m2))
    assert rc == 5 and m3.value == 0 and m2.value == 0               # both outputs empty
    assert np.all(o3 == -1.0) and np.all(o2 == -1.0)
    f3, f2 = pf.cloud_callback(vlp16)                                # the handle goes on
    g3, g2 = _pf().cloud_callback(vlp16)
    assert _same(f3, g3) and _same(f2, g2) and f3.shape[0] > 1000
    for ds in ("NONE", "APPROX_VOXELGRID"):
        n3, n2, band, info = _check_chain(box, dict(R.DEFAULTS, downsample_method=ds), ORIGIN, oracle_lib, f"overflow box {ds}")
        assert n3 > 200 and info["statistical_near"] == 0
        print(f"overflow box {ds}: 3D {n3}, 2D {n2}, band {band}")
