"""The prefilter chain (PrefilteringNodelet::cloud_callback, apps/prefiltering_nodelet.cpp:111-164) on the MI355X against the numpy
restatement tests/prefilter_reference.py: single stages, the hooks, the whole chain on raw HDL-64 / VLP-16 scans, the device path,
independence from a registration sharing the handle, and edge cases."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

import prefilter_reference as R
from delta_graph_slam_amd import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _hdl64(seed=3):
    xyz, _ = synth.street_scan((0.0, 0.0, 0.0), 64, (2.0, -24.8), 4096, seed)
    return synth._xyz1(xyz)


def _vlp16(seed=21):
    xyz, _ = synth.street_scan((-30.0, 1.0, 0.1), 16, (15.0, -15.0), 1875, seed)
    return synth._xyz1(xyz)


@pytest.fixture(scope="module")
def scans():
    return {"hdl64": _hdl64(), "vlp16": _vlp16()}


@pytest.fixture(scope="module")
def down(scans, oracle_lib):
    """Distance-filtered, voxel-grid down-sampled HDL-64 scan: the input of the outlier passes in the nodelet."""
    return oracle_lib.voxel_grid(R.distance_filter(scans["hdl64"]), 0.1)


def _pf(params=None):
    from delta_graph_slam_amd.prefilter import Prefilter
    return Prefilter(params)


def test_distance_filter_is_bit_equal_and_in_order(scans):
    c = scans["hdl64"].copy()
    c[5, 0] = np.nan
    c[6, 2] = np.inf
    c[7, 3] = -3.5          # the pad lane travels with the point
    pf = _pf()
    for near, far in ((1.0, 100.0), (0.1, 100.0), (5.0, 20.0)):
        pf.params.distance_near_thresh, pf.params.distance_far_thresh = near, far
        out = pf.distance_filter(c)
        assert np.array_equal(out, R.distance_filter(c, near, far))


@pytest.mark.parametrize("radius,min_nb", [(0.5, 2), (0.8, 2), (0.3, 5), (0.2, 31)])
def test_radius_filter_is_bit_equal_and_in_order(down, radius, min_nb):
    pf = _pf({"radius_radius": radius, "radius_min_neighbors": min_nb})
    out = pf.radius_outlier_removal(down)
    ref, tie = R.radius_outlier_removal(down, radius, min_nb)
    assert np.array_equal(out, ref)
    print(f"radius {radius} / {min_nb}: kept {out.shape[0]} of {down.shape[0]}, k-th distance ties {int(tie.sum())}")


@pytest.mark.parametrize("mean_k,mul", [(20, 1.0), (30, 1.2), (5, 0.5)])
def test_statistical_filter(down, mean_k, mul):
    pf = _pf({"statistical_mean_k": mean_k, "statistical_stddev": mul})
    out = pf.statistical_outlier_removal(down)
    ref, st = R.statistical_outlier_removal(down, mean_k, mul)
    dist, s = pf.statistics()
    assert s["n"] == down.shape[0]
    assert np.array_equal(dist, st["distances"])                                  # per-point mean distances bit-equal
    assert abs(s["threshold"] - st["threshold"]) <= 1e-12 * abs(st["threshold"])
    assert int(np.count_nonzero(st["near"])) == 0                                  # no point within 1e-9 of the threshold
    assert np.array_equal(out, ref)


def test_normal_pass(scans):
    h = R.height_filter(R.distance_filter(scans["hdl64"]))
    pf = _pf()
    out = pf.normal_filtering(h)
    nv, cov = pf.normals()
    rn, rcov, keep, band, _ = R.normals(h)
    assert nv.shape[0] == h.shape[0]
    assert np.array_equal(cov.view(np.uint32), rcov.view(np.uint32))             # the 9 floats bit for bit
    assert np.max(np.abs(np.abs(nv[:, :3]) - np.abs(rn))) <= 1e-5
    keep_gpu = np.abs(nv[:, 2]) < np.float32(0.2)
    assert not np.any((keep_gpu != keep) & ~band)
    assert np.array_equal(out, h[keep_gpu])
    print(f"normal pass: {h.shape[0]} points, band {int(band.sum())}, decisions that differ {int((keep_gpu != keep).sum())}")


CHAINS = [("defaults", R.DEFAULTS), ("launch", R.LAUNCH)]


@pytest.mark.parametrize("scan", ["hdl64", "vlp16"])
@pytest.mark.parametrize("pname,params", CHAINS)
@pytest.mark.parametrize("ds", ["VOXELGRID", "APPROX_VOXELGRID", "NONE"])
def test_full_chain(scans, oracle_lib, scan, pname, params, ds):
    params = dict(params, downsample_method=ds)
    c = scans[scan]
    lidar = (0.0, 0.0, 0.0)
    pf = _pf(params)
    f3, f2 = pf.cloud_callback(c, lidar)
    r3, r2, info = R.cloud_callback(c, params, lidar, oracle_lib)
    assert np.array_equal(f3, r3)                                                  # /filtered_points bit-equal, in order
    h = info["height"]
    nv, _ = pf.normals()
    assert nv.shape[0] == h.shape[0]
    keep_gpu = np.abs(nv[:, 2]) < np.float32(0.2)
    assert np.array_equal(f2, R.flatten(h[keep_gpu]))
    _, _, keep, band, _ = R.normals(h) if h.shape[0] else (None, None, np.zeros(0, bool), np.zeros(0, bool), None)
    assert not np.any((keep_gpu != keep) & ~band)                                  # /flat_filtered_points equal outside the band
    assert int(band.sum()) <= max(5, h.shape[0] // 1000)
    print(f"{scan} {pname} {ds}: 3D {f3.shape[0]}, 2D {f2.shape[0]}, normal band {int(band.sum())}, "
          f"statistical near {info.get('statistical_near')}, radius ties {info.get('radius_ties')}")


def test_device_tensors_give_the_host_result(scans):
    import torch
    pf = _pf()
    h3, h2 = pf.cloud_callback(scans["vlp16"], (0.0, 0.0, 0.1))
    d3, d2 = pf.cloud_callback(torch.from_numpy(scans["vlp16"]).cuda(), (0.0, 0.0, 0.1))
    assert d3.is_cuda and d2.is_cuda
    assert np.array_equal(d3.cpu().numpy(), h3) and np.array_equal(d2.cpu().numpy(), h2)
    dd = pf.distance_filter(torch.from_numpy(scans["vlp16"]).cuda())
    assert dd.is_cuda and np.array_equal(dd.cpu().numpy(), pf.distance_filter(scans["vlp16"]))


def test_registration_sharing_the_handle_is_untouched(scans):
    from delta_graph_slam_amd.prefilter import Prefilter
    from delta_graph_slam_amd.registration import Registration
    tgt, src, _ = synth.planar_pair(n=16384)
    ref = Registration("NDT_OMP", ndt_resolution=1.0)
    ref.setInputTarget(tgt)
    ref.setInputSource(src)
    ref.align()
    r = Registration("NDT_OMP", ndt_resolution=1.0)
    r.setInputTarget(tgt)
    before, vox_before = r.counts(), r.ndt_voxels()
    Prefilter(None, registration=r).cloud_callback(scans["vlp16"])
    assert r.counts() == before
    vox_after = r.ndt_voxels()
    assert np.array_equal(vox_before["keys"], vox_after["keys"]) and np.array_equal(vox_before["mean"], vox_after["mean"])
    r.setInputSource(src)
    r.align()
    assert np.array_equal(r.getFinalTransformation(), ref.getFinalTransformation())


def test_raw_tensor_through_prefilter_into_odometry_matches_the_host_path():
    import torch
    from delta_graph_slam_amd.odometry import ScanMatchingOdometry
    from delta_graph_slam_amd.prefilter import Prefilter
    clouds, _ = synth.vlp16_stream(n_frames=4)
    pf = Prefilter(R.LAUNCH)
    odo_h = ScanMatchingOdometry(params={"downsample_method": "NONE"})
    odo_d = ScanMatchingOdometry(params={"downsample_method": "NONE"})
    for k, c in enumerate(clouds):
        f_h, _ = pf.cloud_callback(c)
        f_d, _ = pf.cloud_callback(torch.from_numpy(c).cuda())
        assert f_d.is_cuda
        a = odo_h.matching(0.1 * k, f_h)
        b = odo_d.matching(0.1 * k, f_d)
        assert np.array_equal(a, b)


def test_edge_cases():
    from delta_graph_slam_amd import _lib as L
    pf = _pf()
    e3, e2 = pf.cloud_callback(np.zeros((0, 4), np.float32))
    assert e3.shape == (0, 4) and e2.shape == (0, 4)
    far = np.ones((100, 4), np.float32) * 200.0                    # all out of range
    e3, e2 = pf.cloud_callback(far)
    assert e3.shape == (0, 4) and e2.shape == (0, 4)
    bad = np.full((64, 4), np.nan, np.float32)
    bad[::2, :3] = np.inf
    e3, e2 = pf.cloud_callback(bad)
    assert e3.shape == (0, 4) and e2.shape == (0, 4)
    small = np.ones((15, 4), np.float32)
    small[:, :3] = np.random.default_rng(0).uniform(2, 3, (15, 3))
    with pytest.raises(L.DgsError) as ei:                          # n <= mean_k: upstream reads past its lists
        _pf({"downsample_method": "NONE"}).cloud_callback(small)
    assert ei.value.status == 1
    with pytest.raises(L.DgsError) as ei:                          # min_neighbors + 1 > 32
        _pf({"outlier_removal_method": "RADIUS", "radius_min_neighbors": 32}).radius_outlier_removal(small)
    assert ei.value.status == 1
    # fewer than 3 height-filtered points: NaN normals, empty 2-D cloud
    two = np.array([[3, 0, 1, 1], [3, 0.1, 1, 1], [3, 0.2, -1, 1], [3, 0.3, -1, 1]], np.float32)
    f3, f2 = _pf({"downsample_method": "NONE", "outlier_removal_method": "NONE"}).cloud_callback(two)
    assert np.array_equal(f3, two) and f2.shape == (0, 4)
    # duplicate points: zero covariance gives a NaN normal (dropped); the 3-D chain keeps them in order
    dup = np.ones((40, 4), np.float32)
    dup[:, :3] = [4.0, 1.0, 2.0]
    dup[20:, :3] = np.random.default_rng(1).uniform(3, 5, (20, 3))
    p = {"downsample_method": "NONE", "outlier_removal_method": "RADIUS", "radius_radius": 0.5, "radius_min_neighbors": 2}
    f3, f2 = _pf(p).cloud_callback(dup)
    r3, r2, _ = R.cloud_callback(dup, p, (0, 0, 0), None)
    assert np.array_equal(f3, r3) and np.array_equal(f2, r2)
    assert not any(np.array_equal(q[:2], [4.0, 1.0]) for q in f2)


def test_cpp_driver_matches_the_python_path(scans, tmp_path):
    exe = str(tmp_path / "prefilter_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "tests", "stub_pcl"), "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "prefilter_driver.cpp"), "-o", exe,
                           os.path.join(ROOT, "delta_graph_slam_amd", "libdgs_reg.so"), "-Wl,-rpath," + os.path.join(ROOT, "delta_graph_slam_amd"),
                           "-Wl,-rpath,/opt/rocm/lib"])
    c = scans["vlp16"]
    inp, o3, o2 = (str(tmp_path / n) for n in ("in.bin", "o3.bin", "o2.bin"))
    c.tofile(inp)
    subprocess.check_call([exe, "run", inp, "0.0", o3, o2, "outlier_removal_method=RADIUS", "radius_radius=0.5", "distance_near_thresh=0.1"], timeout=120)
    f3, f2 = _pf(R.LAUNCH).cloud_callback(c)
    assert np.array_equal(np.fromfile(o3, np.float32).reshape(-1, 4), f3)
    assert np.array_equal(np.fromfile(o2, np.float32).reshape(-1, 4), f2)
