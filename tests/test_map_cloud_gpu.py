"""MapCloudGenerator::generate (src/hdl_graph_slam/map_cloud_generator.cpp:13-50) on the MI355X against the closed form of
tests/map_cloud_reference.py: bit-equal and in order, with no tolerance -- every operation is IEEE float without contraction or
double.  Inputs: the CPU test's edge clouds, 64 prefiltered synthetic keyframes along a trajectory (flat snapshots and 3-D clouds),
host arrays / device tensors / resident clouds, the switches, the limits, a shared handle, the C++ adapter and the key table at its
edges."""
import os
import struct
import subprocess

import numpy as np
import pytest

import map_cloud_edge_cases as E
import map_cloud_reference as R
from delta_graph_slam_amd import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = E.edge_cases()
SWITCHES = E.switch_cases()
N_KEYFRAMES = 64


def _gen(params=None, registration=None):
    from delta_graph_slam_amd.map_cloud import MapCloudGenerator
    return MapCloudGenerator(registration=registration, params=params)


def _check(gen, kfs, res, sw=None, what=""):
    """one map on the device against the closed form: points, order, and the octree itself through the grid hook"""
    want, grid = R.generate(kfs, res, sw, with_grid=True)
    got = gen.generate(kfs, res)
    g = gen.grid()
    print(f"{what}: res={res} points={sum(len(c) for c, _ in kfs)} voxels={want.shape[0]} got={got.shape[0]} depth={g['depth']}/{grid['depth']} "
          f"growths={g['growths']}/{grid['growths']}")
    assert got.dtype == np.float32 and got.shape == want.shape
    assert got.tobytes() == want.tobytes()
    assert g["depth"] == grid["depth"] and g["growths"] == grid["growths"]
    assert np.array_equal(g["min"], grid["min"]) and np.array_equal(g["max"], grid["max"])
    return got


@pytest.fixture(scope="module")
def gen():
    return _gen()


@pytest.fixture(scope="module")
def keyframes():
    """64 VLP-16 frames along synth.vlp16_stream's S-curve through the prefilter chain: the flat clouds with the snapshot poses
    KeyFrameSnapshot makes of a 2-D estimate, and the 3-D clouds with full poses (a little roll and pitch added)."""
    from delta_graph_slam_amd.map_cloud import snapshot_pose
    from delta_graph_slam_amd.prefilter import Prefilter
    clouds, poses = synth.vlp16_stream(n_frames=N_KEYFRAMES)
    pf = Prefilter(dict(distance_near_thresh=0.1, outlier_removal_method="RADIUS", radius_radius=0.5, radius_min_neighbors=2))
    rng = np.random.default_rng(11)
    flat, full = [], []
    for c, T in zip(clouds, poses):
        f3, f2 = pf.cloud_callback(c)
        yaw = np.arctan2(T[1, 0], T[0, 0])
        est = np.array([[np.cos(yaw), -np.sin(yaw), T[0, 3]], [np.sin(yaw), np.cos(yaw), T[1, 3]], [0, 0, 1]], np.float64)
        flat.append((f2, snapshot_pose(est)))
        tilt = synth.make_transform((0, 0, 0), (rng.uniform(-0.02, 0.02), rng.uniform(-0.02, 0.02), 0.0))
        full.append((f3, T @ tilt))
    return {"flat": flat, "3d": full}


@pytest.mark.parametrize("name", sorted(CASES))
def test_edge_clouds_are_bit_equal_and_in_order(gen, name):
    kfs, res = CASES[name]
    _check(gen, kfs, res, what=name)


@pytest.mark.parametrize("kind", ["flat", "3d"])
@pytest.mark.parametrize("res", [0.05, 0.01, 1.0])
def test_synthetic_keyframes_host_device_and_resident_agree(gen, keyframes, kind, res):
    import torch
    kfs = keyframes[kind]
    assert all(len(c) > 0 for c, _ in kfs)
    host = _check(gen, kfs, res, what=f"{kind} host")
    dev = gen.generate([(torch.from_numpy(c).cuda(), p) for c, p in kfs], res)
    assert dev.is_cuda and np.array_equal(dev.cpu().numpy().view(np.uint32), host.view(np.uint32))
    resident = [(gen.registration.make_cloud(c), p) for c, p in kfs]
    out = gen.generate(resident, res)
    assert out.is_cuda and np.array_equal(out.cpu().numpy().view(np.uint32), host.view(np.uint32))
    assert np.array_equal(gen.last().view(np.uint32), host.view(np.uint32))          # the map stays on the handle
    for c, _ in resident:
        c.close()


@pytest.mark.parametrize("res", [0.0, -1.0])
def test_no_resolution_gives_the_concatenation(gen, keyframes, res):
    import torch
    for kfs in (keyframes["flat"][:8], CASES["nan_and_inf_points"][0], CASES["empty_keyframe_in_the_middle"][0]):
        want = R.generate(kfs, res)
        got = gen.generate(kfs, res)
        assert got.shape == want.shape and got.tobytes() == want.tobytes() and np.all(got[:, 3] == 1.0)
        dev = gen.generate([(torch.from_numpy(np.ascontiguousarray(c)).cuda(), p) for c, p in kfs], res)
        assert dev.is_cuda and dev.cpu().numpy().tobytes() == want.tobytes()
        g = gen.grid()
        assert g["depth"] == 0 and g["growths"] == 0 and not g["min"].any() and not g["max"].any()


@pytest.mark.parametrize("name", sorted(SWITCHES))
def test_each_switch_changes_the_map_on_its_input(name):
    kfs, res = SWITCHES[name]
    out = {v: _check(_gen({name: v}), kfs, res, {name: v}, what=f"{name}={v}") for v in (0, 1)}
    assert out[0].tobytes() != out[1].tobytes()


def test_an_empty_keyframe_in_the_middle_changes_nothing(gen):
    a = gen.generate(*CASES["empty_keyframe_in_the_middle"])
    ga = gen.grid()
    b = gen.generate(*CASES["without_the_empty_keyframe"])
    gb = gen.grid()
    assert a.shape[0] > 0 and a.tobytes() == b.tobytes()
    assert ga["depth"] == gb["depth"] and np.array_equal(ga["min"], gb["min"])
    assert gen.generate([], 0.05) is None                                   # :14-17
    assert gen.generate([(np.zeros((0, 4), np.float32), np.eye(4))], 0.05).shape == (0, 4)


def test_a_span_that_needs_depth_22_is_too_large_and_the_handle_stays_usable(gen):
    from delta_graph_slam_amd import _lib as L
    far = [(E.xyz1([(0, 0, 0), (1, 1, 1), (3.0e4, 0, 0), (2, 2, 2)]), np.eye(4))]
    with pytest.raises(R.GridTooLarge):
        R.generate(far, 0.01)
    with pytest.raises(L.DgsError) as ei:
        gen.generate(far, 0.01)
    assert ei.value.status == 5                                             # DGS_ERR_GRID_TOO_LARGE
    assert gen.last().shape == (0, 4)                                       # nothing is produced
    _check(gen, [(E.xyz1([(0, 0, 0), (2.0e4, 0, 0)]), np.eye(4))], 0.01, what="depth 21")
    assert gen.grid()["depth"] == 21
    _check(gen, *CASES["flat_keyframes"], what="after the error")


def test_a_registration_sharing_the_handle_is_untouched(keyframes):
    from delta_graph_slam_amd.registration import Registration
    tgt, src, _ = synth.planar_pair(n=16384)
    fresh = Registration("NDT_OMP", ndt_resolution=1.0)
    fresh.setInputTarget(tgt)
    fresh.setInputSource(src)
    fresh.align()
    r = Registration("NDT_OMP", ndt_resolution=1.0)
    r.setInputTarget(tgt)
    kfs = keyframes["3d"][:16]
    resident = [r.make_cloud(c) for c, _ in kfs]
    r.setInputSource(resident[3])
    r.align()
    T_before = r.getFinalTransformation().copy()
    before, vox_before = r.counts(), r.ndt_voxels()
    gen = _gen(registration=r)
    got = gen.generate(list(zip(resident, [p for _, p in kfs])), 0.05)
    assert got.cpu().numpy().tobytes() == R.generate(kfs, 0.05).tobytes()
    assert r.counts() == before
    vox_after = r.ndt_voxels()
    assert np.array_equal(vox_before["keys"], vox_after["keys"]) and np.array_equal(vox_before["mean"], vox_after["mean"])
    r.setInputSource(resident[3])                                           # the resident clouds still align to the same result
    r.align()
    assert np.array_equal(r.getFinalTransformation(), T_before)
    r.setInputSource(src)
    r.align()
    assert np.array_equal(r.getFinalTransformation(), fresh.getFinalTransformation())
    for c in resident:
        c.close()


def test_loop_detector_keyframes_come_from_its_resident_clouds(gen, keyframes):
    from delta_graph_slam_amd.loop_detector import KeyFrame, LoopDetector
    from delta_graph_slam_amd.map_cloud import snapshot_pose
    ld = LoopDetector(registration=gen.registration, cache_clouds=True)
    rng = np.random.default_rng(5)
    kfs = []
    for k, (c, _) in enumerate(keyframes["flat"][:12]):
        yaw = rng.uniform(-3, 3)
        est = np.array([[np.cos(yaw), -np.sin(yaw), rng.uniform(-30, 30)], [np.sin(yaw), np.cos(yaw), rng.uniform(-30, 30)], [0, 0, 1]])
        kfs.append(KeyFrame(cloud=c, estimate=est, id=k))
    want = R.generate([(k.cloud, snapshot_pose(k.estimate)) for k in kfs], 0.05)
    got = gen.generate(kfs, 0.05, loop_detector=ld)
    assert got.is_cuda and len(ld._cloud_cache) == len(kfs)
    assert got.cpu().numpy().tobytes() == want.tobytes()
    assert gen.generate(kfs, 0.05).tobytes() == want.tobytes()             # without the detector: the keyframes' own host clouds


def _write_driver_input(path, kfs):
    with open(path, "wb") as f:
        f.write(struct.pack("i", len(kfs)))
        for c, pose in kfs:
            f.write(struct.pack("i", len(c)))
            f.write(np.ascontiguousarray(np.asarray(pose, np.float64).T).tobytes())      # column-major
            f.write(np.ascontiguousarray(c, np.float32).tobytes())


def test_cpp_driver_matches_the_python_path(gen, keyframes, tmp_path):
    exe = str(tmp_path / "map_cloud_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "tests", "stub_pcl"), "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "map_cloud_driver.cpp"), "-o", exe,
                           os.path.join(ROOT, "delta_graph_slam_amd", "libdgs_reg.so"), "-Wl,-rpath," + os.path.join(ROOT, "delta_graph_slam_amd"),
                           "-Wl,-rpath,/opt/rocm/lib"])
    kfs = keyframes["flat"][:12] + [(np.zeros((0, 4), np.float32), np.eye(4))] + keyframes["3d"][:4]
    inp, out = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    _write_driver_input(inp, kfs)
    for res, extra in ((0.05, []), (0.05, ["matrix"]), (0.0, [])):
        msg = subprocess.check_output([exe, "run", inp, repr(res), out] + extra, timeout=120).decode()
        assert '"null"' not in msg and '"is_dense": 0' in msg, msg
        assert np.fromfile(out, np.float32).reshape(-1, 4).tobytes() == gen.generate(kfs, res).tobytes()
    _write_driver_input(inp, [])
    assert '"null": true' in subprocess.check_output([exe, "run", inp, "0.05", out], timeout=120).decode()


def test_key_table_at_high_load_wraps_and_the_sort_path_gives_the_same_map(keyframes):
    from delta_graph_slam_amd import _lib as L
    # the smallest table that holds every voxel: load between 1/2 and 1, the probe sequences run over the table's end; with at most
    # 4096 slots a probe sequence may visit the whole table, so the insert cannot fail
    for name in ("flat_keyframes", "tiny_resolution", "wide_3d_keyframes"):
        kfs, res = CASES[name]
        want = R.generate(kfs, res)
        n = want.shape[0]
        slots = 1 << int(np.ceil(np.log2(n)))
        assert 4096 >= slots >= n > slots // 2
        print(f"{name}: voxels={n} slots={slots} load={n / slots:.3f}")
        for params in ({"dedup_method": "HASH", "hash_slots": slots}, {"dedup_method": "HASH", "hash_slots": slots - 5}, {"dedup_method": "SORT"},
                       {"hash_slots": slots // 2}, {"hash_slots": 2}):      # the last two overflow: AUTO falls back to the sort
            assert _gen(params).generate(kfs, res).tobytes() == want.tobytes(), params
        with pytest.raises(L.DgsError) as ei:         # HASH alone: a table smaller than the map is an error, not a wrong map
            _gen({"dedup_method": "HASH", "hash_slots": slots // 2}).generate(kfs, res)
        assert ei.value.status == 1
    kfs = keyframes["3d"][:8]
    bad = kfs[2][0].copy()
    bad[5, 0] = np.nan            # on the sort path a non-finite point is a sentinel key that must not become a voxel
    kfs = kfs[:2] + [(bad, kfs[2][1])] + kfs[3:]
    want = R.generate(kfs, 0.05)
    for params in ({}, {"dedup_method": "HASH"}, {"dedup_method": "SORT"}, {"hash_slots": 64}):
        assert _gen(params).generate(kfs, 0.05).tobytes() == want.tobytes(), params
