"""interpolate / buildPointCloud / getCloud on the MI355X against the numpy restatement tests/building_cloud_reference.py: points and
item offsets bit for bit (NaN positions equal, payloads free).  No tolerance: every operation is one IEEE float32 add, subtract,
multiply, divide or square root.  What the cases are -- lengths that hit `i_k <= norm` as an equality, a long line that begins at a
tile start, the line on which the norm's association orders differ -- is asserted by tests/test_building_cloud_cpu.py."""
import json
import os
import subprocess

import numpy as np
import pytest

import building_cloud_cases as K
import building_cloud_reference as R

pytestmark = pytest.mark.gpu
F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def reg():
    from delta_graph_slam_amd.registration import Registration
    return Registration("NDT_OMP")


def _stage(c, registration=None):
    from delta_graph_slam_amd.building_cloud import BuildingClouds
    return BuildingClouds(registration=registration, params=c["params"])


def _run(c, registration=None, device=False):
    bc = _stage(c, registration)
    pts, off = bc.clouds(c["items"], c["transforms"], device=device)
    return bc, pts, off


def _assert_case(name, registration, c=None):
    c = c or K.named_cases()[name]
    want, woff = K.reference(name, c)
    bc, pts, off = _run(c, registration)
    assert off.dtype == np.int64 and np.array_equal(off, woff), name
    if pts.shape == want.shape:
        differ = (R.bits(pts) != R.bits(want)) & ~(np.isnan(pts) & np.isnan(want))
        print(f"{name}: {pts.shape[0]} points, {int(differ.sum())} words differ, first at {np.argwhere(differ)[:1].tolist()}")
    assert R.same_bits(pts, want), name
    n = bc.counts()
    assert n["launches"] == 3 and n["host_waits"] == 1 and n["points"] == want.shape[0] and n["items"] == len(c["items"])
    assert n["lines"] == sum(i.shape[0] for i in c["items"])
    return bc, pts, off


def test_tile_is_the_headers(reg):
    bc, _, _ = _run(K.short_call(), reg)
    assert bc.counts()["tile"] == K.TILE                                     # the cases are built around the library's own constant


@pytest.mark.parametrize("k", K.BOUNDARY_KS)
def test_count_boundary(reg, k):
    c, want = K.boundary(k)
    _, _, off = _assert_case(f"boundary_{k}", reg, c)
    assert np.diff(off).tolist() == want                                     # table[k] exactly, the float below, the float above


@pytest.mark.parametrize("n_lines", [1023, 1024, 1025, 2049])
def test_offsets_across_workgroups(reg, n_lines):
    _, pts, off = _assert_case(f"many_items_{n_lines}", reg)
    assert off[0] == off[1] == 0 and off[-1] == off[-2] == pts.shape[0] > K.TILE      # items without lines first and last


def test_no_items_and_one_zero_length_line(reg):
    _, pts, off = _assert_case("no_items", reg)
    assert pts.shape == (0, 4) and off.tolist() == [0]
    _, pts, off = _assert_case("one_zero_length", reg)
    assert pts.tolist() == [[3.25, -7.5, 0.0, 1.0]] and off.tolist() == [0, 1]
    _, pts, _ = _assert_case("zero_length_unguarded", reg)
    assert pts.shape == (1, 4) and np.isnan(pts[0, 0]) and np.isnan(pts[0, 1]) and pts[0, 2:].tolist() == [0.0, 1.0]


@pytest.mark.parametrize("shift", [-1, 0, 1])
def test_owner_search_at_tile_starts(reg, shift):
    _, pts, off = _assert_case(f"owner_{shift}", reg)
    assert pts[K.TILE + shift].tolist() == [3.0, 4.0, 0.0, 1.0]


def test_arithmetic(reg):
    _assert_case("arithmetic", reg)
    sizes = [_assert_case(f"sqnorm_{o}", reg)[1].shape[0] for o in (0, 1, 2)]
    assert sizes == [2100, 2099, 2100]


def test_random_lines(reg):
    lines = K.random_lines(200)
    c = K.case([lines[:70], lines[70:71], lines[71:]], [None, K.rigid(40.0, 3.0, -2.0), None])
    _assert_case("random_lines", reg, c)


def test_bad_input(reg):
    from delta_graph_slam_amd._lib import DgsError
    _, pts, off = _assert_case("nan_endpoint", reg)
    assert np.diff(off).tolist() == [6, 0, 3]                               # the NaN lines give no points
    ok, bad, where = K.past_the_table()
    inf, inf_where = K.infinite_endpoint()
    for c, (item, ln) in ((inf, inf_where), (bad, where)):
        bc = _stage(c, reg)
        with pytest.raises(DgsError) as e:
            bc.clouds(c["items"], c["transforms"])
        assert e.value.status == 1 and f"line {ln} of item {item}" in str(e.value)
        with pytest.raises(DgsError):
            bc.last()                                                        # nothing was produced
        _, pts, _ = _assert_case("table_end_64", reg, ok)                   # the same handle serves the next call
        assert pts.shape[0] == 64
        _assert_case("short_call", reg)


@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("kind", ["none", "shared", "identity", "per_item", "nan"])
def test_transforms(reg, kind, order):
    _, pts, off = _assert_case(f"transform_{kind}_{order}", reg)
    if kind == "identity":
        assert not np.any(np.signbit(pts[:, 0]) & (pts[:, 0] == 0))         # a -0.0 comes out +0.0
    if kind == "none":
        assert np.signbit(pts[off[4], 0]) and pts[off[4], 0] == 0
    if kind == "nan":
        assert np.all(np.isnan(pts[:off[1], 1])) and np.all(np.isnan(pts[off[3]:off[4], 0]))


def test_handle_reuse_and_table_growth():
    from delta_graph_slam_amd.registration import Registration
    one = Registration("NDT_OMP")
    seen = []
    for name in ("short_call", "growing_call", "short_call"):
        fresh = _assert_case(name, Registration("NDT_OMP"))[0].counts()
        bc, _, _ = _assert_case(name, one)
        n = bc.counts()
        seen.append(n)
        assert n["launches"] == fresh["launches"] == 3
    first, grown, again = seen
    assert first["table_added"] == first["table_entries"] > 0                # the first call makes the table
    assert grown["table_added"] > 0 and grown["table_entries"] == first["table_entries"] + grown["table_added"]
    assert again["table_added"] == 0 and again["table_entries"] == grown["table_entries"]
    assert first["host_waits"] == 1 and again["host_waits"] == 1 and 1 <= grown["host_waits"] <= 2
    # another step is another table
    c = K.case(K.short_call()["items"], None, sample_step=0.05)
    bc, _, _ = _assert_case("short_call_step_005", one, c)
    assert bc.counts()["table_added"] == bc.counts()["table_entries"]
    _assert_case("short_call", one)


def test_destinations_and_registration_state():
    import torch
    from delta_graph_slam_amd import synth
    from delta_graph_slam_amd.registration import Registration
    tgt, src, _ = synth.planar_pair(n=4096)
    r = Registration("NDT_OMP", ndt_resolution=1.0)
    r.setInputTarget(tgt)
    r.setInputSource(src)
    r.align()
    T0 = r.getFinalTransformation().copy()
    c = K.transforms("per_item", 0)
    bc, host, off = _run(c, r)
    dev, off_d = bc.last(device=True)
    assert isinstance(dev, torch.Tensor) and dev.is_cuda and np.array_equal(off, off_d)
    assert np.array_equal(R.bits(dev.cpu().numpy()), R.bits(host)) and R.same_bits(host, K.reference("transform_per_item_0")[0])
    assert np.array_equal(r.getFinalTransformation(), T0)                    # the stage left the result alone
    r.align()
    assert np.array_equal(r.getFinalTransformation(), T0)
    assert R.same_bits(bc.last()[0], host)                                  # and the registration left the stage's result alone


def test_python_entry_points(reg):
    from delta_graph_slam_amd import BuildingClouds
    bc = BuildingClouds(registration=reg)
    lines = K.outline(10.0, 5.0, 8.0, 6.0, 12.0)
    m = K.rigid(17.0, 100.0, -80.0)
    assert R.same_bits(bc.interpolate(lines[0, 0], lines[0, 1]), R.clouds([lines[:1]])[0])
    assert R.same_bits(bc.building_cloud(lines), R.clouds([lines])[0])
    assert R.same_bits(bc.get_cloud(lines, m), R.clouds([lines], m)[0])
    pts, off = bc.clouds([lines, lines[:2]], m)
    assert R.same_bits(pts, R.clouds([lines, lines[:2]], m)[0]) and off.tolist() == R.clouds([lines, lines[:2]], m)[1].tolist()


def test_cpp_adapter_gives_the_same_bits(tmp_path, reg):
    exe = str(tmp_path / "building_cloud_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "tests", "stub_pcl"), "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "building_cloud_driver.cpp"), "-o", exe,
                           os.path.join(ROOT, "delta_graph_slam_amd", "libdgs_reg.so"), "-Wl,-rpath," + os.path.join(ROOT, "delta_graph_slam_amd"),
                           "-Wl,-rpath,/opt/rocm/lib"])
    from delta_graph_slam_amd import BuildingClouds
    bc = BuildingClouds(registration=reg)
    lines = K.outline(-30.0, 40.0, 12.5, 7.25, 77.0)
    m = K.rigid(17.0, 100.0, -80.0)

    def run(mode, ls):
        ip, op = str(tmp_path / f"{mode}.in"), str(tmp_path / f"{mode}.out")
        with open(ip, "wb") as f:
            f.write(np.int32(ls.shape[0]).tobytes() + np.ascontiguousarray(ls, np.float64).tobytes() + np.ascontiguousarray(m, F).tobytes())
        res = json.loads(subprocess.check_output([exe, mode, ip, op], timeout=120).decode().splitlines()[-1])
        return res, (np.fromfile(op, F).reshape(-1, 4) if "n" in res else None)

    as_float = lines.astype(F).astype(np.float64)                            # interpolate takes Vector3f end points
    res, pts = run("interpolate", lines)
    assert res["n"] == pts.shape[0] == res["width"] and res["height"] == 1 and np.array_equal(R.bits(pts), R.bits(bc.interpolate(as_float[0, 0], as_float[0, 1])))
    res, pts = run("build", lines)
    assert np.array_equal(R.bits(pts), R.bits(bc.building_cloud(lines)))
    res, pts = run("getcloud", lines)
    assert np.array_equal(R.bits(pts), R.bits(bc.get_cloud(lines, m)))
    too_long = np.array([[[0.0, 0.0, 0.0], [1.0, 0.0, 0.0]], [[0.0, 0.0, 0.0], [30000.0, 1.0, 0.0]]])      # 30 km: past the 2^20 entries
    res, pts = run("build", too_long)
    assert res.get("null") is True and "line 1 of item 0" in res["error"] and pts is None      # the caller falls back to interpolate
