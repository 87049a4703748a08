"""The raw-scan head (deskewing, apps/prefiltering_nodelet.cpp:293-354, and the base_link transform, :122-150, fused into the distance
filter's pass) on the MI355X against the numpy restatement tests/prefilter_scan_reference.py: dgs_prefilter_deskew and
dgs_prefilter_scan bit for bit, at the sizes, switches and thresholds where the head can go wrong.

NaN: IEEE 754 leaves sign and payload of a NaN that an operation produces to the implementation (x86 SSE produces 0xffc00000,
gfx950 0x7fc00000), so where the restatement's arithmetic gives a NaN the device must give a NaN, and every other float must have the
restatement's bits.  Where no arithmetic runs (no angular velocity, no transform, the fourth float, a non-finite point through the
transform) NaN payloads are compared bit for bit as well."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import prefilter_reference as R
import prefilter_scan_reference as S
from delta_graph_slam_amd import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

LARGE = 262144 + 301                       # 1,026 workgroups of 256: the scan's second chunk and its carry run behind the head
SIZES = [1, 2, 63, 64, 65, 1023, 1025, LARGE]
TYPICAL = (0.3, -0.8, 1.1)                 # about 1.4 rad/s
FAST = (30.0, -25.0, 31.0)                 # about 50 rad/s: |q|² far from 1
ZERO = (0.0, 0.0, 0.0)
VELOCITIES = [("typical", TYPICAL), ("fast", FAST), ("zero", ZERO), ("none", None)]
NOFILTER = dict(downsample_method="NONE", outlier_removal_method="NONE")


def _pf(params=None):
    from delta_graph_slam_amd.prefilter import Prefilter
    return Prefilter(params)


def _raw_cloud(n, seed=11):
    """Points on both sides of both distance thresholds, with -0.0f coordinates, NaN (with a payload), +-Inf and odd fourth floats."""
    rng = np.random.default_rng(seed + n)
    c = np.empty((n, 4), np.float32)
    c[:, :3] = rng.normal(size=(n, 3)) * 40.0
    c[::7, :3] *= np.float32(0.01)
    c[:, 3] = rng.normal(size=n)
    if n >= 63:
        nan = np.array([0x7fc12345], np.uint32).view(np.float32)[0]
        c[3, 0] = -0.0
        c[4, :3] = [-0.0, 2.5, -0.0]
        c[5, 1] = nan
        c[6, 2] = np.inf
        c[7, 0] = -np.inf
        c[8, :3] = nan
        c[9, 3] = nan
        c[n - 2, 1] = -0.0
        c[n // 2, 0] = np.inf
    return c


@pytest.fixture(scope="module")
def clouds():
    return {n: _raw_cloud(n) for n in SIZES}


@pytest.fixture(scope="module")
def vlp16():
    xyz, _ = synth.street_scan((-30.0, 1.0, 0.1), 16, (15.0, -15.0), 1875, 21)
    return synth._xyz1(xyz)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _assert_same(out, ref, exact_nan):
    out = np.asarray(out)
    assert out.shape == ref.shape
    if exact_nan:
        assert np.array_equal(_bits(out), _bits(ref))
        return
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(out), nan)
    assert np.array_equal(_bits(out)[~nan], _bits(ref)[~nan])
    assert np.array_equal(_bits(out[:, 3]), _bits(ref[:, 3]))          # the fourth float is copied or set, never computed


def _host(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else x


@pytest.mark.parametrize("n", SIZES)
def test_deskew_is_bit_equal_at_every_size_velocity_and_norm_order(clouds, n):
    import torch
    c = clouds[n]
    cd = torch.from_numpy(c).cuda()
    pf = _pf()
    for vname, w in VELOCITIES:
        for order in S.NORM_ORDERS:
            pf.deskew_norm_order = order
            ref = S.deskew(c, w, deskew_norm_order=order)
            for src in (c, cd):
                out = pf.deskew(src, w)
                assert (src is c) or out.is_cuda
                out = _host(out)
                assert out.shape[0] == n                                # non-finite points included
                _assert_same(out, ref, exact_nan=w is None)
                # the last point carries the largest i / n
                fin = ~np.isnan(ref[n - 1])
                assert np.array_equal(_bits(out[n - 1])[fin], _bits(ref[n - 1])[fin]), (vname, order)
        if w is None:
            assert np.array_equal(_bits(ref), _bits(c))
        elif w is not ZERO and n > 1 and np.all(np.isfinite(c[n - 1, :3])):
            assert not np.array_equal(ref[n - 1, :3], c[n - 1, :3])     # the case moves the last point: the comparison above is not vacuous
    if n >= 63:
        zero = _host(pf.deskew(c, ZERO))
        assert zero[3, 0] == 0 and not np.signbit(zero[3, 0]) and np.signbit(c[3, 0])      # -0.0f comes out +0.0f, as the restatement's
        assert not np.signbit(S.deskew(c, ZERO)[3, 0])
        none = _host(pf.deskew(c, None))
        assert np.signbit(none[3, 0]) and _bits(none[5, 1]) == 0x7fc12345


def test_norm_order_switch_is_observable_on_the_device(clouds):
    c = clouds[1025]
    pf = _pf()
    outs = []
    for order in S.NORM_ORDERS:
        pf.deskew_norm_order = order
        outs.append(pf.deskew(c, FAST))
    fin = np.all(np.isfinite(c[:, :3]), 1)
    for a, b in ((0, 1), (0, 2), (1, 2)):
        assert not np.array_equal(outs[a][fin], outs[b][fin])


@pytest.mark.parametrize("n", [1, 65, 1025])
@pytest.mark.parametrize("sets_w", [1, 0])
def test_transform_is_bit_equal_with_and_without_deskew(clouds, n, sets_w):
    import torch
    c = clouds[n]
    m = S.base_link_matrix()
    pf = _pf(NOFILTER)
    pf.transform_sets_w = sets_w
    for w in (None, TYPICAL):
        ref, lidar = S.head(c, w, m, transform_sets_w=sets_w)
        for src in (c, torch.from_numpy(c).cuda()):
            out = _host(pf.deskew(src, w, m))
            _assert_same(out, ref, exact_nan=w is None)
            nonfin = ~np.all(np.isfinite(S.deskew(c, w)[:, :3]), 1)
            if w is None:
                assert np.array_equal(_bits(out[nonfin]), _bits(c[nonfin]))      # a non-finite point is copied whole, fourth float included
            f3, f2, lp = pf.filter_scan(src, w, m)
            assert np.array_equal(lp, [0.0, 0.0, m[2, 3]]) and np.array_equal(lp, lidar)
            assert np.array_equal(_bits(_host(f3)), _bits(R.distance_filter(ref)))   # bits: a kept point may carry a NaN fourth float
    assert m[0, 3] != 0.0 and m[1, 3] != 0.0                                      # the adapter zeroed them, not the caller
    _, _, lp = pf.filter_scan(c, TYPICAL, None)
    assert np.array_equal(lp, [0.0, 0.0, 0.0])


def threshold_cloud(n=2048, seed=17, near=1.0, far=100.0, rounds=60):
    """Raw points whose norm after deskew (TYPICAL) and transform is the float just below, at, or just above `near` (even slots) or
    `far` (odd slots).  Each slot starts from the float64 pre-image of a point on the threshold sphere and is moved by a few ulps
    until the restatement gives the wanted norm; slots that never get there stay as ordinary points.
    -> (cloud, hit mask, matrix)."""
    rng = np.random.default_rng(seed)
    m, _ = S.centered(S.base_link_matrix())
    idx = np.arange(n)
    # the head is affine per slot in exact arithmetic: out = A_i p + t
    A = np.stack([S.deskew_exact(np.tile(e, (n, 1)), idx, n, TYPICAL) @ m[:3, :3].T for e in np.eye(3)], 2)
    t32 = np.where(idx % 2 == 0, np.float32(near), np.float32(far)).astype(np.float32)
    want = np.where(idx % 3 == 0, np.nextafter(t32, np.float32(0)), np.where(idx % 3 == 1, t32, np.nextafter(t32, np.float32(np.inf))))
    u = rng.normal(size=(n, 3))
    q = u / np.linalg.norm(u, axis=1, keepdims=True) * t32.astype(np.float64)[:, None]
    p0 = np.linalg.solve(A, (q - m[:3, 3])[:, :, None])[:, :, 0]
    cloud = np.ones((n, 4), np.float32)
    cloud[:, :3] = p0
    hit = np.zeros(n, bool)
    for _ in range(rounds):
        out, _ = S.head(cloud, TYPICAL, m)
        d = np.sqrt((out[:, 0] * out[:, 0] + out[:, 1] * out[:, 1]) + out[:, 2] * out[:, 2])
        hit = d == want
        if hit.all():
            break
        base = p0.astype(np.float32)
        cand = base + rng.integers(-4, 5, (n, 3)).astype(np.float32) * np.spacing(np.abs(base))
        cloud[~hit, :3] = cand[~hit]
    return cloud, hit, m


def test_points_on_the_distance_thresholds_are_decided_as_the_restatement_decides():
    cloud, hit, m = threshold_cloud()
    near, far = 1.0, 100.0
    ref, _ = S.head(cloud, TYPICAL, m)
    keep = R.distance_filter(ref, near, far)
    ref_fma, _ = S.head(cloud, TYPICAL, m, fma=True)

    def decide(c):
        d = np.sqrt((c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1]) + c[:, 2] * c[:, 2]).astype(np.float64)
        return (d > near) & (d < far)
    flips = decide(ref) != decide(ref_fma)
    print(f"threshold cloud: {int(hit.sum())} of {cloud.shape[0]} slots within one ulp of a threshold, "
          f"{int(flips.sum())} on which a fused rotation decides the other way, {keep.shape[0]} kept")
    assert int(hit.sum()) >= 300                                   # the search found its points ...
    assert int(flips.sum()) >= 10                                  # ... and points that tell a contracted rotation apart
    assert 0 < keep.shape[0] < cloud.shape[0]
    pf = _pf(NOFILTER)
    f3, _, _ = pf.filter_scan(cloud, TYPICAL, m)
    assert np.array_equal(_bits(f3), _bits(keep))                  # the same points, in order
    import torch
    f3d, _, _ = pf.filter_scan(torch.from_numpy(cloud).cuda(), TYPICAL, m)
    assert np.array_equal(_bits(_host(f3d)), _bits(keep))


@pytest.mark.parametrize("n", SIZES)
def test_fused_head_keeps_the_restatements_points_at_every_size(clouds, n):
    c = clouds[n]
    m = S.base_link_matrix()
    pf = _pf(NOFILTER)
    for w in (FAST, None):
        ref, _ = S.head(c, w, m)
        f3, f2, _ = pf.filter_scan(c, w, m)
        assert np.array_equal(_bits(f3), _bits(R.distance_filter(ref)))
    # neither step: dgs_prefilter on the raw cloud
    f3, f2, lp = pf.filter_scan(c)
    g3, g2 = pf.cloud_callback(c)
    assert np.array_equal(_bits(f3), _bits(g3)) and np.array_equal(_bits(f2), _bits(g2)) and not lp.any()


@pytest.mark.parametrize("pname,params", [("launch", R.LAUNCH), ("defaults", R.DEFAULTS)])
@pytest.mark.parametrize("ds", ["VOXELGRID", "NONE"])
def test_fused_call_equals_its_parts(vlp16, pname, params, ds):
    import torch
    params = dict(params, downsample_method=ds)
    m = S.base_link_matrix()
    pf = _pf(params)
    for src in (vlp16, torch.from_numpy(vlp16).cuda()):
        f3, f2, lp = pf.filter_scan(src, TYPICAL, m)
        mid = pf.deskew(src, TYPICAL, m)
        g3, g2 = pf.cloud_callback(mid, lp)
        assert f3.shape[0] > 1000 and f2.shape[0] > 100
        assert f3.shape == g3.shape and f2.shape == g2.shape
        assert np.array_equal(_bits(_host(f3)), _bits(_host(g3))) and np.array_equal(_bits(_host(f2)), _bits(_host(g2)))
        # neither step enabled: dgs_prefilter on the raw frame with a zero lidar position
        f3, f2, lp = pf.filter_scan(src)
        g3, g2 = pf.cloud_callback(src)
        assert not lp.any()
        assert np.array_equal(_bits(_host(f3)), _bits(_host(g3))) and np.array_equal(_bits(_host(f2)), _bits(_host(g2)))
    print(f"vlp16 {pname} {ds}: fused equals parts")


def _raw_scan(pf, sp, c, cap3, cap2):
    from delta_graph_slam_amd import _lib as L
    o3, o2 = np.zeros((max(cap3, 1), 4), np.float32), np.zeros((max(cap2, 1), 4), np.float32)
    n3, n2 = C.c_int64(-1), C.c_int64(-1)
    lp = np.full(3, -1.0)
    rc = pf._lib.dgs_prefilter_scan(pf._h, C.byref(pf.params), C.byref(sp), c.ctypes.data_as(C.c_void_p), c.shape[0], 0, o3.ctypes.data_as(C.c_void_p),
                                    cap3, o2.ctypes.data_as(C.c_void_p), cap2, 0, C.byref(n3), C.byref(n2), lp.ctypes.data_as(C.c_void_p))
    return rc, n3.value, n2.value, lp


def _raw_chain(pf, c, cap3, cap2):
    o3, o2 = np.zeros((max(cap3, 1), 4), np.float32), np.zeros((max(cap2, 1), 4), np.float32)
    n3, n2 = C.c_int64(-1), C.c_int64(-1)
    rc = pf._lib.dgs_prefilter(pf._h, C.byref(pf.params), c.ctypes.data_as(C.c_void_p), c.shape[0], 0, None, o3.ctypes.data_as(C.c_void_p), cap3,
                               o2.ctypes.data_as(C.c_void_p), cap2, 0, C.byref(n3), C.byref(n2))
    return rc, n3.value, n2.value


def test_errors_behave_as_dgs_prefilter_does(clouds):
    from delta_graph_slam_amd import _lib as L
    c = clouds[1025]
    pf = _pf(NOFILTER)
    sp = pf._scan_params(None, None, 0.1)
    n = c.shape[0]
    ok = _raw_scan(pf, sp, c, n, n)
    assert ok[0] == 0 and ok[:3] == _raw_chain(pf, c, n, n) and ok[1] > 0
    # a capacity that is too small, for either output: the status and the counts of dgs_prefilter
    for cap3, cap2 in ((ok[1] - 1, n), (n, max(ok[2] - 1, 0)), (0, 0)):
        assert _raw_scan(pf, sp, c, cap3, cap2)[:3] == _raw_chain(pf, c, cap3, cap2)
    assert _raw_scan(pf, sp, c, ok[1] - 1, n)[0] == 1
    # wrong struct sizes and a norm order that does not exist
    bad = pf._scan_params(TYPICAL, None, 0.1)
    bad.struct_size -= 4
    assert _raw_scan(pf, bad, c, n, n)[0] == 1
    bad = pf._scan_params(TYPICAL, None, 0.1)
    bad.deskew_norm_order = 3
    assert _raw_scan(pf, bad, c, n, n)[0] == 1
    size = pf.params.struct_size
    pf.params.struct_size = size - 4
    assert _raw_scan(pf, sp, c, n, n)[0] == 1 and _raw_chain(pf, c, n, n)[0] == 1
    pf.params.struct_size = size
    m = C.c_int64(-1)
    out = np.zeros((n, 4), np.float32)
    assert pf._lib.dgs_prefilter_deskew(pf._h, C.byref(bad), c.ctypes.data_as(C.c_void_p), n, 0, out.ctypes.data_as(C.c_void_p), n, 0, C.byref(m)) == 1
    assert pf._lib.dgs_prefilter_deskew(pf._h, C.byref(sp), c.ctypes.data_as(C.c_void_p), n, 0, out.ctypes.data_as(C.c_void_p), n - 1, 0, C.byref(m)) == 1
    with pytest.raises(L.DgsError) as ei:                                   # the chain's own errors pass through: n <= mean_k
        _pf({"downsample_method": "NONE"}).filter_scan(np.ascontiguousarray(c[20:35]), TYPICAL)
    assert ei.value.status == 1
    # n = 0: two empty clouds, and the lidar position all the same
    e = np.zeros((0, 4), np.float32)
    f3, f2, lp = pf.filter_scan(e, TYPICAL, S.base_link_matrix())
    assert f3.shape == (0, 4) and f2.shape == (0, 4) and np.array_equal(lp, [0.0, 0.0, 1.7])
    assert pf.deskew(e, TYPICAL).shape == (0, 4)
    g3, g2 = pf.cloud_callback(e)
    assert g3.shape == f3.shape and g2.shape == f2.shape
    # the handle is still usable
    assert _raw_scan(pf, sp, c, n, n)[:3] == ok[:3]


def test_registration_sharing_the_handle_is_untouched_by_the_scan_entry_points(vlp16):
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
    pf = Prefilter(None, registration=r)
    pf.filter_scan(vlp16, TYPICAL, S.base_link_matrix())
    pf.deskew(vlp16, TYPICAL, S.base_link_matrix())
    assert r.counts() == before
    vox_after = r.ndt_voxels()
    assert np.array_equal(vox_before["keys"], vox_after["keys"]) and np.array_equal(vox_before["mean"], vox_after["mean"])
    r.setInputSource(src)
    r.align()
    assert np.array_equal(r.getFinalTransformation(), ref.getFinalTransformation())


def test_a_handle_that_ran_the_large_size_gives_a_small_cloud_the_bits_of_a_fresh_one(clouds):
    m = S.base_link_matrix()
    used = _pf(NOFILTER)
    used.filter_scan(clouds[LARGE], FAST, m)
    used.deskew(clouds[LARGE], FAST, m)
    for n in (1025, 65, 1):
        fresh = _pf(NOFILTER)
        a = used.filter_scan(clouds[n], TYPICAL, m)
        b = fresh.filter_scan(clouds[n], TYPICAL, m)
        assert np.array_equal(_bits(a[0]), _bits(b[0])) and np.array_equal(_bits(a[1]), _bits(b[1]))
        assert np.array_equal(_bits(used.deskew(clouds[n], TYPICAL, m)), _bits(fresh.deskew(clouds[n], TYPICAL, m)))


def test_cpp_driver_matches_the_python_path(vlp16, tmp_path):
    exe = str(tmp_path / "prefilter_scan_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "tests", "stub_pcl"), "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "prefilter_scan_driver.cpp"), "-o", exe,
                           os.path.join(ROOT, "delta_graph_slam_amd", "libdgs_reg.so"), "-Wl,-rpath," + os.path.join(ROOT, "delta_graph_slam_amd"),
                           "-Wl,-rpath,/opt/rocm/lib"])
    m = S.base_link_matrix()
    inp, o3, o2 = (str(tmp_path / n) for n in ("in.bin", "o3.bin", "o2.bin"))
    vlp16.tofile(inp)
    res = subprocess.check_output([exe, "run", inp, o3, o2, ",".join(repr(v) for v in TYPICAL), ",".join(repr(float(v)) for v in m.reshape(16)),
                                   "outlier_removal_method=RADIUS", "radius_radius=0.5", "distance_near_thresh=0.1", "scan_period=0.1"], timeout=120)
    res = json.loads(res.decode().strip().splitlines()[-1])
    f3, f2, lp = _pf(R.LAUNCH).filter_scan(vlp16, TYPICAL, m)
    assert res["lidar"] == [0.0, 0.0, m[2, 3]] and np.array_equal(lp, res["lidar"])
    assert res["n3d"] == f3.shape[0] and res["n2d"] == f2.shape[0] and f3.shape[0] > 1000
    assert np.array_equal(np.fromfile(o3, np.float32).reshape(-1, 4), f3)
    assert np.array_equal(np.fromfile(o2, np.float32).reshape(-1, 4), f2)
