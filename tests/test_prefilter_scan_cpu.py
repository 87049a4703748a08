"""CPU tests of the raw-scan head (deskewing, apps/prefiltering_nodelet.cpp:293-354, and the base_link transform, :122-150): the
dgs_prefilter_scan_params layout and defaults, the IMU queue in its three forms, and the numpy restatement
tests/prefilter_scan_reference.py against an independent float64 formula."""
import ctypes as C
import json
import os
import subprocess
import tempfile

import numpy as np
import pytest

import prefilter_scan_reference as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_scan_params_layout_and_defaults_match_the_header():
    from delta_graph_slam_amd import _lib as L
    fields = ["has_angular_velocity", "angular_velocity", "scan_period", "has_transform", "transform", "deskew_norm_order", "transform_sets_w"]
    src = r'''
#include <stdio.h>
#include <stddef.h>
#include "dgs_reg.h"
int main(void) {
  printf("%zu", sizeof(dgs_prefilter_scan_params));
''' + "".join(f'  printf(" %zu", offsetof(dgs_prefilter_scan_params, {f}));\n' for f in fields) + r'''
  printf("\n");
  return 0;
}'''
    with tempfile.TemporaryDirectory() as d:
        cfile = os.path.join(d, "t.c")
        open(cfile, "w").write(src)
        exe = os.path.join(d, "t")
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), cfile, "-o", exe])
        vals = [int(x) for x in subprocess.check_output([exe]).split()]
    P = L.PrefilterScanParams
    assert vals == [C.sizeof(P)] + [getattr(P, f).offset for f in fields]
    lib = L.load()
    p = P()
    assert lib.dgs_prefilter_scan_params_init(C.byref(p)) == 0
    assert p.struct_size == C.sizeof(P)
    assert p.has_angular_velocity == 0 and list(p.angular_velocity) == [0.0, 0.0, 0.0] and p.scan_period == S.SCAN_PERIOD
    assert p.has_transform == 0 and np.array_equal(np.array(p.transform).reshape(4, 4), np.eye(4))
    assert p.deskew_norm_order == S.DESKEW_NORM_ORDER and p.transform_sets_w == S.TRANSFORM_SETS_W
    assert lib.dgs_prefilter_scan_params_init(None) == 1
    assert lib.dgs_abi_version() == 5


def test_scan_entry_points_reject_bad_arguments_without_touching_a_device():
    from delta_graph_slam_amd import _lib as L
    lib = L.load()
    cp, sp = L.PrefilterParams(), L.PrefilterScanParams()
    lib.dgs_prefilter_params_init(C.byref(cp))
    lib.dgs_prefilter_scan_params_init(C.byref(sp))
    n3, n2 = C.c_int64(7), C.c_int64(7)
    # no handle
    assert lib.dgs_prefilter_scan(None, C.byref(cp), C.byref(sp), None, 0, 0, None, 0, None, 0, 0, C.byref(n3), C.byref(n2), None) == 1
    assert lib.dgs_prefilter_deskew(None, C.byref(sp), None, 0, 0, None, 0, 0, C.byref(n3)) == 1


# (name, stamps in the queue, scan stamp): empty, all earlier, all later, equal stamps (`>` is strict), one message
QUEUES = [("empty", [], 10.0), ("all earlier", [1.0, 2.0, 3.0], 10.0), ("all later", [11.0, 12.0, 13.0], 10.0),
          ("equal stamps", [9.0, 10.0, 10.0, 11.0, 12.0], 10.0), ("equal is the last", [9.0, 10.0], 10.0),
          ("one earlier", [5.0], 10.0), ("one later", [15.0], 10.0), ("one equal", [10.0], 10.0), ("mixed", [8.0, 9.5, 10.5, 11.0], 10.0)]


@pytest.fixture(scope="module")
def scan_driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("scan_driver") / "prefilter_scan_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "tests", "stub_pcl"), "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "prefilter_scan_driver.cpp"), "-o", exe,
                           os.path.join(ROOT, "delta_graph_slam_amd", "libdgs_reg.so"), "-Wl,-rpath," + os.path.join(ROOT, "delta_graph_slam_amd"),
                           "-Wl,-rpath,/opt/rocm/lib"])
    return exe


@pytest.mark.parametrize("name,stamps,scan", QUEUES, ids=[q[0] for q in QUEUES])
def test_imu_queue_python_cpp_and_transcription_agree(scan_driver, name, stamps, scan):
    from delta_graph_slam_amd.prefilter import ImuQueue
    # the literal transcription of :318-328 (behind the empty check of :295-297)
    lit = [(s, (s, 0.0, 0.0)) for s in stamps]
    want = S.select_imu(lit, scan) if lit else None
    # Python
    q = ImuQueue()
    for s in stamps:
        q.push(s, (s, 0.0, 0.0))
    got = q.select(scan)
    assert got == (None if want is None else want[1])
    assert [e[0] for e in q.queue] == [e[0] for e in lit] and len(q) == len(lit)
    # C++
    res = json.loads(subprocess.check_output([scan_driver, "select", repr(scan)] + [repr(s) for s in stamps]).decode().strip().splitlines()[-1])
    assert res["chosen"] == (None if want is None else want[0])
    assert res["left"] == [e[0] for e in lit]


def test_imu_queue_quirk_is_kept():
    """No message later than the scan: the last one is used and the queue is emptied, so the next scan is not deskewed."""
    from delta_graph_slam_amd.prefilter import ImuQueue
    q = ImuQueue()
    q.push(1.0, (0.1, 0.0, 0.0))
    q.push(2.0, (0.2, 0.0, 0.0))
    assert q.select(5.0) == (0.2, 0.0, 0.0) and len(q) == 0
    assert q.select(5.1) is None
    # a later message is chosen and stays at the front
    q.push(6.0, (0.3, 0.0, 0.0))
    q.push(7.0, (0.4, 0.0, 0.0))
    assert q.select(5.2) == (0.3, 0.0, 0.0) and [e[0] for e in q.queue] == [6.0, 7.0]


def _cloud(n, seed, scale=40.0):
    rng = np.random.default_rng(seed)
    c = np.ones((n, 4), np.float32)
    c[:, :3] = rng.normal(size=(n, 3)) * scale
    return c


@pytest.mark.parametrize("w", [(0.3, -0.8, 1.1), (50.0, -20.0, 35.0)], ids=["typical", "large"])
def test_restated_deskew_stays_within_float_ulps_of_the_exact_rotation(w):
    """Error of the float32 restatement against the float64 value of upstream's own product (deskew_exact: the rotation by the exact
    quaternion, pulled back by 1 / |q|² because delta_q.inverse() is not normalised), relative to |v|, in units of FLT_EPSILON.
    What can accumulate: the three quaternion components, the norm and the four quotients round once each, and _transformVector
    rounds 15 times on terms bounded by a small multiple of |v|; a few epsilons.  Measured on the CPU over 40,000 points and the
    three norm orders: 0.923 (about 1 rad/s), 1.842 (about 64 rad/s, |q|² up to 11).  The bound is 4: a margin of 2.2 over the
    larger figure."""
    c = _cloud(40000, 5)
    idx = np.arange(c.shape[0])
    exact = S.deskew_exact(c[:, :3], idx, c.shape[0], w)
    nv = np.linalg.norm(c[:, :3].astype(np.float64), axis=1)
    worst = 0.0
    for order in S.NORM_ORDERS:
        out = S.deskew(c, w, deskew_norm_order=order)
        err = np.linalg.norm(out[:, :3].astype(np.float64) - exact, axis=1) / nv / np.finfo(np.float32).eps
        worst = max(worst, float(err.max()))
        assert np.array_equal(out[:, 3], c[:, 3])
    print(f"deskew restatement against float64: {worst:.3f} FLT_EPSILON |v| at w = {w}")
    assert worst <= 4.0
    # upstream's product is the rotation pulled back towards v by 1 / |q|^2 (deskew_exact): it is a rotation to first order only
    rot = S.deskew_exact(c[:, :3], idx, c.shape[0], w, rotation_only=True)
    assert np.allclose(np.linalg.norm(rot, axis=1), nv, rtol=1e-12)
    half = S.SCAN_PERIOD * idx / c.shape[0] / 2.0 * np.linalg.norm(S.ang_v_of(w).astype(np.float64))
    pull = np.linalg.norm(exact - rot, axis=1)
    assert np.all(pull <= half * half / (1 + half * half) * np.linalg.norm(rot - c[:, :3], axis=1) * (1 + 1e-9) + 1e-12)
    print(f"upstream's deskew against the pure rotation: up to {float((pull / nv).max()):.3e} |v|")


def test_deskew_norm_orders_differ_on_a_chosen_input():
    """The switch is observable: with a large angular velocity the three associations of the four squares round differently."""
    w = (50.0, -20.0, 35.0)
    n = 4096
    q = [np.stack(S.quaternions(n, w, deskew_norm_order=o), 1) for o in S.NORM_ORDERS]
    c = _cloud(n, 6)
    out = [S.deskew(c, w, deskew_norm_order=o) for o in S.NORM_ORDERS]
    for a, b in ((0, 1), (0, 2), (1, 2)):
        assert not np.array_equal(q[a], q[b]), (a, b)
        assert not np.array_equal(out[a], out[b]), (a, b)
    # one input on which all three differ pairwise, found by search and pinned by index
    diff = [i for i in range(n) if len({q[o][i].tobytes() for o in S.NORM_ORDERS}) == 3]
    assert diff, "no index at which the three orders give three quaternions"
    print(f"norm orders: {len(diff)} of {n} indices give three different quaternions, first {diff[0]}")


def test_none_is_not_zero_angular_velocity():
    c = np.array([[-0.0, 1.0, -0.0, 5.0], [2.0, -0.0, 3.0, -7.0]], np.float32)
    nan = np.array([0x7fc12345], np.uint32).view(np.float32)[0]
    c = np.vstack([c, np.array([[nan, 1.0, 2.0, 3.0]], np.float32)])
    none = S.deskew(c, None)
    assert np.array_equal(none.view(np.uint32), c.view(np.uint32))
    zero = S.deskew(c, (0.0, 0.0, 0.0))
    assert np.array_equal(zero[:2], c[:2])                                   # same values ...
    assert not np.array_equal(zero[:2].view(np.uint32), c[:2].view(np.uint32))   # ... but -0.0f came out +0.0f
    assert not np.signbit(zero[0, 0]) and not np.signbit(zero[0, 2]) and not np.signbit(zero[1, 1])
    assert np.array_equal(zero[:, 3].view(np.uint32), c[:, 3].view(np.uint32))


def test_restated_transform_against_a_matrix_product():
    m, lidar = S.centered(S.base_link_matrix())
    assert m[0, 3] == 0.0 and m[1, 3] == 0.0 and np.array_equal(lidar, [0.0, 0.0, 1.7])
    c = _cloud(5000, 7)
    c[:, 3] = 0.25
    c[3, 0] = np.nan
    c[4, 1] = np.inf
    c[5, 2] = -np.inf
    out = S.transform(c, m)
    fin = np.all(np.isfinite(c[:, :3]), 1)
    with np.errstate(invalid="ignore"):
        ref = c[:, :3].astype(np.float64) @ m[:3, :3].T + m[:3, 3]
    assert np.max(np.abs(out[fin, :3] - ref[fin])) <= 2e-5                    # 100 m coordinates: half an ulp is 3.8e-6 per term
    assert np.all(out[fin, 3] == 1.0)
    assert np.array_equal(out[~fin].view(np.uint32), c[~fin].view(np.uint32))  # copied whole
    keep_w = S.transform(c, m, transform_sets_w=0)
    assert np.array_equal(keep_w[:, 3], c[:, 3]) and np.array_equal(keep_w[:, :3].view(np.uint32), out[:, :3].view(np.uint32))


def test_cpp_scan_driver_builds_against_the_stubs(scan_driver):
    res = json.loads(subprocess.check_output([scan_driver, "select", "1.5", "1.0", "2.0", "3.0"]).decode().strip().splitlines()[-1])
    assert res == {"chosen": 2.0, "left": [2.0, 3.0]}
