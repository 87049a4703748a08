"""The building cloud stage without a device: the two restatements of interpolate / buildPointCloud / getCloud against each other
(tests/building_cloud_reference.py), the measured facts about the table of sample positions, the conditions the GPU tests rely on,
the new symbols, struct layout and defaults, the argument checks that need no device, the adapter header against tests/stub_pcl, and
the host-only helpers in a stand-alone program built under AddressSanitizer and UndefinedBehaviorSanitizer.

Tolerance: none.  Every operation of the stage is one IEEE float32 add, subtract, multiply, divide or square root; bit patterns are
compared, NaN positions must match and NaN payloads are free.  The one exception is building_transform's rotation entries, which come
from the host's atan2f / cosf / sinf: the C++ helper and numpy may use different libm routines, each within one unit in the last
place of a value of magnitude <= 1, so those four entries are compared to 2^-23 and the two translations exactly."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import building_cloud_cases as K
import building_cloud_reference as R

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = list(K.named_cases())


# ---- the restatements agree -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_vectorised_and_scalar_restatements_agree(name):
    c = K.named_cases()[name]
    pts, off = K.reference(name, c)
    spts, soff = R.clouds_scalar(c["items"], c["transforms"], c["params"])
    assert np.array_equal(off, soff) and R.same_bits(pts, spts)


def test_restatements_agree_on_random_lines():
    lines = K.random_lines(200)
    assert np.all(lines[:, :, 2] != 0.0)
    for order in (0, 1, 2):
        p = dict(sqnorm_order=order)
        items = [lines[:70], lines[70:71], lines[71:]]
        pts, off = R.clouds(items, [None, K.rigid(40.0, 3.0, -2.0), None], p)
        spts, soff = R.clouds_scalar(items, [None, K.rigid(40.0, 3.0, -2.0), None], p)
        assert np.array_equal(off, soff) and R.same_bits(pts, spts) and pts.shape[0] > 200 * 1000


def test_restatements_refuse_the_same_lines():
    for make, params in ((K.infinite_endpoint, {}), (lambda: K.past_the_table()[1:], dict(max_points_per_line=64))):
        c, where = make()
        for fn in (R.clouds, R.clouds_scalar):
            with pytest.raises(R.TooLong) as e:
                fn(c["items"], c["transforms"], dict(c["params"], **params))
            assert (e.value.item, e.value.line) == where


# ---- measured facts about the table -----------------------------------------------------------------------------------------------
def test_table_facts():
    t = R.step_table(1 << 20)
    assert t.size == 1 << 20 and np.all(np.diff(t) > 0)                      # strictly increasing over 2^20 entries
    k = np.arange(64)
    assert int(np.nonzero(t[:64] != (k * 0.02).astype(F))[0][0]) == 5       # the running sum leaves float32(k * 0.02) at k = 5
    count = lambda length: int(np.searchsorted(t, F(length), side="right"))
    assert count(20.0) == 1000 and count(1000.0) == 49983 and count(100.0) == 5001
    # an independent running sum
    i, want = F(0), []
    for _ in range(3000):
        want.append(i)
        i = F(i + R.STEP)
    assert np.array_equal(R.bits(t[:3000]), R.bits(np.array(want, F)))


# ---- conditions of the GPU tests ----------------------------------------------------------------------------------------------------
def test_boundary_lengths_hit_the_comparison():
    t = R.step_table(K.TILE + 3)
    for k in K.BOUNDARY_KS:
        v = t[k]
        assert F(np.sqrt(F(v * v))) == v                                     # norm((v, 0, 0)) is v itself: `i_k <= norm` is an equality
        c, want = K.boundary(k)
        _, off = K.reference(f"boundary_{k}", c)
        assert np.diff(off).tolist() == want
    assert K.TILE % 256 == 0 and K.TILE + 1 in K.BOUNDARY_KS


def test_many_items_cases_are_what_the_gpu_tests_assume():
    for n in (1023, 1024, 1025, 2049):
        c = K.many_items(n)
        sizes = [i.shape[0] for i in c["items"]]
        assert sum(sizes) == n and sizes[0] == 0 and sizes[-1] == 0 and 0 in sizes[1:-1] and len(set(sizes)) > 10
        a, dn, norm = R.line_records(np.concatenate(c["items"]))
        counts = np.searchsorted(R.step_table(8), norm, side="right")
        assert set(counts.tolist()) == {1, 2, 3}
        pts, off = K.reference(f"many_items_{n}", c)
        assert off[-1] == counts.sum() == pts.shape[0] > K.TILE              # more than one workgroup of the fill kernel
    assert K.reference("no_items")[0].shape == (0, 4) and K.reference("no_items")[1].tolist() == [0]
    pts, off = K.reference("one_zero_length")
    assert off.tolist() == [0, 1] and pts.tolist() == [[3.25, -7.5, 0.0, 1.0]]
    pts, off = K.reference("zero_length_unguarded")
    assert off.tolist() == [0, 1] and np.isnan(pts[0, 0]) and np.isnan(pts[0, 1]) and pts[0, 2:].tolist() == [0.0, 1.0]


@pytest.mark.parametrize("shift", [-1, 0, 1])
def test_owner_search_cases_put_the_long_line_at_a_tile_start(shift):
    pts, off = K.reference(f"owner_{shift}")
    c = K.owner_search(shift)
    first = 700 + (K.TILE + shift - 700)                                     # one point per line in front of it
    assert off.tolist() == [0, 700, first + 5001 + 10, first + 5001 + 300]
    assert first - K.TILE == shift and pts[first].tolist() == [3.0, 4.0, 0.0, 1.0] and pts[first - 1, 0] == K.TILE + shift - 1
    assert (first + 5001) % K.TILE != 0 and c["items"][1].shape[0] == K.TILE + shift - 700 + 11


def test_arithmetic_cases():
    pts, off = K.reference("arithmetic")
    assert np.all(pts[:, 2] == 0.0) and np.all(pts[:, 3] == 1.0) and np.all(np.isfinite(pts))
    t = R.step_table(2048)
    count = lambda length: int(np.searchsorted(t, F(length), side="right"))
    norms = R.line_records(K.arithmetic()["items"][2])[2]
    assert norms[0] == 13.0 and norms[1] == 20.0 and 8.5 < norms[2] < 8.51   # the norm counts z: (3, 4, -12) is 13 m long, not 5
    assert np.diff(off)[2] == count(13.0) + 1000 + count(norms[2])
    vertical = pts[off[2] + count(13.0):off[2] + count(13.0) + 1000]
    assert np.all(vertical[:, :2] == 0.0)                                    # a vertical line: 1,000 copies of (a.x, a.y, 0)
    first = off[4] - count(2.0)
    assert np.signbit(pts[first, 0]) and pts[first, 1] == 1.0 and pts[first + 1, 0] < 0      # the last line's first point is (-0.0, 1)
    # the three association orders on the committed line: 0 and 2 are the same sum when the fourth term is 0, 1 differs
    n = [R.line_records(K.SQNORM_LINE[None], o)[2][0] for o in (0, 1, 2)]
    assert n[0] == n[2] != n[1]
    sizes = [K.reference(f"sqnorm_{o}")[1][-1] for o in (0, 1, 2)]
    assert sizes == [2100, 2099, 2100]
    assert not R.same_bits(K.reference("sqnorm_0")[0][:2099], K.reference("sqnorm_1")[0])      # dn differs as well


def test_transform_cases():
    none, _ = K.reference("transform_none_0")
    for order in (0, 1):
        ident, off = K.reference(f"transform_identity_{order}")
        assert np.signbit(none[off[4], 0]) and not np.signbit(ident[off[4], 0])         # -0.0 comes out +0.0
        assert np.array_equal(ident[:, 1], none[:, 1]) and np.all(ident[:, 3] == 1.0)
        per, _ = K.reference(f"transform_per_item_{order}")
        assert R.same_bits(per[off[1]:off[2]], none[off[1]:off[2]])                     # an item without a matrix, between two with one
        assert np.all(per[off[3]:off[4], 2] > 0.0) and np.all(per[:off[1], 2] == 0.0)   # the skewed matrix lifts z off the plane
        nan, _ = K.reference(f"transform_nan_{order}")
        assert np.all(np.isnan(nan[:off[1], 1])) and np.all(np.isfinite(nan[:off[1], 0]))   # the NaN entry sits in row y
        assert np.all(np.isnan(nan[off[3]:off[4], 0])) and np.all(np.isfinite(nan[off[3]:off[4], 1]))   # 0 * inf in row x
    a, b = K.reference("transform_shared_0")[0], K.reference("transform_shared_1")[0]
    assert not R.same_bits(a, b) and np.max(np.abs(a - b)) < 1e-4                       # the two orders differ in last bits only


def test_handle_reuse_cases():
    assert K.reference("short_call")[0].shape[0] < 4096 < K.reference("growing_call")[0].shape[0]
    a, dn, norm = R.line_records(np.concatenate(K.growing_call()["items"]))
    assert norm.max() > R.step_table(4096)[-1]


def test_building_transform():
    from delta_graph_slam_amd.building_cloud import building_transform
    rng = np.random.default_rng(4)

    def iso(deg, x, y):
        t = np.deg2rad(deg)
        return np.array([[np.cos(t), -np.sin(t), x], [np.sin(t), np.cos(t), y], [0, 0, 1.0]])

    for _ in range(20):
        pose, est = iso(rng.uniform(-180, 180), *rng.uniform(-100, 100, 2)), iso(rng.uniform(-180, 180), *rng.uniform(-100, 100, 2))
        got, want = building_transform(pose, est), R.building_transform(pose, est)
        assert got.dtype == F and np.array_equal(R.bits(got), R.bits(want))
        # building.cpp:11-14 in matrix form, in double
        full = np.linalg.inv(pose) @ est
        full[:2, 2] += pose[:2, 2] - full[:2, :2] @ pose[:2, 2]
        assert np.max(np.abs(got[:2, :2] - full[:2, :2])) < 1e-6 and np.max(np.abs(got[:2, 3] - full[:2, 2])) < 1e-4
    same = building_transform(iso(33.0, 5.0, 6.0), iso(33.0, 5.0, 6.0))
    assert np.max(np.abs(same - np.eye(4))) < 1e-5


# ---- symbols, layout, defaults ---------------------------------------------------------------------------------------------------------
NEW_SYMBOLS = ["dgs_building_cloud_params_init", "dgs_building_cloud_generate", "dgs_building_cloud_get", "dgs_building_cloud_get_counts"]


def test_new_symbols_are_declared_exported_and_bound():
    import delta_graph_slam_amd
    from delta_graph_slam_amd import _lib as L
    lib = L.load()
    header = open(os.path.join(ROOT, "include", "dgs_reg.h")).read()
    for name in NEW_SYMBOLS:
        assert name + "(" in header and name in L.SYMBOLS and hasattr(lib, name) and getattr(lib, name).argtypes
    assert lib.dgs_abi_version() == 5
    assert "BuildingClouds" in delta_graph_slam_amd.__all__ and delta_graph_slam_amd.BuildingClouds.__name__ == "BuildingClouds"


def test_struct_layout_and_defaults_match_the_header():
    from delta_graph_slam_amd import _lib as L
    fields = ["struct_size", "sample_step", "sqnorm_order", "normalized_guard", "transform_order", "max_points_per_line", "reserved"]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "dgs_reg.h"\nint main(void) {\n  printf("%zu", sizeof(dgs_building_cloud_params));\n'
    src += "".join(f'  printf(" %zu", offsetof(dgs_building_cloud_params, {f}));\n' for f in fields)
    src += '  printf(" %d\\n", (int)DGS_BC_TILE);\n  return 0;\n}\n'
    with tempfile.TemporaryDirectory() as d:
        cfile, exe = os.path.join(d, "t.c"), os.path.join(d, "t")
        open(cfile, "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), cfile, "-o", exe])   # the header is plain C
        vals = [int(x) for x in subprocess.check_output([exe]).split()]
    P = L.BuildingCloudParams
    assert [f for f, _ in P._fields_] == fields
    assert vals == [C.sizeof(P)] + [getattr(P, f).offset for f in fields] + [K.TILE]
    p = P()
    assert L.load().dgs_building_cloud_params_init(C.byref(p)) == 0
    assert p.struct_size == C.sizeof(P) and F(p.sample_step) == F(0.02) and p.sqnorm_order == L.PF_NORM_ORDER["PAIRS_XY_ZW"]
    assert p.normalized_guard == 1 and p.transform_order == 0 and p.max_points_per_line == 1 << 20 and p.reserved == 0
    assert L.load().dgs_building_cloud_params_init(None) == 1


def test_invalid_arguments_are_rejected_without_touching_a_device():
    from delta_graph_slam_amd import _lib as L
    lib = L.load()
    off = np.zeros(1, np.int64)
    n = C.c_int64(0)

    def call(h, **over):
        p = L.BuildingCloudParams()
        assert lib.dgs_building_cloud_params_init(C.byref(p)) == 0
        for k, v in over.items():
            setattr(p, k, v)
        return lib.dgs_building_cloud_generate(h, C.byref(p), None, off.ctypes.data, 0, None, None, C.byref(n))

    assert call(None) == 1 and b"handle" in lib.dgs_last_error(None)                    # a NULL handle
    for over in (dict(struct_size=12), dict(sqnorm_order=3), dict(sqnorm_order=-1), dict(transform_order=2), dict(transform_order=-1),
                 dict(sample_step=0.0), dict(sample_step=-0.02), dict(sample_step=float("nan")), dict(sample_step=float("inf")),
                 dict(max_points_per_line=0)):
        assert call(None, **over) == 1, over
        assert lib.dgs_last_error(None) != b""
    assert lib.dgs_building_cloud_generate(None, None, None, off.ctypes.data, 0, None, None, C.byref(n)) == 1
    assert lib.dgs_building_cloud_get(None, None, 0, 0, None, C.byref(n), None) == 1
    assert lib.dgs_building_cloud_get_counts(None, None) == 1


# ---- C++ ---------------------------------------------------------------------------------------------------------------------------------
def test_adapter_header_and_driver_compile_against_the_stubs(tmp_path):
    exe = str(tmp_path / "building_cloud_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "tests", "stub_pcl"), "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "building_cloud_driver.cpp"), "-o", exe,
                           os.path.join(ROOT, "delta_graph_slam_amd", "libdgs_reg.so"), "-Wl,-rpath," + os.path.join(ROOT, "delta_graph_slam_amd"),
                           "-Wl,-rpath,/opt/rocm/lib"])
    # the matrix helper needs no device
    from delta_graph_slam_amd.building_cloud import building_transform
    t = np.deg2rad(25.0)
    pose = np.array([[np.cos(t), -np.sin(t), 40.0], [np.sin(t), np.cos(t), -12.0], [0, 0, 1.0]])
    u = np.deg2rad(27.5)
    est = np.array([[np.cos(u), -np.sin(u), 40.5], [np.sin(u), np.cos(u), -11.0], [0, 0, 1.0]])
    ip, op = str(tmp_path / "m.bin"), str(tmp_path / "o.bin")
    np.concatenate([pose.reshape(-1), est.reshape(-1)]).tofile(ip)
    subprocess.check_call([exe, "matrix", ip, op], timeout=60)
    got = np.fromfile(op, F).reshape(4, 4).T                                          # column-major
    want = building_transform(pose, est)
    assert np.array_equal(R.bits(got[:, 2:]), R.bits(want[:, 2:])) and np.array_equal(R.bits(got[2:]), R.bits(want[2:]))
    assert np.max(np.abs(got[:2, :2] - want[:2, :2])) <= 2.0 ** -23                   # libm's atan2f / cosf / sinf: see the module docstring


def test_host_helpers_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    exe = str(tmp_path / "building_cloud_host_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "tests", "stub_pcl"), "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "delta_graph_slam_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "building_cloud_host_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, timeout=120)
    assert out.returncode == 0 and out.stdout.decode().strip() == "ok", (out.stdout.decode(), out.stderr.decode())
