"""The map cloud without a GPU: the two restatements of MapCloudGenerator::generate (tests/map_cloud_reference.py: the closed form the
device is compared with, and a literal pointer octree) agree bit for bit and in order on small clouds chosen to exercise the rules
of DESIGN.md §6d; and the new entry points of the C ABI exist, mirror their struct and reject bad arguments without a device."""
import ctypes as C

import numpy as np
import pytest

import map_cloud_edge_cases as E
import map_cloud_reference as R

CASES = E.edge_cases()
SWITCHES = E.switch_cases()


def _same_grid(a, b):
    return a["depth"] == b["depth"] and a["growths"] == b["growths"] and np.array_equal(a["min"], b["min"]) and np.array_equal(a["max"], b["max"])


@pytest.mark.parametrize("name", sorted(CASES))
def test_closed_form_equals_the_pointer_octree(name):
    kfs, res = CASES[name]
    a, ga = R.generate(kfs, res, with_grid=True)
    b, gb = R.generate_literal(kfs, res, with_grid=True)
    assert a.dtype == np.float32 and a.shape == b.shape and a.tobytes() == b.tobytes()
    assert _same_grid(ga, gb)
    if a.shape[0]:
        assert np.all(a[:, 3] == 1.0)


@pytest.mark.parametrize("name", sorted(SWITCHES))
def test_each_switch_changes_the_map_on_its_input(name):
    kfs, res = SWITCHES[name]
    out = {}
    for v in (0, 1):
        a = R.generate(kfs, res, {name: v})
        if name != "key_at_insertion" or v:      # keys under the final min are no tree's: the closed form alone states them
            assert a.tobytes() == R.generate_literal(kfs, res, {name: v}).tobytes()
        out[v] = a
    assert out[0].tobytes() != out[1].tobytes()


def test_cases_exercise_the_rules_they_are_named_for():
    # a lower violation on one axis and an upper violation on another in one growth event
    box = R.Box(1.0, None)
    box.adopt(np.float32([0, 0, 0]))
    lower, upper = box.violations(np.float32([-3, 5, 0]))
    assert lower == [True, False, False] and upper == [False, True, False]
    # exactly on max violates, exactly on min does not
    assert box.mn == [-1.0, -1.0, -1.0] and box.mx == [1.0, 1.0, 1.0] and box.depth == 1
    assert box.violations(np.float32([1, 0, 0])) == ([False] * 3, [True, False, False])
    assert box.violations(np.float32([-1, -1, -1])) == ([False] * 3, [False] * 3)
    # after a growth max = min + (side - FLT_EPSILON), and min moved on the axes without an upper violation
    assert box.adopt(np.float32([1, 0, 0])) == [[False, True, True]]
    assert box.mn == [-1.0, -3.0, -3.0] and box.mx == [3.0 - R.FLT_EPSILON, 1.0 - R.FLT_EPSILON, 1.0 - R.FLT_EPSILON] and box.depth == 2
    # the same points in two orders: other origins, other maps
    (a, ga), (b, gb) = (R.generate(*CASES[k], with_grid=True) for k in ("order_a", "order_b"))
    assert sorted(map(tuple, CASES["order_a"][0][0][0])) == sorted(map(tuple, CASES["order_b"][0][0][0]))
    assert not np.array_equal(ga["min"], gb["min"]) and a.tobytes() != b.tobytes()
    frac = lambda m: np.mod(m, 1.0)
    assert not np.array_equal(frac(ga["min"]), frac(gb["min"]))       # not just another root: another lattice
    # flat snapshots: z = 0 in, one layer of voxels out
    flat = R.generate(*CASES["flat_keyframes"])
    assert all(np.all(c[:, 2] == 0) for c, _ in CASES["flat_keyframes"][0]) and np.unique(flat[:, 2]).size == 1
    # an empty keyframe changes nothing; non-finite points are skipped; duplicates fall into one voxel
    assert R.generate(*CASES["empty_keyframe_in_the_middle"]).tobytes() == R.generate(*CASES["without_the_empty_keyframe"]).tobytes()
    assert R.generate(*CASES["only_non_finite_points"]).shape == (0, 4)
    assert R.generate(*CASES["single_point"]).shape == (1, 4)
    kfs, res = CASES["nan_and_inf_points"]
    cat = R.concatenate(kfs)
    fin = np.isfinite(cat[:, :3]).all(1)
    assert 0 < (~fin).sum() and not fin[0]
    assert R.octree_centres(cat, res).tobytes() == R.octree_centres(cat[fin], res).tobytes()
    assert R.generate([], 0.05) is None


def test_concatenation_is_the_result_without_a_resolution():
    kfs, _ = CASES["nan_and_inf_points"]
    for res in (0.0, -1.0):
        out = R.generate(kfs, res)
        assert out.shape[0] == sum(c.shape[0] for c, _ in kfs) and np.all(out[:, 3] == 1.0)
    # ((m0 x + m1 y) + m2 z) + m3 in float, every step rounded
    c, pose = kfs[1]
    m = pose.astype(np.float32)
    i = 17
    x, y, z = c[i, :3]
    want = np.float32(np.float32(np.float32(m[1, 0] * x) + np.float32(m[1, 1] * y)) + np.float32(m[1, 2] * z)) + m[1, 3]
    assert R.concatenate([kfs[1]])[i, 1] == want


def test_a_span_of_more_than_2_to_the_21_voxels_is_too_large():
    pts = E.xyz1([(0, 0, 0), (3.0e4, 0, 0)])
    with pytest.raises(R.GridTooLarge):
        R.octree_centres(pts, 0.01)             # 3e6 voxels: depth 22
    assert R.replay(E.xyz1([(0, 0, 0), (2.0e4, 0, 0)]), 0.01)[0].depth == 21


# ---------------------------------------------------------------------------------------------------------------- ABI
def test_map_cloud_symbols_exist_and_the_struct_matches():
    from delta_graph_slam_amd import _lib as L
    lib = L.load()
    for name in ("dgs_map_cloud_params_init", "dgs_map_cloud_generate", "dgs_map_cloud_generate_clouds", "dgs_map_cloud_get", "dgs_map_cloud_get_grid"):
        assert hasattr(lib, name) and name in L.SYMBOLS
    p = L.MapCloudParams()
    assert lib.dgs_map_cloud_params_init(C.byref(p)) == 0
    assert p.struct_size == C.sizeof(L.MapCloudParams) == 40
    assert (p.first_box_oversize, p.grow_shift_without_upper, p.max_minus_epsilon, p.child_index_x_msb, p.key_at_insertion) == \
        (R.FIRST_BOX_OVERSIZE, R.GROW_SHIFT_WITHOUT_UPPER, R.MAX_MINUS_EPSILON, R.CHILD_INDEX_X_MSB, R.KEY_AT_INSERTION)
    assert p.dedup_method == L.MAP_DEDUP["AUTO"] and p.hash_slots == 0
    assert lib.dgs_map_cloud_params_init(None) == 1
    assert lib.dgs_abi_version() == 5


def test_map_cloud_rejects_bad_arguments_without_a_device():
    from delta_graph_slam_amd import _lib as L
    lib = L.load()
    p = L.MapCloudParams()
    lib.dgs_map_cloud_params_init(C.byref(p))
    n = C.c_int64(-7)
    bad = 1   # DGS_ERR_INVALID_ARGUMENT
    fake = C.c_void_p(0x1000)   # a handle that is never followed: every call below must return before it touches it
    poses = (C.c_double * 16)()
    sizes = (C.c_int64 * 1)(4)
    cloud = (C.c_float * 16)()
    ptrs = (C.c_void_p * 1)(C.addressof(cloud))
    assert lib.dgs_map_cloud_generate(None, C.byref(p), 0, None, None, 0, None, 0.05, C.byref(n)) == bad
    assert lib.dgs_map_cloud_generate(fake, None, 0, None, None, 0, None, 0.05, C.byref(n)) == bad
    assert lib.dgs_map_cloud_generate(fake, C.byref(p), 0, None, None, 0, None, 0.05, None) == bad
    assert lib.dgs_map_cloud_generate(fake, C.byref(p), -1, ptrs, sizes, 0, poses, 0.05, C.byref(n)) == bad
    assert lib.dgs_map_cloud_generate(fake, C.byref(p), 1, None, sizes, 0, poses, 0.05, C.byref(n)) == bad
    assert lib.dgs_map_cloud_generate(fake, C.byref(p), 1, ptrs, None, 0, poses, 0.05, C.byref(n)) == bad
    assert lib.dgs_map_cloud_generate(fake, C.byref(p), 1, ptrs, sizes, 0, None, 0.05, C.byref(n)) == bad
    assert lib.dgs_map_cloud_generate(fake, C.byref(p), 1, ptrs, sizes, 0, poses, float("nan"), C.byref(n)) == bad
    assert lib.dgs_map_cloud_generate(fake, C.byref(p), 1, ptrs, (C.c_int64 * 1)(-1), 0, poses, 0.05, C.byref(n)) == bad
    assert lib.dgs_map_cloud_generate(fake, C.byref(p), 1, ptrs, (C.c_int64 * 1)(2 ** 31), 0, poses, 0.05, C.byref(n)) == bad
    assert lib.dgs_map_cloud_generate(fake, C.byref(p), 1, (C.c_void_p * 1)(None), sizes, 0, poses, 0.05, C.byref(n)) == bad
    q = L.MapCloudParams()
    lib.dgs_map_cloud_params_init(C.byref(q))
    q.struct_size = 12
    assert lib.dgs_map_cloud_generate(fake, C.byref(q), 1, ptrs, sizes, 0, poses, 0.05, C.byref(n)) == bad
    lib.dgs_map_cloud_params_init(C.byref(q))
    q.dedup_method = 3
    assert lib.dgs_map_cloud_generate(fake, C.byref(q), 1, ptrs, sizes, 0, poses, 0.05, C.byref(n)) == bad
    lib.dgs_map_cloud_params_init(C.byref(q))
    q.hash_slots = -1
    assert lib.dgs_map_cloud_generate(fake, C.byref(q), 1, ptrs, sizes, 0, poses, 0.05, C.byref(n)) == bad
    assert lib.dgs_map_cloud_generate_clouds(None, C.byref(p), 0, None, None, 0.05, C.byref(n)) == bad
    assert lib.dgs_map_cloud_generate_clouds(fake, C.byref(p), -1, None, None, 0.05, C.byref(n)) == bad
    assert lib.dgs_map_cloud_generate_clouds(fake, C.byref(p), 1, None, poses, 0.05, C.byref(n)) == bad
    assert lib.dgs_map_cloud_generate_clouds(fake, C.byref(p), 1, (C.c_void_p * 1)(None), poses, 0.05, C.byref(n)) == bad
    assert lib.dgs_map_cloud_generate_clouds(fake, C.byref(p), 1, ptrs, None, 0.05, C.byref(n)) == bad
    assert lib.dgs_map_cloud_get(None, None, 0, 0, C.byref(n)) == bad
    assert lib.dgs_map_cloud_get(fake, None, 0, 0, None) == bad
    assert lib.dgs_map_cloud_get(fake, None, -1, 0, C.byref(n)) == bad
    assert lib.dgs_map_cloud_get(fake, None, 4, 0, C.byref(n)) == bad
    assert lib.dgs_map_cloud_get_grid(None, None, None, None, None) == bad
    assert n.value == -7


def test_python_layer_is_exported_and_snapshot_pose_is_the_float_round_trip():
    import delta_graph_slam_amd
    from delta_graph_slam_amd.map_cloud import MapCloudGenerator, snapshot_pose
    from delta_graph_slam_amd.transforms import transform2Dto3D
    assert delta_graph_slam_amd.MapCloudGenerator is MapCloudGenerator
    est = np.array([[np.cos(0.3), -np.sin(0.3), 12.3456789], [np.sin(0.3), np.cos(0.3), -7.654321], [0, 0, 1]], np.float64)
    pose = snapshot_pose(est)
    assert pose.dtype == np.float64 and pose.shape == (4, 4)
    assert np.array_equal(pose, transform2Dto3D(est.astype(np.float32)).astype(np.float64))
    assert np.array_equal(pose, pose.astype(np.float32).astype(np.float64))     # every entry is a float
