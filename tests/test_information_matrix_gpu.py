"""calc_fitness_score over a batch of edges between resident clouds (dgs_calc_fitness_score_batch_clouds), the batched index build
(dgs_cloud_build_indices) and the layers above them, on the device.

Scene (tests/information_matrix_reference.py): six 16-beam street scans 2 m apart (4,002 to 4,024 points: index depth 3), sub-clouds of
1 .. 513 points (depths 1 to 3), two scans concatenated (8,026 points: depth 4).  The CPU oracle's answers are computed once per process.
Tolerance: |score - oracle| <= 1e-12 score, `used` exact (R.TOL: both sides add the same float distances in double, in another order)."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import information_matrix_reference as R

pytestmark = pytest.mark.gpu
DBL_MAX = R.DBL_MAX


@pytest.fixture(scope="module")
def reg():
    from delta_graph_slam_amd.registration import Registration
    return Registration("FAST_GICP")   # any handle: only its NN machinery is used; a GICP handle builds nothing at setInputTarget


def device_clouds(reg, names=None):
    """fresh DeviceClouds (no index yet) of the scene's clouds, by name"""
    clouds, _ = R.scene()
    return {n: reg.make_cloud(clouds[n]) for n in (names or clouds)}


def run(reg, dc, edges, max_range=DBL_MAX):
    return reg.calc_fitness_score_batch([dc[a] for a, _, _ in edges], [dc[b] for _, b, _ in edges], [T for _, _, T in edges], max_range, return_used=True)


def check_against(scores, used, ref):
    for e, ((s, u), (rs, ru)) in enumerate(zip(zip(scores, used), ref)):
        print("edge", e, "score", repr(float(s)), "oracle", repr(rs), "used", int(u), "oracle", ru)
    for e, ((s, u), (rs, ru)) in enumerate(zip(zip(scores, used), ref)):
        assert int(u) == ru, (e, u, ru)
        if rs == DBL_MAX:
            assert s == DBL_MAX, (e, s)
        else:
            assert abs(s - rs) <= R.TOL * rs, (e, s, rs)


def same_bits(a, b):
    return np.array_equal(np.asarray(a[0], np.float64).view(np.int64), np.asarray(b[0], np.float64).view(np.int64)) and np.array_equal(a[1], b[1])


@pytest.fixture(scope="module")
def warm(reg):
    """the scene's clouds on the device; their indices get built by whichever test walks them first and are kept"""
    return device_clouds(reg)


# ---------------------------------------------------------------------------------------------- against the oracle
@pytest.mark.parametrize("max_range", [DBL_MAX, 0.05])
def test_scores_equal_the_oracle(reg, warm, max_range):
    scores, used = run(reg, warm, R.main_edges(), max_range)
    check_against(scores, used, R.oracle_edges("main", max_range))


@pytest.mark.parametrize("max_range", [1e-7, -1.0])
def test_dbl_max_when_no_point_qualifies(reg, warm, max_range):
    edges = [e for k, e in enumerate(R.main_edges()) if k != R.SELF_EDGE or max_range < 0]
    scores, used = run(reg, warm, edges, max_range)
    assert np.all(scores == DBL_MAX) and np.all(used == 0)


def test_empty_clouds_and_the_self_edge(reg, warm):
    edges = [("empty", "k1", np.eye(4)), ("k1", "empty", np.eye(4)), ("empty", "empty", np.eye(4)), ("k2", "k2", np.eye(4)), ("sub9", "sub9", np.eye(4))]
    scores, used = run(reg, warm, edges)
    assert list(scores[:3]) == [DBL_MAX] * 3 and list(used[:3]) == [0, 0, 0]
    assert scores[3] == 0.0 and used[3] == len(warm["k2"]) and scores[4] == 0.0 and used[4] == 9
    # identity may also be given as NULL
    s2 = reg.calc_fitness_score_batch([warm["k2"], warm["k1"]], [warm["k2"], warm["k0"]], None, return_used=True)
    s3 = reg.calc_fitness_score_batch([warm["k2"], warm["k1"]], [warm["k2"], warm["k0"]], [np.eye(4)] * 2, return_used=True)
    assert s2[0][0] == 0.0 and same_bits(s2, s3)
    # an all-empty batch launches nothing
    s, u = run(reg, warm, edges[:3])
    assert list(s) == [DBL_MAX] * 3 and reg.fitness_batch_counts()["launches"] == 0 and reg.fitness_batch_counts()["rows"] == 0


def test_cloud2_size_edges_against_every_index_depth(reg, warm):
    scores, used = run(reg, warm, R.size_edges())
    check_against(scores, used, R.oracle_edges("size", DBL_MAX))


def test_non_finite_points_are_not_counted(reg, warm):
    """a NaN point and an infinite point in cloud2: counted by neither dgs_calc_fitness_score nor the batch; the oracle sees the finite ones"""
    from oracle import oracle as orc
    clouds, _ = R.scene()
    nf = clouds["nonfinite"]
    finite = nf[np.isfinite(nf[:, :3]).all(1)]
    T = R.relpose(0, 1)
    for t in R.DEPTH_TARGETS:
        s, u = run(reg, warm, [(t, "nonfinite", T)])
        single = reg.calc_fitness_score(clouds[t], nf, T.astype(np.float32))
        rs, ru, _ = orc.fitness_score(clouds[t], finite, T.astype(np.float32))
        print(t, "batch", repr(float(s[0])), int(u[0]), "single", repr(single), "oracle", repr(rs), ru)
        assert u[0] == ru == nf.shape[0] - 2
        assert abs(s[0] - rs) <= R.TOL * rs and abs(s[0] - single) <= R.TOL * single


# ---------------------------------------------------------------------------------------------- batch independence
def test_an_edge_does_not_depend_on_its_batch(reg, warm):
    edges = list(R.main_edges()) + list(R.size_edges()) + [("k0", "nonfinite", R.relpose(0, 1))]
    for max_range in (DBL_MAX, 0.05):
        full = run(reg, warm, edges, max_range)
        perm = np.random.default_rng(5).permutation(len(edges))
        shuffled = run(reg, warm, [edges[k] for k in perm], max_range)
        assert same_bits((full[0][perm], full[1][perm]), shuffled)
        for k, e in enumerate(edges):
            one = run(reg, warm, [e], max_range)
            assert same_bits((full[0][k:k + 1], full[1][k:k + 1]), one), (k, e[:2])


def test_three_hundred_edges_over_the_tiny_clouds(reg, warm):
    clouds, _ = R.scene()
    tiny = [n for n in clouds if n.startswith(("sub", "e")) and n != "empty"]
    rng = np.random.default_rng(11)
    edges = [(tiny[a], tiny[b], R.relpose(0, 1) if k % 2 else np.eye(4)) for k, (a, b) in enumerate(rng.integers(0, len(tiny), (300, 2)))]
    s, u = run(reg, warm, edges)
    assert reg.fitness_batch_counts()["edges"] == 300 and reg.fitness_batch_counts()["host_waits"] == 1
    seen = {}
    for k, e in enumerate(edges):
        key = (e[0], e[1], k % 2)
        if key not in seen:
            seen[key] = run(reg, warm, [e])
        assert same_bits((s[k:k + 1], u[k:k + 1]), seen[key]), (k, key)
    assert len(seen) > 100


def test_a_table_that_outgrows_its_pinned_block_between_calls():
    """One edge, then 64 edges between clouds of at most 64 points -- 64 entries of 128 bytes, more than the bytes + bytes / 4 + 4 KiB
    the first call left the pinned block with -- then the one edge again, all on one handle: scores, used counts and the call's counts
    are those of a fresh handle"""
    from delta_graph_slam_amd.registration import Registration
    clouds, _ = R.scene()
    T = R.relpose(0, 1)

    def call(r, pairs):
        c1 = [r.make_cloud(clouds["k0"][:a]) for a, _ in pairs]   # cold clouds: the call builds their indices
        c2 = [r.make_cloud(clouds["k1"][:b]) for _, b in pairs]
        return r.calc_fitness_score_batch(c1, c2, [T] * len(pairs), DBL_MAX, return_used=True), r.fitness_batch_counts()

    one, many = [(300, 200)], [(1 + (5 * i) % 64, 1 + (11 * i) % 64) for i in range(64)]
    used = Registration("FAST_GICP")
    for pairs in (one, many, one):
        fresh = Registration("FAST_GICP")
        (a, ca), (b, cb) = call(used, pairs), call(fresh, pairs)
        assert same_bits(a, b) and ca == cb, (len(pairs), ca, cb)
        assert ca["edges"] == len(pairs) and ca["indices_built"] == len(pairs) and ca["host_waits"] == 1 and a[1].sum() > 0
        fresh.close()
    used.close()


# ---------------------------------------------------------------------------------------------- cold equals warm
def test_cold_equals_warm(reg):
    edges = list(R.main_edges()) + list(R.size_edges())
    targets = sorted({e[0] for e in edges})
    cold = device_clouds(reg)
    a = run(reg, cold, edges)                       # the call builds every index itself
    assert reg.fitness_batch_counts()["indices_built"] == len(targets)
    again = run(reg, cold, edges)
    assert reg.fitness_batch_counts()["indices_built"] == 0 and same_bits(a, again)
    pre = device_clouds(reg)
    reg.build_indices([pre[t] for t in targets] + [pre[targets[0]]])   # a cloud listed twice is built once
    c = reg.fitness_batch_counts()
    assert c["indices_built"] == len(targets) and c["host_waits"] == 0 and c["edges"] == 0
    b = run(reg, pre, edges)
    assert reg.fitness_batch_counts()["indices_built"] == 0
    single = device_clouds(reg)
    q = R.scene()[0]["e9"]
    for t in targets:                               # the single-cloud build, as a registration target gets it
        reg.setInputTarget(single[t])
        reg.nearestKSearch(q)
    d = run(reg, single, edges)
    assert reg.fitness_batch_counts()["indices_built"] == 0
    assert same_bits(a, b) and same_bits(a, d)
    check_against(a[0], a[1], R.oracle_edges("main", DBL_MAX) + R.oracle_edges("size", DBL_MAX))


def test_nearest_search_on_batch_built_indices_equals_single_built(reg):
    from helpers import f32_transform
    clouds, _ = R.scene()
    names = ["sub1", "sub8", "sub9", "sub64", "sub65", "sub512", "sub513", "k0", "k4", "big"]
    batch = device_clouds(reg, names)
    single = device_clouds(reg, names)
    reg.build_indices([batch[n] for n in names])
    assert reg.fitness_batch_counts()["indices_built"] == len(names)
    q = np.ones((clouds["k1"].shape[0] + 2, 4), np.float32)
    q[:-2, :3] = f32_transform(R.relpose(0, 1), clouds["k1"])
    q[-2, :3] = (500.0, -300.0, 40.0)
    q[-1, :3] = (np.nan, 0.0, 0.0)
    for n in names:
        reg.setInputTarget(single[n])
        i1, d1 = reg.nearestKSearch(q)
        reg.setInputTarget(batch[n])
        i2, d2 = reg.nearestKSearch(q)
        assert np.array_equal(i1, i2) and np.array_equal(d1.view(np.int32), d2.view(np.int32)), n
    reg.build_indices([batch[n] for n in names] + [single[n] for n in names])
    assert reg.fitness_batch_counts()["indices_built"] == 0 and reg.fitness_batch_counts()["launches"] == 0


def test_a_kd_ordered_index_is_used_as_it_is():
    from delta_graph_slam_amd.registration import Registration
    old = os.environ.get("DGS_NN_KD_ALL")
    os.environ["DGS_NN_KD_ALL"] = "1"
    try:
        kd = Registration("FAST_GICP")
    finally:
        if old is None:
            del os.environ["DGS_NN_KD_ALL"]
        else:
            os.environ["DGS_NN_KD_ALL"] = old
    dc = device_clouds(kd)
    edges = R.main_edges()
    q = R.scene()[0]["e9"]
    for t in sorted({e[0] for e in edges}):
        kd.setInputTarget(dc[t])
        kd.nearestKSearch(q)                         # builds the k-d ordered index into the cloud
    scores, used = run(kd, dc, edges)
    assert kd.fitness_batch_counts()["indices_built"] == 0
    check_against(scores, used, R.oracle_edges("main", DBL_MAX))


# ---------------------------------------------------------------------------------------------- counts
def test_launches_and_waits_do_not_grow_with_the_batch(reg, warm):
    odo = list(R.main_edges()[:7])
    run(reg, warm, odo)
    seen = set()
    for n in range(2, 13):
        run(reg, warm, [odo[k % len(odo)] for k in range(n)])
        c = reg.fitness_batch_counts()
        assert c["edges"] == n and c["host_waits"] == 1 and c["indices_built"] == 0 and c["rows"] > n
        seen.add(c["launches"])
    assert seen == {2}                               # the walk and the closing launch
    clouds, _ = R.scene()
    cold_launches = set()
    for m in range(2, 9):
        fresh = [reg.make_cloud(clouds[f"k{k % 6}"]) for k in range(m)]   # m clouds of equal depth, none indexed
        s, u = reg.calc_fitness_score_batch(fresh, [warm["k1"]] * m, [R.relpose(0, 1)] * m, return_used=True)
        c = reg.fitness_batch_counts()
        assert c["indices_built"] == m and c["host_waits"] == 1
        cold_launches.add(c["launches"])
        assert s[0] == run(reg, warm, [("k0", "k1", R.relpose(0, 1))])[0][0]
    print("cold launches", cold_launches)
    assert len(cold_launches) == 1 and cold_launches.pop() == 2 + 5 + 3   # walk, close; boxes x 2, keys, sort, gather; one launch per level of depth 3


def test_loop_detection_finds_the_index_built_here():
    """`single_builds` counts every single-cloud index build (bvh_build) a handle makes outside the batched build.  A matching whose target
    keyframe was weighed before builds none; the same matching on a detector that weighed nothing builds the target's index itself
    (the control: the counter does see a matching's build)."""
    from delta_graph_slam_amd.information_matrix import InformationMatrixCalculator
    from delta_graph_slam_amd.loop_detector import KeyFrame, LoopDetector
    from delta_graph_slam_amd.registration import DeviceCloud, Registration
    clouds, poses = R.scene()

    def se2(T):
        m = np.eye(3)
        m[:2, :2] = T[:2, :2]
        m[:2, 2] = T[:2, 3]
        return m
    kfs = [KeyFrame(clouds[f"k{i}"], se2(poses[i]), accum_distance=2.0 * i, id=i) for i in range(6)]
    r = Registration("NDT_OMP", ndt_resolution=1.0)
    det = LoopDetector({}, registration=r, cache_clouds=True)
    calc = InformationMatrixCalculator(registration=r, resident=det.resident)
    edges = [(kfs[i], kfs[i - 1], R.relpose(i, i - 1)) for i in range(1, 6)]
    infs = calc.calc_information_matrices(edges)
    assert infs.shape == (5, 3, 3) and r.fitness_batch_counts()["indices_built"] == 5
    ref = R.oracle_edges("main", DBL_MAX)
    for e in range(5):
        assert np.allclose(infs[e], R.information_matrix({}, ref[e][0]), rtol=2.0 ** -23, atol=0)
    dc = det.resident(kfs[5], as_target=True)
    assert isinstance(dc, DeviceCloud)
    calc.calc_information_matrices(edges)
    assert r.fitness_batch_counts()["indices_built"] == 0       # the same resident clouds, already indexed
    before = r.fitness_batch_counts()["single_builds"]
    det.matching([kfs[0], kfs[1]], kfs[5])
    after = r.fitness_batch_counts()["single_builds"]
    print("single builds around a matching on a weighed keyframe:", before, after)
    assert after == before                                       # matching walked the index built above
    assert det.resident(kfs[5], as_target=True) is dc
    r2 = Registration("NDT_OMP", ndt_resolution=1.0)
    det2 = LoopDetector({}, registration=r2, cache_clouds=True)
    b2 = r2.fitness_batch_counts()["single_builds"]
    det2.matching([kfs[0], kfs[1]], kfs[5])
    a2 = r2.fitness_batch_counts()["single_builds"]
    print("single builds around the same matching on a fresh detector:", b2, a2)
    assert a2 > b2                                               # the control


# ---------------------------------------------------------------------------------------------- state and errors
def test_the_registration_state_is_untouched():
    from delta_graph_slam_amd.registration import Registration
    clouds, _ = R.scene()
    r = Registration("NDT_OMP", ndt_resolution=1.0)
    r.setInputTarget(clouds["k0"])
    r.setInputSource(clouds["k1"])
    r.align(R.relpose(0, 1).astype(np.float32))
    T0, f0, it0 = r.getFinalTransformation(), r.getFitnessScore(), r.last_result.iterations
    i0, d0 = r.nearestKSearch(clouds["e257"])
    dc = device_clouds(r)
    scores, used = run(r, dc, R.main_edges())
    check_against(scores, used, R.oracle_edges("main", DBL_MAX))
    assert np.array_equal(r.getFinalTransformation(), T0) and r.getFitnessScore() == f0
    i1, d1 = r.nearestKSearch(clouds["e257"])
    assert np.array_equal(i0, i1) and np.array_equal(d0, d1)
    r.align(R.relpose(0, 1).astype(np.float32))
    assert np.array_equal(r.getFinalTransformation(), T0) and r.last_result.iterations == it0 and r.getFitnessScore() == f0


def test_error_cases(reg, warm):
    import torch
    lib = reg._lib
    out = (C.c_double * 2)()
    a = (C.c_void_p * 2)(warm["k0"]._c.value, None)
    b = (C.c_void_p * 2)(warm["k1"]._c.value, warm["k1"]._c.value)
    for c1, c2 in ((a, b), (b, a)):
        rc = lib.dgs_calc_fitness_score_batch_clouds(reg._h, 2, C.cast(c1, C.c_void_p), C.cast(c2, C.c_void_p), None, DBL_MAX, C.cast(out, C.c_void_p), None)
        assert rc == 1 and b"NULL cloud" in lib.dgs_last_error(reg._h)
    assert lib.dgs_cloud_build_indices(reg._h, 2, C.cast(a, C.c_void_p)) == 1
    assert lib.dgs_calc_fitness_score_batch_clouds(reg._h, -1, None, None, None, DBL_MAX, None, None) == 1
    assert lib.dgs_calc_fitness_score_batch_clouds(reg._h, 2, None, C.cast(b, C.c_void_p), None, DBL_MAX, C.cast(out, C.c_void_p), None) == 1
    # no edges: DGS_OK without a launch
    assert lib.dgs_calc_fitness_score_batch_clouds(reg._h, 0, None, None, None, DBL_MAX, None, None) == 0
    c = reg.fitness_batch_counts()
    assert c["launches"] == 0 and c["edges"] == 0 and c["host_waits"] == 0
    s, u = reg.calc_fitness_score_batch([], [], [], return_used=True)
    assert s.shape == (0,) and u.shape == (0,)
    # a cloud of another device (DGS_ERR_INVALID_ARGUMENT, "lives on another device") needs a second GPU: on a one-GPU machine this branch
    # does not run and that path stays untested (DESIGN.md 6k says so)
    if torch.cuda.device_count() > 1:
        from delta_graph_slam_amd.registration import Registration
        other = Registration("FAST_GICP", device=1)
        oc = other.make_cloud(R.scene()[0]["sub9"])
        with pytest.raises(Exception):
            reg.calc_fitness_score_batch([oc], [warm["k1"]])
    with pytest.raises(ValueError):
        reg.calc_fitness_score_batch([warm["k0"]], [])


# ---------------------------------------------------------------------------------------------- Python and C++
def test_matrices_of_a_batch_equal_the_per_edge_call(reg, warm):
    from delta_graph_slam_amd.information_matrix import InformationMatrixCalculator
    clouds, _ = R.scene()
    calc = InformationMatrixCalculator(registration=reg)
    names = R.main_edges()[:8]
    edges = [(warm[a], warm[b], T) for a, b, T in names]
    infs = calc.calc_information_matrices(edges)
    ref = R.oracle_edges("main", DBL_MAX)
    for e, (c1, c2, T) in enumerate(edges):
        assert np.array_equal(calc.calc_information_matrix(c1, c2, T), infs[e])                    # DeviceClouds: a batch of one
        legacy = calc.calc_information_matrix(clouds[names[e][0]], clouds[names[e][1]], T)          # arrays: dgs_calc_fitness_score
        s_batch = calc.calc_fitness_score(c1, c2, T)
        s_single = calc.calc_fitness_score(clouds[names[e][0]], clouds[names[e][1]], T)
        print("edge", e, "batch", repr(s_batch), "single", repr(s_single), "oracle", repr(ref[e][0]))
        assert abs(s_batch - s_single) <= R.TOL * s_single and abs(s_batch - ref[e][0]) <= R.TOL * ref[e][0]
        # the weights are cast to float: a score that differs in its last bits moves a weight by at most one float rounding step
        assert np.allclose(legacy, infs[e], rtol=2.0 ** -23, atol=0)
        assert np.allclose(infs[e], R.information_matrix({}, ref[e][0]), rtol=2.0 ** -23, atol=0)
    mixed = calc.calc_information_matrices([(clouds[a], warm[b], T) for a, b, T in names])          # arrays are wrapped for the call
    assert np.array_equal(mixed, infs)
    const = InformationMatrixCalculator({"use_const_inf_matrix": True}, registration=reg).calc_information_matrices(edges)
    assert np.array_equal(const, np.stack([R.information_matrix({"use_const_inf_matrix": True}, 0.0)] * 8))


def test_cpp_adapter_equals_python(reg, warm, tmp_path):
    from delta_graph_slam_amd.information_matrix import InformationMatrixCalculator
    clouds, _ = R.scene()
    exe = R.build_driver(tmp_path)
    names = [f"k{i}" for i in range(6)] + ["sub65", "empty"]
    edges = list(R.main_edges()[:8]) + [("sub65", "k1", R.relpose(0, 1)), ("empty", "k1", np.eye(4))]
    prm = {"var_gain_a": 12.0, "fitness_score_thresh": 2.5, "delta_importance_ratio_global": 2.0}
    tail = (0.21, 0.6, 80.0, 0.0)
    ip, op = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    R.write_driver_input(ip, [clouds[n] for n in names], [(names.index(a), names.index(b), T) for a, b, T in edges], tail)
    res = json.loads(subprocess.check_output([exe, ip, op] + [f"{k}={v}" for k, v in prm.items()], timeout=120).decode().splitlines()[-1])
    assert res["ok"], res
    m = R.read_driver_output(op)
    E = len(edges)
    assert m.shape[0] == 2 + 3 * E
    assert np.array_equal(m[0], R.information_matrix_buildings_global(prm, tail[0]))
    assert np.array_equal(m[1], R.information_matrix_buildings_local(prm, tail[1], tail[2], False))
    batch, single, again = m[2:2 + E], m[2 + E:2 + 2 * E], m[2 + 2 * E:]
    assert np.array_equal(batch, single) and np.array_equal(batch, again)
    py = InformationMatrixCalculator(prm, registration=reg).calc_information_matrices([(warm[a], warm[b], T) for a, b, T in edges])
    assert np.allclose(batch, py, rtol=1e-14, atol=0)
