"""-m gpu tests of Registration.assign_batch / dgs_cloud_assign_batch: n inputs down-sampled into n resident clouds by one
chain of launches.  Every cloud must hold, bit for bit and in the same order, what dgs_voxel_grid_filter / dgs_approx_voxel_grid_filter
gives its input alone, and what the oracle's restatement of pcl::VoxelGrid / pcl::ApproximateVoxelGrid gives it: the two device calls run
one body each for the key and the centroid, so only the oracle anchors the arithmetic.  The clouds here are a few hundred
random points in a box, so most cells hold several points."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LEAF = 0.5
SIZES = (0, 1, 255, 256, 257, 1003)   # the shared key array puts the cloud boundaries at 0, 1, 256, 512, 769: inside workgroups of 256 and on their edges


def _box(n, seed, centre=(0.0, 0.0, 0.0), half=3.0):
    rng = np.random.default_rng(seed)
    c = np.ones((n, 4), np.float32)
    c[:, :3] = (rng.uniform(-half, half, (n, 3)) + np.asarray(centre)).astype(np.float32)
    return c


ORACLE = None   # oracle.oracle, once the module's registration exists


@pytest.fixture(scope="module")
def reg(oracle_lib):
    from delta_graph_slam_amd.registration import Registration
    global ORACLE
    ORACLE = oracle_lib
    r = Registration("FAST_GICP", gicp_max_correspondence_distance=2.0)
    yield r
    r.close()


def _empty(reg, n):
    return [reg.make_cloud(np.zeros((0, 4), np.float32)) for _ in range(n)]


def _check(reg, inputs, method="VOXELGRID", leaf=LEAF, clouds=None):
    """assign_batch of `inputs` against the single-cloud filter on each input alone, and both against the oracle -> the clouds"""
    clouds = clouds or _empty(reg, len(inputs))
    sizes = reg.assign_batch(clouds, inputs, method, leaf)
    for i, (c, a) in enumerate(zip(clouds, inputs)):
        alone = a if method == "NONE" else reg.voxel_grid_filter(a, leaf, approximate=(method == "APPROX_VOXELGRID"))
        got = c.read(reg)
        assert sizes[i] == alone.shape[0] == len(c) == got.shape[0], (i, sizes[i], alone.shape, len(c), got.shape)
        assert np.array_equal(got.view(np.uint32), np.ascontiguousarray(alone, np.float32).view(np.uint32)), i
        if method != "NONE":   # same cells, same order, same float sums as upstream's filter
            ref = (ORACLE.approx_voxel_grid if method == "APPROX_VOXELGRID" else ORACLE.voxel_grid)(a, leaf)
            assert got.shape == ref.shape and np.array_equal(got.view(np.uint32), ref.view(np.uint32)), (i, got.shape, ref.shape)
    return clouds


def test_sizes_around_a_workgroup_in_one_batch(reg):
    inputs = [_box(n, 10 + n) for n in SIZES]
    _check(reg, inputs)
    c = reg.cloud_assign_counts()
    assert c["clouds"] == len(SIZES) and c["host_waits"] == 2 and c["launches"] == 8   # whatever n is
    _check(reg, inputs[2:4])
    c2 = reg.cloud_assign_counts()
    assert c2["host_waits"] == 2 and c2["launches"] == 8


def test_identical_clouds_do_not_merge_and_order_does_not_matter(reg):
    a = _box(700, 3)
    inputs = [a, a.copy(), _box(300, 4), a.copy()]
    fwd = _check(reg, inputs)
    rev = _check(reg, inputs[::-1])
    for f, r in zip(fwd, rev[::-1]):
        assert np.array_equal(f.read(reg).view(np.uint32), r.read(reg).view(np.uint32))
    assert len(fwd[0]) == len(fwd[1]) == len(fwd[3]) < 700


def test_non_finite_points(reg):
    only = np.full((64, 4), np.nan, np.float32)
    only[::2, 0] = np.inf
    tail = _box(500, 5)
    tail[430:, 1] = np.nan
    mixed = _box(400, 6)
    mixed[::7, 2] = -np.inf
    clouds = _check(reg, [only, tail, mixed, _box(50, 7)])
    assert len(clouds[0]) == 0 and len(clouds[1]) > 0


def test_clouds_far_apart_have_grids_of_their_own(reg):
    inputs = [_box(600, 8), _box(600, 9, centre=(1000.0, -2000.0, 50.0)), _box(600, 8, centre=(-0.25, 0.25, 0.1)), _box(5, 12, centre=(1e4, 1e4, 0.0), half=0.01)]
    _check(reg, inputs)
    from tests.voxel_lattice import lattice_cloud
    for leaf in (0.5, 0.1):   # points on the cell faces and one float to either side, between two random clouds; exact and inexact 1 / leaf
        _check(reg, [inputs[1], lattice_cloud(leaf), inputs[2]], leaf=leaf)


def test_copy_and_approximate_filters(reg):
    inputs = [_box(n, 20 + n) for n in (0, 1, 300, 257, 1003)]
    _check(reg, inputs, method="NONE")
    _check(reg, inputs, method="APPROX_VOXELGRID")
    assert reg.cloud_assign_counts()["host_waits"] == sum(1 for a in inputs if a.shape[0])   # one per cloud: the header says so


def test_device_inputs_give_the_same_clouds(reg):
    import torch
    inputs = [_box(n, 30 + n) for n in (257, 1003, 64)]
    host = _check(reg, inputs)
    dev = _empty(reg, 3)
    reg.assign_batch(dev, [torch.from_numpy(a).cuda() for a in inputs], "VOXELGRID", LEAF)
    for h, d in zip(host, dev):
        assert np.array_equal(h.read(reg).view(np.uint32), d.read(reg).view(np.uint32))


def test_refill_smaller_then_larger_leaves_nothing_stale(reg):
    from tests import align_pairs_scenes as S
    tgt, src, _ = S.base()
    cloud = reg.make_cloud(S.subset(src, 3000, 1))
    r = S.make_registration()
    T = r.make_cloud(S.subset(tgt, 4000, 2))
    r.align_pairs([T], [cloud])   # the cloud now carries an index and covariances of its 3,000 points
    small, large = S.subset(src, 900, 3), S.subset(src, 5000, 4)
    for a in (small, large):
        _check(r, [a], leaf=0.25, clouds=[cloud])
    fresh = r.make_cloud(r.voxel_grid_filter(large, 0.25))
    a, b = r.align_pairs([T, cloud], [cloud, T]), r.align_pairs([T, fresh], [fresh, T])
    for x, y in zip(a, b):
        assert np.array_equal(x["T"], y["T"]) and x["iterations"] == y["iterations"] and x["converged"] == y["converged"] and x["status"] == y["status"] == 0
        assert np.float64(x["fitness"]).view(np.uint64) == np.float64(y["fitness"]).view(np.uint64)
    r.close()


def test_refilling_a_handles_source_detaches_it(reg):
    from delta_graph_slam_amd import _lib as L
    from tests import align_pairs_scenes as S
    tgt, src, _ = S.base()
    r = S.make_registration()
    T, Sc = r.make_cloud(S.subset(tgt, 2000, 5)), r.make_cloud(S.subset(src, 1000, 6))
    r.setInputTarget(T)
    r.setInputSource(Sc)
    r.align()
    assert r.last_result.status == 0
    reg.assign_batch([Sc], [S.subset(src, 800, 7)], "VOXELGRID", 0.25)   # another handle of the device makes the call
    res = L.Result()
    assert r._lib.dgs_align(r._h, None, C.byref(res), None, 0) == 4 and res.status == 4   # DGS_ERR_NO_SOURCE
    r.setInputSource(Sc)
    r.align()
    assert r.last_result.status == 0
    r.close()


def test_a_leaf_that_overflows_one_cloud_changes_none(reg):
    from delta_graph_slam_amd.registration import DgsError
    inputs = [_box(300, 40, half=0.2), _box(300, 41, half=2.0), _box(300, 42, half=0.2)]
    clouds = _check(reg, inputs, leaf=0.25)
    before = [c.read(reg) for c in clouds]
    with pytest.raises(DgsError) as e:
        reg.assign_batch(clouds, [a[::-1].copy() for a in inputs], "VOXELGRID", 1e-3)
    assert e.value.status == 5 and "cloud 1" in str(e.value)   # DGS_ERR_GRID_TOO_LARGE, the position named
    for c, b in zip(clouds, before):
        assert len(c) == b.shape[0] and np.array_equal(c.read(reg).view(np.uint32), b.view(np.uint32))
    with pytest.raises(DgsError) as e1:
        reg.voxel_grid_filter(inputs[1], 1e-3)   # the single call refuses the same cloud
    assert e1.value.status == 5


def test_errors_and_the_empty_call(reg):
    from delta_graph_slam_amd import _lib as L
    a = _box(100, 50)
    c1, c2 = _empty(reg, 2)
    ptrs = (C.c_void_p * 2)(a.ctypes.data, a.ctypes.data)
    sizes = (C.c_int64 * 2)(100, 100)
    out = (C.c_int64 * 2)()
    call = lambda n, clouds, filt=1, leaf=0.5: reg._lib.dgs_cloud_assign_batch(reg._h, n, C.cast(ptrs, C.c_void_p), C.cast(sizes, C.c_void_p), 0, filt, leaf,
                                                                             C.cast(clouds, C.c_void_p), C.cast(out, C.c_void_p))
    assert call(2, (C.c_void_p * 2)(c1._c.value, c1._c.value)) == 1 and "twice" in reg._lib.dgs_last_error(reg._h).decode()   # DGS_ERR_INVALID_ARGUMENT
    assert call(2, (C.c_void_p * 2)(c1._c.value, None)) == 1
    assert call(2, (C.c_void_p * 2)(c1._c.value, c2._c.value), filt=3) == 1 and call(2, (C.c_void_p * 2)(c1._c.value, c2._c.value), leaf=0.0) == 1
    assert reg._lib.dgs_cloud_size(c1._c) == 0 and reg._lib.dgs_cloud_size(c2._c) == 0
    reg.profile_enable(True)
    reg.profile_reset()
    assert call(2, (C.c_void_p * 2)(c1._c.value, c2._c.value)) == 0
    launches = lambda: sum(reg.profile_get(k)[1] for k in range(L.K_TRANSFORM + 1))
    before = launches()
    assert before > 0 and reg.cloud_assign_counts()["launches"] == 8
    assert reg._lib.dgs_cloud_assign_batch(reg._h, 0, None, None, 0, 1, 0.5, None, None) == 0
    assert reg.assign_batch([], [], "VOXELGRID", 0.5).shape == (0,)
    assert launches() == before and reg.cloud_assign_counts() == {"launches": 0, "host_waits": 0, "clouds": 0}
    reg.profile_enable(False)
