"""-m gpu tests of the batched k-NN covariance pass (delta_graph_slam_amd/csrc/cov_batch.hip): Registration.build_covariances
makes the covariances of many resident clouds in one search launch and one covariance launch per chunk, bit for bit what the single path
makes of each cloud alone.  "Single path": a fresh handle, setInputSource(array), gicp_covariances("source").  "Equal": the float64
arrays hold the same bits (np.array_equal on their uint64 views: NaN rows of non-finite points compare too, and -0.0 is not 0.0)."""
import numpy as np
import pytest

from delta_graph_slam_amd import synth

pytestmark = pytest.mark.gpu

FAMILIES = ["FAST_GICP", "GICP_HIP"]
EDGE_SIZES = [257, 1, 1000, 64, 9, 3001, 128, 7, 255, 65, 8, 129, 63, 256, 127]   # 1 .. 3001 at the edges of every unit, scrambled
_SINGLE = {}


def _cloud(n, seed):
    """n points of the ground-and-two-walls scene, shrunk with n so that neighbourhoods stay comparable: [n, 4] float32, w = 1"""
    rng = np.random.default_rng(seed)
    xyz = synth._planar_surfaces(max(n, 4), rng, 0.02)[rng.permutation(max(n, 4))[:n]]
    out = np.ones((n, 4), dtype=np.float32)
    out[:, :3] = xyz * min(1.0, (n / 16384.0) ** 0.5)
    return out


def _reg(method, k=20, **kw):
    from delta_graph_slam_amd.registration import Registration
    return Registration(method, gicp_correspondence_randomness=k, **kw)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _equal(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _single(method, pts, key, k=20, **kw):
    """the single path's covariances of `pts` ([n, 3, 3]), or None where it refuses the cloud (GICP_HIP: fewer than k points); computed once
    per (method, cloud key, parameters) and left unchanged"""
    from delta_graph_slam_amd.registration import DgsError
    full = (method, key, k, tuple(sorted(kw.items())))
    if full not in _SINGLE:
        r = _reg(method, k, **kw)
        try:
            r.setInputSource(pts)
            _SINGLE[full] = r.gicp_covariances("source")
        except DgsError as e:
            assert method == "GICP_HIP" and pts.shape[0] < k and e.status == 1, str(e)
            _SINGLE[full] = None
        r.close()
    return _SINGLE[full]


def _read(reg, dc):
    reg.setInputSource(dc)
    return reg.gicp_covariances("source")


def _check_batch(method, clouds, keys, k=20, reg=None, **kw):
    """one build_covariances over `clouds`; every cloud's covariances equal the single path's; reading them adds no covariance pass.
    -> (registration, device clouds, counts of the call)"""
    from delta_graph_slam_amd import _lib as L
    from delta_graph_slam_amd.registration import DgsError
    reg = reg or _reg(method, k, **kw)
    dcs = [reg.make_cloud(c) for c in clouds]
    reg.build_covariances(dcs)
    counts = reg.covariance_batch_counts()
    reg.profile_enable(True)
    reg.profile_reset()
    served = 0
    for c, key, dc in zip(clouds, keys, dcs):
        want = _single(method, c, key, k, **kw)
        if want is None:   # left without covariances: the cloud is refused as it is alone
            with pytest.raises(DgsError) as ei:
                _read(reg, dc)
            assert ei.value.status == 1
            continue
        got = _read(reg, dc)
        assert _equal(got, want), (method, key, k, kw, int((_bits(got) != _bits(want)).sum()))
        served += 1
    assert reg.profile_get(L.K_GICP_COVARIANCE)[1] == 0   # every read found the cache the batched pass left
    reg.profile_enable(False)
    assert counts["covered"] + counts["cached"] == served, (counts, served)
    return reg, dcs, counts


# ------------------------------------------------------------------------------------------------------ edges of every unit
@pytest.mark.parametrize("method", FAMILIES)
def test_every_unit_edge_in_one_call_equals_the_single_path(method):
    """leaf (8), window (64), covariance wave (32) and workgroup (128), GICP_HIP's workgroup (256): clouds of 1 .. 3001 points in a
    scrambled order, so that cloud boundaries fall inside the workgroup sequence of both launches"""
    clouds = [_cloud(n, 100 + n) for n in EDGE_SIZES]
    reg, dcs, counts = _check_batch(method, clouds, [("edge", n) for n in EDGE_SIZES])
    short = sum(n < 20 for n in EDGE_SIZES) if method == "GICP_HIP" else 0
    assert counts == {"launches": 2, "host_waits": 0, "listed": 15, "covered": 15 - short, "cached": 0, "chunks": 1, "fallback": 0, "indices_built": 15}, counts
    if method == "GICP_HIP":
        # a cloud of fewer than k points fails the pairs that name it, and only those
        big, small = dcs[EDGE_SIZES.index(1000)], dcs[EDGE_SIZES.index(9)]
        res = reg.align_pairs([big, small, big], [dcs[EDGE_SIZES.index(257)], big, small])
        assert [r["status"] for r in res] == [0, 1, 1], res
    reg.close()


# ------------------------------------------------------------------------------------------------------ widths and k
@pytest.mark.parametrize("k", [1, 8, 32, 33, 64])
@pytest.mark.parametrize("method", FAMILIES)
def test_narrow_and_wide_k_equal_the_single_path(method, k):
    sizes = [65, 1000, 63, 257, 64]
    reg, _, counts = _check_batch(method, [_cloud(n, 200 + n) for n in sizes], [("k", n) for n in sizes], k=k)
    assert counts["launches"] == 2 and counts["chunks"] == 1 and counts["fallback"] == 0
    assert counts["covered"] == sum(n >= k or method == "FAST_GICP" for n in sizes)
    reg.close()


# ------------------------------------------------------------------------------------------------------ regularisation
@pytest.mark.parametrize("svd", [0, 1, 2])
@pytest.mark.parametrize("regularization", [0, 1, 2, 3, 4])
def test_every_regularisation_and_covariance_mode(regularization, svd):
    """mode 2 (upstream order) keeps its per-cloud loop inside the call: equal results, every cloud counted as a fallback"""
    sizes = [300, 77]
    reg, _, counts = _check_batch("FAST_GICP", [_cloud(n, 300 + n) for n in sizes], [("reg", n) for n in sizes], gicp_regularization=regularization,
                                  gicp_cov_jacobi_svd=svd)
    assert counts["covered"] == 2 and counts["fallback"] == (2 if svd == 2 else 0) and counts["chunks"] == (0 if svd == 2 else 1), counts
    reg.close()


# ------------------------------------------------------------------------------------------------------ the careful paths
def _careful_clouds():
    nan_rows = _cloud(400, 41)
    nan_rows[[70, 71, 200], :3] = np.nan                       # non-finite points inside a window of 64
    nan_rows[333, 1] = np.inf
    dup = np.repeat(_cloud(150, 42), 3, axis=0)                # every point three times: ties at the k-th distance
    one = np.repeat(_cloud(1, 43), 100, axis=0)                # one point repeated 100 times
    line = np.ones((40, 4), dtype=np.float32)                  # 40 collinear points
    line[:, :3] = np.outer(np.arange(40, dtype=np.float32), np.float32([0.25, 0.5, -0.125]))
    return {"nan": nan_rows, "dup": dup, "one": one, "line": line}


@pytest.mark.parametrize("which", ["nan", "dup", "one", "line"])
@pytest.mark.parametrize("method", FAMILIES)
def test_irregular_clouds_beside_a_regular_one(method, which):
    reg, _, counts = _check_batch(method, [_careful_clouds()[which], _cloud(500, 44)], [("careful", which), ("careful", "regular")])
    assert counts["covered"] == 2 and counts["launches"] == 2
    reg.close()


# ------------------------------------------------------------------------------------------------------ parts
@pytest.mark.parametrize("method", FAMILIES)
def test_clouds_of_every_parts_value_in_one_call(method):
    """262,144 points (parts 1), 131,080 (parts 2) and 1,000 (parts 4): just above the sizes from which knn_lists chooses 1 (262,137) and
    2 (131,065).  The slot order of a neighbour list follows parts, and FAST_GICP's sums follow slot order."""
    sizes = [262144, 131080, 1000]
    rng = np.random.default_rng(5)
    clouds = []
    for n in sizes:
        c = np.ones((n, 4), dtype=np.float32)
        c[:, :3] = synth._planar_surfaces(n, rng, 0.02)
        clouds.append(c)
    reg, _, counts = _check_batch(method, clouds, [("parts", n) for n in sizes])
    assert counts["covered"] == 3 and counts["chunks"] == 1 and counts["launches"] == 2, counts
    reg.close()


# ------------------------------------------------------------------------------------------------------ chunks
@pytest.mark.parametrize("method,chunks", [("FAST_GICP", 4), ("GICP_HIP", 3)])
def test_chunks_follow_the_point_budget(monkeypatch, method, chunks):
    """DGS_COV_BATCH_POINTS=300 over 129, 200, 64, 500, 10 points: [129] [200 64] [500: above the budget, alone] [10] -- GICP_HIP at
    k = 20 leaves the cloud of 10 points out, and with it the last chunk"""
    monkeypatch.setenv("DGS_COV_BATCH_POINTS", "300")
    reg = _reg(method)
    monkeypatch.delenv("DGS_COV_BATCH_POINTS")   # read when the handle is made: the single path's handles are made without it (and one chunk each anyway)
    sizes = [129, 200, 64, 500, 10]
    _, _, counts = _check_batch(method, [_cloud(n, 500 + n) for n in sizes], [("chunk", n) for n in sizes], reg=reg)
    assert counts["chunks"] == chunks and counts["launches"] == 2 * chunks and counts["host_waits"] == 0, counts
    reg.close()


# ------------------------------------------------------------------------------------------------------ launches do not follow the batch
@pytest.mark.parametrize("method", FAMILIES)
def test_launches_do_not_follow_the_number_of_clouds(method):
    got = []
    for n_clouds in (2, 12):
        sizes = [1000 - 7 * i for i in range(n_clouds)]
        reg, _, counts = _check_batch(method, [_cloud(n, 600 + n) for n in sizes], [("launch", n) for n in sizes])
        assert counts["covered"] == n_clouds and counts["host_waits"] == 0
        got.append(counts["launches"])
        reg.close()
    assert got[0] == got[1] == 2, got


# ------------------------------------------------------------------------------------------------------ cache
@pytest.mark.parametrize("method", FAMILIES)
def test_cache_keys_duplicates_and_refills(method):
    sizes = [300, 450, 77]
    clouds = [_cloud(n, 700 + n) for n in sizes]
    keys = [("cache", n) for n in sizes]
    reg = _reg(method)
    dcs = [reg.make_cloud(c) for c in clouds]
    reg.build_covariances([dcs[0], dcs[1], dcs[0], dcs[2], dcs[1]])   # listed twice: covered once
    c = reg.covariance_batch_counts()
    assert (c["listed"], c["covered"], c["cached"], c["launches"], c["indices_built"]) == (5, 3, 0, 2, 3), c
    reg.build_covariances(dcs)                                        # a second call covers nothing and launches nothing
    c = reg.covariance_batch_counts()
    assert (c["listed"], c["covered"], c["cached"], c["launches"], c["chunks"], c["indices_built"]) == (3, 0, 3, 0, 0, 0), c
    other = _reg(method, k=12)                                        # a handle with another k rebuilds (the index stays)
    other.build_covariances(dcs)
    c = other.covariance_batch_counts()
    assert (c["covered"], c["cached"], c["launches"], c["indices_built"]) == (3, 0, 2, 0), c
    for pts, dc in zip(clouds, dcs):
        assert _equal(_read(other, dc), _single(method, pts, ("cache", pts.shape[0]), 12))
    reg.build_covariances(dcs)                                        # ... and the first handle's key no longer answers
    assert reg.covariance_batch_counts()["covered"] == 3
    fresh = _cloud(222, 799)
    reg.assign_batch([dcs[1]], [fresh])                               # a cloud refilled in place is rebuilt, index and covariances
    reg.build_covariances(dcs)
    c = reg.covariance_batch_counts()
    assert (c["covered"], c["cached"], c["indices_built"]) == (1, 2, 1), c
    assert _equal(_read(reg, dcs[1]), _single(method, fresh, ("cache", "fresh")))
    assert _equal(_read(reg, dcs[0]), _single(method, clouds[0], keys[0]))
    other.close()
    reg.close()


@pytest.mark.parametrize("method", FAMILIES)
def test_a_table_that_outgrows_its_pinned_block_between_calls(method):
    """1 cloud, then 64 clouds of at most 64 points -- 64 entries of 96 bytes, more than the bytes + bytes / 4 + 4 KiB the first call
    left the pinned block with -- then 1 cloud again, all on one handle: every call gives the single path's bits and the counts a fresh
    handle reports"""
    sizes = (20, 33, 64, 47)
    one, many = [_cloud(300, 77)], [_cloud(sizes[i % 4], 200 + sizes[i % 4]) for i in range(64)]   # 64 device clouds of four arrays
    reg = _reg(method)
    for clouds, keys in ((one, [("grow", 300)]), (many, [("grow", sizes[i % 4]) for i in range(64)]), (one, [("grow", 300)])):
        n = len(clouds)
        _, _, counts = _check_batch(method, clouds, keys, reg=reg)
        assert counts == {"launches": 2, "host_waits": 0, "listed": n, "covered": n, "cached": 0, "chunks": 1, "fallback": 0, "indices_built": n}, counts
    reg.close()


# ------------------------------------------------------------------------------------------------------ refusals
@pytest.mark.parametrize("method,name", [("NDT_OMP", "NDT_OMP"), ("ICP_HIP", "ICP_HIP"), ("PCL_NDT_HIP", "PCL_NDT_HIP")])
def test_other_methods_are_refused_with_the_method_named(method, name):
    from delta_graph_slam_amd.registration import DgsError, Registration
    reg = Registration(method)
    dc = reg.make_cloud(_cloud(100, 8))
    with pytest.raises(DgsError) as ei:
        reg.build_covariances([dc])
    assert ei.value.status == 6 and name in str(ei.value), str(ei.value)
    reg.close()


@pytest.mark.parametrize("method", FAMILIES)
def test_k_65_none_and_the_empty_list(method):
    import ctypes as C
    from delta_graph_slam_amd.registration import DgsError
    pts = _cloud(300, 9)
    reg = _reg(method, k=65)
    dc = reg.make_cloud(pts)
    with pytest.raises(DgsError) as ei:
        reg.build_covariances([dc])
    assert ei.value.status == 6 and "64" in str(ei.value), str(ei.value)
    assert np.isfinite(reg.calc_fitness_score(pts, pts))   # the handle works afterwards
    reg.close()
    reg = _reg(method)
    dc = reg.make_cloud(pts)
    with pytest.raises(TypeError):
        reg.build_covariances([dc, None])
    arr = (C.c_void_p * 2)(dc._c.value, None)               # the library's own refusal of a NULL cloud: nothing modified
    assert reg._lib.dgs_cloud_build_covariances(reg._h, 2, C.cast(arr, C.c_void_p)) == 1
    assert reg.fitness_batch_counts()["indices_built"] == 0
    reg.build_covariances([])                                # n == 0: fine, no launch
    c = reg.covariance_batch_counts()
    assert c["launches"] == 0 and c["listed"] == 0
    reg.build_covariances([dc])
    assert reg.covariance_batch_counts()["covered"] == 1
    reg.close()


# ------------------------------------------------------------------------------------------------------ wiring
@pytest.mark.parametrize("method", FAMILIES)
def test_align_pairs_makes_its_covariances_in_one_batched_pass(method):
    from delta_graph_slam_amd import _lib as L
    tgt, src, _ = synth.planar_pair(n=2048)
    reg = _reg(method, gicp_max_correspondence_distance=2.0)
    targets = [reg.make_cloud(np.ascontiguousarray(tgt[i * 100:i * 100 + 1500])) for i in range(3)]
    sources = [reg.make_cloud(np.ascontiguousarray(src[i * 100:i * 100 + 1200])) for i in range(3)]
    reg.profile_enable(True)
    reg.profile_reset()
    res = reg.align_pairs(targets, sources)
    assert [r["status"] for r in res] == [0, 0, 0]
    c = reg.covariance_batch_counts()
    assert (c["listed"], c["covered"], c["chunks"], c["launches"], c["fallback"], c["indices_built"]) == (6, 6, 1, 2, 0, 6), c
    assert reg.profile_get(L.K_GICP_COVARIANCE)[1] == 6     # "covariance passes, one per cloud"
    reg.close()


def test_a_fleet_step_launches_the_same_for_three_and_six_streams():
    from delta_graph_slam_amd.odometry import ScanMatchingOdometryFleet
    from delta_graph_slam_amd.registration import Registration
    frames, _ = synth.vlp16_stream(n_frames=3)
    cfg = dict(keyframe_delta_trans=1.0, keyframe_delta_angle=1.0, keyframe_delta_time=1e9, downsample_method="VOXELGRID", downsample_resolution=0.4)
    got = []
    for b in (3, 6):
        reg = Registration("FAST_GICP", gicp_max_correspondence_distance=2.0, transformation_epsilon=0.1)
        fleet = ScanMatchingOdometryFleet(reg, b, [cfg] * b)
        for k in range(3):
            fleet.step([0.1 * k] * b, [frames[k]] * b)
        c = reg.covariance_batch_counts()   # the third step: one new frame per stream, the keyframes' covariances kept
        assert c["covered"] == b and c["chunks"] == 1 and c["host_waits"] == 0, c
        got.append(c["launches"])
        reg.close()
    assert got[0] == got[1] == 2, got
