"""dgs_prefilter_scan_batch / Prefilter.filter_scan_batch (delta_graph_slam_amd/csrc/prefilter_batch.hip) on the MI355X:
many scans through the prefilter chain in one device call.  The yardstick is the single call filter_scan of the same handle type, scan
by scan; one test compares with the numpy restatements directly.  No tolerance anywhere: every comparison is np.array_equal on the
float32 bits, order included."""
import json
import os
import subprocess

import numpy as np
import pytest

import prefilter_edge_cases as E
import prefilter_reference as R
import prefilter_scan_reference as S
from delta_graph_slam_amd import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TYPICAL = (0.3, -0.8, 1.1)
M = S.base_link_matrix()
HEADS = [(None, None), (TYPICAL, None), (None, M), (TYPICAL, M)]      # none, deskew only, transform only, both
NOFILTER = dict(downsample_method="NONE", outlier_removal_method="NONE")
TINY = (0, 1, 63, 64, 65, 255, 256, 257)


def _pf(params=None, registration=None):
    from delta_graph_slam_amd.prefilter import Prefilter
    return Prefilter(params, registration=registration)


def _bits(a):
    return np.ascontiguousarray(_host(a), np.float32).view(np.uint32)


def _host(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else x


def _dev(c):
    import torch
    return torch.from_numpy(np.ascontiguousarray(c, np.float32)).cuda()


def small_vlp16(seed=22, azimuths=256):
    """A VLP-16 frame of 16 beams x 256 azimuths (3,672 returns).  Seed 22: under LAUNCH / VOXELGRID with both head steps the
    restatement finds no radius tie and no normal within the band of the threshold (test 5 checks it), so that comparison is exact."""
    xyz, _ = synth.street_scan((-30.0, 1.0, 0.1), 16, (15.0, -15.0), azimuths, seed)
    return synth._xyz1(xyz)


def tiny(n):
    return E.blob(n) if n else np.zeros((0, 4), np.float32)


def mixed_batch():
    """The scans of tests 1 and 5 and a head for each: every kind of head beside every other."""
    scans = [tiny(n) for n in TINY] + [small_vlp16()]
    heads = [HEADS[i % 4] for i in range(len(scans))]
    heads[-1] = HEADS[3]
    return scans, heads


def single(pf, cloud, head):
    """filter_scan of one scan -> (f3, f2, lidar, status): the status the single call returned, empty outputs when it failed"""
    from delta_graph_slam_amd import _lib as L
    try:
        f3, f2, lp = pf.filter_scan(cloud, head[0], head[1])
        return f3, f2, lp, 0
    except L.DgsError as e:
        _, _, lp = _pf(NOFILTER, pf.registration).filter_scan(cloud[:0], head[0], head[1])
        return cloud[:0], cloud[:0], lp, e.status


def assert_equals_single(pf, scans, heads, out, statuses, what=""):
    assert len(out) == len(scans) and statuses.shape == (len(scans),)
    for i, (c, hd) in enumerate(zip(scans, heads)):
        f3, f2, lp, st = single(pf, c, hd)
        g3, g2, glp = out[i]
        assert statuses[i] == st, (what, i, statuses[i], st)
        assert g3.shape == f3.shape and g2.shape == f2.shape, (what, i, g3.shape, f3.shape, g2.shape, f2.shape)
        assert np.array_equal(_bits(g3), _bits(f3)), (what, i, E.first_difference(_host(g3), _host(f3)))
        assert np.array_equal(_bits(g2), _bits(f2)), (what, i, E.first_difference(_host(g2), _host(f2)))
        assert np.array_equal(glp, lp), (what, i)


def run_batch(pf, scans, heads, device=False):
    src = [_dev(c) for c in scans] if device else scans
    out, st = pf.filter_scan_batch(src, [h[0] for h in heads], [h[1] for h in heads])
    if device:
        assert all(o[0].is_cuda and o[1].is_cuda for o in out)
    return out, st


# ---- 1. equal to the single call ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pname,params", [("launch", R.LAUNCH), ("defaults", R.DEFAULTS)])
@pytest.mark.parametrize("ds", ["VOXELGRID", "APPROX_VOXELGRID", "NONE"])
def test_every_scan_of_a_batch_equals_the_single_call(pname, params, ds):
    params = dict(params, downsample_method=ds)
    scans, heads = mixed_batch()
    pf = _pf(params)
    for device in (False, True):
        out, st = run_batch(pf, scans, heads, device)
        assert_equals_single(pf, scans, heads, out, st, f"{pname} {ds} device={device}")
        assert out[-1][0].shape[0] > 500 and out[-1][1].shape[0] > 20                     # the frame comes through both outputs
        if pname == "defaults":
            # 0 < points <= mean_k at the statistical pass: that scan's status, counts 0, the others unaffected (compared above)
            assert st[1] == 1 and out[1][0].shape[0] == 0 and out[1][1].shape[0] == 0
            assert st[0] == 0 and st[-1] == 0 and sum(int(s == 0) for s in st) >= 6
        else:
            assert not st.any()
        print(f"{pname} {ds} device={device}: statuses {st.tolist()}, 3D {[o[0].shape[0] for o in out]}, 2D {[o[1].shape[0] for o in out]}, counts {pf.batch_counts().tolist()}")


def test_without_heads_the_batch_is_dgs_prefilter_with_a_zero_lidar_position():
    import ctypes as C
    scans, _ = mixed_batch()
    pf = _pf(R.LAUNCH)
    n = len(scans)
    sizes = np.array([c.shape[0] for c in scans], np.int64)
    o3 = [np.zeros((max(c.shape[0], 1), 4), np.float32) for c in scans]
    o2 = [np.zeros((max(c.shape[0], 1), 4), np.float32) for c in scans]
    arr = lambda xs: (C.c_void_p * n)(*[x.ctypes.data_as(C.c_void_p) for x in xs])
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    m3, m2, st, lp = np.zeros(n, np.int64), np.zeros(n, np.int64), np.full(n, -1, np.int32), np.full((n, 3), -1.0)
    rc = pf._lib.dgs_prefilter_scan_batch(pf._h, C.byref(pf.params), n, None, arr(scans), vp(sizes), 0, arr(o3), vp(sizes), arr(o2), vp(sizes), 0, vp(m3), vp(m2),
                                          vp(lp), vp(st))
    assert rc == 0 and not st.any() and not lp.any()
    for i, c in enumerate(scans):
        g3, g2 = pf.cloud_callback(c)
        assert np.array_equal(_bits(o3[i][:m3[i]]), _bits(g3)) and np.array_equal(_bits(o2[i][:m2[i]]), _bits(g2))
    # a capacity too small fails that scan alone and still reports the full counts, as the single call does
    full3, full2 = m3.copy(), m2.copy()
    cap3, cap2 = sizes.copy(), sizes.copy()
    cap3[-1] = full3[-1] - 1
    cap2[5] = max(full2[5] - 1, 0)
    rc = pf._lib.dgs_prefilter_scan_batch(pf._h, C.byref(pf.params), n, None, arr(scans), vp(sizes), 0, arr(o3), vp(cap3), arr(o2), vp(cap2), 0, vp(m3), vp(m2),
                                          vp(lp), vp(st))
    assert rc == 0 and st[-1] == 1 and np.array_equal(m3, full3) and np.array_equal(m2, full2)
    assert st[5] == (1 if full2[5] > 0 else 0) and not np.delete(st, [5, n - 1]).any()


# ---- 2. independent of the batch -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pname,params", [("launch", R.LAUNCH), ("defaults", R.DEFAULTS)])
def test_a_scan_gets_the_same_bits_wherever_it_stands(pname, params):
    x, hx = small_vlp16(seed=5), HEADS[3]
    a, b, c, d = tiny(257), tiny(65), small_vlp16(seed=9, azimuths=100), tiny(0)
    pf = _pf(params)
    layouts = [([x], 0), ([x, a, b], 0), ([a, c, x, b, d], 2), ([d, b, c, x], 3), ([c, x], 1)]
    got = []
    for scans, pos in layouts:
        heads = [HEADS[(j + pos) % 4] for j in range(len(scans))]
        heads[pos] = hx
        out, st = run_batch(pf, scans, heads, device=len(scans) % 2 == 0)
        assert st[pos] == 0
        got.append((_bits(out[pos][0]), _bits(out[pos][1]), out[pos][2]))
    assert got[0][0].shape[0] > 500 and got[0][1].shape[0] > 20
    for g in got[1:]:
        assert np.array_equal(g[0], got[0][0]) and np.array_equal(g[1], got[0][1]) and np.array_equal(g[2], got[0][2])


# ---- 3. segment edges of the compaction -----------------------------------------------------------------------------------------
def mask_scan(n, name, lift=False):
    """A scan of which the distance filter keeps exactly cloud[mask]; lift: the points form a wall in the plane of their x above
    z = 1 (norm below 11 or above 200 still), so the kept ones pass the height filter and, where enough stand together, the normal filter."""
    cloud, mask = E.mask_case(n, name)
    if lift:
        i = np.arange(n)
        cloud[:, 0] += (0.001 * (i % 3)).astype(np.float32)
        cloud[:, 1] = (0.01 * (i // 7)).astype(np.float32)
        cloud[:, 2] = (1.0 + 0.05 * (i % 7)).astype(np.float32)
    return cloud, mask


def test_compaction_at_the_edges_between_scans():
    layout = [(257, "all"), (256, "none"), (255, "all"),           # a scan that keeps nothing between two that keep everything
              (64, "last"), (65, "first"),                         # a kept last point next to a kept first point of the next scan
              (256, "last"), (257, "first"), (1, "all"), (1, "none"), (63, "random_50"), (1, "all"), (255, "random_50"), (64, "none"),
              (65, "all"), (256, "all"), (63, "last"), (257, "random_50"), (255, "first")]
    cases = [mask_scan(n, name, lift=j % 2 == 0) for j, (n, name) in enumerate(layout)]
    scans = [c for c, _ in cases]
    heads = [HEADS[0]] * len(scans)
    pf = _pf(NOFILTER)
    for device in (False, True):
        out, st = run_batch(pf, scans, heads, device)
        assert not st.any()
        for j, (c, mask) in enumerate(cases):
            assert np.array_equal(_bits(out[j][0]), _bits(c[mask])), (layout[j], E.first_difference(_host(out[j][0]), c[mask]))
        assert_equals_single(pf, scans, heads, out, st, f"device={device}")
    assert any(o[1].shape[0] > 0 for o in out)                      # the lifted scans reach the normal pass


def test_the_scan_kernels_carry_crosses_a_scan_boundary():
    # 56 scans of about 5,000 points: 20 workgroups each, 1,120 in all, so the scan's second chunk begins inside scan 51
    sizes = [5000 + 3 * j for j in range(56)]
    assert sum(sizes) > E.EDGE and (E.CHUNK % 20) != 0
    cases = [mask_scan(n, "random_50" if j % 5 else "all") for j, n in enumerate(sizes)]
    scans = [c for c, _ in cases]
    pf = _pf(NOFILTER)
    out, st = run_batch(pf, scans, [HEADS[0]] * len(scans), device=True)
    assert not st.any()
    for j, (c, mask) in enumerate(cases):
        assert np.array_equal(_bits(out[j][0]), _bits(c[mask])), (j, E.first_difference(_host(out[j][0]), c[mask]))
        assert out[j][1].shape[0] == 0                              # z = 0: the height filter keeps nothing
    for j in (0, 50, 51, 52, 55):
        f3, f2, _, _ = single(pf, scans[j], HEADS[0])
        assert np.array_equal(_bits(out[j][0]), _bits(f3)) and f2.shape[0] == 0


# ---- 4. k-NN length edges per scan inside one batch ------------------------------------------------------------------------------
@pytest.mark.parametrize("mean_k", sorted({k for k, _ in E.STATISTICAL_LENGTHS}))
def test_statistical_lengths_side_by_side(mean_k):
    sizes = [mean_k, mean_k - 1] + [n for k, n in E.STATISTICAL_LENGTHS if k == mean_k]   # k - 1 .. k + 1 of k = mean_k + 1 and beyond
    sizes = [n for n in sizes if n > 0]
    scans = [E.blob(n) for n in sizes]
    heads = [HEADS[0]] * len(scans)
    pf = _pf(dict(downsample_method="NONE", outlier_removal_method="STATISTICAL", statistical_mean_k=mean_k, statistical_stddev=1.0))
    out, st = run_batch(pf, scans, heads)
    stats = pf.batch_statistics()
    assert stats.shape == (len(scans), 4)
    for j, c in enumerate(scans):
        f3, f2, lp, s1 = single(pf, c, heads[j])
        assert st[j] == s1 == (1 if c.shape[0] <= mean_k else 0)
        assert np.array_equal(_bits(out[j][0]), _bits(f3)) and np.array_equal(_bits(out[j][1]), _bits(f2))
        if s1 == 0:
            _, s = pf.statistics()
            assert np.array_equal(stats[j], [s["mean"], s["stddev"], s["threshold"], s["n"]]), (j, stats[j], s)
        else:
            assert not stats[j].any()


@pytest.mark.parametrize("min_nb", sorted({k for k, _ in E.RADIUS_LENGTHS}))
def test_radius_lengths_side_by_side(min_nb):
    scans = [E.blob(n) for k, n in E.RADIUS_LENGTHS if k == min_nb]
    heads = [HEADS[0]] * len(scans)
    kept = 0
    for radius in E.RADIUS_LENGTH_RADII:
        for inclusive in E.SWITCHES:
            pf = _pf(dict(downsample_method="NONE", outlier_removal_method="RADIUS", radius_radius=radius, radius_min_neighbors=min_nb,
                          radius_inclusive=bool(inclusive)))
            out, st = run_batch(pf, scans, heads)
            assert_equals_single(pf, scans, heads, out, st, f"r={radius} inclusive={inclusive}")
            assert not st.any()
            kept += sum(o[0].shape[0] for o in out)
    assert kept > 0


def test_normal_lengths_side_by_side():
    scans = [E.blob(n) for n in E.NORMAL_LENGTHS]
    heads = [HEADS[0]] * len(scans)
    pf = _pf(NOFILTER)
    out, st = run_batch(pf, scans, heads)
    assert_equals_single(pf, scans, heads, out, st)
    assert [o[0].shape[0] for o in out] == list(E.NORMAL_LENGTHS)


@pytest.mark.parametrize("params", [dict(downsample_method="NONE", outlier_removal_method="RADIUS", radius_radius=0.25, radius_min_neighbors=4, distance_near_thresh=0.1),
                                    dict(downsample_method="NONE", outlier_removal_method="RADIUS", radius_radius=0.5, radius_min_neighbors=2, distance_near_thresh=0.1),
                                    dict(downsample_method="NONE", outlier_removal_method="STATISTICAL", statistical_mean_k=20, statistical_stddev=1.0)],
                         ids=["radius_0.25_4", "radius_0.5_2", "statistical"])
def test_tie_clouds_as_neighbours_of_a_scan_crop(params):
    crop = np.ascontiguousarray(small_vlp16()[:2048])
    scans = [E.lattice_plane(), crop, E.cubic_lattice(), E.duplicates(), E.line(), crop[::-1].copy()]
    heads = [HEADS[0]] * len(scans)
    pf = _pf(params)
    out, st = run_batch(pf, scans, heads)
    assert_equals_single(pf, scans, heads, out, st)
    # not vacuous: the lattice (r = spacing, 4 neighbours at exactly r; r = 2 spacings) and the crop keep points in every case
    assert not st.any() and out[0][0].shape[0] > 0 and out[1][0].shape[0] > 0


# ---- 5. against the restatement ------------------------------------------------------------------------------------------------
def test_the_batch_equals_the_numpy_restatement(oracle_lib):
    params = dict(R.LAUNCH, downsample_method="VOXELGRID")
    scans, heads = mixed_batch()
    refs = []
    for c, hd in zip(scans, heads):
        r3, r2, lp, info = S.filter_scan(c, params, hd[0], hd[1], orc=oracle_lib)
        # the scans are chosen so that nothing hangs on a tie or on the last bits of a normal: checked here, on the CPU
        assert info.get("radius_ties", 0) == 0 and int(np.count_nonzero(info["normal_band"])) == 0
        refs.append((r3, r2, lp))
    pf = _pf(params)
    for device in (False, True):
        out, st = run_batch(pf, scans, heads, device)
        assert not st.any()
        for j, (r3, r2, lp) in enumerate(refs):
            assert np.array_equal(_bits(out[j][0]), _bits(r3)), (j, E.first_difference(_host(out[j][0]), r3))
            assert np.array_equal(_bits(out[j][1]), _bits(r2)), (j, E.first_difference(_host(out[j][1]), r2))
            assert np.array_equal(out[j][2], lp)
    assert refs[-1][0].shape[0] > 500 and refs[-1][1].shape[0] > 20


# ---- 6. the contract -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("outlier", ["RADIUS", "STATISTICAL"])
def test_launches_and_host_waits_do_not_follow_the_number_of_scans(outlier):
    big = small_vlp16()
    two = [big, small_vlp16(seed=9, azimuths=100)]
    seven = [tiny(257), big, small_vlp16(seed=9, azimuths=100), tiny(255), small_vlp16(seed=4, azimuths=60), tiny(256), small_vlp16(seed=6, azimuths=200)]
    pf = _pf(dict(R.LAUNCH, outlier_removal_method=outlier, statistical_mean_k=10))
    counts = []
    for scans in (two, seven):
        heads = [HEADS[j % 4] for j in range(len(scans))]
        out, st = run_batch(pf, scans, heads, device=True)
        assert not st.any() and all(o[1].shape[0] > 0 for o in out)
        counts.append(pf.batch_counts())
    print(f"{outlier}: counts of 2 scans {counts[0].tolist()}, of 7 scans {counts[1].tolist()}")
    assert counts[0][0] == counts[1][0] and counts[0][1] == counts[1][1]
    assert counts[0][0] > 0 and counts[0][1] >= 6                   # distance, voxel boxes, voxel sizes, outlier, height, normal
    assert counts[0][2] == 2 and counts[1][2] == 7 and counts[0][3] == 2 and counts[1][3] == 7
    assert counts[0][4] == 0 and counts[1][4] == 0 and counts[0][5] == 1 and counts[1][5] == 1
    assert counts[0][6] == 4 and counts[1][6] == 14                 # two indices per scan: the outlier pass's and the normal pass's


def test_approx_voxelgrid_is_served_per_scan_with_the_same_results():
    scans = [small_vlp16(), tiny(257), small_vlp16(seed=9, azimuths=100)]
    heads = [HEADS[3], HEADS[0], HEADS[1]]
    pf = _pf(dict(R.LAUNCH, downsample_method="APPROX_VOXELGRID"))
    out, st = run_batch(pf, scans, heads)
    assert pf.batch_counts()[4] == len(scans)
    assert_equals_single(pf, scans, heads, out, st)


def test_the_per_query_walk_is_served_per_scan_with_the_same_results(monkeypatch):
    scans, heads = mixed_batch()
    leaf, _ = run_batch(_pf(R.LAUNCH), scans, heads)
    monkeypatch.setenv("DGS_KNN_LEAF", "0")                          # read when the handle is created
    pf = _pf(R.LAUNCH)
    out, st = run_batch(pf, scans, heads)
    assert pf.batch_counts()[4] == len(scans)
    assert_equals_single(pf, scans, heads, out, st)
    for x, y in zip(out, leaf):                                      # the same sets from either search, and the consumers sort them
        assert np.array_equal(_bits(x[0]), _bits(y[0])) and np.array_equal(_bits(x[1]), _bits(y[1]))


def test_chunks_by_a_point_budget_give_the_same_results(monkeypatch):
    scans, heads = mixed_batch()
    whole, _ = run_batch(_pf(R.DEFAULTS), scans, heads)
    monkeypatch.setenv("DGS_PREFILTER_BATCH_POINTS", "400")          # 0 + 1 + 63 + 64 + 65 | 255 | 256 | 257 | 3,672
    pf = _pf(R.DEFAULTS)
    out, st = run_batch(pf, scans, heads)
    assert pf.batch_counts()[5] == 5 and pf.batch_counts()[2] == len(scans)
    assert st.tolist() == [0, 1, 0, 0, 0, 0, 0, 0, 0]
    for x, y in zip(out, whole):
        assert np.array_equal(_bits(x[0]), _bits(y[0])) and np.array_equal(_bits(x[1]), _bits(y[1])) and np.array_equal(x[2], y[2])
    assert pf.batch_statistics()[-1, 3] > 1000 and not pf.batch_statistics()[1].any()


def test_an_empty_batch_launches_nothing():
    pf = _pf(R.LAUNCH)
    out, st = pf.filter_scan_batch([])
    assert out == [] and st.shape == (0,)
    assert not pf.batch_counts().any()                               # no launch, no wait, nothing listed
    pf.filter_scan_batch([tiny(65)])
    assert pf.batch_counts()[0] > 0
    pf.filter_scan_batch([])
    assert not pf.batch_counts().any()
    assert pf.batch_statistics().shape == (0, 4)


def test_the_single_calls_hooks_report_nothing_after_a_batch():
    pf = _pf(R.DEFAULTS)
    pf.filter_scan(small_vlp16())
    assert pf.statistics()[0].shape[0] > 0 and pf.normals()[0].shape[0] > 0
    pf.filter_scan_batch([small_vlp16()])
    assert pf.statistics()[0].shape[0] == 0 and pf.normals()[0].shape[0] == 0


def test_registration_sharing_the_handle_keeps_target_source_and_result():
    from delta_graph_slam_amd.registration import Registration
    tgt, src, _ = synth.planar_pair(n=16384)
    ref = Registration("NDT_OMP", ndt_resolution=1.0)
    ref.setInputTarget(tgt)
    ref.setInputSource(src)
    ref.align()
    r = Registration("NDT_OMP", ndt_resolution=1.0)
    r.setInputTarget(tgt)
    r.setInputSource(src)
    r.align()
    T, fit = r.getFinalTransformation().copy(), r.getFitnessScore()
    before, vox_before = r.counts(), r.ndt_voxels()
    pf = _pf(R.DEFAULTS, registration=r)
    scans, heads = mixed_batch()
    run_batch(pf, scans, heads)
    run_batch(pf, scans, heads, device=True)
    assert r.counts() == before
    assert np.array_equal(r.getFinalTransformation(), T) and r.getFitnessScore() == fit                    # the last result
    vox_after = r.ndt_voxels()
    assert np.array_equal(vox_before["keys"], vox_after["keys"]) and np.array_equal(vox_before["mean"], vox_after["mean"])   # the target
    r.align()                                                                                              # the source
    assert np.array_equal(r.getFinalTransformation(), ref.getFinalTransformation())


def test_a_handle_that_ran_a_large_batch_gives_a_small_batch_the_bits_of_a_fresh_one():
    used = _pf(R.DEFAULTS)
    large = [small_vlp16(seed=s, azimuths=512) for s in (1, 2, 3, 4, 5, 6)]
    used.filter_scan_batch(large)
    scans, heads = mixed_batch()
    scans, heads = scans[3:] + [tiny(33)], heads[3:] + [HEADS[2]]
    a, sa = run_batch(used, scans, heads)
    b, sb = run_batch(_pf(R.DEFAULTS), scans, heads)
    assert np.array_equal(sa, sb)
    for x, y in zip(a, b):
        assert np.array_equal(_bits(x[0]), _bits(y[0])) and np.array_equal(_bits(x[1]), _bits(y[1]))
    assert a[-2][0].shape[0] > 500


def test_a_table_that_outgrows_its_pinned_block_between_calls():
    """1 scan, then 64 scans of at most 64 points -- 64 entries of 144 bytes, more than the bytes + bytes / 4 + 4 KiB the first call left
    the pinned block with -- then the 1 scan again, all on one handle: every call gives the bits, statuses and counts of a fresh handle"""
    one = ([small_vlp16(seed=9, azimuths=100)], [HEADS[3]])
    many = ([tiny(1 + (7 * i) % 64) for i in range(64)], [HEADS[i % 4] for i in range(64)])
    used = _pf(R.LAUNCH)
    for scans, heads in (one, many, one):
        fresh = _pf(R.LAUNCH)
        a, sa = run_batch(used, scans, heads)
        b, sb = run_batch(fresh, scans, heads)
        assert np.array_equal(sa, sb) and np.array_equal(used.batch_counts(), fresh.batch_counts()), (used.batch_counts(), fresh.batch_counts())
        for x, y in zip(a, b):
            assert np.array_equal(_bits(x[0]), _bits(y[0])) and np.array_equal(_bits(x[1]), _bits(y[1])) and np.array_equal(x[2], y[2])
        assert sum(o[0].shape[0] for o in a) > 0


# ---- 7. fleet hand-over ----------------------------------------------------------------------------------------------------------
def test_batch_outputs_feed_the_odometry_fleet_as_the_single_calls_do():
    from delta_graph_slam_amd.odometry import ScanMatchingOdometryFleet
    from delta_graph_slam_amd.registration import Registration
    base, _ = synth.vlp16_stream(n_frames=3)
    moved = synth.make_transform((3.0, -2.0, 0.5), (0.02, -0.01, 0.7))
    streams = [base, [synth.apply_transform(moved, c) for c in base]]
    down = {"downsample_method": "VOXELGRID", "downsample_resolution": 0.4}
    pf = _pf(R.LAUNCH)

    def fleet():
        reg = Registration("FAST_GICP", gicp_max_correspondence_distance=2.0, transformation_epsilon=0.1, batch_independent=True)
        return ScanMatchingOdometryFleet(reg, 2, [dict(down), dict(down)])
    fa, fb = fleet(), fleet()
    for k in range(3):
        frames = [_dev(streams[s][k]) for s in range(2)]
        avs = [TYPICAL, None]
        out, st = pf.filter_scan_batch(frames, avs, [M, M])
        assert not st.any() and out[0][0].is_cuda and out[0][0].shape[0] > 1000
        odo_a = fa.step([0.1 * k] * 2, [out[0][0], out[1][0]])
        singles = [pf.filter_scan(frames[s], avs[s], M)[0] for s in range(2)]
        odo_b = fb.step([0.1 * k] * 2, singles)
        assert np.array_equal(odo_a, odo_b), k
    assert not np.array_equal(odo_a[0], np.eye(4, dtype=np.float32))


# ---- 8. C++ driver -----------------------------------------------------------------------------------------------------------------
def test_cpp_driver_matches_the_python_path(tmp_path):
    exe = str(tmp_path / "prefilter_batch_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "tests", "stub_pcl"), "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "prefilter_batch_driver.cpp"), "-o", exe,
                           os.path.join(ROOT, "delta_graph_slam_amd", "libdgs_reg.so"), "-Wl,-rpath," + os.path.join(ROOT, "delta_graph_slam_amd"),
                           "-Wl,-rpath,/opt/rocm/lib"])
    scans = [small_vlp16(), tiny(257), tiny(1), small_vlp16(seed=9, azimuths=100)]
    heads = [HEADS[3], HEADS[1], HEADS[0], HEADS[2]]
    args = [exe, str(len(scans))]
    for j, (c, hd) in enumerate(zip(scans, heads)):
        inp = str(tmp_path / f"in{j}.bin")
        # pcl::PointXYZ carries no fourth float: the driver's points have w = 1, as HipPrefilter packs them
        c = c.copy()
        c[:, 3] = 1.0
        scans[j] = c
        c.tofile(inp)
        args += [inp, str(tmp_path / f"o3_{j}.bin"), str(tmp_path / f"o2_{j}.bin"), "none" if hd[0] is None else ",".join(repr(v) for v in hd[0]),
                 "none" if hd[1] is None else ",".join(repr(float(v)) for v in hd[1].reshape(16))]
    args += ["outlier_removal_method=STATISTICAL", "statistical_mean_k=20", "scan_period=0.1"]
    res = json.loads(subprocess.check_output(args, timeout=120).decode().strip().splitlines()[-1])
    pf = _pf(R.DEFAULTS)
    out, st = run_batch(pf, scans, heads)
    assert res["status"] == st.tolist() and st.tolist() == [0, 0, 1, 0]
    for j in range(len(scans)):
        g3 = np.fromfile(str(tmp_path / f"o3_{j}.bin"), np.float32).reshape(-1, 4)
        g2 = np.fromfile(str(tmp_path / f"o2_{j}.bin"), np.float32).reshape(-1, 4)
        assert res["n3d"][j] == out[j][0].shape[0] and res["n2d"][j] == out[j][1].shape[0]
        # the driver writes x, y, z, 1: the fourth float of a point that went through no transform is 1 as well here
        assert np.array_equal(g3[:, :3], out[j][0][:, :3]) and np.array_equal(g2[:, :3], out[j][1][:, :3])
        assert np.array_equal(res["lidar"][j], out[j][2].tolist())
    assert res["n3d"][0] > 500
