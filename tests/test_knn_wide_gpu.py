"""-m gpu tests of gicp_correspondence_randomness in 33..64: the wide k-NN kernels (8 slots per lane, neighbour table of stride 64) and the
wide covariance kernels that read them.  Neighbour sets against scipy's cKDTree with ties at the k-th distance resolved to the lower index,
covariances against GicpOracle, upstream-order mode bit for bit, the limit at 64, and the (k, regularisation) key of a resident cloud's
cached covariances.  Under both wide searches: the wave-per-leaf search (the default) and the per-query walk (DGS_KNN_LEAF_WIDE=0)."""
import contextlib
import os

import numpy as np
import pytest

from delta_graph_slam_amd import synth

pytestmark = pytest.mark.gpu

WIDE_KS = (33, 40, 63, 64)
UPSTREAM_ORDER = 2
SIX = ((0, 0, 0, 1, 1, 2), (0, 1, 2, 1, 2, 2))          # the entries the device stores
REGS = ["PLANE", "FROBENIUS", "MIN_EIG", "NORMALIZED_MIN_EIG", "NONE"]
MAX_POINTS = 8192


@contextlib.contextmanager
def _leaf_wide(on):
    """the handle reads the switch when it is made"""
    old = os.environ.get("DGS_KNN_LEAF_WIDE")
    os.environ["DGS_KNN_LEAF_WIDE"] = "1" if on else "0"
    try:
        yield
    finally:
        if old is None:
            del os.environ["DGS_KNN_LEAF_WIDE"]
        else:
            os.environ["DGS_KNN_LEAF_WIDE"] = old


def _device(leaf, method="FAST_GICP", **params):
    from delta_graph_slam_amd.registration import Registration
    with _leaf_wide(leaf):
        return Registration(method, **params)


def _gaussian(rng, n, scale=3.0):
    c = np.ones((n, 4), np.float32)
    c[:, :3] = rng.normal(size=(n, 3)) * scale
    return c


_CLOUDS = {}


def _clouds():
    """The 15 clouds of tests/test_gicp_gpu.py's _knn_cases that run at k = 20 there (its last three only vary k), those of more than 8,192
    points cut to their first 8,192; clouds of n = k - 1, k, k + 1 points come with each k (_clouds_for); the index's level boundaries
    (leaf 8, fan 8); a 3,000-point slice of planar_pair; a lattice on which far more than 64 points tie at the k-th distance."""
    if _CLOUDS:
        return _CLOUDS
    from tests.test_gicp_gpu import _knn_cases
    for name, cloud, k in _knn_cases():
        if k != 20 or name.startswith("k = "):
            continue
        _CLOUDS[name] = np.ascontiguousarray(cloud[:MAX_POINTS], np.float32)
    assert len(_CLOUDS) == 15, sorted(_CLOUDS)
    rng = np.random.default_rng(77)
    for n in (63, 64, 65, 511, 512, 513):
        _CLOUDS.setdefault(f"gaussian {n}", _gaussian(rng, n))
    _CLOUDS["planar slice 3,000"] = np.ascontiguousarray(synth.planar_pair(n=4096)[1][:3000], np.float32)
    g = np.arange(12, dtype=np.float32)
    lat = np.ones((12 ** 3, 4), np.float32)
    lat[:, :3] = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3) * 0.5
    lat = np.concatenate([lat, lat[::3]])          # every third point twice: ties among duplicates and among the lattice's shells
    _CLOUDS["lattice shells"] = lat
    return _CLOUDS


def _clouds_for(k):
    out = dict(_clouds())
    rng = np.random.default_rng(1000 + k)
    for n in (k - 1, k, k + 1):
        out[f"gaussian n = {n}"] = _gaussian(rng, n)
    return out


_REF = {}


def _reference_sets(name, cloud, k):
    """(n, k) indices, -1 = nothing found: the k smallest (float squared distance, index) pairs among the finite points, the distance
    computed as the device's sqdist_rn is stated -- (dx dx + dy dy) + dz dz, every step rounded to float.  cKDTree proposes the
    candidates (every point within its k-th distance, so every tie at the k-th distance is among them); the order relation decides."""
    key = (name, k)
    if key in _REF:
        return _REF[key]
    from scipy.spatial import cKDTree
    pts = cloud[:, :3].astype(np.float32)
    n = pts.shape[0]
    fin = np.nonzero(np.isfinite(pts).all(axis=1))[0]
    out = np.full((n, k), -1, np.int64)
    if fin.size:
        fp = pts[fin]
        tree = cKDTree(fp.astype(np.float64))
        kk = min(k, fin.size)
        dist, _ = tree.query(fp.astype(np.float64), k=kk)
        dist = dist.reshape(fin.size, kk)
        radius = dist[:, -1] * (1 + 1e-6) + 1e-12
        for row, q in enumerate(fin):
            cand = np.asarray(tree.query_ball_point(fp[row].astype(np.float64), radius[row]), np.int64)
            d = fp[cand] - fp[row]
            d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]     # float32 throughout
            order = np.lexsort((fin[cand], d2))[:kk]
            out[q, :kk] = fin[cand[order]]
    _REF[key] = out
    return out


def _raw_cov_of_sets(cloud, sets, k):
    """mean and covariance over the k columns in double, columns that found nothing are zero (upstream's 4 x k matrix)"""
    pts = cloud[:, :3].astype(np.float64)
    nb = np.where((sets >= 0)[:, :, None], pts[np.clip(sets, 0, None)], 0.0)
    mean = nb.sum(axis=1) / k
    d = np.where((sets >= 0)[:, :, None], nb - mean[:, None, :], -mean[:, None, :])
    return np.einsum("nka,nkb->nab", d, d) / k


@pytest.mark.parametrize("leaf", [False, True], ids=["walk", "leaf"])
@pytest.mark.parametrize("k", WIDE_KS)
def test_neighbour_sets_are_exact(k, leaf):
    """Raw covariances (regularisation NONE: the most sensitive read-out of the sets, the hook tests/test_gicp_gpu.py uses) against the
    covariance of the reference sets.  Double sums of k terms in another order differ by k eps ~ 1e-14 of the largest entry; one wrong
    neighbour, or a tie at the k-th distance given to the higher index, moves an entry by ~1 / k of it.  Bound: 1e-11, the figure
    test_wave_per_leaf_knn_finds_the_sets_of_the_per_query_walk uses between the two searches."""
    from delta_graph_slam_amd import _lib as L
    for name, cloud in _clouds_for(k).items():
        r = _device(leaf, gicp_regularization=L.GICP_REG["NONE"], gicp_correspondence_randomness=k)
        r.setInputTarget(cloud)
        r.setInputSource(cloud)
        got = r.gicp_covariances("source", cloud.shape[0])
        finite = np.isfinite(cloud[:, :3]).all(axis=1)
        want = _raw_cov_of_sets(np.where(finite[:, None], cloud, 0).astype(np.float32), _reference_sets(name, cloud, k), k)
        scale = np.maximum(np.abs(want[finite]).max(axis=(1, 2)), 1e-300)
        err = np.abs(got[finite] - want[finite]).max(axis=(1, 2)) / scale
        zero = np.abs(want[finite]).max(axis=(1, 2)) == 0          # identical points: every entry exactly 0
        assert (np.abs(got[finite][zero]) == 0).all(), name
        print(f"k {k} leaf {leaf} {name}: n {cloud.shape[0]} max relative error {float(err[~zero].max()) if (~zero).any() else 0.0:.3g}")
        assert (~zero).sum() == 0 or err[~zero].max() < 1e-11, (name, float(err[~zero].max()), int((err[~zero] > 1e-11).sum()))


@pytest.mark.parametrize("leaf", [False, True], ids=["walk", "leaf"])
@pytest.mark.parametrize("k", WIDE_KS)
@pytest.mark.parametrize("reg", REGS)
def test_covariances_match_oracle(oracle_lib, reg, k, leaf):
    """tests/test_gicp_gpu.py::test_covariances_match_oracle at wide k under both searches, its tolerance taken from there"""
    from delta_graph_slam_amd import _lib as L
    tgt, src, _ = synth.planar_pair(n=4096)
    o = oracle_lib.GicpOracle(regularization=reg, k_correspondences=k)
    o.set_target(tgt)
    o.set_source(src)
    r = _device(leaf, gicp_regularization=L.GICP_REG[reg], gicp_correspondence_randomness=k)
    r.setInputTarget(tgt)
    r.setInputSource(src)
    for which, n in (("source", src.shape[0]), ("target", tgt.shape[0])):
        co = o.covariances(which)
        cg = r.gicp_covariances(which, n)
        err = np.abs(co - cg).max(axis=(1, 2)) / np.abs(co).max(axis=(1, 2))
        print(f"k {k} {reg} {which}: q99.9 {np.quantile(err, 0.999):.3g} max {err.max():.3g}")
        assert np.quantile(err, 0.999) < 1e-9, (which, err.max())
        assert (err > 1e-6).mean() < 1e-3        # a tie at the k-th neighbour may swap one member


@pytest.mark.parametrize("leaf", [False, True], ids=["walk", "leaf"])
def test_covariances_of_a_cloud_smaller_than_k(oracle_lib, leaf):
    """tests/test_gicp_gpu.py::test_covariances_small_k_and_tiny_cloud at wide k: missing neighbours are zero columns upstream"""
    rng = np.random.default_rng(0)
    tiny = _gaussian(rng, 11, 1.0)
    for k in (40, 64):
        o = oracle_lib.GicpOracle(k_correspondences=k)
        o.set_target(tiny)
        o.set_source(tiny)
        r = _device(leaf, gicp_correspondence_randomness=k)
        r.setInputTarget(tiny)
        r.setInputSource(tiny)
        assert np.allclose(o.covariances("source"), r.gicp_covariances("source", 11), rtol=1e-9, atol=1e-12)


@pytest.mark.parametrize("leaf", [False, True], ids=["walk", "leaf"])
@pytest.mark.parametrize("k", [33, 64])
def test_upstream_order_mode_is_bit_equal_to_the_oracle(oracle_lib, k, leaf):
    """gicp_cov_jacobi_svd = UPSTREAM_ORDER against GicpOracle(cov_svd=1): np.array_equal on every covariance of every finite point --
    the claim of tests/test_gicp_upstream_order_gpu.py at wide k, over the same clouds as the sets test."""
    from delta_graph_slam_amd import _lib as L
    for name, cloud in _clouds_for(k).items():
        finite = np.isfinite(cloud[:, :3]).all(axis=1)
        if not finite.all():
            continue          # the oracle's kd-tree takes finite clouds only; the sets test covers this cloud
        for reg in ("PLANE", "NONE"):
            o = oracle_lib.GicpOracle(regularization=reg, k_correspondences=k, cov_svd=1)
            o.set_target(cloud)
            o.set_source(cloud)
            want = o.covariances("source")
            r = _device(leaf, gicp_regularization=L.GICP_REG[reg], gicp_correspondence_randomness=k, gicp_cov_jacobi_svd=UPSTREAM_ORDER)
            r.setInputTarget(cloud)
            r.setInputSource(cloud)
            # the six stored entries, a NaN exactly where the oracle has one: tests/test_gicp_upstream_order_gpu.py's comparison
            got = r.gicp_covariances("source", cloud.shape[0])[:, SIX[0], SIX[1]]
            ref = want[:, SIX[0], SIX[1]]
            differ = (got != ref) & ~(np.isnan(got) & np.isnan(ref))
            assert np.array_equal(got, ref, equal_nan=True), (name, reg, int(differ.any(axis=1).sum()))


@pytest.mark.parametrize("method", ["FAST_GICP", "FAST_VGICP", "GICP_HIP"])
def test_k_65_is_refused_and_the_handle_goes_on_to_serve_k_40(method):
    """k = 65: status 6 (DGS_ERR_UNSUPPORTED) and a message that names 64.  The refusal is not sticky: the refused handle answers the same
    way a second time and still serves what needs no covariances (a fitness score).  GICP_HIP's k can change on a live handle, so that very
    handle goes on to align at k = 40; FAST_GICP / FAST_VGICP take k when the handle is made, so there a new handle shows k = 40."""
    from delta_graph_slam_amd.registration import DgsError, Registration
    tgt, src, _ = synth.planar_pair(n=2048)
    r = Registration(method, gicp_correspondence_randomness=65)
    for _ in range(2):
        with pytest.raises(DgsError) as ei:
            r.setInputTarget(tgt)
            r.setInputSource(src)
            r.align()
        assert ei.value.status == 6 and "64" in str(ei.value), str(ei.value)
    assert np.isfinite(r.calc_fitness_score(tgt, src))
    if method == "GICP_HIP":
        with pytest.raises(DgsError) as ei:
            r.setCorrespondenceRandomness(65)
        assert ei.value.status == 6 and "64" in str(ei.value)
        r.setCorrespondenceRandomness(40)
    else:
        r.close()
        r = Registration(method, gicp_correspondence_randomness=40)
    r.setInputTarget(tgt)
    r.setInputSource(src)
    r.align()
    assert r.hasConverged()


def test_a_resident_cloud_recomputes_between_narrow_and_wide_k():
    """one resident pair aligned with k = 20, 40, 20 on one GICP_HIP handle (its k can change on a live handle): covariances cached on
    the cloud are keyed by k, so the first and third runs are the same bits and the second reads other covariances"""
    from delta_graph_slam_amd.registration import Registration
    tgt, src, _ = synth.planar_pair(n=4096)
    r = Registration("GICP_HIP")
    t, s = r.make_cloud(tgt), r.make_cloud(src[:3000].copy())
    runs, covs = [], []
    for k in (20, 40, 20):
        r.setCorrespondenceRandomness(k)
        r.setInputTarget(t)
        r.setInputSource(s)
        r.align()
        runs.append((r.getFinalTransformation().copy(), r.last_result.iterations, r.last_result.evaluations))
        covs.append(r.gicp_covariances("target").copy())
    assert np.array_equal(runs[0][0], runs[2][0]) and runs[0][1:] == runs[2][1:]
    assert np.array_equal(covs[0], covs[2])
    assert not np.array_equal(covs[0], covs[1])
    assert (np.abs(covs[0] - covs[1]).max(axis=(1, 2)) > 0).mean() > 0.9
