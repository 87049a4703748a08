"""-m gpu tests of dgs_params.gicp_cov_jacobi_svd = 2 (DGS_GICP_COV_UPSTREAM_ORDER): FAST_GICP / FAST_VGICP covariances formed in the CPU
restatement's operation order -- neighbours in ascending (float squared distance, index) order, mean and covariance summed one after another
in double, JacobiSVD -- so that the six stored entries of every covariance are the oracle's (cov_svd = 1) bit for bit."""
import contextlib
import hashlib
import os

import numpy as np
import pytest

from delta_graph_slam_amd import synth
from tests.helpers import TOL_ROT, TOL_TRANS, pose_error
from tests.test_fuzz_gpu import _cases

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "gicp_cov_modes_parent.npz")
REGS = ["NONE", "PLANE", "MIN_EIG", "NORMALIZED_MIN_EIG", "FROBENIUS"]
SIX = (np.array([0, 0, 0, 1, 1, 2]), np.array([0, 1, 2, 1, 2, 2]))   # the device's stored entries: row-major upper triangle
UPSTREAM_ORDER = 2
# launch shape of gicp_cov_ordered_kernel (csrc/gicp_cov_ordered.hip): 4 rounds of 8 points per wave, 4 waves per workgroup
PER_WAVE, PER_BLOCK = 32, 128


@contextlib.contextmanager
def _knn_leaf(leaf):
    """The k-NN search is chosen when the handle is made (DGS_KNN_LEAF: 1 = one wave per index leaf, 0 = the per-query walk)."""
    old = os.environ.get("DGS_KNN_LEAF")
    os.environ["DGS_KNN_LEAF"] = "1" if leaf else "0"
    try:
        yield
    finally:
        if old is None:
            del os.environ["DGS_KNN_LEAF"]
        else:
            os.environ["DGS_KNN_LEAF"] = old


def _gaussian(rng, n, scale=3.0):
    c = np.ones((n, 4), np.float32)
    c[:, :3] = rng.normal(size=(n, 3)) * scale
    return c


def _make_clouds():
    """The small clouds of tests/test_gicp_gpu.py::_knn_cases (same formulas), the slot edges of the 8-lane k-NN layout, and sizes at the
    kernel's points-per-wave and points-per-workgroup boundaries."""
    rng = np.random.default_rng(5)
    out = []
    for n in (11, 63, 64, 65, 71, 1000, 4099):           # fewer points than k, fewer than 8 leaves, exactly 8, partial last leaf
        out.append((f"gaussian {n}", _gaussian(rng, n), 20))
    c = np.ones((6000, 4), np.float32)
    c[:, :3] = np.round(rng.normal(size=(6000, 3)) * 4) / 4     # quarter-lattice: duplicates, ties at the k-th distance
    out.append(("lattice duplicates", c, 20))
    c = np.ones((3000, 4), np.float32)
    c[:, 0] = np.linspace(-50, 50, 3000)
    c[:, 1:3] = 0
    out.append(("collinear", c, 20))
    c = np.ones((3000, 4), np.float32)
    c[:, :3] = np.float32([1.5, -2.25, 0.125])                  # one point 3,000 times
    out.append(("identical points", c, 20))
    out.append(("k = 32 of 100", _gaussian(rng, 100, 1.0), 32))
    edges = _gaussian(rng, 4099)
    for k in (5, 8, 9, 16, 17, 24, 25, 32):                     # a slot row of the 8-lane groups full, one over, the last one full
        out.append((f"4,099 points, k = {k}", edges, k))
    for n in (PER_WAVE - 1, PER_WAVE, PER_WAVE + 1, PER_BLOCK - 1, PER_BLOCK, PER_BLOCK + 1, 2 * PER_BLOCK + 1):
        out.append((f"launch edge {n}", _gaussian(rng, n), 20))
    return out


_CLOUDS = _make_clouds()
_ORACLE = {}


def _pair_of(cloud):
    """target = the cloud, source = the same points in reverse order (other indices: ties between equal distances break the other way)"""
    return cloud, np.ascontiguousarray(cloud[::-1])


def _oracle_covs(oracle_lib, name, cloud, k, reg):
    key = (name, reg)
    if key not in _ORACLE:
        tgt, src = _pair_of(cloud)
        o = oracle_lib.GicpOracle(regularization=reg, k_correspondences=k, cov_svd=1)
        o.set_target(tgt)
        o.set_source(src)
        got = {"source": o.covariances("source"), "target": o.covariances("target")}
        for v in got.values():
            v.setflags(write=False)
        _ORACLE[key] = got
    return _ORACLE[key]


def _device(method, leaf, **params):
    from delta_graph_slam_amd.registration import Registration
    with _knn_leaf(leaf):
        return Registration(method, **params)


@pytest.mark.parametrize("leaf", [1, 0])
@pytest.mark.parametrize("reg", REGS)
def test_covariances_equal_the_oracle_bit_for_bit(oracle_lib, reg, leaf):
    """Mode 2 against GicpOracle(cov_svd=1): np.array_equal on the six stored entries, source and target, every point, under both k-NN
    searches.  On the parent commit the value 2 runs mode 1's 8-lane tree sums and this fails (last-bit differences of the sums on almost
    every cloud, 2e-3 on the rank-deficient neighbourhoods of the lattice, the line and the repeated point).
    equal_nan: one point repeated 3,000 times has an exactly zero covariance, and NORMALIZED_MIN_EIG then divides 0 by 0 -- the oracle's
    six entries are NaN there, which no array equals under the plain comparison, the oracle's own included.  A NaN must stand exactly where
    the oracle has one; every other entry is compared bit for bit as before."""
    from delta_graph_slam_amd import _lib as L
    bad = []
    for name, cloud, k in _CLOUDS:
        want = _oracle_covs(oracle_lib, name, cloud, k, reg)
        tgt, src = _pair_of(cloud)
        r = _device("FAST_GICP", leaf, gicp_regularization=L.GICP_REG[reg], gicp_correspondence_randomness=k, gicp_cov_jacobi_svd=UPSTREAM_ORDER)
        r.setInputTarget(tgt)
        r.setInputSource(src)
        for which in ("source", "target"):
            got = r.gicp_covariances(which, cloud.shape[0])[:, SIX[0], SIX[1]]
            ref = want[which][:, SIX[0], SIX[1]]
            if not np.array_equal(got, ref, equal_nan=True):
                rows = np.flatnonzero(((got != ref) & ~(np.isnan(got) & np.isnan(ref))).any(axis=1))
                with np.errstate(invalid="ignore", divide="ignore"):
                    rel = float(np.nanmax(np.abs(got - ref) / np.abs(ref).max()))
                bad.append((name, which, int(rows.size), int(rows[0]), rel))
        r.close()
    print(f"reg {reg} leaf {leaf}: {len(_CLOUDS)} clouds, mismatching (cloud, side, points, first point, largest relative difference): {bad}")
    assert not bad, bad


def test_vgicp_point_covariances_equal_the_oracle_bit_for_bit(oracle_lib):
    """FAST_VGICP takes its point covariances (source, and target before the voxel averages) through the same pass."""
    name, cloud, k = next(c for c in _CLOUDS if c[0] == "lattice duplicates")
    want = _oracle_covs(oracle_lib, name, cloud, k, "PLANE")
    tgt, src = _pair_of(cloud)
    r = _device("FAST_VGICP", 1, gicp_correspondence_randomness=k, gicp_cov_jacobi_svd=UPSTREAM_ORDER)
    r.setInputTarget(tgt)
    r.setInputSource(src)
    for which in ("source", "target"):
        assert np.array_equal(r.gicp_covariances(which, cloud.shape[0])[:, SIX[0], SIX[1]], want[which][:, SIX[0], SIX[1]]), which


@pytest.mark.parametrize("leaf", [1, 0])
def test_non_finite_points_keep_the_finite_mask_of_mode_0(leaf):
    """The oracle's tree is not specified for non-finite points: only the set of points with a finite covariance is compared, with mode 0's."""
    from delta_graph_slam_amd import _lib as L
    rng = np.random.default_rng(5)
    c = _gaussian(rng, 5000, 2.0)
    c[rng.choice(5000, 40, replace=False), rng.integers(0, 3, 40)] = np.nan
    c[rng.choice(5000, 10, replace=False), 0] = np.inf
    for reg in ("NONE", "PLANE"):
        masks = {}
        for mode in (0, UPSTREAM_ORDER):
            r = _device("FAST_GICP", leaf, gicp_regularization=L.GICP_REG[reg], gicp_cov_jacobi_svd=mode)
            r.setInputTarget(c)
            r.setInputSource(c)
            masks[mode] = np.isfinite(r.gicp_covariances("source", 5000)).all(axis=(1, 2))
        assert np.array_equal(masks[0], masks[UPSTREAM_ORDER]), (reg, int((masks[0] != masks[UPSTREAM_ORDER]).sum()))
        assert masks[0].sum() >= 4950


@pytest.mark.parametrize("method", ["FAST_GICP", "FAST_VGICP"])
def test_gicp_family_sweep_in_upstream_order(oracle_lib, method):
    """The scenes of tests/test_fuzz_gpu.py::test_gicp_family_sweep (seed 23, 24 scenes, the same k / dmax / resolution / search draws) with
    mode 2 against the oracle's cov_svd = 1, under that test's own tolerances: error and Hessian within 1e-9, same `converged`, pose within
    1e-4 m / 1e-5 rad.  Scenes 10 and 14 of the FAST_GICP sweep (duplicated source points; k = 10 and k = 5 in this draw) decide: there JacobiSVD and the
    symmetric eigen-decomposition are different answers (figures of the CPU oracle alone) -- 2.7 % and 1.6 % of the oracle's covariances move by 2e-3 between cov_svd 0 and 1,
    its final pose by 5.1e-5 m / 6.8e-6 rad and 4.4e-5 m / 1.2e-5 rad (the second outside the 1e-5 rad gate) -- and mode 1's tree sums cost
    6.5e-3 relative on the linearisation sums; only JacobiSVD fed the oracle's bits stays inside 1e-9."""
    from delta_graph_slam_amd import _lib as L
    from delta_graph_slam_amd.registration import Registration
    worst = [0.0, 0.0, 0.0, 0.0]
    for c, rng, tgt, src, T in _cases(24, 23):
        k = int(rng.choice([5, 10, 20]))
        if method == "FAST_GICP":
            dmax = float(rng.choice([0.5, 1.0, 2.5]))
            o = oracle_lib.GicpOracle(max_correspondence_distance=dmax, k_correspondences=k, cov_svd=1)
            r = Registration(method, gicp_max_correspondence_distance=dmax, gicp_correspondence_randomness=k, gicp_cov_jacobi_svd=UPSTREAM_ORDER)
        else:
            res = float(rng.choice([0.6, 1.0, 1.5]))
            search = str(rng.choice(["DIRECT1", "DIRECT7", "DIRECT27"]))
            o = oracle_lib.VgicpOracle(resolution=res, search_method=search, k_correspondences=k, cov_svd=1)
            r = Registration(method, vgicp_resolution=res, vgicp_search_method=L.VGICP_SEARCH[search], gicp_correspondence_randomness=k,
                             gicp_cov_jacobi_svd=UPSTREAM_ORDER)
        o.set_target(tgt)
        o.set_source(src)
        r.setInputTarget(tgt)
        r.setInputSource(src)
        Tp = synth.make_transform(T[:3, 3] + rng.uniform(-0.1, 0.1, 3), rng.uniform(-0.02, 0.02, 3))
        Tp[:3, :3] = Tp[:3, :3] @ T[:3, :3]
        eo, Ho, bo = o.linearize(Tp)
        eg, Hg, bg = r.gicp_linearize(Tp)
        ro = o.align(T.astype(np.float32))
        r.align(T.astype(np.float32))
        dt, dr = pose_error(r.getFinalTransformation(), ro["T"])
        figs = (abs(eo - eg) / abs(eo), np.abs(Ho - Hg).max() / np.abs(Ho).max(), dt, dr)
        print(f"{method} scene {c}: k {k}, error {figs[0]:.2e}, Hessian {figs[1]:.2e}, pose {dt:.2e} m / {dr:.2e} rad")
        worst = [max(a, b) for a, b in zip(worst, figs)]
        tol = 1e-9
        assert abs(eo - eg) <= tol * abs(eo) + 1e-9, (c, abs(eo - eg) / abs(eo))
        assert np.abs(Ho - Hg).max() <= tol * np.abs(Ho).max(), c
        assert r.hasConverged() == ro["converged"], c
        assert dt <= TOL_TRANS and dr <= TOL_ROT, (c, dt, dr)
    print(f"{method} worst: error {worst[0]:.2e}, Hessian {worst[1]:.2e}, pose {worst[2]:.2e} m / {worst[3]:.2e} rad")


def _mode_pair():
    """The 4,099-point pair of the golden record (tests/golden/gicp_cov_modes_parent.npz was made from exactly this)."""
    tgt, src, Tgt = synth.planar_pair(n=4099)
    return np.ascontiguousarray(tgt), np.ascontiguousarray(src)


def record_modes(lib_path=None):
    """Raw (NONE) and PLANE covariances of both clouds and the final transform of a FAST_GICP align, for modes 0 and 1: what the golden
    file holds as SHA-256 digests of the arrays' bytes plus the arrays' first 512 points (a mismatch can be located)."""
    from delta_graph_slam_amd import _lib as L
    from delta_graph_slam_amd.registration import Registration
    tgt, src = _mode_pair()
    out = {}
    for mode in (0, 1):
        for reg in ("NONE", "PLANE"):
            r = Registration("FAST_GICP", lib_path=lib_path, gicp_max_correspondence_distance=2.0, gicp_regularization=L.GICP_REG[reg], gicp_cov_jacobi_svd=mode)
            r.setInputTarget(tgt)
            r.setInputSource(src)
            for which, n in (("source", src.shape[0]), ("target", tgt.shape[0])):
                a = np.ascontiguousarray(r.gicp_covariances(which, n)[:, SIX[0], SIX[1]])
                out[f"cov_{reg}_{which}_mode{mode}_sha256"] = np.frombuffer(hashlib.sha256(a.tobytes()).digest(), np.uint8)
                out[f"cov_{reg}_{which}_mode{mode}_head"] = a[:512].copy()
            if reg == "PLANE":
                r.align()
                out[f"T_mode{mode}"] = np.asarray(r.getFinalTransformation()).copy()
                out[f"iterations_mode{mode}"] = np.int64(r.last_result.iterations)
            r.close()
    return out


def test_modes_0_and_1_are_the_parent_commits():
    """Modes 0 and 1 keep their kernels: raw and PLANE covariances of both clouds (every point: SHA-256 of the six stored entries; the first
    512 points also entry by entry) and the final transform equal what a build of the parent commit gave on an MI355X."""
    assert os.path.exists(GOLDEN), "tests/golden/gicp_cov_modes_parent.npz is missing"
    want = np.load(GOLDEN)
    got = record_modes()
    assert sorted(want.files) == sorted(got)
    for key in sorted(got):
        assert np.array_equal(np.asarray(got[key]), want[key]), key


def test_batch_on_resident_clouds_equals_single_aligns_bit_for_bit():
    """Mode 2 through the batch path and resident clouds (whose cached covariances are of their handle's mode): align_batch over three
    4,099-point candidates equals three single aligns -- transform, iterations, evaluations."""
    from delta_graph_slam_amd.registration import Registration
    tgt, src, _ = synth.planar_pair(n=4099)
    rng = np.random.default_rng(7)
    sources, guesses = [], []
    for _ in range(3):
        G = synth.make_transform(rng.uniform(-0.1, 0.1, 3), rng.uniform(-0.01, 0.01, 3))
        s_ = src.copy()
        s_[:, :3] = (src[:, :3].astype(np.float64) @ G[:3, :3].T + G[:3, 3]).astype(np.float32)
        s_[:400] = s_[400:800]                               # duplicated points: rank-deficient neighbourhoods
        sources.append(np.ascontiguousarray(s_[rng.permutation(4099)]))
        guesses.append(synth.make_transform(rng.uniform(-0.05, 0.05, 3), rng.uniform(-0.01, 0.01, 3)).astype(np.float32))
    r = Registration("FAST_GICP", gicp_max_correspondence_distance=2.0, gicp_cov_jacobi_svd=UPSTREAM_ORDER)
    dt = r.make_cloud(tgt)
    ds = [r.make_cloud(s_) for s_ in sources]
    r.setInputTarget(dt)
    res = r.align_batch(ds, guesses)
    assert all(x["status"] == 0 for x in res)
    single = Registration("FAST_GICP", gicp_max_correspondence_distance=2.0, gicp_cov_jacobi_svd=UPSTREAM_ORDER)
    single.setInputTarget(tgt)
    for k in range(3):
        single.setInputSource(sources[k])
        single.align(guesses[k])
        assert np.array_equal(res[k]["T"], single.getFinalTransformation()), k
        assert res[k]["iterations"] == single.last_result.iterations and res[k]["evaluations"] == single.last_result.evaluations, k
        assert res[k]["converged"] == single.hasConverged(), k
    # and the resident clouds serve a second batch from their cached covariances with the same answer
    again = r.align_batch(ds, guesses)
    for a, b in zip(res, again):
        assert np.array_equal(a["T"], b["T"]) and a["iterations"] == b["iterations"] and a["evaluations"] == b["evaluations"]
