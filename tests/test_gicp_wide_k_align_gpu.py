"""-m gpu tests of whole registrations at gicp_correspondence_randomness = 40 and 64 (the wide k-NN and covariance kernels, 32 < k <= 64):
parity with the oracles, the batch entry points against the single align under batch_independent, and GICP_HIP's rule that a cloud of
fewer than k points fails only the pairs that name it."""
import numpy as np
import pytest

from delta_graph_slam_amd import synth
from tests.helpers import TOL_ROT, TOL_TRANS, pose_error

pytestmark = pytest.mark.gpu

_PAIR = {}


def _pair():
    """a planar_pair slice: 4,096 target points, 3,000 source points, the perturbation tests/test_gicp_gpu.py uses (planar_pair's own)"""
    if not _PAIR:
        tgt, src, _ = synth.planar_pair(n=4096)
        _PAIR["p"] = (np.ascontiguousarray(tgt, np.float32), np.ascontiguousarray(src[:3000], np.float32))
    return _PAIR["p"]


@pytest.mark.parametrize("k", [40, 64])
def test_fast_gicp_matches_the_oracle(oracle_lib, k):
    from delta_graph_slam_amd.registration import Registration
    tgt, src = _pair()
    o = oracle_lib.GicpOracle(max_correspondence_distance=2.0, k_correspondences=k)
    o.set_target(tgt)
    o.set_source(src)
    ro = o.align()
    r = Registration("FAST_GICP", gicp_max_correspondence_distance=2.0, gicp_correspondence_randomness=k)
    r.setInputTarget(tgt)
    r.setInputSource(src)
    r.align()
    assert r.hasConverged() == ro["converged"] and r.last_result.iterations == ro["iterations"]
    dt, dr = pose_error(r.getFinalTransformation(), ro["T"])
    assert dt <= TOL_TRANS and dr <= TOL_ROT, (dt, dr)


@pytest.mark.parametrize("search,k", [("DIRECT1", 40), ("DIRECT7", 40), ("DIRECT1", 64)])
def test_fast_vgicp_matches_the_oracle(oracle_lib, search, k):
    from delta_graph_slam_amd import _lib as L
    from delta_graph_slam_amd.registration import Registration
    tgt, src = _pair()
    o = oracle_lib.VgicpOracle(resolution=1.0, search_method=search, k_correspondences=k)
    o.set_target(tgt)
    o.set_source(src)
    ro = o.align()
    r = Registration("FAST_VGICP", vgicp_resolution=1.0, vgicp_search_method=L.VGICP_SEARCH[search], gicp_correspondence_randomness=k)
    r.setInputTarget(tgt)
    r.setInputSource(src)
    r.align()
    assert r.hasConverged() == ro["converged"] and r.last_result.iterations == ro["iterations"]
    dt, dr = pose_error(r.getFinalTransformation(), ro["T"])
    assert dt <= TOL_TRANS and dr <= TOL_ROT, (dt, dr)


@pytest.mark.parametrize("k", [40, 64])
def test_gicp_hip_matches_the_restatement(k):
    from oracle import oracle as orc
    from delta_graph_slam_amd.registration import Registration
    from tests import pcl_gicp_reference as ref
    tgt, src = _pair()
    want = ref.gicp_align(orc, tgt, src, k=k)
    r = Registration("GICP_HIP", gicp_correspondence_randomness=k)
    r.setInputTarget(tgt)
    r.setInputSource(src)
    r.align()
    assert r.hasConverged() == want["converged"] and r.last_result.iterations == want["iterations"]
    dt, dr = pose_error(r.getFinalTransformation(), want["T"])
    assert dt <= TOL_TRANS and dr <= TOL_ROT, (dt, dr)


@pytest.mark.parametrize("k", [40, 64])
def test_gicp_hip_covariances_match_the_restatement(k):
    """pg_cov_wide_kernel (the list sorted in LDS, sums in ascending index order) against pcl_gicp_reference.covariances, with the filter
    and the bound tests/test_pcl_gicp_gpu.py::test_covariances_match_the_restatement uses at k = 20: a dropped or doubled neighbour moves
    an entry by ~1 / k of the largest, the bound is 1e-9 of it."""
    from oracle import oracle as orc
    from delta_graph_slam_amd.registration import Registration
    from tests import pcl_gicp_reference as ref
    tgt, src = _pair()
    r = Registration("GICP_HIP", gicp_correspondence_randomness=k)
    r.setInputTarget(tgt)
    r.setInputSource(src)
    for which, cloud in (("source", src), ("target", tgt)):
        dev = r.gicp_covariances(which)
        want, sv = ref.covariances(orc, cloud, k, 1e-3)
        ok = np.isfinite(sv).all(axis=1) & ((sv[:, 1] - sv[:, 2]) > 1e-3 * sv[:, 0])     # the eps direction is well defined
        assert ok.mean() > 0.9
        err = np.abs(dev[ok] - want[ok]).max(axis=(1, 2))
        print(f"k {k} {which}: {int(ok.sum())} of {ok.size} points, max error {err.max():.3g} of {np.abs(want[ok]).max():.3g}")
        assert err.max() <= 1e-9 * np.abs(want[ok]).max(), err.max()


def _sources_and_guesses():
    tgt, src = _pair()
    rng = np.random.default_rng(11)
    sources = [src.copy(), src[:1777].copy(), src[rng.permutation(3000)[:2500]].copy()]
    guesses = [np.eye(4, dtype=np.float32)] + [synth.make_transform(rng.uniform(-0.1, 0.1, 3), rng.uniform(-0.01, 0.01, 3)).astype(np.float32)
                                               for _ in range(2)]
    return tgt, sources, guesses


@pytest.mark.parametrize("method", ["FAST_GICP", "GICP_HIP"])
def test_batch_entry_points_equal_the_single_align_bit_for_bit(method):
    """batch_independent = True: align_batch and align_pairs give the bits of one align per pair, here at k = 40"""
    from delta_graph_slam_amd.registration import Registration
    tgt, sources, guesses = _sources_and_guesses()
    r = Registration(method, gicp_correspondence_randomness=40)
    r.set_batch_independent(True)
    r.setInputTarget(tgt)
    batch = r.align_batch(sources, guesses, compute_fitness=False)
    pairs = r.align_pairs([tgt] * len(sources), sources, guesses, compute_fitness=False)
    for i, (s, g) in enumerate(zip(sources, guesses)):
        r.setInputTarget(tgt)
        r.setInputSource(s)
        r.align(g)
        T = r.getFinalTransformation()
        for res in (batch[i], pairs[i]):
            assert np.array_equal(res["T"], T), (method, i)
            assert res["converged"] == r.hasConverged() and res["iterations"] == r.last_result.iterations
            assert res["evaluations"] == r.last_result.evaluations


def test_gicp_hip_target_of_39_points_fails_only_its_own_pairs():
    from delta_graph_slam_amd.registration import Registration
    tgt, sources, guesses = _sources_and_guesses()
    short = tgt[:39].copy()
    r = Registration("GICP_HIP", gicp_correspondence_randomness=40)
    r.set_batch_independent(True)
    targets = [tgt, short, tgt]
    res = r.align_pairs(targets, sources, guesses, compute_fitness=False)
    alone = r.align_pairs([tgt, tgt], [sources[0], sources[2]], [guesses[0], guesses[2]], compute_fitness=False)
    assert res[1]["status"] != 0 and not res[1]["converged"]
    for got, want in ((res[0], alone[0]), (res[2], alone[1])):
        assert got["status"] == 0 and got["converged"]
        assert np.array_equal(got["T"], want["T"]) and got["iterations"] == want["iterations"]
