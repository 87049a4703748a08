"""ICP_HIP on the GPU against the test-side restatement (tests/icp_reference.py): per-iteration kept-pair counts and incremental
transforms, iteration counts, convergence and final poses; reciprocal mode; batch independence (bit-identical results alone and in a
ragged batch, host and resident sources); the loop-detector shard through LoopDetector and RegistrationGroup; no covariance work;
edge cases."""
import numpy as np
import pytest
import torch

from delta_graph_slam_amd import _lib as L
from delta_graph_slam_amd import synth
from delta_graph_slam_amd.registration import Registration, RegistrationGroup
from helpers import TOL_ROT, TOL_TRANS, pose_error, sequential_best
import icp_reference as ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle
    return oracle


def _pair(name):
    if name == "planar":
        tgt, src, _ = synth.planar_pair(4096)
    elif name == "kitti":
        tgt, src, _ = synth.kitti_pair()
    else:
        tgt, src, _ = synth.indoor_pair()
    return np.ascontiguousarray(tgt, np.float32), np.ascontiguousarray(src, np.float32)


def _gpu_align(tgt, src, guess=None, **kw):
    reg = Registration("ICP_HIP", device=0, **kw)
    reg.setInputTarget(tgt)
    reg.setInputSource(src)
    reg.align(guess)
    return reg


def _mse_tol(n):
    """The MSE and the score are sums of n non-negative doubles of the same float d2 values on both sides, in a different order, over n:
    they differ by at most n * 2^-53 relative -- below 1e-12 up to 9,007 kept pairs, 7.3e-12 at 65,536 and 2.2e-11 at 200,000."""
    return max(1e-12, n * 2.0 ** -53)


def _compare(reg, r):
    res = reg.last_result
    Tk, mse, nc = reg.icp_trajectory(0)
    m = min(len(r["traj"]), len(nc))
    for k in range(m):
        assert nc[k] == r["traj"][k][2], (k, nc[k], r["traj"][k][2])
        assert abs(mse[k] - r["traj"][k][1]) <= _mse_tol(nc[k]) * r["traj"][k][1], (k, mse[k], r["traj"][k][1])
        assert np.abs(Tk[k] - r["traj"][k][0]).max() <= 1e-6, (k, np.abs(Tk[k] - r["traj"][k][0]).max())
    assert res.iterations == r["iterations"] and len(nc) == r["iterations"]
    assert bool(res.converged) == r["converged"]
    assert res.evaluations == r["evaluations"]
    if r["iterations"]:
        assert abs(res.score - r["score"]) <= _mse_tol(r["traj"][-1][2]) * r["score"], (res.score, r["score"])
    else:
        assert res.score == r["score"]                                       # DBL_MAX on both sides: no iteration ran
    dt, dr = pose_error(reg.getFinalTransformation(), r["T"])
    assert dt <= TOL_TRANS and dr <= TOL_ROT, (dt, dr)


@pytest.mark.parametrize("name", ["planar", "kitti", "indoor"])
@pytest.mark.parametrize("eps", [0.01, 1e-8])
def test_single_align_matches_the_restatement(orc, name, eps):
    tgt, src = _pair(name)
    reg = _gpu_align(tgt, src, transformation_epsilon=eps)
    r = ref.icp_align(orc, tgt, src, transformation_epsilon=eps)
    _compare(reg, r)
    assert reg.last_result.iterations >= 1


@pytest.mark.parametrize("name", ["planar", "kitti"])
@pytest.mark.parametrize("eps", [0.01, 1e-8])
def test_reciprocal_mode_matches_the_restatement(orc, name, eps):
    tgt, src = _pair(name)
    reg = _gpu_align(tgt, src, icp_use_reciprocal_correspondences=True, transformation_epsilon=eps)
    r = ref.icp_align(orc, tgt, src, reciprocal=True, transformation_epsilon=eps)
    _compare(reg, r)
    if eps < 1e-6:
        assert r["iterations"] > 3   # the per-round re-indexing of the working copy is exercised past its first round


@pytest.mark.parametrize("reciprocal", [False, True])
def test_non_finite_points_match_the_restatement(orc, reciprocal):
    """target[0] and a few more target points non-finite, non-finite source points: the NN index never lets them win, and the origin
    of the moment sums is the target's first FINITE point."""
    tgt, src = _pair("planar")
    tgt, src = tgt.copy(), src.copy()
    tgt[0, 0] = np.nan
    tgt[1, 1] = np.inf
    tgt[97::211, 2] = -np.inf
    src[5, 0] = np.nan
    src[33::401, 1] = np.inf
    reg = _gpu_align(tgt, src, transformation_epsilon=1e-8, icp_use_reciprocal_correspondences=reciprocal)
    r = ref.icp_align(orc, tgt, src, transformation_epsilon=1e-8, reciprocal=reciprocal)
    assert r["iterations"] > 3 and np.all(np.isfinite(r["T"]))
    assert np.all(np.isfinite(reg.getFinalTransformation()))
    _compare(reg, r)


def test_walk_order_does_not_depend_on_the_clouds_history():
    """A resident cloud that was the target of a large batch carries a k-d ordered index; as a source it must give the bits the same
    points give as a host array (the walk takes a Hilbert order of its own)."""
    tgt, src = _pair("planar")
    reg = Registration("ICP_HIP", device=0)
    cloud = reg.make_cloud(src)
    reg.setInputTarget(cloud)
    reg.align_batch([tgt] * 10, compute_fitness=False)   # >= 10 candidates: the target index of the batch is k-d ordered
    other = Registration("ICP_HIP", device=0)
    other.setInputTarget(tgt)
    guess = np.eye(4, dtype=np.float32)
    guess[:3, 3] = (0.02, -0.01, 0.03)
    a = other.align_batch([src], [guess], compute_fitness=False)[0]
    reg2 = Registration("ICP_HIP", device=0)
    reg2.setInputTarget(tgt)
    b = reg2.align_batch([cloud], [guess], compute_fitness=False)[0]
    assert np.array_equal(a["T"], b["T"]) and a["score"] == b["score"] and a["iterations"] == b["iterations"]


def _ragged_batch():
    tgt, src = _pair("planar")
    rng = np.random.default_rng(7)
    sources, guesses = [], []
    for c in range(8):
        if c == 2:
            s = np.zeros((0, 4), np.float32)                       # empty source
        elif c == 5:
            s = src[:1000].copy()
            s[:, :3] += 100.0                                        # beyond the gate
        else:
            s = src[: 4096 - 300 * c].copy()
        sources.append(s)
        g = np.eye(4, dtype=np.float32)
        g[:3, 3] = rng.normal(0, 0.05, 3)
        guesses.append(g)
    return tgt, src, sources, guesses


@pytest.mark.parametrize("resident", [False, True])
def test_batch_independence(resident):
    tgt, src, sources, guesses = _ragged_batch()
    reg = Registration("ICP_HIP", device=0)
    reg.setInputTarget(tgt)
    alone = []
    for c in (0, 3, 7):
        reg.setInputSource(sources[c])
        reg.align(guesses[c])
        r = reg.last_result
        alone.append((c, reg.getFinalTransformation().copy(), r.score, r.iterations, r.converged))
    srcs = [reg.make_cloud(s) for s in sources] if resident else sources
    out = reg.align_batch(srcs, guesses, compute_fitness=True)
    for c, T, score, iters, conv in alone:
        assert np.array_equal(out[c]["T"], T)
        assert out[c]["score"] == score and out[c]["iterations"] == iters and out[c]["converged"] == bool(conv)
    assert out[2]["status"] == 4   # DGS_ERR_NO_SOURCE
    assert not out[2]["converged"] and np.array_equal(out[2]["T"], guesses[2])
    assert out[5]["status"] == 0 and not out[5]["converged"] and out[5]["iterations"] == 0 and out[5]["evaluations"] == 1
    assert np.array_equal(out[5]["T"], guesses[5])


def test_loop_shard_through_loop_detector_and_group(orc):
    from delta_graph_slam_amd.loop_detector import KeyFrame, LoopDetector
    from delta_graph_slam_amd.transforms import transform3Dto2D
    tgt, cands, gs, _ = synth.loop_batch(n_candidates=32, n_points=65536, seed=40, distinct_scans=32)
    new = KeyFrame(tgt, np.eye(3), accum_distance=100.0, id=1000)
    kfs = [KeyFrame(c, transform3Dto2D(np.asarray(g, np.float32)).astype(np.float64), accum_distance=float(i), id=i)
           for i, (c, g) in enumerate(zip(cands, gs))]
    guesses = LoopDetector.guesses_for(new, kfs)
    ref_res = [ref.icp_align(orc, tgt, cands[c], guess=guesses[c]) for c in range(32)]
    ref_fit = [orc.fitness_score(tgt, cands[c], ref_res[c]["T"])[0] for c in range(32)]
    want = sequential_best([r["converged"] for r in ref_res], ref_fit)[0]
    for det in (LoopDetector({"fitness_score_thresh": 1e9}, registration=Registration("ICP_HIP", device=0)),
                LoopDetector({"fitness_score_thresh": 1e9}, registration=RegistrationGroup("ICP_HIP", devices=(0, 0)))):
        rec = det.register_shard(kfs, new)
        for c in range(32):
            T = rec[c, 4:20].reshape(4, 4)
            dt, dr = pose_error(T, ref_res[c]["T"])
            assert dt <= TOL_TRANS and dr <= TOL_ROT, (c, dt, dr)
            assert bool(rec[c, 1] > 0.5) == ref_res[c]["converged"]
        assert LoopDetector.select_best(rec)[0] == want


def test_no_covariance_work():
    tgt, src = _pair("planar")
    reg = Registration("ICP_HIP", device=0)
    reg.profile_enable(True)
    reg.setInputTarget(tgt)
    reg.setInputSource(src)
    reg.align()
    reg.align_batch([src, src[:2000]])
    assert reg.profile_get(L.K_GICP_COVARIANCE)[1] == 0
    assert reg.profile_get(L.K_NN_SEARCH)[1] >= reg.last_result.iterations
    reg.profile_enable(False)


def test_edge_cases(orc):
    tgt, src = _pair("planar")
    reg = _gpu_align(tgt, src, maximum_iterations=0)
    r = ref.icp_align(orc, tgt, src, maximum_iterations=0)
    _compare(reg, r)
    assert reg.last_result.iterations == 1 and reg.last_result.converged
    three = np.array([[0.1, 0.2, 0.3, 0], [1.0, -0.5, 0.2, 0], [-0.7, 0.4, 0.9, 0]], np.float32)
    tgt3 = three.copy()
    tgt3[:, :3] += np.float32(0.05)
    reg = _gpu_align(tgt3, three)
    r = ref.icp_align(orc, tgt3, three)
    _compare(reg, r)
    one = np.array([[0.3, -0.2, 0.1, 0]], np.float32)
    reg = _gpu_align(one, src[:200], gicp_max_correspondence_distance=50.0)
    r = ref.icp_align(orc, one, src[:200], max_corr=50.0)
    assert np.all(np.isfinite(reg.getFinalTransformation()))
    _compare(reg, r)
