"""PCL_NDT_HIP (DGS_METHOD_PCL_NDT) on the device against the restatement of tests/pcl_ndt_reference.py, computed
on the DEVICE's own voxel table (so the evaluations are compared on bit-identical voxels): the neighbourhood, the three evaluation
kinds within TOL_EVAL x sum |increment|, single aligns, batch independence, one loop shard through LoopDetector and through a
two-member group on one card, edge cases.  Scenes: tests/pcl_ndt_scenes.py (their properties are asserted in tests/test_pcl_ndt_cpu.py)."""
import numpy as np
import pytest

import pcl_ndt_reference as R
import pcl_ndt_scenes as S
from delta_graph_slam_amd import synth
from delta_graph_slam_amd.registration import DgsError, Registration, RegistrationGroup
from helpers import TOL_ROT, TOL_TRANS, pose_error
from test_pcl_ndt_cpu import ALIGN_POINTS, ALIGN_SCENES

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    """Per scene: a handle with the target set, and the restatement's model made from the handle's voxel table."""
    out = {}
    for kind, res in S.SCENES:
        sc = S.scene(kind, res)
        reg = Registration("PCL_NDT_HIP", device=0, ndt_resolution=res)
        reg.setInputTarget(sc["target"])
        out[kind, res] = (reg, R.Model.from_device(reg, sc["target"], res))
    yield out
    for reg, _ in out.values():
        reg.close()


def _guess(sc):
    return synth.make_transform(sc["p"][:3], sc["p"][3:]).astype(np.float32)


@pytest.mark.parametrize("kind,res", S.SCENES)
def test_neighbours_equal_brute_force(dev, kind, res):
    reg, model = dev[kind, res]
    sc = S.scene(kind, res)
    xt = np.ones((sc["source"].shape[0], 4), np.float32)
    xt[:, :3] = R.transform_f32(R.pose_matrix_f32(sc["p"]), sc["source"])
    counts, ids = reg.pcl_ndt_neighbours(xt)
    want = R.neighbours(model, xt[:, :3])
    assert np.array_equal(counts, [len(v) for v in want])
    for i, v in enumerate(want):
        assert np.array_equal(ids[i, :len(v)], np.sort(v)) and (ids[i, len(v):] == -1).all(), i
    assert counts[2] == 0 and counts[3] == 0 and counts.max() >= 8    # NaN, infinite; the scene's fullest points


@pytest.mark.parametrize("kind,res", S.SCENES)
def test_every_evaluation_kind_is_within_tol_eval_of_the_restatement(dev, kind, res):
    reg, model = dev[kind, res]
    sc = S.scene(kind, res)
    worst = 0.0
    for n in S.SOURCE_SIZES + (sc["source"].shape[0],):
        src = sc["source"][:n]
        reg.setInputSource(src)
        for k in (1, 0, 2):
            ev = R.Evaluation(model, src, sc["p"], kind=k)
            if k == 2:
                got = np.concatenate([np.zeros(7), reg.ndt_hessian_double(sc["p"]).ravel()])
            else:
                s, g, H = reg.ndt_derivatives(sc["p"], hessian=(k == 1))
                got = np.concatenate([[s], g, H.ravel()])
                assert k == 1 or not H.any()
            err = np.abs(got - ev.total)
            ratio = float(np.max(np.where(ev.abs_total > 0, err / np.where(ev.abs_total > 0, ev.abs_total, 1.0), 0.0)))
            worst = max(worst, ratio)
            print(f"{sc['name']} n={n} kind={k} items={ev.pi.size}: max |device - restatement| / sum|increment| = {ratio:.3e}")
            assert np.all(err <= R.TOL_EVAL * ev.abs_total), (n, k, ratio)   # score, gradient and Hessian entries alike
    print(f"{sc['name']}: largest observed {worst:.3e}, TOL_EVAL {R.TOL_EVAL:.3e}")


def _same_as_restatement(reg, ref):
    r = reg.last_result
    print("device", r.iterations, r.evaluations, bool(r.converged), r.score, " restatement", ref["iterations"], ref["evaluations"], ref["converged"], ref["score"])
    assert (r.iterations, r.evaluations, bool(r.converged)) == (ref["iterations"], ref["evaluations"], ref["converged"])
    dt, dr = pose_error(reg.getFinalTransformation(), ref["T"])
    assert dt <= TOL_TRANS and dr <= TOL_ROT, (dt, dr)


@pytest.mark.parametrize("eps", [0.01, 1e-6])
@pytest.mark.parametrize("kind,res", ALIGN_SCENES)
def test_single_align_matches_the_restatement(dev, kind, res, eps):
    _, model = dev[kind, res]
    sc = S.scene(kind, res)
    src = sc["source"][:ALIGN_POINTS]
    reg = Registration("PCL_NDT_HIP", device=0, ndt_resolution=res, transformation_epsilon=eps)
    reg.setInputTarget(sc["target"])
    reg.setInputSource(src)
    reg.align(_guess(sc))
    _same_as_restatement(reg, R.align(model, src, _guess(sc), eps=eps))
    traj = reg.ndt_trajectory()
    assert traj.shape == (reg.last_result.iterations + 1, 6)
    reg.close()


@pytest.mark.parametrize("resident", [False, True])
def test_a_pair_has_the_same_bits_alone_and_in_a_ragged_batch(dev, resident):
    reg, _ = dev["street", 1.0]
    sc = S.scene("street", 1.0)
    sizes = (1, 63, 65, 255, 256, 257, 513, 1000, sc["source"].shape[0])
    rng = np.random.default_rng(11)
    sources = [np.ascontiguousarray(sc["source"][:n]) for n in sizes]
    guesses = []
    for _ in sizes:
        g = _guess(sc).copy()
        g[:3, 3] += rng.normal(0, 0.03, 3).astype(np.float32)
        guesses.append(g)
    alone = []
    for s, g in zip(sources, guesses):
        reg.setInputSource(s)
        reg.align(g)
        r = reg.last_result
        alone.append((reg.getFinalTransformation().copy(), r.score, r.iterations, r.evaluations, bool(r.converged)))
    srcs = [reg.make_cloud(s) for s in sources] if resident else sources
    out = reg.align_batch(srcs, guesses, compute_fitness=True)
    assert len({a[2] for a in alone}) > 1            # the pairs leave the batch at different rounds
    for c, (T, score, iters, evals, conv) in enumerate(alone):
        assert np.array_equal(out[c]["T"], T), c
        assert (out[c]["score"], out[c]["iterations"], out[c]["evaluations"], out[c]["converged"]) == (score, iters, evals, conv), c


def test_loop_shard_through_loop_detector_and_group():
    from delta_graph_slam_amd.loop_detector import KeyFrame, LoopDetector
    from delta_graph_slam_amd.transforms import transform3Dto2D
    n = 4
    tgt, cands, gs, _ = synth.loop_batch(n_candidates=n, n_points=4096, seed=40, distinct_scans=n)
    new = KeyFrame(tgt, np.eye(3), accum_distance=100.0, id=1000)
    kfs = [KeyFrame(c, transform3Dto2D(np.asarray(g, np.float32)).astype(np.float64), accum_distance=float(i), id=i)
           for i, (c, g) in enumerate(zip(cands, gs))]
    guesses = LoopDetector.guesses_for(new, kfs)
    one = Registration("PCL_NDT_HIP", device=0, ndt_resolution=1.0)
    one.setInputTarget(tgt)
    want = []
    for c in range(n):
        one.setInputSource(cands[c])
        one.align(guesses[c])
        want.append((one.getFinalTransformation().copy(), one.hasConverged()))
    assert any(w[1] for w in want)
    for det in (LoopDetector({"fitness_score_thresh": 1e9}, registration=Registration("PCL_NDT_HIP", device=0, ndt_resolution=1.0)),
                LoopDetector({"fitness_score_thresh": 1e9}, registration=RegistrationGroup("PCL_NDT_HIP", devices=(0, 0), ndt_resolution=1.0))):
        rec = det.register_shard(kfs, new)
        for c in range(n):
            assert bool(rec[c, 1] > 0.5) == want[c][1]
            assert np.array_equal(rec[c, 4:20].reshape(4, 4).astype(np.float32), want[c][0]), c   # fixed slices: the batch's bits are the pair's own
            assert rec[c, 3] == 0 and (not want[c][1] or np.isfinite(rec[c, 2]))


def test_edge_cases(dev):
    reg0, model = dev["room", 1.0]
    sc = S.scene("room", 1.0)
    src = sc["source"][:ALIGN_POINTS]
    # a guess that is exactly the identity: the pose vector is zero, upstream's small-angle case in all three angles
    reg = Registration("PCL_NDT_HIP", device=0, ndt_resolution=1.0)
    reg.setInputTarget(sc["target"])
    reg.setInputSource(src)
    reg.align(np.eye(4, dtype=np.float32))
    _same_as_restatement(reg, R.align(model, src, np.eye(4, dtype=np.float32)))
    reg.close()
    # maximum_iterations = 0
    reg = Registration("PCL_NDT_HIP", device=0, ndt_resolution=1.0, maximum_iterations=0)
    reg.setInputTarget(sc["target"])
    reg.setInputSource(src)
    reg.align(_guess(sc))
    _same_as_restatement(reg, R.align(model, src, _guess(sc), max_it=0))
    # an empty source
    reg.setInputSource(np.zeros((0, 4), np.float32))
    reg.align(_guess(sc))
    assert reg.last_result.status == 4 and not reg.hasConverged()                  # DGS_ERR_NO_SOURCE
    assert np.array_equal(reg.getFinalTransformation(), _guess(sc))
    out = reg.align_batch([np.zeros((0, 4), np.float32), src], [_guess(sc)] * 2, compute_fitness=False)
    assert out[0]["status"] == 4 and out[1]["status"] == 0 and out[1]["converged"]
    # a target with only under-populated voxels: nothing to evaluate, the zero step ends the registration
    reg.setInputTarget(S.sparse_target())
    reg.setInputSource(src)
    assert reg.counts()["valid_voxels"] == 0
    s, g, H = reg.ndt_derivatives(np.zeros(6))
    assert s == 0 and not g.any() and not H.any()
    counts, ids = reg.pcl_ndt_neighbours(src)
    assert not counts.any() and (ids == -1).all()
    reg.align(np.eye(4, dtype=np.float32))
    assert reg.last_result.iterations == 0 and np.array_equal(reg.getFinalTransformation(), np.eye(4, dtype=np.float32))
    reg.close()
    # the new hook on a handle of another method
    other = Registration("NDT_OMP", device=0, ndt_resolution=1.0)
    other.setInputTarget(sc["target"])
    with pytest.raises(DgsError) as e:
        other.pcl_ndt_neighbours(src)
    assert e.value.status == 6                                                      # DGS_ERR_UNSUPPORTED
    with pytest.raises(DgsError):
        other.ndt_derivatives(np.zeros(6), hessian=False)                           # the score + gradient hook is PCL_NDT_HIP's
    other.close()
