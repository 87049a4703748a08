"""-m gpu: the cost-ordered dealing of the item-compacted NDT kernel (DGS_NDT_DEAL_BY_COST, default on; deal_workgroup_by_cost in
delta_graph_slam_amd/csrc/common.h) re-labels the workgroups of a launch and nothing else: a pair keeps its number of slices, a slice keeps its
points, the rows are summed in slice order -- so every record of a batch must be BYTE-identical to the one the index-ordered dealing
(DGS_NDT_DEAL_BY_COST=0, read at dgs_create) gives.  Transform, iterations, evaluation count and the bits of the score, for batches whose pairs
fall out of step (launches that hold more than one evaluation kind), batches in the second ballot chunk (65 pairs) and beyond the kept ballots
(257 pairs), and the two cases where there is nothing to order: one pair alone, and 32 pairs that stay in step from their first evaluation on.

That a batch reached a mixed-kind launch is read from the per-pair counters.  Round r of the launch-per-round driver serves every pair's r-th
evaluation.  A pair's evaluations of kind 1 (score, gradient, Hessian) are its first one and the first trial of every iteration it began, so
with E evaluations and I finished iterations a pair made at most x = E - 1 - I evaluations of another kind (a More-Thuente trial, kind 0, or
the closing computeHessian, kind 2) and at least x - 1.  Pair A with x <= 0 made kind 1 only; pair B with x >= 2 made another kind within its
first I_B + 3 evaluations; if A was still evaluating then (E_A >= I_B + 3) some launch held both."""
import os

import numpy as np
import pytest

from delta_graph_slam_amd import synth

pytestmark = pytest.mark.gpu


def _reg(on, **kw):
    from delta_graph_slam_amd.registration import Registration
    old = os.environ.get("DGS_NDT_DEAL_BY_COST")
    os.environ["DGS_NDT_DEAL_BY_COST"] = "1" if on else "0"
    try:
        kw.setdefault("ndt_resolution", 1.0)
        return Registration("NDT_OMP", ndt_strict_order=1, **kw)   # the knob is read at dgs_create
    finally:
        if old is None:
            os.environ.pop("DGS_NDT_DEAL_BY_COST", None)
        else:
            os.environ["DGS_NDT_DEAL_BY_COST"] = old


def _batch(n_pairs, n_points, seed):
    """One target, n_pairs scans of the same surfaces (each its own noise), guesses from very good to poor: the line searches fall out of step."""
    tgt, _, T_gt = synth.planar_pair(n=max(4 * n_points, 16384), seed_target=seed)
    rng = np.random.default_rng(seed)
    sources, guesses = [], []
    for i in range(n_pairs):
        _, src, _ = synth.planar_pair(n=n_points, seed_target=seed, seed_source=seed + 100 + i)
        q = (i % 5) / 4.0   # 0: the ground truth itself ... 1: 0.4 m / 0.06 rad away
        d = synth.make_transform(rng.uniform(-0.4, 0.4, 3) * q, rng.uniform(-0.06, 0.06, 3) * q)
        sources.append(src)
        guesses.append((d @ T_gt).astype(np.float32))
    return tgt, sources, np.stack(guesses)


def _run(on, tgt, sources, guesses, **kw):
    r = _reg(on, **kw)
    r.setInputTarget(tgt)
    res = r.align_batch(sources, guesses, compute_fitness=False)
    r.close()
    return res


def _assert_same(a, b, what):
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        assert (x["converged"], x["iterations"], x["evaluations"], x["status"]) == (y["converged"], y["iterations"], y["evaluations"], y["status"]), (what, i, x, y)
        assert np.asarray(x["T"]).tobytes() == np.asarray(y["T"]).tobytes(), (what, i)
        assert np.float64(x["score"]).tobytes() == np.float64(y["score"]).tobytes(), (what, i, x["score"], y["score"])


def _held_two_kinds(res):
    E = np.array([r["evaluations"] for r in res])
    I = np.array([r["iterations"] for r in res])
    x = E - 1 - I
    only_kind1 = np.flatnonzero(x <= 0)
    other = np.flatnonzero(x >= 2)
    print("evaluations", E.tolist(), "iterations", I.tolist())
    return any(E[a] >= I[b] + 3 for a in only_kind1 for b in other)


@pytest.mark.parametrize("n_pairs,n_points,seed", [(5, 3000, 7), (65, 2000, 8), (257, 1024, 9)])
def test_records_do_not_depend_on_the_dealing_order(n_pairs, n_points, seed):
    tgt, sources, guesses = _batch(n_pairs, n_points, seed)
    off = _run(False, tgt, sources, guesses)
    on = _run(True, tgt, sources, guesses)
    assert _held_two_kinds(off), "no launch of this batch is known to have held two evaluation kinds: choose another seed"
    _assert_same(on, off, (n_pairs, n_points))


def test_one_pair_alone():
    tgt, sources, guesses = _batch(5, 3000, 7)
    for k in (0, 4):
        _assert_same(_run(True, tgt, sources[k:k + 1], guesses[k:k + 1]), _run(False, tgt, sources[k:k + 1], guesses[k:k + 1]), ("alone", k))


def test_32_pairs_in_step():
    """32 times the same scan and guess: from the first evaluation on every launch holds ONE kind for all 32, so there is nothing to order by"""
    tgt, sources, guesses = _batch(5, 2000, 11)
    sources, guesses = [sources[3]] * 32, np.stack([guesses[3]] * 32)
    on = _run(True, tgt, sources, guesses)
    off = _run(False, tgt, sources, guesses)
    assert len({(r["iterations"], r["evaluations"]) for r in off}) == 1   # in step to the end
    _assert_same(on, off, "32 pairs in step")
