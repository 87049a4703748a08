"""-m gpu: a More-Thuente trial pose that its line search has evaluated before is answered from NdtSolver::trial_x inside the closing that
queues it, without a launch (ndt_advance, upstream orders; DGS_NDT_REUSE_TRIALS, default on, read at dgs_create).  With the switch off the
pose is evaluated again and its result replaced by the cached one, as before.  Either way the optimiser goes through the same states, so the
records -- converged, iterations, upstream's evaluation count, transform -- are the oracle's in both positions.

The oracle does not report repeats.  The device counts them (counts()["evaluations_reused"], the same number in both positions: with the
switch off a hit is a replacement) and the tests tie that count to the oracle by
    counts()["evaluations"] + (reused if the switch is on else 0) == sum of the oracle's evaluations,
where counts()["evaluations"] is what ran on the device.  The repeat counts quoted below were counted on the CPU with an instrumented copy
of the oracle's line search; the tests assert `reused >= 1` wherever a repeat is expected, so a scene that stops exercising the path fails.

A repeat FOLLOWED BY A FRESH TRIAL in the same line search does not occur in any scene of this file: wherever a pair repeats, the CPU count
is exactly ndt_mt_max_step_iterations (10, or 1 / 2 / 3 in the capped test), i.e. every chain of reused trials runs into the cap and ends
with computeHessian.  The code path (a chain that ends by queueing a pose that is not cached) is therefore not pinned by a test here."""
import os

import numpy as np
import pytest

from delta_graph_slam_amd import synth

pytestmark = pytest.mark.gpu


def _reg(**kw):
    from delta_graph_slam_amd.registration import Registration
    kw.setdefault("ndt_resolution", 1.0)
    return Registration("NDT_OMP", **kw)


class _env:
    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kv}
        os.environ.update({k: str(v) for k, v in self.kv.items()})

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _reg_switch(on, env=None, **kw):
    """a handle created with DGS_NDT_REUSE_TRIALS = on (and `env`): the switches are read at dgs_create"""
    with _env(DGS_NDT_REUSE_TRIALS=int(on), **(env or {})):
        return _reg(**kw)


_REF = {}


def _oracle(oracle_lib, name, tgt, sources, guesses, **okw):
    """the oracle's runs of a scene, computed once per module"""
    if name not in _REF:
        o = oracle_lib.NdtOracle(resolution=1.0, **okw)
        o.set_target(tgt)
        ref = []
        for s, g in zip(sources, guesses):
            o.set_source(s)
            ref.append(o.align(g))
        _REF[name] = ref
    return _REF[name]


@pytest.fixture(scope="module")
def batch12():
    tgt, sources, guesses, _ = synth.loop_batch(n_candidates=12, n_points=16384, seed=40, distinct_scans=12)
    return tgt, list(sources), list(guesses)


@pytest.fixture(scope="module")
def batch8():
    tgt, sources, guesses, _ = synth.loop_batch(n_candidates=8, n_points=4096, seed=40, distinct_scans=8)
    return tgt, list(sources), list(guesses)


def _assert_records(res, ref, tag):
    for c, (x, y) in enumerate(zip(res, ref)):
        assert x["converged"] == y["converged"] and x["iterations"] == y["iterations"], (tag, c, x["iterations"], y["iterations"])
        assert x["evaluations"] == y["evaluations"], (tag, c, x["evaluations"], y["evaluations"])
        assert np.array_equal(x["T"], y["T"]), (tag, c)


def _assert_counts(r, on, total, tag, expect_repeat=True):
    """executed + reused == the oracle's evaluations; returns the hits"""
    c = r.counts()
    reused, executed = c["evaluations_reused"], c["evaluations"]
    print(tag, "switch", on, "executed", executed, "reused", reused, "oracle", total)
    if expect_repeat:
        assert reused >= 1, (tag, "the scene no longer repeats a trial pose")
    assert executed == (total - reused if on else total), (tag, on, executed, reused, total)
    return reused


def _batch_in_both_positions(tgt, sources, guesses, ref, tag, env=None, reps=2, **kw):
    total = sum(y["evaluations"] for y in ref)
    reused = {}
    for on in (1, 0):
        r = _reg_switch(on, env, ndt_strict_order=1, **kw)
        r.setInputTarget(tgt)
        for rep in range(reps):      # twice on the same handle: the second batch starts from the first one's records and counters
            res = r.align_batch(sources, guesses, compute_fitness=False)
            _assert_records(res, ref, (tag, on, rep))
            hits = _assert_counts(r, on, total, (tag, rep))
            assert reused.setdefault(on, hits) == hits, (tag, on, rep)
        r.close()
    assert reused[1] == reused[0], (tag, reused)
    return reused[1], total


def test_mixed_batch_equals_the_oracle_with_and_without_reuse(oracle_lib, batch12):
    """12 x 16,384 points.  CPU count: evaluations 33, 28, 20, 16, 28, 23, 5, 15, 21, 15, 8, 18 (230), repeats 10, 10, 0, 0, 10, 10, 0, 0, 10,
    0, 0, 0 -- 50 of 230 is the value counted on the CPU.  Pair 1 has a line search whose every loop trial repeats; pair 0 has searches
    with fresh trials beside the one that repeats."""
    tgt, sources, guesses = batch12
    ref = _oracle(oracle_lib, "batch12", tgt, sources, guesses)
    assert [y["evaluations"] for y in ref] == [33, 28, 20, 16, 28, 23, 5, 15, 21, 15, 8, 18]
    reused, total = _batch_in_both_positions(tgt, sources, guesses, ref, "mixed batch")
    assert total == 230 and reused >= 1


@pytest.mark.parametrize("cap", [1, 2, 3])
def test_chain_ended_by_the_step_iteration_cap(oracle_lib, batch12, cap):
    """The first six pairs with ndt_mt_max_step_iterations = cap: a chain of reused trials ends because step_iterations reaches the cap.
    CPU count of repeats per pair: cap, cap, 0, 0, cap, cap."""
    tgt, sources, guesses = batch12
    sources, guesses = sources[:6], guesses[:6]
    ref = _oracle(oracle_lib, "cap%d" % cap, tgt, sources, guesses, mt_max_step_iterations=cap)
    _batch_in_both_positions(tgt, sources, guesses, ref, "cap %d" % cap, ndt_mt_max_step_iterations=cap)


@pytest.mark.parametrize("order", [1, 2])
def test_single_pairs_are_bit_equal_with_and_without_reuse(oracle_lib, batch12, order):
    """One active pair gives every launch the same composition, so skipping rounds changes no double: trajectory, double score and
    transform are equal between the two switch positions.  In order 2 (sums in the CPU's order) the trajectory is the oracle's, bit for
    bit -- which it is only if the computeHessian pass behind a reused accepted trial ran at that trial's pose."""
    tgt, sources, guesses = batch12
    ref = _oracle(oracle_lib, "batch12", tgt, sources, guesses)
    regs = {on: _reg_switch(on, ndt_strict_order=order) for on in (1, 0)}
    for r in regs.values():
        r.setInputTarget(tgt)
    for c in (0, 1, 2):
        got = {}
        for on, r in regs.items():
            r.setInputSource(sources[c])
            r.align(guesses[c])
            hits = _assert_counts(r, on, ref[c]["evaluations"], ("single", order, c), expect_repeat=c in (0, 1))
            got[on] = (r.ndt_trajectory(), r.last_result.score, r.getFinalTransformation(), r.last_result.iterations, r.last_result.evaluations, hits)
            assert (r.hasConverged(), got[on][3], got[on][4]) == (ref[c]["converged"], ref[c]["iterations"], ref[c]["evaluations"]), (order, c, on)
            assert np.array_equal(got[on][2], ref[c]["T"]), (order, c, on)
            if order == 2:
                assert np.array_equal(got[on][0], ref[c]["trajectory"]), (c, on)
        assert np.array_equal(got[1][0], got[0][0]), (order, c)
        assert got[1][1] == got[0][1], (order, c, got[1][1], got[0][1])
        assert np.array_equal(got[1][2], got[0][2]) and got[1][5] == got[0][5], (order, c)
    for r in regs.values():
        r.close()


def test_fixed_slices_batch_is_bit_equal_with_and_without_reuse(oracle_lib, batch12):
    """DGS_NDT_FIXED_SLICES=1: a pair's sums do not depend on the composition of the launch, so the whole batch is bit-equal between the two
    switch positions although its pairs meet other launches: trajectories, double scores, transforms."""
    tgt, sources, guesses = batch12
    ref = _oracle(oracle_lib, "batch12", tgt, sources, guesses)
    total = sum(y["evaluations"] for y in ref)
    got = {}
    for on in (1, 0):
        r = _reg_switch(on, dict(DGS_NDT_FIXED_SLICES=1), ndt_strict_order=1)
        r.setInputTarget(tgt)
        res = r.align_batch(sources, guesses, compute_fitness=False)
        _assert_records(res, ref, ("fixed slices", on))
        hits = _assert_counts(r, on, total, ("fixed slices",))
        got[on] = (res, [r.ndt_trajectory(c) for c in range(len(sources))], hits)
        r.close()
    assert got[1][2] == got[0][2]
    for c in range(len(sources)):
        assert np.array_equal(got[1][1][c], got[0][1][c]), c
        assert got[1][0][c]["score"] == got[0][0][c]["score"], (c, got[1][0][c]["score"], got[0][0][c]["score"])
        assert np.array_equal(got[1][0][c]["T"], got[0][0][c]["T"]), c


@pytest.mark.parametrize("env", [dict(DGS_NDT_FUSED=0), dict(DGS_NDT_STRICT_KERNEL=2), dict(DGS_NDT_SPECULATE=0), dict(DGS_NDT_SOLVE_MIN_ACTIVE=2)],
                         ids=["unfused", "lane-per-point", "no speculation", "Newton steps on the third stream"])
def test_other_launch_structures(oracle_lib, batch8, env):
    """8 x 4,096 points.  CPU count: evaluations 7, 17, 22, 16, 49, 9, 26, 10, repeats 0, 0, 10, 0, 0, 0, 10, 0.  ndt_advance is shared by
    every closing: the solve launch of the unfused path, the lane-per-point kernels, closings that never speculate, and closings that
    leave the Newton step to ndt_strict_solve_kernel."""
    tgt, sources, guesses = batch8
    ref = _oracle(oracle_lib, "batch8", tgt, sources, guesses)
    assert [y["evaluations"] for y in ref] == [7, 17, 22, 16, 49, 9, 26, 10]
    _batch_in_both_positions(tgt, sources, guesses, ref, tuple(env.items()), env=env, reps=1)
