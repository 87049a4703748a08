"""-m gpu: ICP_HIP (delta_graph_slam_amd/csrc/icp.hip) and GICP_HIP (csrc/pcl_gicp.hip) at the edges of their slices, waves, row totals,
gates, minimum counts and degenerate fits, against the two restatements tests/icp_reference.py and tests/pcl_gicp_reference.py.  The pairs
and the kernel line each one aims at: tests/icp_gicp_edge_cases.py (proved on the CPU by tests/test_icp_gicp_edge_cases_cpu.py, which also
proves that no decision of a case is marginal: every count below is compared exactly, no case is exempt).

  * ICP cases: what test_icp_gpu._compare asserts (kept pairs and T_k per iteration, iterations, convergence, evaluations, final pose), and
    the per-iteration MSE and the final score within 1e-12 relative: both sides sum at most 4,353 non-negative doubles of the same float
    d2 values in a different order (bound n * 2^-53 = 4.8e-13).  Far-frame pairs: T_k's translation entries within one float ulp of the
    entry -- both sides round a double to float and the doubles differ by summation order only, but one ulp of an entry near 100 is
    7.6e-6, so the 1e-6 bound holds for the rotation block alone there.  Pairs whose rotation is not unique (`pose_compared = False`):
    counts, iterations, convergence and MSE, and T_k a finite rigid motion.
  * GICP cases: test_pcl_gicp_gpu._compare, unchanged; the evaluation passes are compared exactly wherever the restatement's line
    searches did not end in roundoff (its own rule).  Size and row-total cases: dgs_pcl_gicp_evaluate at a fixed non-zero state against
    ref.evaluate over ref.correspondences, 1e-10 relative -- no BFGS state is involved.  n == k and k = 5: the covariances, 1e-9.
  * batches at the edges: bit-identical T, score, iterations and converged alone and inside one batch, in both orders, host arrays and
    resident clouds; a batch of empty sources only."""
import numpy as np
import pytest

import icp_gicp_edge_cases as E
import test_icp_gpu as I
import test_pcl_gicp_gpu as G
from helpers import TOL_ROT, TOL_TRANS, pose_error
from test_icp_gicp_edge_cases_cpu import forks

pytestmark = pytest.mark.gpu

DBL_MAX = np.finfo(np.float64).max
MSE_TOL = 1e-12
NO_SOURCE = 4             # DGS_ERR_NO_SOURCE


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle
    return oracle


_REGS = {}


def _registration(method, prm):
    """One Registration per method and settings combination."""
    from delta_graph_slam_amd.registration import Registration
    key = (method,) + tuple(sorted(prm.items()))
    if key not in _REGS:
        _REGS[key] = Registration(method, device=0, **prm)
    return _REGS[key]


def _align(c, method):
    reg = _registration(method, E.settings(c, method))
    reg.setInputTarget(c.tgt)
    reg.setInputSource(c.src)
    reg.align(c.guess)
    return reg


def _rel(a, b):
    return 0.0 if a == b else abs(a - b) / abs(b) if b != 0 else np.inf


def _compare_icp(reg, r, c, figures):
    res = reg.last_result
    Tk, mse, nc = reg.icp_trajectory(0)
    assert res.iterations == r["iterations"] and len(nc) == r["iterations"], (res.iterations, len(nc), r["iterations"])
    compared = c.plan.get("pose_compared", True)
    for k in range(len(nc)):
        want_T, want_mse, want_n = r["traj"][k]
        assert nc[k] == want_n, (k, nc[k], want_n)
        e = _rel(float(mse[k]), want_mse)
        figures["mse"] = max(figures.get("mse", 0.0), e)
        assert e <= MSE_TOL, (k, mse[k], want_mse, e)
        assert np.all(np.isfinite(Tk[k])) and np.array_equal(Tk[k][3], [0, 0, 0, 1])
        if not compared:
            R = Tk[k][:3, :3].astype(np.float64)
            assert np.abs(R @ R.T - np.eye(3)).max() <= 1e-6 and abs(np.linalg.det(R) - 1.0) <= 1e-6, (k, R)
        elif c.plan.get("far"):
            assert np.abs(Tk[k][:3, :3] - want_T[:3, :3]).max() <= 1e-6, (k, np.abs(Tk[k][:3, :3] - want_T[:3, :3]).max())
            for a in range(3):
                got, want = np.float32(Tk[k][a, 3]), np.float32(want_T[a, 3])
                ulps = abs(float(got) - float(want)) / float(np.spacing(max(abs(got), abs(want))))
                figures["far_ulps"] = max(figures.get("far_ulps", 0.0), ulps)
                assert ulps <= 1.0, (k, a, got, want, ulps)
        else:
            assert np.abs(Tk[k] - want_T).max() <= 1e-6, (k, np.abs(Tk[k] - want_T).max())
    assert bool(res.converged) == r["converged"]
    assert res.evaluations == r["evaluations"]
    if r["iterations"]:
        e = _rel(float(res.score), r["score"])
        figures["mse"] = max(figures.get("mse", 0.0), e)
        assert e <= MSE_TOL, (res.score, r["score"], e)
    else:
        assert res.score == r["score"] == DBL_MAX
    T = reg.getFinalTransformation()
    assert np.all(np.isfinite(T))
    if compared:
        dt, dr = pose_error(T, r["T"])
        assert dt <= TOL_TRANS and dr <= TOL_ROT, (dt, dr)
    if compared and not c.plan.get("far"):
        I._compare(reg, r)                                                 # the existing comparison itself, whatever it comes to hold
    rec = E.planned(c, E.ICP, "record") or {}
    for key in ("iterations", "converged", "evaluations"):
        if key in rec:
            assert getattr(res, key) == rec[key], (key, getattr(res, key), rec[key])
    if r["iterations"] == 0:
        assert np.array_equal(T, np.eye(4, dtype=np.float32) if c.guess is None else c.guess)


def _compare_gicp(orc, reg, r, c, name, figures):
    res = reg.last_result
    G._compare(reg, r, exact_passes=not any(forks(orc, name)))
    rec = E.planned(c, E.GICP, "record") or {}
    for key in ("iterations", "converged", "evaluations"):
        if key in rec:
            assert getattr(res, key) == rec[key], (key, getattr(res, key), rec[key])
    if c.plan.get("probe"):
        T, guess, m, f, g, _ = E.probe_reference(orc, name)
        md, fd, gd = reg.pcl_gicp_evaluate(E.PROBE_X, transformation=T, guess=guess)
        ef, eg = abs(fd - f) / abs(f), np.abs(gd - g).max() / max(np.abs(g).max(), 1e-300)
        figures["probe"] = max(figures.get("probe", 0.0), ef, eg)
        assert md == m, (md, m)
        assert ef <= 1e-10, (fd, f)
        assert eg <= 1e-10, (gd, g)
    if c.plan.get("covariances"):
        for which, want, sv in (("source", r["Cs"], r["sv_src"]), ("target", r["Ct"], r["sv_tgt"])):
            dev = reg.gicp_covariances(which)
            ok = G._nondegenerate(sv)
            assert ok.mean() > 0.9
            err = np.abs(dev[ok] - want[ok]).max(axis=(1, 2))
            figures["cov"] = max(figures.get("cov", 0.0), float(err.max() / np.abs(want[ok]).max()))
            assert err.max() <= 1e-9 * np.abs(want[ok]).max(), (which, err.max())


def _run_family(orc, family, method):
    """Every case of the family on the device; the failures of all of them in one report."""
    failures, figures = [], {}
    names = [n for n, m in E.RUNS if m == method and E.case(n).family == family]
    assert names
    for name in names:
        c = E.case(name)
        print(name, "--", c.aim)
        try:
            r = E.reference(orc, name, method)
            reg = _align(c, method)
            if method == E.ICP:
                _compare_icp(reg, r, c, figures)
            else:
                _compare_gicp(orc, reg, r, c, name, figures)
        except AssertionError as e:
            failures.append(f"{name}: {e}")
    print(family, method, "largest figures:", {k: f"{v:.3g}" for k, v in figures.items()})
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("family", [f for f in E.FAMILIES if any(E.case(n).family == f for n, m in E.RUNS if m == E.ICP)])
def test_icp_edge_cases(orc, family):
    _run_family(orc, family, E.ICP)


@pytest.mark.parametrize("family", [f for f in E.FAMILIES if any(E.case(n).family == f for n, m in E.RUNS if m == E.GICP)])
def test_gicp_edge_cases(orc, family):
    _run_family(orc, family, E.GICP)


# ============================================================================================ batches at the edges
def _edge_batch(method):
    tgt, src = E.pair()
    G_ = E.ROW_GROUPS[method]
    big = E.SLICE * G_ + 1
    far = src[:300].copy()
    far[:, :3] += np.float32(100.0)                                       # beyond the gate
    full = src if big <= src.shape[0] else E.extended_source(big)
    sources = [src[:1 if method == E.ICP else 20], src[:255], src[:256], src[:257], full[:big], np.zeros((0, 4), np.float32), far]
    rng = np.random.default_rng(11)
    guesses = []
    for _ in sources:
        g = np.eye(4, dtype=np.float32)
        g[:3, 3] = rng.normal(0, 0.05, 3)
        guesses.append(g)
    return tgt, [np.ascontiguousarray(s) for s in sources], guesses


@pytest.mark.parametrize("resident", [False, True])
@pytest.mark.parametrize("method", [E.ICP, E.GICP])
def test_batch_independence_at_the_edges(method, resident):
    from delta_graph_slam_amd.registration import Registration
    tgt, sources, guesses = _edge_batch(method)
    reg = Registration(method, device=0, **(E.ICP_WALK if method == E.ICP else {}))
    reg.setInputTarget(tgt)
    alone = []
    for s, g in zip(sources, guesses):
        if s.shape[0] == 0:
            alone.append(None)
            continue
        reg.setInputSource(s)
        reg.align(g)
        r = reg.last_result
        alone.append((reg.getFinalTransformation().copy(), r.score, r.iterations, bool(r.converged)))
    assert alone[4][2] >= 1 and alone[4][3] and (method == E.GICP or alone[0][2] == 0)       # one point: ICP stops below 3 pairs
    assert alone[6][2] == 0 and not alone[6][3] and np.array_equal(alone[6][0], guesses[6])
    for order in (list(range(len(sources))), list(range(len(sources)))[::-1]):
        srcs = [sources[i] for i in order]
        srcs = [reg.make_cloud(s) for s in srcs] if resident else srcs
        out = reg.align_batch(srcs, [guesses[i] for i in order], compute_fitness=True)
        for o, i in zip(out, order):
            if alone[i] is None:
                assert o["status"] == NO_SOURCE and not o["converged"] and np.array_equal(o["T"], guesses[i])
                continue
            T, score, iters, conv = alone[i]
            assert o["status"] == 0
            assert np.array_equal(o["T"], T), (i, order)
            assert o["score"] == score and o["iterations"] == iters and o["converged"] == conv, (i, order)


@pytest.mark.parametrize("resident", [False, True])
@pytest.mark.parametrize("method", [E.ICP, E.GICP])
def test_a_batch_of_empty_sources_only(method, resident):
    """total_slices == 0: no launch may have an empty grid -- icp_align_batch runs its rounds under `n_live > 0`, pg_run_batch its
    prepare kernel under `total_slices > 0` and its rounds under `n_live > 0`; the fitness pass always has one workgroup per pair."""
    from delta_graph_slam_amd.registration import Registration
    tgt, _ = E.pair()
    reg = Registration(method, device=0)
    reg.setInputTarget(tgt)
    guesses = [E.translation((0.25 * k, -0.5, 0.125 * k)) for k in range(3)]
    empty = [np.zeros((0, 4), np.float32) for _ in range(3)]
    srcs = [reg.make_cloud(s) for s in empty] if resident else empty
    out = reg.align_batch(srcs, guesses, compute_fitness=True)            # raises unless the call returns DGS_OK
    assert len(out) == 3
    for o, g in zip(out, guesses):
        assert o["status"] == NO_SOURCE and not o["converged"] and o["iterations"] == 0
        assert np.array_equal(o["T"], g)
    assert (reg._lib.dgs_last_error(reg._h) or b"") == b""
