"""-m gpu: the upstream-order NDT kernel (ndt_strict_order = 1, ndt_strict3_kernel in delta_graph_slam_amd/csrc/ndt_strict.h) at the
edges of its item loop, against the CPU oracle.  The cases and the boundary each one hits: tests/strict_edge_cases.py (proved on the CPU
by tests/test_strict_edge_cases_cpu.py).

Per evaluation, Registration.ndt_derivatives (one pair alone; its hook runs ndt_strict3_kernel<SEARCH, false, true, false> -- unfused,
with the double pass, the LDS record ring -- as a kernel trace of one call shows) against NdtOracle.derivatives, all four searches, a
power-of-two and a non-power-of-two resolution, identity and a small motion:
  * order 2: score, gradient and all 36 Hessian entries bit-identical;
  * order 1, default and under DGS_NDT_FIXED_SLICES=1 (the plain item loop): score within 1e-12 relative, g and H within 1e-11 of their
    max -- the association of the double sums is the only difference;
  * kind 2 (PCL's double computeHessian, 64-point tiles, plain loop): bit-identical in order 2, within 1e-11 in order 1;
  * the outside case: exact zeros on both sides; non-finite source points: the oracle's semantics, nothing -- the same bits as the
    oracle without those points (on the device a NaN cell index converts to 0, which is inside this grid, and the point's items are
    dropped by the weight test);
  * the solid case against oracle/ndt_ref.py's independent float64 score (5e-7, test_oracle_ndt.py's bound);
  * the full-queue cases three times in the process: bit-identical.
Per batch, one align_batch of ragged cuts of a scan (every size above, one empty source, one full 65,536-point scan so that a pair of a
few points is spread over dozens of slices, most of them empty) against NdtOracle.align of each pair alone, in the default launch, under
DGS_NDT_FIXED_SLICES=1, unfused, and in order 2.

Found by this file: at resolution 0.7 the striped 32,768-point source puts one (point, voxel) pair of the KDTREE search at a squared
centroid distance of exactly float(0.7f * 0.7f).  The device's radius test (leaf * leaf in float, as upstream's float resolution_ squared)
dropped it, the oracle's (float(0.7 * 0.7) from the double resolution, one ulp larger) kept it; the oracle now squares its float leaf size."""
import contextlib
import itertools
import os

import numpy as np
import pytest

from delta_graph_slam_amd import _lib as L
from delta_graph_slam_amd import synth
from oracle import ndt_ref
from tests import strict_edge_cases as E

pytestmark = pytest.mark.gpu

SEARCHES = ("DIRECT7", "DIRECT1", "DIRECT26", "KDTREE")
OFFSETS = {"DIRECT7": ndt_ref._OFF7, "DIRECT26": np.array(list(itertools.product((-1, 0, 1), repeat=3)))}


@contextlib.contextmanager
def _env(**kv):
    """Settings read at handle creation (dgs_create)."""
    old = {k: os.environ.get(k) for k in kv}
    os.environ.update({k: str(v) for k, v in kv.items()})
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _reg(order, **kw):
    from delta_graph_slam_amd.registration import Registration
    return Registration("NDT_OMP", ndt_strict_order=order, **kw)


def _bits(*a):
    return b"".join(np.ascontiguousarray(np.asarray(x, np.float64)).tobytes() for x in a)


def _close(ref, got, what):
    so, go, Ho = ref
    s, g, H = got
    assert abs(so - s) <= 1e-12 * abs(so) + 1e-300, (what, so, s)
    assert np.abs(go - g).max() <= 1e-11 * (np.abs(go).max() + 1e-300), what
    assert np.abs(Ho - H).max() <= 1e-11 * (np.abs(Ho).max() + 1e-300), what


@pytest.mark.parametrize("res", E.RESOLUTIONS)
@pytest.mark.parametrize("search", SEARCHES)
def test_evaluations_at_the_edges(oracle_lib, search, res):
    kw = dict(ndt_resolution=res, ndt_search_method=L.NDT_SEARCH[search])
    regs = {"order 1": _reg(1, **kw), "order 2": _reg(2, **kw)}
    with _env(DGS_NDT_FIXED_SLICES=1):
        regs["order 1, fixed slices"] = _reg(1, **kw)
    o = oracle_lib.NdtOracle(resolution=res, search_method=search)
    o_clean = oracle_lib.NdtOracle(resolution=res, search_method=search)
    checked = dict(items=0, outside=0, repeats=0, f64=0)
    target_of = None
    for case, sizes in E.CASE_SIZES.items():
        for n in sizes:
            tgt, src, _ = E.CASES[case](n, res)
            if target_of is None or not np.array_equal(target_of, tgt):
                target_of = tgt
                o.set_target(tgt)
                o_clean.set_target(tgt)
                for r in regs.values():
                    r.setInputTarget(tgt)
            o.set_source(src)
            for r in regs.values():
                r.setInputSource(src)
            if case == "nonfinite":
                o_clean.set_source(src[np.isfinite(src[:, :3]).all(1)])
            for k, p in enumerate(E.POSES):
                what = (case, n, k, search, res)
                ref = o.derivatives(p)
                Hd = o.hessian_double(p)
                assert _bits(*regs["order 2"].ndt_derivatives(p)) == _bits(*ref), what
                assert np.array_equal(regs["order 2"].ndt_hessian_double(p), Hd), what
                for name in ("order 1", "order 1, fixed slices"):
                    got = regs[name].ndt_derivatives(p)
                    _close(ref, got, what + (name,))
                    Hd1 = regs[name].ndt_hessian_double(p)
                    assert np.abs(Hd1 - Hd).max() <= 1e-11 * (np.abs(Hd).max() + 1e-300), what + (name, "kind 2")
                if case == "outside":
                    assert ref[0] == 0 and not ref[1].any() and not ref[2].any() and not Hd.any(), what
                    assert got[0] == 0 and not got[1].any() and not got[2].any() and not Hd1.any(), what
                    checked["outside"] += 1
                else:
                    assert ref[0] != 0 and np.abs(ref[2]).max() > 0, what   # the case has items
                    checked["items"] += 1
                if case == "nonfinite":
                    assert _bits(*o_clean.derivatives(p)) == _bits(*ref), what + ("a non-finite point contributes nothing",)
                    assert np.array_equal(o_clean.hessian_double(p), Hd), what
                if case == "solid" and n in E.FULL_QUEUE_SIZES:
                    # the longest stretch of DMA overlapping compute: the same bits every time
                    first = _bits(*regs["order 1"].ndt_derivatives(p))
                    for _ in range(2):
                        assert _bits(*regs["order 1"].ndt_derivatives(p)) == first, what + ("repeat",)
                    checked["repeats"] += 1
                if case == "solid" and search in OFFSETS and n in (1, 129, 4097):
                    model = ndt_ref.VoxelModel(tgt, res)
                    sets = ndt_ref.neighbour_sets(model, src, p, OFFSETS[search])
                    s64 = ndt_ref.score(model, src, p, sets)
                    s1 = regs["order 1"].ndt_derivatives(p)[0]
                    assert abs(s1 - s64) <= 5e-7 * abs(s64), what + (s1, s64)
                    checked["f64"] += 1
    assert checked["items"] > 0 and checked["outside"] > 0 and checked["repeats"] > 0
    assert checked["f64"] > 0 or search not in OFFSETS
    for r in regs.values():
        r.close()


BATCH_SIZES = E.SIZES


@pytest.fixture(scope="module")
def edge_batch(oracle_lib):
    """Ragged cuts of loop_batch scans at every size of E.SIZES, one empty source, one full 65,536-point scan (cap_blocks = 128), with
    the oracle's run of every pair alone."""
    k = len(BATCH_SIZES) + 2
    tgt, scans, guesses, _ = synth.loop_batch(n_candidates=k, n_points=65536, seed=43, distinct_scans=4)
    sources = [scans[c][:n] for c, n in enumerate(BATCH_SIZES)] + [np.zeros((0, 4), np.float32), scans[k - 1]]
    o = oracle_lib.NdtOracle(resolution=1.0)
    o.set_target(tgt)
    ref = []
    for c, s in enumerate(sources):
        if s.shape[0] == 0:
            ref.append(None)
            continue
        o.set_source(s)
        ref.append(o.align(guesses[c]))
    return tgt, sources, guesses, ref


@pytest.mark.parametrize("variant", ["default", "fixed slices", "unfused", "order 2"])
def test_ragged_batch_at_the_edges(edge_batch, variant):
    tgt, sources, guesses, ref = edge_batch
    env = {"fixed slices": dict(DGS_NDT_FIXED_SLICES=1), "unfused": dict(DGS_NDT_FUSED=0)}.get(variant, {})
    with _env(**env):
        r = _reg(2 if variant == "order 2" else 1, ndt_resolution=1.0)
    r.setInputTarget(tgt)
    res = r.align_batch(sources, guesses, compute_fitness=False)
    for c, (x, ro) in enumerate(zip(res, ref)):
        n = sources[c].shape[0]
        if ro is None:
            assert x["status"] == 4 and not x["converged"], (variant, c)   # DGS_ERR_NO_SOURCE
            continue
        assert x["status"] == 0, (variant, c, n)
        assert (x["converged"], x["iterations"], x["evaluations"]) == (ro["converged"], ro["iterations"], ro["evaluations"]), (variant, c, n)
        assert np.array_equal(x["T"], ro["T"], equal_nan=True), (variant, c, n, np.abs(x["T"] - ro["T"]).max())
    r.close()
