"""-m gpu: the item-compacted upstream-order NDT kernel (ndt_strict3_kernel, delta_graph_slam_amd/csrc/ndt_strict.h) multiplies every
point with the pair's angle tables from a per-workgroup copy in LDS (StrictHeader<true>); the fixed-slices instantiations
(DGS_NDT_FIXED_SLICES=1) keep reading the NdtPair record in global memory.  Same multiplications in the same order: the two must agree
bit for bit.

One pair alone, so the default launch deals the pair exactly the slices the fixed-slices launch gives it -- cap = max(ceil(n/512),
min(64, ceil(n/256))) slices of 256 points (tests/test_strict_hd_ring_gpu.py) -- and the sums associate the same way.  Wave w of slice q
takes points q * 256 + 64 w + lane, then the same a stride of 256 * cap further on; the float kinds' tile is two such sub-tiles.  Sizes:
  * 1: a source of one point -- a sub-tile with one live lane, three waves with no point at all;
  * 63, 64, 65: a sub-tile with 63 / 64 live lanes; 65: one live lane in the second wave;
  * 257: a second slice of one point;
  * 16385, 16447, 16448 (cap = 64, stride 16,384): the SECOND sub-tile of a tile with 1, 63 and 64 live lanes.
For each: the three evaluation kinds as single evaluations through the probe hooks (score + gradient, with the Hessian, the double
computeHessian) at two poses, and a full align -- score, gradient, Hessian, evaluation count and transform bit-identical.
Then a 12-candidate batch whose pairs are in different evaluation kinds in the same launch and leave at different rounds, twice on one
handle, against the oracle as tests/test_round4_gpu.py compares it: a header left over from another pair or launch would show."""
import contextlib
import os

import numpy as np
import pytest

from delta_graph_slam_amd import synth
from tests import strict_edge_cases as E

pytestmark = pytest.mark.gpu

RES = E.RES_POW2
SIZES = (1, 63, 64, 65, 257, 16385, 16447, 16448)


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


def _reg(**kw):
    from delta_graph_slam_amd.registration import Registration
    return Registration("NDT_OMP", ndt_strict_order=1, ndt_resolution=RES, ndt_hessian_recompute_double=1, **kw)


def _bits(*a):
    return b"".join(np.ascontiguousarray(np.asarray(x, np.float64)).tobytes() for x in a)


@pytest.fixture(scope="module")
def cloud():
    tgt, src, _ = E.solid(max(SIZES), RES)
    return tgt, src


def test_header_from_lds_equals_header_from_the_record_bit_for_bit(cloud):
    tgt, solid = cloud
    lds = _reg()
    with _env(DGS_NDT_FIXED_SLICES=1):
        rec = _reg()
    for r in (lds, rec):
        r.setInputTarget(tgt)
    guess = np.eye(4, dtype=np.float32)
    guess[:3, 3] = (0.03, -0.02, 0.01)
    for n in SIZES:
        src = solid[:n]
        for r in (lds, rec):
            r.setInputSource(src)
        for k, p in enumerate(E.POSES):
            what = (n, k)
            s0, g0 = lds.ndt_score_gradient(p)
            s1, g1, H1 = lds.ndt_derivatives(p)
            H2 = lds.ndt_hessian_double(p)
            assert s0 != 0 and np.abs(g1).max() > 0 and np.abs(H1).max() > 0 and np.abs(H2).max() > 0, what   # the case has items
            assert _bits(s0, g0) == _bits(*rec.ndt_score_gradient(p)), what + ("score + gradient",)
            assert _bits(s1, g1, H1) == _bits(*rec.ndt_derivatives(p)), what + ("with the Hessian",)
            assert _bits(H2) == _bits(rec.ndt_hessian_double(p)), what + ("double computeHessian",)
        out = []
        for r in (lds, rec):
            r.align(guess)
            out.append((r.hasConverged(), r.last_result.iterations, r.last_result.evaluations, r.getFinalTransformation().tobytes(),
                        _bits(r.ndt_trajectory())))
        print(n, "align: converged %s, %d iterations, %d evaluations" % out[0][:3])
        assert out[0][2] >= 1, n
        assert out[0] == out[1], (n, "align", out[0][:3], out[1][:3])
    for r in (lds, rec):
        r.close()


def test_no_header_survives_from_one_launch_or_pair_to_the_next(oracle_lib):
    tgt, sources, guesses, _ = synth.loop_batch(n_candidates=12, n_points=16384, seed=40, distinct_scans=12)
    o = oracle_lib.NdtOracle(resolution=1.0)
    o.set_target(tgt)
    ref = []
    for c in range(12):
        o.set_source(sources[c])
        ref.append(o.align(guesses[c]))
    assert len({r["evaluations"] for r in ref}) >= 4 and sum(r["hessian_recomputes"] for r in ref) >= 6   # mixed kinds per launch
    r = _reg()
    r.setInputTarget(tgt)
    for rep in range(2):      # twice on one handle: the second batch runs over whatever the first left in the pairs' records
        res = r.align_batch(sources, guesses, compute_fitness=False)
        for c in range(12):
            assert res[c]["converged"] == ref[c]["converged"] and res[c]["iterations"] == ref[c]["iterations"], (rep, c)
            assert res[c]["evaluations"] == ref[c]["evaluations"], (rep, c, res[c]["evaluations"], ref[c]["evaluations"])
            assert np.array_equal(res[c]["T"], ref[c]["T"]), (rep, c)
    r.close()
