"""-m gpu: the tile prologue of the upstream-order NDT item kernel (ndt_strict3_kernel, delta_graph_slam_amd/csrc/ndt_strict.h) at the
edges of its 128-point tiles, against the CPU oracle: DIRECT7, order 1, evaluation kinds 0 (score + gradient) and 1 (with the Hessian).

A wave's tile of the float kinds is two sub-tiles of 64 points one slice stride apart, their tables and queue entries written one
sub-tile after the other, sub-tile 0's items in front of sub-tile 1's in the queue.  A pair alone is cut into
max(ceil(n / 512), min(64, ceil(n / 256))) slices, so
  * sizes 1 .. 513 (the wave and the sub-tile, each minus one / exact / plus one): every second sub-tile is empty (beyond the cloud);
  * sizes above 16,384 (64 slices, stride 16,384): the points 16,384 .. n - 1 are the second sub-tiles -- one point, 63, exactly 64 (filled
    for one wave, empty for all others), and 3,616 (56 waves filled, one partly, the rest empty);
  * `far_tail`: the 20,000-point source with every point of a second sub-tile moved outside the target's grid: filled sub-tiles that meet
    no voxel, in front of and behind tiles that do.
Score, gradient and Hessian against the oracle's evaluation at 1e-13 (relative for the score, of the largest entry for gradient and
Hessian): tests/test_properties_gpu.py's bound for an order-1 score.  The float terms are the oracle's bit for bit; only the association of
their double sums differs, each sum of at most 20,000 x 7 terms.  Transforms, iterations and evaluation counts of full aligns -- one pair
alone and five pairs in one batch -- equal the oracle's."""
import numpy as np
import pytest

from delta_graph_slam_amd import synth

pytestmark = pytest.mark.gpu

SIZES = (1, 63, 64, 65, 127, 128, 129, 191, 192, 513, 16385, 16447, 16448, 20000)
STRIDE = 16384   # a pair alone above 16,384 points: 64 slices of 256 threads
POSES = (np.zeros(6), np.array([0.04, -0.03, 0.02, 0.004, -0.006, 0.008]))
TOL = 1e-13
BATCH = (513, 129, 16447, "far_tail", 20000)


@pytest.fixture(scope="module")
def clouds():
    tgt, src, _ = synth.planar_pair(n=20000)
    far = src.copy()
    far[STRIDE:, :3] += np.float32(500.0)   # far outside the target's grid at every pose
    return tgt, src, far


def _source(clouds, n):
    return clouds[2] if n == "far_tail" else clouds[1][:n]


@pytest.fixture(scope="module")
def oracle(oracle_lib, clouds):
    o = oracle_lib.NdtOracle(resolution=1.0)
    o.set_target(clouds[0])
    return o


@pytest.fixture(scope="module")
def reg(clouds):
    from delta_graph_slam_amd.registration import Registration
    r = Registration("NDT_OMP", ndt_strict_order=1, ndt_resolution=1.0)
    r.setInputTarget(clouds[0])
    yield r
    r.close()


def _rel(ref, got):
    ref, got = np.asarray(ref, np.float64), np.asarray(got, np.float64)
    return float(np.abs(ref - got).max() / (np.abs(ref).max() + 1e-300))


@pytest.mark.parametrize("n", SIZES + ("far_tail",))
def test_evaluations_at_the_tile_edges(clouds, oracle, reg, n):
    src = _source(clouds, n)
    oracle.set_source(src)
    reg.setInputSource(src)
    for k, p in enumerate(POSES):
        so, go, Ho = oracle.derivatives(p)
        s1, g1, H1 = reg.ndt_derivatives(p)               # kind 1
        s0, g0 = reg.ndt_score_gradient(p)                # kind 0
        so0, go0, _ = oracle.derivatives(p, compute_hessian=False)
        figures = dict(score1=_rel(so, s1), grad1=_rel(go, g1), hess1=_rel(Ho, H1), score0=_rel(so0, s0), grad0=_rel(go0, g0))
        print(n, k, figures)
        assert so != 0 and np.abs(Ho).max() > 0, (n, k)   # the case has items
        assert max(figures.values()) <= TOL, (n, k, figures)
    if n == "far_tail":
        # the moved points contribute nothing: the evaluation is the first 16,384 points'
        oracle.set_source(src[:STRIDE])
        assert oracle.derivatives(POSES[1])[0] == so


def _same_as_oracle(x, ro, what):
    assert x["status"] == 0, what
    assert (x["converged"], x["iterations"], x["evaluations"]) == (ro["converged"], ro["iterations"], ro["evaluations"]), what
    assert np.array_equal(x["T"], ro["T"]), (what, np.abs(x["T"] - ro["T"]).max())


@pytest.fixture(scope="module")
def oracle_aligns(clouds, oracle):
    ref = {}
    for n in BATCH:
        oracle.set_source(_source(clouds, n))
        ref[n] = oracle.align()
    return ref


@pytest.mark.parametrize("n", BATCH)
def test_one_pair_alone_aligns_like_the_oracle(clouds, reg, oracle_aligns, n):
    (x,) = reg.align_batch([_source(clouds, n)], compute_fitness=False)
    _same_as_oracle(x, oracle_aligns[n], n)


def test_five_pairs_align_like_the_oracle(clouds, reg, oracle_aligns):
    res = reg.align_batch([_source(clouds, n) for n in BATCH], compute_fitness=False)
    for n, x in zip(BATCH, res):
        _same_as_oracle(x, oracle_aligns[n], n)
