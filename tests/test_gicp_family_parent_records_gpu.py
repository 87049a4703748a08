"""-m gpu: FAST_GICP / FAST_VGICP give, bit for bit, the records the library gave before its round kernels were written once and its
k-NN search and covariance pass moved to files of their own.  tests/golden/gicp_family_parent_records.npz was written on an
MI355X by the library built from the commit BEFORE that change, never by the code under test:

    DGS_REG_LIB=<that commit's libdgs_reg.so> python -m tests.test_gicp_family_parent_records_gpu

What it pins that nothing else does: FAST_VGICP's default batch (FAST_GICP's is in tests/test_batch_independent_gpu.py::
test_the_default_is_untouched), align_pairs with the batch-independent switch off (the table-target correspond kernel and the table-target
linearize kernel with slices that follow the launch), and the covariances of both k-NN widths through both searches.  Compared: transform,
converged, iterations, evaluations, status and the bits of the score; the bits of every covariance entry."""
import os

import numpy as np
import pytest

from tests import align_pairs_scenes as S
from tests.test_batch_independent_gpu import CASE1_SIZES, _bits, _case1_scene, _env, _guess, _make

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gicp_family_parent_records.npz")
SEARCHES = ("DIRECT1", "DIRECT7")
# (k, points, wave-per-leaf search): both list widths (k <= 32, 32 < k <= 64); 513 points = 65 index leaves, the last one partial, 50 points =
# fewer than 8 leaves, which the wave-per-leaf kernel answers on its careful path; DGS_KNN_LEAF at its default and 0 (the per-query walk)
COV_CASES = [(k, n, leaf) for k in (20, 40) for n in (513, 50) for leaf in (True, False)]
PAIR_SOURCE_SIZES = (255, 257, 2000)   # a slice short of kBlock = 256, one point past it, 8 slices


def _records(results):
    return dict(T=np.stack([r["T"] for r in results]).astype(np.float32), converged=np.array([int(r["converged"]) for r in results]),
                iterations=np.array([r["iterations"] for r in results]), evaluations=np.array([r["evaluations"] for r in results]),
                status=np.array([r["status"] for r in results]), score_bits=np.array([_bits(r["score"]) for r in results], dtype=np.uint64))


def vgicp_default_batch(search):
    """case 1 of tests/test_batch_independent_gpu.py (one 8,192-point target, sources of 1 .. 5,000 points) as one default align_batch"""
    tgt, sources, guesses, _, _ = _case1_scene()
    reg = _make("FAST_VGICP", False, search=search)
    reg.setInputTarget(tgt)
    out = _records(reg.align_batch(sources, guesses, compute_fitness=False))
    reg.close()
    return out


def align_pairs_default():
    """Five pairs over the three targets of align_pairs_scenes.distinct_pairs (8,192 / 5,000 / 4,500 points) and an empty one, switch off."""
    tgt, src, _ = S.base()
    rng = np.random.default_rng(811)
    targets = [tgt, S.subset(tgt, 5000, 21), S.subset(tgt, 4500, 22), np.zeros((0, 4), np.float32)]
    sources = [S.subset(src, m, 800 + k) for k, m in enumerate(PAIR_SOURCE_SIZES)]
    pairs = [(0, 0), (1, 1), (2, 2), (3, 1), (0, 2)]   # (target, source); pair 3 has no target
    guesses = [_guess(rng) for _ in pairs]
    reg = S.make_registration()
    tc, sc = [reg.make_cloud(c) for c in targets], [reg.make_cloud(c) for c in sources]
    out = _records(reg.align_pairs([tc[t] for t, _ in pairs], [sc[s] for _, s in pairs], guesses, compute_fitness=False))
    reg.close()
    return out


def covariance_bits(k, n, leaf):
    from delta_graph_slam_amd.registration import Registration
    cloud = S.subset(S.base()[1], n, 900 + n)
    old = os.environ.pop("DGS_KNN_LEAF", None)   # the search is chosen when the handle is made; leaf = True is the variable unset
    try:
        with _env(**({} if leaf else {"DGS_KNN_LEAF": 0})):
            reg = Registration("FAST_GICP", gicp_correspondence_randomness=k)
    finally:
        if old is not None:
            os.environ["DGS_KNN_LEAF"] = old
    reg.setInputTarget(cloud)
    reg.setInputSource(cloud)
    out = reg.gicp_covariances("source").view(np.uint64)
    reg.close()
    return out


def _cov_key(k, n, leaf):
    return "cov_k%d_n%d_%s" % (k, n, "leaf" if leaf else "walk")


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def _assert_records(got, golden, prefix):
    for field, value in got.items():
        want = golden[prefix + field]
        print(prefix + field, "equal" if np.array_equal(value, want) else (value.tolist(), want.tolist()))
        assert np.array_equal(value, want), (prefix + field, np.argwhere(np.asarray(value != want)).tolist()[:4])


@pytest.mark.parametrize("search", SEARCHES)
def test_fast_vgicp_default_batch_gives_the_parent_records(golden, search):
    assert golden["case1_sizes"].tolist() == list(CASE1_SIZES)
    _assert_records(vgicp_default_batch(search), golden, "vgicp_%s_" % search)


def test_align_pairs_with_the_switch_off_gives_the_parent_records(golden):
    got = align_pairs_default()
    assert got["status"][3] != 0 and got["converged"][3] == 0   # the pair without a target never ran
    _assert_records(got, golden, "pairs_")


@pytest.mark.parametrize("k,n,leaf", COV_CASES, ids=[_cov_key(*c)[4:] for c in COV_CASES])
def test_covariances_carry_the_parent_bits(golden, k, n, leaf):
    got, want = covariance_bits(k, n, leaf), golden[_cov_key(k, n, leaf)]
    assert got.shape == (n, 3, 3) and got.shape == want.shape
    bad = np.argwhere(got != want)
    print(_cov_key(k, n, leaf), "entries that differ:", len(bad))
    assert len(bad) == 0, bad[:4].tolist()


if __name__ == "__main__":
    from delta_graph_slam_amd import _lib
    out = {"case1_sizes": np.array(CASE1_SIZES)}
    for search in SEARCHES:
        out.update({"vgicp_%s_%s" % (search, f): v for f, v in vgicp_default_batch(search).items()})
    out.update({"pairs_" + f: v for f, v in align_pairs_default().items()})
    out.update({_cov_key(*c): covariance_bits(*c) for c in COV_CASES})
    np.savez_compressed(GOLDEN, **out)
    print("written by", _lib.LIB_PATH, "->", GOLDEN, os.path.getsize(GOLDEN), "bytes")
