"""-m gpu tests of Registration.align_pairs on GICP_HIP (pairs that each name their own target) against today's per-target
path, setInputTarget(target) + align, and against the test-side restatement (tests/pcl_gicp_reference.py).

GICP_HIP sums over fixed slices (a pair's workgroups are a function of its own size), so the comparison with today's path is bit for bit.
Clouds come from synth.planar_pair(4096): the targets hold 500 points (a subset), 4,096 (the target itself) and 4,500 (the target and 404
points of the source moved into its frame), which with 8-point leaves and a fan-out of 8 are index depths 2, 3 and 4 -- one launch reads
three table entries of different depth.  Sources are subsets of the pair's source."""
import numpy as np
import pytest

from delta_graph_slam_amd import synth
import pcl_gicp_reference as ref
from helpers import TOL_ROT, TOL_TRANS, pose_error

pytestmark = pytest.mark.gpu

FIT_RTOL = 1e-9   # the edge scorer against the batch scorer
K = 20            # the factory's reg_correspondence_randomness
EMPTY = np.zeros((0, 4), np.float32)
EYE = np.eye(4, dtype=np.float32)

_CACHE = {}


def _registration(method="GICP_HIP", **kw):
    from delta_graph_slam_amd.registration import Registration
    return Registration(method, device=0, **kw)


def _subset(cloud, m, seed):
    return cloud[np.random.default_rng(seed).permutation(cloud.shape[0])[:m]].copy()


def _scene():
    """-> (targets [500, 4096, 4500 points], the 4,096-point source)"""
    if "scene" not in _CACHE:
        tgt, src, T = synth.planar_pair(4096)
        tgt, src = np.ascontiguousarray(tgt, np.float32), np.ascontiguousarray(src, np.float32)
        moved = synth.apply_transform(T, _subset(src, 404, 1)).astype(np.float32)
        _CACHE["scene"] = ([_subset(tgt, 500, 2), tgt, np.ascontiguousarray(np.concatenate([tgt, moved]))], src)
        assert [t.shape[0] for t in _CACHE["scene"][0]] == [500, 4096, 4500]
    return _CACHE["scene"]


def _guess(rng):
    return synth.make_transform(rng.uniform(-0.15, 0.15, 3), rng.uniform(-0.02, 0.02, 3)).astype(np.float32)


def _single(reg, target, source, guess):
    """today's path for one pair, on `reg`: the dict align_pairs gives, fitness from getFitnessScore"""
    reg.setInputTarget(target)
    reg.setInputSource(source)
    reg.align(guess)
    lr = reg.last_result
    return dict(T=reg.getFinalTransformation().copy(), converged=reg.hasConverged(), iterations=lr.iterations, evaluations=lr.evaluations,
                status=lr.status, score=lr.score, fitness=reg.getFitnessScore())


def _assert_bits(res, want, what):
    """transform, flags, counts and score bit for bit; -> the relative fitness difference, held to FIT_RTOL"""
    assert res["status"] == 0 == want["status"], (what, res["status"])
    assert np.array_equal(res["T"], want["T"]), (what, np.abs(res["T"] - want["T"]).max())
    assert res["converged"] == want["converged"], what
    assert (res["iterations"], res["evaluations"]) == (want["iterations"], want["evaluations"]), (what, res["iterations"], want["iterations"],
                                                                                                res["evaluations"], want["evaluations"])
    assert np.float64(res["score"]).view(np.uint64) == np.float64(want["score"]).view(np.uint64), (what, res["score"], want["score"])
    if res["fitness"] == want["fitness"]:
        return 0.0
    df = abs(res["fitness"] - want["fitness"]) / abs(want["fitness"])
    assert df <= FIT_RTOL, (what, res["fitness"], want["fitness"])
    return df


def _against_single(clouds, pairs, what):
    """align_pairs over resident clouds on one registration, today's path on a second one over the SAME DeviceClouds (so both use the
    same index and covariances): bit-equal.  pairs: (target index, source index, guess).  -> (results, single results)"""
    reg, single = _registration(), _registration()
    resident = [reg.make_cloud(c) for c in clouds]
    res = reg.align_pairs([resident[t] for t, _, _ in pairs], [resident[s] for _, s, _ in pairs], [g for _, _, g in pairs])
    want = [_single(single, resident[t], resident[s], g) for t, s, g in pairs]
    worst = 0.0
    for k in range(len(pairs)):
        worst = max(worst, _assert_bits(res[k], want[k], f"{what}, pair {k}"))
    print(f"{what}: largest relative fitness difference {worst:.3e}; iterations {[r['iterations'] for r in res]}, evaluations {[r['evaluations'] for r in res]}")
    single.close()
    reg.close()
    return res, want


# ---------------------------------------------------------------------------------------------- 1. the bits of today's path
def test_interleaved_targets_give_the_bits_of_the_per_target_path():
    targets, src = _scene()
    rng = np.random.default_rng(11)
    clouds = list(targets)
    pairs = []
    for k in range(9):
        clouds.append(_subset(src, int(rng.integers(500, 4097)), 20 + k))
        pairs.append((k % 3, len(clouds) - 1, _guess(rng)))
    pairs.append((1, 3 + 4, synth.make_transform((2.5, 2.0, 0.5), (0.1, -0.1, 0.8)).astype(np.float32)))   # about 3 m and 0.8 rad off
    res, _ = _against_single(clouds, pairs, "interleaved targets")
    ev = [r["evaluations"] for r in res]
    assert max(ev) >= 2 * min(ev), ev   # the pairs do finish in very different rounds


# ---------------------------------------------------------------------------------------------- 2. slice and size edges
def test_slice_and_size_edges_give_the_bits_of_the_per_target_path():
    """sources of 20 (= k), 256, 257, 513 and 4,096 points: 1, 1, 2, 3 and 16 slices of 256 slots, neighbours on different targets"""
    targets, src = _scene()
    rng = np.random.default_rng(12)
    clouds = list(targets)
    pairs = []
    for j, m in enumerate((K, 256, 257, 513, 4096)):
        clouds.append(src if m == 4096 else _subset(src, m, 40 + j))
        pairs.append(((j + 1) % 3, len(clouds) - 1, _guess(rng)))
    _against_single(clouds, pairs, "slice edges")


# ---------------------------------------------------------------------------------------------- 3, 4. the restatement
@pytest.fixture(scope="module")
def restated(oracle_lib):
    """three pairs, one per target, in ONE align_pairs; the restatement's align of each, computed once"""
    targets, src = _scene()
    rng = np.random.default_rng(13)
    sources = [_subset(src, 1500, 60 + t) for t in range(3)]
    guesses = [_guess(rng) for _ in range(3)]
    reg = _registration()
    res = reg.align_pairs(targets, sources, guesses, compute_fitness=False)
    traj = [reg.pcl_gicp_trajectory(t) for t in range(3)]
    want = [ref.gicp_align(oracle_lib, targets[t], sources[t], guess=guesses[t]) for t in range(3)]
    reg.close()
    return res, traj, want


def test_row_totals_match_the_restatement_per_iteration(restated):
    """The pair on the 4,500-point target, per outer iteration and without BFGS between the two: kept pairs, inner iterations, evaluation
    passes (where the restatement's line searches did not end in roundoff), transformation_ within 1e-5 before the two take different
    trial points and TOL_TRANS after, f within a relative 1e-6 (tests/test_pcl_gicp_gpu.py::_compare's rules, over the pair's record)."""
    res, traj, want = restated[0][2], restated[1][2], restated[2][2]
    assert want["iterations"] >= 1
    assert len(traj["n"]) == want["iterations"] == res["iterations"]
    forked = False
    for k, t in enumerate(want["traj"]):
        assert traj["n"][k] == t["n"], (k, traj["n"][k], t["n"])
        assert traj["inner"][k] == t["inner"], (k, traj["inner"][k], t["inner"])
        if not t["roundoff"]:
            assert traj["passes"][k] == t["passes"], (k, traj["passes"][k], t["passes"])
        forked = forked or traj["passes"][k] != t["passes"]
        tol = TOL_TRANS if forked else 1e-5
        assert np.abs(traj["T"][k] - t["T"]).max() <= tol, (k, np.abs(traj["T"][k] - t["T"]).max())
        assert abs(traj["f"][k] - t["f"]) <= 1e-6 * max(1.0, abs(t["f"])), (k, traj["f"][k], t["f"])
    assert res["converged"] == want["converged"]
    assert res["evaluations"] >= want["iterations"] + sum(t["inner"] for t in want["traj"])
    dt, dr = pose_error(res["T"], want["T"])
    assert dt <= TOL_TRANS and dr <= TOL_ROT, (dt, dr)


def test_one_pair_per_target_matches_the_restatement(restated):
    res, _, want = restated
    for t in range(3):
        assert res[t]["status"] == 0 and res[t]["converged"] == want[t]["converged"], t
        dt, dr = pose_error(res[t]["T"], want[t]["T"])
        assert dt <= TOL_TRANS and dr <= TOL_ROT, (t, dt, dr)


# ---------------------------------------------------------------------------------------------- 5. shared, empty and short clouds
def test_shared_empty_and_short_clouds():
    """Cloud 3 is the target of pairs 0 and 1, the source of pair 6 and both sides of pair 7.  In the middle: an empty target, an empty
    source, a 10-point target and a 10-point source (k = 20).  The dead pairs report their status and their guess; the live ones are
    bit-equal to their single aligns."""
    targets, src = _scene()
    rng = np.random.default_rng(14)
    clouds = list(targets) + [_subset(src, 2000, 70), _subset(src, 1000, 71), _subset(src, 700, 72), EMPTY, _subset(targets[1], 10, 73),
                              _subset(src, 10, 74)]
    g = [_guess(rng) for _ in range(9)]
    pairs = [(3, 4, g[0]), (3, 5, g[1]), (6, 4, g[2]), (1, 6, g[3]), (7, 5, g[4]), (2, 8, g[5]), (2, 3, g[6]), (3, 3, EYE), (6, 6, g[8])]
    status = {2: 3, 3: 4, 4: 1, 5: 1, 8: 3}   # DGS_ERR_NO_TARGET (tested first: pair 8), DGS_ERR_NO_SOURCE, DGS_ERR_INVALID_ARGUMENT
    reg, single = _registration(), _registration()
    resident = [reg.make_cloud(c) for c in clouds]
    res = reg.align_pairs([resident[t] for t, _, _ in pairs], [resident[s] for _, s, _ in pairs], [p[2] for p in pairs])
    for k, (t, s, guess) in enumerate(pairs):
        if k in status:
            assert res[k]["status"] == status[k] and not res[k]["converged"] and np.array_equal(res[k]["T"], guess) and np.isnan(res[k]["fitness"]), (k, res[k])
            assert res[k]["iterations"] == 0 and res[k]["evaluations"] == 0, (k, res[k])
        else:
            _assert_bits(res[k], _single(single, resident[t], resident[s], guess), f"pair {k}")
    dt, dr = pose_error(res[7]["T"], EYE)
    assert res[7]["converged"] and dt <= TOL_TRANS and dr <= TOL_ROT, (dt, dr)


# ---------------------------------------------------------------------------------------------- 6. dead pair first
@pytest.mark.parametrize("dead", ["target", "source", "short target"])
def test_a_dead_pair_with_the_largest_cloud_first_takes_no_room_from_the_live_ones(dead):
    """On a fresh handle pair 0 never becomes active and holds the batch's largest cloud (4,500 points) on its other side; the live pairs
    behind it are small (400 + 300 points).  The slot arrays and the slice table are sized for the live pairs alone."""
    targets, src = _scene()
    rng = np.random.default_rng(15)
    clouds = [EMPTY, targets[2], targets[0], _subset(src, 400, 80), _subset(src, 300, 81), _subset(targets[1], 10, 82)]
    first = {"target": (0, 1), "source": (1, 0), "short target": (5, 1)}[dead] + (_guess(rng),)
    live = [(2, 3, _guess(rng)), (2, 4, _guess(rng))]

    def run(pairs):
        reg = _registration()
        out = reg.align_pairs([clouds[t] for t, _, _ in pairs], [clouds[s] for _, s, _ in pairs], [g for _, _, g in pairs])
        reg.close()
        return out
    alone, res = run(live), run([first] + live)
    assert res[0]["status"] == {"target": 3, "source": 4, "short target": 1}[dead] and not res[0]["converged"] and np.array_equal(res[0]["T"], first[2])
    for k in (0, 1):
        assert alone[k]["converged"] and _assert_bits(res[k + 1], alone[k], f"live pair {k} behind a dead one") == 0.0


# ---------------------------------------------------------------------------------------------- 7. handle state
def test_the_handle_keeps_its_own_target_source_and_result():
    targets, src = _scene()
    rng = np.random.default_rng(16)
    r = _registration()
    r.setInputTarget(targets[1])
    r.setInputSource(_subset(src, 3000, 90))
    r.align()
    before = (r.getFinalTransformation(), r.hasConverged(), r.last_result.iterations, r.last_result.evaluations, r.last_result.score, r.getFitnessScore())
    counts = r.counts()
    assert counts["evaluations"] == before[3] > 0 and counts["target_points"] == 4096 and counts["source_points"] == 3000
    r.align_pairs([targets[0], targets[2]], [_subset(src, 800, 91), _subset(src, 1200, 92)], [_guess(rng), _guess(rng)])
    assert r.counts() == counts
    assert r.getFitnessScore() == before[5] and np.array_equal(r.getFinalTransformation(), before[0])
    assert (r.hasConverged(), r.last_result.iterations, r.last_result.evaluations, r.last_result.score) == before[1:5]
    r.align()   # still its own target and source
    after = (r.getFinalTransformation(), r.hasConverged(), r.last_result.iterations, r.last_result.evaluations, r.last_result.score, r.getFitnessScore())
    assert np.array_equal(after[0], before[0]) and after[1:] == before[1:]


# ---------------------------------------------------------------------------------------------- 8. cache key
def test_a_new_k_recomputes_the_covariances_of_resident_clouds():
    targets, src = _scene()
    rng = np.random.default_rng(17)
    clouds = [targets[0], targets[2], _subset(src, 900, 95), _subset(src, 1300, 96)]
    g = [_guess(rng), _guess(rng)]
    r = _registration()
    resident = [r.make_cloud(c) for c in clouds]
    at20 = r.align_pairs(resident[:2], resident[2:], g)
    r.setCorrespondenceRandomness(10)
    at10 = r.align_pairs(resident[:2], resident[2:], g)
    fresh = _registration(gicp_correspondence_randomness=10)
    want = fresh.align_pairs(clouds[:2], clouds[2:], g)
    for k in range(2):
        assert _assert_bits(at10[k], want[k], f"k = 10, pair {k}") == 0.0
    assert any(not np.array_equal(at10[k]["T"], at20[k]["T"]) or at10[k]["score"] != at20[k]["score"] for k in range(2))   # and k does matter


# ---------------------------------------------------------------------------------------------- 9. other methods, the empty call
def _launches(reg):
    from delta_graph_slam_amd import _lib as L
    return sum(reg.profile_get(k)[1] for k in range(L.K_TRANSFORM + 1))


def test_other_methods_and_the_empty_call():
    targets, src = _scene()
    rng = np.random.default_rng(18)
    g = [_guess(rng), _guess(rng), _guess(rng)]
    pg, omp = _registration(), _registration("GICP_OMP_HIP")
    fg = _registration("FAST_GICP", gicp_max_correspondence_distance=2.0)
    T = [pg.make_cloud(t) for t in targets]
    S = [pg.make_cloud(_subset(src, m, 100 + m)) for m in (600, 1100, 2100)]
    fast_before = fg.align_pairs(T, S, g)       # FAST_GICP's covariances and GICP_HIP's live in separate slots of the cloud
    a = pg.align_pairs(T, S, g)
    b = omp.align_pairs(T, S, g)
    fast_after = fg.align_pairs(T, S, g)
    for k in range(3):
        assert a[k]["status"] == 0 and a[k]["converged"]
        assert _assert_bits(b[k], a[k], f"GICP_OMP_HIP, pair {k}") == 0.0
        assert _assert_bits(fast_after[k], fast_before[k], f"FAST_GICP before and after, pair {k}") == 0.0
    pg.profile_enable(True)
    pg.align_pairs(T[:1], S[:1])
    before = _launches(pg)
    assert before > 0
    assert pg.align_pairs([], []) == [] and pg.align_pairs_records([], []).shape == (0, 20)
    assert pg._lib.dgs_align_pairs_clouds(pg._h, 0, None, None, None, 1, 1e300, None) == 0
    assert _launches(pg) == before
