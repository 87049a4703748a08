"""-m gpu tests of Registration.align_pairs / dgs_align_pairs_clouds (FAST_GICP pairs that each name their own target) against
today's per-target path: setInputTarget(target) + align.  Clouds are synth.planar_pair(n=8192) and slices of it."""
import ctypes as C

import numpy as np
import pytest

from tests import align_pairs_scenes as S
from tests.helpers import TOL_ROT, TOL_TRANS, pose_error

pytestmark = pytest.mark.gpu


def _bits_equal(a, b):
    """transform, flags, counts, score and status of two result dicts, bit for bit"""
    return (np.array_equal(a["T"], b["T"], equal_nan=True) and a["converged"] == b["converged"] and a["iterations"] == b["iterations"]
            and a["evaluations"] == b["evaluations"] and a["status"] == b["status"]
            and np.array_equal(np.float64(a["score"]).view(np.uint64), np.float64(b["score"]).view(np.uint64)))


def _run_pairs(reg, clouds, pairs, resident=None):
    """align_pairs over (target, source, guess) index triples; `resident` maps a cloud index to the DeviceCloud to use for it"""
    pick = (lambda i: resident[i]) if resident is not None else (lambda i: clouds[i])
    return reg.align_pairs([pick(t) for t, _, _ in pairs], [pick(s) for _, s, _ in pairs], [g for _, _, g in pairs])


# ---------------------------------------------------------------------------------------------- 1. same target, same bits
def test_same_target_gives_the_bits_of_align_batch():
    """Same n, same max_n, same cached index and covariances: same launch shape and dealing, so every bit of the optimiser's answer must
    be align_batch's; the fitness comes from the edge scorer's fixed slices instead of the batch scorer's rows: relative 1e-9."""
    tgt, sources, guesses = S.many_sources()
    r = S.make_registration()
    T = r.make_cloud(tgt)
    Ss = [r.make_cloud(s) for s in sources]
    r.setInputTarget(T)
    batch = r.align_batch(Ss, guesses, compute_fitness=True)
    pairs = r.align_pairs([T] * 12, Ss, guesses)
    worst = 0.0
    for k in range(12):
        assert _bits_equal(pairs[k], batch[k]), (k, pairs[k], batch[k])
        if k == 4:
            assert pairs[k]["status"] == 4 and not pairs[k]["converged"] and np.array_equal(pairs[k]["T"], guesses[4]) and np.isnan(pairs[k]["fitness"])
            continue
        df = abs(pairs[k]["fitness"] - batch[k]["fitness"]) / abs(batch[k]["fitness"])
        worst = max(worst, df)
        assert df <= S.FIT_RTOL, (k, pairs[k]["fitness"], batch[k]["fitness"])
    print(f"same target: largest relative fitness difference {worst:.3e}")


# ---------------------------------------------------------------------------------------------- 2. distinct targets
def _check_scene(clouds, pairs, ref, cov_mode=0):
    """The existing batch-against-single comparison on this scene: per target, setInputTarget + align_batch over its pairs against `ref`."""
    batch_reg = S.make_registration(cov_mode)
    for t in sorted({t for t, _, _ in pairs}):
        mine = [k for k, p in enumerate(pairs) if p[0] == t]
        batch_reg.setInputTarget(clouds[t])
        res = batch_reg.align_batch([clouds[pairs[k][1]] for k in mine], [pairs[k][2] for k in mine], compute_fitness=True)
        for k, rb in zip(mine, res):
            S.compare(rb, ref[k], f"scene check, pair {k}")
    batch_reg.close()


@pytest.fixture(scope="module")
def distinct():
    clouds, pairs = S.distinct_pairs()
    ref = S.single_reference(clouds, pairs, key="distinct")
    _check_scene(clouds, pairs, ref)
    assert ref[-1]["iterations"] >= 4 * max(r["iterations"] for r in ref[:-1])   # the poor guess does finish many rounds after the others
    res = _run_pairs(S.make_registration(), clouds, pairs)
    return clouds, pairs, ref, res


def test_distinct_targets_match_the_per_target_path(distinct):
    clouds, pairs, ref, res = distinct
    worst = np.zeros(3)
    for k in range(len(pairs)):
        worst = np.maximum(worst, S.compare(res[k], ref[k], f"pair {k}"))
    print(f"distinct targets: worst differences {worst[0]:.3e} m, {worst[1]:.3e} rad, fitness {worst[2]:.3e} relative; iterations {[r['iterations'] for r in ref]}")


# ---------------------------------------------------------------------------------------------- 3. oracle
def test_distinct_targets_match_the_oracle(distinct, oracle_lib):
    clouds, pairs, ref, res = distinct
    o = oracle_lib.GicpOracle(max_correspondence_distance=S.DMAX)
    for k, (t, s, g) in enumerate(pairs):
        o.set_target(clouds[t])
        o.set_source(clouds[s])
        ro = o.align(g)
        assert res[k]["converged"] == ro["converged"] and res[k]["iterations"] == ro["iterations"], k
        dt, dr = pose_error(res[k]["T"], ro["T"])
        assert dt <= TOL_TRANS and dr <= TOL_ROT, (k, dt, dr)


# ---------------------------------------------------------------------------------------------- 4. edges of the kernels
def _edge_scene():
    """Targets of 1 point, fewer than a leaf, around a leaf (8) and around the level boundaries (64, 512), each with a 200-point source;
    sources of 1, 7, 8, 9 points (a round of a wave is 8) and of 1,003 (no multiple of 8 x the per-wave run, whatever the run) against
    larger targets."""
    tgt, src, _ = S.base()
    clouds, pairs = [], []
    eye = np.eye(4, dtype=np.float32)
    src200 = S.corner_clouds(1, 200)[1]
    clouds.append(src200)
    L, F = S.K_LEAF, S.K_FAN
    for nt in (1, 5, L - 1, L, L + 1, L * F - 1, L * F, L * F + 1, L * F * F - 1, L * F * F, L * F * F + 1):
        clouds.append(S.corner_clouds(nt, 1)[0])
        pairs.append((len(clouds) - 1, 0, eye))
    big = len(clouds)
    clouds.append(S.corner_clouds(L * F * F + 1, 1)[0])
    for ns in (1, S.ROUND_POINTS - 1, S.ROUND_POINTS, S.ROUND_POINTS + 1):
        clouds.append(S.corner_clouds(1, ns)[1])
        pairs.append((big, len(clouds) - 1, eye))
    clouds.append(S.subset(tgt, 4096, 31))
    clouds.append(S.subset(src, 1003, 32))
    pairs.append((len(clouds) - 2, len(clouds) - 1, eye))
    return clouds, pairs


def test_edges_of_the_kernels_match_the_per_target_path():
    clouds, pairs = _edge_scene()
    ref = S.single_reference(clouds, pairs)
    res = _run_pairs(S.make_registration(), clouds, pairs)
    for k in range(len(pairs)):
        S.compare(res[k], ref[k], f"edge pair {k}: target {clouds[pairs[k][0]].shape[0]}, source {clouds[pairs[k][1]].shape[0]}")


def test_one_pair_gives_the_bits_of_align():
    tgt, src, _ = S.base()
    g = S.distinct_pairs()[1][0][2]
    r = S.make_registration()
    T, Sc = r.make_cloud(S.subset(tgt, 5000, 41)), r.make_cloud(S.subset(src, 3000, 42))
    r.setInputTarget(T)        # this path indexes the clouds first
    r.setInputSource(Sc)
    r.align(g)
    lr = r.last_result
    one = r.align_pairs([T], [Sc], [g], compute_fitness=False)[0]
    assert np.array_equal(one["T"], r.getFinalTransformation()) and one["converged"] == r.hasConverged()
    assert (one["iterations"], one["evaluations"], one["status"]) == (lr.iterations, lr.evaluations, lr.status) and one["score"] == lr.score


@pytest.mark.parametrize("n", [33, 70])
def test_many_pairs_of_mixed_sizes_match_the_per_target_path(n):
    """more pairs than one chunk of the dealing's ballots holds at 70; three targets, sources of 300 to 4,096 points"""
    tgt, src, _ = S.base()
    rng = np.random.default_rng(100 + n)
    clouds = [S.subset(tgt, 4096, 51), S.subset(tgt, 2000, 52), S.subset(tgt, 700, 53)]
    for m in (300, 777, 1500, 2048, 3001, 4096):
        clouds.append(src[rng.permutation(8192)[:m]].copy())
    pairs = [(k % 3, 3 + int(rng.integers(0, 6)), synth_guess(rng)) for k in range(n)]
    ref = S.single_reference(clouds, pairs)
    r = S.make_registration()
    resident = [r.make_cloud(c) for c in clouds]
    res = _run_pairs(r, clouds, pairs, resident)
    for k in range(n):
        S.compare(res[k], ref[k], f"pair {k} of {n}")


def synth_guess(rng):
    from delta_graph_slam_amd import synth
    return synth.make_transform(rng.uniform(-0.15, 0.15, 3), rng.uniform(-0.02, 0.02, 3)).astype(np.float32)


def test_empty_clouds_in_the_middle_and_shared_clouds():
    """An empty source and an empty target in the middle: their statuses, the neighbours unaffected.  A cloud as both sides of one pair;
    a cloud that is the target of one pair and the source of another."""
    tgt, src, _ = S.base()
    rng = np.random.default_rng(3)
    empty = np.zeros((0, 4), np.float32)
    eye = np.eye(4, dtype=np.float32)
    clouds = [S.subset(tgt, 4096, 61), S.subset(tgt, 3000, 62), S.subset(src, 2500, 63), S.subset(src, 3500, 64), empty]
    g = [synth_guess(rng) for _ in range(4)]
    pairs = [(0, 2, g[0]), (1, 4, g[1]), (1, 3, g[2]), (4, 2, g[3]), (0, 3, g[3]),
             (0, 0, eye),                    # target and source of one pair
             (2, 3, eye), (1, 2, g[0])]      # cloud 2: target of pair 6, source of pairs 0 and 7
    ref = S.single_reference(clouds, pairs)
    r = S.make_registration()
    resident = [r.make_cloud(c) for c in clouds]
    res = _run_pairs(r, clouds, pairs, resident)
    assert res[1]["status"] == 4 and not res[1]["converged"] and np.array_equal(res[1]["T"], g[1]) and np.isnan(res[1]["fitness"])   # DGS_ERR_NO_SOURCE
    assert res[3]["status"] == 3 and not res[3]["converged"] and np.array_equal(res[3]["T"], g[3]) and np.isnan(res[3]["fitness"])   # DGS_ERR_NO_TARGET
    for k in (0, 2, 4, 5, 6, 7):
        S.compare(res[k], ref[k], f"pair {k}")
    dt, dr = pose_error(res[5]["T"], eye)
    assert res[5]["converged"] and dt < r.params.transformation_epsilon and dr < r.params.gicp_rotation_epsilon, (dt, dr)


@pytest.mark.parametrize("dead", ["target", "source"])
def test_a_dead_pair_with_the_largest_cloud_first_takes_no_room_from_the_live_ones(dead):
    """On a fresh handle: pair 0 has an empty target (or source) and the batch's LARGEST cloud on its other side, the live pairs behind it
    are small.  The work arrays are sized for the live pairs alone (1,400 points, with the allocator's slack 1,814), so a slot of 8,192
    points for the dead pair would put every later pair's correspondences and Mahalanobis matrices past their end."""
    tgt, src, _ = S.base()
    rng = np.random.default_rng(9)
    empty = np.zeros((0, 4), np.float32)
    clouds = [empty, src.copy(), tgt.copy(), S.subset(tgt, 3000, 91), S.subset(src, 1000, 92), S.subset(src, 400, 93)]
    first = (0, 1, synth_guess(rng)) if dead == "target" else (2, 0, synth_guess(rng))
    pairs = [first, (3, 4, synth_guess(rng)), (3, 5, synth_guess(rng))]
    ref = S.single_reference(clouds, pairs)
    res = _run_pairs(S.make_registration(), clouds, pairs)
    assert res[0]["status"] == (3 if dead == "target" else 4) and not res[0]["converged"] and np.array_equal(res[0]["T"], first[2])
    for k in (1, 2):
        S.compare(res[k], ref[k], f"live pair {k} behind a dead one")


# ---------------------------------------------------------------------------------------------- 5. batch independence
def test_fitness_does_not_depend_on_the_batch(distinct):
    """The same pair alone, first in a batch and last in a batch.  The edge scorer's slices are a function of the pair's own source, so the
    fitness of one final transform is the same bits anywhere; the optimiser's sums are formed by as many workgroups as the batch leaves
    the pair, so its double pose moves in the last places -- below the float the final transform is rounded to."""
    clouds, pairs, ref, _ = distinct
    k = 4
    r = S.make_registration()
    resident = [r.make_cloud(c) for c in clouds]
    alone = _run_pairs(r, clouds, [pairs[k]], resident)[0]
    first = _run_pairs(r, clouds, [pairs[k]] + [pairs[j] for j in (0, 2, 8, 9)], resident)[0]
    last = _run_pairs(r, clouds, [pairs[j] for j in (9, 1, 3, 5, 6)] + [pairs[k]], resident)[-1]
    for other in (first, last):
        assert np.float64(other["fitness"]).view(np.uint64) == np.float64(alone["fitness"]).view(np.uint64), (other["fitness"], alone["fitness"])
        dt, dr = pose_error(other["T"], alone["T"])
        assert dt <= S.POSE_TOL[0] and dr <= S.POSE_TOL[1], (dt, dr)
    S.compare(alone, ref[k], "alone")


# ---------------------------------------------------------------------------------------------- 6. handle untouched
def test_the_handle_keeps_its_own_target_source_and_result(distinct):
    clouds, pairs, _, _ = distinct
    tgt, src, _ = S.base()
    r = S.make_registration()
    r.setInputTarget(S.subset(tgt, 6000, 71))
    r.setInputSource(S.subset(src, 4000, 72))
    r.align()
    before = (r.getFinalTransformation(), r.hasConverged(), r.last_result.iterations, r.last_result.evaluations, r.last_result.score, r.getFitnessScore())
    counts = r.counts()
    assert counts["evaluations"] == before[3] > 0
    _run_pairs(r, clouds, pairs[:4])
    assert r.counts() == counts
    assert r.getFitnessScore() == before[5] and np.array_equal(r.getFinalTransformation(), before[0])
    r.align()
    after = (r.getFinalTransformation(), r.hasConverged(), r.last_result.iterations, r.last_result.evaluations, r.last_result.score, r.getFitnessScore())
    assert np.array_equal(after[0], before[0]) and after[1:] == before[1:]


# ---------------------------------------------------------------------------------------------- 7. covariance mode
def test_upstream_order_covariances_are_honoured():
    from delta_graph_slam_amd import _lib as L
    mode = L.GICP_COV["UPSTREAM_ORDER"]
    clouds, pairs = S.distinct_pairs()
    ref = S.single_reference(clouds, pairs, cov_mode=mode, key="distinct")
    _check_scene(clouds, pairs, ref, cov_mode=mode)
    r = S.make_registration(mode)
    resident = [r.make_cloud(c) for c in clouds]
    res = _run_pairs(r, clouds, pairs, resident)
    for k in range(len(pairs)):
        S.compare(res[k], ref[k], f"pair {k}, covariance mode {mode}")
    r.setInputTarget(resident[1])            # the covariances align_pairs left on the cloud ...
    mine = r.gicp_covariances("target")
    other = S.make_registration(mode)        # ... against the existing path's, made for a target of its own
    other.setInputTarget(clouds[1])
    theirs = other.gicp_covariances("target")
    assert mine.shape == theirs.shape == (clouds[1].shape[0], 3, 3) and np.array_equal(mine.view(np.uint64), theirs.view(np.uint64))
    plain = S.make_registration(0)
    plain.setInputTarget(clouds[1])
    assert not np.array_equal(plain.gicp_covariances("target"), mine)   # and the mode does change them


# ---------------------------------------------------------------------------------------------- 8. errors
def _launches(reg):
    from delta_graph_slam_amd import _lib as L
    return sum(reg.profile_get(k)[1] for k in range(L.K_TRANSFORM + 1))


def test_errors_and_the_empty_call():
    from delta_graph_slam_amd import _lib as L
    from delta_graph_slam_amd.registration import DgsError, Registration, RegistrationGroup
    tgt, src, _ = S.base()
    r = S.make_registration()
    T, Sc = r.make_cloud(S.subset(tgt, 2000, 81)), r.make_cloud(S.subset(src, 1000, 82))
    res = (L.Result * 2)()
    with_null = (C.c_void_p * 2)(T._c.value, None)
    ok = (C.c_void_p * 2)(Sc._c.value, Sc._c.value)
    assert r._lib.dgs_align_pairs_clouds(r._h, 2, C.cast(with_null, C.c_void_p), C.cast(ok, C.c_void_p), None, 1, 1e300, res) == 1   # DGS_ERR_INVALID_ARGUMENT
    assert r._lib.dgs_align_pairs_clouds(r._h, 2, C.cast(ok, C.c_void_p), C.cast(with_null, C.c_void_p), None, 1, 1e300, res) == 1
    r.profile_enable(True)
    r.align_pairs([T], [Sc])
    before = _launches(r)
    assert before > 0
    assert r.align_pairs([], []) == [] and r.align_pairs_records([], []).shape == (0, 20)
    assert r.align_pairs([], [], guesses=[]) == [] and r.align_pairs_records([], [], guesses=np.zeros((0, 4, 4), np.float32)).shape == (0, 20)
    assert r._lib.dgs_align_pairs_clouds(r._h, 0, None, None, None, 1, 1e300, None) == 0
    assert _launches(r) == before
    for method, name in (("NDT_OMP", "NDT_OMP"), ("FAST_VGICP", "FAST_VGICP"), ("ICP_HIP", "ICP_HIP")):
        other = Registration(method)
        with pytest.raises(DgsError) as e:
            other.align_pairs([S.subset(tgt, 500, 83)], [S.subset(src, 500, 84)])
        assert e.value.status == 6 and name in str(e.value)   # DGS_ERR_UNSUPPORTED, the method named
        other.close()
    with pytest.raises(NotImplementedError):
        RegistrationGroup.align_pairs(None, [], [])
