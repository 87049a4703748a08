"""-m gpu tests of the batch-independent switch (dgs_set_batch_independent).  With the switch on, every dgs_result field of a
pair, and every fitness, is a function of (method parameters, target, source, guess) alone.  FAST_GICP / FAST_VGICP: the fixed layout is the
one a lone default align gets, so the reference of nearly every test here is a single align on a second registration with the switch OFF.
All comparisons are array_equal on transform, converged, iterations, evaluations and score unless a tolerance is named.  Scenes and
guesses: tests/align_pairs_scenes.py."""
import os

import numpy as np
import pytest

from delta_graph_slam_amd import synth
from tests import align_pairs_scenes as S
from tests.helpers import TOL_ROT, TOL_TRANS, pose_error

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "batch_independent_default_records.npz")
CASE1_SIZES = (1, 255, 256, 257, 511, 512, 513, 4096, 5000)     # around kBlock = 256 and 2 kBlock: 1, 2 and 3 slices; 16 and 20 slices
POOR_GUESS = synth.make_transform((2.5, 2.0, 0.5), (0.1, -0.1, 0.8)).astype(np.float32)   # align_pairs_scenes' poor guess: about 3 m, 0.8 rad
_CACHE = {}


def _env(**kv):
    class E:
        def __enter__(self):
            self.old = {k: os.environ.get(k) for k in kv}
            os.environ.update({k: str(v) for k, v in kv.items()})

        def __exit__(self, *a):
            for k, v in self.old.items():
                if v is None:
                    os.environ.pop(k, None)
                else:
                    os.environ[k] = v
    return E()


def _bits(x):
    return np.float64(x).view(np.uint64)


def _same(a, b, fitness=False):
    """transform, flags, counts, status and score of two result dicts, bit for bit (and the fitness when asked)"""
    ok = (np.array_equal(a["T"], b["T"], equal_nan=True) and a["converged"] == b["converged"] and a["iterations"] == b["iterations"]
          and a["evaluations"] == b["evaluations"] and a["status"] == b["status"] and _bits(a["score"]) == _bits(b["score"]))
    return ok and (not fitness or _bits(a["fitness"]) == _bits(b["fitness"]))


def _show(a):
    return (a["iterations"], a["evaluations"], int(a["converged"]), a["status"], float(a["score"]).hex(), float(a["fitness"]).hex(),
            [float(v).hex() for v in a["T"][:3].ravel()])


def _guess(rng):
    return synth.make_transform(rng.uniform(-0.15, 0.15, 3), rng.uniform(-0.02, 0.02, 3)).astype(np.float32)


def _single(reg, source, guess):
    """setInputSource + align + getFitnessScore on `reg` (its target is set) -> a result dict of align_batch's shape"""
    reg.setInputSource(source)
    reg.align(guess)
    lr = reg.last_result
    return dict(T=reg.getFinalTransformation(), converged=reg.hasConverged(), iterations=lr.iterations, evaluations=lr.evaluations, status=lr.status,
                score=lr.score, fitness=reg.getFitnessScore())


def _make(method, on, **kw):
    from delta_graph_slam_amd import _lib as L
    from delta_graph_slam_amd.registration import Registration
    if method == "FAST_GICP":
        return S.make_registration(batch_independent=on, **kw)
    search = kw.pop("search")
    return Registration("FAST_VGICP", vgicp_resolution=1.0, vgicp_search_method=L.VGICP_SEARCH[search], batch_independent=on, **kw)   # tests/test_vgicp_gpu.py's resolution


METHODS = [("FAST_GICP", {}), ("FAST_VGICP", dict(search="DIRECT1")), ("FAST_VGICP", dict(search="DIRECT7"))]
METHOD_IDS = ["FAST_GICP", "FAST_VGICP-DIRECT1", "FAST_VGICP-DIRECT7"]


def _case1_scene():
    if "case1" not in _CACHE:
        tgt, src, _ = S.base()
        rng = np.random.default_rng(601)
        sources = [S.subset(src, m, 600 + k) for k, m in enumerate(CASE1_SIZES)]
        extra = [S.subset(src, 5000, 650 + k) for k in range(3)]
        _CACHE["case1"] = (tgt, sources, [_guess(rng) for _ in sources], extra, [_guess(rng) for _ in extra])
    return _CACHE["case1"]


def _case2_scene():
    """40 pairs: four of 16,384 points (64 slices) among 36 of 2,000 (8 slices); grid_l sits at its 2,048 ceiling, so a large pair has 51
    workgroups for its 64 slices at first and more as the small pairs finish.  Pair 17 carries the poor guess."""
    if "case2" not in _CACHE:
        tgt, src, _ = S.base()
        big = synth.planar_pair(n=16384)[1]
        rng = np.random.default_rng(602)
        small = [S.subset(src, 2000, 700 + k) for k in range(6)]
        sources, guesses = [], []
        for k in range(40):
            is_big = k in (3, 17, 18, 39)
            sources.append(big if is_big else small[k % 6])
            guesses.append(POOR_GUESS if k == 17 else _guess(rng))
        _CACHE["case2"] = (tgt, sources, guesses)
    return _CACHE["case2"]


def _check_against_singles(method, kw, tgt, sources, guesses, compositions, fitness):
    """the batch with the switch ON, in every composition, against each source's own single align on a second registration with the switch
    OFF; compositions: lists of (source, guess) index orders, an index >= len(sources) is not compared"""
    on, off = _make(method, True, **dict(kw)), _make(method, False, **dict(kw))
    assert on.batch_independent is True and off.batch_independent is False
    on.setInputTarget(tgt)
    off.setInputTarget(tgt)
    ref = {}
    bad = []
    first = None
    for order, (srcs, gs, n_compared) in enumerate(compositions):
        res = on.align_batch(srcs, gs, compute_fitness=fitness)
        for pos, k in enumerate(n_compared):
            if k is None:
                continue
            if k not in ref:
                ref[k] = _single(off, sources[k], guesses[k])
            r, s = res[pos], ref[k]
            if not _same(r, s):
                bad.append((order, k, sources[k].shape[0], _show(r), _show(s)))
            if fitness:   # the same float distances through other rows: relative 1e-9 against the switch-off value (DESIGN.md 6n's figure)
                assert abs(r["fitness"] - s["fitness"]) <= S.FIT_RTOL * abs(s["fitness"]), (order, k, r["fitness"], s["fitness"])
        if first is None:
            first = (res, n_compared)
        elif fitness:   # a pair's fitness is the same bits in every composition
            by_k = {k: first[0][pos] for pos, k in enumerate(first[1]) if k is not None}
            for pos, k in enumerate(n_compared):
                if k is not None:
                    assert _bits(res[pos]["fitness"]) == _bits(by_k[k]["fitness"]), (order, k, res[pos]["fitness"], by_k[k]["fitness"])
    iters = sorted({(sources[k].shape[0], ref[k]["iterations"]) for k in ref})
    print(f"{method} {kw}: {len(ref)} pairs, (points, iterations) {iters[:12]}, mismatches {len(bad)}")
    for b in bad[:6]:
        print("  mismatch (composition, pair, points, got, single):", b)
    assert not bad, [b[:3] for b in bad]
    return on, off, ref, first[0]


# ---------------------------------------------------------------------------------------------- 1 / 5 / 8: align_batch, slice edges, compositions
@pytest.mark.parametrize("method,kw", METHODS, ids=METHOD_IDS)
def test_align_batch_pairs_carry_the_bits_of_their_single_aligns(method, kw):
    """One target of 8,192 points, sources of 1 .. 5,000 points in one batch: each equals its single align with the switch off; reversed
    and with three more 5,000-point sources the records are the same.  Fitness (case 8): equal bits alone, in the batch and in the
    permuted batch, within 1e-9 relative of the switch-off value, and getFitnessScore() after a single align equals the batch's entry."""
    tgt, sources, guesses, extra, extra_g = _case1_scene()
    n = len(sources)
    idx = list(range(n))
    comps = [(sources, guesses, idx),
             (sources[::-1], guesses[::-1], idx[::-1]),
             (extra[:2] + sources + extra[2:], extra_g[:2] + guesses + extra_g[2:], [None, None] + idx + [None])]
    on, off, ref, res = _check_against_singles(method, kw, tgt, sources, guesses, comps, fitness=True)
    for k in (0, 3, 8):   # alone on the switched-on handle: align + getFitnessScore against the batch's entry
        alone = _single(on, sources[k], guesses[k])
        assert _same(alone, res[k], fitness=True), (k, _show(alone), _show(res[k]))
        one = on.align_batch([sources[k]], [guesses[k]], compute_fitness=True)[0]
        assert _same(one, res[k], fitness=True), (k, _show(one), _show(res[k]))


# ---------------------------------------------------------------------------------------------- 2 / 5: fewer workgroups than slices, re-dealt across rounds
@pytest.mark.parametrize("method,kw", METHODS, ids=METHOD_IDS)
def test_fewer_workgroups_than_slices_and_redealing_across_rounds(method, kw):
    tgt, sources, guesses = _case2_scene()
    idx = list(range(40))
    on, off, ref, res = _check_against_singles(method, kw, tgt, sources, guesses, [(sources, guesses, idx)], fitness=False)
    small = max(ref[k]["evaluations"] for k in idx if sources[k].shape[0] == 2000)
    if method == "FAST_GICP":   # the poor guess does run on after the small pairs have finished: the large pair's share of workgroups changes
        assert ref[17]["evaluations"] > small, (ref[17]["evaluations"], small)


# ---------------------------------------------------------------------------------------------- 3: the 512-slice cap
def test_the_512_slice_cap():
    """140,000 points: ceil(n / 256) = 547 slices are capped at 512, so slices 0 .. 34 take a second stretch; beside seven pairs of 3,000."""
    tgt, src, _ = S.base()
    big = synth.planar_pair(n=140000)[1]
    rng = np.random.default_rng(603)
    sources = [S.subset(src, 3000, 800 + k) for k in range(3)] + [big] + [S.subset(src, 3000, 810 + k) for k in range(4)]
    guesses = [_guess(rng) for _ in sources]
    _check_against_singles("FAST_GICP", {}, tgt, sources, guesses, [(sources, guesses, list(range(8)))], fitness=False)


# ---------------------------------------------------------------------------------------------- 4: fused against unfused
def test_unfused_rounds_give_the_fused_records():
    tgt, sources, guesses, _, _ = _case1_scene()
    fused = _make("FAST_GICP", True)
    fused.setInputTarget(tgt)
    a = fused.align_batch(sources, guesses, compute_fitness=False)
    with _env(DGS_GICP_FUSED=0):
        unfused = _make("FAST_GICP", True)      # the environment is read at dgs_create
    unfused.setInputTarget(tgt)
    b = unfused.align_batch(sources, guesses, compute_fitness=False)
    for k in range(len(sources)):
        assert _same(a[k], b[k]), (k, _show(a[k]), _show(b[k]))
    big_t, big_s, big_g = _case2_scene()
    fused.setInputTarget(big_t)
    unfused.setInputTarget(big_t)
    a, b = fused.align_batch(big_s, big_g, compute_fitness=False), unfused.align_batch(big_s, big_g, compute_fitness=False)
    for k in range(40):
        assert _same(a[k], b[k]), (k, _show(a[k]), _show(b[k]))


# ---------------------------------------------------------------------------------------------- 6 / 8 / 13: align_pairs
@pytest.fixture(scope="module")
def pairs_scene():
    """The three-target scene of tests/test_align_pairs_gpu.py (8,192 / 5,000 / 4,500 points, 9 interleaved pairs and the poor-guess one)
    with dead pairs in front and in the middle; switch on.  References: setInputTarget(the same DeviceCloud) + align, switch off."""
    clouds, live = S.distinct_pairs()
    clouds = list(clouds) + [np.zeros((0, 4), np.float32)]
    empty = len(clouds) - 1
    eye = np.eye(4, dtype=np.float32)
    pairs = [(empty, 3, eye)] + list(live[:5]) + [(1, empty, eye), (empty, empty, eye)] + list(live[5:])   # dead in front and in the middle
    on, off = S.make_registration(batch_independent=True), S.make_registration()
    res_clouds = [on.make_cloud(c) for c in clouds]
    res = on.align_pairs([res_clouds[t] for t, _, _ in pairs], [res_clouds[s] for _, s, _ in pairs], [g for _, _, g in pairs], compute_fitness=True)
    ref = []
    for t, s, g in pairs:
        if clouds[t].shape[0] == 0 or clouds[s].shape[0] == 0:
            ref.append(None)
            continue
        off.setInputTarget(res_clouds[t])
        ref.append(_single(off, res_clouds[s], g))
    return clouds, pairs, res, ref, on, res_clouds


def test_align_pairs_carry_the_bits_of_their_single_aligns(pairs_scene):
    clouds, pairs, res, ref, on, res_clouds = pairs_scene
    eye = np.eye(4, dtype=np.float32)
    assert res[0]["status"] == 3 and res[7]["status"] == 3 and res[6]["status"] == 4     # no target (first of all), no source: as in DESIGN.md 6n
    for k in (0, 6, 7):
        assert not res[k]["converged"] and np.array_equal(res[k]["T"], eye) and np.isnan(res[k]["fitness"])
    bad = [(k, _show(res[k]), _show(ref[k])) for k in range(len(pairs)) if ref[k] is not None and not _same(res[k], ref[k])]
    print(f"align_pairs: iterations {[r['iterations'] for r in ref if r is not None]}, mismatches {len(bad)}")
    assert not bad, bad[:3]
    for k in range(len(pairs)):
        if ref[k] is not None:
            assert abs(res[k]["fitness"] - ref[k]["fitness"]) <= S.FIT_RTOL * abs(ref[k]["fitness"]), (k, res[k]["fitness"], ref[k]["fitness"])


def test_align_pairs_fitness_is_the_single_fitness_in_any_batch(pairs_scene):
    """Case 8 on the pairs scene: a pair alone, the permuted batch, and getFitnessScore() after a single align on the switched-on handle."""
    clouds, pairs, res, ref, on, rc = pairs_scene
    live = [k for k in range(len(pairs)) if ref[k] is not None]
    perm = live[::-1]
    again = on.align_pairs([rc[pairs[k][0]] for k in perm], [rc[pairs[k][1]] for k in perm], [pairs[k][2] for k in perm], compute_fitness=True)
    for pos, k in enumerate(perm):
        assert _same(again[pos], res[k], fitness=True), (k, _show(again[pos]), _show(res[k]))
    for k in (live[0], live[-1]):
        t, s, g = pairs[k]
        alone = on.align_pairs([rc[t]], [rc[s]], [g], compute_fitness=True)[0]
        assert _same(alone, res[k], fitness=True), (k, _show(alone), _show(res[k]))
        on.setInputTarget(rc[t])
        single = _single(on, rc[s], g)
        assert _same(single, res[k], fitness=True), (k, _show(single), _show(res[k]))


def test_align_pairs_meet_the_oracle(pairs_scene, oracle_lib):
    clouds, pairs, res, ref, _, _ = pairs_scene
    o = oracle_lib.GicpOracle(max_correspondence_distance=S.DMAX)
    for k, (t, s, g) in enumerate(pairs):
        if ref[k] is None:
            continue
        o.set_target(clouds[t])
        o.set_source(clouds[s])
        ro = o.align(g)
        dt, dr = pose_error(res[k]["T"], ro["T"])
        assert dt <= TOL_TRANS and dr <= TOL_ROT, (k, dt, dr)


# ---------------------------------------------------------------------------------------------- 7: exact ties
def _tie_scenes():
    tgt, src, _ = S.base()
    half = S.subset(tgt, 2048, 900)
    doubled = np.concatenate([half, half], 0)                      # every target point occurs twice: each NN is a tie of i and i + 2,048
    ax = np.arange(16, dtype=np.float32) * 0.25                    # lattice, spacing 0.25 m: multiples of 2^-2, exact in float
    lat = np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), -1).reshape(-1, 3)
    lattice = np.concatenate([lat, np.ones((4096, 1), np.float32)], 1).astype(np.float32)
    shifted = S.subset(lattice, 1000, 901)
    shifted[:, :3] += np.float32(0.125)                            # half a spacing: under the identity guess every point has 8 nearest lattice points
    return [("doubled", doubled, S.subset(src, 1000, 902), None), ("lattice", lattice, shifted, np.eye(4, dtype=np.float32))]


@pytest.mark.parametrize("which", [0, 1], ids=["doubled", "lattice"])
def test_exact_ties_resolve_the_same_alone_and_in_a_batch(which):
    """gicp_correspond_kernel's result per point is (exact minimum distance, lowest index among the points at that distance) whatever bound
    the walk starts from, so a tie cannot follow the launch shape: alone, in a batch of 9 and in a single align the records are equal.
    (dgs_gicp_linearize probes one pair on one handle and returns sums, not `corr`: records only.)"""
    name, target, source, g0 = _tie_scenes()[which]
    _, src, _ = S.base()
    rng = np.random.default_rng(903)
    g = _guess(rng) if g0 is None else g0
    others = [S.subset(src, m, 910 + k) for k, m in enumerate((300, 4096, 1000, 2500, 77, 5000, 1234, 640))]
    on, off = S.make_registration(batch_independent=True), S.make_registration()
    on.setInputTarget(target)
    off.setInputTarget(target)
    alone = on.align_batch([source], [g], compute_fitness=True)[0]
    batch = on.align_batch(others[:4] + [source] + others[4:], [_guess(rng) for _ in range(4)] + [g] + [_guess(rng) for _ in range(4)], compute_fitness=True)[4]
    single = _single(off, source, g)
    print(f"ties, {name}: iterations {alone['iterations']}, evaluations {alone['evaluations']}, score {alone['score']:.6g}")
    assert _same(alone, batch, fitness=True), (_show(alone), _show(batch))
    assert _same(alone, single), (_show(alone), _show(single))


# ---------------------------------------------------------------------------------------------- 9: NDT and the other methods
def test_ndt_upstream_order_takes_the_fixed_slices_through_the_setter():
    from delta_graph_slam_amd.registration import DgsError, Registration
    tgt, src, _ = S.base()
    rng = np.random.default_rng(904)
    sources = [S.subset(src, 4000, 920 + k) for k in range(8)]
    guesses = [_guess(rng) for _ in sources]
    kw = dict(ndt_resolution=1.0)                     # ndt_strict_order 1 and DIRECT7 are the defaults
    with _env(DGS_NDT_FIXED_SLICES=1):
        by_env = Registration("NDT_OMP", **kw)
    by_setter = Registration("NDT_OMP", **kw)
    assert by_setter.batch_independent is False
    by_setter.set_batch_independent(True)
    assert by_setter.batch_independent is True and by_env.batch_independent is False
    by_env.setInputTarget(tgt)
    by_setter.setInputTarget(tgt)
    a = by_env.align_batch(sources, guesses, compute_fitness=False)
    b = by_setter.align_batch(sources, guesses, compute_fitness=True)
    for k in range(8):
        assert _same(a[k], b[k]), (k, _show(a[k]), _show(b[k]))
    for k in (0, 5):                                  # alone and in the batch of 8: equal, fitness included
        one = by_setter.align_batch([sources[k]], [guesses[k]], compute_fitness=True)[0]
        assert _same(one, b[k], fitness=True), (k, _show(one), _show(b[k]))
        single = _single(by_setter, sources[k], guesses[k])
        assert _same(single, b[k], fitness=True), (k, _show(single), _show(b[k]))
    plain = Registration("NDT_OMP", **kw)             # against the default fitness: the same float distances through other rows
    plain.setInputTarget(tgt)
    c = plain.align_batch(sources, guesses, compute_fitness=True)
    for k in range(8):
        if np.array_equal(c[k]["T"], b[k]["T"]):
            assert abs(c[k]["fitness"] - b[k]["fitness"]) <= S.FIT_RTOL * abs(c[k]["fitness"]), (k, c[k]["fitness"], b[k]["fitness"])
    fast = Registration("NDT_OMP", ndt_strict_order=0, **kw)
    with pytest.raises(DgsError) as e:
        fast.set_batch_independent(True)
    assert e.value.status == 6 and "fast order" in str(e.value) and fast.batch_independent is False   # DGS_ERR_UNSUPPORTED, with the reason
    with pytest.raises(DgsError) as e:
        Registration("NDT_OMP", ndt_strict_order=0, batch_independent=True, **kw)
    assert e.value.status == 6
    with _env(DGS_NDT_STRICT_KERNEL=2):
        lane_per_point = Registration("NDT_OMP", **kw)
    with pytest.raises(DgsError) as e:
        lane_per_point.set_batch_independent(True)
    assert e.value.status == 6 and "DGS_NDT_STRICT_KERNEL" in str(e.value)


@pytest.mark.parametrize("method,kw", [("ICP_HIP", dict(gicp_max_correspondence_distance=S.DMAX)), ("GICP_HIP", dict(gicp_max_correspondence_distance=S.DMAX)),
                                       ("PCL_NDT_HIP", dict(ndt_resolution=1.0)), ("NDT_OMP", dict(ndt_resolution=1.0, ndt_strict_order=2))])
def test_methods_with_fixed_sums_accept_the_switch_and_only_reroute_their_fitness(method, kw):
    from delta_graph_slam_amd.registration import Registration
    tgt, src, _ = S.base()
    rng = np.random.default_rng(905)
    sources = [S.subset(src, m, 930 + k) for k, m in enumerate((1500, 3000, 700, 2200))]
    guesses = [_guess(rng) for _ in sources]
    on, off = Registration(method, batch_independent=True, **kw), Registration(method, **kw)
    assert on.batch_independent is True
    on.setInputTarget(tgt)
    off.setInputTarget(tgt)
    a, b = on.align_batch(sources, guesses, compute_fitness=True), off.align_batch(sources, guesses, compute_fitness=True)
    for k in range(4):
        assert _same(a[k], b[k]), (method, k, _show(a[k]), _show(b[k]))     # the sums do not move
        assert abs(a[k]["fitness"] - b[k]["fitness"]) <= S.FIT_RTOL * abs(b[k]["fitness"]), (method, k, a[k]["fitness"], b[k]["fitness"])
    one = on.align_batch([sources[2]], [guesses[2]], compute_fitness=True)[0]
    assert _same(one, a[2], fitness=True), (method, _show(one), _show(a[2]))
    assert _same(_single(on, sources[2], guesses[2]), a[2], fitness=True)


# ---------------------------------------------------------------------------------------------- 10: group
def test_groups_of_one_two_and_four_members_give_the_same_records():
    from delta_graph_slam_amd.registration import RegistrationGroup
    tgt, src, _ = S.base()
    rng = np.random.default_rng(906)
    sources = [S.subset(src, 3000, 940 + k) for k in range(16)]
    guesses = [_guess(rng) for _ in sources]
    records = []
    for devices in ((0,), (0, 0), (0, 0, 0, 0)):
        g = RegistrationGroup("FAST_GICP", devices=devices, gicp_max_correspondence_distance=S.DMAX, batch_independent=True)
        assert g.batch_independent is True
        g.setInputTarget(tgt)
        records.append(g.align_batch(sources, guesses, compute_fitness=True))
        g.close()
    for other in records[1:]:
        for k in range(16):
            assert _same(records[0][k], other[k], fitness=True), (k, _show(records[0][k]), _show(other[k]))
    single = S.make_registration()      # and each is its single align with the switch off
    single.setInputTarget(tgt)
    for k in (0, 7, 15):
        assert _same(records[0][k], _single(single, sources[k], guesses[k])), k


# ---------------------------------------------------------------------------------------------- 11: loop detector
def _se2(x, y, yaw):
    c, s = np.cos(yaw), np.sin(yaw)
    return np.array([[c, -s, x], [s, c, y], [0, 0, 1]], np.float64)


def _tick():
    """The tick of tests/test_loop_detector_batched_gpu.py: 8 old keyframes and 4 new ones that all see the same planar scene from slightly
    different poses (4,096 points each, drawn apart); the second new keyframe is gated out by the first's loop, the last two are not."""
    from delta_graph_slam_amd.loop_detector import KeyFrame
    world, _, _ = synth.planar_pair(n=8192)
    rng = np.random.default_rng(77)

    def keyframe(kid, x, y, yaw, accum, sigma):
        est = _se2(x, y, yaw)
        T = np.eye(4)
        T[:2, :2], T[:2, 3] = est[:2, :2], est[:2, 2]
        pts = S.subset(world, 4096, 1000 + kid)
        pts[:, :3] += rng.normal(0.0, sigma, (4096, 3)).astype(np.float32)
        return KeyFrame(cloud=synth.apply_transform(np.linalg.inv(T), pts).astype(np.float32), estimate=est + 0.0, accum_distance=accum, id=kid)

    place = [0, 0, 0, 1, 1, 2, 2, 2]
    old = [keyframe(k, 8.0 * place[k] + 0.3 * (k % 3), -0.2 * (k % 3), 0.01 * k, 2.0 * k, 0.01 + 0.01 * k) for k in range(8)]
    new = [keyframe(8, 0.5, 0.3, 0.02, 40.0, 0.01), keyframe(9, 0.7, 0.2, 0.03, 40.5, 0.01),
           keyframe(10, 8.3, 0.2, -0.02, 46.0, 0.01), keyframe(11, 16.2, -0.3, 0.04, 52.0, 0.01)]
    for k, nk in enumerate(new):
        nk.estimate = nk.estimate @ _se2(0.05 * (k + 1), -0.04, 0.004 * (k + 1))
    return old, new


def test_the_batched_tick_equals_the_sequential_tick_bit_for_bit():
    from delta_graph_slam_amd.loop_detector import LoopDetector
    old, new = _tick()
    params = dict(distance_thresh=5.0, accum_distance_thresh=15.0, min_edge_interval=5.0, fitness_score_thresh=0.5)
    seq = LoopDetector(params, registration=S.make_registration(batch_independent=True), cache_clouds=True, batch_new_keyframes=False)
    bat = LoopDetector(params, registration=S.make_registration(batch_independent=True), cache_clouds=True, batch_new_keyframes=True)
    loops_seq = seq.detect(old, new)
    loops_bat = bat.detect_batched(old, new)
    assert len(loops_seq) == 3
    assert [(l.key1.id, l.key2.id) for l in loops_bat] == [(l.key1.id, l.key2.id) for l in loops_seq]
    assert bat.last_edge_accum_distance == seq.last_edge_accum_distance
    for a, b in zip(loops_bat, loops_seq):
        assert np.array_equal(a.relative_pose, b.relative_pose), (a.key1.id, pose_error(a.relative_pose, b.relative_pose))
        assert _bits(a.score) == _bits(b.score), (a.key1.id, a.score, b.score)


# ---------------------------------------------------------------------------------------------- 12: the default is untouched
def test_the_default_is_untouched():
    """With the switch never set, case 1's batch gives the records the library gave before it knew the switch (tests/golden/
    batch_independent_default_records.npz: written by the parent commit's library, which has none of the new symbols, on an MI355X); after
    set_batch_independent(True) then (False) the records equal the never-set ones."""
    tgt, sources, guesses, _, _ = _case1_scene()
    never = S.make_registration()
    never.setInputTarget(tgt)
    a = never.align_batch(sources, guesses, compute_fitness=True)
    toggled = S.make_registration()
    toggled.set_batch_independent(True)
    toggled.setInputTarget(tgt)
    toggled.align_batch(sources, guesses, compute_fitness=True)
    toggled.set_batch_independent(False)
    assert toggled.batch_independent is False
    b = toggled.align_batch(sources, guesses, compute_fitness=True)
    for k in range(len(sources)):
        assert _same(a[k], b[k], fitness=True), (k, _show(a[k]), _show(b[k]))
    G = np.load(GOLDEN)
    assert G["sizes"].tolist() == list(CASE1_SIZES)
    for k in range(len(sources)):
        assert np.array_equal(a[k]["T"], G["T"][k]) and int(a[k]["converged"]) == G["converged"][k], k
        assert (a[k]["iterations"], a[k]["evaluations"], a[k]["status"]) == (G["iterations"][k], G["evaluations"][k], G["status"][k]), k
        assert _bits(a[k]["score"]) == G["score_bits"][k] and _bits(a[k]["fitness"]) == G["fitness_bits"][k], k
