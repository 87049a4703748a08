"""CPU proof of tests/line_extraction_edge_cases.py, on the numpy restatement alone: `raw_for_pairs` against R.draw_stream, every case's
`plan` against the restatement's record (so a scene cannot silently miss its edge), the winner's margin of exactly one inlier, the same
discrete trace under both trigonometries, and the tolerance the GPU tests use on the doubles."""
import numpy as np
import pytest

import line_extraction_edge_cases as E
import line_extraction_reference as R

# Largest difference of any A / B coordinate or statistic between the restatement with numpy's float32 trigonometry and with it
# evaluated in float64 and rounded, over every edge case (test_edge_tolerance_spread measures it again).  Every cloud but the planted
# scenes is flat and most are collinear: c0 = 0, the roots come from the quadratic branch, no trigonometry runs.  Measured: 0.
EDGE_SPREAD = 0.0
EDGE_TOL = 4.0 * EDGE_SPREAD


def _counts(cloud, prm, sample):
    p = dict(R.DEFAULTS, **prm)
    p0, u = R.sample_model(cloud[sample[0]], cloud[sample[1]])
    return np.nonzero(R.inlier_mask(cloud, p0, u, p["sac_distance_threshold"], p["sqnorm_order"]))[0]


def first_list(case):
    """The length of a round's first draw list (ln_extract)."""
    p = dict(R.DEFAULTS, **case.params)
    d = p["max_iterations"] + 1 + E.SLACK
    return d if case.raw is None else min(d, len(case.raw) // 2)


def test_raw_for_pairs_reproduces_the_wanted_pairs():
    rng = np.random.default_rng(1)
    for n, count in ((2, 12), (3, 40), (50, 200), (2049, 200)):
        pairs = []
        for d in range(count):
            i0, i1 = rng.choice(n, 2, replace=False)
            pairs.append((int(i0), int(i1)))
        pairs[5:8] = [pairs[4]] * 3                          # a pair repeated: nothing moves
        pairs[9] = pairs[8][::-1]                            # and the same two indices the other way round
        raw = E.raw_for_pairs(n, pairs)
        assert raw.dtype == np.uint32 and raw.shape == (2 * count,)
        st = R.draw_stream(n, raw)
        assert [next(st) for _ in range(count)] == pairs
        with pytest.raises(R.StreamEnd):
            next(st)
    assert list(E.raw_for_pairs(2, [(1, 0), (1, 0), (0, 1)])) == [1, 0, 0, 0, 1, 0]
    with pytest.raises(AssertionError):
        E.raw_for_pairs(5, [(3, 3)])


def test_the_registry_holds_every_case_with_its_aim():
    cs = E.cases()
    assert len(cs) == len(E.NAMES) >= 45
    for name, c in cs.items():
        assert "ln_" in c.aims and c.aims.endswith("."), name
        assert c.cloud.dtype == np.float32 and c.cloud.ndim == 2 and c.cloud.shape[1] == 4 and c.cloud.shape[0] <= 2100, name
        assert dict(R.DEFAULTS, **c.params)["max_rounds"] <= 3 or name in ("n0", "n1_min1", "n2_min2"), name
        assert c.raw is None or c.raw.dtype == np.uint32, name


@pytest.mark.parametrize("name", E.NAMES)
def test_case_hits_its_edge(name):
    c = E.case(name)
    plan, prm = c.plan, dict(R.DEFAULTS, **c.params)
    lines, rounds, status = E.reference(name)
    print(name, status, [(r["n_before"], r["draws"], r["iterations"], r["sample"], r.get("winner_rank"), r["inliers"], r["cluster"], r["emitted"])
                         for r in rounds])
    if "status" in plan:
        assert status == plan["status"]
    assert status not in ("RNG_EXHAUSTED", "STALL") or name == "oversized_and_allowed"
    if "rounds" in plan:
        assert len(rounds) == plan["rounds"]
    # no round but the planned ones asks for a longer draw list
    for k, r in enumerate(rounds):
        if not (k == 0 and plan.get("relaunches", 0)):
            assert r["draws"] <= first_list(c), (k, r["draws"])
    if not rounds:
        return
    r0 = rounds[0]
    for key in ("winner_rank", "iterations", "draws", "inliers", "cluster", "emitted", "sample"):
        if key in plan:
            assert r0.get(key) == plan[key], (key, r0.get(key), plan[key])
    if "bad_draws" in plan:
        assert r0["draws"] - r0["iterations"] == plan["bad_draws"]
    if plan.get("relaunches", 0):
        # the lists ln_extract uploads: x 4 up to the cap and the caller's stream, until one holds every draw the walk takes
        d, grown, cap = first_list(c), 0, (prm["max_iterations"] + 1) * E.BAD_RUN + E.BAD_RUN
        while d < r0["draws"]:
            d, grown = min(len(c.raw) // 2, d * 4, cap), grown + 1
        assert grown == plan["relaunches"]
        if name == "regrow_to_cap":
            assert d == cap < len(c.raw) // 2
    if "runner" in plan:
        # the margin: the runner-up, at a lower rank, counts exactly one inlier fewer -- one missed point of the winner changes the trace
        win, run = _counts(c.cloud, prm, r0["sample"]), _counts(c.cloud, prm, plan["runner"])
        assert win.size == run.size + 1 == E.N_WIN and plan["runner_rank"] < plan["winner_rank"]
        assert np.array_equal(win, r0["inlier_idx"])
        rank = plan["winner_rank"]
        assert r0["iterations"] > (rank // E.CHUNK) * E.CHUNK and rank // E.CHUNK == (rank >= 512) + (rank >= 1024)
        if "late" in plan:
            late = win[win >= plan["late_from"]]
            assert late.size == plan["late"] and win.size - late.size <= run.size          # without them the runner-up stays
            assert np.array_equal(late, np.arange(c.cloud.shape[0] - plan["late"], c.cloud.shape[0]))
            if c.cloud.shape[0] > E.TILE:
                assert plan["late_from"] == E.TILE * ((c.cloud.shape[0] - 1) // E.TILE) and run.max() < plan["late_from"]
    if "components" in plan:
        q = c.cloud[r0["inlier_idx"], :3]
        sizes = sorted((k.size for k in R.components(q, prm["cluster_tolerance"], prm["cluster_inclusive"])), reverse=True)
        assert sizes == plan["components"], sizes
    if "cluster_holds" in plan:
        assert plan["cluster_holds"] in r0["cluster_idx"]
        t = (c.cloud[r0["cluster_idx"], :2].astype(np.float64) - np.array([-3.0, 4.0])) @ np.array(E.DIAG)
        assert plan["cluster_t"][0] - 1e-5 < t.min() and t.max() < plan["cluster_t"][1] + 1e-5       # the middle component
    if plan.get("one_component"):
        assert all(r["cluster"] == r["inliers"] > 0 for r in rounds)
    if "mean" in plan:
        assert r0["mean"] == plan["mean"]
    if "length" in plan:
        assert r0["length"] == plan["length"]


def test_the_named_ranks_sizes_and_chains_are_what_the_names_say():
    for rank in (511, 512, 513, 1023, 1024, 1100):
        assert E.case(f"chunk_rank_{rank}").plan["winner_rank"] == rank
    c = E.case("chunk_and_tile")
    assert c.cloud.shape[0] == 2049 and c.plan["winner_rank"] >= E.CHUNK and c.plan["late_from"] == 2 * E.TILE
    for n in (1023, 1024, 1025, 2049):
        assert E.case(f"tile_tail_{n}").cloud.shape[0] == n
    # the exact chain: one component under <=, singletons under <, as the issue recorded them
    for name, want in (("chain_exact_tol_incl", (40, 40, 1)), ("chain_exact_tol_excl", (40, 1, 0))):
        r0 = E.reference(name)[1][0]
        assert (r0["inliers"], r0["cluster"], r0["emitted"]) == want
    # the diagonal chain: rounding decides, and it decides differently for some link under the two comparisons or the restatement says so
    for name in ("chain_diagonal_tol", "chain_diagonal_tol_excl"):
        c = E.case(name)
        r0 = E.reference(name)[1][0]
        q = c.cloud[r0["inlier_idx"], :3]
        d = (q[:, None, :] - q[None, :, :]).astype(np.float32)
        d2 = ((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]).astype(np.float64)
        near = np.abs(d2 - 0.25) < 1e-5
        print(name, "pairs within 1e-5 of tol2:", int(near.sum()) // 2, "below", int((near & (d2 < 0.25)).sum()) // 2, "equal",
              int((near & (d2 == 0.25)).sum()) // 2, "above", int((near & (d2 > 0.25)).sum()) // 2, "cluster", r0["cluster"])
        assert near.sum() // 2 == 39 and (near & (d2 > 0.25)).any() and (near & (d2 <= 0.25)).any()


def _trace(res):
    lines, rounds, status = res
    return status, len(lines), [(r["n_before"], r["draws"], r["iterations"], r["sample"], r.get("winner_rank"), r["inliers"], r["cluster"], r["emitted"],
                                 r["inlier_idx"].tolist(), r["cluster_idx"].tolist()) for r in rounds]


def test_edge_tolerance_spread():
    """Every case gives the same discrete trace under both trigonometries; the spread of the doubles is EDGE_SPREAD."""
    spread = 0.0
    for name in E.NAMES:
        a, b = E.reference(name), E.reference(name, "f64")
        assert _trace(a) == _trace(b), name
        for x, y in zip(a[0], b[0]):
            for k in x:
                spread = max(spread, float(np.max(np.abs(np.asarray(x[k]) - np.asarray(y[k])))))
    print("edge spread", spread)
    assert spread <= EDGE_SPREAD and EDGE_TOL < 1e-4


def test_edge_thresholds_are_farther_than_the_tolerance():
    seen = 0
    for name in E.NAMES:
        p = dict(R.DEFAULTS, **E.case(name).params)
        for k, r in enumerate(E.reference(name)[1]):
            if "mean" not in r:
                continue
            seen += 1
            dm = abs(r["mean"] - float(np.float32(p["merror_threshold"])))
            dl = abs(r["length"] - float(np.float32(p["line_length_threshold"])))
            if name in E.EQUALITY_CASES and k == 0:
                assert (dm == 0.0) != (dl == 0.0)               # exactly one of the two sits on its threshold
                continue
            assert dm > EDGE_TOL and dl > EDGE_TOL, (name, k, r["mean"], r["length"])
    assert seen > 40
