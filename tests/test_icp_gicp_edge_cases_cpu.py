"""CPU proof of tests/icp_gicp_edge_cases.py, on the two restatements alone (tests/icp_reference.py, tests/pcl_gicp_reference.py): every
case's `plan` against the restatement's record (so a scene cannot silently miss its edge); the stability condition the exact count
comparison on the GPU rests on, with no case exempt (gate margins; ICP under T_k nudged by one ulp; GICP under perturbed functor sums);
the rank of H of the degenerate fits and the sign of det H where the flip decides; which GICP iterations end a line search in roundoff
(`forks`, read by tests/test_icp_gicp_edges_gpu.py)."""
import math

import numpy as np
import pytest

import icp_gicp_edge_cases as E
from helpers import f32_sqdist, f32_transform
from test_pcl_gicp_gpu import _nondegenerate

MARGIN = 1e-3                 # every unplanted d2 of every pass stays this far, relatively, from max^2
# PCL's `delta < 1` after an outer GICP iteration.  Where a line search ended in roundoff the device may accept a state up to the
# final-pose tolerance away (helpers.TOL_TRANS = 1e-4 m against transformation_epsilon = 0.01, TOL_ROT = 1e-5 against 2e-3: 0.02 of delta
# for the two poses of a difference); elsewhere the states agree to 1e-5 (0.01 of delta).  A delta that decides -- the iteration cap
# does not already end the loop there -- must be five times farther from 1 than that.
DELTA_MARGIN = 0.1


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle
    return oracle


def forks(orc, name):
    """Per outer iteration of the GICP restatement: did a line search end in roundoff there?  The GPU file compares the evaluation
    passes of the other iterations exactly (test_pcl_gicp_gpu._compare's own rule)."""
    return [t["roundoff"] for t in E.reference(orc, name, E.GICP)["traj"]]


def _kept(r):
    return [int(p["keep"].sum()) for p in r["trace"]]


def test_the_registry_holds_every_family_with_its_aim():
    assert len(E.NAMES) == len(set(E.NAMES)) == len(E.CASES) >= 60
    assert {c.family for c in E.CASES.values()} == set(E.FAMILIES)
    tgt, src = E.pair()
    for name, c in E.CASES.items():
        assert c.aim.endswith(".") and len(c.aim) > 40, name
        assert set(c.method) <= {E.ICP, E.GICP} and c.method, name
        for cloud in (c.tgt, c.src):
            assert cloud.dtype == np.float32 and cloud.ndim == 2 and cloud.shape[1] == 4, name
            assert cloud.shape[0] <= E.MAX_POINTS or name in E.OVERSIZE, name
        assert c.guess is None or (c.guess.dtype == np.float32 and c.guess.shape == (4, 4)), name
        assert c.plan.get("pose_compared", True) or name in ("collinear", "coincident"), name
    assert not E.case("collinear").plan["pose_compared"] and not E.case("coincident").plan["pose_compared"]
    assert [E.case(n).src.shape[0] for n in E.OVERSIZE] == [256 * 31 + 1, 256 * 32 + 1]
    # the sizes, slice counts and caps the families must hold
    sizes = {m: sorted(c.src.shape[0] for n, c in E.CASES.items() if c.family == "sizes" and c.method == (m,) and "_k" not in n) for m in (E.ICP, E.GICP)}
    assert sizes[E.ICP] == [1, 2, 3, 7, 8, 9, 63, 64, 65, 255, 256, 257, 511, 513]
    assert sizes[E.GICP] == [20, 21, 63, 64, 65, 255, 256, 257, 513]
    for edge in (E.RUN, E.WAVE, E.SLICE):                                  # one 8-slot group, one wave, one slice: a slot short, full, one over
        assert {edge - 1, edge, edge + 1} <= set(sizes[E.ICP]) and (edge == E.RUN or {edge - 1, edge, edge + 1} <= set(sizes[E.GICP]))
    c = E.case("size_gicp_k20_n20")
    assert c.tgt.shape[0] == c.src.shape[0] == 20 == E.settings(c, E.GICP)["gicp_correspondence_randomness"]
    assert [(E.case(f"size_gicp_k5_n{n}").src.shape[0], E.settings(E.case(f"size_gicp_k5_n{n}"), E.GICP)["gicp_correspondence_randomness"]) for n in (5, 9)] == [(5, 5), (9, 5)]
    rows = {m: sorted(c.plan["n_slices"] for c in E.CASES.values() if c.family == "rows" and c.method == (m,)) for m in (E.ICP, E.GICP)}
    assert rows == {E.ICP: [7, 8, 9, 16, 17], E.GICP: [15, 16, 17, 32, 33]}
    for m in (E.ICP, E.GICP):
        G = E.ROW_GROUPS[m]
        assert {G - 1, G, G + 1, 2 * G, 2 * G + 1} == set(rows[m])
    assert sorted(E.settings(c, E.ICP)["gicp_max_correspondence_distance"] for c in E.CASES.values() if c.family == "gate") == [0.1, 1.7, 2.5, 2.5]
    assert sorted(c.plan["origin"] for c in E.CASES.values() if c.family == "origin" and c.plan["origin"] is not None) == [0, 63, 64, 255, 256, 257]
    for it in (0, 1, 2):
        c = E.case(f"cap_{it}")
        assert c.method == (E.ICP, E.GICP) and c.src.shape[0] == 257 and E.settings(c, E.GICP)["maximum_iterations"] == it
    # deterministic: the base pair is the seeded generator's, the extension adds float-exact offsets well inside the gate
    from delta_graph_slam_amd import synth
    t2, s2, _ = synth.planar_pair(4096)
    assert np.array_equal(tgt, t2.astype(np.float32)) and np.array_equal(src, s2.astype(np.float32))
    ext = E.extended_source(4353)
    assert np.array_equal(ext[:4096], src) and np.array_equal(ext[4096:, :3], src[:257, :3] + np.asarray(E.JITTER, np.float32))
    assert float(np.linalg.norm(np.asarray(E.JITTER, np.float64))) < 0.05


@pytest.mark.parametrize("name,method", E.RUNS)
def test_case_hits_its_edge(orc, name, method):
    c = E.case(name)
    p = E.settings(c, method)
    r = E.reference(orc, name, method)
    kept, tr = _kept(r), r["trace"]
    print(name, method, "--", c.aim)
    print("   iterations", r["iterations"], "converged", r["converged"], "evaluations", r["evaluations"], "kept", kept)
    n = c.src.shape[0]
    assert len(tr) >= 1 and all(t["d2"].shape == (n,) for t in tr)
    if E.planned(c, method, "kept_first") is not None:
        assert kept[0] == E.planned(c, method, "kept_first")
    if "kept" in c.plan:
        assert kept == c.plan["kept"]
    if "n" in c.plan:
        assert n == c.plan["n"]
    if "n_slices" in c.plan:
        G = E.ROW_GROUPS[method]
        s = c.plan["n_slices"]
        assert math.ceil(n / E.SLICE) == s and (n == E.SLICE * G if s == G else n == E.SLICE * (s - 1) + 1)
    rec = E.planned(c, method, "record")
    if rec:
        for key in ("iterations", "converged", "evaluations"):
            if key in rec:
                assert r[key] == rec[key], (key, r[key], rec[key])
        if rec.get("runs"):
            assert r["iterations"] >= 1 and r["converged"]
    if c.family == "min_count" and name != "min_second_pass":
        m = kept[0]
        assert np.array_equal(np.nonzero(tr[0]["keep"])[0], np.arange(m))                  # the m points that stayed, nothing else
        assert (m < E.MIN_PAIRS[method]) == (r["iterations"] == 0) and m in (E.MIN_PAIRS[method] - 1, E.MIN_PAIRS[method])
    if name == "min_second_pass":
        assert kept[0] >= E.MIN_PAIRS[method] > kept[1] and len(kept) == 2
    if c.family == "gate":
        m2, g = E.gate_floats(p["gicp_max_correspondence_distance"])
        assert p["maximum_iterations"] == 1 and len(tr) == 1
        assert float(g) <= m2 < float(np.nextafter(g, np.float32(np.inf))) and c.plan["gate_is_float"] == (float(g) == m2)
        W = f32_transform(np.eye(4, dtype=np.float32) if c.guess is None else c.guess, c.src[:, :3])
        want = E.planned(c, method, "kept_planted")
        for side, i in c.plan["planted"].items():
            d2 = tr[0]["d2"][i]
            assert d2 == f32_sqdist(W[i], c.tgt[c.plan["home"], :3]) == np.float32(c.plan["d2"][side]), (side, d2)
            assert tr[0]["j"][i] == c.plan["home"] and np.all(c.tgt[c.plan["home"], :3] == 0)
            assert bool(tr[0]["keep"][i]) == want[side], (side, d2, m2)
            others = np.delete(np.arange(c.tgt.shape[0]), c.plan["home"])
            assert f32_sqdist(W[i], c.tgt[others, :3]).min() > 4 * m2                          # its only near target
        d = c.plan["d2"]
        assert np.nextafter(np.float32(d["on"]), np.float32(0)) == np.float32(d["below"]) and np.nextafter(np.float32(d["on"]), np.float32(np.inf)) == np.float32(d["above"])
        assert np.float32(d["on"]) == g
        # ICP keeps the point on the gate; GICP drops it exactly when max^2 is a float
        assert E.planned(c, E.ICP, "kept_planted")["on"] and E.planned(c, E.GICP, "kept_planted")["on"] == (not c.plan["gate_is_float"])
    if "rank" in c.plan:
        t0 = tr[0]
        P = t0["W"][t0["keep"]].astype(np.float64) - t0["o"]
        Q = c.tgt[t0["j"][t0["keep"]], :3].astype(np.float64) - t0["o"]
        H = P.T @ Q - np.outer(P.sum(axis=0), Q.mean(axis=0))
        sv = np.linalg.svd(H, compute_uv=False)
        # numerical rank against the scale of the moments: what 50 .. 300 rounded products can leave behind is ~1e-14 of it
        scale = np.linalg.norm(P - P.mean(axis=0)) * np.linalg.norm(Q - Q.mean(axis=0))
        rank = int((sv > 1e-10 * max(scale, np.linalg.norm(P) * np.linalg.norm(Q) * 1e-3)).sum())
        print("   singular values of H", sv, "rank", rank)
        assert rank <= c.plan["rank"] and (rank == 2) == (c.plan["rank"] == 2)
        assert c.plan["pose_compared"] == (rank >= 2)
        if not c.plan["pose_compared"]:
            assert rank <= 1 and p["maximum_iterations"] == 1
    if c.plan.get("far"):
        assert np.abs(c.tgt[:, :3]).max() > 2000 and np.abs(c.src[:, :3]).max() > 2000 and p["maximum_iterations"] == 1
        assert np.array_equal(tr[0]["o"], c.tgt[0, :3].astype(np.float64))
    if c.family == "origin":
        fin = np.isfinite(c.tgt[:, :3]).all(axis=1)
        if c.plan["origin"] is None:
            assert not fin.any() and np.all(tr[0]["o"] == 0) and kept == [0] and np.array_equal(r["T"], np.eye(4, dtype=np.float32))
        else:
            i = c.plan["origin"]
            assert fin[i] and not fin[:i].any() and np.array_equal(tr[0]["o"], c.tgt[i, :3].astype(np.float64))
    if c.family == "nonfinite":
        bad = ~np.isfinite(c.src[:, :3]).all(axis=1)
        assert kept[0] == n - int(bad.sum()) and not tr[0]["keep"][bad].any()
        if name == "nonfinite_last_slot":
            assert n == E.SLICE + 1 and bad.sum() == 1
        else:
            assert bad.sum() == 2 * E.RUN
    if "inner" in c.plan:
        assert all(t["inner"] == c.plan["inner"] for t in r["traj"])
    if method == E.GICP and c.family == "caps" and "inner" not in c.plan:
        assert r["iterations"] == max(1, p["maximum_iterations"])
    if method == E.ICP and c.family == "caps":
        assert r["iterations"] == max(1, p["maximum_iterations"]) and r["converged"]


@pytest.mark.parametrize("name,method", E.RUNS)
def test_no_decision_of_a_case_is_marginal(orc, name, method):
    """What lets the GPU tests compare kept counts and iteration counts exactly.  No case is exempt."""
    c = E.case(name)
    p = E.settings(c, method)
    r = E.reference(orc, name, method)
    m2 = float(p["gicp_max_correspondence_distance"]) ** 2
    planted = np.zeros(c.src.shape[0], bool)
    if c.family == "gate":
        planted[list(c.plan["planted"].values())] = True
        assert len(r["trace"]) == 1                                 # planted points decide in a first pass whose working copy is exact
    worst = np.inf
    for t in r["trace"]:
        d2 = t["d2"][~planted].astype(np.float64)
        d2 = d2[np.isfinite(d2)]
        if d2.size:
            worst = min(worst, float(np.abs(d2 / m2 - 1.0).min()))
    print(name, method, "smallest relative distance of an unplanted d2 from the gate:", worst)
    assert worst >= MARGIN
    if method == E.ICP:
        for nudge in (1, -1):
            rn = E.reference(orc, name, method, nudge=nudge)
            assert _kept(rn) == _kept(r) and rn["iterations"] == r["iterations"] and rn["converged"] == r["converged"], nudge
        return
    # GICP: the optimiser under sums taken in another order, the loop's own decision, and the neighbour lists the covariances are made of
    for seed in (1, 2, 3):
        rn = E.reference(orc, name, method, perturb_seed=seed)
        assert _kept(rn) == _kept(r) and rn["iterations"] == r["iterations"] and rn["converged"] == r["converged"], seed
        for a, b in zip(rn["traj"], r["traj"]):
            assert (a["inner"], a["passes"]) == (b["inner"], b["passes"]), (seed, a["inner"], b["inner"], a["passes"], b["passes"])
            assert np.abs(a["T"] - b["T"]).max() <= 1e-6, (seed, np.abs(a["T"] - b["T"]).max())       # a tenth of what the GPU comparison allows
    cap = max(1, p["maximum_iterations"])
    forked = False
    for k, t in enumerate(r["traj"]):
        forked = forked or t["roundoff"]
        if k + 1 < cap:                                              # at the cap the loop ends whatever delta is
            assert abs(t["delta"] - 1.0) > (DELTA_MARGIN if forked else DELTA_MARGIN / 2), (k, t["delta"])
    k = p["gicp_correspondence_randomness"]
    for cloud in (c.tgt, c.src):
        fin = cloud[np.isfinite(cloud[:, :3]).all(axis=1)]
        if fin.shape[0] > k:
            q = np.zeros((fin.shape[0], 4), np.float32)
            q[:, :3] = fin[:, :3]
            _, d = orc.knn(q, q, k + 1)
            assert np.all(d[:, k - 1] < d[:, k])                      # no list ends in a tie: the k nearest are a set, not a choice
    if c.family == "gate":
        assert _nondegenerate(r["sv_tgt"]).all() and _nondegenerate(r["sv_src"]).all()     # usable covariances: the eps direction is defined


@pytest.mark.parametrize("name", [n for n, c in E.CASES.items() if c.plan.get("probe")])
def test_probe_pass_keeps_every_point_clear_of_the_gate(orc, name):
    c = E.case(name)
    T, guess, m, f, g, t = E.probe_reference(orc, name)
    m2 = float(E.settings(c, E.GICP)["gicp_max_correspondence_distance"]) ** 2
    assert m == c.src.shape[0] and np.isfinite(f) and np.all(np.isfinite(g)) and f > 0
    assert float(np.abs(t["d2"].astype(np.float64) / m2 - 1.0).min()) >= MARGIN


@pytest.mark.parametrize("name", [n for n, c in E.CASES.items() if c.plan.get("covariances")])
def test_small_cloud_covariances_are_well_defined(orc, name):
    r = E.reference(orc, name, E.GICP)
    for sv in (r["sv_tgt"], r["sv_src"]):
        ok = _nondegenerate(sv)
        print(name, "nondegenerate", int(ok.sum()), "of", ok.size)
        assert ok.mean() > 0.9


def test_forks_are_recorded_for_every_gicp_case(orc):
    seen = 0
    for name, method in E.RUNS:
        if method == E.GICP:
            f = forks(orc, name)
            assert len(f) == E.reference(orc, name, method)["iterations"]
            seen += any(f)
    # none since the cases run 3 BFGS steps per outer iteration; a case that does fork gets test_pcl_gicp_gpu._compare's rule on the GPU
    print("GICP cases with a line search that ends in roundoff:", seen)


def test_the_det_flip_decides_in_registered_cases(orc):
    """Where H has full rank and det H < 0, det U det V < 0 for every SVD of it (the singular values are positive): without the flip of
    V's last column the fit is a reflection.  The planar pair's ground points give such an H, with a third singular value ~1e-6 of the
    first -- ten orders above rounding -- in the first pass of these cases; the coplanar pair's H has rank 2 exactly, there the signs of
    the two last columns are the SVD routine's choice."""
    hit = []
    for name, method in E.RUNS:
        t0 = E.reference(orc, name, method)["trace"][0] if method == E.ICP else None
        if t0 is None or t0["keep"].sum() < 3:
            continue
        c = E.case(name)
        P = t0["W"][t0["keep"]].astype(np.float64) - t0["o"]
        Q = c.tgt[t0["j"][t0["keep"]], :3].astype(np.float64) - t0["o"]
        H = P.T @ Q - np.outer(P.sum(axis=0), Q.mean(axis=0))
        sv = np.linalg.svd(H, compute_uv=False)
        if np.linalg.det(H) < 0 and sv[2] > 1e-9 * sv[0]:
            hit.append(name)
    print("det H < 0 in the first pass:", hit)
    assert {"size_icp_64", "size_icp_257", "rows_icp_8", "far_frame", "cap_1"} <= set(hit)
