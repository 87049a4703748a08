"""Scenes that put the line extraction (delta_graph_slam_amd/csrc/line_extraction.hip) at the edges of its kernels: the hypothesis chunks
and point tiles of sac_score_kernel<LnModel, 512>, the carry of sac_prepare_kernel<LnModel> across its 1024-draw chunks, the regrowth of the draw list, the
windowed union-find clustering at its tolerance, ln_pick_kernel's choice, the 256-term staging of the refit and the statistics, the
strict emission thresholds and the host loop at its smallest inputs.

Plain numpy with fixed seeds, no GPU.  `rng_raw` stands in for the generator and the draw permutation is invertible, so `raw_for_pairs`
makes draw d come out as any wanted pair: a scene decides which hypothesis sits at which rank, which draws are bad and which sample
wins.  tests/test_line_extraction_edge_cases_cpu.py proves on the restatement what each case claims (`plan`),
tests/test_line_extraction_edges_gpu.py runs the cases on the device against tests/line_extraction_reference.py.
"""
from __future__ import annotations

from typing import NamedTuple, Optional

import numpy as np

import line_extraction_reference as R

F = np.float32
TILE, CHUNK, PREPARE, BLOCK = 1024, 512, 1024, 256     # kSacTile, kLnHypChunk, kSacPrepareBlock, kBlock of sac.h / line_extraction.hip
BAD_RUN, SLACK = 1000, 64                              # kLnBadRun, kLnDrawSlack


class Case(NamedTuple):
    cloud: np.ndarray
    params: dict
    raw: Optional[np.ndarray]
    aims: str            # the kernel line the case aims at
    plan: dict           # what the restatement's record must show for the case to hit its edge (checked on the CPU)


def raw_for_pairs(n, pairs):
    """The uint32 rng_raw that makes draw d of R.draw_stream(n, raw) come out as pairs[d] (i0 != i1).  The permutation and the position
    of every index are tracked: a is the position of i0; after the first swap b is the position of i1, which is >= 1; (a, b - 1) is
    emitted, and a % n = a, 1 + (b - 1) % (n - 1) = b."""
    s, pos = list(range(n)), list(range(n))
    out = np.empty(2 * len(pairs), np.uint32)

    def swap(i, j):
        s[i], s[j] = s[j], s[i]
        pos[s[i]], pos[s[j]] = i, j

    for d, (i0, i1) in enumerate(pairs):
        i0, i1 = int(i0), int(i1)
        assert i0 != i1 and 0 <= i0 < n and 0 <= i1 < n
        a = pos[i0]
        swap(0, a)
        b = pos[i1]
        assert b >= 1
        swap(1, b)
        out[2 * d], out[2 * d + 1] = a, b - 1
    return out


def with_tail(raw, seed, draws=300):
    """`raw` followed by `draws` arbitrary draws: the later iterations and rounds of a case whose first draws are pinned."""
    tail = np.random.default_rng(seed).integers(0, 2**31, 2 * draws, dtype=np.uint32)
    return np.concatenate([np.asarray(raw, np.uint32), tail])


def cloud_of(xy):
    xy = np.asarray(xy, np.float64).reshape(-1, 2)
    c = np.zeros((xy.shape[0], 4), F)
    c[:, :2] = xy
    c[:, 3] = 1
    return c


def shuffled(xy, seed, first=None):
    """-> (cloud, where): the points in a shuffled index order, where[j] the index of xy[j]; xy[first] goes to index 0."""
    xy = np.asarray(xy, np.float64).reshape(-1, 2)
    n = xy.shape[0]
    where = np.random.default_rng(seed).permutation(n)
    if first is not None:
        j = int(np.nonzero(where == 0)[0][0])
        where[j], where[first] = where[first], 0
    c = np.zeros((n, 2))
    c[where] = xy
    return cloud_of(c), where


def on_line(t, origin=(0.0, 0.0), direction=(1.0, 0.0)):
    t = np.asarray(t, np.float64)
    return np.stack([origin[0] + t * direction[0], origin[1] + t * direction[1]], 1)


DIAG = (0.8, 0.6)
DEG30 = (float(np.cos(np.pi / 6)), 0.5)

# ==================================================================================================== chunks and tiles of sac_score_kernel
# Sparse clutter, uniform in +-40 m: with the threshold 0.1 a clutter hypothesis counts a handful of points, so k stays in the thousands
# and the walk runs to max_iterations + 1.  Two planted lines hold every other count: the runner-up, 30 points on y = 10, at a low
# rank, and the winner, 31 points on x = 15, at the rank the case names.  No clutter point lies within 0.5 of either (infinite) line, so
# the two counts are exactly 30 and 31.
N_WIN, N_RUN = 31, 30


def _sparse_scene(n, seed, win_idx, run_idx):
    rng = np.random.default_rng(seed)
    xy = np.zeros((n, 2))
    m = 0
    while m < n:
        p = rng.uniform(-40, 40, (n, 2))
        p = p[(np.abs(p[:, 1] - 10.0) > 0.5) & (np.abs(p[:, 0] - 15.0) > 0.5)][:n - m]
        xy[m:m + p.shape[0]] = p
        m += p.shape[0]
    xy[win_idx] = on_line(-20.0 + 0.2 * np.arange(N_WIN), (15.0, 0.0), (0.0, 1.0))
    xy[run_idx] = on_line(-30.0 + 0.2 * np.arange(N_RUN), (0.0, 10.0), (1.0, 0.0))
    return cloud_of(xy)


def _winner_case(n, seed, win_rank, run_rank, max_iterations, late, aims):
    """n points; the winner's last `late` points take the last `late` indices, everything else planted lies below n - late."""
    rng = np.random.default_rng(seed)
    low = rng.permutation(n - late)[:N_WIN - late + N_RUN]
    win_idx = np.concatenate([np.sort(low[:N_WIN - late]), np.arange(n - late, n)]).astype(np.int64)
    run_idx = np.sort(low[N_WIN - late:])
    cloud = _sparse_scene(n, seed + 1, win_idx, run_idx)
    free = np.setdiff1d(np.arange(n), np.concatenate([win_idx, run_idx]))
    pairs = []
    for d in range(max_iterations + 1):
        i0, i1 = rng.choice(free, 2, replace=False)
        pairs.append((int(i0), int(i1)))
    pairs[win_rank] = (int(win_idx[0]), int(win_idx[-1]))
    pairs[run_rank] = (int(run_idx[0]), int(run_idx[-1]))
    plan = dict(winner_rank=win_rank, runner=pairs[run_rank], runner_rank=run_rank, iterations=max_iterations + 1, draws=max_iterations + 1,
                inliers=N_WIN, cluster=N_WIN, emitted=1, sample=pairs[win_rank], relaunches=0)
    if late:
        plan.update(late=late, late_from=n - late)
    return Case(cloud, dict(max_iterations=max_iterations, max_rounds=2), with_tail(raw_for_pairs(n, pairs), seed + 2, 8), aims, plan)


def _chunk_rank(rank):
    return _winner_case(700, 1000 + rank, rank, 3, 600 if rank < 600 else 1200, 0,
                        f"ln_round's sac_score_kernel<LnModel, 512>: the winner's count is s_cnt[{rank} - h0] of hypothesis chunk blockIdx.y = {rank // CHUNK}, and the walk reads "
                        f"counts[] up to max_iterations.")


def _tile_tail(n):
    late = 1 if n > TILE else 2
    return _winner_case(n, 2000 + n, 5, 2, 40, late,
                        f"ln_round's sac_score_kernel<LnModel, 512>: the winner leads the runner-up only through the last {late} point(s) of the cloud, which sit in the "
                        f"{'partial ' if n % TILE else ''}last tile (blockIdx.x = {(n - 1) // TILE}, ok[k] = i < n).")


# ==================================================================================================== draw list: sac_prepare_kernel, regrowth
# One point repeated 30 times, eight points in general position and three collinear ones: a draw is bad exactly when both of its
# indices are copies of the repeated point.  A pair of general points counts 2, the collinear pair 3.
def _dup_scene(seed):
    rng = np.random.default_rng(seed)
    general = np.array([[-9.0, 4.0], [-6.5, -7.25], [-2.0, 8.5], [3.25, -5.0], [6.0, 6.75], [8.5, -1.5], [11.0, 3.0], [-4.0, -0.75]])
    line = np.array([[-3.0, 12.0], [-2.25, 12.0], [-1.5, 12.0]])
    xy = np.concatenate([np.tile([[1.5, -2.0]], (30, 1)), general, line])
    cloud, where = shuffled(xy, seed)
    return cloud, where[:30], where[30:38], where[38:], rng


def _draw_case(seed, kinds, line_at, params, aims, plan):
    """kinds[d]: True for a good draw, False for a bad one; the collinear pair sits at draw `line_at`."""
    cloud, dup, general, line, rng = _dup_scene(seed)
    pairs = []
    for d, good in enumerate(kinds):
        i0, i1 = rng.choice(general if good else dup, 2, replace=False)
        pairs.append((int(i0), int(i1)))
    if line_at is not None:
        assert kinds[line_at]
        pairs[line_at] = (int(line[0]), int(line[2]))
        plan = dict(plan, sample=pairs[line_at])
    prm = dict(dict(sac_distance_threshold=0.01, min_cluster_size=2, max_rounds=1), **params)
    return Case(cloud, prm, raw_for_pairs(cloud.shape[0], pairs), aims, plan)


def _bad_run(length):
    kinds = [True] * 501 + [False] * length + [True] * (1600 - 501 - length)
    aims = ("ln_round's sac_prepare_kernel<LnModel>: a bad run that starts after 501 good draws and straddles draw 1024 -- s_last carries the last good draw "
            f"across the chunk edge, and d - last == {BAD_RUN} ")
    if length == BAD_RUN - 1:
        return _draw_case(31, kinds, 1505, dict(max_iterations=520), aims + "is never true: the round goes on and the winner is drawn behind the run.",
                          dict(winner_rank=506, iterations=521, draws=1520, bad_draws=999, inliers=3, cluster=3, emitted=1, relaunches=1,
                               status="MAX_ROUNDS"))
    return _draw_case(31, kinds, None, dict(max_iterations=520), aims + "holds at draw 1500: ln_walk_kernel meets hyps[501].draw > fail_at.",
                      dict(status="RANSAC_FAILED", iterations=501, draws=1501, bad_draws=1000, relaunches=1, sample=(-1, -1)))


def _bad_run_behind_the_stop():
    rng = np.random.default_rng(41)
    xy = np.concatenate([np.tile([[1.5, -2.0]], (20, 1)), on_line(0.2 * np.arange(60), (0.0, 3.0)),
                         [[-9.0, 4.0], [-6.5, -7.25], [-2.0, 8.5], [3.25, -5.0], [8.5, -11.5]]])
    cloud, where = shuffled(xy, 41)
    dup, line, general = where[:20], where[20:80], where[80:]
    kinds = [True] * 10 + [False] * BAD_RUN + [True] * 290
    pairs = [tuple(int(v) for v in rng.choice(general if g else dup, 2, replace=False)) for g in kinds]
    pairs[0] = (int(line[0]), int(line[59]))
    return Case(cloud, dict(max_iterations=1200, min_cluster_size=10, max_rounds=1), raw_for_pairs(85, pairs),
                "ln_walk_kernel: 60 of 85 inliers stop the walk after 7 iterations; fail_at = 1009 lies inside the first list but "
                "hyps[it].draw > fail_at is never true.",
                dict(winner_rank=0, iterations=7, draws=7, bad_draws=0, inliers=60, cluster=60, emitted=1, relaunches=0, status="MAX_ROUNDS",
                     sample=pairs[0]))


def _regrow_twice():
    kinds = [d % 40 == 0 and d <= 400 for d in range(500)]
    return _draw_case(51, kinds, 320, dict(max_iterations=10),
                      "ln_extract: eleven good draws 40 apart -- the lists of 75 and 300 draws end in LN_NEED_DRAWS, the third (D * 4, cut to "
                      "the caller's 500) holds the winner at draw 320.",
                      dict(winner_rank=8, iterations=11, draws=401, bad_draws=390, inliers=3, cluster=3, emitted=1, relaunches=2, status="MAX_ROUNDS"))


def _regrow_to_cap():
    kinds = [d in (500, 1400) for d in range(3100)]
    return _draw_case(52, kinds, 1400, dict(max_iterations=1),
                      "ln_extract: good draws at 500 and 1400 with max_iterations = 1 -- lists of 66, 264 and 1056 draws run out, the fourth is "
                      "cut by the cap max_hyp * 1000 + 1000 = 3000.",
                      dict(winner_rank=1, iterations=2, draws=1401, bad_draws=1399, inliers=3, cluster=3, emitted=1, relaunches=3, status="MAX_ROUNDS"))


# ==================================================================================================== clustering
def _pinned(xy, seed, s0, s1, params, aims, plan, first=None, tail=300):
    """The points shuffled, draw 0 pinned to the sample (xy[s0], xy[s1]); arbitrary draws follow."""
    cloud, where = shuffled(xy, seed, first)
    sample = (int(where[s0]), int(where[s1]))
    raw = with_tail(raw_for_pairs(cloud.shape[0], [sample]), seed + 1, tail)
    return Case(cloud, params, raw, aims, dict(dict(winner_rank=0, sample=sample, relaunches=0), **plan))


def _chain_exact(inclusive):
    xy = on_line(0.5 * np.arange(40))
    plan = dict(inliers=40, cluster=40, emitted=1, components=[40]) if inclusive else dict(inliers=40, cluster=1, emitted=0, components=[1] * 40)
    return _pinned(xy, 61, 0, 39, dict(cluster_tolerance=0.5, cluster_inclusive=inclusive, min_cluster_size=5, max_iterations=20, max_rounds=3),
                   "ln_link_kernel: every neighbour pair has d2 == tol2 exactly (0.25): `inclusive ? d2 <= tol2 : d2 < tol2`.", plan)


def _chain_diagonal(inclusive):
    xy = on_line(0.5 * np.arange(40), (1.0, -2.0), DEG30)
    return _pinned(xy, 62, 0, 39, dict(cluster_tolerance=0.5, cluster_inclusive=inclusive, min_cluster_size=5, max_iterations=20, max_rounds=3),
                   "ln_link_kernel: neighbours 0.5 apart on a 30 degree line -- the rounding of sqdist_rn decides every link against tol2.",
                   dict(inliers=40))


def _chain_1025():
    xy = np.concatenate([on_line(0.3 * np.arange(1025), (-150.0, -100.0), DIAG), [[0.0, 30.0], [5.0, -40.0], [-20.0, 25.0], [40.0, 45.0], [60.0, -60.0]]])
    return _pinned(xy, 63, 0, 1024, dict(cluster_tolerance=0.5, max_iterations=20, max_rounds=2),
                   "ln_link_kernel / ln_find: one chain of 1025 inliers over five 256-lane workgroups, every link a CAS on a root of another "
                   "workgroup; ln_refit_kernel and ln_stats_kernel stage 4 x 256 + 1 terms.",
                   dict(inliers=1025, cluster=1025, emitted=1, components=[1025]))


def _stacks():
    t = np.concatenate([np.zeros(300), [1, 2, 3, 4], np.full(300, 5.0), [6, 7, 8.5, 9.5], np.full(300, 10.0)])
    return _pinned(on_line(t, (2.0, 1.0), DIAG), 64, 0, 907, dict(cluster_tolerance=1.1, max_iterations=20, max_rounds=1),
                   "ln_link_kernel: three stacks of 300 identical points (all pairs link, every CAS contended), joined by single points but for "
                   "one gap of 1.5.",
                   dict(inliers=908, cluster=606, emitted=1, components=[606, 302]))


def _rails(name):
    stagger, tol = (0.0, 0.17) if name == "rails_aligned" else (0.075, 0.2 if name == "rails_joined" else 0.17)
    xa, xb = 0.15 * np.arange(40), stagger + 0.15 * np.arange(41)
    xy = np.concatenate([[[-5.0, 0.0], [20.0, 0.0]], np.stack([xa, np.full(40, 0.09)], 1), np.stack([xb, np.full(41, -0.09)], 1)])
    comps = [81, 1, 1] if name == "rails_joined" else [41, 40, 1, 1]
    what = {"rails": "staggered rows 0.195 apart, 0.15 within a row, tolerance 0.17: the window holds points of the other row that must not link",
            "rails_aligned": "two rows with equal projections 0.18 apart, tolerance 0.17: equal sproj, d2 > tol2",
            "rails_joined": "staggered rows 0.195 apart, tolerance 0.2: the rows join"}[name]
    return _pinned(xy, 65, 0, 1, dict(cluster_tolerance=tol, min_cluster_size=10, max_iterations=20, max_rounds=3),
                   "ln_link_kernel: " + what + ".", dict(inliers=83, cluster=comps[0], emitted=1, components=comps))


def _tol_zero(inclusive):
    t = np.concatenate([0.25 * np.arange(20), np.full(4, 1.0), np.full(2, 3.0), np.full(4, 2.5)])      # 5 points at 1.0 and at 2.5, 3 at 3.0
    comps = [5, 5, 3] + [1] * 17 if inclusive else [1] * 30
    return _pinned(on_line(t), 66, 0, 19, dict(cluster_tolerance=0.0, cluster_inclusive=inclusive, min_cluster_size=2, max_iterations=20, max_rounds=3),
                   "ln_link_kernel: tol = 0 -- the window is the rounding margin alone, tol2 = 0 links duplicates only under `<=`; "
                   "ln_pick_kernel: two stacks of 5.",
                   dict(inliers=30, cluster=5 if inclusive else 1, emitted=0, components=comps), first=27 if inclusive else None)


def _tol_huge():
    cloud = R.scene(300, segments=2, seed=67)
    return Case(cloud, dict(cluster_tolerance=1e4, max_iterations=50, max_rounds=3), None,
                "ln_link_kernel: a tolerance larger than the cloud -- the window never breaks, every lane walks all later inliers.",
                dict(relaunches=0, one_component=True))


def _far_from_origin():
    cloud = R.scene(257, segments=2, seed=257)
    cloud[:, 0] += F(100.0)
    cloud[:, 1] -= F(80.0)
    return Case(cloud, dict(max_iterations=100, max_rounds=3), None,
                "ln_key_kernel / ln_link_kernel: projections around 100 m, where the float projections are coarse and the window's "
                "2e-5 * max|t| term is what covers them.", dict(relaunches=0))


def _oversized_and_allowed():
    t = np.concatenate([0.1 * np.arange(60), 20.0 + 0.1 * np.arange(20)])
    return _pinned(on_line(t, (-3.0, 4.0), DIAG), 68, 0, 79, dict(max_cluster_size=40, min_cluster_size=10, max_iterations=20, max_rounds=3),
                   "ln_pick_kernel: `sz > max_cluster` skips the component of 60, the one of 20 next to it is taken.",
                   dict(inliers=80, cluster=20, emitted=1, components=[60, 20]))


def _three_way_tie():
    t = np.concatenate([0.1 * np.arange(20), 10.0 + 0.1 * np.arange(20), 20.0 + 0.1 * np.arange(20)])
    return _pinned(on_line(t, (-3.0, 4.0), DIAG), 69, 0, 59, dict(min_cluster_size=10, max_iterations=20, max_rounds=3),
                   "ln_pick_kernel: three components of 20, the key's low word INT_MAX - cminpos decides -- index 0 is in the middle one.",
                   dict(inliers=60, cluster=20, emitted=1, components=[20, 20, 20], cluster_holds=0, cluster_t=(10.0, 11.9)), first=27)


# ==================================================================================================== staging, refit, thresholds
def _members(m):
    rng = np.random.default_rng(70 + m)
    xy = on_line(0.05 * np.arange(m), (-4.0, 2.0), DIAG)
    off = rng.uniform(-0.02, 0.02, m)
    off[[0, m - 1]] = 0.0                                   # the sample lies on the line
    xy += np.stack([-DIAG[1] * off, DIAG[0] * off], 1)
    xy = np.concatenate([xy, [[30.0, -20.0], [-25.0, 18.0], [12.0, 33.0], [-31.0, -7.0], [2.0, -29.0]]])
    return _pinned(xy, 70 + m, 0, m - 1, dict(max_iterations=20, max_rounds=2),
                   f"ln_refit_kernel / ln_stats_kernel: {m} members -- `e = min(kBlock, m - base)` at {m % BLOCK or BLOCK} terms in the last stage "
                   f"of {-(-m // BLOCK)}.", dict(inliers=m, cluster=m, emitted=1, components=[m]))


def _inliers(m):
    rng = np.random.default_rng(80 + m)
    xy = rng.uniform(-20, 20, (30, 2))
    xy[0], xy[1] = (1.0, 2.0), (1.5, 2.25)
    if m == 3:
        xy[2] = (1.25, 2.125)                               # the midpoint, exact in float
    return _pinned(xy, 80 + m, 0, 1, dict(sac_distance_threshold=1e-3, min_cluster_size=2, line_length_threshold=0.25, max_iterations=20, max_rounds=2),
                   f"ln_refit_kernel: m = {m} -- " + ("`m > 2` is false, the sample's model is kept." if m == 2 else "the smallest refit."),
                   dict(inliers=m, cluster=m, emitted=1, components=[m]))


def _threshold(name):
    if name == "mean_equals_threshold":
        xy, prm = on_line(0.25 * np.arange(40)), dict(merror_threshold=0.0)
        aims, plan = "ln_stats_kernel: `mean < merror` with mean == merror == 0.", dict(emitted=0, mean=0.0)
    else:
        xy = on_line(np.arange(33) / 16.0)
        thr = 2.0 if name == "length_equals_threshold" else float(np.nextafter(F(2), F(0)))
        prm = dict(line_length_threshold=thr)
        aims = "ln_stats_kernel: `len > min_length` with len == 2" + (" == min_length." if thr == 2.0 else " and min_length one float below.")
        plan = dict(emitted=int(thr != 2.0), length=2.0)
    n = xy.shape[0]
    return _pinned(xy, 90, 0, n - 1, dict(prm, max_iterations=20, max_rounds=2), aims, dict(plan, inliers=n, cluster=n, components=[n]))


# ==================================================================================================== host loop
def _host(name):
    if name == "max_rounds_0":
        cloud, prm = R.size_scene(64, 100)
        return Case(cloud, dict(prm, max_rounds=0), None, "ln_extract: max_rounds = 0 ends before the first round.", dict(status="MAX_ROUNDS", rounds=0))
    if name == "n0":
        return Case(np.zeros((0, 4), F), dict(max_iterations=20), None, "ln_extract: n = 0, nothing is reserved or launched.", dict(status="DONE", rounds=0))
    if name == "n1_min1":
        return Case(cloud_of([[1.0, 2.0]]), dict(min_cluster_size=1, max_iterations=20), None, "ln_extract: `n < 2` -- a record and RANSAC_FAILED.",
                    dict(status="RANSAC_FAILED", rounds=1, sample=(-1, -1), draws=0, iterations=0, launched=0))
    if name == "n2_min2":
        return Case(cloud_of([[1.0, 2.0], [1.5, 2.0]]), dict(min_cluster_size=2, line_length_threshold=0.25, max_iterations=20), None,
                    "sac_draws<2>: n = 2, `1 + raw % (n - 1)` has one choice; ln_refit_kernel keeps the sample's model.",
                    dict(status="DONE", rounds=1, inliers=2, cluster=2, emitted=1, relaunches=0))
    xy = np.concatenate([on_line(0.2 * np.arange(25), (1.0, -3.0), DIAG), [[30.0, -20.0], [-25.0, 18.0], [12.0, 33.0], [-31.0, -7.0], [2.0, -29.0]]])
    return _pinned(xy, 95, 0, 24, dict(max_iterations=20, max_rounds=2), "ln_stats_kernel: `c < min_cluster` with c == min_cluster_size == 25.",
                   dict(inliers=25, cluster=25, emitted=1, components=[25], status="DONE"))


_BUILDERS = {}
for _r in (511, 512, 513, 1023, 1024, 1100):
    _BUILDERS[f"chunk_rank_{_r}"] = (_chunk_rank, _r)
for _n in (1023, 1024, 1025, 2049):
    _BUILDERS[f"tile_tail_{_n}"] = (_tile_tail, _n)
_BUILDERS["chunk_and_tile"] = (lambda _: _winner_case(2049, 3000, 600, 3, 700, 1,
                                                      "ln_round's sac_score_kernel<LnModel, 512>: grid (3, 2) -- the winner at rank 600 (blockIdx.y = 1) leads through index 2048 "
                                                      "(blockIdx.x = 2)."), None)
_BUILDERS["bad_run_999_over_1024"] = (_bad_run, BAD_RUN - 1)
_BUILDERS["bad_run_1000_over_1024"] = (_bad_run, BAD_RUN)
_BUILDERS["bad_run_behind_the_stop"] = (lambda _: _bad_run_behind_the_stop(), None)
_BUILDERS["regrow_twice"] = (lambda _: _regrow_twice(), None)
_BUILDERS["regrow_to_cap"] = (lambda _: _regrow_to_cap(), None)
_BUILDERS["chain_exact_tol_incl"] = (_chain_exact, 1)
_BUILDERS["chain_exact_tol_excl"] = (_chain_exact, 0)
_BUILDERS["chain_diagonal_tol"] = (_chain_diagonal, 1)
_BUILDERS["chain_diagonal_tol_excl"] = (_chain_diagonal, 0)
_BUILDERS["chain_1025"] = (lambda _: _chain_1025(), None)
_BUILDERS["stacks"] = (lambda _: _stacks(), None)
for _k in ("rails", "rails_aligned", "rails_joined"):
    _BUILDERS[_k] = (_rails, _k)
_BUILDERS["tol_zero_incl"] = (_tol_zero, 1)
_BUILDERS["tol_zero_excl"] = (_tol_zero, 0)
_BUILDERS["tol_huge"] = (lambda _: _tol_huge(), None)
_BUILDERS["far_from_origin"] = (lambda _: _far_from_origin(), None)
_BUILDERS["oversized_and_allowed"] = (lambda _: _oversized_and_allowed(), None)
_BUILDERS["three_way_tie"] = (lambda _: _three_way_tie(), None)
for _m in (255, 256, 257, 513):
    _BUILDERS[f"members_{_m}"] = (_members, _m)
_BUILDERS["inliers_2"] = (_inliers, 2)
_BUILDERS["inliers_3"] = (_inliers, 3)
for _k in ("mean_equals_threshold", "length_equals_threshold", "length_above"):
    _BUILDERS[_k] = (_threshold, _k)
for _k in ("max_rounds_0", "n0", "n1_min1", "n2_min2", "cluster_equals_min"):
    _BUILDERS[_k] = (_host, _k)

NAMES = tuple(_BUILDERS)
EQUALITY_CASES = ("mean_equals_threshold", "length_equals_threshold")
_CASES = {}


def case(name) -> Case:
    if name not in _CASES:
        f, arg = _BUILDERS[name]
        _CASES[name] = f(arg)
    return _CASES[name]


def cases():
    """name -> Case(cloud, params, raw, aims, plan)."""
    return {name: case(name) for name in NAMES}


def reference(name, trig="f32"):
    """The restatement's result for a case, computed once and shared (read-only)."""
    c = case(name)
    return R.cached("edge_" + name, c.cloud, c.params, c.raw, trig)
