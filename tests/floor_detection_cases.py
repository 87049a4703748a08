"""Scenes and draw lists shared by test_floor_detection_cpu.py (which checks, with the restatement alone, the conditions the GPU tests
rely on) and test_floor_detection_gpu.py (device against restatement).  Every case is a dict(cloud, params, raw, tilt, tilt_inv) whose
restatement result is computed once per process (floor_detection_reference.cached)."""
import numpy as np

import floor_detection_reference as R
from delta_graph_slam_amd import synth

F = np.float32
TILE = 1024                 # points per workgroup of sac_score_kernel (kSacTile)
PREPARE_CHUNK = 1024        # draws per pass of sac_prepare_kernel (kSacPrepareBlock)
CHUNK_FIRST, CHUNK = 64, 512
SENSOR_Z = 1.73             # synth.street_scan's sensor height over the street

# sparse clutter in a 20 m cube with the clip band opened wide: a clutter triple's slab of +-0.1 m holds a few points only, so the walk
# stays open up to max_iterations
OPEN = dict(use_normal_filtering=0, height_clip_range=50.0, floor_pts_thresh=10)


def identity():
    return np.eye(4, dtype=F), np.eye(4, dtype=F)


def case(cloud, params, raw=None, tilt_deg=0.0):
    t, ti = R.tilt_matrices(tilt_deg)
    return dict(cloud=np.ascontiguousarray(cloud, F), params=dict(params, tilt_deg=tilt_deg), raw=raw, tilt=t, tilt_inv=ti)


def reference(key, c):
    return R.cached(key, lambda: R.detect(c["cloud"], c["params"], c["raw"], c["tilt"], c["tilt_inv"]))


# ---- the prefiltered synthetic scans -----------------------------------------------------------------------------------------
def raw_scan(kind):
    if kind == "hdl64":
        xyz, _ = synth.street_scan((0.0, 0.0, 0.0), 64, (2.0, -24.8), 1024, 3)
    else:
        xyz, _ = synth.street_scan((-30.0, 1.0, 0.1), 16, (15.0, -15.0), 1875, 21)
    return synth._xyz1(xyz)


SCAN_PARAMS = dict(sensor_height=SENSOR_Z)


# ---- two planted planes in sparse clutter --------------------------------------------------------------------------------------
def two_planes(n, seed=0, extra_diagonal=0):
    """n points: plane A (z = -2 + 0.01 x) with m points, plane B (z = -4 - 0.02 y) with m + 1 points of which one is the LAST point of the
    cloud, `extra_diagonal` points on the line x = y = z (any three of them are a bad sample), the rest clutter in [-10, 10]^3 farther than
    0.3 m from both planes.  -> (cloud, idx_a, idx_b, idx_clutter, idx_diagonal), index arrays ascending."""
    rng = np.random.default_rng(seed)
    m = int(0.15 * n)
    n_cl = n - (2 * m + 1) - extra_diagonal
    a = np.concatenate([rng.uniform(-10, 10, (m, 2)), np.zeros((m, 1))], 1)
    a[:, 2] = -2.0 + 0.01 * a[:, 0]
    b = np.concatenate([rng.uniform(-10, 10, (m + 1, 2)), np.zeros((m + 1, 1))], 1)
    b[:, 2] = -4.0 - 0.02 * b[:, 1]
    cl = np.zeros((0, 3))
    while cl.shape[0] < n_cl:
        q = rng.uniform(-10, 10, (2 * n_cl + 16, 3))
        ok = (np.abs(q[:, 2] - (-2.0 + 0.01 * q[:, 0])) > 0.3) & (np.abs(q[:, 2] - (-4.0 - 0.02 * q[:, 1])) > 0.3)
        cl = np.concatenate([cl, q[ok]])[:n_cl]
    dg = (np.arange(extra_diagonal)[:, None] * 0.5 + 5.0) * np.ones((1, 3))          # (5, 5, 5), (5.5, 5.5, 5.5), ...: far from both planes
    kind = np.concatenate([np.zeros(m, int), np.ones(m, int), np.full(n_cl, 2), np.full(extra_diagonal, 3)])
    body = np.concatenate([a, b[:m], cl, dg])
    perm = rng.permutation(n - 1)
    pts = np.ones((n, 4), F)
    pts[:n - 1, :3] = body[perm]
    pts[n - 1, :3] = b[m]                                                             # B's lead sits at the last index
    kind = np.concatenate([kind[perm], [1]])
    return pts, np.nonzero(kind == 0)[0], np.nonzero(kind == 1)[0], np.nonzero(kind == 2)[0], np.nonzero(kind == 3)[0]


def _triples(rng, idx, count):
    out = []
    for _ in range(count):
        out.append(tuple(int(v) for v in rng.choice(idx, 3, replace=False)))
    return out


def rank_edge(n, winner_rank, max_iterations=1000, seed=0, chunk_first=None, chunk=None):
    """The winner (plane B, m + 1 inliers, leading only through the last point) at hypothesis `winner_rank`, the runner-up (plane A, m
    inliers) at rank 3, clutter triples everywhere else, for max_iterations + 1 hypotheses."""
    pts, ia, ib, ic, _ = two_planes(n, seed)
    rng = np.random.default_rng(seed + 1000)
    tr = _triples(rng, ic, max_iterations + 1)
    tr[3] = tuple(int(v) for v in ia[:3])
    tr[winner_rank] = tuple(int(v) for v in ib[:3])
    prm = dict(OPEN, max_iterations=max_iterations)
    if chunk_first is not None:
        prm.update(hyp_chunk_first=chunk_first, hyp_chunk=chunk)
    c = case(pts, prm, R.raw_for_triples(n, tr))
    c.update(m=ia.size, winner_rank=winner_rank)
    return c


RANKS = (CHUNK_FIRST - 1, CHUNK_FIRST, CHUNK_FIRST + 1, CHUNK_FIRST + CHUNK - 1, CHUNK_FIRST + CHUNK, CHUNK_FIRST + CHUNK + 1)
SIZES = (TILE - 1, TILE, TILE + 1, 2 * TILE + 1)


def bad_run(length, first_bad=30, max_iterations=40, n=600, seed=5):
    """`first_bad` good clutter draws, `length` bad ones (three points of the diagonal line), then good ones again: a run of
    max_sample_checks - 1 is survived, a run of max_sample_checks ends the walk.  With first_bad = 30 the run straddles the prepare kernel's
    chunk boundary at draw 1024."""
    pts, ia, ib, ic, idg = two_planes(n, seed, extra_diagonal=8)
    rng = np.random.default_rng(seed + 2000)
    tr = _triples(rng, ic, first_bad) + _triples(rng, idg, length) + _triples(rng, ic, max_iterations + 1)
    tr[3] = tuple(int(v) for v in ia[:3])
    assert first_bad < PREPARE_CHUNK < first_bad + length
    return case(pts, dict(OPEN, max_iterations=max_iterations), R.raw_for_triples(n, tr))


def run_behind_the_stop(n=4000, seed=9):
    """A dense floor: the walk closes after a few hypotheses; the draw list goes on with a completed run of 1000 bad draws, inside the
    list the device prepares (max_iterations + 1 + 64 draws), which nobody takes."""
    rng = np.random.default_rng(seed)
    pts = R.floor_scene(n - 208, 200, seed=seed)
    dg = np.ones((8, 4), F)
    dg[:, :3] = (np.arange(8)[:, None] * 0.25 - 2.9) * np.ones((1, 3))               # z in [-2.9, -1.15]: inside the default clip band
    pts = np.concatenate([pts, dg])
    floor = np.nonzero(np.abs(pts[:n - 8, 2] - (-2.0 + 0.03 * pts[:n - 8, 0] - 0.02 * pts[:n - 8, 1])) < 0.03)[0]   # floor_scene's plane
    tr = _triples(rng, floor, 5) + _triples(rng, np.arange(n - 8, n), 1000) + _triples(rng, floor, 40)
    return case(pts, dict(use_normal_filtering=0), R.raw_for_triples(n, tr))


def tilted_plane(angle_deg, n=1500, seed=3, flip=False):
    """An exact plane through (0, 0, -2) tilted by angle_deg about the x axis, in sparse clutter; the first draw is three plane points,
    ordered so that the raw normal points up (or down with flip)."""
    rng = np.random.default_rng(seed)
    m = 900
    uv = rng.uniform(-8, 8, (m, 2))
    a = np.deg2rad(angle_deg)
    plane = np.stack([uv[:, 0], uv[:, 1] * np.cos(a), -2.0 + uv[:, 1] * np.sin(a)], 1)
    cl = rng.uniform(-10, 10, (n - m, 3))
    pts = np.ones((n, 4), F)
    pts[:m, :3] = plane
    pts[m:, :3] = cl
    i0, i1, i2 = 0, 1, 2
    u, v = plane[i1] - plane[i0], plane[i2] - plane[i0]
    if (np.cross(u, v)[2] < 0) != flip:
        i1, i2 = i2, i1
    tr = [(i0, i1, i2)] + _triples(rng, np.arange(m, n), 1100)
    return case(pts, dict(OPEN, floor_pts_thresh=100), R.raw_for_triples(n, tr))


# ---- planted end-to-end scenes -------------------------------------------------------------------------------------------------
def planted(tilt_deg=5.0, normal=False, seed=11, **params):
    """A sloped floor with range noise and clutter in the clip band, given in the sensor frame of a sensor tilted by tilt_deg."""
    pts = R.floor_scene(2600, 700, seed=seed)
    _, ti = R.tilt_matrices(tilt_deg)
    return case(R.transform(pts, ti), dict(params, use_normal_filtering=int(normal)), None, tilt_deg)


def planted_empty_band(tilt_deg=5.0, seed=13):
    """A jittered grid floor (exact slope, no range noise: normals within a degree of the plane's) and a wall a metre beyond its edge
    (horizontal normals): no normal comes near the 20 degree threshold."""
    floor = R.grid_floor(44, 44, spacing=0.25, slope=(0.03, -0.02), jitter=0.05, seed=seed)
    rng = np.random.default_rng(seed)
    wy, wz = np.meshgrid(np.arange(40) * 0.25 - 5.0, np.arange(7) * 0.25 - 2.9, indexing="ij")
    wall = np.ones((wy.size, 4), F)
    wall[:, 0] = 7.0
    wall[:, 1] = wy.ravel() + rng.uniform(-0.05, 0.05, wy.size)
    wall[:, 2] = wz.ravel() + rng.uniform(-0.05, 0.05, wy.size)
    pts = np.concatenate([floor, wall])[rng.permutation(floor.shape[0] + wall.shape[0])]
    _, ti = R.tilt_matrices(tilt_deg)
    return case(R.transform(pts, ti), dict(use_normal_filtering=1), None, tilt_deg)


def quirk_cloud():
    """Upstream's quirk: p2 == p0 and p1 differing in one axis give NaN ratios, so the sample is 'good'; its cross product is zero, the
    model (0, 0, 0, 0) takes every point as an inlier and the verticality check rejects it."""
    pts = R.floor_scene(600, 100, seed=17)
    pts[1] = pts[0]
    pts[1, 0] += F(0.5)
    pts[2] = pts[0]
    return case(pts, dict(use_normal_filtering=0, floor_pts_thresh=100), R.raw_for_triples(700, [(0, 1, 2)] + [(3, 4, 5)] * 4))


def diagonal_cloud(n=64):
    """Every triple is collinear on x = y = z: 1000 bad draws in a row, no model, empty inliers."""
    pts = np.ones((n, 4), F)
    pts[:, :3] = (np.arange(n)[:, None] * F(0.03125) - F(2.9)) * np.ones((1, 3), F)
    return case(pts, dict(use_normal_filtering=0, floor_pts_thresh=10))
