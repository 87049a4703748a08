"""Inputs that put the prefilter chain (delta_graph_slam_amd/csrc/prefilter.hip) at the edges of its kernels: the stable compaction at
wave / workgroup / scan-chunk boundaries and across the scan's carry, the plain predicates at their thresholds, the k-NN passes on
clouds with equal distances, lists at their shortest and longest, and a box that overflows the voxel index.

Plain numpy with fixed seeds, no GPU.  tests/test_prefilter_edge_cases_cpu.py proves on the CPU what each generator claims,
tests/test_prefilter_edges_gpu.py runs the cases on the device against tests/prefilter_reference.py.

Every cloud is float32 [n, 4]; the pad lane w carries the point's own index, so a compaction that moves, drops or duplicates a point shows
as a wrong w and not only as a wrong count.
"""
from __future__ import annotations

import numpy as np

import prefilter_reference as R

F = np.float32
WAVE, BLOCK, CHUNK = 64, 256, 1024            # kWave, kBlock of common.h, kCompactScanBlock of compact.h
EDGE = CHUNK * BLOCK                          # 262,144 points: the first point of the scan's second chunk


def index_lane(n: int) -> np.ndarray:
    """The point's index in the pad lane: as a float (exact below 2^24), as its bit pattern beyond."""
    i = np.arange(n)
    return i.astype(F) if n <= (1 << 24) else i.astype(np.uint32).view(F)


def with_index(xyz) -> np.ndarray:
    xyz = np.asarray(xyz)
    out = np.empty((xyz.shape[0], 4), F)
    out[:, :3] = xyz
    out[:, 3] = index_lane(xyz.shape[0])
    return out


# ==================================================================================================== compaction masks
# Driven through the distance filter with its default thresholds (near 1, far 100): a point at norm 10 is kept, one at norm 200 is not.
KEEP_NORM, DROP_NORM = 10.0, 200.0
SMALL_SIZES = (1, 63, 64, 65, 255, 256, 257)                       # the wave and the workgroup
# 1023 * 256 + 255 == 1024 * 256 - 1: the last point of chunk 0; then the first point of chunk 1, one workgroup and one point into it,
# the first point of chunk 2, and three chunks and a ragged workgroup
LARGE_SIZES = (EDGE - 1, EDGE, EDGE + 1, EDGE + 257, 2 * EDGE + 1, 3 * EDGE + 321)


def _random(density, seed):
    return lambda n: np.random.default_rng(seed + n).random(n) < density


def _range(lo, hi):
    def f(n):
        m = np.zeros(n, bool)
        m[lo:hi] = True
        return m
    return f


def _only(pos):
    def f(n):
        m = np.zeros(n, bool)
        m[pos] = True
        return m
    return f


MASKS = {
    "all": lambda n: np.ones(n, bool),
    "none": lambda n: np.zeros(n, bool),
    "first": _only(0),
    "last": _only(-1),
    "last_lane_of_every_wave": lambda n: np.arange(n) % WAVE == WAVE - 1,
    "first_lane_of_every_workgroup": lambda n: np.arange(n) % BLOCK == 0,
    "alternating": lambda n: np.arange(n) % 2 == 1,
    "random_1": _random(0.01, 11),
    "random_50": _random(0.50, 12),
    "random_99": _random(0.99, 13),
    # the scan's carry must move a non-zero total across the chunk edge: the last workgroup of chunk 0 and the first of chunk 1
    "workgroups_1023_1024": _range((CHUNK - 1) * BLOCK, (CHUNK + 1) * BLOCK),
    "chunk0_empty_chunk1_full": _range(EDGE, 2 * EDGE),
    "chunk0_full_chunk1_empty": _range(0, EDGE),
}
EVERY_SIZE_MASKS = ("all", "none", "random_50")


def mask_case_ids():
    """(n, mask name): every mask at the sizes around the chunk edge and above, three masks at every small size."""
    out = [(n, m) for n in SMALL_SIZES for m in EVERY_SIZE_MASKS]
    out += [(n, m) for n in LARGE_SIZES for m in MASKS]
    return out


def mask_case(n: int, name: str):
    """-> (cloud, mask): the distance filter with the default thresholds keeps exactly cloud[mask]."""
    mask = MASKS[name](n)
    xyz = np.zeros((n, 3), F)
    xyz[:, 0] = np.where(mask, F(KEEP_NORM), F(DROP_NORM))
    return with_index(xyz), mask


def first_difference(got, want) -> str:
    """Where two compacted clouds part: for the failure message of a mask case."""
    if got.shape != want.shape:
        m = min(got.shape[0], want.shape[0])
        d = np.nonzero(np.any(got[:m].view(np.uint32) != want[:m].view(np.uint32), 1))[0]
        return f"{got.shape[0]} points for {want.shape[0]}, first differing output index {int(d[0]) if d.size else m}"
    d = np.nonzero(np.any(got.view(np.uint32) != want.view(np.uint32), 1))[0]
    return "equal" if d.size == 0 else f"first differing output index {int(d[0])}: w {got[d[0], 3]!r} for {want[d[0], 3]!r}"


# ==================================================================================================== predicate thresholds
THRESHOLD_PAIRS = ((1.0, 100.0), (0.1, 100.0), (0.0, 3.4e38))
MIN_FOUND = 32
NAN_PAYLOADS = (0x7fc12345, 0xffc00001, 0x7f812345)   # quiet, negative quiet, signalling: the pad lane travels bit for bit


def f32_norm(xyz):
    """The distance filter's norm: sqrt((x*x + y*y) + z*z) in float32, no FMA."""
    x, y, z = (np.asarray(xyz, F)[:, a] for a in range(3))
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        return np.sqrt((x * x + y * y) + z * z)


def other_norms(xyz):
    """-> (the norm with the sum of squares fused as fma(z, z, fma(y, y, x*x)), the norm from the float64 sum), both rounded to float32.
    A float32 product is exact in float64, so each fused step is one float64 addition rounded to float32 (double rounding is possible
    and harmless: the result is only used to pick points at which the fused and the unfused sums part)."""
    x, y, z = (np.asarray(xyz, F)[:, a].astype(np.float64) for a in range(3))
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        fused = (z * z + (y * y + (x * x).astype(F).astype(np.float64)).astype(F).astype(np.float64)).astype(F)
        return np.sqrt(fused), np.sqrt((x * x + y * y) + z * z).astype(F)


def _sphere(t, count, seed):
    """count float32 points at norm t up to rounding, in random directions."""
    rng = np.random.default_rng(seed)
    v = rng.normal(size=(count, 3))
    v /= np.linalg.norm(v, axis=1)[:, None]
    return (v * float(t)).astype(F)


def threshold_points(t, seed=5, count=16384):
    """Points around the norm t = float32(threshold), found by search among `count` random directions -> dict of [m, 3] arrays:
    exact / below / above: the float32 norm is t, the float below it, the float above it;
    parts: the unfused float32 norm differs from the fused one or from the float64 one;
    flips: of those, the ones where that difference changes the side of t the norm falls on."""
    t = F(t)
    c = _sphere(t, count, seed)
    d = f32_norm(c)
    fused, dbl = other_norms(c)
    lo, hi = np.nextafter(t, F(-np.inf)), np.nextafter(t, F(np.inf))
    parts = (d != fused) | (d != dbl)
    flips = parts & (((d > t) != (dbl > t)) | ((d < t) != (dbl < t)) | ((d > t) != (fused > t)) | ((d < t) != (fused < t)))
    return dict(exact=c[d == t], below=c[d == lo], above=c[d == hi], parts=c[parts][:512], flips=c[flips][:512])


def _axis_points(t):
    """+-t on each axis, one ulp either side, and 3-4-5 style points whose sum of squares is exact when t / 5 has few bits."""
    t = F(t)
    out = []
    for v in (t, np.nextafter(t, F(-np.inf)), np.nextafter(t, F(np.inf))):
        for a in range(3):
            for s in (1, -1):
                p = np.zeros(3, F)
                p[a] = s * v
                out.append(p)
        u = F(v / F(5))
        out += [np.array([3 * u, 4 * u, 0], F), np.array([0, -4 * u, 3 * u], F), np.array([4 * u, 0, -3 * u], F)]
    return np.asarray(out, F)


def special_points():
    """Overflowing squares, subnormals, zeros and non-finite coordinates -> [m, 3]."""
    out = [[0, 0, 0], [-0.0, -0.0, -0.0], [0.0, -0.0, 0.0]]
    for a in range(3):
        for v in (2e19, -2e19,              # the square overflows: d = inf, dropped whatever far is
                  1.8e19,                   # the square is 3.24e38: finite, below 3.4e38
                  1e-40, -1e-40,            # subnormal coordinate: the square underflows to 0, d = 0
                  1e-23,                    # normal coordinate, the square underflows to 0
                  1e-20,                    # normal coordinate, subnormal square, d = 1e-20 > 0
                  1.1754944e-38,            # FLT_MIN
                  np.nan, np.inf, -np.inf):
            p = [0.0, 0.0, 0.0]
            p[a] = v
            out.append(p)
            if not np.isfinite(v):          # a non-finite coordinate beside a point that would be kept
                q = [6.0, 6.0, 6.0]
                q[a] = v
                out.append(q)
    return np.asarray(out, F)


def threshold_cloud(near, far):
    """-> (cloud, found): the points of one (near, far) pair; found[threshold][kind] counts what the searches gave."""
    parts, found = [special_points()], {}
    for t in (near, far):
        if not 0 < t < 1e19:                             # no sphere of norm 0, none whose squares overflow
            continue
        tp = threshold_points(t)
        found[t] = {k: int(v.shape[0]) for k, v in tp.items()}
        parts += [_axis_points(t), tp["exact"][:64], tp["below"][:64], tp["above"][:64], tp["parts"], tp["flips"]]
    xyz = np.concatenate(parts)
    cloud = with_index(xyz)
    nan_w = np.full((len(NAN_PAYLOADS), 4), 6.0, F)      # NaN in w only: kept at every pair, w bit for bit
    nan_w[:, 3] = np.asarray(NAN_PAYLOADS, np.uint32).view(F)
    return np.concatenate([cloud, nan_w]), found


HEIGHT_LIDAR_Z = (0.0, -0.0, 0.1, 1.73)
HEIGHT_PARAMS = dict(downsample_method="NONE", outlier_removal_method="NONE")


def height_test_values(lz):
    """z values at the height predicate's threshold: float32(lz), two floats either side (which brackets the double lz), and +-0."""
    z = F(lz)
    vals = [z]
    lo = hi = z
    for _ in range(2):
        lo, hi = np.nextafter(lo, F(-np.inf)), np.nextafter(hi, F(np.inf))
        vals += [lo, hi]
    return np.asarray(vals + [F(0.0), F(-0.0)], F)


def height_cloud(lz):
    """A wall in the plane x = 5 (+- 1 mm): one column per test value with the test point at its foot and four rows 0.1 m apart above
    max(lz, 0), which the height filter keeps.  Every kept point has ten neighbours in the wall, so its normal is close to the x axis and
    the normal filter keeps it: the 2-D output shows, by its w lane, exactly which test points passed the height filter."""
    vals = np.repeat(height_test_values(lz), 3)
    m = vals.shape[0]
    rng = np.random.default_rng(17)
    base = max(float(lz), 0.0)
    cols = []
    for j in range(m):
        y = -1.0 + 0.1 * j
        cols.append([5.0 + rng.uniform(-1e-3, 1e-3), y, vals[j]])
        cols += [[5.0 + rng.uniform(-1e-3, 1e-3), y, base + 0.1 * r] for r in range(1, 5)]
    return with_index(np.asarray(cols, np.float64).astype(F))


# ==================================================================================================== tie clouds
def lattice_plane(spacing=0.25, side=80, z=1.0, x0=2.0):
    """An exact square lattice in the plane z = const: 4 neighbours at d, 4 at d * sqrt(2), 4 at 2 d -- every coordinate and every
    difference is exact in float32, so equal distances are equal bit for bit."""
    a = x0 + spacing * np.arange(side)
    g = np.stack(np.meshgrid(a, a - (x0 + spacing * side / 2), indexing="ij"), -1).reshape(-1, 2)
    return with_index(np.concatenate([g, np.full((g.shape[0], 1), z)], 1))


def cubic_lattice(spacing=0.25, side=16, x0=2.0):
    a = x0 + spacing * np.arange(side)
    g = np.stack(np.meshgrid(a, a - 4.0, a - 3.0, indexing="ij"), -1).reshape(-1, 3)
    return with_index(g)


def duplicates(distinct=200, fold=20, seed=23):
    """`distinct` points with coordinates on a 1/8 grid (every moment of ten copies is exact: the covariance is exactly zero), each
    `fold` times, interleaved so that the copies of a point are `distinct` indices apart."""
    rng = np.random.default_rng(seed)
    p = rng.integers(16, 80, (distinct, 3)) / 8.0
    return with_index(np.tile(p, (fold, 1)))


def ring(n=2048, radius=10.0, z=0.5):
    """One ring of a spinning LiDAR: locally collinear points, symmetric neighbours at (nearly or exactly) equal distances."""
    a = 2 * np.pi * np.arange(n) / n
    return with_index(np.stack([radius * np.cos(a), radius * np.sin(a), np.full(n, z)], 1))


def line(n=256, spacing=0.25):
    """Exactly collinear: y and z constant, so only the xx entry of the covariance is non-zero and every cross product is zero."""
    return with_index(np.stack([2.0 + spacing * np.arange(n), np.full(n, 2.0), np.full(n, 1.0)], 1))


def quantised_crop(down, n=8192, step=0.002):
    """The n points of `down` (the distance-filtered, voxel-grid down-sampled HDL-64 scan) nearest to the sensor, in their order, with
    coordinates rounded to the 2 mm of a real driver."""
    d = np.asarray(down, F)
    near = np.sort(np.argsort(f32_norm(d[:, :3]), kind="stable")[:n])
    return with_index(np.round(d[near, :3].astype(np.float64) / step) * step)


def exact_radius(spacing, squares):
    """A double r with r * r == squares * spacing^2 exactly (the float32 d^2 of a lattice neighbour), or None."""
    target = float(F(squares * spacing * spacing))
    r = np.sqrt(target)
    for cand in (r, np.nextafter(r, 0.0), np.nextafter(r, np.inf)):
        if cand * cand == target:
            return float(cand)
    return None


def lattice_half():
    """Spacing 0.5, for radius_radius = 0.5: 0.5 * 0.5 == 0.25f == the d^2 of the four nearest neighbours."""
    return lattice_plane(spacing=0.5, side=64, z=1.0, x0=2.0)


# Near 0.25 * sqrt(2), the d^2 = 0.125f of the four diagonal neighbours: no double squares to 0.125 exactly (sqrt(0.125) and its two
# neighbours miss it), so R_DIAG is None and that lattice case is dropped; the spacings 0.5 and 0.25 with r = spacing are exact.
R_DIAG = exact_radius(0.25, 2)

# name -> (builder, radius cases [(radius, min_neighbors)], statistical cases [(mean_k, mul)] or None).
# The lattices, the ring among them, are not statistical cases: away from the border every mean distance is the same number, the variance is the rounding of
# a difference of two equal sums and its sign decides every point at once -- chaotic by construction, not a property of the kernel.
# For the duplicates a mean_k below the fold gives mean distances that are all zero (variance 0): only mean_k >= fold is a case.
TIE_CLOUDS = {
    "lattice_plane": (lattice_plane, [(0.25, 4), (0.3, 2)] + ([(R_DIAG, 8)] if R_DIAG else []), None),
    "lattice_half": (lattice_half, [(0.5, 2), (0.5, 4)], None),
    "cubic_lattice": (cubic_lattice, [(0.25, 6), (0.25, 3)], None),
    "duplicates": (duplicates, [(0.0, 19), (0.2, 20), (0.5, 31)], [(20, 1.0), (31, 0.5)]),
    "ring": (ring, [(0.05, 2), (0.1, 6)], None),       # a lattice in one dimension: variance / mean^2 is 4e-11 (mean_k 5), not a case
    "line": (line, [(0.25, 2), (0.5, 4)], None),
    "quantised_crop": (None, [(0.5, 2), (0.2, 5), (0.1, 1)], [(20, 1.0), (30, 1.2), (5, 0.5)]),
}
# clouds whose k-th squared distance equals r * r exactly for (radius, min_neighbors): the two values of radius_inclusive must differ
EXACT_TIE_RADIUS = [("lattice_half", 0.5, 2), ("lattice_half", 0.5, 4), ("lattice_plane", 0.25, 4)] + ([("lattice_plane", R_DIAG, 8)] if R_DIAG else [])
SWITCHES = (1, 0)


def tie_cloud(name, down=None):
    build = TIE_CLOUDS[name][0]
    return quantised_crop(down) if build is None else build()


def tie_chain_params(name):
    """The chain on a tie cloud: no down-sampling (the voxel grid's centroids would undo the construction), the cloud's first radius
    case, or its first statistical case."""
    _, radius, stat = TIE_CLOUDS[name]
    out = [dict(downsample_method="NONE", outlier_removal_method="RADIUS", radius_radius=radius[0][0], radius_min_neighbors=radius[0][1], distance_near_thresh=0.1)]
    if stat:
        out.append(dict(downsample_method="NONE", outlier_removal_method="STATISTICAL", statistical_mean_k=stat[0][0], statistical_stddev=stat[0][1]))
    return out


# ==================================================================================================== list lengths
def blob(n, seed=31):
    """n points uniform in a 2 m cube, 3 m from the sensor."""
    return with_index(np.random.default_rng(seed + n).uniform(2.0, 4.0, (n, 3)))


# (mean_k, n): mean_k + 1 is the smallest legal cloud.  At (1, 2) both points have the same mean distance d and the variance is what
# the float product d * d leaves of 2 * fl(d * d) - 2 d^2: 1e-8 of the squared mean for this blob and positive, so the case stands.
STATISTICAL_LENGTHS = [(1, 2), (1, 3), (1, 33), (1, 257), (2, 3), (2, 4), (2, 33), (2, 257), (31, 32), (31, 33), (31, 257)]
# (min_neighbors, n): k = min_neighbors + 1; n = k - 1 removes everything (no point finds k neighbours), n = k is the smallest cloud that can keep one
RADIUS_LENGTHS = [(0, 1), (0, 2), (0, 33), (0, 257), (1, 1), (1, 2), (1, 3), (1, 33), (1, 257), (31, 31), (31, 32), (31, 33), (31, 257)]
RADIUS_LENGTH_RADII = (0.0, 0.4, 1.5)          # r = 0 with min_neighbors = 0: d_k^2 = 0 == r * r, the switch decides every point
NORMAL_LENGTHS = (1, 2, 3, 9, 10, 11)


# ==================================================================================================== voxel index overflow
def overflow_box(interior=300, seed=41):
    """A frame whose bounding box is 199 m x 199 m x 60 m with every point inside the default far threshold of 100 m.  The eight corners
    of such a box lie 144 m out and would not survive the distance filter, so the box is spanned by the centres of its six faces and by
    two more points on the x faces; a few hundred points near the sensor fill it.  At leaf 0.1 that is 1991 * 1991 * 601 = 2.38e9 cells,
    more than INT32_MAX."""
    rng = np.random.default_rng(seed)
    span = np.array([[99.5, 0, 0], [-99.5, 0, 0], [0, 99.5, 0], [0, -99.5, 0], [0, 0, 30], [0, 0, -30], [99.5, 0.5, 1], [-99.5, -0.5, 1]])
    inner = rng.uniform([-20, -20, 0.2], [20, 20, 3.0], (interior, 3))
    inner = inner[np.linalg.norm(inner, axis=1) > 2.0]
    return with_index(np.concatenate([span, inner]))


def voxel_cells(cloud, leaf=0.1):
    """The dense index size of pcl::VoxelGrid for this cloud: the product of the per-axis divisions."""
    c = np.asarray(cloud, F)[:, :3]
    inv = F(1.0) / F(leaf)
    lo = np.floor(c.min(0) * inv).astype(np.int64)
    hi = np.floor(c.max(0) * inv).astype(np.int64)
    return int(np.prod(hi - lo + 1))
