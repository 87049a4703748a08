"""numpy restatement of PrefilteringNodelet's filter chain (apps/prefiltering_nodelet.cpp:111-291, PCL 1.10), float op for op.

k-NN sets: candidates by brute force (small clouds) or from scipy's cKDTree, in a window that grows until no tie group of a k-th
distance is cut; the float32 FLANN distance (tests/helpers.py::f32_sqdist) recomputed and sorted by (distance, index) -- the order
relation of the HIP k-NN.  The switches are the ABI's (dgs_prefilter_params): same names.
Down-sampling is the oracle's VoxelGrid / ApproximateVoxelGrid restatement (oracle/oracle.py), which the device matches bit for bit.
"""
from __future__ import annotations

import hashlib

import numpy as np
from scipy.spatial import cKDTree

from helpers import f32_sqdist

F = np.float32
FLT_EPSILON = F(np.finfo(np.float32).eps)
FLT_MIN = F(np.finfo(np.float32).tiny)
NORMAL_K = 10                 # ne.setKSearch(10) (:227)
NORMAL_THRESH = F(0.2)        # normal_filter_thresh (:235)
NORMAL_BAND = 1e-4            # |n.z| this close to the threshold: libm / device trig may decide either way
RADIUS_INCLUSIVE = True       # dgs_prefilter_params.radius_inclusive default: keep iff d_k^2 <= r^2
STATISTICAL_SQRT_FLOAT = True # dgs_prefilter_params.statistical_sqrt_float default: sqrt of the float d^2 in float
DEFAULTS = dict(downsample_method="VOXELGRID", downsample_resolution=0.1, outlier_removal_method="STATISTICAL", statistical_mean_k=20,
                statistical_stddev=1.0, radius_radius=0.8, radius_min_neighbors=2, use_distance_filter=True, distance_near_thresh=1.0,
                distance_far_thresh=100.0)
LAUNCH = dict(DEFAULTS, distance_near_thresh=0.1, outlier_removal_method="RADIUS", statistical_mean_k=30, statistical_stddev=1.2,
              radius_radius=0.5, radius_min_neighbors=2)   # launch/delta_graph_slam.launch:30-42


def distance_filter(cloud, near=1.0, far=100.0):
    c = np.asarray(cloud, F)
    x, y, z = c[:, 0], c[:, 1], c[:, 2]
    with np.errstate(invalid="ignore", over="ignore"):
        d = np.sqrt((x * x + y * y) + z * z).astype(np.float64)
        keep = (d > near) & (d < far)
    return c[keep].copy()


_KNN_MEMO = {}
KNN_BRUTE_MAX = 8192          # up to here the candidates come from all n float32 distances, not from the tree


def _candidates(p, m, brute):
    """[n, m] indices holding, per point, m points none of the others is nearer than: in the float32 FLANN distance (brute force) or in
    cKDTree's float64 one.  Which members of a tie group at the m-th place are taken is arbitrary: knn() checks that it does not matter."""
    n = p.shape[0]
    if not brute:
        _, cand = cKDTree(p.astype(np.float64)).query(p.astype(np.float64), k=m)
        return np.asarray(cand).reshape(n, m)
    cand = np.empty((n, m), np.int64)
    for a in range(0, n, 512):
        d2 = f32_sqdist(p[a:a + 512, None, :], p[None, :, :])
        cand[a:a + 512] = np.argpartition(d2, m - 1, axis=1)[:, :m] if m < n else np.arange(n)[None, :]
    return cand


def knn(pts, k, margin=8, brute=None):
    """-> (idx [n,k] int64 (-1 none), d2 [n,k] float32 (inf none), tie [n] bool: k-th and (k+1)-th distances are equal).

    Safe under ties: the candidate window grows until, for every point, its last candidate is strictly farther than the k-th neighbour
    (or the window is the whole cloud), so the whole tie group of the k-th distance is inside the window and the (distance, index) order
    decides its members.  brute: all n distances in float32 (default up to KNN_BRUTE_MAX points), else cKDTree candidates."""
    p = np.ascontiguousarray(np.asarray(pts, F)[:, :3])
    n = p.shape[0]
    kk = min(k, n)
    if brute is None:
        brute = n <= KNN_BRUTE_MAX
    memo = (hashlib.sha1(p.tobytes()).digest(), n, k, margin, bool(brute))   # the tests ask for the same lists under both switch values
    if memo in _KNN_MEMO:
        return _KNN_MEMO[memo]
    with np.errstate(invalid="ignore", over="ignore"):
        while True:
            m = min(n, k + margin)
            cand = _candidates(p, m, brute)
            d2 = f32_sqdist(p[:, None, :], p[cand])
            order = np.lexsort((cand, d2), axis=-1)
            cand = np.take_along_axis(cand, order, 1)
            d2 = np.take_along_axis(d2, order, 1)
            cut = int(np.count_nonzero(~(d2[:, m - 1] > d2[:, kk - 1]))) if m < n else 0
            if cut == 0:
                break
            margin *= 2
    assert cut == 0                  # a condition, not a tolerance: no point's k-th tie group may be cut by the window
    idx = np.full((n, k), -1, np.int64)
    dd = np.full((n, k), np.inf, F)
    idx[:, :kk] = cand[:, :kk]
    dd[:, :kk] = d2[:, :kk]
    tie = (d2[:, kk - 1] == d2[:, kk]) if m > kk else np.zeros(n, bool)
    if len(_KNN_MEMO) >= 8:
        _KNN_MEMO.pop(next(iter(_KNN_MEMO)))
    _KNN_MEMO[memo] = (idx, dd, tie)
    return idx, dd, tie


def radius_outlier_removal(cloud, radius, min_neighbors, inclusive=RADIUS_INCLUSIVE):
    c = np.asarray(cloud, F)
    k = min_neighbors + 1
    n = c.shape[0]
    if n < k:
        return c[:0].copy(), np.zeros(0, bool)
    _, dd, tie = knn(c, k)
    dk = dd[:, k - 1].astype(np.float64)
    keep = (dk <= radius * radius) if inclusive else (dk < radius * radius)
    return c[keep].copy(), tie


def statistical_mean_distances(cloud, mean_k, sqrt_float=STATISTICAL_SQRT_FLOAT):
    c = np.asarray(cloud, F)
    _, dd, tie = knn(c, mean_k + 1)
    dist_sum = np.zeros(c.shape[0], np.float64)
    for j in range(1, mean_k + 1):   # index 0 is the query point
        dist_sum += np.sqrt(dd[:, j]).astype(np.float64) if sqrt_float else np.sqrt(dd[:, j].astype(np.float64))
    return (dist_sum / mean_k).astype(F), tie


def statistical_threshold(distances, mul):
    d = np.asarray(distances, F)
    n = float(d.shape[0])
    s = float(np.sum(d.astype(np.float64)))
    sq = float(np.sum((d * d).astype(np.float64)))
    mean = s / n
    var = (sq - s * s / n) / (n - 1.0)
    std = np.sqrt(var)
    return mean, std, mean + mul * std


def statistical_outlier_removal(cloud, mean_k, mul, sqrt_float=STATISTICAL_SQRT_FLOAT):
    c = np.asarray(cloud, F)
    if c.shape[0] == 0:
        return c.copy(), dict(distances=np.zeros(0, F), threshold=np.nan, near=0, tie=np.zeros(0, bool))
    if c.shape[0] <= mean_k:
        raise ValueError("n <= mean_k")
    dist, tie = statistical_mean_distances(c, mean_k, sqrt_float)
    mean, std, thr = statistical_threshold(dist, mul)
    keep = ~(dist.astype(np.float64) > thr)
    near = np.abs(dist.astype(np.float64) - thr) <= 1e-9 * abs(thr)
    return c[keep].copy(), dict(distances=dist, mean=mean, stddev=std, threshold=thr, near=near, tie=tie)


def height_filter(cloud, lz=0.0):
    c = np.asarray(cloud, F)
    return c[c[:, 2].astype(np.float64) > lz].copy()


# ---- pcl::eigen33 in float32, vectorised over points ------------------------------------------------------------------------
def _roots2(b, c):
    d = ((b * b).astype(np.float64) - 4.0 * c.astype(np.float64)).astype(F)
    d = np.where(d < 0, F(0), d)
    sd = np.sqrt(d)
    return np.zeros_like(b), F(0.5) * (b - sd), F(0.5) * (b + sd)


def _roots(m, census=None):
    m00, m01, m02, m11, m12, m22 = m[:, 0], m[:, 1], m[:, 2], m[:, 4], m[:, 5], m[:, 8]
    c0 = m00 * m11 * m22 + F(2) * m01 * m02 * m12 - m00 * m12 * m12 - m11 * m02 * m02 - m22 * m01 * m01
    c1 = m00 * m11 - m01 * m01 + m00 * m22 - m02 * m02 + m11 * m22 - m12 * m12
    c2 = m00 + m11 + m22
    s_inv3 = F(1.0 / 3.0)
    s_sqrt3 = np.sqrt(F(3))
    c2_over_3 = c2 * s_inv3
    a_over_3 = (c1 - c2 * c2_over_3) * s_inv3
    a_over_3 = np.where(a_over_3 > 0, F(0), a_over_3)
    half_b = F(0.5) * (c0 + c2_over_3 * (F(2) * c2_over_3 * c2_over_3 - c1))
    q = half_b * half_b + a_over_3 * a_over_3 * a_over_3
    q = np.where(q > 0, F(0), q)
    rho = np.sqrt(-a_over_3)
    theta = np.arctan2(np.sqrt(-q), half_b) * s_inv3
    ct, st = np.cos(theta), np.sin(theta)
    r0 = c2_over_3 + F(2) * rho * ct
    r1 = c2_over_3 - rho * (ct + s_sqrt3 * st)
    r2 = c2_over_3 - rho * (ct - s_sqrt3 * st)
    sw = r0 >= r1
    r0, r1 = np.where(sw, r1, r0), np.where(sw, r0, r1)
    sw = r1 >= r2
    r1, r2 = np.where(sw, r2, r1), np.where(sw, r1, r2)
    sw2 = sw & (r0 >= r1)
    r0, r1 = np.where(sw2, r1, r0), np.where(sw2, r0, r1)
    q0, q1, q2 = _roots2(c2, c1)
    use2 = (np.abs(c0) < FLT_EPSILON) | (r0 <= 0)
    if census is not None:
        census["c0_small"] = np.abs(c0) < FLT_EPSILON
        census["root_nonpositive"] = ~census["c0_small"] & (r0 <= 0)
    return np.where(use2, q0, r0)


def eigen33_smallest(cov9, census=None):
    """census: a dict that receives one boolean mask per branch of eigen33 (which points took it); the arithmetic is the same."""
    cov9 = np.asarray(cov9, F)
    scale = np.abs(cov9).max(axis=1)
    if census is not None:
        census["scale_tiny"] = scale <= FLT_MIN
    scale = np.where(scale <= FLT_MIN, F(1), scale)
    m = cov9 / scale[:, None]
    r0 = _roots(m, census)
    m = m.copy()
    for a in (0, 4, 8):
        m[:, a] = m[:, a] - r0
    rows = [m[:, 0:3], m[:, 3:6], m[:, 6:9]]

    def cross(u, v):
        return np.stack([u[:, 1] * v[:, 2] - u[:, 2] * v[:, 1], u[:, 2] * v[:, 0] - u[:, 0] * v[:, 2], u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]], 1)

    v1, v2, v3 = cross(rows[0], rows[1]), cross(rows[0], rows[2]), cross(rows[1], rows[2])
    l1, l2, l3 = [(v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2] for v in (v1, v2, v3)]
    pick1 = (l1 >= l2) & (l1 >= l3)
    pick2 = ~pick1 & (l2 >= l1) & (l2 >= l3)
    v = np.where(pick1[:, None], v1, np.where(pick2[:, None], v2, v3))
    ln = np.where(pick1, l1, np.where(pick2, l2, l3))
    if census is not None:
        census["pick1"], census["pick2"], census["pick3"] = pick1, pick2, ~pick1 & ~pick2
    return v / np.sqrt(ln)[:, None]


def normals(cloud, lidar=(0.0, 0.0, 0.0), census=None):
    """-> (normals [n,3] normalised and flipped, cov9 [n,9], keep [n], band [n], tie [n])."""
    c = np.asarray(cloud, F)
    n = c.shape[0]
    k = min(NORMAL_K, n)
    idx, _, tie = knn(c, k)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        acc = np.zeros((n, 9), F)
        for j in range(k):
            p = c[idx[:, j], :3]
            x, y, z = p[:, 0], p[:, 1], p[:, 2]
            for a, v in enumerate((x * x, x * y, x * z, y * y, y * z, z * z, x, y, z)):
                acc[:, a] = acc[:, a] + v
        acc = acc / F(k)
        cov = np.empty((n, 9), F)
        cov[:, 0] = acc[:, 0] - acc[:, 6] * acc[:, 6]
        cov[:, 1] = acc[:, 1] - acc[:, 6] * acc[:, 7]
        cov[:, 2] = acc[:, 2] - acc[:, 6] * acc[:, 8]
        cov[:, 4] = acc[:, 3] - acc[:, 7] * acc[:, 7]
        cov[:, 5] = acc[:, 4] - acc[:, 7] * acc[:, 8]
        cov[:, 8] = acc[:, 5] - acc[:, 8] * acc[:, 8]
        cov[:, 3], cov[:, 6], cov[:, 7] = cov[:, 1], cov[:, 2], cov[:, 5]
        nv = eigen33_smallest(cov, census)
        vp = np.asarray([F(lidar[0]), F(lidar[1]), F(lidar[2])], F)
        d = vp[None, :] - c[:, :3]
        cos_t = (d[:, 0] * nv[:, 0] + d[:, 1] * nv[:, 1]) + d[:, 2] * nv[:, 2]
        nv = np.where((cos_t < 0)[:, None], -nv, nv)
        zz = (nv[:, 0] * nv[:, 0] + nv[:, 1] * nv[:, 1]) + nv[:, 2] * nv[:, 2]
        nv = np.where((zz > 0)[:, None], nv / np.sqrt(np.where(zz > 0, zz, F(1)))[:, None], nv)
        if k < 3:
            nv[:] = np.nan
            cov[:] = np.nan
        keep = np.abs(nv[:, 2]) < NORMAL_THRESH
        band = np.abs(np.abs(nv[:, 2]).astype(np.float64) - float(NORMAL_THRESH)) < NORMAL_BAND
    return nv, cov, keep, band, tie


def normal_filter(cloud, lidar=(0.0, 0.0, 0.0)):
    c = np.asarray(cloud, F)
    if c.shape[0] == 0:
        return c.copy(), np.zeros(0, bool)
    _, _, keep, band, _ = normals(c, lidar)
    return c[keep].copy(), band


def flatten(cloud):
    out = np.array(cloud, F, copy=True)
    out[:, 2] = 0
    return out


def cloud_callback(cloud, params=None, lidar=(0.0, 0.0, 0.0), orc=None):
    """-> (filtered3d, filtered2d, info): info has the band masks / counts of the stages."""
    pr = dict(DEFAULTS)
    pr.update(params or {})
    info = {}
    c = distance_filter(cloud, pr["distance_near_thresh"], pr["distance_far_thresh"])
    if c.shape[0] and pr["downsample_method"] == "VOXELGRID":
        c = orc.voxel_grid(c, pr["downsample_resolution"])
    elif c.shape[0] and pr["downsample_method"] == "APPROX_VOXELGRID":
        c = orc.approx_voxel_grid(c, pr["downsample_resolution"])
    if pr["outlier_removal_method"] == "STATISTICAL":
        c, st = statistical_outlier_removal(c, pr["statistical_mean_k"], pr["statistical_stddev"],
                                                pr.get("statistical_sqrt_float", STATISTICAL_SQRT_FLOAT))
        info["statistical_near"] = int(np.count_nonzero(st["near"]))
    elif pr["outlier_removal_method"] == "RADIUS":
        c, tie = radius_outlier_removal(c, pr["radius_radius"], pr["radius_min_neighbors"], pr.get("radius_inclusive", RADIUS_INCLUSIVE))
        info["radius_ties"] = int(np.count_nonzero(tie))
    f3 = c
    h = height_filter(f3, lidar[2])
    if h.shape[0]:
        nv, cov, keep, band, _ = normals(h, lidar)
        info["normal_band"] = band
        f2 = flatten(h[keep])
    else:
        info["normal_band"] = np.zeros(0, bool)
        f2 = h.copy()
    info["height"] = h
    return f3, f2, info
