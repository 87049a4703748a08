"""numpy restatement of FloorDetectionNodelet::detect as DESIGN.md 6j states it: the float32 operations one by one (tilt transform, plane
clips, sample test, plane model, inlier test, checks), float64 where upstream is double (thresholds, the walk).  Step 3 is
prefilter_reference.normals.  No device, no library: the GPU tests compare against this, the CPU tests check it on its own."""
import math

import numpy as np

import prefilter_reference as PR
from line_extraction_reference import MT19937

F = np.float32
INT_MAX = 2**31 - 1
NORMAL_BAND = PR.NORMAL_BAND
DEFAULTS = dict(tilt_deg=0.0, sensor_height=2.0, height_clip_range=1.0, floor_pts_thresh=512, floor_normal_thresh=10.0,
                use_normal_filtering=1, normal_filter_thresh=20.0, distance_threshold=0.1, max_iterations=1000, probability=0.99,
                max_sample_checks=1000, transform_order=0, plane_dot_order=0)
STATUS = ("DETECTED", "TOO_FEW_POINTS", "TOO_FEW_INLIERS", "NOT_VERTICAL", "RNG_EXHAUSTED")

_MT_RAW = []


def mt_raw(count):
    """boost::mt19937(12345)() >> 1, the first `count` values."""
    if len(_MT_RAW) < count:
        g = MT19937(12345)
        _MT_RAW[:] = [g() >> 1 for _ in range(max(2 * count, 8192))]
    return _MT_RAW[:count]


class StreamEnd(Exception):
    pass


def draw_stream(n, raw=None):
    """Generator of (s[0], s[1], s[2]) per draw: drawIndexSample on an identity permutation that carries over between draws."""
    s = {}
    get = lambda i: s.get(i, i)
    d = 0
    while True:
        if raw is None:
            r = mt_raw(3 * d + 3)[3 * d:3 * d + 3]
        else:
            if 3 * d + 3 > len(raw):
                raise StreamEnd()
            r = [int(raw[3 * d]), int(raw[3 * d + 1]), int(raw[3 * d + 2])]
        for i in range(3):
            j = i + r[i] % (n - i)
            s[i], s[j] = get(j), get(i)
        d += 1
        yield get(0), get(1), get(2)


def raw_for_triples(n, triples):
    """The inverse of the three-swap permutation: raw values under which draw_stream(n, raw) yields `triples` (distinct indices each)."""
    s, pos = {}, {}
    gs = lambda i: s.get(i, i)
    gp = lambda v: pos.get(v, v)
    raw = []
    for t in triples:
        assert len(set(t)) == 3 and all(0 <= v < n for v in t)
        for i in range(3):
            j = gp(t[i])
            assert j >= i
            raw.append(j - i)
            a, b = gs(i), gs(j)
            s[i], s[j] = b, a
            pos[b], pos[a] = i, j
    return np.array(raw, np.uint32)


def tilt_matrices(tilt_deg):
    """AngleAxisf((float)(tilt_deg * M_PI / 180.0f), UnitY).toRotationMatrix() in an identity, and its float32 numpy.linalg.inv."""
    angle = F(float(tilt_deg) * math.pi / float(F(180.0)))
    s, c = F(np.sin(angle)), F(np.cos(angle))
    t = np.eye(4, dtype=F)
    t[0, 0] = F(F(0) + c)
    t[1, 1] = F(F(F(F(1) - c) * F(1)) + c)
    t[2, 2] = F(F(0) + c)
    t[0, 2] = F(F(0) + s)
    t[2, 0] = F(F(0) - s)
    return t, np.linalg.inv(t).astype(F)


def transform(cloud, m, order=0):
    """pcl::transformPointCloud(Matrix4f) in float32: the fourth float becomes 1, non-finite points go through the arithmetic."""
    c = np.asarray(cloud, F)
    m = np.asarray(m, F)
    out = np.ones_like(c)
    x, y, z = c[:, 0], c[:, 1], c[:, 2]
    with np.errstate(invalid="ignore", over="ignore"):
        for r in range(3):
            if order == 0:
                out[:, r] = x * m[r, 0] + (y * m[r, 1] + (z * m[r, 2] + m[r, 3]))
            else:
                out[:, r] = ((m[r, 0] * x + m[r, 1] * y) + m[r, 2] * z) + m[r, 3]
    return out


def clip(cloud, sensor_height, height_clip_range):
    c = np.asarray(cloud, F)
    hi, lo = F(sensor_height + height_clip_range), F(sensor_height - height_clip_range)
    with np.errstate(invalid="ignore", over="ignore"):
        base = (F(0) * c[:, 0] + F(0) * c[:, 1]) + F(1) * c[:, 2]
        keep = ((base + hi) >= 0) & ~((base + lo) >= 0)
    return c[keep].copy()


def normal_keep(clipped, sensor_height, thresh_deg):
    """-> (keep, band, tie, normals): the floor rule over prefilter_reference.normals with the viewpoint (0, 0, (float)sensor_height)."""
    nv, _, _, _, tie = PR.normals(clipped, (0.0, 0.0, float(F(sensor_height))))
    cos_thr = math.cos(thresh_deg * math.pi / 180.0)
    with np.errstate(invalid="ignore"):
        az = np.abs(nv[:, 2]).astype(np.float64)
        keep = az > cos_thr
        band = np.abs(az - cos_thr) < NORMAL_BAND
    return keep, band, tie, nv


def dot4(a, b, order):
    x, y, z, w = F(a[0] * b[0]), F(a[1] * b[1]), F(a[2] * b[2]), F(a[3] * b[3])
    if order == 0:
        return F(F(x + y) + F(z + w))
    if order == 1:
        return F(F(x + z) + F(y + w))
    return F(F(F(x + y) + z) + w)


def sample_good(p0, p1, p2):
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        r = (p1[:3] - p0[:3]).astype(F) / (p2[:3] - p0[:3]).astype(F)
    return bool(r[0] != r[1] or r[2] != r[1])


def plane_model(p0, p1, p2, order=0):
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        u, v = (p1[:3] - p0[:3]).astype(F), (p2[:3] - p0[:3]).astype(F)
        a = F(F(u[1] * v[2]) - F(u[2] * v[1]))
        b = F(F(u[2] * v[0]) - F(u[0] * v[2]))
        c = F(F(u[0] * v[1]) - F(u[1] * v[0]))
        s2 = dot4((a, b, c, F(0)), (a, b, c, F(0)), order)
        if s2 > 0:
            s = np.sqrt(s2)
            a, b, c = F(a / s), F(b / s), F(c / s)
        d = F(F(-1) * dot4((a, b, c, F(0)), (p0[0], p0[1], p0[2], p0[3]), order))
    return np.array([a, b, c, d], F)


def inlier_mask(pts, coef, thr, order=0):
    p = np.asarray(pts, F)
    with np.errstate(invalid="ignore", over="ignore"):
        x, y, z, w = coef[0] * p[:, 0], coef[1] * p[:, 1], coef[2] * p[:, 2], np.full(p.shape[0], coef[3] * F(1), F)
        if order == 0:
            d = (x + y) + (z + w)
        elif order == 1:
            d = (x + z) + (y + w)
        else:
            d = ((x + y) + z) + w
        return np.abs(d).astype(np.float64) < float(thr)


def walk(counts, n, max_iterations=1000, probability=0.99):
    """RandomSampleConsensus::computeModel over a sequence of inlier counts -> (winner, iterations, k_margin): k_margin is the smallest
    |k - it| over the loop's `it < k` decisions.  `counts` may be any indexable; an ArithmeticError from it is the empty selection."""
    it, k, best, win = 0, 1.0, -INT_MAX, -1
    eps = np.finfo(np.float64).eps
    log1mp = math.log(1.0 - probability)
    margin = math.inf
    failed = False
    while True:
        margin = min(margin, abs(k - it))
        if not it < k:
            break
        try:
            c = counts[it]
        except ArithmeticError:
            failed = True
            break
        if c > best:
            best, win = c, it
            w = float(c) / float(n)
            p = 1.0 - math.pow(w, 3.0)
            p = max(eps, p)
            p = min(1.0 - eps, p)
            k = log1mp / math.log(p)
        it += 1
        if it > max_iterations:
            break
    return win, it, margin, failed


def ransac(filtered, prm, raw=None):
    """Steps 5-8 -> dict(status 'ok' | 'stream_end', draws, iterations, winner_rank, sample, count, ransac_failed, coeffs (raw), inliers,
    k_margin)."""
    pts = np.asarray(filtered, F)
    n = pts.shape[0]
    out = dict(status="ok", draws=0, iterations=0, winner_rank=-1, sample=(-1, -1, -1), count=0, ransac_failed=0, coeffs=np.zeros(4, F),
               inliers=np.zeros(0, np.int64), k_margin=math.inf)
    if n < 3:
        out["ransac_failed"] = 1
        return out
    stream = draw_stream(n, raw)
    hyps = []
    state = dict(draws=0)
    order, thr = prm["plane_dot_order"], prm["distance_threshold"]

    class Counts:
        def __getitem__(self, it):
            bad = 0
            while True:
                i0, i1, i2 = next(stream)          # StreamEnd propagates
                state["draws"] += 1
                if sample_good(pts[i0], pts[i1], pts[i2]):
                    break
                bad += 1
                if bad == prm["max_sample_checks"]:
                    raise ArithmeticError()
            coef = plane_model(pts[i0], pts[i1], pts[i2], order)
            c = int(inlier_mask(pts, coef, thr, order).sum())
            hyps.append(((i0, i1, i2), coef, c))
            return c

    try:
        win, it, margin, failed = walk(Counts(), n, prm["max_iterations"], prm["probability"])
    except StreamEnd:
        out.update(status="stream_end", draws=state["draws"], iterations=len(hyps))
        return out
    out.update(draws=state["draws"], iterations=it, ransac_failed=int(failed), k_margin=margin)
    if win >= 0:
        sample, coef, c = hyps[win]
        out.update(winner_rank=win, sample=sample, count=c, coeffs=coef, inliers=np.nonzero(inlier_mask(pts, coef, thr, order))[0])
    return out


def finish(filtered, params=None, raw=None, tilt_inv=None):
    """Steps 4 (size check) to 9 from a filtered cloud -> dict(coeffs or None, status, inliers, trace)."""
    prm = dict(DEFAULTS)
    prm.update(params or {})
    if tilt_inv is None:
        tilt_inv = tilt_matrices(prm["tilt_deg"])[1]
    tilt_inv = np.asarray(tilt_inv, F)
    pts = np.asarray(filtered, F)
    res = dict(coeffs=None, status="TOO_FEW_POINTS", inliers=np.zeros(0, np.int64), trace=None)
    if pts.shape[0] < prm["floor_pts_thresh"]:
        return res
    r = ransac(pts, prm, raw)
    res["trace"] = r
    if r["status"] == "stream_end":
        res["status"] = "RNG_EXHAUSTED"
        return res
    res["inliers"] = r["inliers"]
    if r["inliers"].size < prm["floor_pts_thresh"]:
        res["status"] = "TOO_FEW_INLIERS"
        return res
    co = r["coeffs"].copy()
    ref = tilt_inv[:3, 2]
    with np.errstate(invalid="ignore", over="ignore"):
        dot = F(F(F(co[0] * ref[0]) + F(co[1] * ref[1])) + F(co[2] * ref[2]))
        r["dot"] = dot
        if abs(float(dot)) < math.cos(prm["floor_normal_thresh"] * math.pi / 180.0):
            res["status"] = "NOT_VERTICAL"
            return res
        up = F(F(F(F(0) * co[0]) + F(F(0) * co[1])) + F(F(1) * co[2]))
        if up < 0:
            co = (co * F(-1)).astype(F)
    res.update(coeffs=co, status="DETECTED")
    return res


def detect(cloud, params=None, raw=None, tilt=None, tilt_inv=None):
    """-> dict(coeffs or None, status, clipped, filtered, inliers, trace, band, tie, keep)."""
    prm = dict(DEFAULTS)
    prm.update(params or {})
    if prm["floor_pts_thresh"] < 0:
        raise ValueError("floor_pts_thresh < 0")
    c = np.ascontiguousarray(cloud, F)
    if tilt is None or tilt_inv is None:
        t, ti = tilt_matrices(prm["tilt_deg"])
        tilt = t if tilt is None else tilt
        tilt_inv = ti if tilt_inv is None else tilt_inv
    e = np.zeros(0, bool)
    res = dict(coeffs=None, status="TOO_FEW_POINTS", clipped=np.zeros((0, 4), F), filtered=np.zeros((0, 4), F), inliers=np.zeros(0, np.int64),
               trace=None, band=e, tie=e, keep=e)
    if c.shape[0] == 0:
        return res
    clipped = clip(transform(c, tilt, prm["transform_order"]), prm["sensor_height"], prm["height_clip_range"])
    kept = clipped
    if prm["use_normal_filtering"] and clipped.shape[0] > 0:
        keep, band, tie, _ = normal_keep(clipped, prm["sensor_height"], prm["normal_filter_thresh"])
        res.update(band=band, tie=tie, keep=keep)
        kept = clipped[keep]
    filtered = transform(kept, tilt_inv, prm["transform_order"])
    res.update(clipped=clipped, filtered=filtered)
    res.update(finish(filtered, prm, raw, tilt_inv))
    return res


# ---- scenes ----------------------------------------------------------------------------------------------------------------
def floor_scene(n_floor, n_clutter, seed=0, slope=(0.03, -0.02), height=-2.0, noise=0.02, extent=10.0, clutter_z=(-2.9, -1.1)):
    """float32 [N,4]: a planted floor z = height + slope . (x, y) + noise over [-extent, extent]^2 and uniform clutter inside the clip band,
    shuffled."""
    rng = np.random.default_rng(seed)
    xy = rng.uniform(-extent, extent, (n_floor, 2))
    z = height + slope[0] * xy[:, 0] + slope[1] * xy[:, 1] + rng.normal(0, noise, n_floor)
    cl = np.concatenate([rng.uniform(-extent, extent, (n_clutter, 2)), rng.uniform(clutter_z[0], clutter_z[1], (n_clutter, 1))], 1)
    pts = np.ones((n_floor + n_clutter, 4), F)
    pts[:, :3] = np.concatenate([np.concatenate([xy, z[:, None]], 1), cl])[rng.permutation(n_floor + n_clutter)]
    return pts


def grid_floor(nx, ny, spacing=0.25, height=-2.0, slope=(0.0, 0.0), jitter=0.0, seed=0):
    """A regular grid floor: with slope 0 and no jitter every interior normal is exactly vertical, so the normal band is empty."""
    rng = np.random.default_rng(seed)
    gx, gy = np.meshgrid(np.arange(nx) * spacing - nx * spacing / 2, np.arange(ny) * spacing - ny * spacing / 2, indexing="ij")
    x = gx.ravel() + rng.uniform(-jitter, jitter, nx * ny)
    y = gy.ravel() + rng.uniform(-jitter, jitter, nx * ny)
    pts = np.ones((nx * ny, 4), F)
    pts[:, 0], pts[:, 1], pts[:, 2] = x, y, height + slope[0] * x + slope[1] * y
    return pts


_CACHE = {}


def cached(key, fn):
    """fn()'s result, computed once per key and shared between tests (read-only)."""
    if key not in _CACHE:
        _CACHE[key] = fn()
    return _CACHE[key]
