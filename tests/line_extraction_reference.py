"""numpy restatement of LineBasedScanmatcher::line_extraction as DESIGN.md 6e states it: the float32 operations one by one where the
contract is exact (draw stream, sample model, inlier test, walk, refit sums, clustering), float64 where upstream is double.
No device, no library: the GPU tests compare against this, the CPU tests check it on its own."""
import numpy as np

F = np.float32
INT_MAX = 2**31 - 1
DEFAULTS = dict(min_cluster_size=25, max_cluster_size=25000, cluster_tolerance=1.0, sac_distance_threshold=0.1, max_iterations=500,
                merror_threshold=150.0, line_length_threshold=1.0, sac_method_type=0, sample_good_any_axis=1, sqnorm_order=0,
                cluster_inclusive=1, max_rounds=4096)
LAUNCH = dict(min_cluster_size=40, max_cluster_size=25000, cluster_tolerance=1.5, sac_distance_threshold=0.1, max_iterations=100,
              merror_threshold=0.1, line_length_threshold=1.5)      # launch/delta_graph_slam.launch:149-156


class MT19937:
    """The standard's mt19937; the 10000th output of seed 5489 is 4123659995."""

    def __init__(self, seed=5489):
        mt = [seed & 0xFFFFFFFF]
        for i in range(1, 624):
            mt.append((1812433253 * (mt[-1] ^ (mt[-1] >> 30)) + i) & 0xFFFFFFFF)
        self.mt, self.i = mt, 624

    def __call__(self):
        if self.i >= 624:
            mt = self.mt
            for k in range(624):
                y = (mt[k] & 0x80000000) | (mt[(k + 1) % 624] & 0x7FFFFFFF)
                mt[k] = mt[(k + 397) % 624] ^ (y >> 1) ^ (0x9908B0DF if y & 1 else 0)
            self.i = 0
        y = self.mt[self.i]
        self.i += 1
        y ^= y >> 11
        y ^= (y << 7) & 0x9D2C5680
        y ^= (y << 15) & 0xEFC60000
        y ^= y >> 18
        return y & 0xFFFFFFFF


_MT_RAW = []


def mt_raw(count):
    """boost::mt19937(12345)() >> 1, the first `count` values (uniform_int<>(0, INT_MAX))."""
    if len(_MT_RAW) < count:
        g = MT19937(12345)
        _MT_RAW[:] = [g() >> 1 for _ in range(max(2 * count, 4096))]
    return _MT_RAW[:count]


class StreamEnd(Exception):
    pass


def draw_stream(n, raw=None):
    """Generator of (s[0], s[1]) per draw: drawIndexSample on an identity permutation that carries over between draws."""
    s = {}
    get = lambda i: s.get(i, i)
    d = 0
    while True:
        if raw is None:
            if 2 * d + 2 > len(_MT_RAW):
                mt_raw(2 * d + 2)
            r0, r1 = _MT_RAW[2 * d], _MT_RAW[2 * d + 1]
        else:
            if 2 * d + 2 > len(raw):
                raise StreamEnd()
            r0, r1 = int(raw[2 * d]), int(raw[2 * d + 1])
        a = r0 % n
        s[0], s[a] = get(a), get(0)
        b = 1 + r1 % (n - 1)
        s[1], s[b] = get(b), get(1)
        d += 1
        yield get(0), get(1)


def sample_good(p0, p1, any_axis=1):
    ne = p0[:3] != p1[:3]
    return bool(ne.any() if any_axis else ne.all())


def sample_model(p0, p1):
    u = (p1[:3] - p0[:3]).astype(F)
    n2 = F(F(F(u[0] * u[0]) + F(u[1] * u[1])) + F(u[2] * u[2]))
    if n2 > 0:
        u = (u / np.sqrt(n2)).astype(F)
    return p0[:3].astype(F).copy(), u


def sq_distances(pts, p0, u, order=0):
    """(p0 - p).cross3(u).squaredNorm() per point in float32, the three terms associated as sqnorm_order says."""
    a = (p0[None, :] - pts[:, :3]).astype(F)
    cx = a[:, 1] * u[2] - a[:, 2] * u[1]
    cy = a[:, 2] * u[0] - a[:, 0] * u[2]
    cz = a[:, 0] * u[1] - a[:, 1] * u[0]
    xx, yy, zz = cx * cx, cy * cy, cz * cz
    if order == 0:
        return (xx + yy) + (zz + F(0))
    if order == 1:
        return (xx + zz) + (yy + F(0))
    return ((xx + yy) + zz) + F(0)


def inlier_mask(pts, p0, u, thr, order=0):
    return sq_distances(pts, p0, u, order).astype(np.float64) < float(F(thr)) * float(F(thr))


def walk(counts, n, max_iterations):
    """RandomSampleConsensus::computeModel over a sequence of inlier counts -> (winner, iterations).  `counts` may be any indexable."""
    it, k, best, win = 0, 1.0, -INT_MAX, -1
    eps = np.finfo(np.float64).eps
    while it < k:
        c = counts[it]
        if c > best:
            best, win = c, it
            w = float(c) / float(n)
            p = 1.0 - w * w
            p = max(eps, p)
            p = min(1.0 - eps, p)
            k = float(np.log(1.0 - 0.99) / np.log(p))
        it += 1
        if it > max_iterations:
            break
    return win, it


def ransac(pts, prm, raw=None):
    """-> dict(status 'ok' | 'failed' | 'stream_end', draws, iterations, sample, p0, u, winner_rank: the walk's `win`)."""
    n = pts.shape[0]
    stream = draw_stream(n, raw)
    hyps = []
    state = dict(draws=0, status="ok")

    class Counts:
        def __getitem__(self, it):
            bad = 0
            while True:
                i0, i1 = next(stream)          # StreamEnd propagates
                state["draws"] += 1
                if sample_good(pts[i0], pts[i1], prm["sample_good_any_axis"]):
                    break
                bad += 1
                if bad == 1000:
                    raise ArithmeticError()
            p0, u = sample_model(pts[i0], pts[i1])
            hyps.append((i0, i1, p0, u))
            return int(inlier_mask(pts, p0, u, prm["sac_distance_threshold"], prm["sqnorm_order"]).sum())

    try:
        win, it = walk(Counts(), n, prm["max_iterations"])
    except ArithmeticError:
        return dict(status="failed", draws=state["draws"], iterations=len(hyps), sample=(-1, -1))
    except StreamEnd:
        return dict(status="stream_end", draws=state["draws"], iterations=len(hyps), sample=(-1, -1))
    i0, i1, p0, u = hyps[win]
    return dict(status="ok", draws=state["draws"], iterations=it, sample=(i0, i1), p0=p0, u=u, winner_rank=win)


def _trig(theta_args, trig):
    y, x = theta_args
    if trig == "f32":
        theta = F(np.arctan2(F(y), F(x)) * F(1.0 / 3.0))
        return F(np.cos(theta)), F(np.sin(theta))
    theta = F(F(np.arctan2(float(y), float(x))) * F(1.0 / 3.0))
    return F(np.cos(float(theta))), F(np.sin(float(theta)))


def compute_roots2(b, c):
    d = F(float(F(b * b)) - 4.0 * float(c))
    if d < 0:
        d = F(0)
    sd = np.sqrt(d)
    return [F(0), F(F(0.5) * F(b - sd)), F(F(0.5) * F(b + sd))]


def compute_roots(m, trig="f32"):
    """pcl::computeRoots on a symmetric float32 3 x 3 -> ascending roots."""
    m00, m01, m02, m11, m12, m22 = m[0, 0], m[0, 1], m[0, 2], m[1, 1], m[1, 2], m[2, 2]
    c0 = F(F(F(F(F(F(m00 * m11) * m22) + F(F(F(F(2) * m01) * m02) * m12)) - F(F(m00 * m12) * m12)) - F(F(m11 * m02) * m02)) - F(F(m22 * m01) * m01))
    c1 = F(F(F(F(F(F(m00 * m11) - F(m01 * m01)) + F(m00 * m22)) - F(m02 * m02)) + F(m11 * m22)) - F(m12 * m12))
    c2 = F(F(m00 + m11) + m22)
    if abs(c0) < np.finfo(F).eps:
        return compute_roots2(c2, c1)
    inv3, sqrt3 = F(1.0 / 3.0), np.sqrt(F(3))
    c2_3 = F(c2 * inv3)
    a_3 = F(F(c1 - F(c2 * c2_3)) * inv3)
    if a_3 > 0:
        a_3 = F(0)
    half_b = F(F(0.5) * F(c0 + F(c2_3 * F(F(F(F(2) * c2_3) * c2_3) - c1))))
    q = F(F(half_b * half_b) + F(F(a_3 * a_3) * a_3))
    if q > 0:
        q = F(0)
    rho = np.sqrt(F(-a_3))
    ct, st = _trig((np.sqrt(F(-q)), half_b), trig)
    r = [F(c2_3 + F(F(F(2) * rho) * ct)), F(c2_3 - F(rho * F(ct + F(sqrt3 * st)))), F(c2_3 - F(rho * F(ct - F(sqrt3 * st))))]
    if r[0] >= r[1]:
        r[0], r[1] = r[1], r[0]
    if r[1] >= r[2]:
        r[1], r[2] = r[2], r[1]
        if r[0] >= r[1]:
            r[0], r[1] = r[1], r[0]
    if r[0] <= 0:
        return compute_roots2(c2, c1)
    return r


def _cross(u, v):
    return np.array([F(F(u[1] * v[2]) - F(u[2] * v[1])), F(F(u[2] * v[0]) - F(u[0] * v[2])), F(F(u[0] * v[1]) - F(u[1] * v[0]))], F)


def eigenvector_of(cov, root_index, trig="f32"):
    """eigen33(mat, evals) then computeCorrespondingEigenVector(mat, evals[root_index])."""
    scale = F(np.abs(cov).max())
    if scale <= np.finfo(F).tiny:
        scale = F(1)
    sm = (cov / scale).astype(F)
    ev = F(compute_roots(sm, trig)[root_index] * scale)
    shift = F(ev / scale)
    for a in range(3):
        sm[a, a] = F(sm[a, a] - shift)
    vs = [_cross(sm[0], sm[1]), _cross(sm[0], sm[2]), _cross(sm[1], sm[2])]
    ls = [F(F(F(v[0] * v[0]) + F(v[1] * v[1])) + F(v[2] * v[2])) for v in vs]
    if ls[0] >= ls[1] and ls[0] >= ls[2]:
        v, l = vs[0], ls[0]
    elif ls[1] >= ls[0] and ls[1] >= ls[2]:
        v, l = vs[1], ls[1]
    else:
        v, l = vs[2], ls[2]
    return (v / np.sqrt(l)).astype(F)


def _seq_sum(x, dtype):
    return np.cumsum(x, dtype=dtype)[-1]      # cumsum adds in order, one rounding per term


def refit(pts, inl, p0, u, trig="f32"):
    """-> (line_xy float64 [2], dir_xy float64 [2] renormalised): optimizeModelCoefficients, then :360-364."""
    px, py, vx, vy = p0[0], p0[1], u[0], u[1]
    if inl.size > 2:
        q = pts[inl, :3].astype(F)
        c = np.array([_seq_sum(q[:, a], F) for a in range(3)], F) / F(inl.size)
        d = (q - c[None, :]).astype(F)
        cov = np.zeros((3, 3), F)
        for a in range(3):
            for b in range(a, 3):
                cov[a, b] = cov[b, a] = _seq_sum(d[:, a] * d[:, b], F)
        v = eigenvector_of(cov, 2, trig)
        px, py, vx, vy = c[0], c[1], v[0], v[1]
    dx, dy = float(vx), float(vy)
    z = dx * dx + dy * dy
    if z > 0:
        s = np.sqrt(z)
        dx, dy = dx / s, dy / s
    return np.array([float(px), float(py)]), np.array([dx, dy])


def components(q, tol, inclusive=1):
    """Connected components of float32 points q under d2 <= tol^2 (or <) -> list of index arrays, each ascending."""
    m = q.shape[0]
    tol2 = float(F(tol)) * float(F(tol))
    seen = np.zeros(m, bool)
    out = []
    for s in range(m):
        if seen[s]:
            continue
        seen[s] = True
        todo, comp = [s], []
        while todo:
            i = todo.pop()
            comp.append(i)
            d = (q[i][None, :] - q).astype(F)
            d2 = ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]).astype(np.float64)
            near = (d2 <= tol2) if inclusive else (d2 < tol2)
            new = np.nonzero(near & ~seen)[0]
            seen[new] = True
            todo.extend(new.tolist())
        out.append(np.sort(np.array(comp, np.int64)))
    return out


def cluster(pts, inl, prm):
    """extract_cluster -> positions of the cluster taken (ascending), or None when every component was dropped / there is none."""
    if inl.size == 0:
        return None
    comps = [c for c in components(pts[inl, :3].astype(F), prm["cluster_tolerance"], prm["cluster_inclusive"]) if c.size <= prm["max_cluster_size"]]
    if not comps:
        return None
    best = max(comps, key=lambda c: (c.size, -int(c[0])))
    return inl[best]


def statistics(pts, clu, line, d):
    """:383-442 in float64 -> (A, B, mean, sigma, max, min)."""
    p = pts[clu, :3].astype(np.float64)
    lx, ly, dx, dy = line[0], line[1], d[0], d[1]
    n2 = dx * dx + dy * dy
    nx, ny = (dx / np.sqrt(n2), dy / np.sqrt(n2)) if n2 > 0 else (dx, dy)
    tn = (p[:, 0] - lx) * nx + (p[:, 1] - ly) * ny
    ex, ey, ez = p[:, 0] - (lx + nx * tn), p[:, 1] - (ly + ny * tn), p[:, 2]
    err = np.sqrt((ex * ex + ey * ey) + ez * ez)
    mean = _seq_sum(err, np.float64) / float(clu.size)
    t0 = (p[:, 0] - lx) * dx + (p[:, 1] - ly) * dy
    vx, vy = lx + dx * t0, ly + dy * t0
    t = (vx - lx) * dx + (vy - ly) * dy
    ia, ib = int(np.argmin(t)), int(np.argmax(t))          # first of equal values: the strict comparisons of :423-429
    sigma = np.sqrt(_seq_sum((err - mean) * (err - mean), np.float64) / float(clu.size))
    A, B = np.array([vx[ia], vy[ia], 0.0]), np.array([vx[ib], vy[ib], 0.0])
    return A, B, float(mean), float(sigma), float(max(0.0, err.max())), float(min(100000.0, err.min()))


def line_extraction(cloud, params=None, raw=None, trig="f32"):
    """-> (lines, rounds, status).  lines: dicts A, B, mean, sigma, max, min; rounds: dicts with the trace, the index lists, for a round
    with a winner its rank among the hypotheses (winner_rank) and, for an evaluated cluster, mean and length (what the thresholds see)."""
    prm = dict(DEFAULTS)
    prm.update(params or {})
    pts = np.ascontiguousarray(cloud, F).copy()
    lines, rounds, status = [], [], "DONE"
    while pts.shape[0] >= prm["min_cluster_size"] and pts.shape[0] > 0:
        if len(rounds) >= prm["max_rounds"]:
            status = "MAX_ROUNDS"
            break
        n = pts.shape[0]
        rec = dict(n_before=n, draws=0, iterations=0, sample=(-1, -1), inliers=0, cluster=0, emitted=0, inlier_idx=np.zeros(0, np.int64),
                   cluster_idx=np.zeros(0, np.int64))
        rounds.append(rec)
        if n < 2:
            status = "RANSAC_FAILED"
            break
        r = ransac(pts, prm, raw)
        rec.update(draws=r["draws"], iterations=r["iterations"])
        if r["status"] != "ok":
            status = "RANSAC_FAILED" if r["status"] == "failed" else "RNG_EXHAUSTED"
            break
        inl = np.nonzero(inlier_mask(pts, r["p0"], r["u"], prm["sac_distance_threshold"], prm["sqnorm_order"]))[0]
        line, d = refit(pts, inl, r["p0"], r["u"], trig)
        clu = cluster(pts, inl, prm)
        rec.update(sample=r["sample"], winner_rank=r["winner_rank"], inliers=int(inl.size), inlier_idx=inl, cluster=0 if clu is None else int(clu.size),
                   cluster_idx=np.zeros(0, np.int64) if clu is None else clu)
        if clu is None:
            status = "STALL"
            break
        if clu.size >= prm["min_cluster_size"]:
            A, B, mean, sigma, mx, mn = statistics(pts, clu, line, d)
            length = float(np.sqrt(((A - B) ** 2).sum()))
            rec.update(mean=mean, length=length)
            if mean < float(F(prm["merror_threshold"])) and length > float(F(prm["line_length_threshold"])):
                rec["emitted"] = 1
                lines.append(dict(A=A, B=B, mean=mean, sigma=sigma, max=mx, min=mn))
        keep = np.ones(n, bool)
        keep[clu] = False
        pts = pts[keep]
    return lines, rounds, status


def scene(n, segments=2, seed=0, noise=0.02, clutter=0.3, z=0.0, length=8.0):
    """n float32 [N,4] points: `segments` planted 2-D segments with noise, the rest uniform clutter."""
    rng = np.random.default_rng(seed)
    n_cl = int(n * clutter)
    per = (n - n_cl) // segments
    out = []
    for s in range(segments):
        m = per if s < segments - 1 else n - n_cl - per * (segments - 1)
        ang = rng.uniform(0, np.pi)
        c = rng.uniform(-10, 10, 2)
        t = rng.uniform(-length / 2, length / 2, m)
        off = rng.normal(0, noise, m)
        x = c[0] + t * np.cos(ang) - off * np.sin(ang)
        y = c[1] + t * np.sin(ang) + off * np.cos(ang)
        out.append(np.stack([x, y], 1))
    out.append(rng.uniform(-15, 15, (n_cl, 2)))
    xy = np.concatenate(out)[rng.permutation(n)]
    pts = np.zeros((n, 4), F)
    pts[:, :2] = xy
    pts[:, 2] = z if np.isscalar(z) else rng.uniform(z[0], z[1], n)
    pts[:, 3] = 1
    return pts


SIZES = (24, 25, 63, 64, 65, 257, 1500, 4099)
ITERATIONS = (0, 1, 100)


def size_scene(n, max_iterations):
    """The planted scene of n points and its parameters: the constructor's defaults but for max_iterations, with a round cap that keeps
    the clutter's long tail of tiny clusters out of the tests (and reaches DGS_LE_MAX_ROUNDS on the large sizes)."""
    return scene(n, segments=2, seed=n), dict(max_iterations=max_iterations, max_rounds=12)


def nonflat_scene():
    """z != 0: the covariance has three non-zero roots, so the refit goes through eigen33's trigonometric branch."""
    return scene(900, segments=3, seed=7, noise=0.04, clutter=0.2, z=(-0.08, 0.08), length=3.0), dict(max_iterations=100, max_rounds=12)


_CACHE = {}


def cached(key, cloud, params, raw=None, trig="f32"):
    """line_extraction's result, computed once per key and shared between tests (read-only)."""
    if (key, trig) not in _CACHE:
        _CACHE[(key, trig)] = line_extraction(cloud, params, raw, trig)
    return _CACHE[(key, trig)]
