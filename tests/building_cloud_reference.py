"""interpolate (upstream src/hdl_graph_slam/ros_utils.cpp:146-165), buildPointCloud's concatenation and getCloud's
pcl::transformPointCloud restated twice in float32: `clouds`, vectorised numpy (a table of the loop variable, an upper bound search, a
broadcast), and `clouds_scalar`, a plain loop with the running sum, written independently of the first.  Every operation is one IEEE
float32 add, subtract, multiply, divide or square root, so the two -- and the device -- must agree bit for bit."""
import numpy as np

from floor_detection_reference import transform

F = np.float32
STEP = F(0.02)
DEFAULTS = dict(sample_step=0.02, sqnorm_order=0, normalized_guard=1, transform_order=0, max_points_per_line=1 << 20)


class TooLong(ValueError):
    """a line whose norm is +inf or past the table's last entry: .item, .line (within the item), .flat (within the call)"""

    def __init__(self, item, line, flat):
        super().__init__(f"line {line} of item {item}")
        self.item, self.line, self.flat = item, line, flat


_tables = {}


def step_table(n, step=STEP):
    """i_0 = 0, i_{k+1} = fl(i_k + step): the first n entries, fewer where the sequence stops growing."""
    step = F(step)
    key = step.tobytes()
    t = _tables.get(key)
    if t is None or t.size < n:
        t = np.zeros(n, F)
        t[1:] = np.add.accumulate(np.full(n - 1, step, F), dtype=F)      # accumulate adds left to right, each sum rounded to float32
        stall = np.nonzero(np.diff(t) <= 0)[0]
        if stall.size:
            t = t[:stall[0] + 1]
        _tables[key] = t
    return t[:n]


def lines_array(lines):
    return np.ascontiguousarray(lines, np.float64).reshape(-1, 2, 3)


def line_records(lines, sqnorm_order=0, normalized_guard=1):
    """-> a (float32 [L, 3]), dn (the normalised direction) and norm per line"""
    l = lines_array(lines)
    a, b = l[:, 0].astype(F), l[:, 1].astype(F)
    with np.errstate(all="ignore"):
        d = b - a
        sq = d * d
        zero = F(0)
        if sqnorm_order == 0:
            n2 = (sq[:, 0] + sq[:, 1]) + (sq[:, 2] + zero)
        elif sqnorm_order == 1:
            n2 = (sq[:, 0] + sq[:, 2]) + (sq[:, 1] + zero)
        else:
            n2 = ((sq[:, 0] + sq[:, 1]) + sq[:, 2]) + zero
        norm = np.sqrt(n2)
        dn = d / norm[:, None]
        if normalized_guard:
            dn = np.where((n2 > 0)[:, None], dn, d)
    return a, dn.astype(F), norm.astype(F)


def _matrices(n_items, transforms):
    if transforms is None:
        return [None] * n_items
    if isinstance(transforms, np.ndarray) and transforms.shape == (4, 4):
        return [transforms] * n_items
    assert len(transforms) == n_items
    return list(transforms)


def clouds(items, transforms=None, params=None):
    """-> points float32 [N, 4], offsets int64 [len(items) + 1]"""
    p = dict(DEFAULTS, **(params or {}))
    arrays = [lines_array(it) for it in items]
    sizes = np.array([a.shape[0] for a in arrays], np.int64)
    flat = np.concatenate(arrays) if arrays else np.zeros((0, 2, 3))
    a, dn, norm = line_records(flat, p["sqnorm_order"], p["normalized_guard"])
    need = float(np.max(norm[np.isfinite(norm)], initial=0.0))
    entries = min(p["max_points_per_line"], int(need / float(F(p["sample_step"])) * 1.01) + 64)
    table = step_table(entries, p["sample_step"])
    while table.size == entries < p["max_points_per_line"] and not table[-1] > need:
        entries = min(p["max_points_per_line"], 2 * entries)
        table = step_table(entries, p["sample_step"])
    with np.errstate(invalid="ignore"):
        bad = np.nonzero(norm > table[-1])[0]
    if bad.size:
        if np.isfinite(norm[bad[0]]):                                        # past the table's true end, not past what was built of it
            assert table.size == p["max_points_per_line"] or step_table(table.size + 1, p["sample_step"]).size == table.size
        item = int(np.searchsorted(np.cumsum(sizes), bad[0], side="right"))
        raise TooLong(item, int(bad[0] - np.sum(sizes[:item])), int(bad[0]))
    counts = np.where(np.isnan(norm), 0, np.searchsorted(table, np.nan_to_num(norm, nan=0.0), side="right")).astype(np.int64)
    line_off = np.concatenate([[0], np.cumsum(counts)])
    owner = np.repeat(np.arange(flat.shape[0]), counts)
    k = np.arange(line_off[-1]) - line_off[owner]
    pts = np.zeros((int(line_off[-1]), 4), F)
    pts[:, 3] = 1
    with np.errstate(all="ignore"):
        ik = table[k]
        pts[:, 0] = a[owner, 0] + ik * dn[owner, 0]
        pts[:, 1] = a[owner, 1] + ik * dn[owner, 1]
    offsets = line_off[np.concatenate([[0], np.cumsum(sizes)])]
    for i, m in enumerate(_matrices(len(arrays), transforms)):
        if m is not None:
            pts[offsets[i]:offsets[i + 1]] = transform(pts[offsets[i]:offsets[i + 1]], np.asarray(m, F), p["transform_order"])
    return pts, offsets.astype(np.int64)


def interpolate_scalar(a, b, params=None):
    """ros_utils.cpp:146-165 line by line: the loop variable is the running float32 sum."""
    p = dict(DEFAULTS, **(params or {}))
    step = F(p["sample_step"])
    a = [F(v) for v in a]
    b = [F(v) for v in b]
    out = []
    with np.errstate(all="ignore"):
        d = [F(b[c] - a[c]) for c in range(3)]
        xx, yy, zz = F(d[0] * d[0]), F(d[1] * d[1]), F(d[2] * d[2])
        if p["sqnorm_order"] == 0:
            n2 = F(F(xx + yy) + F(zz + F(0)))
        elif p["sqnorm_order"] == 1:
            n2 = F(F(xx + zz) + F(yy + F(0)))
        else:
            n2 = F(F(F(xx + yy) + zz) + F(0))
        norm = F(np.sqrt(n2))
        if not p["normalized_guard"] or n2 > 0:
            dn = [F(d[c] / norm) for c in range(3)]
        else:
            dn = d
        if np.isinf(norm):
            return None
        i = F(0)
        while i <= norm:
            out.append((F(a[0] + F(i * dn[0])), F(a[1] + F(i * dn[1])), F(0), F(1)))
            nxt = F(i + step)
            if len(out) == p["max_points_per_line"] or not nxt > i:      # i is the last sample position there is
                return None if norm > i else out
            i = nxt
    return out


def transform_scalar(pt, m, order):
    m = np.asarray(m, F)
    x, y, z = pt[0], pt[1], pt[2]
    q = []
    with np.errstate(all="ignore"):
        for r in range(3):
            if order == 0:
                q.append(F(F(x * m[r, 0]) + F(F(y * m[r, 1]) + F(F(z * m[r, 2]) + m[r, 3]))))
            else:
                q.append(F(F(F(F(m[r, 0] * x) + F(m[r, 1] * y)) + F(m[r, 2] * z)) + m[r, 3]))
    return (q[0], q[1], q[2], F(1))


def clouds_scalar(items, transforms=None, params=None):
    p = dict(DEFAULTS, **(params or {}))
    mats = _matrices(len(items), transforms)
    pts, offsets, flat = [], [0], 0
    for i, it in enumerate(items):
        for j, l in enumerate(lines_array(it)):
            got = interpolate_scalar(l[0], l[1], p)
            if got is None:
                raise TooLong(i, j, flat)
            pts += got if mats[i] is None else [transform_scalar(q, mats[i], p["transform_order"]) for q in got]
            flat += 1
        offsets.append(len(pts))
    return np.array(pts, F).reshape(-1, 4), np.array(offsets, np.int64)


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def same_bits(got, want):
    """bit patterns equal; NaN positions equal, payloads free"""
    got, want = np.ascontiguousarray(got, F), np.ascontiguousarray(want, F)
    if got.shape != want.shape:
        return False
    gn, wn = np.isnan(got), np.isnan(want)
    return bool(np.array_equal(gn, wn) and np.array_equal(bits(got)[~gn], bits(want)[~wn]))


def building_transform(pose, estimate):
    """building.cpp:11-15 written out entry by entry in double, then transform2Dto3D in float32"""
    P, E = np.asarray(pose, np.float64), np.asarray(estimate, np.float64)
    r00, r01, r10, r11 = P[0, 0], P[1, 0], P[0, 1], P[1, 1]                      # the inverse's rotation: the transpose
    ix, iy = -(r00 * P[0, 2] + r01 * P[1, 2]), -(r10 * P[0, 2] + r11 * P[1, 2])
    t = np.eye(3)
    t[0, 0], t[0, 1] = r00 * E[0, 0] + r01 * E[1, 0], r00 * E[0, 1] + r01 * E[1, 1]
    t[1, 0], t[1, 1] = r10 * E[0, 0] + r11 * E[1, 0], r10 * E[0, 1] + r11 * E[1, 1]
    t[0, 2] = (r00 * E[0, 2] + r01 * E[1, 2]) + ix
    t[1, 2] = (r10 * E[0, 2] + r11 * E[1, 2]) + iy
    t[0, 2] += P[0, 2] - (t[0, 0] * P[0, 2] + t[0, 1] * P[1, 2])
    t[1, 2] += P[1, 2] - (t[1, 0] * P[0, 2] + t[1, 1] * P[1, 2])
    t = t.astype(F)
    ang = F(np.arctan2(t[1, 0], t[0, 0]))
    c, s = F(np.cos(ang)), F(np.sin(ang))
    out = np.eye(4, dtype=F)
    out[0, 0], out[0, 1], out[1, 0], out[1, 1] = c, -s, s, c
    out[0, 3], out[1, 3] = t[0, 2], t[1, 2]
    return out
