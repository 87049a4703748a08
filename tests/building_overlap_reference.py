"""numpy float64 restatement of are_buildings_overlapped (upstream include/hdl_graph_slam/check_overlapping.hpp), getOverlappedBuildings
(apps/delta_graph_slam_nodelet.cpp:767-787) and LineBasedScanmatcher::align_overlapped_buildings (src/hdl_graph_slam/
line_based_scanmatcher.cpp:29-107, from the building-frame lines on), written from the upstream source on the primitives of
tests/line_align_reference.py (Trig, edge_extraction, align_edges, gate_angle, transform_lines) and independent of the library's
headers.  Lines are float64 arrays [L, 2, 3] (pointA, pointB); a building is such an array and a centre.

The pair search has no trigonometry: its result is exact.  The alignment goes through `Trig(seed)`: seed None is numpy's arctan2 / sin /
cos, a seed nudges every result by one ulp up or down, which is how TOL_OVERLAP and the unstable hypotheses are measured."""
import numpy as np

import line_align_reference as R

GATE_PASS, GATE_ANGLE, GATE_OVERLAP = 0, 3, 7
MAX_ANGLE = np.pi / 3.0
SHRINK = 0.99
DBL_MAX = R.DBL_MAX


# ---- check_overlapping.hpp -----------------------------------------------------------------------------------------------------------
def shrink(lines, center):
    """shrink_polygon (:51-70): center + 0.99 * (point - center) per coordinate; x and y only.  lines [..., 2, 3] -> [..., 2, 2]"""
    c = np.asarray(center, np.float64)[..., :2]
    return c + SHRINK * (np.asarray(lines, np.float64)[..., :2] - c)


def lines_intersected(l1, l2):
    """are_lines_intersected (:24-49) with is_point_on_the_line (:10-22) over broadcast shapes [..., 2, 2] -> bool"""
    x11, y11, x12, y12 = l1[..., 0, 0], l1[..., 0, 1], l1[..., 1, 0], l1[..., 1, 1]
    x21, y21, x22, y22 = l2[..., 0, 0], l2[..., 0, 1], l2[..., 1, 0], l2[..., 1, 1]
    a1 = y12 - y11
    b1 = x11 - x12
    c1 = a1 * x11 + b1 * y11
    a2 = y22 - y21
    b2 = x21 - x22
    c2 = a2 * x21 + b2 * y21
    det = a1 * b2 - a2 * b1
    ok = det != 0
    with np.errstate(all="ignore"):
        sd = np.where(ok, det, 1.0)
        x = (b2 * c1 - b1 * c2) / sd
        y = (a1 * c2 - a2 * c1) / sd
    on1 = ((x < x11) != (x < x12)) | ((y < y11) != (y < y12))
    on2 = ((x < x21) != (x < x22)) | ((y < y21) != (y < y22))
    return ok & on1 & on2


def buildings_overlapped(a, ca, b, cb):
    """are_buildings_overlapped (:97-114)"""
    sa, sb = shrink(a, ca), shrink(b, cb)
    if sa.shape[0] == 0 or sb.shape[0] == 0:
        return False
    return bool(lines_intersected(sa[:, None], sb[None, :]).any())


def overlapped_pairs(buildings, centers):
    """getOverlappedBuildings: every i < j with are_buildings_overlapped, i ascending then j ascending -> int32 [P, 2]"""
    B = len(buildings)
    centers = np.asarray(centers, np.float64).reshape(B, 3)
    shr = [shrink(np.asarray(b, np.float64).reshape(-1, 2, 3), centers[i]) for i, b in enumerate(buildings)]
    off = np.concatenate([[0], np.cumsum([s.shape[0] for s in shr])]).astype(np.int64)
    allb = np.concatenate(shr) if B and off[-1] else np.zeros((0, 2, 2))
    out = []
    for i in range(B):
        if shr[i].shape[0] == 0 or i + 1 >= B:
            continue
        rest = allb[off[i + 1]:]
        hit = lines_intersected(shr[i][:, None], rest[None, :]).any(axis=0)
        cs = np.concatenate([[0], np.cumsum(hit)])
        o = off[i + 1:] - off[i + 1]
        flag = (cs[o[1:]] - cs[o[:-1]]) > 0
        out += [(i, i + 1 + int(j)) for j in np.nonzero(flag)[0]]
    return np.array(out, np.int32).reshape(-1, 2)


# ---- align_overlapped_buildings --------------------------------------------------------------------------------------------------------
def align_lines(T, l1, l2):
    """align_lines (:742-767) over arrays: l1, l2 = (pointA, pointB) tuples of vectors -> rotation (4 arrays), translation (3 arrays)"""
    a1, b1 = l1
    a2, b2 = l2
    angle = R._angle_between(T, R._sub(a1, b1), R._sub(a2, b2))
    angle = np.where(angle > np.pi / 2, angle - np.pi, np.where(angle < -np.pi / 2, angle + np.pi, angle))
    d = R._normalized(R._sub(a2, b2))
    proj = R._add(a2, R._scale(d, R._dot(R._sub(a1, a2), d)))
    r = R._rot_z(T, angle)
    t = R._sub(proj, R._rotate(r, a1))
    return r, t


def align_overlapped(src, trg, center_source=(0.0, 0.0, 0.0), center_target=(0.0, 0.0, 0.0), float_chain=1, seed=None, batch=256):
    """-> dict: edges_source, edges_target, per-hypothesis gate, rot1 (edge pairs), rotation, translation, tn; winner, transformation,
    translation_norm, aligned_lines, n_edge, n_line, n_angle_passed, n_not_overlapped, is_identity.  Hypothesis h = es * Et + et, then
    Es * Et + i * Lt + j.  Every angle-passing hypothesis gets its overlap test; upstream skips it when the norm is no better already."""
    T = R.Trig(seed)
    src = np.asarray(src, np.float64).reshape(-1, 2, 3)
    trg = np.asarray(trg, np.float64).reshape(-1, 2, 3)
    es, et = R.edge_extraction(src), R.edge_extraction(trg)
    Es, Et, Ls, Lt = es.shape[0], et.shape[0], src.shape[0], trg.shape[0]
    n_edge, n_line = Es * Et, Ls * Lt
    with np.errstate(all="ignore"):
        a, b = np.repeat(np.arange(Es), Et), np.tile(np.arange(Et), Es)
        r1, t1, first = R.align_edges(T, tuple(R._v(es[a, k]) for k in range(3)), tuple(R._v(et[b, k]) for k in range(3)))
        i, j = np.repeat(np.arange(Ls), Lt), np.tile(np.arange(Lt), Ls)
        r2, t2 = align_lines(T, (R._v(src[i, 0]), R._v(src[i, 1])), (R._v(trg[j, 0]), R._v(trg[j, 1])))
        bc = lambda v, n: [np.broadcast_to(np.asarray(c, np.float64), (n,)) for c in v]
        rot = np.concatenate([np.stack(bc(r1, n_edge), 1).reshape(-1, 4), np.stack(bc(r2, n_line), 1).reshape(-1, 4)])
        tr = np.concatenate([np.stack(bc(t1, n_edge), 1).reshape(-1, 3), np.stack(bc(t2, n_line), 1).reshape(-1, 3)])
        tn = R._norm(R._v(tr))
        H = n_edge + n_line
        gate = np.full(H, GATE_ANGLE, np.int32)
        if H:
            ang = R.gate_angle(T, tuple(rot[:, k] for k in range(4)), float_chain)
            gate[T.cos(ang) > np.cos(MAX_ANGLE)] = GATE_PASS
        passed = np.nonzero(gate == GATE_PASS)[0]
        target = shrink(trg, center_target)
        for b0 in range(0, passed.size, batch):
            hs = passed[b0:b0 + batch]
            moved = shrink(R.transform_lines(src, rot[hs], tr[hs]), center_source)       # the source centre is not moved
            hit = lines_intersected(moved[:, :, None], target[None, None, :]).any(axis=(1, 2))
            gate[hs[hit]] = GATE_OVERLAP
    winner, best = -1, DBL_MAX
    for h in np.nonzero(gate == GATE_PASS)[0]:            # strict < in h order from DBL_MAX; a NaN compares false
        if tn[h] < best:
            winner, best = int(h), float(tn[h])
    if winner >= 0:
        Tm = R._mat(rot[winner], tr[winner])
        aligned = R.transform_lines(src, rot[winner][None], tr[winner][None])[0]
    else:
        Tm = np.eye(4)
        aligned = src.copy()
    return dict(edges_source=es, edges_target=et, gate=gate, rot1=np.asarray(first).reshape(-1), rotation=rot, translation=tr, tn=tn, winner=winner,
                transformation=Tm, translation_norm=best, aligned_lines=aligned, n_edge=n_edge, n_line=n_line,
                n_angle_passed=int(np.count_nonzero(gate != GATE_ANGLE)), n_not_overlapped=int(np.count_nonzero(gate == GATE_PASS)),
                is_identity=bool(np.array_equal(Tm, np.eye(4))))


def _spread(x, y):
    x, y = np.asarray(x, np.float64).ravel(), np.asarray(y, np.float64).ravel()
    same = (x == y) | (np.isnan(x) & np.isnan(y))
    with np.errstate(all="ignore"):
        return float(np.max(np.where(same, 0.0, np.abs(x - y)), initial=0.0))


def compare_runs(a, b):
    """Two runs of one item (plain and nudged trigonometry) -> (unstable h, spread per hypothesis, spread of the final record).  A
    hypothesis is unstable when its gate or its rot1 / rot2 choice differs.  Transforms and norms are compared for the hypotheses that
    pass the angle gate: behind the gate, perpendicular walls sit on align_lines' wrap at +-pi / 2, where one ulp turns the rotation by
    180 degrees and the gate code stays ANGLE either way."""
    un = a["gate"] != b["gate"]
    un[:a["n_edge"]] |= (a["rot1"] != b["rot1"]) & (a["gate"][:a["n_edge"]] != GATE_ANGLE)
    ok = ~un & (a["gate"] != GATE_ANGLE)
    s_hyp = max(_spread(a[k][ok], b[k][ok]) for k in ("tn", "rotation", "translation"))
    s_final = max(_spread(a[k], b[k]) for k in ("transformation", "aligned_lines", "translation_norm"))
    return np.nonzero(un)[0], s_hyp, s_final


def margin(r):
    """The smallest norm among passing hypotheses that move differently from the winner, minus the winner's (inf when there is none)."""
    if r["winner"] < 0:
        return np.inf
    w = r["winner"]
    s = np.nonzero(r["gate"] == GATE_PASS)[0]
    other = s[np.any(r["rotation"][s] != r["rotation"][w], axis=1) | np.any(r["translation"][s] != r["translation"][w], axis=1)]
    tn = r["tn"][other]
    tn = tn[~np.isnan(tn)]
    return float(tn.min() - r["tn"][w]) if tn.size else np.inf


def own_rule_winner(gate, tn):
    """The rule on a set of hypothesis records: the lowest h among the smallest norms with gate PASS (-1: none)."""
    ok = (gate == GATE_PASS) & (tn < DBL_MAX)
    if not ok.any():
        return -1
    return int(np.nonzero(ok & (tn == tn[ok].min()))[0][0])


# ---- builders --------------------------------------------------------------------------------------------------------------------------
rectangle, move, seg = R.rectangle, R.move, R.seg
NONE = np.zeros((0, 2, 3))


def polygon(pts):
    pts = np.asarray(pts, np.float64)
    n = pts.shape[0]
    return np.array([seg(*pts[k], *pts[(k + 1) % n]) for k in range(n)], np.float64)


def l_shape(cx, cy, w, h, nw, nh, angle=0.0):
    """A w x h rectangle with an nw x nh notch cut from its upper right corner, rotated about its centre: six walls."""
    p = np.array([[0, 0], [w, 0], [w, h - nh], [w - nw, h - nh], [w - nw, h], [0, h]], np.float64) - [w / 2, h / 2]
    c, s = np.cos(angle), np.sin(angle)
    return polygon(p @ np.array([[c, s], [-s, c]]) + [cx, cy])


def ngon(cx, cy, radius, n, phase=0.0):
    a = phase + 2 * np.pi * np.arange(n) / n
    return polygon(np.stack([cx + radius * np.cos(a), cy + radius * np.sin(a)], 1))


def fence(n, x0, y0, pitch, length, slope=0.0, cross=True):
    """n parallel pickets (no edges among themselves) and, with `cross`, one rail across them in place of the last picket."""
    out = [seg(x0 + pitch * k, y0 + slope * k, x0 + pitch * k + 0.05 * k / n, y0 + slope * k + length) for k in range(n - (1 if cross else 0))]
    if cross:
        out.append(seg(x0 - 1.5, y0 + 0.31 * length, x0 + pitch * n + 1.5, y0 + 0.33 * length))
    return np.array(out, np.float64)


def centroid(lines):
    lines = np.asarray(lines, np.float64).reshape(-1, 2, 3)
    return lines.reshape(-1, 3).mean(axis=0) * [1, 1, 0] if lines.size else np.zeros(3)


_CACHE = {}


def _city(B, seed, pitch=14.0, jitter=2.6):
    """B buildings (rectangles and L-shapes) on a jittered grid; neighbours overlap now and then."""
    rng = np.random.default_rng(seed)
    side = int(np.ceil(np.sqrt(B)))
    bl, ce = [], []
    for k in range(B):
        cx, cy = pitch * (k % side) + rng.uniform(-jitter, jitter), pitch * (k // side) + rng.uniform(-jitter, jitter)
        w, h, ang = rng.uniform(7, 11.5), rng.uniform(6, 11.5), rng.uniform(0, np.pi)
        b = rectangle(cx, cy, w, h, ang) if rng.integers(0, 3) else l_shape(cx, cy, w, h, 0.4 * w, 0.45 * h, ang)
        bl.append(b)
        ce.append([cx + rng.uniform(-0.5, 0.5), cy + rng.uniform(-0.5, 0.5), 0.0])
    return bl, np.array(ce, np.float64).reshape(B, 3)


def pair_scenes():
    """name -> (list of buildings' lines, centres [B, 3])"""
    if "pairs" in _CACHE:
        return _CACHE["pairs"]
    sc = {}
    box = rectangle(0, 0, 10, 6)
    sc["b0"] = ([], np.zeros((0, 3)))
    sc["b1"] = ([box], np.zeros((1, 3)))
    sc["b2"] = ([box, rectangle(6, 2, 10, 6)], np.array([[0, 0, 0], [6, 2, 0.0]]))
    # 0 lines, 1 line, 65 lines against 3: the triangle crosses only the last walls of the 65-gon, so the hit is past lane 63
    gon = ngon(40, 0, 10, 65)
    far = gon[60, 0]
    tri = polygon([far[:2] * [1, 1] + [-1.5, -1.0], far[:2] + [2.5, -0.5], far[:2] + [0.5, -3.0]])
    sc["odd_sizes"] = ([NONE, np.array([seg(-2, -8, 3, 8)]), gon, tri, box, NONE],
                       np.array([[0, 0, 0], [0.5, 0, 0], [40, 0, 0], centroid(tri), [0, 0, 0], [5, 5, 0]], np.float64))
    sc["shared_wall"] = ([box, rectangle(10, 0, 10, 6)], np.array([[0, 0, 0], [10, 0, 0.0]]))
    sc["crossing"] = ([box, rectangle(3, 2, 4, 12)], np.array([[0, 0, 0], [3, 2, 0.0]]))
    sc["inside"] = ([box, rectangle(0.5, 0.2, 3, 2)], np.array([[0, 0, 0], [0.5, 0.2, 0.0]]))
    sc["collinear"] = ([np.array([seg(0, 0, 10, 0)]), np.array([seg(4, 0, 16, 0)]), np.array([seg(2, 1, 12, 1), seg(2, 0, 8, 0)])],
                       np.array([[5, 0, 0], [10, 0, 0], [7, 0, 0.0]]))
    # axis-aligned walls: one extent is empty, the other decides.  The plus crosses, the T's bar ends 2 m short of the stem
    sc["axis_aligned"] = ([np.array([seg(-5, 0, 5, 0)]), np.array([seg(0, -5, 0, 5)]), np.array([seg(7, -5, 7, 5)])],
                          np.array([[0, 0, 0], [0, 0, 0], [7, 0, 0.0]]))
    sc["clique24"] = ([rectangle(0.3 * np.cos(k), 0.3 * np.sin(k), 30, 1.0, np.pi * k / 24) for k in range(24)],
                      np.array([[0.3 * np.cos(k), 0.3 * np.sin(k), 0] for k in range(24)], np.float64))
    sc["grid65"] = _city(65, 65)
    bl, ce = _city(129, 129)
    ce[128] = ce[63] + [3.0, 2.0, 0.0]                       # the last building onto building 63: a pair whose j is the first bit of the third word
    bl[128] = rectangle(ce[128][0], ce[128][1], 9, 8, 0.3)
    sc["grid129"] = (bl, ce)
    sc["random300"] = _city(300, 300, pitch=13.0, jitter=4.0)
    _CACHE["pairs"] = sc
    return sc


def pair_result(name):
    k = ("pairs", name)
    if k not in _CACHE:
        _CACHE[k] = overlapped_pairs(*pair_scenes()[name])
    return _CACHE[k]


def _turned(item, angle):
    """The whole item turned about the origin: nothing stays axis-parallel, so no angle is an exact multiple of pi / 2."""
    s, t, cs, ct = item
    c, sn = np.cos(angle), np.sin(angle)
    return (move(s, 0, 0, angle), move(t, 0, 0, angle), np.array([c * cs[0] - sn * cs[1], sn * cs[0] + c * cs[1], 0.0]),
            np.array([c * ct[0] - sn * ct[1], sn * ct[0] + c * ct[1], 0.0]))


def _mixed_item(k):
    """A rectangle (odd k) or an L-shape (even k) against a turned rectangle that overlaps it"""
    rng = np.random.default_rng(1000 + k)
    ang, dx, dy = rng.uniform(-0.4, 0.4), rng.uniform(5, 8), rng.uniform(-4, 4)
    s = rectangle(0, 0, rng.uniform(8, 12), rng.uniform(5, 9)) if k % 2 else l_shape(0, 0, 11, 9, 4.5, 4, rng.uniform(-0.2, 0.2))
    t = rectangle(dx, dy, rng.uniform(6, 10), rng.uniform(6, 10), ang)
    return _turned((s, t, np.zeros(3), np.array([dx + 0.1, dy - 0.1, 0.0])), 0.05 + 0.01 * k)


def align_scenes():
    """name -> (source lines, target lines, center_source, center_target), in the source building's frame"""
    if "align" in _CACHE:
        return _CACHE["align"]
    sc = {}
    Z = np.zeros(3)
    a = rectangle(0, 0, 10, 6)
    b = rectangle(8.5, 4.0, 9, 7)
    # the minimal move is unique: the right wall onto the target's left wall, 1 m; 8.5 cm of clearance after it, 1 m of overlap before
    sc["offset_rects"] = _turned((a, b, Z, np.array([8.5, 4.0, 0])), 0.2)
    sc["rotated_rects"] = (a, rectangle(7.4, 3.2, 9, 7, np.deg2rad(12)), Z, np.array([7.6, 3.1, 0]))
    sc["l_shape"] = (l_shape(0, 0, 12, 9, 5, 4, np.deg2rad(8)), rectangle(6.2, 5.1, 8, 6, np.deg2rad(-5)), Z, np.array([6.0, 5.0, 0]))
    sc["edge_pair_winner"] = _mixed_item(EDGE_WINNER_ITEM)
    sc["one_line_source"] = (np.array([seg(-6, 1, 7, 2)]), rectangle(5, 1, 6, 5, np.deg2rad(20)), Z, np.array([5, 1, 0.0]))
    sc["empty_source"] = (NONE, b, Z, np.array([8.5, 4.0, 0]))
    sc["empty_target"] = (a, NONE, Z, np.array([8.5, 4.0, 0]))
    sc["all_angle_gated"] = (np.array([seg(-5, 0, 5, 0), seg(-5, 2, 5, 2.1)]), move(np.array([seg(-4, 0, 4, 0), seg(-4, 1.5, 4, 1.4)]), 1, 1, np.deg2rad(75)),
                             Z, np.array([1, 1, 0.0]))
    # a 3 x 3 mesh of 60 m lines, 6 m and 5 m apart, and two diagonals, over a 9 m x 7 m rectangle: wherever a hypothesis puts it,
    # another line cuts through
    mesh = np.array([seg(-30, y, 30, y + 0.2) for y in (-5, 0, 5)] + [seg(x, -30, x - 0.25, 30) for x in (-6, 0, 6)] +
                    [seg(-30, -29, 30, 31), seg(-30, 29.5, 30, -30.5)])
    sc["all_overlapped"] = (mesh, rectangle(0.3, 0.2, 9, 7, np.deg2rad(4)), Z, np.array([0.4, 0.1, 0]))
    sc["line_pair_winner"] = (a, rectangle(5.6, 0.4, 3, 14, np.deg2rad(3)), Z, np.array([5.5, 0.5, 0]))
    sc["fences65"] = (fence(65, -10, -3, 0.33, 6.0, cross=False), move(fence(65, -9, -2, 0.3, 5.0, slope=0.01, cross=False), 0.5, 0.4, np.deg2rad(6)),
                      Z, np.array([0.5, 0.5, 0]))
    # two equal squares on the diagonal: the moves along the two axes are rivals of (nearly) equal norm, and every target wall is there
    # twice, so every hypothesis on it has a twin of bit-equal norm at a higher h
    sq = rectangle(0, 0, 8, 8)
    tw = rectangle(6, 6, 8, 8)
    sc["symmetric_squares"] = _turned((sq, np.concatenate([tw, tw]), Z, np.array([6.0, 6.0, 0])), 0.3)
    _CACHE["align"] = sc
    return sc


EDGE_WINNER_ITEM = 30


def batch_mixed():
    """33 items: every scene, then rectangles and L-shapes against their neighbours, with an empty and a no-edge item in between"""
    if "batch" in _CACHE:
        return _CACHE["batch"]
    sc = align_scenes()
    items = [sc[n] for n in sc]
    while len(items) < 33:
        k = len(items)
        it = _mixed_item(k)
        if k == 16:
            it = (NONE,) + it[1:]
        if k == 20:
            it = (np.array([seg(-4, 0.5, 6, 0.2)]), np.array([seg(3, -4, 3.5, 5)])) + it[2:]       # no edge on either side
        items.append(it)
    _CACHE["batch"] = items
    return items


def cached(key, item, seed=None):
    k = ("align", key, seed)
    if k not in _CACHE:
        _CACHE[k] = align_overlapped(*item, seed=seed)
    return _CACHE[k]


def scene_result(name, seed=None):
    return cached(name, align_scenes()[name], seed)


def batch_result(b, seed=None):
    return cached(("batch", b), batch_mixed()[b], seed)


# ---- files for tests/cpp/building_overlap_driver.cpp -----------------------------------------------------------------------------------
def write_buildings(path, buildings, centers):
    off = np.concatenate([[0], np.cumsum([np.asarray(b).reshape(-1, 2, 3).shape[0] for b in buildings])]).astype(np.int64)
    with open(path, "wb") as f:
        np.array([len(buildings)], np.int64).tofile(f)
        off.tofile(f)
        for b in buildings:
            np.asarray(b, np.float64).tofile(f)
        np.asarray(centers, np.float64).reshape(-1, 3).tofile(f)


def write_items(path, items):
    so = np.concatenate([[0], np.cumsum([it[0].shape[0] for it in items])]).astype(np.int64)
    to = np.concatenate([[0], np.cumsum([it[1].shape[0] for it in items])]).astype(np.int64)
    with open(path, "wb") as f:
        np.array([len(items)], np.int64).tofile(f)
        so.tofile(f)
        to.tofile(f)
        for it in items:
            np.asarray(it[0], np.float64).tofile(f)
        for it in items:
            np.asarray(it[1], np.float64).tofile(f)
        np.array([it[2] for it in items], np.float64).reshape(-1, 3).tofile(f)
        np.array([it[3] for it in items], np.float64).reshape(-1, 3).tofile(f)
