"""Inputs of the building cloud tests, shared by the CPU and the GPU files.  A case is dict(items=[float64 [L, 2, 3] per item],
transforms=None | one 4 x 4 | a list with a 4 x 4 or None per item, params={...}); `reference(name)` is the vectorised restatement's
result, computed once per process."""
import os
import re

import numpy as np

import building_cloud_reference as R

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the fill kernel's tile as the header states it; the GPU tests take it from the library's counts hook and compare
TILE = int(re.search(r"#define DGS_BC_TILE (\d+)", open(os.path.join(ROOT, "include", "dgs_reg.h")).read()).group(1))
BOUNDARY_KS = (0, 1, 5, 50, 255, 256, 257, TILE - 1, TILE, TILE + 1)

# found by a seeded search over random float32 end points (50 m box, lines up to 52 m): (x² + y²) + z² and (x² + z²) + y² round to
# different norms here, and the two norms lie on either side of a sample position: 2,100 points under orders 0 and 2, 2,099 under 1
SQNORM_LINE = np.array([[23.898122787475586, -42.0658073425293, 35.80266571044922],
                        [49.2385139465332, -65.32461547851562, 11.734485626220703]], np.float64)


def line(a, b):
    return np.array([[a, b]], np.float64)


def below(v):
    return float(np.nextafter(F(v), F(-np.inf)))


def above(v):
    return float(np.nextafter(F(v), F(np.inf)))


def case(items, transforms=None, **params):
    return dict(items=[np.ascontiguousarray(i, np.float64).reshape(-1, 2, 3) for i in items], transforms=transforms, params=params)


# ---- count boundary ---------------------------------------------------------------------------------------------------------
def boundary(k):
    """axis-aligned lines of length table[k] exactly, the float below it and the float above it -> k + 1, k and k + 1 points
    (k = 0: no length below zero, that line is left out)"""
    v = float(R.step_table(k + 2)[k])
    lengths = [v, above(v)] if k == 0 else [v, below(v), above(v)]
    return case([line((0.0, 0.0, 0.0), (l, 0.0, 0.0)) for l in lengths]), [k + 1, k + 1] if k == 0 else [k + 1, k, k + 1]


# ---- offsets across workgroups ------------------------------------------------------------------------------------------------
def short_lines(n_lines, seed):
    """n_lines lines of one to three points at random places and angles"""
    rng = np.random.default_rng(seed)
    a = rng.uniform(-200.0, 200.0, (n_lines, 3))
    a[:, 2] = 0.0
    ang = rng.uniform(0.0, 2.0 * np.pi, n_lines)
    length = rng.choice([0.005, 0.03, 0.05], n_lines)
    b = a + np.stack([length * np.cos(ang), length * np.sin(ang), np.zeros(n_lines)], axis=1)
    return np.stack([a, b], axis=1)


def many_items(n_lines, seed=0):
    """the lines dealt to items of 0 .. 40 lines; items without lines first, in the middle and last"""
    rng = np.random.default_rng(100 + seed)
    lines = short_lines(n_lines, seed)
    items, at = [lines[:0]], 0
    while at < n_lines:
        n = int(min(rng.integers(0, 41), n_lines - at))
        items.append(lines[at:at + n])
        at += n
        if len(items) == 20:
            items.append(lines[:0])
            items.append(lines[:0])
    items.append(lines[:0])
    return case(items)


# ---- owner search at tile starts -------------------------------------------------------------------------------------------------
def owner_search(shift):
    """TILE + shift one-point lines, one 100 m line (5,001 points), 300 one-point lines: the long line begins one point before (shift -1),
    at (0) and one point after (1) a tile start, and ends inside a later tile"""
    before = np.zeros((TILE + shift, 2, 3))
    before[:, :, 0] = np.arange(TILE + shift)[:, None]
    after = np.zeros((300, 2, 3))
    after[:, :, 1] = -1.0 - np.arange(300)[:, None]
    long = line((3.0, 4.0, 0.0), (3.0 + 60.0, 4.0 + 80.0, 0.0))
    return case([before[:700], np.concatenate([before[700:], long, after[:10]]), after[10:]])


# ---- arithmetic ------------------------------------------------------------------------------------------------------------------
def arithmetic():
    rng = np.random.default_rng(7)
    diag = []
    for deg in (0.001, 29.7, 45.0, 89.999, 123.4, 180.0, 269.9, 333.3):
        t = np.deg2rad(deg)
        a = rng.uniform(-5.0, 5.0, 2)
        diag.append([[a[0], a[1], 0.0], [a[0] + 13.7 * np.cos(t), a[1] + 13.7 * np.sin(t), 0.0]])
    far = [[[100.013, -80.007, 0.0], [103.51, -77.77, 0.0]], [[99.99, -79.99, 0.0], [100.01, -80.01, 0.0]],
           [[100.0 + 1e-5, -80.0, 0.0], [100.0, -80.0 - 1e-5, 0.0]]]
    tall = [[[1.0, 2.0, 3.0], [4.0, 6.0, -9.0]], [[0.0, 0.0, 10.0], [0.0, 0.0, -10.0]], [[-1.5, 2.5, 0.25], [7.0, 2.5, 0.5]]]
    signed = [[[-0.0, 1.0, 0.0], [-0.0, 3.0, 0.0]], [[2.0, -0.0, 0.0], [-2.0, -0.0, 0.0]], [[-0.0, -0.0, -0.0], [-0.0, -0.0, -0.0]],
              [[-0.0, 1.0, 0.0], [-2.0, 1.0, 0.0]]]
    return case([np.array(diag), np.array(far), np.array(tall), np.array(signed)])


def sqnorm(order):
    return case([SQNORM_LINE[None]], sqnorm_order=order)


def zero_length(guard):
    return case([line((3.25, -7.5, 1.0), (3.25, -7.5, 1.0))], normalized_guard=guard)


# ---- bad input -----------------------------------------------------------------------------------------------------------------
def nan_endpoint():
    """the NaN line, and a line with a NaN z alone, give no points; their neighbours are served"""
    ok = [[0.0, 0.0, 0.0], [0.05, 0.0, 0.0]]
    return case([np.array([ok, [[np.nan, 0.0, 0.0], [1.0, 0.0, 0.0]], ok]), np.array([[[0.0, 0.0, np.nan], [1.0, 1.0, 0.0]]]), np.array([ok])])


def infinite_endpoint():
    ok = [[0.0, 0.0, 0.0], [0.05, 0.0, 0.0]]
    return case([np.array([ok]), np.array([ok, ok, [[0.0, 0.0, 0.0], [np.inf, 0.0, 0.0]], ok])]), (1, 2)


def past_the_table(max_points=64):
    """with max_points_per_line = 64 the table ends at entry 63: that length is served with 64 points, the next float is refused"""
    v = float(R.step_table(max_points)[max_points - 1])
    ok = case([line((0.0, 0.0, 0.0), (v, 0.0, 0.0))], max_points_per_line=max_points)      # from the origin: the difference is v exactly
    bad = case([line((0.0, 0.0, 0.0), (0.01, 0.0, 0.0)), np.array([[[0.0, 0.0, 0.0], [0.01, 0.0, 0.0]], [[0.0, 0.0, 0.0], [above(v), 0.0, 0.0]]])],
               max_points_per_line=max_points)
    return ok, bad, (1, 1)


# ---- transforms ------------------------------------------------------------------------------------------------------------------
def rigid(deg, tx, ty):
    t = np.deg2rad(deg)
    m = np.eye(4, dtype=F)
    m[0, 0], m[0, 1], m[1, 0], m[1, 1] = np.cos(t), -np.sin(t), np.sin(t), np.cos(t)
    m[0, 3], m[1, 3] = tx, ty
    return m


def outline(cx, cy, w, h, deg=0.0):
    """a closed rectangle outline as four lines, as buildPointCloud makes them from five nodes"""
    t = np.deg2rad(deg)
    c = np.array([[-w, -h], [w, -h], [w, h], [-w, h], [-w, -h]]) / 2.0
    c = c @ np.array([[np.cos(t), np.sin(t)], [-np.sin(t), np.cos(t)]]) + [cx, cy]
    p = np.concatenate([c, np.zeros((5, 1))], axis=1)
    return np.stack([p[:-1], p[1:]], axis=1)


def transforms(kind, order=0):
    items = [outline(10.0, 5.0, 8.0, 6.0, 12.0), outline(-30.0, 40.0, 12.5, 7.25, 77.0), np.zeros((0, 2, 3)), outline(2.0, -3.0, 1.0, 1.0),
             np.array([[[-0.0, 1.0, 0.0], [-2.0, 1.0, 0.0]]])]      # its first point is (-0.0, 1): 0 * dn.x is -0 and -0 + -0 stays -0
    skew = rigid(31.0, -4.0, 9.0)
    skew[2, 0], skew[2, 1], skew[2, 3], skew[0, 2] = 0.25, -0.5, 1.5, 3.0      # z picks up x and y; the column of z meets z = 0
    nan = rigid(5.0, 1.0, 2.0)
    nan[1, 1] = np.nan
    inf_z = rigid(5.0, 1.0, 2.0)
    inf_z[0, 2] = np.inf                                                        # 0 * inf: NaN in x alone
    t = dict(none=None, shared=rigid(17.0, 100.0, -80.0), identity=np.eye(4, dtype=F),
             per_item=[rigid(17.0, 100.0, -80.0), None, np.eye(4, dtype=F), skew, np.eye(4, dtype=F)],
             nan=[nan, None, None, inf_z, None])[kind]
    return case(items, t, transform_order=order)


# ---- handle reuse ----------------------------------------------------------------------------------------------------------------
def short_call():
    return case([outline(0.0, 0.0, 4.0, 3.0, 30.0), outline(9.0, 9.0, 2.0, 2.0)], rigid(3.0, 1.0, 1.0))


def growing_call():
    """a 300 m line: past the 4,096 entries (81.9 m) a table starts with"""
    return case([outline(0.0, 0.0, 4.0, 3.0), line((-150.0, 2.0, 0.0), (150.0, 2.5, 0.0))])


def random_lines(n=200, seed=5):
    """lengths 0 - 60 m, random directions, z != 0"""
    rng = np.random.default_rng(seed)
    a = rng.uniform(-100.0, 100.0, (n, 3))
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    b = a + d * rng.uniform(0.0, 60.0, n)[:, None]
    return np.stack([a, b], axis=1)


def named_cases():
    """every case that has a result (no error), by name"""
    c = {}
    for k in BOUNDARY_KS:
        c[f"boundary_{k}"] = boundary(k)[0]
    for n in (1023, 1024, 1025, 2049):
        c[f"many_items_{n}"] = many_items(n)
    c["no_items"] = case([])
    c["one_zero_length"] = zero_length(1)
    c["zero_length_unguarded"] = zero_length(0)
    for s in (-1, 0, 1):
        c[f"owner_{s}"] = owner_search(s)
    c["arithmetic"] = arithmetic()
    for o in (0, 1, 2):
        c[f"sqnorm_{o}"] = sqnorm(o)
    c["nan_endpoint"] = nan_endpoint()
    c["table_end_64"] = past_the_table()[0]
    for kind in ("none", "shared", "identity", "per_item", "nan"):
        for order in (0, 1):
            c[f"transform_{kind}_{order}"] = transforms(kind, order)
    c["short_call"] = short_call()
    c["growing_call"] = growing_call()
    return c


_refs = {}


def reference(name, c=None):
    if name not in _refs:
        c = c or named_cases()[name]
        pts, off = R.clouds(c["items"], c["transforms"], c["params"])
        pts.setflags(write=False)
        off.setflags(write=False)
        _refs[name] = (pts, off)
    return _refs[name]
