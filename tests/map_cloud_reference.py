"""numpy restatement of MapCloudGenerator::generate (src/hdl_graph_slam/map_cloud_generator.cpp:13-50) over PCL 1.10's
pcl::octree::OctreePointCloud, float32 / float64 operation for operation.

Two implementations of the octree part:
  generate()          the closed form: growth replay (adoptBoundingBoxToPoint over the points in order) -> per point the key under the
                      box of its insertion, moved by the later growths -> unique -> ascending bit-interleaved key -> centres;
  generate_literal()  a pointer octree: every point inserted one by one, a new root on each growth, leaves created by the key's
                      bits from the top, and a depth-first walk over child indices 0..7.
The switches are the ABI's (dgs_map_cloud_params): same names, 1 = as recalled from PCL 1.10.
"""
from __future__ import annotations

import math

import numpy as np

F = np.float32
FLT_EPSILON = float(np.finfo(np.float32).eps)   # const float minValue = std::numeric_limits<float>::epsilon(), promoted to double
MAX_DEPTH = 21                                  # 3 x 21 key bits in a 64-bit word
FIRST_BOX_OVERSIZE = 1
GROW_SHIFT_WITHOUT_UPPER = 1
MAX_MINUS_EPSILON = 1
CHILD_INDEX_X_MSB = 1
KEY_AT_INSERTION = 1
DEFAULTS = dict(first_box_oversize=FIRST_BOX_OVERSIZE, grow_shift_without_upper=GROW_SHIFT_WITHOUT_UPPER, max_minus_epsilon=MAX_MINUS_EPSILON,
                child_index_x_msb=CHILD_INDEX_X_MSB, key_at_insertion=KEY_AT_INSERTION)


class GridTooLarge(Exception):
    """the octree would be deeper than MAX_DEPTH levels (DGS_ERR_GRID_TOO_LARGE)"""


def concatenate(keyframes):
    """:22-29: pose = keyframe->pose.matrix().cast<float>(); dst = pose * (x, y, z, 1), per row ((m0 x + m1 y) + m2 z) + m3 in float,
    every step rounded; the output pad lane is 1."""
    out = []
    for cloud, pose in keyframes:
        c = np.asarray(cloud, F).reshape(-1, 4)
        m = np.asarray(pose, np.float64).astype(F)
        x, y, z = c[:, 0], c[:, 1], c[:, 2]
        q = np.ones((c.shape[0], 4), F)
        with np.errstate(invalid="ignore", over="ignore"):
            for r in range(3):
                q[:, r] = ((m[r, 0] * x + m[r, 1] * y) + m[r, 2] * z) + m[r, 3]
        out.append(q)
    return np.concatenate(out, 0) if out else np.zeros((0, 4), F)


class Box:
    """bounding box, depth and growth count of an OctreePointCloud; all arithmetic in double (python floats)"""

    def __init__(self, resolution, sw):
        self.res = float(resolution)
        self.sw = dict(DEFAULTS, **(sw or {}))
        self.mn = [0.0, 0.0, 0.0]
        self.mx = [0.0, 0.0, 0.0]
        self.depth = 0
        self.growths = 0
        self.defined = False

    def violations(self, q):
        lower = [float(q[a]) < self.mn[a] for a in range(3)]
        upper = [float(q[a]) >= self.mx[a] for a in range(3)]
        return lower, upper

    def define(self, q):
        """first finite point: [p - res/2, p + res/2], then getKeyBitSize with no leaves yet"""
        res = self.res
        for a in range(3):
            self.mn[a] = float(q[a]) - res / 2
            self.mx[a] = float(q[a]) + res / 2
        max_voxels = 2
        for a in range(3):
            max_voxels = max(max_voxels, int(math.ceil((self.mx[a] - self.mn[a] - FLT_EPSILON) / res)))
        self.depth = int(min(32.0, math.ceil(math.log2(float(max_voxels)) - FLT_EPSILON)))
        if self.depth > MAX_DEPTH:
            raise GridTooLarge()
        side = float(1 << self.depth) * res
        for a in range(3):
            if self.sw["first_box_oversize"]:
                over = (side - (self.mx[a] - self.mn[a])) / 2.0
                if over > FLT_EPSILON:
                    self.mn[a] -= over
                    self.mx[a] += over
            else:
                self.mx[a] = self.mn[a] + side
        self.defined = True

    def grow(self, upper, lower):
        """one new root.  Returns the child index the old root takes under it."""
        if self.depth + 1 > MAX_DEPTH:
            raise GridTooLarge()
        side = float(1 << self.depth) * self.res
        shift = [(not upper[a]) if self.sw["grow_shift_without_upper"] else lower[a] for a in range(3)]
        for a in range(3):
            if shift[a]:
                self.mn[a] -= side
        self.depth += 1
        side = float(1 << self.depth) * self.res
        if self.sw["max_minus_epsilon"]:
            side = side - FLT_EPSILON
        for a in range(3):
            self.mx[a] = self.mn[a] + side
        self.growths += 1
        return shift

    def adopt(self, q):
        """adoptBoundingBoxToPoint; -> list of `shift` triples, one per growth"""
        if not self.defined:
            self.define(q)
            return []
        events = []
        while True:
            lower, upper = self.violations(q)
            if not (any(lower) or any(upper)):
                return events
            events.append(self.grow(upper, lower))

    def key(self, q):
        """genOctreeKeyforPoint: (unsigned)(((double)x - min) / resolution)"""
        return tuple(int((float(q[a]) - self.mn[a]) / self.res) for a in range(3))

    def centre(self, k):
        """genLeafNodeCenterFromOctreeKey: (float)((key + 0.5) * resolution + min)"""
        return [F((float(k[a]) + 0.5) * self.res + self.mn[a]) for a in range(3)]

    def as_dict(self):
        return dict(min=np.array(self.mn, np.float64), max=np.array(self.mx, np.float64), depth=self.depth, growths=self.growths)


def _spread(v):
    """bits of an axis key (<= 21 of them, uint64 array) to every third bit"""
    x = v & np.uint64(0x1fffff)
    x = (x | (x << np.uint64(32))) & np.uint64(0x1f00000000ffff)
    x = (x | (x << np.uint64(16))) & np.uint64(0x1f0000ff0000ff)
    x = (x | (x << np.uint64(8))) & np.uint64(0x100f00f00f00f00f)
    x = (x | (x << np.uint64(4))) & np.uint64(0x10c30c30c30c30c3)
    x = (x | (x << np.uint64(2))) & np.uint64(0x1249249249249249)
    return x


def _compact(x):
    x = x & np.uint64(0x1249249249249249)
    x = (x | (x >> np.uint64(2))) & np.uint64(0x10c30c30c30c30c3)
    x = (x | (x >> np.uint64(4))) & np.uint64(0x100f00f00f00f00f)
    x = (x | (x >> np.uint64(8))) & np.uint64(0x1f0000ff0000ff)
    x = (x | (x >> np.uint64(16))) & np.uint64(0x1f00000000ffff)
    x = (x | (x >> np.uint64(32))) & np.uint64(0x1fffff)
    return x


def replay(points, resolution, sw=None):
    """The growth replay over the finite points of `points` [N,4] in order, without touching the points that stay inside the box:
    the first point that violates the current box is found by a vector pass over the rest.
    -> (Box, epochs).  An epoch is a run of points inserted under one box: dict(start = index of its first point among the finite
    points, mn = the box's min then, off = what the later growths add to a key made then: 2^depth per axis whose min moved -- the
    old root's child index under the new root)."""
    box = Box(resolution, sw)
    p = np.asarray(points, F)
    fin = np.isfinite(p[:, 0]) & np.isfinite(p[:, 1]) & np.isfinite(p[:, 2])
    pd = p[fin, :3].astype(np.float64)
    epochs = []
    pos = 0
    while pos < pd.shape[0]:
        if not box.defined:
            box.define(pd[0])
            epochs.append(dict(start=0, mn=list(box.mn), off=[0, 0, 0]))
            pos = 1
            continue
        rest = pd[pos:]
        mn, mx = np.array(box.mn), np.array(box.mx)
        bad = ((rest < mn) | (rest >= mx)).any(1)
        hit = np.flatnonzero(bad)
        if hit.size == 0:
            break
        i = pos + int(hit[0])
        depth = box.depth
        for shift in box.adopt(pd[i]):
            for e in epochs:
                for a in range(3):
                    e["off"][a] += int(shift[a]) << depth
            depth += 1
        epochs.append(dict(start=i, mn=list(box.mn), off=[0, 0, 0]))
        pos = i + 1
    return box, epochs


def octree_centres(points, resolution, sw=None, with_grid=False):
    """addPointsFromInputCloud + getOccupiedVoxelCenters, closed form: a point's key is made with the box of its own epoch
    (genOctreeKeyforPoint at insertion) and moved by the growths that follow, as the leaf is in the tree"""
    box, epochs = replay(points, resolution, sw)
    if not box.defined:
        out = np.zeros((0, 4), F)
        return (out, dict(min=np.zeros(3), max=np.zeros(3), depth=0, growths=0)) if with_grid else out
    p = np.asarray(points, F)
    fin = np.isfinite(p[:, 0]) & np.isfinite(p[:, 1]) & np.isfinite(p[:, 2])
    pd = p[fin, :3].astype(np.float64)
    if not box.sw["key_at_insertion"]:      # every key with the final min (the pointer octree cannot do this: it is not what a tree does)
        epochs = [dict(start=0, mn=list(box.mn), off=[0, 0, 0])]
    ep = np.searchsorted(np.array([e["start"] for e in epochs]), np.arange(pd.shape[0]), side="right") - 1
    mn = np.array([e["mn"] for e in epochs], np.float64)[ep]
    off = np.array([e["off"] for e in epochs], np.uint64)[ep]
    k = ((pd - mn) / box.res).astype(np.uint64) + off              # truncation of a non-negative double
    x_msb = box.sw["child_index_x_msb"]
    hi, lo = (k[:, 0], k[:, 2]) if x_msb else (k[:, 2], k[:, 0])
    code = np.unique((_spread(hi) << np.uint64(2)) | (_spread(k[:, 1]) << np.uint64(1)) | _spread(lo))   # ascending
    a2, a1, a0 = _compact(code >> np.uint64(2)), _compact(code >> np.uint64(1)), _compact(code)
    kx, kz = (a2, a0) if x_msb else (a0, a2)
    out = np.ones((code.shape[0], 4), F)
    for a, ka in enumerate((kx, a1, kz)):
        out[:, a] = ((ka.astype(np.float64) + 0.5) * box.res + box.mn[a]).astype(F)
    return (out, box.as_dict()) if with_grid else out


def generate(keyframes, resolution, sw=None, with_grid=False):
    """MapCloudGenerator::generate, closed form.  keyframes: (cloud [N,4], pose 4x4 double) pairs.  None for an empty list."""
    keyframes = list(keyframes)
    if len(keyframes) == 0:
        return None
    cloud = concatenate(keyframes)
    if not resolution > 0.0:
        return (cloud, dict(min=np.zeros(3), max=np.zeros(3), depth=0, growths=0)) if with_grid else cloud
    return octree_centres(cloud, resolution, sw, with_grid)


# ---------------------------------------------------------------------------------------------------- the literal pointer octree
class _Branch:
    __slots__ = ("child",)

    def __init__(self):
        self.child = [None] * 8


_LEAF = object()


def octree_centres_literal(points, resolution, sw=None, with_grid=False):
    """Point by point: adoptBoundingBoxToPoint (a new root per growth, the old root under child index
    (!upper_x << 2) | (!upper_y << 1) | !upper_z -- in general: the axes whose min moved), genOctreeKeyforPoint,
    createLeafRecursive along the key's bits from the top, then the depth-first walk of getOccupiedVoxelCenters."""
    box = Box(resolution, sw)
    x_msb = box.sw["child_index_x_msb"]
    root = _Branch()

    def child_index(bx, by, bz):
        return (bx << 2) | (by << 1) | bz if x_msb else (bz << 2) | (by << 1) | bx

    for q in np.asarray(points, F):
        if not (np.isfinite(q[0]) and np.isfinite(q[1]) and np.isfinite(q[2])):
            continue
        for shift in box.adopt(q):
            new_root = _Branch()
            new_root.child[child_index(int(shift[0]), int(shift[1]), int(shift[2]))] = root
            root = new_root
        k = box.key(q)
        node = root
        for level in range(box.depth - 1, -1, -1):
            ci = child_index((k[0] >> level) & 1, (k[1] >> level) & 1, (k[2] >> level) & 1)
            if level == 0:
                node.child[ci] = _LEAF
            else:
                if node.child[ci] is None:
                    node.child[ci] = _Branch()
                node = node.child[ci]
    out = []

    def walk(node, key, level):
        for ci in range(8):
            ch = node.child[ci]
            if ch is None:
                continue
            b2, b1, b0 = (ci >> 2) & 1, (ci >> 1) & 1, ci & 1
            bx, bz = (b2, b0) if x_msb else (b0, b2)
            nk = ((key[0] << 1) | bx, (key[1] << 1) | b1, (key[2] << 1) | bz)
            if ch is _LEAF:
                out.append(box.centre(nk) + [F(1.0)])
            else:
                walk(ch, nk, level - 1)

    if box.defined:
        walk(root, (0, 0, 0), box.depth)
    res = np.array(out, F).reshape(-1, 4)
    grid = box.as_dict() if box.defined else dict(min=np.zeros(3), max=np.zeros(3), depth=0, growths=0)
    return (res, grid) if with_grid else res


def generate_literal(keyframes, resolution, sw=None, with_grid=False):
    keyframes = list(keyframes)
    if len(keyframes) == 0:
        return None
    cloud = concatenate(keyframes)
    if not resolution > 0.0:
        return (cloud, dict(min=np.zeros(3), max=np.zeros(3), depth=0, growths=0)) if with_grid else cloud
    return octree_centres_literal(cloud, resolution, sw, with_grid)
