"""Inputs that put the building overlap kernels (delta_graph_slam_amd/csrc/building_overlap.hip) at the edges their own launch shapes
create: flag rows longer than 64 words, full words, rows and columns at word and tile boundaries, the scan at every ownership size,
the last line pair of a 512 x 512 pair space; target tables past one LDS fill trip, twins of bit-equal norm one arg-min trip or several
waves apart, every unit-table size around kBoUnits, empty items at the ends of a batch, the item and hypothesis limits.

Plain numpy on tests/building_overlap_reference.py (BR), no GPU.  tests/test_building_overlap_edge_cases_cpu.py proves on the restatement
what each builder claims and runs the host header on every scene; tests/test_building_overlap_edges_gpu.py runs the device on them.
Restatement results are memoised per scene content; edge extraction (the scalar pair loop that dominates a 512-line item, and has no
trigonometry) is computed once per line list and shared between the plain and the nudged run."""
import json
import os

import numpy as np

import building_overlap_reference as BR

NONE, seg, rectangle, move, fence = BR.NONE, BR.seg, BR.rectangle, BR.move, BR.fence
WAVE, BLOCK, TILE_ROWS, UNITS = 64, 256, 2, 16            # kWave, kBlock, kBoTileRows, kBoUnits of building_overlap.hip
MAX_ITEMS, MAX_HYPOTHESES = 4096, 1 << 21                 # DGS_LA_MAX_ITEMS, DGS_LA_MAX_HYPOTHESES
Z = np.zeros(3)
_CACHE = {}


def _memo(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


# ==================================================================================================== pair search
def _thin(k, n):
    """clique24's recipe: the k-th of n thin rectangles through (nearly) one point"""
    return rectangle(0.3 * np.cos(k), 0.3 * np.sin(k), 30, 1.0, np.pi * k / n), [0.3 * np.cos(k), 0.3 * np.sin(k), 0.0]


def clique(n):
    both = [_thin(k, n) for k in range(n)]
    return [b for b, _ in both], np.array([c for _, c in both], np.float64)


WORDS66_AT = (0, 63, 64, 65, 4095, 4096, 4159, 4160)


def words66():
    """4161 buildings (66 words a row), all empty but eight mutually crossing rectangles"""
    B = 4161
    bl, ce = [NONE] * B, np.zeros((B, 3))
    for k, i in enumerate(WORDS66_AT):
        bl[i], ce[i] = _thin(k, len(WORDS66_AT))
    return bl, ce


ALIGN_ROWS, ALIGN_COLS = (62, 63, 64, 65), (127, 128, 129)


def planted_alignment_pairs(B):
    return [(i, j) for i in ALIGN_ROWS for j in (i + 1,) + ALIGN_COLS if i < j < B]


def alignment_rows(B):
    """B <= 130 buildings, empty but: posts 62 .. 65, each crossed by its successor's arm (66 is an arm only), and three long rails at
    127, 128 and 129 (those below B) that cross every post and nothing else"""
    bl, ce = [NONE] * B, np.zeros((B, 3))
    post = lambda k: seg(10.0 * (k - 62), -2.0, 10.0 * (k - 62) + 0.1, 6.0)
    arm = lambda k: seg(10.0 * (k - 62) - 12.0, 4.3, 10.0 * (k - 62) - 8.0, 4.5)
    for k in range(62, 67):
        bl[k] = np.array(([post(k)] if k < 66 else []) + ([arm(k)] if k > 62 else []))
    for n, j in enumerate(ALIGN_COLS):
        if j < B:
            bl[j] = np.array([seg(-5.0, 0.5 * n, 45.0, 0.5 * n + 0.2)])
    for k in range(B):
        ce[k] = BR.centroid(bl[k])
    return bl, ce


SCAN_SIZES = (255, 256, 257, 511, 512, 513, 4097)


def scan_city(B):
    """A jittered grid of B buildings; buildings 0, B - 2 and B - 1 stand apart from it, the last one across the other two"""
    bl, ce = BR._city(B, B)
    bl, ce = list(bl), ce.copy()
    for k, b in ((0, rectangle(-100, 0, 8, 6, 0.1)), (B - 2, rectangle(-100, 30, 8, 6, 0.2)), (B - 1, rectangle(-100, 15, 3, 40, 0.05))):
        bl[k], ce[k] = b, BR.centroid(b)
    return bl, ce


# per = 64: thread t of the scan owns rows [64 t, 64 t + 64).  Rows at both ends of an owner's range, in its middle, in the last owner's
# range; columns in the row's own word, in later words and in the last word
SPARSE_PAIRS = ((0, 1), (0, 16383), (1, 64), (63, 64), (63, 4096), (64, 65), (65, 127), (127, 128), (128, 8191), (4095, 4096), (4096, 4097),
                (4097, 16382), (8191, 8192), (8192, 12345), (12345, 12346), (16319, 16320), (16320, 16321), (16320, 16381), (16381, 16382),
                (16382, 16383))


def scan_sparse():
    """2^14 buildings, empty but for the buildings of SPARSE_PAIRS: a building is a cross of one stroke per pair it is in, strokes of a
    pair cross each other 100 m from every other pair"""
    B = 1 << 14
    strokes = {}
    for n, (i, j) in enumerate(SPARSE_PAIRS):
        strokes.setdefault(i, []).append(seg(100.0 * n - 3, -2.0, 100.0 * n + 3, 2.5))
        strokes.setdefault(j, []).append(seg(100.0 * n - 3, 2.0, 100.0 * n + 2.5, -2.5))
    bl, ce = [NONE] * B, np.zeros((B, 3))
    for k, s in strokes.items():
        bl[k] = np.array(s)
    return bl, ce           # every centre at the origin: shrinking scales the whole scene


def _pickets(n, x0, pitch, y0, y1):
    """exactly vertical: a pair of them has det == 0 whatever the centres, and a line that meets their carrier outside [y0, y1] misses"""
    return [seg(x0 + pitch * k, y0, x0 + pitch * k, y1) for k in range(n)]


def picket_pair(parallel=False):
    """Two buildings of 512 lines: 511 pickets and, last, a long line high above every picket.  The long lines cross each other
    (`parallel`: they do not), so line pair (511, 511) is the only one that can intersect."""
    a = np.array(_pickets(511, 0.0, 0.1, 0.0, 1.0) + [seg(-10, 10, 60, 12)])
    b = np.array(_pickets(511, 0.05, 0.1, 2.0, 3.0) + [seg(-10, 11, 60, 13) if parallel else seg(-10, 12, 60, 9)])
    return a, b, BR.centroid(a), BR.centroid(b)


def line_space_scenes():
    """name -> (buildings, centres)"""
    a, b, ca, cb = picket_pair()
    _, bp, _, cbp = picket_pair(parallel=True)
    tri = BR.polygon([[49, 9.0], [51, 9.2], [50, 10.2]])        # across the second long line only
    ct = BR.centroid(tri)
    return {"last_line_pair": ([a, b], np.array([ca, cb])), "no_line_pair": ([a, bp], np.array([ca, cbp])),
            "tile_512_3": ([a, tri, b], np.array([ca, ct, cb])), "tile_none_512": ([NONE, a, tri, b], np.array([Z, ca, ct, cb]))}


def far(scene, offset=500.0):
    bl, ce = scene
    d = np.array([offset, offset, 0.0])
    return [b + d for b in bl], ce + d


def pair_scenes():
    """name -> (buildings, centres): every pair scene of this module"""
    def make():
        sc = {"words66": words66(), "clique130": clique(130), "scan_sparse": scan_sparse()}
        for B in (130, 129, 128):
            sc["rows%d" % B] = alignment_rows(B)
        for B in SCAN_SIZES:
            sc["scan%d" % B] = scan_city(B)
        sc.update(line_space_scenes())
        return sc
    return _memo("pair_scenes", make)


PAIR_NAMES = (["words66", "clique130", "scan_sparse"] + ["rows%d" % B for B in (130, 129, 128)] + ["scan%d" % B for B in SCAN_SIZES] +
              ["last_line_pair", "no_line_pair", "tile_512_3", "tile_none_512"])


# The restatement walks 4097 rows of five lines against 20,000 later lines: 11 s.  Its list is kept as a fixture, which the CPU test
# compares with a fresh restatement run; every other list is computed where it is needed.
GOLDEN = {"scan4097": os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "building_overlap_scan4097_pairs.json")}


def pair_result_fresh(name):
    return _memo(("pairs_fresh", name), lambda: BR.overlapped_pairs(*pair_scenes()[name]))


def pair_result(name):
    if name in GOLDEN:
        return _memo(("pairs", name), lambda: np.array(json.load(open(GOLDEN[name]))["pairs"], np.int32).reshape(-1, 2))
    return pair_result_fresh(name)


def position(pairs, i, j):
    """where pair (i, j) stands in a list"""
    return int(np.nonzero((pairs[:, 0] == i) & (pairs[:, 1] == j))[0][0])


# ==================================================================================================== alignment
_edge_extraction = BR.R.edge_extraction


def _edges_once(lines, cases=None):
    if cases is not None:
        return _edge_extraction(lines, cases)
    return _memo(("edges", np.asarray(lines, np.float64).tobytes()), lambda: _edge_extraction(lines))


def restated(item, seed=None):
    """BR.align_overlapped(*item, seed=seed), memoised on the item's content"""
    def make():
        BR.R.edge_extraction = _edges_once
        try:
            return BR.align_overlapped(*item, seed=seed)
        finally:
            BR.R.edge_extraction = _edge_extraction
    return _memo(("align", seed) + tuple(np.asarray(x, np.float64).tobytes() for x in item), make)


SOURCE_LINES = np.array([seg(-4, 0, 4, 0.05), seg(-0.5, -1.03, 0.5, -1.024), seg(-3, -2.07, -2, -2.064)])
CENTER_WALLS = np.array([0.0, 26.0, 0.0])


def _walls(ks, pitch=0.2):
    """nearly parallel walls above the source lines, wall k at height 1 + pitch k: the source is nearest to wall 0"""
    return np.array([seg(-5, 1 + pitch * k, 5, 1 + pitch * k + 0.01 * pitch * k) for k in ks]).reshape(-1, 2, 3)


def twins(first, ks, reps=2):
    """One source line against walls `first` (each once), then walls `ks` listed `reps` times; the scene turned by 0.2 rad"""
    trg = np.concatenate([_walls(first)] + [_walls(ks)] * reps)
    return BR._turned((SOURCE_LINES[:1], trg, Z, CENTER_WALLS), 0.2)


def _nearest_at(pos, n):
    ks = list(range(1, n))
    ks.insert(pos, 0)
    return ks


TWIN_CASES = {
    # name: (first, ks, the twins' h)
    "trip_lane0": ([], _nearest_at(0, 256), (0, 256)),               # the same lane on consecutive trips: lane 0 of wave 0,
    "trip_wave3": ([], _nearest_at(200, 256), (200, 456)),           # a lane of wave 3,
    "trip_last_lane": ([], _nearest_at(255, 256), (255, 511)),       # the last lane of the workgroup
    "waves_1_3": ([], _nearest_at(99, 100), (99, 199)),              # the lower h in wave 1, its twin in wave 3
    "waves_3_0": (list(range(100, 300)), _nearest_at(0, 100), (200, 300)),   # the lower h in wave 3, its twin in wave 0 on the second trip
}


def twin_item(name):
    first, ks, _ = TWIN_CASES[name]
    return _memo(("twin", name), lambda: twins(first, ks))


def _blocker(y0, y1):
    """ten degrees off the walls' normal, across the band [y0, y1] of walls where a moved source line comes to lie"""
    return seg(0.3, y0, 0.3 + np.tan(np.deg2rad(10)) * (y1 - y0), y1)


PAST_255 = {
    # Lt: (Ls, bands): Lt - len(bands) walls, then one blocker per band: the blockers are the last target lines
    256: (2, [(10, 16)]),
    257: (3, [(10, 16)]),
    512: (1, [(3, 8), (14, 20), (30, 36), (44, 49)]),
}


def past_255(Lt):
    def make():
        Ls, bands = PAST_255[Lt]
        trg = np.concatenate([_walls(range(Lt - len(bands)), pitch=0.1), np.array([_blocker(*b) for b in bands])])
        return BR._turned((SOURCE_LINES[:Ls], trg, Z, CENTER_WALLS), 0.2)
    return _memo(("past255", Lt), make)


def overlap_gates_without_lines_from(item, first):
    """-> (gate [Ls, first] of the item with its target cut to `first` lines, gate [Ls, first] of the whole item over the same line
    pairs); both without edge pairs"""
    src, trg, cs, ct = item
    cut, whole = restated((src, trg[:first], cs, ct)), restated(item)
    assert cut["n_edge"] == 0 and whole["n_edge"] == 0
    return cut["gate"].reshape(src.shape[0], first), whole["gate"].reshape(src.shape[0], trg.shape[0])[:, :first]


def _source_fence():
    return fence(256, -25, -3, 0.2, 6.0, cross=False)


def source_limit(Lt):
    """256 pickets against: a line ten degrees off them near their right end (Lt = 1); that and a line seventy degrees off them, behind
    the angle gate, which the moved pickets reach from some hypotheses (Lt = 2); or those two with 255 short far walls between them
    (Lt = 257), so that the only line any moved picket can meet is target line 256"""
    def make():
        onto = seg(24, -4, 24 + 8 * np.tan(np.deg2rad(10)), 4)
        across = seg(36, -4, 47, 0)
        far_walls = [seg(-20 + 0.15 * k, 30 + 0.05 * k, -17 + 0.15 * k, 30.9 + 0.05 * k) for k in range(255)]
        trg = {1: [onto], 2: [onto, across], 257: [onto] + far_walls + [across]}[Lt]
        return BR._turned((_source_fence(), np.array(trg), Z, np.array([30.0, 0.0, 0.0])), 0.2)
    return _memo(("source_limit", Lt), make)


UNIT_H = (0, 1, 15, 16, 17, 0, 0, 31, 32, 33, 16, 1, 0)
_UNIT_SHAPES = ((0, 5), (1, 1), (3, 5), (4, 4), (1, 17), (3, 0), (0, 0), (31, 1), (4, 8), (3, 11), (16, 1), (1, 1), (2, 0))


def _picket_item(Ls, Lt, k):
    """fences65's recipe at Ls x Lt, shifted a little with k.  From three target lines on, target line 0 is a short blocker, seventy
    degrees off the pickets and so behind the angle gate, across the middle of the last target picket: the hypotheses that lay a source
    line there, the item's last one among them, are overlapped"""
    s = fence(Ls, -10, -3, 0.33, 6.0, cross=False) if Ls else NONE
    x0, n = -9 + 0.07 * k, Lt - 1 if Lt >= 3 else Lt
    t = fence(n, x0, -2, 0.3, 5.0, slope=0.01, cross=False) if n else NONE
    if n < Lt:
        x, y = x0 + 0.3 * (n - 1), -2 + 0.01 * (n - 1) + 2.5
        t = np.concatenate([[seg(x - 0.5, y - 0.18, x + 0.5, y + 0.18)], t])
    return BR._turned((s, move(t, 0.5, 0.4, np.deg2rad(6)), Z, np.array([0.5, 0.5, 0.0])), 0.05 + 0.01 * k)


def batch_units():
    """13 line-only items whose hypothesis counts are UNIT_H: one, 15, 16 and 17, 31, 32 and 33 hypotheses, empty items first, last and
    back to back (an empty source, an empty target, both)"""
    return _memo("units", lambda: [_picket_item(Ls, Lt, k) for k, (Ls, Lt) in enumerate(_UNIT_SHAPES)])


def prototypes():
    """8 small items: line-only ones of batch_units (among them a 1 x 1 and an empty one) and BR's mixed items, which have edge pairs"""
    u = batch_units()
    return _memo("prototypes", lambda: [u[1], u[0], u[2], BR._mixed_item(3), u[4], BR._mixed_item(4), u[7], u[9]])


def over_the_hypothesis_limit():
    """17 items of 256 x 512 pickets: 17 x 2^17 hypotheses"""
    it = (_source_fence(), fence(512, -30, 2, 0.11, 5.0, cross=False), Z, Z)
    return [it] * 17
