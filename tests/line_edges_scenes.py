"""Scenes of the edge-extraction tests (test_line_edges_cpu.py, test_line_edges_gpu.py) and of scripts/bench_line_align.py's `crossing`
rows, with the two raw calls the tests compare: the host's dgs_line_edges_angular and the device's dgs_line_edge_extraction_batch.

A scene is a list of segments, a segment an array of lines [n, 2, 3].  The kernels give a segment of n lines n * n consecutive pair
slots (p = i * n + j, nothing for j <= i), the batch's slots run through in workgroups of 256 and the workgroup sums are scanned in
chunks of 1024 workgroups, so the boundaries are: 255 / 256 / 257 slots in a batch (one short of a workgroup, exactly one, one over) and
512 * 512 + 1 slots (one over a scan chunk)."""
import ctypes as C

import numpy as np

import line_align_reference as R

MODES = [(False, 7.0), (True, 7.0), (True, 0.01)]            # align_global's call, align_local's target, align_local's source
WORKGROUP, SCAN_CHUNK = 256, 1024 * 256


def random_lines(n, seed, box=40.0):
    """n lines of 2 .. 12 m with arbitrary doubles for coordinates, any direction."""
    rng = np.random.default_rng(seed)
    c = rng.uniform(-box, box, (n, 2))
    a = rng.uniform(0.0, np.pi, n)
    h = 0.5 * rng.uniform(2.0, 12.0, n)
    d = np.stack([np.cos(a), np.sin(a)], 1) * h[:, None]
    out = np.zeros((n, 2, 3))
    out[:, 0, :2] = c - d
    out[:, 1, :2] = c + d
    return out


def star(n_h, n_v):
    """Long lines through well separated crossings: every roughly-horizontal line crosses every roughly-vertical one 50 m and more from
    all four ends (get_edges' fourth case, four edges), and lines of one family are nearly parallel (gated)."""
    out = [R.seg(-100.0, 5.0 * i + 0.1, 100.0, 5.0 * i + 0.37 + 0.01 * i) for i in range(n_h)]
    out += [R.seg(5.0 * j + 2.5, -100.0, 5.0 * j + 2.9 - 0.01 * j, 100.0) for j in range(n_v)]
    return np.array(out, np.float64)


def gate_lines():
    """A wall and lines at 0, 59, 60 -+ a hair, 61, 90, 119, 120 -+ a hair, 121 and 180 degrees to it: both sides of |cos| > 0.5."""
    out = [R.seg(-6.0, 0.0, 6.0, 0.0)]
    hair = 1e-9
    for deg in (0.0, 59.0, 60.0 - hair, 60.0, 60.0 + hair, 61.0, 90.0, 119.0, 120.0 - hair, 120.0, 120.0 + hair, 121.0, 180.0):
        a = np.deg2rad(deg)
        out.append(R.seg(0.5 - 6.0 * np.cos(a), 0.25 - 6.0 * np.sin(a), 0.5 + 6.0 * np.cos(a), 0.25 + 6.0 * np.sin(a)))
    for y in (0.8660254037844386, 0.8660254037844387, 0.8660254037844385):   # sqrt(3) / 2 and its neighbours against (1, 0)
        out.append(R.seg(0.25, -1.0, 0.25 + 4.0 * 0.5, -1.0 + 4.0 * y))
    return np.array(out, np.float64)


def max_lines():
    """DGS_LA_MAX_LINES_TARGET lines whose last pair (510, 511) is a crossing."""
    lines = random_lines(512, 512)
    lines[510] = R.seg(-3.0, 0.125, 4.0, 0.25)
    lines[511] = R.seg(0.5, -2.0, 0.625, 5.0)
    return lines


def crossing(n_buildings, corners=4, seed=None):
    """-> (source lines, target lines): a scan that sees two perpendicular facades of the first `corners` buildings of a ring (their
    middles, from a pose that is off by (0.3, -0.2) m and 2 degrees), so the source has edges, against all walls of the ring."""
    walls = R.ring(n_buildings, radius=35.0, seed=n_buildings if seed is None else seed)
    seen = np.concatenate([walls[4 * b:4 * b + 2] for b in range(min(corners, n_buildings))])
    return R.move(R.trim(seen), 0.3, -0.2, np.deg2rad(2.0)), walls


_E = np.zeros((0, 2, 3))
_L = lambda *segs: np.array(segs, np.float64).reshape(-1, 2, 3)
CASES = {   # one scene per get_edges case (tests/test_line_align_cpu.py's EDGE_SCENES), and the angular distance on either side of 7.0
    "case1_both_same": _L(R.seg(1, 0, 6, 0), R.seg(0, 1.5, 0, 7)),
    "case1_far": _L(R.seg(8, 0, 15, 0), R.seg(0, 9, 0, 16)),
    "case2_same1_only": _L(R.seg(1, 0, 6, 0), R.seg(0, -3, 0, 4)),
    "case2_far": _L(R.seg(7.5, 0, 16, 0), R.seg(0, -3, 0, 4)),
    "case3_same2_only": _L(R.seg(-3, 0, 4, 0), R.seg(0, 1, 0, 6)),
    "case3_other_end": _L(R.seg(-5, 0, 2, 0), R.seg(0, 6, 0, 1)),
    "case3_far": _L(R.seg(-3, 0, 4, 0), R.seg(0, 7.25, 0, 12)),
    "case4_neither": _L(R.seg(-3, 0, 4, 0), R.seg(0, -2, 0, 5)),
    "case4_short_arms": _L(R.seg(-0.5, 0, 4, 0), R.seg(0, -2, 0, 0.7)),
}
_CACHE = {}


def scenes():
    """name -> list of segments"""
    if "scenes" in _CACHE:
        return _CACHE["scenes"]
    two, three = CASES["case4_neither"], _L(R.seg(-3, 0, 4, 0), R.seg(0, -2, 0, 5), R.seg(-3, 1, 4, 1.25))
    one = two[:1]
    sc = {"n0": [_E], "n1": [one], "n2": [two], "n3": [three],
          "mixed_sizes": [_E, three, _E, _E, two, one, three + 0.5, _E]}
    sc.update({k: [v] for k, v in CASES.items()})
    sc["star"] = [star(5, 7)]
    sc["gate60"] = [gate_lines()]
    sc["wg_short"] = [random_lines(n, 100 + n) for n in (15, 5, 2, 1)]                   # 225 + 25 + 4 + 1 = 255 slots
    sc["wg_exact"] = [random_lines(16, 116)]                                             # 256
    sc["wg_over"] = [random_lines(16, 116), random_lines(1, 101)]                        # 257
    sc["wg_over_emits"] = [random_lines(15, 115), random_lines(5, 105), two + 1.0, one, two]   # 259: the last segment's crossing is slot 256, the second workgroup's first
    sc["tri23"] = [random_lines(23, 23)]                                                 # 253 pairs i < j
    sc["tri24"] = [random_lines(24, 24)]                                                 # 276
    sc["max512"] = [max_lines()]                                                         # exactly one scan chunk
    sc["scan_over"] = [max_lines(), one, three]                                          # one slot over it, then edges behind the carry
    _CACHE["scenes"] = sc
    return sc


def slots(segments):
    return sum(len(s) ** 2 for s in segments)


# ---- the two raw calls ---------------------------------------------------------------------------------------------------------------
def features(lines):
    """[n, 2, 3] -> the dgs_line_feature rows [n, 10] (statistics zero)."""
    out = np.zeros((max(len(lines), 1), 10), np.float64)
    out[:len(lines), :6] = np.asarray(lines, np.float64).reshape(-1, 6)
    return out


def host_edges(lines, only, dist):
    """dgs_line_edges_angular -> [m, 3, 3]"""
    from delta_graph_slam_amd import _lib as L
    lib = L.load()
    f = features(lines)
    n = C.c_int64(0)
    rc = lib.dgs_line_edges_angular(f.ctypes.data, len(lines), 1 if only else 0, float(dist), None, 0, C.byref(n))
    assert rc == 0 or n.value > 0, rc
    out = np.zeros((max(n.value, 1), 3, 3), np.float64)
    assert lib.dgs_line_edges_angular(f.ctypes.data, len(lines), 1 if only else 0, float(dist), out.ctypes.data, n.value, C.byref(n)) == 0
    return out[:n.value]


def host_batch(segments, only, dist):
    """-> (edges [m, 3, 3], offsets [n + 1]) of the host function, segment by segment; computed once per (scene, mode) by the callers"""
    e = [host_edges(s, only, dist) for s in segments]
    return np.concatenate(e + [np.zeros((0, 3, 3))]), np.cumsum([0] + [len(x) for x in e]).astype(np.int64)


def device_batch_raw(lib, handle, segments, modes, capacity=None, want_offsets=True):
    """dgs_line_edge_extraction_batch with a per-segment (only, dist) list -> (rc, edges [m, 3, 3], offsets [n + 1], n_edges).  `capacity`
    None: room for 4 edges per pair."""
    n = len(segments)
    f = features(np.concatenate(list(segments) + [_E]))
    off = np.cumsum([0] + [len(s) for s in segments]).astype(np.int64)
    only = np.array([1 if m[0] else 0 for m in modes] + [0], np.int32)
    dist = np.array([m[1] for m in modes] + [0.0], np.float64)
    cap = sum(2 * len(s) * (len(s) - 1) for s in segments) if capacity is None else capacity
    out = np.zeros((max(cap, 1), 3, 3), np.float64)
    eo = np.full(n + 1, -1, np.int64)
    ne = C.c_int64(-1)
    rc = lib.dgs_line_edge_extraction_batch(handle, f.ctypes.data, off.ctypes.data, n, only.ctypes.data, dist.ctypes.data,
                                            out.ctypes.data if cap else None, cap, eo.ctypes.data if want_offsets else None, C.byref(ne))
    return rc, out[:max(min(ne.value, cap), 0)], eo, ne.value
