"""-m gpu: the double computeHessian pass of the upstream-order NDT kernel (evaluation kind 2, ndt_strict_order = 1 with
ndt_hessian_recompute_double) with its voxel rows brought through the wave's LDS ring (strict_items_hd in
delta_graph_slam_amd/csrc/ndt_strict.h; DIRECT7 -- the other searches have no room for the ring and keep the plain loop).

One pair alone and one evaluation (Registration.ndt_hessian_double), so the slices are a function of the source size alone:
cap = max(ceil(n/512), min(64, ceil(n/256))) slices of 256 points, in the default launch and under DGS_NDT_FIXED_SLICES=1 alike.
  * DIRECT7, order 1 against the oracle, BIT FOR BIT on the 36 doubles.  The oracle (NdtOracle.hessian_double) adds the items' terms in
    point order; the kernel adds the same terms per lane in queue order.  So the reference is made from the oracle's own per-item terms:
    an item's 36 terms are what the oracle returns for that one point against a target holding that one voxel's points (same points in
    the same order: the same mean and inverse covariance) -- checked first: added in point / slot order they give the oracle's Hessian of
    the whole scene, bit for bit.  They are then added in float64 in the kernel's order (_kernel_order_sum): a wave's 64-point tile
    queues its items slot-major at ballot positions, lane l takes items l, 64 + l, ... into its own sums, a wave adds its lanes in lane
    order from 0.0, the workgroup ((wave 0 + wave 1) + wave 2) + wave 3, the slices' rows (at most two here) are added.
  * default launch against fixed slices (the plain loop: 23-field table, the row gathered where it is used): bit-identical, every search;
  * order 2 against the oracle: bit-identical; order 1 against the oracle for DIRECT1 / DIRECT26 (plain loop): tests/test_strict_edges_gpu.py's 1e-11.
The item counts each scene is meant to produce are checked on the CPU first, from the items the reference sum is made of (_items: the
valid voxels of every point at the pose, through oracle/ndt_ref.py's voxel model): see the `scenes` fixture."""
import concurrent.futures
import contextlib
import os

import numpy as np
import pytest

from delta_graph_slam_amd import _lib as L
from oracle import ndt_ref
from tests import strict_edge_cases as E

pytestmark = pytest.mark.gpu

RES = E.RES_POW2
SIZES = (1, 63, 64, 65, 127, 129, 257)


@contextlib.contextmanager
def _env(**kv):
    old = {k: os.environ.get(k) for k in kv}
    os.environ.update({k: str(v) for k, v in kv.items()})
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _reg(order, search, **kw):
    from delta_graph_slam_amd.registration import Registration
    return Registration("NDT_OMP", ndt_strict_order=order, ndt_resolution=RES, ndt_search_method=L.NDT_SEARCH[search],
                        ndt_hessian_recompute_double=1, **kw)


def _items(tgt, src, pose):
    """Per point, the kernel's seven DIRECT7 slots in upstream's visiting order ((0,0,0) +x -x +y -y +z -z): the cell of the voxel the slot
    holds, or None.  The transformed point in float as oracle/ndt_ref.neighbour_sets makes it.  A NaN coordinate makes all of xt NaN, and
    the device's (int)floorf(NaN) = 0 puts the point into cell (0, 0, 0): its items ARE queued and then fail upstream's weight test
    (e != e).  An infinite coordinate gives infinite (or, at the identity, NaN and infinite) xt: a cell outside the grid, no items."""
    model = ndt_ref.VoxelModel(tgt, RES)
    R = ndt_ref.rot_xyz(*pose[3:])
    with np.errstate(invalid="ignore", over="ignore"):
        xt = (np.asarray(src, np.float64)[:, :3] @ R.T + pose[:3]).astype(np.float32)
        q = np.floor(xt / np.float32(RES))
    out = []
    for i in range(xt.shape[0]):
        if np.isinf(q[i]).any():
            out.append([None] * 7)
            continue
        ijk = np.where(np.isnan(q[i]), 0.0, q[i]).astype(np.int64)
        out.append([tuple(int(v) for v in ijk + o) if model.lookup(ijk + o) is not None else None for o in ndt_ref._OFF7])
    return out


def _counts(items):
    return np.array([sum(c is not None for c in it) for it in items])


def _terms(orc, tgt, src, pose, items, cache):
    """(point, slot) -> the item's 36 terms: the oracle's double computeHessian of that one point against that one voxel's points.
    cache: (point, cell) -> terms at this pose and target, shared by the scenes that are cuts of one cloud."""
    cells = np.floor(tgt[:, :3] / np.float32(RES)).astype(np.int64)
    by_cell = {}
    for i, it in enumerate(items):
        for k, c in enumerate(it):
            if c is not None:
                by_cell.setdefault(c, []).append((i, k))
    finite = np.isfinite(src[:, :3]).all(1)
    terms = {}

    def work(part):   # a call costs ~2.6 ms whatever the source size (the oracle clears its term buffer): four oracles side by side
        o = orc.NdtOracle(resolution=RES, search_method="DIRECT7", num_threads=1)
        for c, users in part:
            o.set_target(tgt[(cells == np.array(c)).all(1)])
            for i, k in users:
                key = (src[i].tobytes(), c)
                if not finite[i]:
                    cache[key] = np.zeros(36)         # the oracle's semantics: a non-finite point contributes nothing
                elif key not in cache:
                    o.set_source(src[i:i + 1])
                    cache[key] = o.hessian_double(pose).ravel().copy()
                terms[(i, k)] = cache[key]

    todo = list(by_cell.items())
    with concurrent.futures.ThreadPoolExecutor(4) as ex:
        list(ex.map(work, [todo[j::4] for j in range(4)]))
    return terms


def _point_order_sum(items, terms):
    H = np.zeros(36)
    for i, it in enumerate(items):
        for k, c in enumerate(it):
            if c is not None:
                H = H + terms[(i, k)]
    return H.reshape(6, 6)


def _kernel_order_sum(n, items, terms):
    """The 36 sums as ndt_strict3_kernel's double pass adds them for one pair alone (see the module docstring)."""
    n_slices = max((n + 511) // 512, min(64, (n + 255) // 256), 1)
    total = np.zeros(36)
    for q in range(n_slices):
        waves = []
        for w in range(4):
            acc = np.zeros((64, 36))
            for first in range(q * 256 + w * 64, n, n_slices * 256):          # the wave's 64-point tiles of this slice
                queue = [(first + lane, k) for k in range(7) for lane in range(64) if first + lane < n and items[first + lane][k] is not None]
                for pos, key in enumerate(queue):
                    acc[pos % 64] = acc[pos % 64] + terms[key]
            v = np.zeros(36)
            for lane in range(64):
                v = v + acc[lane]
            waves.append(v)
        total = total + (((waves[0] + waves[1]) + waves[2]) + waves[3])
    return total.reshape(6, 6)


def _pick(counts, total, n_max=64):
    """Indices of at most n_max points whose item counts add up to `total` exactly (subset sum over the first points that have items)."""
    reach = {0: []}
    for i, c in enumerate(counts):
        if c == 0:
            continue
        for s, idx in list(reach.items()):
            t = s + int(c)
            if t <= total and t not in reach and len(idx) < n_max:
                reach[t] = idx + [i]
        if total in reach:
            return reach[total]
    raise AssertionError("no subset with %d items" % total)


@pytest.fixture(scope="module")
def scenes(oracle_lib):
    """name -> (target, source, per pose: the items and their terms, the oracle's Hessian, the reference sum in the kernel's order): built
    once, on the CPU, and left unchanged.  The intended item counts are asserted here, from the very items the reference sum is made of."""
    raw = {}
    tgt, solid, _ = E.solid(max(SIZES), RES)
    for n in SIZES:                           # cuts of one cloud (an item's terms are computed once); solid 64 is also the longest queue:
        raw["solid %d" % n] = (tgt, solid[:n])    # 64 points x 7 valid voxels = 448 items, 7 full rounds
    tgt, src, _ = E.outside(129, RES)
    raw["no valid voxel"] = (tgt, src)
    tgt, pool, _ = E.faces(512, RES)          # points on the faces of the box: 1 .. 7 valid voxels
    c = _counts(_items(tgt, pool, E.POSES[0]))
    assert c.min() < 7 and c.max() == 7
    for total in (64, 65):                    # one full round / a full round and a one-item second round, all in wave 0's tile
        raw["%d items" % total] = (tgt, pool[_pick(c, total)])
    tgt, src, _ = E.nonfinite(64, RES)        # NaN / Inf points among finite ones, one wave's tile
    raw["weight test fails"] = (tgt, src)
    o = oracle_lib.NdtOracle(resolution=RES, search_method="DIRECT7")
    out = {}
    caches = {}
    for name, (tgt, src) in raw.items():
        o.set_target(tgt)
        o.set_source(src)
        per_pose = []
        for p in E.POSES:
            items = _items(tgt, src, p)
            terms = _terms(oracle_lib, tgt, src, p, items, caches.setdefault((tgt.tobytes(), p.tobytes()), {}))
            Hd = o.hessian_double(p)
            # the per-item terms are the oracle's: in its own order of addition they give its Hessian of the whole scene, bit for bit
            assert _point_order_sum(items, terms).tobytes() == Hd.tobytes(), (name, "per-item terms")
            per_pose.append(dict(counts=_counts(items), terms=terms, Hd=Hd, ref=_kernel_order_sum(src.shape[0], items, terms)))
        out[name] = (tgt, src, per_pose)
    cnt = {name: [pp["counts"] for pp in v[2]] for name, v in out.items()}
    for k in range(len(E.POSES)):
        assert cnt["no valid voxel"][k].sum() == 0                                    # qn = 0 in every tile: no DMA may be issued
        assert (cnt["solid 64"][k] == 7).all()                                        # the longest queue
        for n in SIZES:
            assert cnt["solid %d" % n][k].sum() == 7 * n
    # exactly 64 and 65 items in wave 0's tile at POSES[0], where the points lie exactly on voxel faces; POSES[1] moves them off the
    # faces and the counts there are what they are (printed by the test), still one tile of one wave
    assert cnt["64 items"][0].sum() == 64 and cnt["65 items"][0].sum() == 65 and len(cnt["65 items"][0]) <= 64
    # the weight test in the middle of a round: the NaN points (a NaN coordinate) queue their seven items, in rounds whose other lanes
    # hold items of finite points, and every one of them is rejected (the oracle gives no term for such a point); the +-Inf points queue nothing
    src = raw["weight test fails"][1]
    for k in range(len(E.POSES)):
        c = cnt["weight test fails"][k]
        for i in (i for i in E.NONFINITE_AT if i < 64):
            assert c[i] == (7 if np.isnan(src[i, :3]).any() else 0), (i, c[i])
        assert c.sum() > 6 * 64   # their rounds are full of finite points' items
    return out


@pytest.mark.parametrize("search", ["DIRECT7", "DIRECT1", "DIRECT26"])
def test_double_pass_ring_against_plain_loop_and_oracle(oracle_lib, scenes, search):
    r1, r2 = _reg(1, search), _reg(2, search)
    with _env(DGS_NDT_FIXED_SLICES=1):
        r1_fixed = _reg(1, search)
    o = oracle_lib.NdtOracle(resolution=RES, search_method=search)
    last_tgt = None
    for name, (tgt, src, per_pose) in scenes.items():
        if last_tgt is None or not np.array_equal(last_tgt, tgt):
            last_tgt = tgt
            o.set_target(tgt)
            for r in (r1, r2, r1_fixed):
                r.setInputTarget(tgt)
        o.set_source(src)
        for r in (r1, r2, r1_fixed):
            r.setInputSource(src)
        for k, p in enumerate(E.POSES):
            what = (name, search, k)
            Hd = o.hessian_double(p)
            H1, H1f, H2 = r1.ndt_hessian_double(p), r1_fixed.ndt_hessian_double(p), r2.ndt_hessian_double(p)
            err = np.abs(H1 - Hd).max() / (np.abs(Hd).max() + 1e-300)
            print(what, "items", int(per_pose[k]["counts"].sum()), "order 1 against the oracle: %.3g of the largest entry; ring == plain: %s"
                  % (err, H1.tobytes() == H1f.tobytes()))
            if search == "DIRECT7":
                ref = per_pose[k]["ref"]
                print(what, "order 1 against the oracle's terms in the kernel's order: %d of 36 doubles differ" % int((H1 != ref).sum()))
                assert H1.tobytes() == ref.tobytes(), what + ("order 1 against the oracle's terms added in the kernel's order",)
            else:
                assert err <= 1e-11, what + ("order 1 against the oracle", err)
            assert H1.tobytes() == H1f.tobytes(), what + ("ring loop against the plain loop",)
            assert np.array_equal(H2, Hd), what + ("order 2 against the oracle",)
            if name == "no valid voxel":
                assert not H1.any() and not Hd.any(), what
            else:
                assert np.abs(Hd).max() > 0, what
            assert r1.ndt_hessian_double(p).tobytes() == H1.tobytes(), what + ("repeat",)
    for r in (r1, r2, r1_fixed):
        r.close()
