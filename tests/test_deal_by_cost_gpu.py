"""-m gpu: deal_workgroup_by_cost (delta_graph_slam_amd/csrc/common.h) deals the workgroups of an item-compacted NDT launch to the active
pairs ranked by (cost class of the evaluation kind they wait for, heaviest first; then pair index).  Everything else is deal_workgroup's:
with A active pairs, blocks_per_pair = max(1, min(grid / A, cap_blocks)), workgroup b serves slice b % blocks_per_pair of the pair of rank
b / blocks_per_pair, or nothing when that rank is >= A -- so the SET of (pair, slice) served is the same and only the workgroup that serves
each changes, which is why no sum of the kernel can change (tests/test_deal_by_cost_bits_gpu.py).

Through the test hook dgs_deal_probe_cost (activity mask and a kind per pair as data; writes what EVERY wave of every workgroup derived, and
the class order the library was built with): n_pairs on either side of the 64-pair ballot and of the 256 kept pairs, grids of 1024 + n_pairs
workgroups, a cap that binds and one that does not, the masks of tests/test_deal_workgroup_gpu.py, and kind patterns that put a class
boundary at every place the ranking can get wrong."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N_PAIRS = (1, 3, 5, 32, 64, 65, 200, 256, 257, 300)
CAPS = (1024, 3)


def _reference(active, cap_blocks, grid):
    """deal_workgroup's mapping, restated: the pair of rank b / per in INDEX order"""
    idx = np.flatnonzero(active)
    out = np.full((grid, 4), -1, np.int32)
    out[:, 3] = idx.size
    if idx.size == 0:
        return out
    per = max(1, min(grid // idx.size, cap_blocks))
    b = np.arange(grid)
    rank, sl = b // per, b % per
    ok = rank < idx.size
    out[ok, 0] = idx[rank[ok]]
    out[ok, 1] = sl[ok]
    out[ok, 2] = per
    return out


def _masks(n):
    rng = np.random.default_rng(n)
    alt = (np.arange(n) % 2).astype(np.int32)
    last = np.zeros(n, np.int32)
    last[-1] = 1
    return {"empty": np.zeros(n, np.int32), "full": np.ones(n, np.int32), "alternating": alt, "alternating, other phase": 1 - alt,
            "random 30 %": (rng.random(n) < 0.3).astype(np.int32), "the last pair alone": last}


def _kinds(n, order):
    heavy, light = order[0], order[2]
    rng = np.random.default_rng(1000 + n)
    only_heavy_last = np.full(n, light, np.int32)
    only_heavy_last[-1] = heavy
    only_light_first = np.full(n, heavy, np.int32)
    only_light_first[0] = light
    return {"all 0": np.zeros(n, np.int32), "all 1": np.ones(n, np.int32), "all 2": np.full(n, 2, np.int32),
            "cycling 0 1 2": (np.arange(n) % 3).astype(np.int32), "the only heavy pair last": only_heavy_last,
            "the only light pair first": only_light_first, "random": rng.integers(0, 3, n).astype(np.int32)}


@pytest.fixture(scope="module")
def reg():
    from delta_graph_slam_amd.registration import Registration
    r = Registration("NDT_OMP")
    yield r
    r.close()


def _probe(r, mask, kinds, n, cap, grid):
    out = np.full((grid, 4, 4), -7, np.int32)
    order = np.full(3, -7, np.int32)
    rc = r._lib.dgs_deal_probe_cost(r._h, mask.ctypes.data_as(C.c_void_p), kinds.ctypes.data_as(C.c_void_p), n, cap, grid, out.ctypes.data_as(C.c_void_p),
                                    order.ctypes.data_as(C.c_void_p))
    assert rc == 0, (n, cap, rc)
    return out, order


@pytest.mark.parametrize("n", N_PAIRS)
def test_cost_ordered_dealing(reg, n):
    grid = 1024 + n
    _, order = _probe(reg, np.ones(n, np.int32), np.zeros(n, np.int32), n, 1024, grid)
    assert sorted(order.tolist()) == [0, 1, 2], order
    cls_of_kind = np.empty(3, np.int64)
    cls_of_kind[order] = np.arange(3)   # 0 = heaviest class
    checked = 0
    for mname, mask in _masks(n).items():
        for kname, kinds in _kinds(n, order).items():
            for cap in CAPS:
                what = (n, mname, kname, cap)
                out, _ = _probe(reg, mask, kinds, n, cap, grid)
                for w in range(1, 4):   # every wave of a workgroup derives the same
                    assert np.array_equal(out[:, w, :], out[:, 0, :]), what + ("wave %d" % w, np.flatnonzero((out[:, w, :] != out[:, 0, :]).any(1))[:8])
                got = out[:, 0, :]
                ref = _reference(mask, cap, grid)
                active = np.flatnonzero(mask)
                assert np.array_equal(got[:, 3], ref[:, 3]), what   # n_active, everywhere
                served = got[:, 0] >= 0
                assert np.array_equal(served, ref[:, 0] >= 0), what   # the same workgroups have work: ranks 0 .. n_active - 1
                assert np.array_equal(got[served, 2], ref[served, 2]), what   # blocks_per_pair
                assert np.all(got[~served, :3] == -1), what
                if active.size == 0:
                    assert not served.any(), what
                    checked += 1
                    continue
                per = max(1, min(grid // active.size, cap))
                # the multiset of (pair, slice) is exactly {active pairs} x range(per), each once
                keys = np.sort(got[served, 0].astype(np.int64) * per + got[served, 1])
                want = np.sort((active.astype(np.int64)[:, None] * per + np.arange(per)[None, :]).ravel())
                assert np.all((got[served, 1] >= 0) & (got[served, 1] < per)), what
                assert np.array_equal(keys, want), what
                # walking blockIdx upward: the cost class never gets heavier, and inside a class the pair index never decreases
                cls = cls_of_kind[kinds[got[served, 0]]]
                assert np.all(np.diff(cls) >= 0), what
                same = np.diff(cls) == 0
                assert np.all(np.diff(got[served, 0])[same] >= 0), what
                # slices of a pair in order, and workgroup b serves slice b % per
                assert np.array_equal(got[served, 1], np.flatnonzero(served) % per), what
                if np.unique(kinds[active]).size == 1:   # nothing to order by: deal_workgroup's mapping, as the device derives it
                    plain = np.full((grid, 4, 4), -7, np.int32)
                    assert reg._lib.dgs_deal_probe(reg._h, mask.ctypes.data_as(C.c_void_p), n, cap, grid, plain.ctypes.data_as(C.c_void_p)) == 0, what
                    assert np.array_equal(out, plain), what
                    assert np.array_equal(got, ref), what
                checked += 1
    assert checked == 6 * 7 * 2
