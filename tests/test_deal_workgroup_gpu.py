"""-m gpu: deal_workgroup (delta_graph_slam_amd/csrc/common.h) deals the workgroups of a launch to the active pairs of a batch.  It
counts the active pairs with one ballot per 64 pairs and then finds the pair of its rank; the ballots of the first 256 pairs are now kept
from the first pass instead of being evaluated (a load and its round trip) a second time.  The mapping must be what it always was, which
is stated here by definition: with A active pairs, blocks_per_pair = max(1, min(grid / A, cap_blocks)), workgroup b serves slice
b % blocks_per_pair of the (b / blocks_per_pair)-th active pair in index order, or nothing when that rank is >= A.

Through the test hook dgs_deal_probe (a kernel that calls deal_workgroup with the activity mask as its predicate and writes what EVERY
wave of every workgroup derived): n_pairs on either side of the 64-pair ballot and of the 256 kept pairs, masks that are empty, full,
alternating (both phases) and random, grids of 1024 + n_pairs workgroups, a cap that binds and one that does not."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N_PAIRS = (1, 5, 32, 64, 65, 200, 256, 257, 300)


def _reference(active, cap_blocks, grid):
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
            "random": (rng.random(n) < 0.3).astype(np.int32), "the last pair alone": last}


def test_dealing_is_the_rank_th_active_pair_for_every_wave():
    from delta_graph_slam_amd.registration import Registration
    r = Registration("NDT_OMP")
    checked = 0
    for n in N_PAIRS:
        grid = 1024 + n
        for name, mask in _masks(n).items():
            for cap in (1024, 3):
                out = np.full((grid, 4, 4), -7, np.int32)
                rc = r._lib.dgs_deal_probe(r._h, mask.ctypes.data_as(C.c_void_p), n, cap, grid, out.ctypes.data_as(C.c_void_p))
                assert rc == 0, (n, name, cap, rc)
                ref = _reference(mask, cap, grid)
                for w in range(4):
                    assert np.array_equal(out[:, w, :], ref), (n, name, cap, "wave %d" % w, np.flatnonzero((out[:, w, :] != ref).any(1))[:8])
                checked += 1
    assert checked == len(N_PAIRS) * 6 * 2
    r.close()
