"""CPU proof that every case of tests/strict_edge_cases.py hits the edge it claims (tests/test_strict_edges_gpu.py runs them on the device).

Neighbour counts come from the independent float64 voxel model (oracle/ndt_ref.py: VoxelModel, neighbour_sets with 1, 7 or 27 offsets),
cross-checked against the CPU oracle's voxel table; margins and face positions are computed in float32 the way the device computes them."""
import itertools

import numpy as np
import pytest

from oracle import ndt_ref
from tests import strict_edge_cases as E
from tests.helpers import f32_transform

OFF1 = np.zeros((1, 3), int)
OFF7 = ndt_ref._OFF7
OFF27 = np.array(list(itertools.product((-1, 0, 1), repeat=3)))
N_BOX = (E.BOX_HI - E.BOX_LO) ** 3


def _counts(model, src, p, offsets):
    return np.array([len(s) for s in ndt_ref.neighbour_sets(model, src, p, offsets)])


@pytest.fixture(scope="module", params=E.RESOLUTIONS)
def model(request):
    res = request.param
    return res, ndt_ref.VoxelModel(E.solid_target(res), res)


def test_solid_target_is_a_box_of_valid_isotropic_voxels(model, oracle_lib):
    res, m = model
    assert len(m.cells) == N_BOX and min(c[3] for c in m.cells.values()) >= 20
    for mean, cov, icov, n in m.cells.values():
        ev = np.linalg.eigvalsh(cov)
        assert ev[0] > 0.1 * ev[2], "well conditioned: the 0.01 * lmax clamp never acts"
    assert list(m.min_b) == [E.BOX_LO] * 3 and list(m.max_b) == [E.BOX_HI - 1] * 3
    o = oracle_lib.NdtOracle(resolution=res)
    o.set_target(E.solid_target(res))
    v = o.voxels()
    assert int(v["valid"].sum()) == N_BOX
    # cell (0, 0, 0) is an interior valid cell: a non-finite coordinate that a float -> int conversion turned into 0 would land in the grid
    assert all(m.lookup(np.array(o3)) is not None for o3 in OFF27)


@pytest.mark.parametrize("n", [1, 65, 513, 4097])
def test_solid_every_point_has_every_neighbour(model, n):
    res, m = model
    _, src, _ = E.solid(n, res)
    p = E.POSES[0]
    assert (_counts(m, src, p, OFF1) == 1).all()
    assert (_counts(m, src, p, OFF7) == 7).all()
    assert (_counts(m, src, p, OFF27) == 27).all()


def _face_margin(res, src, p, oracle_lib):
    xt = f32_transform(oracle_lib.pose_to_matrix_f32(p), src[:, :3])
    u = (xt / np.float32(res)).astype(np.float64)
    frac = u - np.floor(u)
    return np.minimum(frac, 1.0 - frac).min(), np.floor(u)


@pytest.mark.parametrize("n", [1, 65, 513, 4097, 32768])
def test_solid_margin_to_the_faces_of_its_cell_at_every_pose(model, n, oracle_lib):
    """>= 0.05 * res from any face of its own cell, in float32 at every pose: the float and the double transform agree on the cell,
    and so the cells (and the neighbour counts above) are the same at both poses."""
    res, _ = model
    _, src, _ = E.solid(n, res)
    cells = []
    for p in E.POSES:
        marg, c = _face_margin(res, src, p, oracle_lib)
        assert marg >= 0.05, (res, n, marg)
        cells.append(c)
    assert np.array_equal(cells[0], cells[1])
    assert (cells[0] >= E.INNER_LO).all() and (cells[0] <= E.INNER_HI).all()


@pytest.mark.parametrize("n", [1, 129, 4097])
def test_outside_has_no_neighbour(model, n):
    res, m = model
    _, src, _ = E.outside(n, res)
    for p in E.POSES:
        assert (_counts(m, src, p, OFF27) == 0).all()


@pytest.mark.parametrize("n", [255, 513, 4097])
def test_striped_blocks_alternate_between_all_and_none(model, n):
    res, m = model
    _, src, _ = E.striped(n, res)
    odd = (np.arange(n) // E.STRIPE) % 2 == 1
    c7, c27 = _counts(m, src, E.POSES[0], OFF7), _counts(m, src, E.POSES[0], OFF27)
    assert (c7[~odd] == 7).all() and (c27[~odd] == 27).all()
    assert (c27[odd] == 0).all() and odd.any()


@pytest.mark.parametrize("res", E.RESOLUTIONS)
def test_faces_has_points_exactly_on_faces(res):
    r32 = np.float32(res)
    tgt, src, _ = E.faces(4097, res)
    faces = np.arange(E.BOX_LO, E.BOX_HI + 1, dtype=np.float32) * r32
    for cloud, share in ((tgt, 40), (src, 10)):
        xyz = cloud[:, :3]
        u = xyz / r32                                   # float32, as the device (x / leaf; x * inv_leaf is the same for 1.0) and the oracle
        on = u == np.floor(u)
        assert (on.sum(0) > cloud.shape[0] // share).all(), on.sum(0)
        assert ((xyz < 0) & on).any(), "negative faces"
        assert (np.isin(xyz, faces) & (xyz != 0)).any() and np.isin(np.nextafter(xyz, np.float32(np.inf)), faces).any(), "on a face, one ulp below one"
    assert (np.signbit(src[:, :3]) & (src[:, :3] == 0)).any(), "-0.0"


def test_nonfinite_points_are_where_the_case_says(oracle_lib):
    _, src, _ = E.nonfinite(4097, 1.0)
    bad = ~np.isfinite(src[:, :3]).all(1)
    assert list(np.flatnonzero(bad)) == list(E.NONFINITE_AT)
    assert np.isnan(src[:, :3]).any() and np.isposinf(src[:, :3]).any() and np.isneginf(src[:, :3]).any()
    for p in E.POSES:
        with np.errstate(invalid="ignore"):
            xt = f32_transform(oracle_lib.pose_to_matrix_f32(p), src[:, :3])
        assert (~np.isfinite(xt[bad])).all(1).all(), "every transformed coordinate of such a point is non-finite"


def test_sizes_straddle_the_kernel_strides():
    """The slice count of one pair (choose_launch, ndt_align.hip) at the listed sizes: a wave holds one 64-point sub-tile up to 16,384
    points, 16,385 opens a second sub-tile, 32,768 fills every 128-point tile."""
    def cap(n):
        return max(-(-n // 512), min(64, -(-n // 256)))
    for n in E.SIZES[:-1]:
        assert cap(n) * 256 >= n
    assert cap(16385) * 256 == 16384 and cap(32768) * 256 * 2 == 32768
    assert {63, 64, 65, 127, 128, 129, 255, 256, 257} <= set(E.SIZES)
    for case, sizes in E.CASE_SIZES.items():
        assert case in E.CASES and sizes
