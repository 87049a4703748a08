"""Source / target generators that put the upstream-order NDT kernel (ndt_strict3_kernel, delta_graph_slam_amd/csrc/ndt_strict.h) at the
edges of its item loop: tile queue lengths of 0, < 64, exact multiples of 64 and the full PTS x NB, point counts on either side of the
kernel's own strides, empty waves inside active slices, points exactly on voxel faces, non-finite source points.

Plain numpy with fixed seeds, no GPU.  Every generator returns (target, source, claim): float32 [n, 4] clouds and a short statement of
the property it claims; tests/test_strict_edge_cases_cpu.py proves each claim on the CPU, tests/test_strict_edges_gpu.py runs the cases
against the oracle on the device.

The target of every case but `faces` is SOLID: the box of cells [-4, 4)^3 (in units of the resolution), every cell filled uniformly with
PER_CELL points, so every cell of the box is a valid voxel with a well-conditioned covariance (no eigenvalue clamp).  It spans the origin:
cell (0, 0, 0) is an interior cell of the grid.
"""
from __future__ import annotations

import numpy as np

RES_POW2 = 1.0      # the device multiplies by inv_leaf
RES_NPOW2 = 0.7     # the device divides by leaf, as the oracle does
RESOLUTIONS = (RES_POW2, RES_NPOW2)

BOX_LO, BOX_HI = -4, 4          # cells [BOX_LO, BOX_HI) per axis
PER_CELL = 24                   # target points per cell (>= 20)
INNER_LO, INNER_HI = BOX_LO + 1, BOX_HI - 2   # source cells: at least one cell from every face of the box
FRAC_LO, FRAC_HI = 0.1, 0.9     # source point inside its cell, in units of the resolution: 0.1 at identity, >= 0.05 after POSES[1]

# Identity and a small motion (translation / XYZ Euler angles as in NdtOracle.derivatives).  The motion moves a point of the box by
# < 0.03 m, so every solid-case point keeps its cell and a 0.05 * res margin to the cell's faces at both poses, for both resolutions.
POSES = (np.zeros(6), np.array([0.004, -0.003, 0.002, 0.001, -0.0015, 0.002]))

# Source sizes and the boundary each straddles.  One pair alone (ndt_derivatives) is cut into cap = max(ceil(n/512), min(64, ceil(n/256)))
# slices of 256 points (4 waves of 64), so up to 16,384 points a wave holds at most one 64-point sub-tile; the DIRECT7 / DIRECT1 tiles of
# 128 points (two sub-tiles, stride apart) start to fill beyond that.
SIZES = (
    1, 2,                 # one lane of one wave; every other wave of the workgroup empty
    63, 64, 65,           # the wave (64): DIRECT1 qn = 63 / 64 (exact multiple: no next-round DMA) / 64 + a wave with qn = 1
    127, 128, 129,        # the DIRECT7 tile (128 points): two waves, the second one full / one point in the third wave
    255, 256, 257,        # the workgroup (256): one slice, full / two slices (the second one point)
    511, 512, 513,        # two slices of 256 (cap = 2, 2, 3)
    4095, 4096, 4097,     # 16 slices / 17 slices, the last one point
    16385,                # cap = 64 slices, stride 16,384: the first point of a second sub-tile (slice 0, wave 0)
)
FULL_QUEUE_SIZES = (
    256,                  # DIRECT26 tile = 64 points x 27 = 1,728 items: the full queue, 27 rounds
    32768,                # cap = 64, stride 16,384: every DIRECT7 / DIRECT1 tile holds 128 points (896 / 128 items)
)
STRIPE = 64


def _xyz1(xyz) -> np.ndarray:
    out = np.ones((xyz.shape[0], 4), np.float32)
    out[:, :3] = xyz
    return out


def solid_target(res: float, seed: int = 1) -> np.ndarray:
    """PER_CELL points uniform in every cell of the box (within 0.02 * res of no face, so the float cell of each point is the intended one)."""
    rng = np.random.default_rng(seed)
    ax = np.arange(BOX_LO, BOX_HI)
    cells = np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), -1).reshape(-1, 3)
    c = np.repeat(cells, PER_CELL, 0).astype(np.float64)
    xyz = (c + rng.uniform(0.02, 0.98, c.shape)) * res
    return _xyz1(xyz[rng.permutation(xyz.shape[0])])


def _inner_points(rng, n, res):
    c = rng.integers(INNER_LO, INNER_HI + 1, (n, 3)).astype(np.float64)
    return (c + rng.uniform(FRAC_LO, FRAC_HI, (n, 3))) * res


def solid(n: int, res: float, seed: int = 2):
    """Every source point in an interior cell of the box, >= 0.05 * res from its cell's faces at every pose of POSES: 1 / 7 / 27 valid
    neighbours for DIRECT1 / DIRECT7 / DIRECT26.  DIRECT1: a wave's queue holds exactly its point count."""
    rng = np.random.default_rng(seed + n)
    return solid_target(res), _xyz1(_inner_points(rng, n, res)), "every point has 1/1, 7/7, 27/27 valid neighbours"


def outside(n: int, res: float, seed: int = 3):
    """The source lies wholly outside the target grid (> 2 cells beyond its +x face): no point has any item, every queue is empty."""
    rng = np.random.default_rng(seed + n)
    xyz = _inner_points(rng, n, res)
    xyz[:, 0] += (BOX_HI - INNER_LO + 3) * res
    return solid_target(res), _xyz1(xyz), "no point has a neighbour voxel"


def striped(n: int, res: float, seed: int = 4):
    """Consecutive 64-point blocks alternate between the solid interior (even blocks) and far outside the grid (odd blocks): the waves
    of odd blocks run tiles with qn = 0 between full ones."""
    _, src, _ = solid(n, res, seed)
    _, far, _ = outside(n, res, seed)
    odd = (np.arange(n) // STRIPE) % 2 == 1
    src[odd] = far[odd]
    return solid_target(res), src, "64-point blocks alternate: all neighbours / none"


def _on_faces(rng, n, res, lo, hi):
    """Coordinates exactly on cell faces in float32 (x / res == k, the test the device and the oracle make), one ulp off them, and
    interior values, mixed per coordinate; includes negative faces and -0.0."""
    r32 = np.float32(res)
    ks = np.arange(lo, hi + 1)
    face = (ks.astype(np.float32) * r32).astype(np.float32)
    face = face[(face / r32) == ks.astype(np.float32)]           # keep the products that divide back to the integer exactly
    pick = rng.integers(0, 4, (n, 3))
    f = face[rng.integers(0, face.size, (n, 3))]
    out = np.where(pick == 0, f, np.where(pick == 1, np.nextafter(f, np.float32(-np.inf)), np.where(pick == 2, np.nextafter(f, np.float32(np.inf)),
                                                                                                     _inner_points(rng, n, res).astype(np.float32))))
    out = out.astype(np.float32)
    out[::7, 0] = np.float32(-0.0)
    out[3::11, 1] = np.float32(-0.0)
    return out


def faces(n: int, res: float, seed: int = 5):
    """Target and source coordinates at exact multiples of the resolution (negative ones and -0.0 included), and one ulp beside them."""
    rng = np.random.default_rng(seed)        # the target does not depend on n
    tgt = solid_target(res)
    m = tgt.shape[0] // 6
    tgt[:m, :3] = _on_faces(rng, m, res, BOX_LO + 1, BOX_HI - 1)
    tgt = tgt[rng.permutation(tgt.shape[0])]
    rng = np.random.default_rng(seed + n)
    return tgt, _xyz1(_on_faces(rng, n, res, INNER_LO, INNER_HI + 1)), "coordinates exactly on voxel faces"


NONFINITE_AT = (17, 33, 40, 47, 90, 101)   # inside the first 128-point tile


def nonfinite(n: int, res: float, seed: int = 6):
    """The solid source with NaN / +-Inf coordinates at NONFINITE_AT (those below n): the oracle's semantics is that such a point
    contributes nothing."""
    tgt, src, _ = solid(n, res, seed)
    vals = ((0, np.nan), (1, np.inf), (2, -np.inf), (slice(0, 3), np.nan), (0, -np.inf), (1, np.nan))
    for i, (col, v) in zip(NONFINITE_AT, vals):
        if i < n:
            src[i, col] = v
    return tgt, src, "non-finite points contribute nothing"


CASES = {"solid": solid, "outside": outside, "striped": striped, "faces": faces, "nonfinite": nonfinite}

# the sizes each case runs at on the device (the solid case at every size, the others where their edge is)
CASE_SIZES = {
    "solid": SIZES + FULL_QUEUE_SIZES,
    "outside": (1, 64, 129, 4097),
    "striped": (127, 255, 257, 513, 4097, 16385, 32768),
    "faces": (512, 4097),
    "nonfinite": (128, 4097),
}
