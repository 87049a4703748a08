"""-m gpu: the block reduction behind an upstream-order NDT evaluation (strict_block_row, delta_graph_slam_amd/csrc/ndt_strict.h) in passes
as wide as the item-compacted kernel's table region allows (22 columns) against the stand-alone form's passes of 11 columns, through the
test hook dgs_strict_row_probe: one workgroup over a caller-given [256][43] matrix of per-thread totals, both forms in one launch.

The width of a pass must not enter the sums: a column is added by one lane over its wave's 64 entries in thread order, the four waves'
sums as ((w0 + w1) + w2) + w3.  Every column of the matrix spans more than 2^53 in magnitude and mixes signs, so that a sum in any other
association rounds differently -- checked here on the CPU: the pairwise sum of the same matrix differs from the lane-order sum."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BLOCK, ACCUM, PAD, WAVE = 256, 43, 48, 64


def _matrix(seed=7):
    rng = np.random.default_rng(seed)
    # magnitudes 2^-40 .. 2^40 (a span of 2^80 > 2^53) with 53 random mantissa bits and random signs, every column alike
    m = rng.uniform(1.0, 2.0, (BLOCK, ACCUM)) * np.exp2(rng.integers(-40, 41, (BLOCK, ACCUM)).astype(np.float64))
    return np.ascontiguousarray(m * rng.choice((-1.0, 1.0), (BLOCK, ACCUM)))


def _lane_order(m, ncol):
    """The reduction as specified: per wave 0.0 + e0 + e1 + ... + e63 in thread order, then ((w0 + w1) + w2) + w3."""
    row = np.zeros(PAD)
    for c in range(ncol):
        w = []
        for k in range(BLOCK // WAVE):
            v = 0.0
            for x in m[k * WAVE:(k + 1) * WAVE, c]:
                v = v + float(x)
            w.append(v)
        row[c] = ((w[0] + w[1]) + w[2]) + w[3]
    return row


def _pairwise(m, ncol):
    row = np.zeros(PAD)
    for c in range(ncol):
        v = m[:, c].copy()
        while v.size > 1:
            v = v[0::2] + v[1::2]
        row[c] = v[0]
    return row


@pytest.fixture(scope="module")
def reg():
    from delta_graph_slam_amd.registration import Registration
    r = Registration("NDT_OMP")
    yield r
    r.close()


@pytest.fixture(scope="module")
def matrix():
    m = _matrix()
    assert (np.log2(np.abs(m).max(0) / np.abs(m).min(0)) > 53).all() and ((m > 0).any(0) & (m < 0).any(0)).all()
    return m


def test_the_matrix_tells_associations_apart(matrix):
    a, b = _lane_order(matrix, ACCUM), _pairwise(matrix, ACCUM)
    assert (a[:ACCUM] != b[:ACCUM]).sum() >= ACCUM // 2, "a pairwise sum of this matrix should differ from the lane-order sum in most columns"


@pytest.mark.parametrize("ncol", [7, 43])
def test_wide_passes_give_the_bits_of_the_11_column_form(reg, matrix, ncol):
    rows = np.full((2, PAD), np.nan)
    rc = reg._lib.dgs_strict_row_probe(reg._h, matrix.ctypes.data_as(C.c_void_p), ncol, rows.ctypes.data_as(C.c_void_p))
    assert rc == 0, rc
    wide, narrow = rows
    assert np.array_equal(wide, narrow), (ncol, np.flatnonzero(wide != narrow))
    assert not wide[ncol:].any(), ncol
    assert np.array_equal(wide, _lane_order(matrix, ncol)), ncol
