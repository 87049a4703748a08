"""-m gpu: the synthetic tick of tests/test_loop_detector_batched_gpu.py through LoopDetector(batch_new_keyframes=True) on a GICP_HIP
registration against the sequential detector: the same accepted (key1, key2), relative poses bit-equal (GICP_HIP sums over fixed slices,
DESIGN.md 6o), the same final last_edge_accum_distance."""
import numpy as np
import pytest

from delta_graph_slam_amd.loop_detector import LoopDetector
from delta_graph_slam_amd.registration import Registration
from test_loop_detector_batched_gpu import MARGIN, _tick

pytestmark = pytest.mark.gpu

FIT_RTOL = 1e-9   # the edge scorer of align_pairs against the batch scorer of align_batch


def _detector(batch, method="GICP_HIP"):
    params = dict(distance_thresh=5.0, accum_distance_thresh=15.0, min_edge_interval=5.0, fitness_score_thresh=0.5)
    return LoopDetector(params, registration=Registration(method, device=0), cache_clouds=True, batch_new_keyframes=batch)


@pytest.mark.parametrize("method", ["GICP_HIP", "GICP_OMP_HIP"])
def test_batching_is_offered_for_gicp_hip(method):
    assert _detector(True, method)._can_batch_tick()


def test_one_batched_tick_gives_the_sequential_loops():
    old, new = _tick()
    seq, bat = _detector(False), _detector(True)
    # the sequential run is the reference: its records, keyframe by keyframe, must meet the margin condition
    loops_seq, n_candidates = [], []
    for nk in new:
        cands = seq.find_candidates(old, nk)
        loop = seq.matching(cands, nk)
        if cands:
            n_candidates.append(len(cands))
            rec = seq.last_records
            fit = np.sort(rec[rec[:, 1] > 0.5, 2])
            assert fit.size >= 2 and fit[1] - fit[0] > MARGIN * fit[1], (nk.id, fit)
            assert abs(fit[0] - seq.fitness_score_thresh) > MARGIN * seq.fitness_score_thresh, (nk.id, fit)
        if loop is not None:
            loops_seq.append(loop)
    assert len(n_candidates) == 3 and all(2 <= c <= 3 for c in n_candidates), n_candidates
    assert len(loops_seq) == 3     # a loop accepted early in the tick gates a later keyframe out
    calls = []
    pairs_call = bat.registration.align_pairs_records
    bat.registration.align_pairs_records = lambda *a, **kw: calls.append(len(a[0])) or pairs_call(*a, **kw)
    loops_bat = bat.detect(old, new)
    assert len(calls) == 1 and calls[0] >= sum(n_candidates)   # ONE device call for the tick (it also holds the pairs the replay gates out)
    assert [(l.key1.id, l.key2.id) for l in loops_bat] == [(l.key1.id, l.key2.id) for l in loops_seq]
    assert bat.last_edge_accum_distance == seq.last_edge_accum_distance
    for a, b in zip(loops_bat, loops_seq):
        assert np.array_equal(a.relative_pose, b.relative_pose), (a.key1.id, np.abs(a.relative_pose - b.relative_pose).max())
        assert abs(a.score - b.score) <= FIT_RTOL * abs(b.score)
