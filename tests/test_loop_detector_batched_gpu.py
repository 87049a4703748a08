"""-m gpu: one synthetic tick through LoopDetector(batch_new_keyframes=True) on a real FAST_GICP registration against the sequential
detector: the same accepted (key1, key2), relative poses within the batch-against-single figures."""
import numpy as np
import pytest

from delta_graph_slam_amd import synth
from delta_graph_slam_amd.loop_detector import KeyFrame, LoopDetector
from tests import align_pairs_scenes as S
from tests.helpers import pose_error

pytestmark = pytest.mark.gpu

MARGIN = 1e-6   # relative: best against second-best fitness, and best fitness against the threshold, on every keyframe


def _se2(x, y, yaw):
    c, s = np.cos(yaw), np.sin(yaw)
    return np.array([[c, -s, x], [s, c, y], [0, 0, 1]], np.float64)


def _tick():
    """8 old keyframes and 4 new ones that all see the same planar scene from slightly different poses (4,096 points each, drawn apart);
    the new keyframes lie 0.5 to 6 m of accumulated distance apart, so the second is gated out by the first's loop and the last two are
    not; each has 2 or 3 candidates (the old keyframes within distance_thresh of it)."""
    world, _, _ = synth.planar_pair(n=8192)
    rng = np.random.default_rng(77)

    def keyframe(kid, x, y, yaw, accum, sigma):
        est = _se2(x, y, yaw)
        T = np.eye(4)
        T[:2, :2], T[:2, 3] = est[:2, :2], est[:2, 2]
        pts = S.subset(world, 4096, 1000 + kid)
        pts[:, :3] += rng.normal(0.0, sigma, (4096, 3)).astype(np.float32)   # a noisier keyframe scores worse: the fitness values are well apart
        return KeyFrame(cloud=synth.apply_transform(np.linalg.inv(T), pts).astype(np.float32), estimate=est + 0.0, accum_distance=accum, id=kid)

    # old keyframes in three places 8 m apart (distance_thresh is 5): 0-2, 3-4 and 5-7; the new ones come back to them in turn
    place = [0, 0, 0, 1, 1, 2, 2, 2]
    old = [keyframe(k, 8.0 * place[k] + 0.3 * (k % 3), -0.2 * (k % 3), 0.01 * k, 2.0 * k, 0.01 + 0.01 * k) for k in range(8)]
    new = [keyframe(8, 0.5, 0.3, 0.02, 40.0, 0.01), keyframe(9, 0.7, 0.2, 0.03, 40.5, 0.01),
           keyframe(10, 8.3, 0.2, -0.02, 46.0, 0.01), keyframe(11, 16.2, -0.3, 0.04, 52.0, 0.01)]
    for k, nk in enumerate(new):   # odometry drift: the estimate is off, so the guess is not the answer
        nk.estimate = nk.estimate @ _se2(0.05 * (k + 1), -0.04, 0.004 * (k + 1))
    return old, new


def _detector(batch):
    params = dict(distance_thresh=5.0, accum_distance_thresh=15.0, min_edge_interval=5.0, fitness_score_thresh=0.5)
    return LoopDetector(params, registration=S.make_registration(), cache_clouds=True, batch_new_keyframes=batch)


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
    loops_bat = bat.detect(old, new)
    assert [(l.key1.id, l.key2.id) for l in loops_bat] == [(l.key1.id, l.key2.id) for l in loops_seq]
    assert bat.last_edge_accum_distance == seq.last_edge_accum_distance
    for a, b in zip(loops_bat, loops_seq):
        dt, dr = pose_error(a.relative_pose, b.relative_pose)
        assert dt <= S.POSE_TOL[0] and dr <= S.POSE_TOL[1], (a.key1.id, dt, dr)
        assert abs(a.score - b.score) <= S.FIT_RTOL * abs(b.score)
