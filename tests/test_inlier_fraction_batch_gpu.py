"""-m gpu tests of Registration.calc_inlier_fraction_batch / dgs_calc_inlier_fraction_batch_clouds: the inlier count of
publish_scan_matching_status for many (keyframe, frame, pose) edges in one launch.  The count is an integer and must equal
dgs_get_inlier_fraction's for the same pair exactly."""
import numpy as np
import pytest

from delta_graph_slam_amd import synth
from tests import align_pairs_scenes as S

pytestmark = pytest.mark.gpu


def test_counts_equal_the_single_call_per_pair():
    """align_pairs_scenes.distinct_pairs() under its final transforms.  The registration is batch-independent, so the transform the single
    align leaves on its handle is, bit for bit, the one align_pairs reports: both counts are taken under the same pose."""
    clouds, pairs = S.distinct_pairs()
    reg = S.make_registration(batch_independent=True)
    res = reg.align_pairs([clouds[t] for t, _, _ in pairs], [clouds[s] for _, s, _ in pairs], [g for _, _, g in pairs], compute_fitness=False)
    dev = [reg.make_cloud(c) for c in clouds]
    Ts = [r["T"] for r in res]
    frac, cnt = reg.calc_inlier_fraction_batch([dev[t] for t, _, _ in pairs], [dev[s] for _, s, _ in pairs], Ts, 0.25, return_counts=True)
    counts = reg.fitness_batch_counts()
    assert counts["launches"] >= 2 and counts["host_waits"] == 1 and counts["edges"] == len(pairs) and counts["indices_built"] == 3   # the three targets, one build
    single = S.make_registration(batch_independent=True)
    for k, (t, s, g) in enumerate(pairs):
        single.setInputTarget(clouds[t])
        single.setInputSource(clouds[s])
        single.align(g)
        assert np.array_equal(single.getFinalTransformation(), Ts[k]), k
        f1 = single.getInlierFraction(0.25)
        print(f"pair {k}: inliers {cnt[k]} of {clouds[s].shape[0]}, fraction {frac[k]!r} / single {f1!r}")
        assert np.float64(f1).view(np.uint64) == np.float64(frac[k]).view(np.uint64), (k, f1, frac[k])
        assert cnt[k] == round(f1 * clouds[s].shape[0]) and 0 < cnt[k] <= clouds[s].shape[0]
    # the same edges in another order and alone: the same integers
    order = [7, 2, 9, 0, 4]
    f2, c2 = reg.calc_inlier_fraction_batch([dev[pairs[k][0]] for k in order], [dev[pairs[k][1]] for k in order], [Ts[k] for k in order], 0.25, return_counts=True)
    assert np.array_equal(c2, cnt[order]) and np.array_equal(f2, frac[order])
    f3, c3 = reg.calc_inlier_fraction_batch([dev[pairs[3][0]]], [dev[pairs[3][1]]], [Ts[3]], 0.25, return_counts=True)
    assert c3[0] == cnt[3] and f3[0] == frac[3]
    single.close()
    reg.close()


def test_threshold_equal_to_a_distance_is_strict_and_empty_clouds_give_nan():
    tgt, src, T = S.base()
    a, b = S.subset(tgt, 3000, 31), synth.apply_transform(T, S.subset(src, 1500, 32))   # b already in a's frame: the edge's pose is the identity
    reg = S.make_registration()
    reg.setInputTarget(a)
    _, sq = reg.nearestKSearch(b)            # the exact squared 1-NN distances, float32
    sq = np.asarray(sq, np.float32)
    v = np.sort(sq)[sq.size // 2]            # a threshold that IS one of the distances
    A, B, E = reg.make_cloud(a), reg.make_cloud(b), reg.make_cloud(np.zeros((0, 4), np.float32))
    below, upto = int((sq < v).sum()), int((sq <= v).sum())
    assert upto > below
    eye = np.eye(4, dtype=np.float32)
    frac, cnt = reg.calc_inlier_fraction_batch([A, E, A, A, A], [B, B, B, E, B], [eye] * 5, float(v), return_counts=True)
    print(f"threshold {v!r}: {cnt[0]} strictly below, {upto} up to it")
    assert cnt[0] == cnt[2] == cnt[4] == below and frac[0] == below / 1500
    assert cnt[1] == 0 and cnt[3] == 0 and np.isnan(frac[1]) and np.isnan(frac[3])      # empty cloud1 / empty cloud2: the other edges ran
    nxt = float(np.nextafter(v, np.float32(np.inf)))
    assert reg.calc_inlier_fraction_batch([A], [B], [eye], nxt, return_counts=True)[1][0] == upto
    assert reg.calc_inlier_fraction_batch([A], [B], [eye], 1e300, return_counts=True)[1][0] == 1500
    assert reg.calc_inlier_fraction_batch([], [], None).shape == (0,)
    with pytest.raises(Exception):
        reg.calc_inlier_fraction_batch([A], [B], [eye], float("nan"))
    reg.close()
