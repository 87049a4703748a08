"""LoopDetector(batch_new_keyframes=True) against the sequential detector, with a fake registration that answers both call shapes from one
deterministic table keyed by (target id, source id): same loops, same final last_edge_accum_distance, one align_pairs_records call per
tick that has any pair.  No GPU."""
import numpy as np
import pytest

from delta_graph_slam_amd.loop_detector import KeyFrame, LoopDetector

N_TICKS = 200


def _table_row(tid, sid):
    """(converged, fitness, T) of registering keyframe `sid` against keyframe `tid`: a pure function of the two ids.  Fitness takes few
    values, so ties inside a candidate list are common (the later candidate must win), some of them above the threshold."""
    h = (tid * 7919 + sid * 104729) % 1000
    converged = h % 5 != 0
    fitness = (0.1, 0.3, 0.3, 0.45, 0.7, 0.1, 0.9)[h % 7]
    T = np.eye(4)
    T[:3, 3] = (0.01 * tid, 0.02 * sid, 0.001 * h)
    return converged, fitness, T


class FakeRegistration:
    """setInputTarget / align_batch_records and align_pairs_records over clouds that carry their keyframe id in element [0, 0]"""
    method = "FAST_GICP"

    def __init__(self):
        self.target = None
        self.batch_calls = 0
        self.pairs_calls = 0
        self.pairs_sizes = []

    @staticmethod
    def _records(tids, sids):
        out = np.full((len(sids), 20), -1.0)
        for j, (t, s) in enumerate(zip(tids, sids)):
            converged, fitness, T = _table_row(t, s)
            out[j, 1], out[j, 2], out[j, 3] = float(converged), fitness, 0.0
            out[j, 4:20] = T.reshape(16)
        return out

    def setInputTarget(self, cloud):
        self.target = int(cloud[0, 0])

    def align_batch_records(self, sources, guesses=None, compute_fitness=True, fitness_max_range=0.0):
        self.batch_calls += 1
        assert len(guesses) == len(sources)
        return self._records([self.target] * len(sources), [int(s[0, 0]) for s in sources])

    def align_pairs_records(self, targets, sources, guesses=None, compute_fitness=True, fitness_max_range=0.0):
        self.pairs_calls += 1
        self.pairs_sizes.append(len(sources))
        assert len(targets) == len(sources) == len(guesses) and len(sources) > 0
        return self._records([int(t[0, 0]) for t in targets], [int(s[0, 0]) for s in sources])


def _keyframe(kid, x, y, accum):
    est = np.eye(3)
    est[:2, 2] = (x, y)
    cloud = np.full((1, 4), float(kid), np.float32)
    return KeyFrame(cloud=cloud, estimate=est, accum_distance=accum, id=kid)


def _ticks(seed=1234):
    """A walk that keeps returning to the same block: per tick 0..5 new keyframes, steps of 0.3..4 m of accumulated distance (closer
    together and farther apart than min_edge_interval = 5), positions inside a 12 m square, so old keyframes are candidates again and
    again; some ticks have no candidates at all."""
    rng = np.random.default_rng(seed)
    keyframes, ticks, accum, kid = [], [], 0.0, 0
    for t in range(N_TICKS):
        new = []
        for _ in range(int(rng.integers(0, 6))):
            accum += float(rng.uniform(0.3, 4.0))
            x, y = rng.uniform(-6, 6, 2) if t % 9 else rng.uniform(40, 60, 2)   # every ninth tick far away: no candidates
            new.append(_keyframe(kid, x, y, accum))
            kid += 1
        ticks.append((list(keyframes), new))
        keyframes += new
    return ticks


def _run(detector, ticks):
    out = []
    for keyframes, new in ticks:
        out.append([(l.key1.id, l.key2.id, l.score, l.relative_pose.copy()) for l in detector.detect(keyframes, new)])
    return out


def _same(a, b):
    assert len(a) == len(b)
    for la, lb in zip(a, b):
        assert [(x[0], x[1], x[2]) for x in la] == [(x[0], x[1], x[2]) for x in lb]
        for x, y in zip(la, lb):
            assert np.array_equal(x[3], y[3])


def test_batched_ticks_give_the_sequential_loops():
    ticks = _ticks()
    seq_reg, bat_reg = FakeRegistration(), FakeRegistration()
    seq = LoopDetector(registration=seq_reg)
    bat = LoopDetector(registration=bat_reg, batch_new_keyframes=True)
    expected_calls = 0
    gated_inside_a_tick = ties = 0
    loops_seq, loops_bat = [], []
    for keyframes, new in ticks:
        # what the batched tick must register: every new keyframe that passes the gate with the PRE-tick value and has candidates
        pre = seq.last_edge_accum_distance
        probe = LoopDetector(registration=FakeRegistration())
        probe.last_edge_accum_distance = pre
        cands_of = {nk.id: probe.find_candidates(keyframes, nk) for nk in new}
        with_pairs = [nk for nk in new if cands_of[nk.id]]
        expected_calls += 1 if with_pairs else 0
        calls_before = bat_reg.pairs_calls
        loops_seq.append([(l.key1.id, l.key2.id, l.score, l.relative_pose.copy()) for l in seq.detect(keyframes, new)])
        loops_bat.append([(l.key1.id, l.key2.id, l.score, l.relative_pose.copy()) for l in bat.detect(keyframes, new)])
        assert bat_reg.pairs_calls - calls_before == (1 if with_pairs else 0)
        assert bat.last_edge_accum_distance == seq.last_edge_accum_distance
        accepted = {l[0] for l in loops_seq[-1]}
        first = min((nk.accum_distance for nk in with_pairs if nk.id in accepted), default=None)
        if first is not None:   # keyframes registered by the batch and then gated out by an acceptance earlier in the tick
            gated_inside_a_tick += sum(1 for nk in with_pairs if nk.accum_distance > first and nk.accum_distance - first < seq.distance_from_last_edge_thresh)
        for nk in with_pairs:
            cands = cands_of[nk.id]
            rec = FakeRegistration._records([nk.id] * len(cands), [c.id for c in cands])
            ok = rec[rec[:, 1] > 0.5, 2]
            ties += int(ok.size > 1 and (ok == ok.min()).sum() > 1)
    _same(loops_seq, loops_bat)
    assert bat_reg.pairs_calls == expected_calls and bat_reg.batch_calls == 0 and seq_reg.pairs_calls == 0
    # the input does exercise what it is meant to
    assert len(ticks) >= 200 and sum(len(l) for l in loops_seq) >= 20
    assert gated_inside_a_tick >= 5 and ties >= 5
    assert any(len(new) > 0 and n == 0 for (_, new), n in zip(ticks, [len(l) for l in loops_seq]))
    assert max(bat_reg.pairs_sizes) > 10


def test_a_tick_without_pairs_makes_no_call():
    reg = FakeRegistration()
    det = LoopDetector(registration=reg, batch_new_keyframes=True)
    old = [_keyframe(0, 0.0, 0.0, 1.0)]
    assert det.detect(old, []) == []
    assert det.detect(old, [_keyframe(1, 0.0, 0.0, 3.0)]) == []       # fails the last-edge gate
    assert det.detect(old, [_keyframe(2, 50.0, 50.0, 30.0)]) == []    # passes it, no candidates
    assert reg.pairs_calls == 0 and reg.batch_calls == 0


class _OtherMethod(FakeRegistration):
    method = "NDT_OMP"


class _Group(FakeRegistration):
    devices = (0, 1)

    def make_cloud(self, cloud, owner=None):
        return cloud


@pytest.mark.parametrize("make,why", [(_OtherMethod, "another method"), (_Group, "a group of devices"), (FakeRegistration, "the switch off: the default")])
def test_fallbacks_take_the_sequential_path(make, why):
    ticks = _ticks(seed=99)[:60]
    ref = _run(LoopDetector(registration=FakeRegistration()), ticks)
    reg = make()
    det = LoopDetector(registration=reg, batch_new_keyframes=(make is not FakeRegistration))
    _same(_run(det, ticks), ref)
    assert reg.pairs_calls == 0 and reg.batch_calls > 0, why


def test_a_registration_without_align_pairs_takes_the_sequential_path():
    class Plain:
        method = "FAST_GICP"

        def __init__(self):
            self.inner = FakeRegistration()
            self.setInputTarget = self.inner.setInputTarget
            self.align_batch_records = self.inner.align_batch_records

    ticks = _ticks(seed=7)[:60]
    ref = _run(LoopDetector(registration=FakeRegistration()), ticks)
    reg = Plain()
    _same(_run(LoopDetector(registration=reg, batch_new_keyframes=True), ticks), ref)
    assert reg.inner.batch_calls > 0 and reg.inner.pairs_calls == 0


def test_local_only_keeps_its_meaning_and_batches():
    ticks = _ticks(seed=5)[:60]
    ref = _run(LoopDetector(registration=FakeRegistration()), ticks)
    reg = FakeRegistration()
    _same(_run(LoopDetector(registration=reg, batch_new_keyframes=True, local_only=True), ticks), ref)
    assert reg.pairs_calls > 0 and reg.batch_calls == 0


def test_a_second_rank_or_a_forced_exchange_switches_the_batch_off(monkeypatch):
    det = LoopDetector(registration=FakeRegistration(), batch_new_keyframes=True)
    assert det._can_batch_tick()
    det.force_exchange = True
    assert not det._can_batch_tick()
    det.force_exchange = False
    monkeypatch.setattr(det, "_world", lambda: (0, 2))
    assert not det._can_batch_tick()
