"""dgs::HipRegistration::alignPairs on a GICP_HIP object through tests/cpp/align_pairs_driver.cpp, the way tests/test_align_pairs_adapter.py
runs it for FAST_GICP: it compiles against the PCL-shape stubs and links with libdgs_reg.so, fails soft without a GPU, and on one gives the
bits of the Python call on the same inputs."""
import numpy as np
import pytest

from delta_graph_slam_amd import synth
from test_align_pairs_adapter import _run, driver  # noqa: F401  (driver: the fixture that builds the binary)

DMAX = 2.0   # what test_align_pairs_adapter._run hands the driver as reg_max_correspondence_distance (align_pairs_scenes.DMAX)


def _scene():
    """3 targets of 500 / 4,096 / 3,000 points and 4 sources out of synth.planar_pair(4096), an empty cloud, 6 interleaved pairs"""
    tgt, src, _ = synth.planar_pair(4096)
    rng = np.random.default_rng(21)
    sub = lambda c, m: c[rng.permutation(c.shape[0])[:m]].copy()   # noqa: E731
    clouds = [sub(tgt, 500), np.ascontiguousarray(tgt, np.float32), sub(tgt, 3000)] + [sub(src, m) for m in (257, 900, 1500, 2048)]
    clouds.append(np.zeros((0, 4), np.float32))
    g = lambda: synth.make_transform(rng.uniform(-0.15, 0.15, 3), rng.uniform(-0.02, 0.02, 3)).astype(np.float32)   # noqa: E731
    pairs = [(k % 3, 3 + k % 4, g()) for k in range(6)]
    return clouds, pairs


def test_driver_compiles_links_and_fails_soft_without_a_gpu(driver, tmp_path):   # noqa: F811
    import torch
    clouds, pairs = _scene()
    info, rec = _run(driver, tmp_path, "GICP_HIP", [c[:256] for c in clouds], pairs[:2])
    assert info["pairs"] == 2
    if not torch.cuda.is_available():   # no device: never throws, nothing registered, the object's own result untouched
        assert info["ok"] is False and rec.size == 0 and info["own_untouched"] is True


@pytest.mark.gpu
def test_driver_gives_the_bits_of_the_python_call(driver, tmp_path):   # noqa: F811
    from delta_graph_slam_amd.registration import Registration
    clouds, pairs = _scene()
    e = len(clouds) - 1
    pairs = pairs[:3] + [(1, e, np.eye(4, dtype=np.float32)), (e, 4, np.eye(4, dtype=np.float32))] + pairs[3:]
    info, rec = _run(driver, tmp_path, "GICP_HIP", clouds, pairs)
    assert info["ok"] is True and info["error"] == "" and info["repeat_equal"] is True and info["own_untouched"] is True
    reg = Registration("GICP_HIP", device=0, gicp_max_correspondence_distance=DMAX)
    res = reg.align_pairs([clouds[t] for t, _, _ in pairs], [clouds[s] for _, s, _ in pairs], [g for _, _, g in pairs])
    assert rec.shape == (len(pairs),)
    for k, r in enumerate(res):
        assert np.array_equal(rec["T"][k].reshape(4, 4).T, r["T"]), k
        assert (bool(rec["converged"][k]), rec["iterations"][k], rec["evaluations"][k], rec["status"][k]) == (r["converged"], r["iterations"], r["evaluations"], r["status"]), k
        assert np.array_equal(rec["score"][k:k + 1].view(np.uint64), np.float64([r["score"]]).view(np.uint64)), k
        assert np.array_equal(rec["fitness"][k:k + 1].view(np.uint64), np.float64([r["fitness"]]).view(np.uint64)), k
    assert rec["status"][3] == 4 and rec["status"][4] == 3
    assert all(rec["status"][k] == 0 and rec["converged"][k] for k in (0, 1, 2, 5, 6, 7))
