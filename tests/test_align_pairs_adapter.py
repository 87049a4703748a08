"""dgs::HipRegistration::alignPairs (include/dgs/hip_registration.hpp) through tests/cpp/align_pairs_driver.cpp: it compiles against the
PCL-shape stubs and links with libdgs_reg.so, fails soft without a GPU, and on one gives the bits of the Python call on the same inputs."""
import json
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import align_pairs_scenes as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("align_pairs") / "align_pairs_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "tests", "stub_pcl"), "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "align_pairs_driver.cpp"), "-o", out,
                           os.path.join(ROOT, "delta_graph_slam_amd", "libdgs_reg.so"), "-Wl,-rpath," + os.path.join(ROOT, "delta_graph_slam_amd"),
                           "-Wl,-rpath,/opt/rocm/lib"])
    return out


def _write_input(path, clouds, pairs):
    with open(path, "wb") as f:
        f.write(struct.pack("<q", len(clouds)))
        for c in clouds:
            c = np.ascontiguousarray(c, np.float32).reshape(-1, 4)
            f.write(struct.pack("<q", c.shape[0]))
            f.write(c.tobytes())
        f.write(struct.pack("<q", len(pairs)))
        for t, s, g in pairs:
            f.write(struct.pack("<qq", t, s))
            f.write(np.ascontiguousarray(np.asarray(g, np.float32).T).tobytes())   # column-major, as Eigen holds it


def _run(driver, tmp_path, method, clouds, pairs):
    from delta_graph_slam_amd.registration import _RESULT_DTYPE
    pin, pout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    _write_input(pin, clouds, pairs)
    info = json.loads(subprocess.check_output([driver, method, pin, pout, str(S.DMAX)]).decode().strip().splitlines()[-1])
    return info, np.fromfile(pout, dtype=_RESULT_DTYPE)


def test_driver_compiles_links_and_fails_soft_without_a_gpu(driver, tmp_path):
    import torch
    clouds, pairs = S.distinct_pairs()
    info, rec = _run(driver, tmp_path, "FAST_GICP_HIP", [c[:256] for c in clouds], pairs[:2])
    assert info["pairs"] == 2
    if not torch.cuda.is_available():   # no device: never throws, nothing registered, the object's own result untouched
        assert info["ok"] is False and rec.size == 0 and info["own_untouched"] is True
    assert subprocess.call([driver, "BOGUS", str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], stdout=subprocess.DEVNULL) == 3


@pytest.mark.gpu
def test_driver_gives_the_bits_of_the_python_call(driver, tmp_path):
    clouds, pairs = S.distinct_pairs()
    clouds = clouds + [np.zeros((0, 4), np.float32)]
    pairs = pairs[:5] + [(1, len(clouds) - 1, np.eye(4, dtype=np.float32)), (len(clouds) - 1, 4, np.eye(4, dtype=np.float32))] + pairs[5:]
    info, rec = _run(driver, tmp_path, "FAST_GICP_HIP", clouds, pairs)
    assert info["ok"] is True and info["error"] == "" and info["repeat_equal"] is True and info["own_untouched"] is True
    res = S.make_registration().align_pairs([clouds[t] for t, _, _ in pairs], [clouds[s] for _, s, _ in pairs], [g for _, _, g in pairs])
    assert rec.shape == (len(pairs),)
    for k, r in enumerate(res):
        assert np.array_equal(rec["T"][k].reshape(4, 4).T, r["T"]), k
        assert (bool(rec["converged"][k]), rec["iterations"][k], rec["evaluations"][k], rec["status"][k]) == (r["converged"], r["iterations"], r["evaluations"], r["status"]), k
        assert np.array_equal(rec["score"][k:k + 1].view(np.uint64), np.float64([r["score"]]).view(np.uint64)), k
        assert np.array_equal(rec["fitness"][k:k + 1].view(np.uint64), np.float64([r["fitness"]]).view(np.uint64)), k
    assert rec["status"][5] == 4 and rec["status"][6] == 3
    # a handle of another method: the adapter's soft failure, with the method named
    info, rec = _run(driver, tmp_path, "NDT_HIP", clouds, pairs[:2])
    assert info["ok"] is False and "NDT" in info["error"] and rec.size == 0
