"""GICP_HIP without a GPU: the C ABI's new enumerator / options struct / defaults, the Python and C++ factory branches (they reach
dgs_create and fail there for want of a device, unlike the reference's own "GICP" / "GICP_OMP"), and self-tests of the test-side
restatement tests/pcl_gicp_reference.py that the GPU tests compare against."""
import ctypes as C
import json
import math
import os
import subprocess
import tempfile

import numpy as np
import pytest

from helpers import f32_transform
import pcl_gicp_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _has_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


def test_params_init_pcl_gicp_defaults():
    from delta_graph_slam_amd import _lib as L
    lib = L.load()
    p = L.Params()
    assert L.METHOD_PCL_GICP == 4
    assert lib.dgs_params_init(C.byref(p), 4) == 0
    assert p.method == 4 and p.transformation_epsilon == 0.01 and p.maximum_iterations == 64
    assert p.gicp_max_correspondence_distance == 2.5 and p.gicp_correspondence_randomness == 20
    assert lib.dgs_params_init(C.byref(p), 7) != 0


def test_pcl_gicp_options_defaults_and_layout():
    from delta_graph_slam_amd import _lib as L
    lib = L.load()
    o = L.PclGicpOptions()
    assert lib.dgs_pcl_gicp_options_init(C.byref(o)) == 0
    assert o.struct_size == C.sizeof(L.PclGicpOptions)
    assert o.max_optimizer_iterations == 20 and o.rotation_epsilon == 2e-3 and o.gicp_epsilon == 1e-3 and o.use_reciprocal_correspondences == 0
    src = r'''
#include <stdio.h>
#include <stddef.h>
#include "dgs_reg.h"
int main(void) {
  dgs_pcl_gicp_options o;
  dgs_params p;
  int rc = dgs_pcl_gicp_options_init(&o);
  printf("%zu %zu %zu %zu %zu %zu %d %d %d %g %g %d %d %d\n", sizeof(dgs_pcl_gicp_options), offsetof(dgs_pcl_gicp_options, max_optimizer_iterations),
         offsetof(dgs_pcl_gicp_options, rotation_epsilon), offsetof(dgs_pcl_gicp_options, gicp_epsilon),
         offsetof(dgs_pcl_gicp_options, use_reciprocal_correspondences), sizeof(dgs_params), (int)DGS_METHOD_PCL_GICP, rc,
         o.max_optimizer_iterations, o.rotation_epsilon, o.gicp_epsilon, o.use_reciprocal_correspondences, dgs_params_init(&p, 7) != 0,
         dgs_abi_version());
  return 0;
}'''
    with tempfile.TemporaryDirectory() as d:
        cfile = os.path.join(d, "t.c")
        open(cfile, "w").write(src)
        exe = os.path.join(d, "t")
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), cfile, "-o", exe, os.path.join(ROOT, "delta_graph_slam_amd", "libdgs_reg.so"),
                               "-Wl,-rpath," + os.path.join(ROOT, "delta_graph_slam_amd"), "-Wl,-rpath,/opt/rocm/lib"])
        vals = subprocess.check_output([exe]).split()
    O = L.PclGicpOptions
    assert [int(v) for v in vals[:8]] == [C.sizeof(O), O.max_optimizer_iterations.offset, O.rotation_epsilon.offset, O.gicp_epsilon.offset,
                                          O.use_reciprocal_correspondences.offset, C.sizeof(L.Params), 4, 0]
    assert int(vals[8]) == 20 and float(vals[9]) == 2e-3 and float(vals[10]) == 1e-3 and int(vals[11]) == 0
    assert int(vals[12]) == 1 and int(vals[13]) == 5   # method 7 still rejected; the ABI version stays 5


def test_set_pcl_gicp_options_rejects_null():
    from delta_graph_slam_amd import _lib as L
    lib = L.load()
    o = L.PclGicpOptions()
    lib.dgs_pcl_gicp_options_init(C.byref(o))
    assert lib.dgs_set_pcl_gicp_options(None, C.byref(o)) == 1
    assert lib.dgs_group_set_pcl_gicp_options(None, C.byref(o)) == 1
    assert lib.dgs_pcl_gicp_set_probe(None, None, None) == 1


@pytest.mark.skipif(_has_gpu(), reason="the no-device failure path")
def test_gicp_hip_reaches_dgs_create_without_a_gpu():
    from delta_graph_slam_amd.registration import DgsError, Registration, select_registration_method
    for name in ("GICP_HIP", "GICP_OMP_HIP"):
        with pytest.raises(DgsError) as e:
            Registration(name, gicp_max_optimizer_iterations=5, gicp_rotation_epsilon=1e-3, gicp_epsilon=1e-4)
        assert e.value.status == 2
        with pytest.raises(DgsError) as e:
            select_registration_method({"registration_method": name, "reg_max_optimizer_iterations": 7})
        assert e.value.status == 2
    for name in ("GICP", "GICP_OMP"):
        with pytest.raises(NotImplementedError):
            select_registration_method({"registration_method": name})
    with pytest.raises(TypeError):
        Registration("FAST_GICP", gicp_max_optimizer_iterations=3)


def test_cpp_factory_builds_gicp_hip(tmp_path):
    out = str(tmp_path / "pcl_gicp_factory_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "tests", "stub_pcl"), "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "pcl_gicp_factory_driver.cpp"), "-o", out,
                           os.path.join(ROOT, "delta_graph_slam_amd", "libdgs_reg.so"), "-Wl,-rpath," + os.path.join(ROOT, "delta_graph_slam_amd"),
                           "-Wl,-rpath,/opt/rocm/lib"])
    for name in ("GICP_HIP", "GICP_OMP_HIP"):
        res = json.loads(subprocess.check_output([out, name]).decode().strip().splitlines()[-1])
        assert res["name"] == "dgs::HipRegistration<PCL_GICP>"
        assert res["method"] == 4
        assert res["transformation_epsilon"] == 0.001 and res["maximum_iterations"] == 32
        assert res["max_correspondence_distance"] == 1.5 and res["k"] == 15
        assert res["max_optimizer_iterations"] == 9 and res["reciprocal"] == 1
        assert res["rotation_epsilon"] == 2e-3 and res["gicp_epsilon"] == 1e-3
        assert res["plain_gicp_served"] == 0 and res["gicp_omp_served"] == 0


# ---- the restatement -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def orc():
    from oracle import oracle
    return oracle


def _planes(n, rng):
    """Points on three orthogonal planes (every neighbourhood has a clear normal) with a little noise."""
    k = n // 3
    a = np.c_[rng.uniform(-4, 4, k), rng.uniform(-4, 4, k), rng.normal(0, 0.01, k)]
    b = np.c_[rng.uniform(-4, 4, k), rng.normal(0, 0.01, k) + 3.0, rng.uniform(0, 3, k)]
    c = np.c_[rng.normal(0, 0.01, n - 2 * k) - 3.0, rng.uniform(-4, 4, n - 2 * k), rng.uniform(0, 3, n - 2 * k)]
    return np.vstack([a, b, c]).astype(np.float32)


def _motion(t, r):
    from delta_graph_slam_amd.synth import euler_to_matrix
    T = np.eye(4)
    T[:3, :3] = euler_to_matrix(*r)
    T[:3, 3] = t
    return T


def test_regularised_covariances_have_the_plane_normal_as_epsilon_direction(orc):
    rng = np.random.default_rng(1)
    xy = rng.uniform(-1, 1, (400, 2))
    pts = np.c_[xy, 0.3 * xy[:, 0] - 0.2 * xy[:, 1] + rng.normal(0, 1e-3, 400)].astype(np.float32)
    C, sv = ref.covariances(orc, pts, 20, 1e-3)
    normal = np.array([0.3, -0.2, -1.0])
    normal /= np.linalg.norm(normal)
    for i in range(0, 400, 37):
        s = np.linalg.svd(C[i], compute_uv=False)
        assert np.allclose(s, [1.0, 1.0, 1e-3], atol=1e-12)
        w, V = np.linalg.eigh(0.5 * (C[i] + C[i].T))
        assert abs(abs(V[:, 0] @ normal) - 1.0) < 1e-3   # the eps direction is the plane's normal
    assert np.all(sv[:, 0] >= sv[:, 1]) and np.all(sv[:, 1] >= sv[:, 2])


def test_analytic_gradient_matches_central_differences(orc):
    rng = np.random.default_rng(2)
    tgt = _planes(1500, rng)
    src = f32_transform(np.linalg.inv(_motion((0.1, -0.05, 0.02), (0.01, -0.02, 0.03))), tgt)
    Ct, _ = ref.covariances(orc, tgt, 20)
    Cs, _ = ref.covariances(orc, src, 20)
    guess = np.eye(4, dtype=np.float32)
    si, tj, M = ref.correspondences(orc, tgt, src, np.eye(4, dtype=np.float32), guess, Cs, Ct, 2.5)
    assert si.size > 1000
    P, Q = src[si], tgt[tj]
    # f of the float pipeline is piecewise constant at the float rounding of T(x): difference over steps far larger than that
    for x in (np.zeros(6), np.array([0.05, -0.02, 0.01, 0.01, -0.015, 0.02]), np.array([0.1, -0.05, 0.02, 0.01, -0.02, 0.03])):
        f, g = ref.evaluate(x, P, Q, M)
        for k in range(6):
            h = 1e-3
            xp, xm = x.copy(), x.copy()
            xp[k] += h
            xm[k] -= h
            num = (ref.evaluate(xp, P, Q, M)[0] - ref.evaluate(xm, P, Q, M)[0]) / (2 * h)
            assert abs(num - g[k]) <= 2e-3 * max(1.0, abs(g[k])) + 1e-3 * np.abs(g).max(), (x, k, num, g[k])


def test_line_searches_meet_the_strong_wolfe_conditions(orc):
    rng = np.random.default_rng(3)
    tgt = _planes(3000, rng)
    src = f32_transform(np.linalg.inv(_motion((0.2, -0.1, 0.05), (0.02, -0.01, 0.04))), tgt)
    r = ref.gicp_align(orc, tgt, src, transformation_epsilon=1e-6, maximum_iterations=10)
    via_sigma = [s for s in r["searches"] if s[6]]
    assert len(via_sigma) >= 5
    for status, alpha, f0, fp0, fa, fpa, _ in via_sigma:
        assert status == ref.SUCCESS and alpha > 0 and fp0 < 0
        assert fa <= f0 + ref.RHO * alpha * fp0                   # sufficient decrease
        assert abs(fpa) <= -ref.SIGMA * fp0                       # strong curvature condition


def test_reference_recovers_a_rigid_motion(orc):
    rng = np.random.default_rng(4)
    tgt = _planes(3000, rng)
    T = _motion((0.15, -0.08, 0.04), (0.015, -0.01, 0.03))
    src = f32_transform(np.linalg.inv(T), tgt)
    r = ref.gicp_align(orc, tgt, src, transformation_epsilon=1e-6, maximum_iterations=30)
    assert r["converged"] and r["iterations"] >= 2
    assert np.abs(r["T"].astype(np.float64) - T).max() < 1e-3
    assert len(r["traj"]) == r["iterations"]
    assert r["evaluations"] == r["iterations"] + sum(t["passes"] for t in r["traj"])
    assert all(1 <= t["inner"] <= 20 for t in r["traj"])
    assert r["score"] == r["traj"][-1]["f"]


def test_fewer_than_four_pairs_is_not_converged_with_final_equal_to_guess(orc):
    rng = np.random.default_rng(5)
    tgt = rng.uniform(-1, 1, (300, 3)).astype(np.float32)
    src = tgt + np.float32(50.0)
    src[:3] = tgt[:3]                                          # three pairs within the gate: still fewer than 4
    guess = np.eye(4, dtype=np.float32)
    guess[0, 3] = 0.01
    r = ref.gicp_align(orc, tgt, src, guess=guess)
    assert r["iterations"] == 0 and not r["converged"] and r["evaluations"] == 1
    assert np.array_equal(r["T"], guess)


def test_maximum_iterations_zero_still_runs_one_outer_iteration(orc):
    rng = np.random.default_rng(6)
    tgt = _planes(900, rng)
    src = tgt + np.float32(0.03)
    r = ref.gicp_align(orc, tgt, src, maximum_iterations=0)
    assert r["iterations"] == 1 and r["converged"]
    assert r["evaluations"] == 1 + r["traj"][0]["passes"]


def test_gate_is_strict(orc):
    tgt = np.array([[0, 0, 0], [10, 0, 0], [0, 10, 0], [0, 0, 10], [10, 10, 0], [10, 0, 10]], np.float32)
    src = tgt + np.array([2.0, 0, 0], np.float32)           # every d2 is exactly 4.0 = max_corr^2: none kept
    Ct = np.tile(np.eye(3), (6, 1, 1))
    si, _, _ = ref.correspondences(orc, tgt, src, np.eye(4, dtype=np.float32), np.eye(4, dtype=np.float32), Ct, Ct, 2.0)
    assert si.size == 0
    si, _, _ = ref.correspondences(orc, tgt, src, np.eye(4, dtype=np.float32), np.eye(4, dtype=np.float32), Ct, Ct, math.nextafter(2.0, 3.0))
    assert si.size == 6


def test_apply_state_round_trips_through_state_of():
    x = np.array([0.3, -0.2, 0.1, 0.05, -0.04, 0.7])
    T = ref.apply_state(x)
    R = T[:3, :3].astype(np.float64)
    assert np.abs(R @ R.T - np.eye(3)).max() < 1e-6
    y = ref.state_of(T)
    assert np.abs(y - x).max() < 1e-6
