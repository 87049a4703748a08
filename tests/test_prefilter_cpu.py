"""CPU tests of the prefilter chain (PrefilteringNodelet::cloud_callback): parameters and defaults against initialize_params
(apps/prefiltering_nodelet.cpp:55-109), the dgs_prefilter_params layout, the numpy restatement against independent float64
formulas, and the C++ adapter against the PCL-shape stubs."""
import ctypes as C
import json
import os
import subprocess
import tempfile

import numpy as np

import prefilter_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_params_defaults_are_initialize_params():
    from delta_graph_slam_amd import _lib as L
    from delta_graph_slam_amd.prefilter import params_from_dict
    lib = L.load()
    p = L.PrefilterParams()
    assert lib.dgs_prefilter_params_init(C.byref(p)) == 0
    assert p.struct_size == C.sizeof(L.PrefilterParams)
    assert p.downsample_method == L.PF_DOWNSAMPLE["VOXELGRID"] and p.downsample_resolution == 0.1
    assert p.outlier_removal_method == L.PF_OUTLIER["STATISTICAL"] and p.statistical_mean_k == 20 and p.statistical_stddev == 1.0
    assert p.radius_radius == 0.8 and p.radius_min_neighbors == 2
    assert p.use_distance_filter == 1 and p.distance_near_thresh == 1.0 and p.distance_far_thresh == 100.0
    assert p.radius_inclusive == int(R.RADIUS_INCLUSIVE) and p.statistical_sqrt_float == int(R.STATISTICAL_SQRT_FLOAT)
    assert lib.dgs_prefilter_params_init(None) == 1
    q = params_from_dict({})
    assert bytes(q) == bytes(p)
    q = params_from_dict(R.LAUNCH)
    assert q.outlier_removal_method == L.PF_OUTLIER["RADIUS"] and q.radius_radius == 0.5 and q.distance_near_thresh == 0.1
    assert q.statistical_mean_k == 30 and q.statistical_stddev == 1.2
    # unknown methods fall back to NONE (:71-76, :97-99); use_distance_filter is read and ignored (:100, :153)
    q = params_from_dict({"downsample_method": "OCTREE", "outlier_removal_method": "MEDIAN", "use_distance_filter": False})
    assert q.downsample_method == L.PF_DOWNSAMPLE["NONE"] and q.outlier_removal_method == L.PF_OUTLIER["NONE"] and q.use_distance_filter == 0


def test_prefilter_params_layout_matches_the_header():
    from delta_graph_slam_amd import _lib as L
    src = r'''
#include <stdio.h>
#include <stddef.h>
#include "dgs_reg.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(dgs_prefilter_params), offsetof(dgs_prefilter_params, downsample_resolution),
         offsetof(dgs_prefilter_params, outlier_removal_method), offsetof(dgs_prefilter_params, statistical_stddev),
         offsetof(dgs_prefilter_params, radius_radius), offsetof(dgs_prefilter_params, radius_min_neighbors),
         offsetof(dgs_prefilter_params, distance_near_thresh), offsetof(dgs_prefilter_params, distance_far_thresh),
         offsetof(dgs_prefilter_params, radius_inclusive), offsetof(dgs_prefilter_params, statistical_sqrt_float));
  return 0;
}'''
    with tempfile.TemporaryDirectory() as d:
        cfile = os.path.join(d, "t.c")
        open(cfile, "w").write(src)
        exe = os.path.join(d, "t")
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), cfile, "-o", exe])
        vals = [int(x) for x in subprocess.check_output([exe]).split()]
    P = L.PrefilterParams
    assert vals == [C.sizeof(P), P.downsample_resolution.offset, P.outlier_removal_method.offset, P.statistical_stddev.offset,
                    P.radius_radius.offset, P.radius_min_neighbors.offset, P.distance_near_thresh.offset, P.distance_far_thresh.offset,
                    P.radius_inclusive.offset, P.statistical_sqrt_float.offset]


def _patches(seed=0, n_patches=200):
    """Well-conditioned planar patches of 10 points (spread 1 m x 0.5 m, thickness 1 mm) at a few metres from the origin."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n_patches):
        A = np.linalg.qr(rng.normal(size=(3, 3)))[0]
        local = np.stack([rng.uniform(-0.5, 0.5, 10), rng.uniform(-0.25, 0.25, 10), rng.normal(0, 1e-3, 10)], 1)
        out.append(local @ A.T + rng.uniform(-3, 3, 3))
    return np.asarray(out, np.float32)


def test_restated_normals_agree_with_eigh_up_to_sign():
    P = _patches()
    cov = []
    for p in P:
        m = p.astype(np.float64).mean(0)
        cov.append(((p - m).T @ (p - m) / 10.0).reshape(9))
    cov = np.asarray(cov)
    with np.errstate(invalid="ignore", divide="ignore"):
        nv = R.eigen33_smallest(cov.astype(np.float32))
    w, V = np.linalg.eigh(cov.reshape(-1, 3, 3))
    ref = V[:, :, 0]
    dots = np.abs(np.sum(nv.astype(np.float64) * ref, 1))
    assert np.all(dots > 1 - 1e-5), dots.min()


def test_restated_normal_pass_on_patches_gives_the_plane_normal():
    P = _patches(1, 50)
    for p in P:
        cloud = np.ones((10, 4), np.float32)
        cloud[:, :3] = p
        with np.errstate(invalid="ignore", divide="ignore"):
            nv, cov, keep, band, _ = R.normals(cloud)
        m = p.astype(np.float64).mean(0)
        w, V = np.linalg.eigh((p - m).T @ (p - m))
        assert np.all(np.abs(np.abs(nv.astype(np.float64) @ V[:, 0]) - 1) < 1e-4)
        assert np.allclose(cov[0].reshape(3, 3), ((p - m).T @ (p - m) / 10.0), atol=1e-4)
        # flipped towards the viewpoint: (vp - p) . n >= 0
        assert np.all(np.sum(-cloud[:, :3] * nv, 1) >= 0)


def test_restated_statistical_threshold_is_mean_plus_std():
    rng = np.random.default_rng(3)
    d = rng.gamma(2.0, 0.05, 5000).astype(np.float32)
    mean, std, thr = R.statistical_threshold(d, 1.0)
    assert abs(mean - np.mean(d.astype(np.float64))) <= 1e-12 * mean
    assert abs(std - np.std(d.astype(np.float64), ddof=1)) <= 1e-9 * std
    assert abs(thr - (mean + std)) <= 1e-12 * thr


def test_restated_knn_and_outlier_filters_on_a_small_cloud():
    rng = np.random.default_rng(4)
    c = np.ones((400, 4), np.float32)
    c[:, :3] = rng.uniform(-2, 2, (400, 3))
    c[:5, :3] = [50, 50, 50]      # five coincident far points: each other's neighbours at distance 0
    idx, dd, _ = R.knn(c, 4)
    full = np.array([[np.sum((c[i, :3] - c[j, :3]) ** 2, dtype=np.float32) for j in range(400)] for i in range(20)])
    for i in range(20):
        o = np.lexsort((np.arange(400), full[i]))[:4]
        assert np.array_equal(idx[i], o)
    out, _ = R.radius_outlier_removal(c, 0.5, 2)
    assert any(np.array_equal(p, c[0]) for p in out)          # 2 neighbours at distance 0 within 0.5 m
    out, _ = R.radius_outlier_removal(c, 0.5, 5)
    assert not any(np.array_equal(p, c[0]) for p in out)      # only 4 others exist there
    out, st = R.statistical_outlier_removal(c, 8, 1.0)
    assert st["distances"].shape == (400,) and out.shape[0] < 400


def test_restated_distance_filter_drops_non_finite_points():
    c = np.array([[0.5, 0, 0, 1], [2, 0, 0, 1], [np.nan, 0, 0, 1], [np.inf, 0, 0, 1], [0, 0, 150, 1], [1, 0, 0, 1]], np.float32)
    out = R.distance_filter(c, 1.0, 100.0)
    assert np.array_equal(out, c[[1]])       # d == 1.0 is not > near


def test_cpp_prefilter_driver_builds_against_the_stubs(tmp_path):
    out = str(tmp_path / "prefilter_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "tests", "stub_pcl"), "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "prefilter_driver.cpp"), "-o", out,
                           os.path.join(ROOT, "delta_graph_slam_amd", "libdgs_reg.so"), "-Wl,-rpath," + os.path.join(ROOT, "delta_graph_slam_amd"),
                           "-Wl,-rpath,/opt/rocm/lib"])
    res = json.loads(subprocess.check_output([out, "params"]).decode().strip().splitlines()[-1])
    assert res == dict(downsample_method=1, downsample_resolution=0.1, outlier_removal_method=1, statistical_mean_k=20, statistical_stddev=1.0,
                       radius_radius=0.8, radius_min_neighbors=2, use_distance_filter=1, distance_near_thresh=1.0, distance_far_thresh=100.0)
    res = json.loads(subprocess.check_output([out, "params", "outlier_removal_method=RADIUS", "radius_radius=0.5", "downsample_method=APPROX_VOXELGRID",
                                              "distance_near_thresh=0.1"]).decode().strip().splitlines()[-1])
    assert res["outlier_removal_method"] == 2 and res["radius_radius"] == 0.5 and res["downsample_method"] == 2 and res["distance_near_thresh"] == 0.1
