"""What the information-matrix tests share: a float64 restatement of the reference's weights and matrices
(src/hdl_graph_slam/information_matrix_calculator.cpp:53-75,110-157, include/hdl_graph_slam/information_matrix_calculator.hpp:46-54),
the test scene with its edges, the CPU oracle's answers (computed once per process), and the C++ driver's file format."""
from __future__ import annotations

import functools
import math
import os
import struct
import subprocess
from types import SimpleNamespace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DBL_MAX = 1.7976931348623157e308
# |score - oracle| <= TOL * score (tests/test_ndt_gpu.py:186).  Both sides add the same float distances in double; only the order
# differs, and the worst-case reordering error of a sum of N non-negative terms is N * 2^-53 relative: 9.1e-13 at N = 8,192.
TOL = 1e-12

DEFAULTS = dict(use_const_inf_matrix=False, const_stddev_x=0.5, const_stddev_q=0.1, var_gain_a=20.0, min_stddev_x=0.1, max_stddev_x=5.0,
                min_stddev_q=0.05, max_stddev_q=0.2, fitness_score_thresh=0.5, delta_var_gain_a=20.0, delta_min_stddev_x=0.1,
                delta_max_stddev_x=5.0, delta_min_stddev_q=0.05, delta_max_stddev_q=0.2, delta_avg_fitness_score=0.5,
                delta_importance_ratio_global=1.0, delta_importance_ratio_local=1.0)


# ---------------------------------------------------------------------------------------------- the reference's arithmetic
def _exp(x):
    try:
        return math.exp(x)
    except OverflowError:
        return math.inf


def weight(a, max_x, min_y, max_y, x):
    y = (1.0 - _exp(-a * x)) / (1.0 - _exp(-a * max_x))
    return min_y + (max_y - min_y) * y


def b_weight(a, avg_x, min_y, max_y, x):
    e = _exp(a * (x - avg_x))
    y = e / (e + 1.0) if e != math.inf else math.nan
    return min_y + (max_y - min_y) * y


def _f32(x):
    return float(np.float32(x))   # `float w_x = weight(...)`


def _diag(wx, wq):
    inf = np.eye(3)
    inf[:2, :2] /= wx
    inf[2, 2] /= wq
    return inf


def information_matrix(p, fitness):
    """.cpp:53-75 behind calc_fitness_score"""
    p = {**DEFAULTS, **p}
    if p["use_const_inf_matrix"]:
        return _diag(p["const_stddev_x"], p["const_stddev_q"])
    wx = _f32(weight(p["var_gain_a"], p["fitness_score_thresh"], p["min_stddev_x"] ** 2, p["max_stddev_x"] ** 2, fitness))
    wq = _f32(weight(p["var_gain_a"], p["fitness_score_thresh"], p["min_stddev_q"] ** 2, p["max_stddev_q"] ** 2, fitness))
    return _diag(wx, wq)


def information_matrix_buildings_global(p, fitness):
    """.cpp:110-132: the constant matrix is returned undivided"""
    p = {**DEFAULTS, **p}
    if p["use_const_inf_matrix"]:
        return _diag(p["const_stddev_x"], p["const_stddev_q"])
    return information_matrix(p, fitness) / p["delta_importance_ratio_global"]


def information_matrix_buildings_local(p, avg_distance, coverage_percentage, is_edge_aligned):
    """.cpp:134-157: no use_const_inf_matrix branch; the edge factor first, then the coverage factor"""
    p = {**DEFAULTS, **p}
    wx = _f32(b_weight(p["delta_var_gain_a"], p["delta_avg_fitness_score"], p["delta_min_stddev_x"] ** 2, p["delta_max_stddev_x"] ** 2, avg_distance))
    wq = _f32(b_weight(p["delta_var_gain_a"], p["delta_avg_fitness_score"], p["delta_min_stddev_q"] ** 2, p["delta_max_stddev_q"] ** 2, avg_distance))
    inf = _diag(wx, wq)
    if is_edge_aligned:
        inf = inf * p["delta_importance_ratio_local"]
    return inf * (coverage_percentage / 100.0)


def alignment(avg_distance, coverage_percentage, is_edge_aligned):
    """the fields of BestFitAlignment the local form reads"""
    return SimpleNamespace(fitness_score=SimpleNamespace(avg_distance=avg_distance, coverage_percentage=coverage_percentage), isEdgeAligned=is_edge_aligned)


# ---------------------------------------------------------------------------------------------- the scene
SUB_SIZES = (1, 8, 9, 64, 65, 512, 513)                           # index depths 1, 1, 1, 1, 2, 2, 3
SIZE_EDGES = (0, 1, 7, 8, 9, 31, 32, 33, 255, 256, 257)           # cloud2 sizes around a group, a wave, a workgroup's round
DEPTH_TARGETS = ("sub1", "sub65", "k0", "big")                    # one cloud1 per index depth 1 .. 4


@functools.lru_cache(maxsize=None)
def scene():
    """-> (clouds: name -> float32 [n, 4], poses: 6 x T_world_sensor).  k0 .. k5: six 16-beam street scans 2 m apart; sub<n>: the first n
    points of k0; big: k0 and k3 concatenated (more than 4,096 points: depth 4); e<n>: the first n points of k1; nonfinite: the first
    300 points of k1 with one NaN and one infinite point; empty."""
    from delta_graph_slam_amd import synth
    clouds, poses = {}, []
    for i in range(6):
        xyz, T = synth.street_scan((2.0 * i, 0.0, 0.0), 16, (2.0, -24.8), 256, 30 + i)
        c = np.ones((xyz.shape[0], 4), np.float32)
        c[:, :3] = xyz.astype(np.float32)
        clouds[f"k{i}"] = c
        poses.append(T)
    for n in SUB_SIZES:
        clouds[f"sub{n}"] = clouds["k0"][:n].copy()
    clouds["big"] = np.concatenate([clouds["k0"], clouds["k3"]])
    for n in SIZE_EDGES:
        clouds[f"e{n}"] = clouds["k1"][:n].copy()
    nf = clouds["k1"][:300].copy()
    nf[17, 1] = np.nan
    nf[203, 0] = np.inf
    clouds["nonfinite"] = nf
    clouds["empty"] = np.zeros((0, 4), np.float32)
    return clouds, poses


def relpose(i, j):
    """pose_i^-1 pose_j: cloud j in the frame of cloud i"""
    _, poses = scene()
    return np.linalg.inv(poses[i]) @ poses[j]


@functools.lru_cache(maxsize=None)
def main_edges():
    """(cloud1, cloud2, relpose) by name: the five odometry edges, two loop edges sharing key1, a self edge, one edge onto every
    sub-cloud and one onto the depth-4 cloud."""
    e = [(f"k{i}", f"k{i - 1}", relpose(i, i - 1)) for i in range(1, 6)]
    e += [("k5", "k0", relpose(5, 0)), ("k5", "k1", relpose(5, 1))]
    e += [("k2", "k2", np.eye(4))]
    e += [(f"sub{n}", "k1", relpose(0, 1)) for n in SUB_SIZES]
    e += [("big", "k1", relpose(0, 1))]
    return tuple(e)


N_ODOMETRY = 5
SELF_EDGE = 7


@functools.lru_cache(maxsize=None)
def size_edges():
    """every cloud2 size of SIZE_EDGES against every index depth"""
    return tuple((t, f"e{n}", relpose(0, 1)) for t in DEPTH_TARGETS for n in SIZE_EDGES)


@functools.lru_cache(maxsize=None)
def oracle_edges(which, max_range):
    """the CPU oracle's (score, used) of main_edges() / size_edges(), computed once"""
    from oracle import oracle as orc
    orc.build()
    clouds, _ = scene()
    edges = main_edges() if which == "main" else size_edges()
    out = []
    for c1, c2, T in edges:
        if clouds[c1].shape[0] == 0 or clouds[c2].shape[0] == 0:
            out.append((DBL_MAX, 0))
            continue
        s, used, _ = orc.fitness_score(clouds[c1], clouds[c2], np.asarray(T, np.float64).astype(np.float32), max_range)
        out.append((s, used))
    return tuple(out)


def index_depth(n):
    leaves, slots, depth = (n + 7) // 8, 8, 1
    while slots < leaves:
        slots *= 8
        depth += 1
    return depth


# ---------------------------------------------------------------------------------------------- the C++ driver
def build_driver(tmp_dir):
    exe = os.path.join(str(tmp_dir), "information_matrix_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "tests", "stub_pcl"),
                           os.path.join(ROOT, "tests", "cpp", "information_matrix_driver.cpp"), "-o", exe,
                           os.path.join(ROOT, "delta_graph_slam_amd", "libdgs_reg.so"), "-Wl,-rpath," + os.path.join(ROOT, "delta_graph_slam_amd"),
                           "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def write_driver_input(path, cloud_list, edges, tail4):
    """cloud_list: arrays; edges: (index1, index2, 4x4 relpose); tail4: fitness, avg_distance, coverage_percentage, isEdgeAligned"""
    with open(path, "wb") as f:
        f.write(struct.pack("<q", len(cloud_list)))
        for c in cloud_list:
            c = np.ascontiguousarray(c, np.float32).reshape(-1, 4)
            f.write(struct.pack("<q", c.shape[0]))
            f.write(c.tobytes())
        f.write(struct.pack("<q", len(edges)))
        for i, j, T in edges:
            f.write(struct.pack("<qq", i, j))
            f.write(np.ascontiguousarray(T, np.float64).reshape(16).tobytes())
        f.write(np.asarray(tail4, np.float64).tobytes())


def read_driver_output(path):
    """-> [k, 3, 3]"""
    return np.fromfile(path, np.float64).reshape(-1, 3, 3)
