"""pcl::VoxelGrid's grid from a box without a GPU: the host plan that the NDT target build, dgs_voxel_grid_filter and
dgs_cloud_assign_batch share, against hand-written expectations."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_grid_plan_against_hand_written_expectations(tmp_path):
    """voxel_grid_plan.h has no HIP in it: a plain g++ program includes it alone and checks min_b / div_b / mul1 / mul2 and the three
    states (empty, ok, too large) for a box with both signs at leaf 0.5, +-0.3 at leaf 0.1 (inexact inverse), the cubes of 1290 (fits)
    and 1291 cells (dense product over), truncated extents over, a single point, the start values +-FLT_MAX and a NaN in every place;
    built with the host sanitizers and run directly"""
    exe = str(tmp_path / "voxel_grid_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "delta_graph_slam_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "voxel_grid_plan_check.cpp"),
                           "-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 0 and p.stdout.strip().splitlines()[-1] == "ok", p.stdout + p.stderr

