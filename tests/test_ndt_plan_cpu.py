"""CPU test of the NDT host driver's launch plan (delta_graph_slam_amd/csrc/ndt_plan.h): tests/cpp/ndt_plan_driver.cpp enumerates the cross
product of the handle knobs and parameters the plan depends on and checks every field, and the stream of every derivative launch, against
the expressions the driver used to repeat at each place of use.  Built with the address and undefined-behaviour sanitizers and run as a
program of its own."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def plan_report(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("ndt_plan") / "ndt_plan_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           os.path.join(ROOT, "tests", "cpp", "ndt_plan_driver.cpp"), "-o", exe])
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    out = run.stdout.decode()
    assert run.returncode == 0, out
    return json.loads(out.strip().splitlines()[-1])


def test_every_plan_field_equals_the_expression_it_replaced(plan_report):
    # 3 orders x kernel 2 / 3 x exp_libm x 3 voxel bounds x 2^8 flags x solve_min_active 0 / 2
    assert plan_report["cases"] == 3 * 2 * 2 * 3 * 2 ** 7 * 2
    assert plan_report["failures"] == 0


def test_launch_stream_is_the_stream_the_kernel_went_to(plan_report):
    """(launch < 0, 0, 5) x (hd or not) per case.  Where the profiler's stream and the launch's stream of the earlier driver differ -- the
    item-compacted kernel asked for a computeHessian launch of a fused round -- there is no launch at all and the driver never asks."""
    assert plan_report["stream_cases"] == 6 * plan_report["cases"]
    assert plan_report["pst_lst_disagree_launched"] == 0
