"""-m gpu: the closing of a fused upstream-order NDT launch (ndt_close_strict, delta_graph_slam_amd/csrc/ndt_strict.h) sums a pair's rows
as ndt_solve_kernel does for the unfused path (DGS_NDT_FUSED=0): five partial sums, sum g over the rows g, g + 5, ... four rows per step,
(((v + r0) + r1) + r2) + r3, then the five in order -- in the closing by five groups of threads, in ndt_solve_kernel by one thread per
column.  One pair alone, cut into exactly `rows` rows (DGS_NDT_CAP is read once per process, hence a fresh child process per case):
1 / 3 / 4 / 5 rows (a step of four partly filled, filled, one row into the second group), 19 / 20 / 21 (five groups x four rows minus one /
exact / plus one: the thread's second step), 128 (what a 65,536-point pair alone gets: 26 rows per thread).  The two paths' records --
transform, score, iterations, evaluations, convergence and the trajectory of poses -- must be the same bits.

Found by this file: ndt_solve_kernel used to add an order-1 pair's rows one after the other in slice order -- the closing's additions up to
five rows, another association above.  Measured with that form: 19 rows: the final score one ulp apart (0x410a953b507c0ab4 fused, ...b5
unfused); 20 and 21 rows: trajectories one to three ulps apart in some pose components; 128 rows: the score three ulps apart.
ndt_solve_kernel now forms the closing's five partial sums; the fused path, which is the one that is timed, keeps its bits."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS = (1, 3, 4, 5, 19, 20, 21, 128)

CHILD = r"""
import json, os, sys
import numpy as np
from delta_graph_slam_amd import synth
from delta_graph_slam_amd.registration import Registration

tgt, src, _ = synth.planar_pair(n=65536)
out = {}
for name, fused in (("fused", "1"), ("unfused", "0")):
    os.environ["DGS_NDT_FUSED"] = fused          # read at handle creation
    r = Registration("NDT_OMP", ndt_strict_order=1, ndt_resolution=1.0)
    r.setInputTarget(tgt)
    (x,) = r.align_batch([src], compute_fitness=False)
    traj = np.ascontiguousarray(r.ndt_trajectory(0), dtype=np.float64)
    out[name] = dict(status=int(x["status"]), converged=bool(x["converged"]), iterations=int(x["iterations"]), evaluations=int(x["evaluations"]),
                     score=np.float64(x["score"]).tobytes().hex(), T=np.ascontiguousarray(x["T"], dtype=np.float64).tobytes().hex(),
                     trajectory=traj.tobytes().hex(), trajectory_len=int(traj.shape[0]))
    r.close()
print("RECORDS " + json.dumps(out))
"""


@pytest.mark.parametrize("rows", ROWS)
def test_fused_closing_sums_like_the_solve_kernel(rows):
    env = dict(os.environ, DGS_NDT_CAP=str(rows))
    env.pop("DGS_NDT_FUSED", None)
    p = subprocess.run([sys.executable, "-c", CHILD], cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, (rows, p.stdout[-2000:], p.stderr[-2000:])
    line = [l for l in p.stdout.splitlines() if l.startswith("RECORDS ")][-1]
    rec = json.loads(line[len("RECORDS "):])
    fused, unfused = rec["fused"], rec["unfused"]
    assert fused["status"] == 0 and fused["iterations"] > 1 and fused["evaluations"] > fused["iterations"], (rows, fused)   # a real registration with line-search trials
    assert fused == unfused, (rows, {k: (fused[k], unfused[k]) for k in fused if fused[k] != unfused[k] and len(str(fused[k])) < 80})
