"""CPU test of the sample-consensus core both RANSAC stages share (delta_graph_slam_amd/csrc/sac.h): tests/cpp/sac_driver.cpp runs the draw
stream, computeModel's walk, its bookkeeping around a draw list and the draw-list size policy for 2-point (line) and 3-point (plane)
samples, against the two numpy restatements.  Built with the address and undefined-behaviour sanitizers and run as a program of its own."""
import math
import os
import subprocess

import numpy as np
import pytest

import floor_detection_reference as FR
import line_extraction_reference as LR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INT_MAX = 2**31 - 1
K_MARGIN = 1e-6      # test_floor_detection_cpu's: a walk decision `it < k` closer to a tie than this may hang on libm's last bit
OK, FAILED, NEED_DRAWS = 0, 1, 2
STREAM = {2: LR.draw_stream, 3: FR.draw_stream}


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("sac") / "sac_driver")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           os.path.join(ROOT, "tests", "cpp", "sac_driver.cpp"), "-o", exe])

    def run(commands):
        """-> one list of ints per command line"""
        r = subprocess.run([exe], input="\n".join(commands) + "\n", stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert r.returncode == 0, r.stdout
        rows = [[int(v) for v in ln.split()] for ln in r.stdout.splitlines()]
        assert len(rows) == len(commands), r.stdout
        return rows

    return run


@pytest.mark.parametrize("K", [2, 3])
def test_draws_follow_the_restatement_and_restore_the_permutation(driver, K):
    D = 300
    sizes = (K, K + 1, 1024, 30011)
    raws = [np.random.default_rng(1 + i).integers(0, 2**31, K * D, dtype=np.uint32) for i in range(len(sizes))]
    cmds, want = [], []
    for n, raw in zip(sizes, raws):        # one process: the permutation carries over from call to call, growing on the way
        for r in (None, raw):
            cmds.append(f"draws {K} {n} {D} " + ("0" if r is None else f"{r.size} " + " ".join(str(int(v)) for v in r)))
            st = STREAM[K](n, r)
            want.append([int(v) for _ in range(D) for v in next(st)])
    for n, row, exp in zip([n for n in sizes for _ in range(2)], driver(cmds), want):
        assert row[:-1] == exp, n
        assert row[-1] == 1, f"the permutation is not the identity after n = {n}"


def _line_margin(counts, n, max_iterations):
    """the smallest |k - it| over the `it < k` decisions of line_extraction_reference.walk (w * w, probability 0.99)"""
    it, k, best, margin = 0, 1.0, -INT_MAX, math.inf
    eps = np.finfo(np.float64).eps
    while True:
        margin = min(margin, abs(k - it))
        if not it < k:
            break
        c = counts[it]
        if c > best:
            best = c
            w = float(c) / float(n)
            k = float(np.log(1.0 - 0.99) / np.log(min(1.0 - eps, max(eps, 1.0 - w * w))))
        it += 1
        if it > max_iterations:
            break
    return margin


@pytest.mark.parametrize("K", [2, 3])
def test_walk_agrees_with_the_restatement(driver, K):
    rng = np.random.default_rng(2)         # the sequences of test_library_draw_list_and_walk_agree_with_the_restatement
    cmds, want, skipped = [], [], 0
    for trial in range(200):
        n = int(rng.integers(50, 5000))
        hi = int(rng.integers(1, n + 1))
        counts = rng.integers(0, hi + 1, 1200)
        mi = int(rng.choice([0, 1, 5, 1000]))
        if K == 3:
            win, it, margin, _ = FR.walk(counts, n, mi)
        else:
            win, it = LR.walk(counts, n, mi)
            margin = _line_margin(counts, n, mi)
        if margin <= K_MARGIN:             # libm's last bit could decide `it < k`
            skipped += 1
            continue
        cmds.append(f"walk {K} {n} {mi} {0.99!r} {counts.size} " + " ".join(str(int(c)) for c in counts))
        want.append([win, it, 0])
    assert skipped <= 2
    cmds.append(f"walk {K} 1000 1000 {0.99!r} 2 3 4")          # ran past the counts with the loop still open
    want.append([1, 2, 1])
    assert driver(cmds) == want


def test_list_bookkeeping(driver):
    cases = [
        # a hypothesis from draw `draw` with a run of bad draws completed at fail_at -> (loop goes on, status, draws)
        ("next 0 2147483647", [1, OK, 1]),
        ("next 41 2147483647", [1, OK, 42]),
        ("next 1029 1030", [1, OK, 1030]),
        ("next 1030 1030", [1, OK, 1031]),                  # draw == fail_at cannot happen (fail_at is a bad draw); it would not fail
        ("next 1031 1030", [0, FAILED, 1031]),              # draw == fail_at + 1: the run completed just before it
        ("next 5000 999", [0, FAILED, 1000]),
        # no further hypothesis in a list of D draws -> (status, draws)
        ("end 999 1064", [FAILED, 1000]),
        ("end 1063 1064", [FAILED, 1064]),                  # the run completes on the list's last draw
        ("end 1064 1064", [NEED_DRAWS, 1064]),              # it would complete on the first draw behind the list
        ("end 2147483647 1064", [NEED_DRAWS, 1064]),
        ("end 2147483647 1", [NEED_DRAWS, 1]),
    ]
    assert driver([c for c, _ in cases]) == [w for _, w in cases]


def test_draw_list_size_policy(driver):
    big = 2**31 - 1
    cases = [
        # avail max_hyp bad_run grows -> empty, first D, then (grew, D) per growth
        (f"plan {big} 1001 1000 6", [0, 1065, 1, 4260, 1, 17040, 1, 68160, 1, 272640, 1, 1002000, 1, 1002000]),   # the cap: 1001 * 1000 + 1000
        (f"plan {big} 1 1000 3", [0, 65, 1, 260, 1, 1040, 1, 2000]),
        ("plan 5000 1001 1000 3", [0, 1065, 1, 4260, 1, 5000, 0, 5000]),          # a short caller stream bounds the list, then is exhausted
        ("plan 400 1001 1000 1", [0, 400, 0, 400]),
        ("plan 1065 1001 1000 1", [0, 1065, 0, 1065]),
        ("plan 0 1001 1000 1", [1, 0, 0, 0]),                   # not a single draw
    ]
    assert driver([c for c, _ in cases]) == [w for _, w in cases]
