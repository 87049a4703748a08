"""Test-side restatement of pcl::IterativeClosestPoint::computeTransformation with DefaultConvergenceCriteria, as ICP_HIP computes it
(DESIGN.md "ICP_HIP"): exact float 1-NN (oracle.knn: FLANN's distance order, ties to the lowest index), the `<=` distance gate squared in
double, optional reciprocal check, Kabsch in double with raw moments about the origin o = the target's first finite point, T_k rounded
to float, the float working copy and final transformation, and the criteria in PCL's order.  Returns the per-iteration trajectory for the GPU tests."""
from __future__ import annotations

import numpy as np

from helpers import f32_transform

DBL_MAX = np.finfo(np.float64).max


def _nn(orc, cloud, queries):
    if queries.shape[0] == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.float32)
    c = np.zeros((cloud.shape[0], 4), np.float32)
    c[:, :3] = cloud[:, :3]
    q = np.zeros((queries.shape[0], 4), np.float32)
    q[:, :3] = queries[:, :3]
    idx, d2 = orc.knn(c, q, 1)
    return idx[:, 0].astype(np.int64), d2[:, 0]


def kabsch(p, q, o):
    """Rigid T (float64 4x4) with q ~ R p + t over the pairs, accumulated about the origin o: H = sum p' q'^T - (sum p') cq'^T."""
    pp = p.astype(np.float64) - o
    qq = q.astype(np.float64) - o
    n = float(pp.shape[0])
    sp, sq = pp.sum(axis=0), qq.sum(axis=0)
    cp, cq = sp / n, sq / n
    H = pp.T @ qq - np.outer(sp, cq)
    U, _, Vt = np.linalg.svd(H)
    V = Vt.T.copy()
    if np.linalg.det(U) * np.linalg.det(V) < 0:
        V[:, 2] = -V[:, 2]
    R = V @ U.T
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = (cq + o) - R @ (cp + o)
    return T


def f32_matmul4(A, B):
    """float32 4x4 product, each entry ((a0 b0 + a1 b1) + a2 b2) + a3 b3, every operation rounded."""
    A = np.asarray(A, np.float32)
    B = np.asarray(B, np.float32)
    C = np.empty((4, 4), np.float32)
    for r in range(4):
        for c in range(4):
            C[r, c] = ((A[r, 0] * B[0, c] + A[r, 1] * B[1, c]) + A[r, 2] * B[2, c]) + A[r, 3] * B[3, c]
    return C


def icp_align(orc, tgt, src, guess=None, max_corr=2.5, transformation_epsilon=0.01, maximum_iterations=64, reciprocal=False,
              euclidean_fitness_epsilon=-DBL_MAX, rotation_epsilon=0.0, trace=None, nudge=0):
    """trace: a list that receives, per correspondence pass, dict(d2, keep, j, W) (tests/test_icp_gicp_edge_cases_cpu.py reads the
    margins of every decision there).  nudge = +1 / -1: every entry of T_k's three rows moved one float ulp up / down before it is used,
    the stability probe of the same file."""
    tgt = np.asarray(tgt, np.float32)[:, :3]
    src = np.asarray(src, np.float32)[:, :3]
    final = np.eye(4, dtype=np.float32) if guess is None else np.asarray(guess, np.float32).copy()
    W = f32_transform(final, src)
    max_sq = float(max_corr) * float(max_corr)
    rot_thr = rotation_epsilon if rotation_epsilon > 0 else 1.0 - transformation_epsilon
    finite = np.nonzero(np.isfinite(tgt).all(axis=1))[0]
    o = tgt[finite[0]].astype(np.float64) if finite.size else np.zeros(3)   # the target's first finite point
    prev_mse, mse = DBL_MAX, DBL_MAX
    iterations, evaluations, converged = 0, 0, False
    traj = []
    while True:
        evaluations += 1
        j, d2 = _nn(orc, tgt, W)
        keep = d2.astype(np.float64) <= max_sq     # a non-finite query (or none found: d2 = inf) is never kept
        if reciprocal:
            kept = np.nonzero(keep)[0]
            i2, d2r = _nn(orc, W, tgt[j[kept]])
            ok = (i2 == kept) & (d2r.astype(np.float64) <= max_sq)
            keep[kept[~ok]] = False
        n = int(keep.sum())
        if trace is not None:
            trace.append(dict(d2=d2.copy(), keep=keep.copy(), j=j.copy(), W=W.copy(), o=o.copy()))
        if n < 3:
            converged = False
            break
        Tk = kabsch(W[keep], tgt[j[keep]], o).astype(np.float32)
        if nudge:
            Tk[:3] = np.nextafter(Tk[:3], np.float32(np.inf if nudge > 0 else -np.inf))
        mse = float(d2[keep].astype(np.float64).sum() / n)
        W = f32_transform(Tk, W)
        final = f32_matmul4(Tk, final)
        iterations += 1
        traj.append((Tk.copy(), mse, n))
        T = Tk.astype(np.float64)
        if iterations >= maximum_iterations:
            converged = True
            break
        cos_angle = 0.5 * (((T[0, 0] + T[1, 1]) + T[2, 2]) - 1.0)
        tsq = (T[0, 3] * T[0, 3] + T[1, 3] * T[1, 3]) + T[2, 3] * T[2, 3]
        if cos_angle >= rot_thr and tsq <= transformation_epsilon:
            converged = True
            break
        d = abs(mse - prev_mse)
        if d < 1e-12 or d / prev_mse < euclidean_fitness_epsilon:
            converged = True
            break
        prev_mse = mse
    return dict(T=final, converged=converged, iterations=iterations, evaluations=evaluations, score=mse, traj=traj)
