"""Test-side restatement of pcl::GeneralizedIterativeClosestPoint<PointXYZ, PointXYZ>::computeTransformation, as GICP_HIP computes it
(DESIGN.md "GICP_HIP", every recalled detail marked [UPSTREAM-RECALL] there):

* computeCovariances: exact k-NN in the cloud itself (the point included), raw moments accumulated in double from float products,
  cov = S/k - mean mean^T, JacobiSVD U, C = sum_j v_j u_j u_j^T with v = (1, 1, gicp_epsilon).
* the outer loop: output = guess * source (float); R = top-left 3x3 of double(transformation_) * double(guess); per source point the
  exact float 1-NN of transformation_ * output[i] in the target with the strict gate (double) d2 < corr_dist^2, and
  M_i = ((R C1) R^T + C2)^-1 (Eigen's cofactor inverse); fewer than 4 pairs: stop, not converged.
* estimateRigidTransformationBFGS: pcl/registration/bfgs.h (GSL's vector_bfgs2 with the Fletcher line search of linear_minimize.c),
  rho = sigma = 0.01, tau1 = 9, tau2 = 0.05, tau3 = 0.5, cubic interpolation; testGradient(1e-2); applyState's float quaternion product.
* the convergence test on the 4 x 4 difference scaled by 1/rotation_epsilon and 1/transformation_epsilon; final = transformation_ * guess.

Every BFGS / line-search operation is sequential double arithmetic in a fixed order that csrc/pcl_gicp.hip repeats; the device's
per-point sums run in an order of their own, so f and g agree to rounding only."""
from __future__ import annotations

import math

import numpy as np

from helpers import f32_transform
from icp_reference import f32_matmul4

DBL_MAX = np.finfo(np.float64).max
DBL_EPS = float(np.finfo(np.float64).eps)
RHO, SIGMA, TAU1, TAU2, TAU3 = 0.01, 0.01, 9.0, 0.05, 0.5
LS_ITERS = 100                      # bracket_iters = section_iters, one counter shared by both phases
SUCCESS, NO_PROGRESS, RUNNING = 0, 1, -1
GRADIENT_EPS = 1e-2

f32 = np.float32


# ---- covariances ------------------------------------------------------------------------------------------------------------------
def covariances(orc, cloud, k, gicp_epsilon=1e-3):
    """PCL-style covariances (n, 3, 3) of every point of `cloud`; non-finite points get NaN (they never pair up, never are neighbours).
    Also returns the singular values of the raw k-NN covariance (n, 3), for the tests' degeneracy filter."""
    pts = np.asarray(cloud, np.float32)[:, :3]
    n = pts.shape[0]
    out = np.full((n, 3, 3), np.nan)
    sv = np.full((n, 3), np.nan)
    fin = np.nonzero(np.isfinite(pts).all(axis=1))[0]
    if fin.size == 0:
        return out, sv
    fp = np.ascontiguousarray(pts[fin])
    c4 = np.zeros((fp.shape[0], 4), np.float32)
    c4[:, :3] = fp
    idx, _ = orc.knn(c4, c4, k)
    nb = np.where((idx >= 0)[:, :, None], fp[np.clip(idx, 0, None)], f32(0))      # slots that found nothing are zero columns
    mean = nb.astype(np.float64).sum(axis=1)
    S = np.zeros((fp.shape[0], 3, 3))
    for l in range(3):
        for m in range(l + 1):
            S[:, l, m] = (nb[:, :, l] * nb[:, :, m]).astype(np.float64).sum(axis=1)   # products in float, sums in double
    mean = mean / float(k)
    cov = np.zeros_like(S)
    for l in range(3):
        for m in range(l + 1):
            cov[:, l, m] = S[:, l, m] / float(k) - mean[:, l] * mean[:, m]
            cov[:, m, l] = cov[:, l, m]
    U, s, _ = np.linalg.svd(cov)
    v = (1.0, 1.0, float(gicp_epsilon))
    C = np.zeros_like(cov)
    for j in range(3):
        u = U[:, :, j]
        C += (v[j] * u)[:, :, None] * u[:, None, :]
    out[fin] = C
    sv[fin] = s
    return out, sv


def inv3_eigen(A):
    """Eigen's 3 x 3 cofactor inverse, batched: inv(r, c) = cofactor(c, r) / det, det along column 0."""
    def cof(i, j):
        i1, i2, j1, j2 = (i + 1) % 3, (i + 2) % 3, (j + 1) % 3, (j + 2) % 3
        return A[..., i1, j1] * A[..., i2, j2] - A[..., i1, j2] * A[..., i2, j1]
    c0 = [cof(0, 0), cof(1, 0), cof(2, 0)]
    det = (c0[0] * A[..., 0, 0] + c0[1] * A[..., 1, 0]) + c0[2] * A[..., 2, 0]
    invdet = 1.0 / det
    out = np.empty_like(A)
    for r in range(3):
        for c in range(3):
            out[..., r, c] = cof(c, r) * invdet
    return out


# ---- applyState / the functor ---------------------------------------------------------------------------------------------------
def _qmul(a, b):   # Eigen's quaternion product, (w, x, y, z), every operation rounded to float
    aw, ax, ay, az = a
    bw, bx, by, bz = b
    return (aw * bw - ax * bx - ay * by - az * bz,
            aw * bx + ax * bw + ay * bz - az * by,
            aw * by + ay * bw + az * bx - ax * bz,
            aw * bz + az * bw + ax * by - ay * bx)


def _half(angle):
    ha = f32(0.5) * f32(angle)
    return f32(math.cos(float(ha))), f32(math.sin(float(ha)))


def apply_state(x):
    """applyState(I, x): AngleAxisf(x5, Z) * AngleAxisf(x4, Y) * AngleAxisf(x3, X) as float quaternions, toRotationMatrix, float t."""
    z0 = f32(0)
    cz, sz = _half(x[5])
    cy, sy = _half(x[4])
    cx, sx = _half(x[3])
    q = _qmul(_qmul((cz, sz * z0, sz * z0, sz), (cy, sy * z0, sy, sy * z0)), (cx, sx, sx * z0, sx * z0))
    w, qx, qy, qz = q
    tx, ty, tz = f32(2) * qx, f32(2) * qy, f32(2) * qz
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * qx, ty * qx, tz * qx
    tyy, tyz, tzz = ty * qy, tz * qy, tz * qz
    T = np.zeros((4, 4), np.float32)
    T[0] = (f32(1) - (tyy + tzz), txy - twz, txz + twy, f32(x[0]))
    T[1] = (txy + twz, f32(1) - (txx + tzz), tyz - twx, f32(x[1]))
    T[2] = (txz - twy, tyz + twx, f32(1) - (txx + tyy), f32(x[2]))
    T[3, 3] = 1
    return T


def state_of(T):
    """The BFGS start of estimateRigidTransformationBFGS: (t, atan2(r21, r22), asin(-r20), atan2(r10, r00)) of the float matrix,
    each angle through the float overloads (rounded to float)."""
    T = np.asarray(T, np.float32)
    return np.array([float(T[0, 3]), float(T[1, 3]), float(T[2, 3]),
                     float(f32(math.atan2(float(T[2, 1]), float(T[2, 2])))),
                     float(f32(math.asin(-float(T[2, 0])))),
                     float(f32(math.atan2(float(T[1, 0]), float(T[0, 0]))))])


def r_derivatives(x):
    """computeRDerivative's closed forms: dR/dphi, dR/dtheta, dR/dpsi (3 x 3 each), in double."""
    phi, theta, psi = x[3], x[4], x[5]
    cphi, sphi, cth, sth, cpsi, spsi = math.cos(phi), math.sin(phi), math.cos(theta), math.sin(theta), math.cos(psi), math.sin(psi)
    a = np.array([[0., sphi * spsi + cphi * cpsi * sth, cphi * spsi - cpsi * sphi * sth],
                  [0., -cpsi * sphi + cphi * spsi * sth, -cphi * cpsi - sphi * spsi * sth],
                  [0., cphi * cth, -cth * sphi]])
    b = np.array([[-cpsi * sth, cpsi * cth * sphi, cphi * cpsi * cth],
                  [-spsi * sth, cth * sphi * spsi, cphi * cth * spsi],
                  [-cth, -sphi * sth, -cphi * sth]])
    c = np.array([[-cth * spsi, -cphi * cpsi - sphi * spsi * sth, cpsi * sphi - cphi * spsi * sth],
                  [cpsi * cth, -cphi * spsi + cpsi * sphi * sth, sphi * spsi + cphi * cpsi * sth],
                  [0., 0., 0.]])
    return a, b, c


def inner_prod(dR, Rs):
    """matricesInnerProd(dR, Rs) = sum_ij dR(j, i) Rs(i, j) = tr(dR Rs), summed i-major."""
    r = 0.0
    for i in range(3):
        for j in range(3):
            r += dR[j, i] * Rs[i, j]
    return r


def evaluate(x, P, Q, M):
    """OptimizationFunctorWithIndices f and df at state x over the pairs (P = output points, Q = their target points, M = Mahalanobis)."""
    P = np.asarray(P, np.float32)[:, :3]
    Q = np.asarray(Q, np.float32)[:, :3]
    m = P.shape[0]
    T = apply_state(x)
    pp = f32_transform(T, P)
    res = pp.astype(np.float64) - Q.astype(np.float64)
    temp = (M[:, :, 0] * res[:, 0:1] + M[:, :, 1] * res[:, 1:2]) + M[:, :, 2] * res[:, 2:3]
    f = float(((res[:, 0] * temp[:, 0] + res[:, 1] * temp[:, 1]) + res[:, 2] * temp[:, 2]).sum()) / m
    g = np.zeros(6)
    g[:3] = temp.sum(axis=0) * (2.0 / m)
    Rs = (P.astype(np.float64)[:, :, None] * temp[:, None, :]).sum(axis=0) * (2.0 / m)
    for k, dR in enumerate(r_derivatives(x)):
        g[3 + k] = inner_prod(dR, Rs)
    return f, g


# ---- bfgs.h ---------------------------------------------------------------------------------------------------------------------
def _dot(a, b):
    r = 0.0
    for i in range(6):
        r += a[i] * b[i]
    return r


def _norm(a):
    return math.sqrt(_dot(a, a))


def _cubic(c0, c1, c2, c3, z):
    return c0 + z * (c1 + z * (c2 + z * c3))


def _cubicmin(f0, fp0, f1, fp1, zl, zh):
    eta = 3 * (f1 - f0) - 2 * fp0 - fp1
    xi = fp0 + fp1 - 2 * (f1 - f0)
    c0, c1, c2, c3 = f0, fp0, eta, xi
    zmin, fmin = zl, _cubic(c0, c1, c2, c3, zl)
    y = _cubic(c0, c1, c2, c3, zh)
    if y < fmin:
        zmin, fmin = zh, y
    # roots of c1 + 2 c2 z + 3 c3 z^2 (bfgs.h's PolynomialSolver<_, 2>): two real roots, one double root, or none
    a2, b1, c0p = 3 * c3, 2 * c2, c1
    roots = []
    if a2 != 0.0:
        disc = b1 * b1 - 4 * a2 * c0p
        if disc > 0:
            sd = math.sqrt(disc)
            r0, r1 = (-b1 - sd) / (2 * a2), (-b1 + sd) / (2 * a2)
            roots = [min(r0, r1), max(r0, r1)]
        elif disc == 0:
            roots = [-b1 / (2 * a2)]
    for z in roots:
        if zl < z < zh:
            y = _cubic(c0, c1, c2, c3, z)
            if y < fmin:
                zmin, fmin = z, y
    return zmin


def _interp_quad(f0, fp0, f1, zl, zh):
    fl = f0 + zl * (fp0 + zl * (f1 - f0 - fp0))
    fh = f0 + zh * (fp0 + zh * (f1 - f0 - fp0))
    c = 2 * (f1 - f0 - fp0)
    zmin, fmin = zl, fl
    if fh < fmin:
        zmin, fmin = zh, fh
    if c > 0:
        z = -fp0 / c
        if zl < z < zh:
            fz = f0 + z * (fp0 + z * (f1 - f0 - fp0))
            if fz < fmin:
                zmin, fmin = z, fz
    return zmin


def _interpolate(a, fa, fpa, b, fb, fpb, xmin, xmax):
    zmin = (xmin - a) / (b - a)
    zmax = (xmax - a) / (b - a)
    if zmin > zmax:
        zmin, zmax = zmax, zmin
    if not math.isnan(fpb):
        z = _cubicmin(fa, fpa * (b - a), fb, fpb * (b - a), zmin, zmax)
    else:
        z = _interp_quad(fa, fpa * (b - a), fb, zmin, zmax)
    return a + z * (b - a)


class Bfgs:
    """bfgs.h's BFGS<Functor> with a combined f / df cache keyed by alpha: each distinct trial point costs one evaluation pass."""

    def __init__(self, fdf, x):
        self.fdf = fdf
        self.passes = 0
        self.searches = []                 # per line search: (status, alpha_new, f0, fp0, f(alpha), f'(alpha), via sigma test)
        f, g = self._eval(np.array(x, np.float64))
        self.x = np.array(x, np.float64)
        self.f, self.g = f, g.copy()
        self.x0, self.g0 = self.x.copy(), g.copy()
        self.g0norm = _norm(self.g0)
        self.p = np.array([(g[i] * -1.0) / self.g0norm for i in range(6)])
        self.pnorm = _norm(self.p)
        self.fp0 = -self.g0norm
        self.delta_f = 0.0
        self.dx = np.zeros(6)
        self.cache = (0.0, self.x.copy(), f, g.copy())

    def _eval(self, x):
        self.passes += 1
        return self.fdf(x)

    def _at(self, alpha):
        if alpha != self.cache[0]:
            x = np.array([self.x0[i] + alpha * self.p[i] for i in range(6)])
            f, g = self._eval(x)
            self.cache = (alpha, x, f, g)
        return self.cache

    def _line_search(self, alpha1):
        f0 = self.cache[2]
        fp0 = _dot(self.cache[3], self.p)
        alpha, alpha_prev = alpha1, 0.0
        falpha_prev, fpalpha_prev = f0, fp0
        a, b, fa, fb, fpa, fpb = 0.0, alpha, f0, 0.0, fp0, 0.0
        i = 0
        bracketed = False
        while True:
            i += 1
            if not (i - 1 < LS_ITERS):
                break
            _, _, falpha, galpha = self._at(alpha)
            if falpha > f0 + alpha * RHO * fp0 or falpha >= falpha_prev:
                a, fa, fpa = alpha_prev, falpha_prev, fpalpha_prev
                b, fb, fpb = alpha, falpha, math.nan
                bracketed = True
                break
            fpalpha = _dot(galpha, self.p)
            if abs(fpalpha) <= -SIGMA * fp0:
                self.searches.append((SUCCESS, alpha, f0, fp0, falpha, fpalpha, True))
                return SUCCESS, alpha
            if fpalpha >= 0:
                a, fa, fpa = alpha, falpha, fpalpha
                b, fb, fpb = alpha_prev, falpha_prev, fpalpha_prev
                bracketed = True
                break
            delta = alpha - alpha_prev
            lower = alpha + delta
            upper = alpha + TAU1 * delta
            alpha_next = _interpolate(alpha_prev, falpha_prev, fpalpha_prev, alpha, falpha, fpalpha, lower, upper)
            alpha_prev, falpha_prev, fpalpha_prev = alpha, falpha, fpalpha
            alpha = alpha_next
        del bracketed
        while True:
            i += 1
            if not (i - 1 < LS_ITERS):
                break
            delta = b - a
            lower = a + TAU2 * delta
            upper = b - TAU3 * delta
            alpha = _interpolate(a, fa, fpa, b, fb, fpb, lower, upper)
            _, _, falpha, galpha = self._at(alpha)
            if (a - alpha) * fpa <= DBL_EPS:
                self.searches.append((NO_PROGRESS, 0.0, f0, fp0, falpha, math.nan, False))
                return NO_PROGRESS, 0.0
            if falpha > f0 + RHO * alpha * fp0 or falpha >= fa:
                b, fb, fpb = alpha, falpha, math.nan
            else:
                fpalpha = _dot(galpha, self.p)
                if abs(fpalpha) <= -SIGMA * fp0:
                    self.searches.append((SUCCESS, alpha, f0, fp0, falpha, fpalpha, True))
                    return SUCCESS, alpha
                if ((b - a) >= 0 and fpalpha >= 0) or ((b - a) <= 0 and fpalpha <= 0):
                    b, fb, fpb = a, fa, fpa
                    a, fa, fpa = alpha, falpha, fpalpha
                else:
                    a, fa, fpa = alpha, falpha, fpalpha
        self.searches.append((SUCCESS, 0.0, f0, fp0, math.nan, math.nan, False))
        return SUCCESS, 0.0

    def step(self):
        """minimizeOneStep."""
        f0 = self.f
        if self.pnorm == 0.0 or self.g0norm == 0.0 or self.fp0 == 0:
            self.dx = np.zeros(6)
            return NO_PROGRESS
        if self.delta_f < 0:
            d = max(-self.delta_f, 10 * DBL_EPS * abs(f0))
            alpha1 = min(1.0, 2.0 * d / (-self.fp0))
        else:
            alpha1 = 1.0
        status, alpha = self._line_search(alpha1)
        if status != SUCCESS:
            return status
        _, x, f, g = self._at(alpha)               # updatePosition
        self.x, self.f, self.g = x.copy(), f, g.copy()
        self.delta_f = f - f0
        dx0 = np.array([self.x[i] - self.x0[i] for i in range(6)])
        dg0 = np.array([self.g[i] - self.g0[i] for i in range(6)])
        self.dx = dx0
        dxg, dgg, dxdg = _dot(dx0, self.g), _dot(dg0, self.g), _dot(dx0, dg0)
        dgnorm = _norm(dg0)
        if dxdg != 0:
            B = dxg / dxdg
            A = -(1.0 + dgnorm * dgnorm / dxdg) * B + dgg / dxdg
        else:
            A = B = 0.0
        p = np.array([(self.g[i] + (-A) * dx0[i]) + (-B) * dg0[i] for i in range(6)])
        self.g0, self.x0 = self.g.copy(), self.x.copy()
        self.g0norm = _norm(self.g0)
        pnorm = _norm(p)
        dirn = -1.0 if _dot(p, self.g) > 0 else 1.0
        s = dirn / pnorm
        self.p = np.array([p[i] * s for i in range(6)])
        self.pnorm = _norm(self.p)
        self.fp0 = _dot(self.p, self.g0)
        self.cache = (0.0, self.x0.copy(), self.f, self.g0.copy())      # changeDirection
        return SUCCESS


def estimate_bfgs(x0, P, Q, M, max_inner, perturb=None):
    """estimateRigidTransformationBFGS from state x0 -> (x, f, inner iterations, evaluation passes, the optimiser).  perturb: maps every
    (f, g) the functor returns to another one (a stand-in for another summation order, tests/test_icp_gicp_edge_cases_cpu.py)."""
    fdf = (lambda x: evaluate(x, P, Q, M)) if perturb is None else (lambda x: perturb(*evaluate(x, P, Q, M)))
    opt = Bfgs(fdf, x0)
    inner = 0
    while True:
        inner += 1
        result = opt.step()
        if result != SUCCESS:
            break
        result = SUCCESS if _norm(opt.g) < GRADIENT_EPS else RUNNING
        if not (result == RUNNING and inner < max_inner):
            break
    return opt.x, opt.f, inner, opt.passes, opt


# ---- computeTransformation ------------------------------------------------------------------------------------------------------
def _R_of(T, guess):
    A, B = np.asarray(T, np.float32).astype(np.float64), np.asarray(guess, np.float32).astype(np.float64)
    R = np.zeros((3, 3))
    for i in range(3):
        for j in range(3):
            R[i, j] = ((A[i, 0] * B[0, j] + A[i, 1] * B[1, j]) + A[i, 2] * B[2, j]) + A[i, 3] * B[3, j]
    return R


def _nn_finite(orc, tgt, fin_t, queries):
    """Exact float 1-NN of every query among the target's finite points (FLANN's order, ties to the lowest index) -> (index, d2)."""
    n = queries.shape[0]
    j = np.full(n, -1, np.int64)
    d2 = np.full(n, np.inf, np.float32)
    ok = np.isfinite(queries).all(axis=1)
    if fin_t.size == 0 or not ok.any():
        return j, d2
    c = np.zeros((fin_t.size, 4), np.float32)
    c[:, :3] = tgt[fin_t]
    q = np.zeros((int(ok.sum()), 4), np.float32)
    q[:, :3] = queries[ok]
    idx, dd = orc.knn(c, q, 1)
    j[ok] = fin_t[idx[:, 0]]
    d2[ok] = dd[:, 0]
    return j, d2


def correspondences(orc, tgt, output, T, guess, Cs, Ct, max_corr, trace=None):
    """One correspondence pass: (kept source indices, their target indices, M of each).  trace: a list that receives dict(d2, keep, j)."""
    tgt = np.asarray(tgt, np.float32)[:, :3]
    output = np.asarray(output, np.float32)[:, :3]
    fin_t = np.nonzero(np.isfinite(tgt).all(axis=1))[0]
    R = _R_of(T, guess)
    query = f32_transform(T, output)
    j, d2 = _nn_finite(orc, tgt, fin_t, query)
    keep = (j >= 0) & (d2.astype(np.float64) < float(max_corr) * float(max_corr))
    if trace is not None:
        trace.append(dict(d2=d2.copy(), keep=keep.copy(), j=j.copy()))
    src_i = np.nonzero(keep)[0]
    tgt_j = j[keep]
    RC = R[None] @ Cs[src_i]
    Mi = inv3_eigen(RC @ R.T[None] + Ct[tgt_j])
    return src_i, tgt_j, Mi


def gicp_align(orc, tgt, src, guess=None, max_corr=2.5, transformation_epsilon=0.01, maximum_iterations=64, k=20,
               max_optimizer_iterations=20, rotation_epsilon=2e-3, gicp_epsilon=1e-3, Ct=None, Cs=None, trace=None, perturb=None):
    tgt = np.asarray(tgt, np.float32)[:, :3]
    src = np.asarray(src, np.float32)[:, :3]
    guess = np.eye(4, dtype=np.float32) if guess is None else np.asarray(guess, np.float32).copy()
    if Ct is None:
        Ct = covariances(orc, tgt, k, gicp_epsilon)[0]
    if Cs is None:
        Cs = covariances(orc, src, k, gicp_epsilon)[0]
    output = f32_transform(guess, src)
    T = np.eye(4, dtype=np.float32)
    iterations, evaluations, converged, score = 0, 0, False, DBL_MAX
    traj, searches = [], []
    while not converged:
        evaluations += 1
        si, tj, Mi = correspondences(orc, tgt, output, T, guess, Cs, Ct, max_corr, trace)
        if si.size < 4:
            break
        x, f, inner, passes, opt = estimate_bfgs(state_of(T), output[si], tgt[tj], Mi, max_optimizer_iterations, perturb)
        evaluations += passes
        searches += opt.searches
        # a line search that ended in roundoff (NoProgress, or its step budget spent) turns on comparisons of f values a few ulps
        # apart: there the device's own summation order may take other trial points (DESIGN.md "GICP_HIP", numerics)
        roundoff = any(not s_[6] for s_ in opt.searches)
        prev = T
        T = apply_state(x)
        delta = 0.0
        for r in range(4):
            for c in range(4):
                ratio = 1.0 / rotation_epsilon if (r < 3 and c < 3) else 1.0 / transformation_epsilon
                cd = ratio * float(abs(f32(prev[r, c]) - f32(T[r, c])))
                if cd > delta:
                    delta = cd
        iterations += 1
        score = f
        traj.append(dict(T=T.copy(), n=int(si.size), inner=inner, passes=passes, f=f, roundoff=roundoff, delta=delta))
        if iterations >= maximum_iterations or delta < 1:
            converged = True
    final = f32_matmul4(T, guess)
    return dict(T=final, converged=converged, iterations=iterations, evaluations=evaluations, score=score, traj=traj, searches=searches)
