// GICP_HIP: pcl::GeneralizedIterativeClosestPoint<PointXYZ, PointXYZ>::computeTransformation, the object the reference's factory builds
// for "GICP" (src/hdl_graph_slam/registrations.cpp:65-87; pclomp's copy is the same algorithm).  Behaviour: DESIGN.md "GICP_HIP"; the
// test-side restatement tests/pcl_gicp_reference.py is the specification this file reproduces.
//
// MI355X design
//   * Covariances (computeCovariances): knn_lists.hip's k-NN lists (knn_lists), then pg_cov_kernel, one lane per point: the list sorted by
//     index (a register sorting network: the sums do not depend on which index ordered the search), raw moments in double from float
//     products, JacobiSVD (jacobi_svd3_d) and U diag(1, 1, eps) U^T.  Kept per cloud in CloudState::pcov, keyed by (k, eps).
//   * One launch per round for the whole batch (pg_round_kernel), every pair in its own phase.  A pair owns a FIXED number of
//     workgroups (slices) derived from its own size; each slice walks kPgSlicePoints source slots in the source index's spatial order.
//     CORRESPOND: 8-lane groups move output[i] by transformation_, find the gated exact 1-NN, and one lane writes q and
//     M_i = ((R C1) R^T + C2)^-1 per slot.  EVALUATE: one lane per slot forms the 13 double sums of OptimizationFunctorWithIndices
//     (f, sum temp, sum p temp^T) at the pair's trial state.  Wave DPP sums -> LDS -> one fixed-order row per slice; the pair's last
//     workgroup (ticket, common.h "in-launch hand-off") sums the rows in slice order and runs, on one lane, the BFGS / Fletcher
//     line-search state machine of bfgs.h up to its next evaluation request, or PCL's convergence test and the next correspondence pass.
//   * Every pass computes f and g together: a trial step costs one pass, and a cached alpha none.
//   * The host enqueues launches in chunks and polls a pinned done counter once per chunk: no host round trip per evaluation.
#include <algorithm>
#include <cfloat>
#include <climits>
#include <cmath>
#include <cstddef>
#include <cstring>
#include <vector>

#include "batch_rounds.h"
#include "handle.h"
#include "nn_group.h"
#include "pg_cov.h"
#include "slice_rows.h"
#include "small_linalg.h"

namespace dgs {

enum : int { PG_CORRESPOND = 0, PG_EVALUATE = 1 };
enum : int { PG_AT_INIT = 0, PG_AT_BRACKET = 1, PG_AT_SECTION = 2, PG_AT_UPDATE = 3, PG_AT_PROBE = 4 };

struct PgPair {
  float final_T[16];   // column-major, = final_transformation_ (read by the fitness pass)
  float T[16];         // transformation_, row-major
  float guess[16];     // row-major
  double R[9];         // top-left 3 x 3 of double(transformation_) * double(guess) of the running correspondence pass
  // bfgs.h's state
  double x[6], x0[6], g[6], g0[6], p[6];
  double f, g0norm, pnorm, fp0, delta_f, f0s;
  double ck, cf, cg[6], cx[6];   // the f / g cache: values at x0 + ck p
  double ta, xt[6];              // trial alpha and point of the pending evaluation pass
  // lineSearch's locals, kept across passes
  double ls_f0, ls_fp0, alpha, alpha_prev, falpha_prev, fpalpha_prev, a, b, fa, fb, fpa, fpb, alpha_new;
  double score;                  // the last accepted f
  int phase, resume, ls_i, ls_status, inner, passes, m;
  int active, iterations, evaluations, converged, ticket, probe;
};

struct PgItem {
  const float4* src;         // source points in the caller's order
  const float4* src_sorted;  // the same points in their own Hilbert index's order, w = original index
  const double* cs;          // the source's PCL-style covariances (9 per point, caller's order)
  long long off;             // first slot of this pair in the batch-wide slot arrays
  int n, slice0, n_slices;
  int tgt;                   // per-pair targets (pcl_gicp_align_pairs): the pair's entry of the launch's target table; 0 on the single-target path
};

struct PgInit {
  float guess[16];   // column-major
  float T[16];       // column-major: transformation_ at the start (identity, or the probe's)
  double x[6];       // probe: the state to evaluate
  int n, skip, probe, pad;
};

struct PgConsts {
  double trans_eps, rot_eps;
  long long total;   // slots of the batch: plane stride of the M arrays
  float gate;        // largest float g with (double) g < corr_dist^2: d2 <= gate <=> (double) d2 < corr_dist^2
  int max_iterations, max_inner, traj_cap;
};

constexpr int kPgRun = 8;                                // points per 8-lane group and slice
constexpr int kPgSlicePoints = (kBlock / 8) * kPgRun;    // 256 slots per workgroup: one lane each in EVALUATE
constexpr int kPgAccum = 13;                             // f, sum temp (3), sum p temp^T (9, row-major); CORRESPOND: [0] = kept pairs
constexpr int kPgPad = 16;                               // row stride (doubles)
constexpr int kPgLsIters = 100;                          // bracket_iters = section_iters, one counter for both
constexpr double kPgRho = 0.01, kPgSigma = 0.01, kPgTau1 = 9.0, kPgTau2 = 0.05, kPgTau3 = 0.5, kPgGradEps = 1e-2;

// ================================================================================================ covariances
// computeCovariances over one cloud: the bodies are pg_cov.h's (the batched pass of cov_batch.hip runs the same ones over many clouds).
__global__ __launch_bounds__(kBlock) void pg_cov_kernel(const BvhView b, const float4* __restrict__ pts, const int n, const int k, const double eps,
                                                        const int* __restrict__ nbr, double* __restrict__ cov9) {
  pg_cov_body(b, pts, n, k, eps, nbr, cov9, (int)blockIdx.x);
}
__global__ __launch_bounds__(kPgWideBlock) void pg_cov_wide_kernel(const BvhView b, const float4* __restrict__ pts, const int n, const int k, const double eps,
                                                                   const int* __restrict__ nbr, double* __restrict__ cov9) {
  pg_cov_wide_body(b, pts, n, k, eps, nbr, cov9, (int)blockIdx.x);
}

// ================================================================================================ device helpers
// applyState(I, x): AngleAxisf(x5, Z) * AngleAxisf(x4, Y) * AngleAxisf(x3, X) as float quaternions (half-angle sin / cos in double,
// rounded to float), toRotationMatrix, float translation.  T12: row-major 3 x 4.
__device__ void pg_apply_state(const double* x, float* T12) {
#pragma clang fp contract(off)
  float c[3], s[3];
  for (int a = 0; a < 3; a++) {
    const float ha = 0.5f * (float)x[3 + a];
    c[a] = (float)cos((double)ha);
    s[a] = (float)sin((double)ha);
  }
  const float z0 = 0.f;
  // (w, x, y, z) of Z, Y, X
  const float az[4] = {c[2], s[2] * z0, s[2] * z0, s[2]};
  const float ay[4] = {c[1], s[1] * z0, s[1], s[1] * z0};
  const float ax[4] = {c[0], s[0], s[0] * z0, s[0] * z0};
  auto qmul = [](const float* A, const float* B, float* o) {
    o[0] = A[0] * B[0] - A[1] * B[1] - A[2] * B[2] - A[3] * B[3];
    o[1] = A[0] * B[1] + A[1] * B[0] + A[2] * B[3] - A[3] * B[2];
    o[2] = A[0] * B[2] + A[2] * B[0] + A[3] * B[1] - A[1] * B[3];
    o[3] = A[0] * B[3] + A[3] * B[0] + A[1] * B[2] - A[2] * B[1];
  };
  float zy[4], q[4];
  qmul(az, ay, zy);
  qmul(zy, ax, q);
  const float w = q[0], qx = q[1], qy = q[2], qz = q[3];
  const float tx = 2.f * qx, ty = 2.f * qy, tz = 2.f * qz;
  const float twx = tx * w, twy = ty * w, twz = tz * w;
  const float txx = tx * qx, txy = ty * qx, txz = tz * qx;
  const float tyy = ty * qy, tyz = tz * qy, tzz = tz * qz;
  T12[0] = 1.f - (tyy + tzz); T12[1] = txy - twz; T12[2] = txz + twy; T12[3] = (float)x[0];
  T12[4] = txy + twz; T12[5] = 1.f - (txx + tzz); T12[6] = tyz - twx; T12[7] = (float)x[1];
  T12[8] = txz - twy; T12[9] = tyz + twx; T12[10] = 1.f - (txx + tyy); T12[11] = (float)x[2];
}

__device__ double pg_dot6(const double* a, const double* b) {
#pragma clang fp contract(off)
  double r = 0.0;
  for (int i = 0; i < 6; i++) r += a[i] * b[i];
  return r;
}

__device__ __forceinline__ double pg_cubic(double c0, double c1, double c2, double c3, double z) { return c0 + z * (c1 + z * (c2 + z * c3)); }

__device__ double pg_cubicmin(double f0, double fp0, double f1, double fp1, double zl, double zh) {
#pragma clang fp contract(off)
  const double eta = 3 * (f1 - f0) - 2 * fp0 - fp1;
  const double xi = fp0 + fp1 - 2 * (f1 - f0);
  const double c0 = f0, c1 = fp0, c2 = eta, c3 = xi;
  double zmin = zl, fmin = pg_cubic(c0, c1, c2, c3, zl);
  double y = pg_cubic(c0, c1, c2, c3, zh);
  if (y < fmin) { zmin = zh; fmin = y; }
  const double a2 = 3 * c3, b1 = 2 * c2, c0p = c1;
  double r[2];
  int nr = 0;
  if (a2 != 0.0) {
    const double disc = b1 * b1 - 4 * a2 * c0p;
    if (disc > 0) {
      const double sd = sqrt(disc);
      const double r0 = (-b1 - sd) / (2 * a2), r1 = (-b1 + sd) / (2 * a2);
      r[0] = (r1 < r0) ? r1 : r0;
      r[1] = (r1 < r0) ? r0 : r1;
      nr = 2;
    } else if (disc == 0) {
      r[0] = -b1 / (2 * a2);
      nr = 1;
    }
  }
  for (int q = 0; q < nr; q++) {
    const double z = r[q];
    if (zl < z && z < zh) {
      y = pg_cubic(c0, c1, c2, c3, z);
      if (y < fmin) { zmin = z; fmin = y; }
    }
  }
  return zmin;
}

__device__ double pg_interp_quad(double f0, double fp0, double f1, double zl, double zh) {
#pragma clang fp contract(off)
  const double fl = f0 + zl * (fp0 + zl * (f1 - f0 - fp0));
  const double fh = f0 + zh * (fp0 + zh * (f1 - f0 - fp0));
  const double c = 2 * (f1 - f0 - fp0);
  double zmin = zl, fmin = fl;
  if (fh < fmin) { zmin = zh; fmin = fh; }
  if (c > 0) {
    const double z = -fp0 / c;
    if (zl < z && z < zh) {
      const double fz = f0 + z * (fp0 + z * (f1 - f0 - fp0));
      if (fz < fmin) { zmin = z; fmin = fz; }
    }
  }
  return zmin;
}

__device__ double pg_interpolate(double a, double fa, double fpa, double b, double fb, double fpb, double xmin, double xmax) {
#pragma clang fp contract(off)
  double zmin = (xmin - a) / (b - a);
  double zmax = (xmax - a) / (b - a);
  if (zmin > zmax) { const double t = zmin; zmin = zmax; zmax = t; }
  const double z = !isnan(fpb) ? pg_cubicmin(fa, fpa * (b - a), fb, fpb * (b - a), zmin, zmax) : pg_interp_quad(fa, fpa * (b - a), fb, zmin, zmax);
  return a + z * (b - a);
}

// R of the next correspondence pass: top-left 3 x 3 of double(T) * double(guess), each entry summed over k = 0..3 in order
__device__ void pg_set_R(PgPair* s) {
#pragma clang fp contract(off)
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) {
      double r = 0.0;
      for (int k = 0; k < 4; k++) r = (k == 0) ? (double)s->T[i * 4 + 0] * (double)s->guess[0 * 4 + j] : r + (double)s->T[i * 4 + k] * (double)s->guess[k * 4 + j];
      s->R[i * 3 + j] = r;
    }
}

// The loop has ended: final_transformation_ = transformation_ * guess (float 4 x 4, ICP_HIP's rounding), column-major.
__device__ void pg_finish(PgPair* s, int converged, int* done_counter) {
  for (int r = 0; r < 4; r++)
    for (int c = 0; c < 4; c++)
      s->final_T[c * 4 + r] = add_rn(add_rn(add_rn(mul_rn(s->T[r * 4 + 0], s->guess[0 * 4 + c]), mul_rn(s->T[r * 4 + 1], s->guess[1 * 4 + c])),
                                            mul_rn(s->T[r * 4 + 2], s->guess[2 * 4 + c])),
                                     mul_rn(s->T[r * 4 + 3], s->guess[3 * 4 + c]));
  s->converged = converged;
  s->active = 0;
  atomicAdd(done_counter, 1);
}

__device__ void pg_request(PgPair* s, double alpha, int resume) {
#pragma clang fp contract(off)
  s->ta = alpha;
  for (int i = 0; i < 6; i++) s->xt[i] = s->x0[i] + alpha * s->p[i];   // moveTo
  s->resume = resume;
  s->phase = PG_EVALUATE;
}

// bfgs.h driven by evaluation results: (fe, ge) are f and g at s->xt (alpha s->ta).  Runs until the next evaluation request, or through
// the end of estimateRigidTransformationBFGS and the outer iteration's bookkeeping.  One lane.  Locals are declared up front: the labels
// are re-entry points.
__device__ __noinline__ void pg_run(PgPair* s, const double fe, const double* ge, const PgConsts c, int* done_counter, float* traj_T,
                                    int* traj_i, double* traj_f, const int pair) {
#pragma clang fp contract(off)
  double alpha1, falpha, fpalpha, delta, lower, upper, alpha_next, dxg, dgg, dxdg, dgnorm, A, B, pnorm, dir, sc, dmax, gn;
  double dx0[6], dg0[6], pn[6];
  float prevT[16], T12[12];
  int status;
  s->ck = s->ta;
  s->cf = fe;
  for (int i = 0; i < 6; i++) { s->cg[i] = ge[i]; s->cx[i] = s->xt[i]; }
  switch (s->resume) {
    case PG_AT_BRACKET: goto bracket_f;
    case PG_AT_SECTION: goto section_f;
    case PG_AT_UPDATE: goto update_f;
    case PG_AT_PROBE:
      s->f = fe;
      for (int i = 0; i < 6; i++) s->g[i] = ge[i];
      s->active = 0;
      atomicAdd(done_counter, 1);
      return;
    default: break;
  }
  // ---- minimizeInit
  s->f = fe;
  for (int i = 0; i < 6; i++) { s->x[i] = s->xt[i]; s->x0[i] = s->xt[i]; s->g[i] = ge[i]; s->g0[i] = ge[i]; }
  s->g0norm = sqrt(pg_dot6(s->g0, s->g0));
  for (int i = 0; i < 6; i++) s->p[i] = (ge[i] * -1.0) / s->g0norm;
  s->pnorm = sqrt(pg_dot6(s->p, s->p));
  s->fp0 = -s->g0norm;
  s->delta_f = 0.0;
  s->inner = 0;
step:
  // ---- one inner iteration: minimizeOneStep
  s->inner += 1;
  s->f0s = s->f;
  if (s->pnorm == 0.0 || s->g0norm == 0.0 || s->fp0 == 0) {
    status = 1;   // NoProgress
    goto step_status;
  }
  if (s->delta_f < 0) {
    const double del = fmax(-s->delta_f, 10 * DBL_EPSILON * fabs(s->f0s));
    alpha1 = fmin(1.0, 2.0 * del / (-s->fp0));
  } else {
    alpha1 = 1.0;
  }
  // lineSearch: f and f' at 0 are the cache (changeDirection / minimizeInit left it there)
  s->ls_f0 = s->cf;
  s->ls_fp0 = pg_dot6(s->cg, s->p);
  s->alpha = alpha1;
  s->alpha_prev = 0.0;
  s->falpha_prev = s->ls_f0;
  s->fpalpha_prev = s->ls_fp0;
  s->a = 0.0; s->b = alpha1; s->fa = s->ls_f0; s->fb = 0.0; s->fpa = s->ls_fp0; s->fpb = 0.0;
  s->ls_i = 0;
  s->alpha_new = 0.0;
bracket_top:
  if (!(s->ls_i++ < kPgLsIters)) goto section_top;
  if (s->alpha != s->ck) { pg_request(s, s->alpha, PG_AT_BRACKET); return; }
bracket_f:
  falpha = s->cf;
  if (falpha > s->ls_f0 + s->alpha * kPgRho * s->ls_fp0 || falpha >= s->falpha_prev) {
    s->a = s->alpha_prev; s->fa = s->falpha_prev; s->fpa = s->fpalpha_prev;
    s->b = s->alpha; s->fb = falpha; s->fpb = NAN;
    goto section_top;
  }
  fpalpha = pg_dot6(s->cg, s->p);
  if (fabs(fpalpha) <= -kPgSigma * s->ls_fp0) {
    s->alpha_new = s->alpha;
    s->ls_status = 0;
    goto ls_done;
  }
  if (fpalpha >= 0) {
    s->a = s->alpha; s->fa = falpha; s->fpa = fpalpha;
    s->b = s->alpha_prev; s->fb = s->falpha_prev; s->fpb = s->fpalpha_prev;
    goto section_top;
  }
  delta = s->alpha - s->alpha_prev;
  lower = s->alpha + delta;
  upper = s->alpha + kPgTau1 * delta;
  alpha_next = pg_interpolate(s->alpha_prev, s->falpha_prev, s->fpalpha_prev, s->alpha, falpha, fpalpha, lower, upper);
  s->alpha_prev = s->alpha;
  s->falpha_prev = falpha;
  s->fpalpha_prev = fpalpha;
  s->alpha = alpha_next;
  goto bracket_top;
section_top:
  if (!(s->ls_i++ < kPgLsIters)) {
    s->ls_status = 0;   // Success with alpha_new as it stands
    goto ls_done;
  }
  delta = s->b - s->a;
  lower = s->a + kPgTau2 * delta;
  upper = s->b - kPgTau3 * delta;
  s->alpha = pg_interpolate(s->a, s->fa, s->fpa, s->b, s->fb, s->fpb, lower, upper);
  if (s->alpha != s->ck) { pg_request(s, s->alpha, PG_AT_SECTION); return; }
section_f:
  falpha = s->cf;
  if ((s->a - s->alpha) * s->fpa <= DBL_EPSILON) {
    s->ls_status = 1;   // roundoff prevents progress
    goto ls_done;
  }
  if (falpha > s->ls_f0 + kPgRho * s->alpha * s->ls_fp0 || falpha >= s->fa) {
    s->b = s->alpha; s->fb = falpha; s->fpb = NAN;
  } else {
    fpalpha = pg_dot6(s->cg, s->p);
    if (fabs(fpalpha) <= -kPgSigma * s->ls_fp0) {
      s->alpha_new = s->alpha;
      s->ls_status = 0;
      goto ls_done;
    }
    if (((s->b - s->a) >= 0 && fpalpha >= 0) || ((s->b - s->a) <= 0 && fpalpha <= 0)) {
      s->b = s->a; s->fb = s->fa; s->fpb = s->fpa;
      s->a = s->alpha; s->fa = falpha; s->fpa = fpalpha;
    } else {
      s->a = s->alpha; s->fa = falpha; s->fpa = fpalpha;
    }
  }
  goto section_top;
ls_done:
  if (s->ls_status != 0) {
    status = s->ls_status;
    goto step_status;
  }
  // updatePosition(alpha_new)
  if (s->alpha_new != s->ck) { pg_request(s, s->alpha_new, PG_AT_UPDATE); return; }
update_f:
  for (int i = 0; i < 6; i++) { s->x[i] = s->cx[i]; s->g[i] = s->cg[i]; }
  s->f = s->cf;
  s->delta_f = s->f - s->f0s;
  for (int i = 0; i < 6; i++) { dx0[i] = s->x[i] - s->x0[i]; dg0[i] = s->g[i] - s->g0[i]; }
  dxg = pg_dot6(dx0, s->g);
  dgg = pg_dot6(dg0, s->g);
  dxdg = pg_dot6(dx0, dg0);
  dgnorm = sqrt(pg_dot6(dg0, dg0));
  if (dxdg != 0) {
    B = dxg / dxdg;
    A = -(1.0 + dgnorm * dgnorm / dxdg) * B + dgg / dxdg;
  } else {
    B = 0;
    A = 0;
  }
  for (int i = 0; i < 6; i++) pn[i] = (s->g[i] + (-A) * dx0[i]) + (-B) * dg0[i];
  for (int i = 0; i < 6; i++) { s->g0[i] = s->g[i]; s->x0[i] = s->x[i]; }
  s->g0norm = sqrt(pg_dot6(s->g0, s->g0));
  pnorm = sqrt(pg_dot6(pn, pn));
  dir = (pg_dot6(pn, s->g) > 0) ? -1.0 : 1.0;
  sc = dir / pnorm;
  for (int i = 0; i < 6; i++) s->p[i] = pn[i] * sc;
  s->pnorm = sqrt(pg_dot6(s->p, s->p));
  s->fp0 = pg_dot6(s->p, s->g0);
  // changeDirection: the cache now holds alpha 0 of the new line
  s->ck = 0.0;
  for (int i = 0; i < 6; i++) { s->cx[i] = s->x0[i]; s->cg[i] = s->g0[i]; }
  s->cf = s->f;
  status = 0;
step_status:
  if (status == 0) {
    gn = sqrt(pg_dot6(s->g, s->g));   // testGradient
    if (!(gn < kPgGradEps) && s->inner < c.max_inner) goto step;
  }
  // ---- estimateRigidTransformationBFGS accepts x; computeTransformation's delta and convergence test
  for (int k = 0; k < 16; k++) prevT[k] = s->T[k];
  pg_apply_state(s->x, T12);
  for (int k = 0; k < 12; k++) s->T[k] = T12[k];
  s->T[12] = 0.f; s->T[13] = 0.f; s->T[14] = 0.f; s->T[15] = 1.f;
  dmax = 0.0;
  for (int r = 0; r < 4; r++)
    for (int cc = 0; cc < 4; cc++) {
      const double ratio = (r < 3 && cc < 3) ? 1.0 / c.rot_eps : 1.0 / c.trans_eps;
      const double cd = ratio * (double)fabsf(prevT[r * 4 + cc] - s->T[r * 4 + cc]);
      if (cd > dmax) dmax = cd;
    }
  s->iterations += 1;
  s->score = s->f;
  if (s->iterations - 1 < c.traj_cap) {
    const size_t e = (size_t)pair * c.traj_cap + (s->iterations - 1);
    for (int r = 0; r < 4; r++)
      for (int cc = 0; cc < 4; cc++) traj_T[e * 16 + cc * 4 + r] = s->T[r * 4 + cc];
    traj_i[e * 3 + 0] = s->m;
    traj_i[e * 3 + 1] = s->inner;
    traj_i[e * 3 + 2] = s->passes;
    traj_f[e] = s->f;
  }
  if (s->iterations >= c.max_iterations || dmax < 1) {
    pg_finish(s, 1, done_counter);
  } else {
    pg_set_R(s);
    s->phase = PG_CORRESPOND;
  }
}

// Closing of one pass of one pair (one lane of its last workgroup): tot = the pair's sums.
__device__ __noinline__ void pg_close(PgPair* s, const double* tot, const PgConsts c, int* done_counter, float* traj_T, int* traj_i, double* traj_f,
                                      const int pair) {
#pragma clang fp contract(off)
  s->evaluations += 1;
  if (s->phase == PG_CORRESPOND) {
    s->m = (int)tot[0];
    if (s->probe) {   // dgs_pcl_gicp_evaluate: one pass at the probe's state
      s->resume = PG_AT_PROBE;
      s->phase = PG_EVALUATE;
      return;
    }
    if (s->m < 4) {   // "Need at least 4 points": the loop ends, not converged, nr_iterations_ unchanged
      pg_finish(s, 0, done_counter);
      return;
    }
    // the BFGS start: (t, atan2(r21, r22), asin(-r20), atan2(r10, r00)) of transformation_, angles through the float overloads
    const float* T = s->T;
    s->x0[0] = T[3]; s->x0[1] = T[7]; s->x0[2] = T[11];
    s->x0[3] = (double)(float)atan2((double)T[9], (double)T[10]);
    s->x0[4] = (double)(float)asin(-(double)T[8]);
    s->x0[5] = (double)(float)atan2((double)T[4], (double)T[0]);
    for (int i = 0; i < 6; i++) s->xt[i] = s->x0[i];
    s->ta = 0.0;
    s->passes = 0;
    s->resume = PG_AT_INIT;
    s->phase = PG_EVALUATE;
    return;
  }
  s->passes += 1;
  const double m = (double)s->m;
  double g[6], Rs[9];
  const double f = tot[0] / m;
  const double sc = 2.0 / m;
  for (int a = 0; a < 3; a++) g[a] = tot[1 + a] * sc;
  for (int a = 0; a < 9; a++) Rs[a] = tot[4 + a] * sc;
  // computeRDerivative at the trial state: g[3 + k] = tr(dR_k Rs) (matricesInnerProd), closed forms in double
  const double* x = s->xt;
  const double cphi = cos(x[3]), sphi = sin(x[3]), cth = cos(x[4]), sth = sin(x[4]), cpsi = cos(x[5]), spsi = sin(x[5]);
  const double d[3][9] = {
      {0., sphi * spsi + cphi * cpsi * sth, cphi * spsi - cpsi * sphi * sth, 0., -cpsi * sphi + cphi * spsi * sth, -cphi * cpsi - sphi * spsi * sth, 0., cphi * cth,
       -cth * sphi},
      {-cpsi * sth, cpsi * cth * sphi, cphi * cpsi * cth, -spsi * sth, cth * sphi * spsi, cphi * cth * spsi, -cth, -sphi * sth, -cphi * sth},
      {-cth * spsi, -cphi * cpsi - sphi * spsi * sth, cpsi * sphi - cphi * spsi * sth, cpsi * cth, -cphi * spsi + cpsi * sphi * sth, sphi * spsi + cphi * cpsi * sth,
       0., 0., 0.}};
  for (int k = 0; k < 3; k++) {
    double r = 0.0;
    for (int i = 0; i < 3; i++)
      for (int j = 0; j < 3; j++) r += d[k][j * 3 + i] * Rs[i * 3 + j];
    g[3 + k] = r;
  }
  pg_run(s, f, g, c, done_counter, traj_T, traj_i, traj_f, pair);
}

// output = guess * source for every slot of every pair (once per batch), walk order.
__global__ __launch_bounds__(kBlock) void pg_prepare_kernel(const PgItem* __restrict__ items, const PgPair* __restrict__ pairs, const int* __restrict__ blk_pair,
                                                            float4* __restrict__ W) {
#pragma clang fp contract(off)
  const int pair = blk_pair[blockIdx.x];
  const PgItem it = items[pair];
  const int slice = (int)blockIdx.x - it.slice0;
  const int pos = slice * kPgSlicePoints + (int)threadIdx.x;
  if (pos >= it.n) return;
  const float* G = pairs[pair].guess;
  const int i = (int)__float_as_uint(it.src_sorted[pos].w);
  float4 o = make_float4(NAN, NAN, NAN, __int_as_float(-1));
  if (i >= 0 && i < it.n) {
    const float4 s = it.src[i];
    o = make_float4(affine_row_rn(G[0], G[1], G[2], G[3], s.x, s.y, s.z), affine_row_rn(G[4], G[5], G[6], G[7], s.x, s.y, s.z),
                    affine_row_rn(G[8], G[9], G[10], G[11], s.x, s.y, s.z), __int_as_float(i));
  }
  W[it.off + pos] = o;
}

// One round of one active pair's slice: its correspondence pass or its evaluation pass, then (last workgroup) the pair's closing.  The
// body of both round kernels below; (tv, tgt, tcov) is the pair's target: index view, points in the caller's order, PCL-style covariances.
__device__ __forceinline__ void pg_round_body(const BvhView tv, const float4* __restrict__ tgt, const double* __restrict__ tcov, const PgItem it, PgPair* st,
                                              const int pair, const float4* __restrict__ W, float4* __restrict__ Q, double* __restrict__ Mp,
                                              double* __restrict__ rows, const PgConsts c, int* __restrict__ done_counter, float* __restrict__ traj_T,
                                              int* __restrict__ traj_i, double* __restrict__ traj_f) {
#pragma clang fp contract(off)
  const int slice = (int)blockIdx.x - it.slice0;
  const int n = it.n;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, sub = lane & 7;
  double acc[kPgAccum];
#pragma unroll
  for (int k = 0; k < kPgAccum; k++) acc[k] = 0.0;
  __shared__ float sT[12];
  const bool correspond = st->phase == PG_CORRESPOND;
  if (correspond) {
    float T[12];
#pragma unroll
    for (int k = 0; k < 12; k++) T[k] = st->T[k];
    double R[9];
#pragma unroll
    for (int k = 0; k < 9; k++) R[k] = st->R[k];
    const int first = (slice * (kBlock / kWave) + wave) * (8 * kPgRun) + (lane >> 3);
    float px = 0.f, py = 0.f, pz = 0.f, prev_best = INFINITY;
    bool prev_found = false;
    for (int r = 0; r < kPgRun; r++) {
      const int pos = first + r * 8;
      const float4 w = (pos < n) ? W[it.off + pos] : make_float4(0.f, 0.f, 0.f, __int_as_float(-1));
      const int i = __float_as_int(w.w);
      float x = 0.f, y = 0.f, z = 0.f;
      bool alive = pos < n && i >= 0 && i < n;
      if (alive) {   // query = transformation_ * output[i]
        x = affine_row_rn(T[0], T[1], T[2], T[3], w.x, w.y, w.z);
        y = affine_row_rn(T[4], T[5], T[6], T[7], w.x, w.y, w.z);
        z = affine_row_rn(T[8], T[9], T[10], T[11], w.x, w.y, w.z);
        alive = isfinite(x) && isfinite(y) && isfinite(z);
        if (!alive) { x = 0.f; y = 0.f; z = 0.f; }
      }
      float best;
      int bi;
      const float bound = fminf(c.gate, nn_warm_bound_round(prev_best, prev_found, x, y, z, px, py, pz));
      nn_query_group(tv, x, y, z, alive, bound, best, bi);
      prev_found = alive && bi != 0x7FFFFFFF;
      prev_best = best;
      px = x; py = y; pz = z;
      const bool keep = alive && bi != 0x7FFFFFFF;   // d2 <= gate <=> (double) d2 < corr_dist^2
      if (sub == 0 && pos < n) {
        float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
        if (keep) {
          q = tgt[bi];
          q.w = 1.f;
          const double* C1 = it.cs + (size_t)i * 9;
          const double* C2 = tcov + (size_t)bi * 9;
          double RC[9], S[9], Mi[9];
          for (int a = 0; a < 3; a++)
            for (int b = 0; b < 3; b++) RC[a * 3 + b] = (R[a * 3 + 0] * C1[0 * 3 + b] + R[a * 3 + 1] * C1[1 * 3 + b]) + R[a * 3 + 2] * C1[2 * 3 + b];
          for (int a = 0; a < 3; a++)
            for (int b = 0; b < 3; b++) S[a * 3 + b] = ((RC[a * 3 + 0] * R[b * 3 + 0] + RC[a * 3 + 1] * R[b * 3 + 1]) + RC[a * 3 + 2] * R[b * 3 + 2]) + C2[a * 3 + b];
          // Eigen's 3 x 3 inverse: inv(r, c) = cofactor(c, r) / det, det along column 0
          auto cof = [&S](int i0, int j0) {
            const int i1 = (i0 + 1) % 3, i2 = (i0 + 2) % 3, j1 = (j0 + 1) % 3, j2 = (j0 + 2) % 3;
            return S[i1 * 3 + j1] * S[i2 * 3 + j2] - S[i1 * 3 + j2] * S[i2 * 3 + j1];
          };
          const double det = (cof(0, 0) * S[0] + cof(1, 0) * S[3]) + cof(2, 0) * S[6];
          const double invdet = 1.0 / det;
          for (int a = 0; a < 3; a++)
            for (int b = 0; b < 3; b++) Mi[a * 3 + b] = cof(b, a) * invdet;
#pragma unroll
          for (int k = 0; k < 9; k++) Mp[(size_t)k * c.total + it.off + pos] = Mi[k];
          acc[0] += 1.0;
        }
        Q[it.off + pos] = q;
      }
    }
  } else {
    if (threadIdx.x == 0) pg_apply_state(st->xt, sT);
    __syncthreads();
    const int pos = slice * kPgSlicePoints + (int)threadIdx.x;
    if (pos < n) {
      const float4 q = Q[it.off + pos];
      if (q.w != 0.f) {
        const float4 w = W[it.off + pos];
        const float ppx = affine_row_rn(sT[0], sT[1], sT[2], sT[3], w.x, w.y, w.z);
        const float ppy = affine_row_rn(sT[4], sT[5], sT[6], sT[7], w.x, w.y, w.z);
        const float ppz = affine_row_rn(sT[8], sT[9], sT[10], sT[11], w.x, w.y, w.z);
        const double r0 = (double)ppx - (double)q.x, r1 = (double)ppy - (double)q.y, r2 = (double)ppz - (double)q.z;
        double M[9];
#pragma unroll
        for (int k = 0; k < 9; k++) M[k] = Mp[(size_t)k * c.total + it.off + pos];
        const double t0 = (M[0] * r0 + M[1] * r1) + M[2] * r2;
        const double t1 = (M[3] * r0 + M[4] * r1) + M[5] * r2;
        const double t2 = (M[6] * r0 + M[7] * r1) + M[8] * r2;
        const double p0 = w.x, p1 = w.y, p2 = w.z;
        acc[0] = (r0 * t0 + r1 * t1) + r2 * t2;
        acc[1] = t0; acc[2] = t1; acc[3] = t2;
        acc[4] = p0 * t0; acc[5] = p0 * t1; acc[6] = p0 * t2;
        acc[7] = p1 * t0; acc[8] = p1 * t1; acc[9] = p1 * t2;
        acc[10] = p2 * t0; acc[11] = p2 * t1; acc[12] = p2 * t2;
      }
    }
  }
  // this slice's row, the pair's ticket; in the pair's closing workgroup the rows summed in slice order (slice_rows.h)
  __shared__ double tot[kPgPad];
  if (!slice_rows_close(acc, correspond ? 1 : kPgAccum, rows, it.slice0, it.n_slices, &st->ticket, tot)) return;
  if (threadIdx.x == 0) pg_close(st, tot, c, done_counter, traj_T, traj_i, traj_f, pair);
}

// One round of every active pair against the handle's target.
__global__ __launch_bounds__(kBlock) void pg_round_kernel(const BvhView tv, const float4* __restrict__ tgt, const double* __restrict__ tcov, const PgItem* __restrict__ items,
                                                          PgPair* __restrict__ pairs, const int* __restrict__ blk_pair, const float4* __restrict__ W,
                                                          float4* __restrict__ Q, double* __restrict__ Mp, double* __restrict__ rows, const PgConsts c,
                                                          int* __restrict__ done_counter, float* __restrict__ traj_T, int* __restrict__ traj_i,
                                                          double* __restrict__ traj_f) {
  const int pair = blk_pair[blockIdx.x];
  PgPair* st = pairs + pair;
  if (!st->active) return;   // uniform per pair: the closing workgroup clears it after every slice of this launch has read it
  const PgItem it = items[pair];
  pg_round_body(tv, tgt, tcov, it, st, pair, W, Q, Mp, rows, c, done_counter, traj_T, traj_i, traj_f);
}

// Per-pair targets (pcl_gicp_align_pairs): the same round, but the target's index view, points and covariances are not kernel arguments.
// They are an entry of a device table, chosen by PgItem::tgt.  blk_pair[blockIdx.x] is workgroup-uniform and items[pair] a scalar load, so
// targets[it.tgt] has a uniform address: its 64 bytes come in through scalar loads, once per wave, and live in SGPRs where pg_round_kernel
// keeps its arguments.  No lane loads a target field.
struct PgTarget {
  BvhView b;            // exact-NN index of the target cloud
  const float4* pts;    // its points in the caller's order
  const double* pcov;   // its PCL-style covariances, 9 doubles per point
  int n, pad;
};
static_assert(sizeof(PgTarget) == 64, "one target is one 64-byte scalar load");

__global__ __launch_bounds__(kBlock) void pg_round_pairs_kernel(const PgTarget* __restrict__ targets, const PgItem* __restrict__ items, PgPair* __restrict__ pairs,
                                                                const int* __restrict__ blk_pair, const float4* __restrict__ W, float4* __restrict__ Q,
                                                                double* __restrict__ Mp, double* __restrict__ rows, const PgConsts c,
                                                                int* __restrict__ done_counter, float* __restrict__ traj_T, int* __restrict__ traj_i,
                                                                double* __restrict__ traj_f) {
  const int pair = blk_pair[blockIdx.x];
  PgPair* st = pairs + pair;
  if (!st->active) return;
  const PgItem it = items[pair];
  const PgTarget t = targets[it.tgt];   // uniform address: scalar loads
  pg_round_body(t.b, t.pts, t.pcov, it, st, pair, W, Q, Mp, rows, c, done_counter, traj_T, traj_i, traj_f);
}

__global__ void pg_init_kernel(PgPair* __restrict__ pairs, const PgInit* __restrict__ inits, const int n_pairs) {
  const int pi = blockIdx.x * blockDim.x + threadIdx.x;
  if (pi >= n_pairs) return;
  PgPair* s = pairs + pi;
  const PgInit* in = inits + pi;
  for (int r = 0; r < 4; r++)
    for (int c = 0; c < 4; c++) {
      s->guess[r * 4 + c] = in->guess[c * 4 + r];
      s->T[r * 4 + c] = in->T[c * 4 + r];
    }
  for (int k = 0; k < 16; k++) s->final_T[k] = in->guess[k];
  for (int k = 0; k < 6; k++) {
    s->x[k] = s->x0[k] = s->g[k] = s->g0[k] = s->p[k] = s->cg[k] = s->cx[k] = 0.0;
    s->xt[k] = in->x[k];
  }
  s->f = s->g0norm = s->pnorm = s->fp0 = s->delta_f = s->f0s = s->ck = s->cf = s->ta = 0.0;
  s->ls_f0 = s->ls_fp0 = s->alpha = s->alpha_prev = s->falpha_prev = s->fpalpha_prev = 0.0;
  s->a = s->b = s->fa = s->fb = s->fpa = s->fpb = s->alpha_new = 0.0;
  s->score = DBL_MAX;
  s->phase = PG_CORRESPOND;
  s->resume = PG_AT_INIT;
  s->ls_i = s->ls_status = s->inner = s->passes = s->m = 0;
  s->active = (in->n > 0 && !in->skip) ? 1 : 0;   // an empty source never starts (PCL's initCompute refuses it)
  s->iterations = 0;
  s->evaluations = 0;
  s->converged = 0;
  s->ticket = 0;
  s->probe = in->probe;
  pg_set_R(s);
}

// ================================================================================================ host
static PgConsts pg_consts(const dgs_handle* h) {
  PgConsts c;
  const double d = h->prm.gicp_max_correspondence_distance;
  const double max_sq = d * d;
  float g = (float)max_sq;   // round to nearest, then step down until (double) g < max_sq
  if (!(max_sq > 0.0)) g = -1.f;
  else if (max_sq > (double)FLT_MAX) g = FLT_MAX;
  else if ((double)g >= max_sq) g = std::nextafter(g, 0.f);
  c.gate = g;
  c.trans_eps = h->prm.transformation_epsilon;
  c.rot_eps = h->pg_opt.rotation_epsilon;
  c.max_iterations = h->prm.maximum_iterations;
  c.max_inner = h->pg_opt.max_optimizer_iterations;
  c.traj_cap = std::max(1, h->prm.maximum_iterations);
  c.total = 0;
  return c;
}

// the PCL-style covariances of a cloud, computed once per (k, epsilon)
int ensure_pcov(dgs_handle* h, CloudState& c) {
  const int k = h->prm.gicp_correspondence_randomness;
  const double eps = h->pg_opt.gicp_epsilon;
  if (c.pcov_valid && c.pcov_k == k && c.pcov_eps == eps) return DGS_OK;
  if (k > kKnnMaxWide) {
    h->err = kKnnTooWide;
    return DGS_ERR_UNSUPPORTED;
  }
  if ((int64_t)k > c.n) {
    h->err = "k_correspondences_ exceeds the number of points of the cloud";
    return DGS_ERR_INVALID_ARGUMENT;
  }
  DGS_HIP_TRY(h, c.pcov.reserve((size_t)c.n * 9));
  int slot = prof_begin(h, DGS_K_GICP_COVARIANCE);
  int stride = 0;
  int rc = knn_lists(h, c, k, nullptr, &stride);
  if (rc) return rc;
  const BvhView v = make_bvh_view(c.bvh);
  if (stride == kKnnMaxWide)
    hipLaunchKernelGGL(pg_cov_wide_kernel, dim3((unsigned)((c.n + kPgWideBlock - 1) / kPgWideBlock)), dim3(kPgWideBlock), 0, h->stream, v, c.pts.ptr, (int)c.n, k, eps, h->knn_nbr.ptr, c.pcov.ptr);
  else
    hipLaunchKernelGGL(pg_cov_kernel, dim3((unsigned)((c.n + kBlock - 1) / kBlock)), dim3(kBlock), 0, h->stream, v, c.pts.ptr, (int)c.n, k, eps, h->knn_nbr.ptr, c.pcov.ptr);
  prof_end(h, DGS_K_GICP_COVARIANCE, slot);
  DGS_HIP_TRY(h, hipGetLastError());
  c.pcov_valid = true;
  c.pcov_k = k;
  c.pcov_eps = eps;
  return DGS_OK;
}

using PgStaging = BatchStaging<PgInit, PgItem, PgPair>;

// Per-pair targets of a batch (pcl_gicp_align_pairs): the distinct target clouds, indexed and with their covariances, and pair i's entry
// of[i] of that table; of[i] < 0: the pair has no usable target and never becomes active.
struct PgTargets {
  int n;
  CloudState* const* clouds;
  const int* of;
};

// computeTransformation for every source of a batch, against the handle's target or (tg != nullptr) each against the target it names
// (probe != nullptr: one pair, the test hook's single correspondence + evaluation pass; single-target only).  Per-pair status in
// out[i].status.  A pair that never becomes active -- an empty source, a source of fewer than k points, no usable target -- owns no
// slice and no slot of the work arrays.
static int pg_run_batch(dgs_handle* h, int n, CloudState* const* srcs, const float* guesses16, dgs_result* out, const double* probe_x,
                        PgPair* probe_out, const PgTargets* tg = nullptr) {
  hipStream_t st = h->stream;
  PgConsts c = pg_consts(h);
  int rc = DGS_OK;
  if (!tg) {
    rc = ensure_target_index(h);
    if (rc) return rc;
    rc = ensure_pcov(h, *h->tgt);
    if (rc) return rc;
  }
  const int k = h->prm.gicp_correspondence_randomness;
  int64_t total = 0;
  int n_live = 0;
  std::vector<int> skip(n, 0);
  std::vector<long long> off(n);
  std::vector<int64_t> live_n(n, 0);
  std::vector<CloudState*> live;
  for (int i = 0; i < n; i++) {
    CloudState& s = *srcs[i];
    off[i] = total;
    if (s.n <= 0) continue;
    if ((int64_t)k > s.n || (tg && tg->of[i] < 0)) { skip[i] = 1; continue; }   // computeCovariances refuses the cloud: this registration fails
    rc = ensure_walk_order(h, s);
    if (rc) return rc;
    live.push_back(&s);
    live_n[i] = s.n;
    total += s.n;
    n_live++;
  }
  // the sources' covariances: one batched pass (cov_batch.hip), a lone source on the single pass; pcl_gicp_align_pairs has made them with its targets'
  if (!tg) {
    rc = live.size() == 1 ? ensure_pcov(h, *live[0]) : ensure_covariances(h, (int)live.size(), live.data(), covplan::kPcl);
    if (rc) return rc;
  }
  SliceTable slices(live_n, kPgSlicePoints);
  const int total_slices = slices.total_slices;
  c.total = std::max<int64_t>(total, 1);
  DGS_HIP_TRY(h, h->pgpairs.reserve(n));
  DGS_HIP_TRY(h, h->pgitems.reserve(n));
  DGS_HIP_TRY(h, h->pginits.reserve(n));
  DGS_HIP_TRY(h, h->pg_w.reserve((size_t)c.total));
  DGS_HIP_TRY(h, h->pg_q.reserve((size_t)c.total));
  DGS_HIP_TRY(h, h->pg_m.reserve((size_t)c.total * 9));
  DGS_HIP_TRY(h, h->pg_traj_T.reserve((size_t)n * c.traj_cap * 16));
  DGS_HIP_TRY(h, h->pg_traj_i.reserve((size_t)n * c.traj_cap * 3));
  DGS_HIP_TRY(h, h->pg_traj_f.reserve((size_t)n * c.traj_cap));
  DGS_HIP_TRY(h, h->done_counter.reserve(16));
  const PgStaging stg(h, n);
  // the target table travels from the pinned block, behind the batch's own staging
  const size_t tab_off = (stg.bytes + 63) & ~(size_t)63, tab_bytes = tg ? (size_t)std::max(tg->n, 1) * sizeof(PgTarget) : 0;
  if (ensure_pinned(h, tab_off + tab_bytes) != DGS_OK) return DGS_ERR_HIP;
  PgInit* hin = stg.inits();
  PgItem* hit = stg.items();
  for (int i = 0; i < n; i++) {
    const CloudState& s = *srcs[i];
    std::memset(&hin[i], 0, sizeof(PgInit));
    std::memcpy(hin[i].guess, probe_x ? h->pg_probe_guess : (guesses16 ? guesses16 + 16 * i : kIdentity16), sizeof(float) * 16);
    std::memcpy(hin[i].T, probe_x ? h->pg_probe_T : kIdentity16, sizeof(float) * 16);
    if (probe_x)
      for (int a = 0; a < 6; a++) hin[i].x[a] = probe_x[a];
    hin[i].n = (int)s.n;
    hin[i].skip = skip[i];
    hin[i].probe = probe_x ? 1 : 0;
    hit[i].src = s.pts.ptr;
    hit[i].src_sorted = walk_sorted(s);
    hit[i].cs = s.pcov.ptr;
    hit[i].off = off[i];
    hit[i].n = (int)live_n[i];
    hit[i].slice0 = slices.slice0[i];
    hit[i].n_slices = slices.n_slices[i];
    hit[i].tgt = tg ? std::max(tg->of[i], 0) : 0;
  }
  rc = slices.upload(h, kPgPad);
  if (rc) return rc;
  DGS_HIP_TRY(h, hipMemcpyAsync(h->pginits.ptr, hin, (size_t)n * sizeof(PgInit), hipMemcpyHostToDevice, st));
  DGS_HIP_TRY(h, hipMemcpyAsync(h->pgitems.ptr, hit, (size_t)n * sizeof(PgItem), hipMemcpyHostToDevice, st));
  if (tg && n_live > 0) {
    DGS_HIP_TRY(h, h->pgtargets.reserve((size_t)tg->n));
    PgTarget* tab = reinterpret_cast<PgTarget*>(reinterpret_cast<char*>(h->pinned) + tab_off);
    for (int t = 0; t < tg->n; t++) {
      const CloudState& tc = *tg->clouds[t];
      tab[t] = PgTarget{make_bvh_view(tc.bvh), tc.pts.ptr, tc.pcov.ptr, (int)tc.n, 0};
    }
    DGS_HIP_TRY(h, hipMemcpyAsync(h->pgtargets.ptr, tab, (size_t)tg->n * sizeof(PgTarget), hipMemcpyHostToDevice, st));
  }
  DGS_HIP_TRY(h, hipMemsetAsync(h->done_counter.ptr, 0, 16 * sizeof(int), st));
  hipLaunchKernelGGL(pg_init_kernel, dim3((n + 63) / 64), dim3(64), 0, st, h->pgpairs.ptr, h->pginits.ptr, n);
  if (total_slices > 0)
    hipLaunchKernelGGL(pg_prepare_kernel, dim3(total_slices), dim3(kBlock), 0, st, h->pgitems.ptr, h->pgpairs.ptr, h->slice_blk_pair.ptr, h->pg_w.ptr);
  DGS_HIP_TRY(h, hipGetLastError());
  DGS_HIP_TRY(h, hipStreamSynchronize(st));   // slices.blk is pageable host memory
  const BvhView tv = tg ? BvhView{} : make_bvh_view(h->tgt->bvh);
  auto launch_round = [&]() {
    int slot = prof_begin(h, DGS_K_NN_SEARCH);
    if (tg)
      hipLaunchKernelGGL(pg_round_pairs_kernel, dim3(total_slices), dim3(kBlock), 0, st, h->pgtargets.ptr, h->pgitems.ptr, h->pgpairs.ptr, h->slice_blk_pair.ptr,
                         h->pg_w.ptr, h->pg_q.ptr, h->pg_m.ptr, h->slice_rows.ptr, c, h->done_counter.ptr, h->pg_traj_T.ptr, h->pg_traj_i.ptr, h->pg_traj_f.ptr);
    else
      hipLaunchKernelGGL(pg_round_kernel, dim3(total_slices), dim3(kBlock), 0, st, tv, h->tgt->pts.ptr, h->tgt->pcov.ptr, h->pgitems.ptr, h->pgpairs.ptr,
                         h->slice_blk_pair.ptr, h->pg_w.ptr, h->pg_q.ptr, h->pg_m.ptr, h->slice_rows.ptr, c, h->done_counter.ptr, h->pg_traj_T.ptr, h->pg_traj_i.ptr,
                         h->pg_traj_f.ptr);
    prof_end(h, DGS_K_NN_SEARCH, slot);
  };
  if (n_live > 0) {
    // every round is one pass of every live pair: at most 1 correspondence pass, 1 start and 2 * kPgLsIters + 1 trial points per inner
    // iteration, per outer iteration
    const long max_rounds = probe_x ? 2 : (long)std::max(1, c.max_iterations) * (2 + (long)std::max(1, c.max_inner) * (2 * kPgLsIters + 1));
    rc = run_rounds_polled(h, n_live, max_rounds, 8, launch_round);
    if (rc != DGS_OK) return rc;
  }
  rc = stg.read_back(h->pgpairs, n, "GICP_HIP state");
  if (rc) return rc;
  const PgPair* hp = stg.pairs();
  if (probe_out) {
    *probe_out = hp[0];
    return DGS_OK;
  }
  long evals = 0;
  h->pg_last_iters.assign(n, 0);
  h->pg_traj_cap = c.traj_cap;
  for (int i = 0; i < n; i++) {
    std::memcpy(out[i].final_transformation, hp[i].final_T, sizeof(float) * 16);
    const bool empty = srcs[i]->n <= 0;
    const bool ran = !empty && !skip[i];
    out[i].converged = (ran && !hp[i].active) ? hp[i].converged : 0;
    out[i].iterations = hp[i].iterations;
    out[i].evaluations = hp[i].evaluations;
    out[i].status = empty ? DGS_ERR_NO_SOURCE : (skip[i] ? DGS_ERR_INVALID_ARGUMENT : DGS_OK);
    out[i].score = hp[i].score;
    out[i].fitness = NAN;
    evals += hp[i].evaluations;
    h->pg_last_iters[i] = hp[i].iterations;
  }
  h->last_evaluations = evals;
  return DGS_OK;
}

int pcl_gicp_align_batch(dgs_handle* h, int n, CloudState* const* srcs, const float* guesses16, dgs_result* out) {
  return pg_run_batch(h, n, srcs, guesses16, out, nullptr, nullptr);
}

int pcl_gicp_align(dgs_handle* h, const float* guess16, dgs_result* out) {
  CloudState* one[1] = {h->src};
  int rc = pg_run_batch(h, 1, one, guess16, out, nullptr, nullptr);
  if (rc == DGS_OK && out->status == DGS_ERR_INVALID_ARGUMENT) {
    h->err = "k_correspondences_ exceeds the number of source points";
    return DGS_ERR_INVALID_ARGUMENT;
  }
  return rc;
}

// ---- per-pair targets: pair i = (tgts[i], srcs[i], guess i), every pair in its own phase of the same round launches
// (pg_round_pairs_kernel).  The handle's own target, source, last result and counts are not touched; the trajectory arrays answer for
// this batch afterwards.  A pair whose target is empty or has fewer than k points never becomes active: out[i].status says which (an
// empty target first, then an empty source, then k > n of either cloud); the other pairs run.
int pcl_gicp_align_pairs(dgs_handle* h, int n, dgs_cloud* const* tgts, dgs_cloud* const* srcs, const float* guesses16, dgs_result* out) {
  const int k = h->prm.gicp_correspondence_randomness;
  if (k > kKnnMaxWide) {
    h->err = kKnnTooWide;
    return DGS_ERR_UNSUPPORTED;
  }
  // the distinct targets that can serve (not empty, at least k points), by pointer, in order of first appearance
  std::vector<dgs_cloud*> uniq;
  std::vector<int> tgt_of((size_t)n);
  for (int i = 0; i < n; i++) {
    tgt_of[i] = -1;
    if (tgts[i]->st.n <= 0 || (int64_t)k > tgts[i]->st.n) continue;
    const auto at = std::find(uniq.begin(), uniq.end(), tgts[i]);
    tgt_of[i] = (int)(at - uniq.begin());
    if (at == uniq.end()) uniq.push_back(tgts[i]);
  }
  // every index that is missing, of targets and sources alike, in ONE batched build (the bits of a single build: fitness_batch.hip)
  std::vector<dgs_cloud*> all(tgts, tgts + n);
  all.insert(all.end(), srcs, srcs + n);
  StageCounts build;
  int rc = fitness_batch_build_indices(h, 2 * n, all.data(), &build);
  if (rc) return rc;
  // the covariances of the distinct targets and of the live pairs' sources in ONE batched pass (cov_batch.hip), cached on the cloud under
  // (k, epsilon): shared with every other path that uses the cloud
  std::vector<CloudState*> tc(uniq.size()), cs((size_t)n), need;
  for (size_t t = 0; t < uniq.size(); t++) {
    tc[t] = &uniq[t]->st;
    need.push_back(tc[t]);
  }
  for (int i = 0; i < n; i++) {
    cs[i] = &srcs[i]->st;
    if (tgt_of[i] >= 0 && cs[i]->n >= (int64_t)k) need.push_back(cs[i]);
  }
  rc = ensure_covariances(h, (int)need.size(), need.data(), covplan::kPcl);
  h->cb.counts8[7] = build.built;
  if (rc) return rc;
  const PgTargets tg{(int)uniq.size(), tc.data(), tgt_of.data()};
  const int64_t own_evaluations = h->last_evaluations;   // dgs_get_counts keeps reporting the handle's own last align / batch
  rc = pg_run_batch(h, n, cs.data(), guesses16, out, nullptr, nullptr, &tg);
  h->last_evaluations = own_evaluations;
  if (rc) return rc;
  for (int i = 0; i < n; i++)
    if (tgts[i]->st.n <= 0) out[i].status = DGS_ERR_NO_TARGET;
  return DGS_OK;
}

// device pointer and stride of the batch's final transforms (column-major float[16] per pair) for the fitness kernel
const float* pcl_gicp_final_transforms(dgs_handle* h, size_t* stride_bytes) {
  *stride_bytes = sizeof(PgPair);
  return reinterpret_cast<const float*>(reinterpret_cast<const char*>(h->pgpairs.ptr) + offsetof(PgPair, final_T));
}

int pcl_gicp_covariances(dgs_handle* h, int which, double* host_out9, int64_t n) {
  CloudState& c = which ? *h->tgt : *h->src;
  int rc = ensure_pcov(h, c);
  if (rc) return rc;
  DGS_HIP_TRY(h, hipStreamSynchronize(h->stream));
  DGS_HIP_TRY(h, hipMemcpy(host_out9, c.pcov.ptr, (size_t)n * 9 * sizeof(double), hipMemcpyDeviceToHost));
  return DGS_OK;
}

int pcl_gicp_evaluate(dgs_handle* h, const double* x6, int32_t* m, double* f, double* g6) {
  CloudState* one[1] = {h->src};
  dgs_result r;
  PgPair p;
  if ((int64_t)h->prm.gicp_correspondence_randomness > h->src->n) {
    h->err = "k_correspondences_ exceeds the number of source points";
    return DGS_ERR_INVALID_ARGUMENT;
  }
  int rc = pg_run_batch(h, 1, one, nullptr, &r, x6, &p);
  if (rc) return rc;
  *m = p.m;
  *f = p.f;
  for (int a = 0; a < 6; a++) g6[a] = p.g[a];
  return DGS_OK;
}

int pcl_gicp_trajectory(dgs_handle* h, int pair, float* T16s, int32_t* n_corr, int32_t* inner, int32_t* passes, double* f, int capacity, int* len) {
  int m;
  size_t e;
  int rc = traj_window(h->pg_last_iters, h->pg_traj_cap, pair, capacity, len, &m, &e);
  if (rc || m == 0) return rc;
  DGS_HIP_TRY(h, hipStreamSynchronize(h->stream));
  if (T16s) DGS_HIP_TRY(h, hipMemcpy(T16s, h->pg_traj_T.ptr + e * 16, (size_t)m * 16 * sizeof(float), hipMemcpyDeviceToHost));
  if (f) DGS_HIP_TRY(h, hipMemcpy(f, h->pg_traj_f.ptr + e, (size_t)m * sizeof(double), hipMemcpyDeviceToHost));
  if (n_corr || inner || passes) {
    std::vector<int> t((size_t)m * 3);
    DGS_HIP_TRY(h, hipMemcpy(t.data(), h->pg_traj_i.ptr + e * 3, t.size() * sizeof(int), hipMemcpyDeviceToHost));
    for (int k = 0; k < m; k++) {
      if (n_corr) n_corr[k] = t[(size_t)k * 3 + 0];
      if (inner) inner[k] = t[(size_t)k * 3 + 1];
      if (passes) passes[k] = t[(size_t)k * 3 + 2];
    }
  }
  return DGS_OK;
}

void pcl_gicp_release(dgs_handle* h) {
  h->pgpairs.release(); h->pgitems.release(); h->pginits.release(); h->pgtargets.release(); h->pg_w.release(); h->pg_q.release(); h->pg_m.release();
  h->pg_traj_T.release(); h->pg_traj_i.release(); h->pg_traj_f.release();
}

}  // namespace dgs
