// The NDT optimiser on the device: the next evaluation's transform and angle tables (write_evaluation), the More-Thuente line
// search, the Newton step (begin_iteration / end_iteration), the state machine ndt_advance, and the two things that drive it for
// the default order: ndt_close_evaluation (a workgroup sums a pair's rows and advances it) and ndt_solve_kernel (the stand-alone
// solve launch of the unfused paths).  Included by ndt_align.hip inside namespace dgs, below ndt_fast.h and the contraction
// pragma (every operation here is rounded on its own), above ndt_strict.h, which calls ndt_advance.  Needs handle.h and solve6.h.

// ================================================================================================ solver
// float transform + angle-derivative tables of pose x (computeAngleDerivatives: double trig, |angle| < 1e-4 snap),
// written to the pair's HBM record by lane 0 (`writer`); every lane computes the same values.
// double sin/cos is software on the GPU (~100s of instructions per call) and an evaluation needs twelve of them; when the
// whole wave runs this code with identical inputs (solve kernel), lane k evaluates angle k and the results are broadcast.
// pcl_ndt.hip includes this file with DGS_NDT_PCL_DOUBLE defined: PCL_NDT_HIP evaluates every kind in double, so write_evaluation leaves the
// double angle vectors with every evaluation, and the stand-alone kernels of this file and ndt_strict.h are left to ndt_align.hip.
#ifdef DGS_NDT_PCL_DOUBLE
constexpr bool kNdtDoubleTablesAlways = true;
#else
constexpr bool kNdtDoubleTablesAlways = false;
#endif
template <bool WAVE>
__device__ __forceinline__ void trig6(const double* ang, double* sn, double* cs) {
  if (WAVE) {
    const int lane = threadIdx.x & 63;
    // the six angles as values, chosen by selects: chosen by index, `ang` is a stack array read at a per-lane offset (48 B of scratch per lane
    // in every kernel that inlines this)
    const double a0 = ang[0], a1 = ang[1], a2 = ang[2], a3 = ang[3], a4 = ang[4], a5 = ang[5];
    const double a = (lane == 5) ? a5 : (lane == 4) ? a4 : (lane == 3) ? a3 : (lane == 2) ? a2 : (lane == 1) ? a1 : a0;
    double sv, cv;
    sincos(a, &sv, &cv);
#pragma unroll
    for (int k = 0; k < 6; k++) { sn[k] = readlane_f64(sv, k); cs[k] = readlane_f64(cv, k); }
  } else {
#pragma unroll
    for (int k = 0; k < 6; k++) sincos(ang[k], &sn[k], &cs[k]);
  }
}

template <bool COH>
__device__ __forceinline__ void hdr_put(float* p, float v) {
  if (COH) __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  else *p = v;
}
template <bool COH>
__device__ __forceinline__ void hdr_put_int(int* p, int v) {
  if (COH) __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  else *p = v;
}

// `hdr` receives what the derivative pass of the evaluation reads (transform, angle tables, need_hessian): the pair's own record, or -- in
// the queue kernel -- the record slot of the pair's NEXT round; final_T always goes to the pair's record `st`.
// COH: read by other workgroups of the SAME launch (queue kernel): every word is written through (agent-scope stores)
template <bool WAVE, bool COH = false>
__device__ __forceinline__ void write_evaluation(NdtPair* st, NdtPair* hdr, NdtSolver& s, const NdtConsts& c, const double* x, int need_hessian, bool write_T, bool writer) {
  // angles 0..2: the FLOAT-rounded pose angles (transform entries), 3..5: the double pose angles (derivative tables)
  const double ang[6] = {(double)(float)x[3], (double)(float)x[4], (double)(float)x[5], x[3], x[4], x[5]};
  double sn[6], cs[6];
  trig6<WAVE>(ang, sn, cs);
  if (write_T) {
    // Eigen builds Translation * AngleAxis(x) * AngleAxis(y) * AngleAxis(z) in float.  One ulp of a rotation entry moves
    // a point at 50 m by 3 um, which the q = x' - mean cancellation turns into ~1e-4 of that point's contribution, so
    // the entries are formed reproducibly: trig of the FLOAT angle evaluated in double and rounded once (what a
    // correctly rounded cosf/sinf returns), products individually rounded in the source order of the expression.
    const float cx = (float)cs[0], sx = (float)sn[0], cy = (float)cs[1], sy = (float)sn[1], cz = (float)cs[2], sz = (float)sn[2];
    const float r00 = mul_rn(cy, cz), r01 = mul_rn(-cy, sz), r02 = sy;
    const float r10 = add_rn(mul_rn(cx, sz), mul_rn(mul_rn(sx, sy), cz)), r11 = sub_rn(mul_rn(cx, cz), mul_rn(mul_rn(sx, sy), sz)), r12 = mul_rn(-sx, cy);
    const float r20 = sub_rn(mul_rn(sx, sz), mul_rn(mul_rn(cx, sy), cz)), r21 = add_rn(mul_rn(sx, cz), mul_rn(mul_rn(cx, sy), sz)), r22 = mul_rn(cx, cy);
    const float t0 = (float)x[0], t1 = (float)x[1], t2 = (float)x[2];
    if (writer) {
      hdr_put<COH>(&hdr->T[0], r00); hdr_put<COH>(&hdr->T[1], r01); hdr_put<COH>(&hdr->T[2], r02); hdr_put<COH>(&hdr->T[3], t0);
      hdr_put<COH>(&hdr->T[4], r10); hdr_put<COH>(&hdr->T[5], r11); hdr_put<COH>(&hdr->T[6], r12); hdr_put<COH>(&hdr->T[7], t1);
      hdr_put<COH>(&hdr->T[8], r20); hdr_put<COH>(&hdr->T[9], r21); hdr_put<COH>(&hdr->T[10], r22); hdr_put<COH>(&hdr->T[11], t2);
      float* F = st->final_T;  // column-major
      hdr_put<COH>(&F[0], r00); hdr_put<COH>(&F[1], r10); hdr_put<COH>(&F[2], r20); hdr_put<COH>(&F[3], 0.f);
      hdr_put<COH>(&F[4], r01); hdr_put<COH>(&F[5], r11); hdr_put<COH>(&F[6], r21); hdr_put<COH>(&F[7], 0.f);
      hdr_put<COH>(&F[8], r02); hdr_put<COH>(&F[9], r12); hdr_put<COH>(&F[10], r22); hdr_put<COH>(&F[11], 0.f);
      hdr_put<COH>(&F[12], t0); hdr_put<COH>(&F[13], t1); hdr_put<COH>(&F[14], t2); hdr_put<COH>(&F[15], 1.f);
    }
  }
  double cx, cy, cz, sx, sy, sz;
  if (fabs(x[3]) < 10e-5) { cx = 1.0; sx = 0.0; } else { cx = cs[3]; sx = sn[3]; }
  if (fabs(x[4]) < 10e-5) { cy = 1.0; sy = 0.0; } else { cy = cs[4]; sy = sn[4]; }
  if (fabs(x[5]) < 10e-5) { cz = 1.0; sz = 0.0; } else { cz = cs[5]; sz = sn[5]; }
  if (writer) {
    float (*J)[3] = hdr->jang;
    hdr_put<COH>(&J[0][0], (float)(-sx * sz + cx * sy * cz)); hdr_put<COH>(&J[0][1], (float)(-sx * cz - cx * sy * sz)); hdr_put<COH>(&J[0][2], (float)(-cx * cy));
    hdr_put<COH>(&J[1][0], (float)(cx * sz + sx * sy * cz));  hdr_put<COH>(&J[1][1], (float)(cx * cz - sx * sy * sz));  hdr_put<COH>(&J[1][2], (float)(-sx * cy));
    hdr_put<COH>(&J[2][0], (float)(-sy * cz));                hdr_put<COH>(&J[2][1], (float)(sy * sz));                 hdr_put<COH>(&J[2][2], (float)(cy));
    hdr_put<COH>(&J[3][0], (float)(sx * cy * cz));            hdr_put<COH>(&J[3][1], (float)(-sx * cy * sz));           hdr_put<COH>(&J[3][2], (float)(sx * sy));
    hdr_put<COH>(&J[4][0], (float)(-cx * cy * cz));           hdr_put<COH>(&J[4][1], (float)(cx * cy * sz));            hdr_put<COH>(&J[4][2], (float)(-cx * sy));
    hdr_put<COH>(&J[5][0], (float)(-cy * sz));                hdr_put<COH>(&J[5][1], (float)(-cy * cz));                hdr_put<COH>(&J[5][2], 0.f);
    hdr_put<COH>(&J[6][0], (float)(cx * cz - sx * sy * sz));  hdr_put<COH>(&J[6][1], (float)(-cx * sz - sx * sy * cz)); hdr_put<COH>(&J[6][2], 0.f);
    hdr_put<COH>(&J[7][0], (float)(sx * cz + cx * sy * sz));  hdr_put<COH>(&J[7][1], (float)(cx * sy * cz - sx * sz));  hdr_put<COH>(&J[7][2], 0.f);
    float (*H)[3] = hdr->hang;
    if (need_hessian) {  // a score + gradient evaluation (More-Thuente trial) never reads the second-derivative tables
    hdr_put<COH>(&H[0][0], (float)(-cx * sz - sx * sy * cz)); hdr_put<COH>(&H[0][1], (float)(-cx * cz + sx * sy * sz)); hdr_put<COH>(&H[0][2], (float)(sx * cy));    // a2
    hdr_put<COH>(&H[1][0], (float)(-sx * sz + cx * sy * cz)); hdr_put<COH>(&H[1][1], (float)(-cx * sy * sz - sx * cz)); hdr_put<COH>(&H[1][2], (float)(-cx * cy));   // a3
    hdr_put<COH>(&H[2][0], (float)(cx * cy * cz));            hdr_put<COH>(&H[2][1], (float)(-cx * cy * sz));           hdr_put<COH>(&H[2][2], (float)(cx * sy));    // b2
    hdr_put<COH>(&H[3][0], (float)(sx * cy * cz));            hdr_put<COH>(&H[3][1], (float)(-sx * cy * sz));           hdr_put<COH>(&H[3][2], (float)(sx * sy));    // b3
    hdr_put<COH>(&H[4][0], (float)(-sx * cz - cx * sy * sz)); hdr_put<COH>(&H[4][1], (float)(sx * sz - cx * sy * cz));  hdr_put<COH>(&H[4][2], 0.f);                 // c2
    hdr_put<COH>(&H[5][0], (float)(cx * cz - sx * sy * sz));  hdr_put<COH>(&H[5][1], (float)(-sx * sy * cz - cx * sz)); hdr_put<COH>(&H[5][2], 0.f);                 // c3
    // d1: upstream PCL / ndt_omp carry +sy in the z slot; the exact second derivative is -sy (dgs_params.ndt_fix_hessian_d1)
    hdr_put<COH>(&H[6][0], (float)(-cy * cz));                hdr_put<COH>(&H[6][1], (float)(cy * sz));                 hdr_put<COH>(&H[6][2], (float)(c.fix_hessian_d1 ? -sy : sy));
    hdr_put<COH>(&H[7][0], (float)(-sx * sy * cz));           hdr_put<COH>(&H[7][1], (float)(sx * sy * sz));            hdr_put<COH>(&H[7][2], (float)(sx * cy));    // d2
    hdr_put<COH>(&H[8][0], (float)(cx * sy * cz));            hdr_put<COH>(&H[8][1], (float)(-cx * sy * sz));           hdr_put<COH>(&H[8][2], (float)(-cx * cy));   // d3
    hdr_put<COH>(&H[9][0], (float)(sy * sz));                 hdr_put<COH>(&H[9][1], (float)(sy * cz));                 hdr_put<COH>(&H[9][2], 0.f);                 // e1
    hdr_put<COH>(&H[10][0], (float)(-sx * cy * sz));          hdr_put<COH>(&H[10][1], (float)(-sx * cy * cz));          hdr_put<COH>(&H[10][2], 0.f);                // e2
    hdr_put<COH>(&H[11][0], (float)(cx * cy * sz));           hdr_put<COH>(&H[11][1], (float)(cx * cy * cz));           hdr_put<COH>(&H[11][2], 0.f);                // e3
    hdr_put<COH>(&H[12][0], (float)(-cy * cz));               hdr_put<COH>(&H[12][1], (float)(cy * sz));                hdr_put<COH>(&H[12][2], 0.f);                // f1
    hdr_put<COH>(&H[13][0], (float)(-cx * sz - sx * sy * cz)); hdr_put<COH>(&H[13][1], (float)(-cx * cz + sx * sy * sz)); hdr_put<COH>(&H[13][2], 0.f);              // f2
    hdr_put<COH>(&H[14][0], (float)(-sx * sz + cx * sy * cz)); hdr_put<COH>(&H[14][1], (float)(-cx * sy * sz - sx * cz)); hdr_put<COH>(&H[14][2], 0.f);              // f3
    }
    if (need_hessian == 2 || kNdtDoubleTablesAlways) {   // computeHessian in PCL's double form reads the double angle vectors (never inside the queue kernel: plain stores)
      double (*Jd)[3] = hdr->jang_d;
      Jd[0][0] = (-sx * sz + cx * sy * cz); Jd[0][1] = (-sx * cz - cx * sy * sz); Jd[0][2] = (-cx * cy);
      Jd[1][0] = (cx * sz + sx * sy * cz);  Jd[1][1] = (cx * cz - sx * sy * sz);  Jd[1][2] = (-sx * cy);
      Jd[2][0] = (-sy * cz);                Jd[2][1] = (sy * sz);                 Jd[2][2] = (cy);
      Jd[3][0] = (sx * cy * cz);            Jd[3][1] = (-sx * cy * sz);           Jd[3][2] = (sx * sy);
      Jd[4][0] = (-cx * cy * cz);           Jd[4][1] = (cx * cy * sz);            Jd[4][2] = (-cx * sy);
      Jd[5][0] = (-cy * sz);                Jd[5][1] = (-cy * cz);                Jd[5][2] = 0.0;
      Jd[6][0] = (cx * cz - sx * sy * sz);  Jd[6][1] = (-cx * sz - sx * sy * cz); Jd[6][2] = 0.0;
      Jd[7][0] = (sx * cz + cx * sy * sz);  Jd[7][1] = (cx * sy * cz - sx * sz);  Jd[7][2] = 0.0;
      double (*Hd)[3] = hdr->hang_d;
      Hd[0][0] = (-cx * sz - sx * sy * cz); Hd[0][1] = (-cx * cz + sx * sy * sz); Hd[0][2] = (sx * cy);
      Hd[1][0] = (-sx * sz + cx * sy * cz); Hd[1][1] = (-cx * sy * sz - sx * cz); Hd[1][2] = (-cx * cy);
      Hd[2][0] = (cx * cy * cz);            Hd[2][1] = (-cx * cy * sz);           Hd[2][2] = (cx * sy);
      Hd[3][0] = (sx * cy * cz);            Hd[3][1] = (-sx * cy * sz);           Hd[3][2] = (sx * sy);
      Hd[4][0] = (-sx * cz - cx * sy * sz); Hd[4][1] = (sx * sz - cx * sy * cz);  Hd[4][2] = 0.0;
      Hd[5][0] = (cx * cz - sx * sy * sz);  Hd[5][1] = (-sx * sy * cz - cx * sz); Hd[5][2] = 0.0;
      Hd[6][0] = (-cy * cz);                Hd[6][1] = (cy * sz);                 Hd[6][2] = (c.fix_hessian_d1 ? -sy : sy);
      Hd[7][0] = (-sx * sy * cz);           Hd[7][1] = (sx * sy * sz);            Hd[7][2] = (sx * cy);
      Hd[8][0] = (cx * sy * cz);            Hd[8][1] = (-cx * sy * sz);           Hd[8][2] = (-cx * cy);
      Hd[9][0] = (sy * sz);                 Hd[9][1] = (sy * cz);                 Hd[9][2] = 0.0;
      Hd[10][0] = (-sx * cy * sz);          Hd[10][1] = (-sx * cy * cz);          Hd[10][2] = 0.0;
      Hd[11][0] = (cx * cy * sz);           Hd[11][1] = (cx * cy * cz);           Hd[11][2] = 0.0;
      Hd[12][0] = (-cy * cz);               Hd[12][1] = (cy * sz);                Hd[12][2] = 0.0;
      Hd[13][0] = (-cx * sz - sx * sy * cz); Hd[13][1] = (-cx * cz + sx * sy * sz); Hd[13][2] = 0.0;
      Hd[14][0] = (-sx * sz + cx * sy * cz); Hd[14][1] = (-cx * sy * sz - sx * cz); Hd[14][2] = 0.0;
    }
    hdr_put_int<COH>(&hdr->need_hessian, need_hessian);
  }
#pragma unroll
  for (int k = 0; k < 6; k++) s.x_t[k] = x[k];
}

// ---- More-Thuente helpers (More & Thuente 1994; Sun & Yuan 2006 eq. 2.4.x) ---------------------------------
__device__ inline double mt_psi(double a, double f_a, double f_0, double g_0, double mu) { return f_a - f_0 - mu * g_0 * a; }
__device__ inline double mt_dpsi(double g_a, double g_0, double mu) { return g_a - mu * g_0; }

__device__ __forceinline__ double mt_trial_value(double a_l, double f_l, double g_l, double a_u, double f_u, double g_u, double a_t, double f_t, double g_t) {
  if (f_t > f_l) {
    const double z = 3 * (f_t - f_l) / (a_t - a_l) - g_t - g_l;
    const double w = sqrt(z * z - g_t * g_l);
    const double a_c = a_l + (a_t - a_l) * (w - g_l - z) / (g_t - g_l + 2 * w);
    const double a_q = a_l - 0.5 * (a_l - a_t) * g_l / (g_l - (f_l - f_t) / (a_l - a_t));
    return (fabs(a_c - a_l) < fabs(a_q - a_l)) ? a_c : 0.5 * (a_q + a_c);
  } else if (g_t * g_l < 0) {
    const double z = 3 * (f_t - f_l) / (a_t - a_l) - g_t - g_l;
    const double w = sqrt(z * z - g_t * g_l);
    const double a_c = a_l + (a_t - a_l) * (w - g_l - z) / (g_t - g_l + 2 * w);
    const double a_s = a_l - (a_l - a_t) / (g_l - g_t) * g_l;
    return (fabs(a_c - a_t) >= fabs(a_s - a_t)) ? a_c : a_s;
  } else if (fabs(g_t) <= fabs(g_l)) {
    const double z = 3 * (f_t - f_l) / (a_t - a_l) - g_t - g_l;
    const double w = sqrt(z * z - g_t * g_l);
    const double a_c = a_l + (a_t - a_l) * (w - g_l - z) / (g_t - g_l + 2 * w);
    const double a_s = a_l - (a_l - a_t) / (g_l - g_t) * g_l;
    const double a_n = (fabs(a_c - a_t) < fabs(a_s - a_t)) ? a_c : a_s;
    return (a_t > a_l) ? fmin(a_t + 0.66 * (a_u - a_t), a_n) : fmax(a_t + 0.66 * (a_u - a_t), a_n);
  }
  const double z = 3 * (f_t - f_u) / (a_t - a_u) - g_t - g_u;
  const double w = sqrt(z * z - g_t * g_u);
  return a_u + (a_t - a_u) * (w - g_u - z) / (g_t - g_u + 2 * w);
}

__device__ __forceinline__ bool mt_update_interval(double& a_l, double& f_l, double& g_l, double& a_u, double& f_u, double& g_u, double a_t, double f_t,
                                   double g_t) {
  if (f_t > f_l) {
    a_u = a_t; f_u = f_t; g_u = g_t;
    return false;
  } else if (g_t * (a_l - a_t) > 0) {
    a_l = a_t; f_l = f_t; g_l = g_t;
    return false;
  } else if (g_t * (a_l - a_t) < 0) {
    a_u = a_l; f_u = f_l; g_u = g_l;
    a_l = a_t; f_l = f_t; g_l = g_t;
    return false;
  }
  return true;
}

constexpr double kMu = 1.e-4, kNu = 0.9;

__device__ inline double dot6(const double* a, const double* b) {
  return a[0] * b[0] + a[1] * b[1] + a[2] * b[2] + a[3] * b[3] + a[4] * b[4] + a[5] * b[5];
}

// Starts one outer iteration from (score, grad, hess) at s.p.  Returns true when an evaluation was queued,
// false when the iteration finished without one (zero step) or the registration ended.
// STRICT: the upstream evaluation orders -- JacobiSVD(H).solve(-g) in the CPU checker's sequence of operations (Eigen's two-sided
// Jacobi across the wave, or rounds 2-3's one-sided Jacobi: dgs_params.ndt_newton_solver); otherwise the default order's Gauss-Jordan
// step.  A template argument, not a run-time test, so that the default order's fused kernel carries none of the SVD code.
// fast_solver (STRICT only): the direction from the Gauss-Jordan elimination instead -- a SPECULATED step (ndt_strict.h): the exact one follows
// beside the next launch and the closing behind it verifies; *fast_ok tells whether the elimination was well conditioned.
template <bool STRICT, bool SVD_REGS, bool COH = false>
__device__ __forceinline__ bool begin_iteration(NdtPair* st, NdtPair* hdr, NdtSolver& s, const NdtConsts& c, bool writer, const bool fast_solver = false, bool* fast_ok = nullptr) {
  double neg_g[6], delta[6], rc;
#pragma unroll
  for (int k = 0; k < 6; k++) neg_g[k] = -s.grad[k];
  if (STRICT && fast_solver) {
    gj_solve6_columns(s.hess, s.grad, delta, &rc);
    *fast_ok = rc > 1e-10;
    if (!*fast_ok) return false;
  } else if (STRICT) {
    if (c.newton_solver) jsvd_solve6_wave(s.hess, neg_g, delta);
    else if (SVD_REGS) svd_solve6_regs_dev(s.hess, neg_g, delta, 1e-17, 60);
    else svd_solve6_dev(s.hess, neg_g, delta, 1e-17, 60);
  } else {
    gj_solve6_columns(s.hess, s.grad, delta, &rc);
    if (!(rc > 1e-13)) svd_solve6_dev(s.hess, neg_g, delta);
  }
#ifdef DGS_CLOSE_STAMPS
  if (threadIdx.x == 0 && st->s.nr_iterations == 1) st->traj[kTrajCap - 2][0] = (double)wall_clock64();
#endif
  double norm = sqrt(dot6(delta, delta));
  if (norm == 0 || norm != norm) {
    s.converged = (norm == norm) ? 1 : 0;
    s.phase = PH_DONE;
    return false;
  }
#pragma unroll
  for (int k = 0; k < 6; k++) s.dir[k] = delta[k] / norm;
  // computeStepLengthMT(p, dir, norm, step_size, eps / 2, ...)
  s.phi_0 = -s.score;
  s.d_phi_0 = -dot6(s.grad, s.dir);
  s.step_init = norm;
  if (s.d_phi_0 >= 0) {
    if (s.d_phi_0 == 0) {
      s.a_t = 0;  // "not a descent direction": zero step, no evaluation
      return false;
    }
    s.d_phi_0 = -s.d_phi_0;
#pragma unroll
    for (int k = 0; k < 6; k++) s.dir[k] = -s.dir[k];
  }
  const double step_max = c.step_size, step_min = c.trans_eps / 2;
  s.step_iterations = 0;
  s.trial_n = 0;
  s.trial_next = 0;
  s.a_l = 0; s.a_u = 0;
  s.f_l = mt_psi(0, s.phi_0, s.phi_0, s.d_phi_0, kMu);
  s.g_l = mt_dpsi(s.d_phi_0, s.d_phi_0, kMu);
  s.f_u = s.f_l;
  s.g_u = s.g_l;
  s.interval_converged = (c.line_search == DGS_NDT_LS_FIXED_STEP) ? ((step_max - step_min) > 0) : ((step_max - step_min) < 0);
  s.open_interval = 1;
  const double a_t = fmax(fmin(norm, step_max), step_min);
  s.a_t = a_t;
  double x[6];
#pragma unroll
  for (int k = 0; k < 6; k++) x[k] = s.p[k] + s.dir[k] * a_t;
#ifdef DGS_CLOSE_STAMPS
  if (threadIdx.x == 0 && st->s.nr_iterations == 1) st->traj[kTrajCap - 2][1] = (double)wall_clock64();
#endif
  write_evaluation<true, COH>(st, hdr, s, c, x, 1, true, writer);
#ifdef DGS_CLOSE_STAMPS
  if (threadIdx.x == 0 && st->s.nr_iterations == 1) st->traj[kTrajCap - 2][2] = (double)wall_clock64();
#endif
  s.phase = PH_MT_FIRST;
  return true;
}

// p += a_t * dir; convergence test of computeTransformation.  Returns true when the registration ended.
__device__ __forceinline__ bool end_iteration(NdtPair* st, NdtSolver& s, const NdtConsts& c, bool writer) {
  const double a = s.a_t;
#pragma unroll
  for (int k = 0; k < 6; k++) s.p[k] += s.dir[k] * a;
  if (writer && s.traj_len < kTrajCap) {
#pragma unroll
    for (int k = 0; k < 6; k++) st->traj[s.traj_len][k] = s.p[k];
  }
  s.traj_len++;
  bool conv = false;
  if (s.nr_iterations > c.max_iterations || (s.nr_iterations && (fabs(a) < c.trans_eps))) conv = true;
  s.nr_iterations++;
  if (conv) {
    s.converged = 1;
    s.phase = PH_DONE;
  }
  return conv;
}

__device__ inline bool mt_keep_going(const NdtSolver& s, const NdtConsts& c, double psi_t, double d_phi_t) {
  return !s.interval_converged && s.step_iterations < c.mt_max_step_iterations && !(psi_t <= 0 && d_phi_t <= -kNu * s.d_phi_0);
}

template <bool COH = false>
__device__ __forceinline__ void queue_trial(NdtPair* st, NdtPair* hdr, NdtSolver& s, const NdtConsts& c, double a_t, bool writer) {
  const double step_max = c.step_size, step_min = c.trans_eps / 2;
  a_t = fmax(fmin(a_t, step_max), step_min);
  s.a_t = a_t;
  double x[6];
#pragma unroll
  for (int k = 0; k < 6; k++) x[k] = s.p[k] + s.dir[k] * a_t;
  write_evaluation<true, COH>(st, hdr, s, c, x, 0, true, writer);
  s.phase = PH_MT_TRIAL;
}

// Consumes one evaluation result (already stored in s.score/grad/hess) and advances the state machine until
// the next evaluation is queued or the registration is finished.  Executed by all lanes of one wave in lock step.
// SVD_REGS: the stand-alone solve launch of the validation modes keeps the SVD workspace in registers (solve6.h)
// defer_solve (upstream order, ndt_strict.h): stop in front of the next iteration's Newton step (phase PH_SOLVE_PENDING); a later call
// with that phase -- from ndt_strict_solve_kernel -- continues there.
// speculate (upstream order, fused item-compacted kernel): take the next iteration's Newton step from the fast solver and tell the caller
// (*speculated) -- see NdtPair::spec_s.
// `make ab AB=-DDGS_NDT_REUSE_TRIALS=0`: ndt_advance without the reuse of cached trial poses (as DGS_NDT_REUSE_TRIALS=0 chooses at run time)
#ifndef DGS_NDT_REUSE_TRIALS
#define DGS_NDT_REUSE_TRIALS 1
#endif
// the entry of this line search's trial cache that holds pose s.x_t (all six doubles equal), or -1
__device__ __forceinline__ int trial_cached(const NdtSolver& s) {
  int hit = -1;
  for (int k = 0; k < s.trial_n; k++) {
    bool eq = true;
#pragma unroll
    for (int j = 0; j < 6; j++) eq = eq && (s.trial_x[k][j] == s.x_t[j]);
    if (eq && hit < 0) hit = k;
  }
  return hit;
}

template <bool SVD_REGS = false, bool COH = false, bool STRICT = false>
__device__ __forceinline__ void ndt_advance(NdtPair* st, NdtPair* hdr, NdtSolver& s, const NdtConsts& c, bool writer, bool defer_solve = false, bool speculate = false,
                                            bool* speculated = nullptr) {
  bool iteration_open = false;  // true: an iteration's line search has accepted its step, close it
  const bool resume = STRICT && s.phase == PH_SOLVE_PENDING;
  if (!resume) s.evaluations++;
  // One pass per trial consumed.  The upstream orders go round again when the trial just queued is a pose this line search has evaluated
  // before (NdtConsts::reuse_trials): its value is in the cache, so it is consumed here and now instead of costing the pair a launch.
  for (;;) {
  if (STRICT && (s.phase == PH_MT_FIRST || s.phase == PH_MT_TRIAL)) {
    // a trial point this line search has evaluated before takes the value it had then (NdtSolver::trial_x): same pose, same doubles, as on the CPU
    const int hit = trial_cached(s);
    if (hit >= 0) {
      s.trial_hits++;
      s.score = s.trial_score[hit];
#pragma unroll
      for (int j = 0; j < 6; j++) s.grad[j] = s.trial_grad[hit][j];
    } else {
      const int k = s.trial_next;
#pragma unroll
      for (int j = 0; j < 6; j++) { s.trial_x[k][j] = s.x_t[j]; s.trial_grad[k][j] = s.grad[j]; }
      s.trial_score[k] = s.score;
      s.trial_next = (k + 1) % NdtSolver::kTrialCache;
      if (s.trial_n < NdtSolver::kTrialCache) s.trial_n++;
    }
  }
  switch (resume ? PH_INIT_EVAL : s.phase) {
    case PH_PROBE:
      s.phase = PH_DONE;
      return;
    case PH_INIT_EVAL:
      break;
    case PH_MT_FIRST:
    case PH_MT_TRIAL: {
      const double phi_t = -s.score;
      const double d_phi_t = -dot6(s.grad, s.dir);
      const double psi_t = mt_psi(s.a_t, phi_t, s.phi_0, s.d_phi_0, kMu);
      const double d_psi_t = mt_dpsi(d_phi_t, s.d_phi_0, kMu);
      if (s.phase == PH_MT_TRIAL) {
        if (s.open_interval && (psi_t <= 0 && d_psi_t >= 0)) {
          s.open_interval = 0;
          s.f_l = s.f_l + s.phi_0 - kMu * s.d_phi_0 * s.a_l;
          s.g_l = s.g_l + kMu * s.d_phi_0;
          s.f_u = s.f_u + s.phi_0 - kMu * s.d_phi_0 * s.a_u;
          s.g_u = s.g_u + kMu * s.d_phi_0;
        }
        if (s.open_interval)
          s.interval_converged = mt_update_interval(s.a_l, s.f_l, s.g_l, s.a_u, s.f_u, s.g_u, s.a_t, psi_t, d_psi_t);
        else
          s.interval_converged = mt_update_interval(s.a_l, s.f_l, s.g_l, s.a_u, s.f_u, s.g_u, s.a_t, phi_t, d_phi_t);
        s.step_iterations++;
      }
      if (mt_keep_going(s, c, psi_t, d_phi_t)) {
        const double a_n = s.open_interval ? mt_trial_value(s.a_l, s.f_l, s.g_l, s.a_u, s.f_u, s.g_u, s.a_t, psi_t, d_psi_t)
                                           : mt_trial_value(s.a_l, s.f_l, s.g_l, s.a_u, s.f_u, s.g_u, s.a_t, phi_t, d_phi_t);
        // (queued in full on a hit too: the pair's record holds the transform and the angle tables of the pose in flight, which the
        //  computeHessian pass behind an accepted trial and final_T read)
        queue_trial<COH>(st, hdr, s, c, a_n, writer);
        if (STRICT && DGS_NDT_REUSE_TRIALS != 0 && c.reuse_trials && trial_cached(s) >= 0) {
          s.evaluations++;   // upstream's count: the CPU evaluates this pose again
          continue;          // mt_keep_going bounds the chain: every pass is a loop trial, step_iterations < mt_max_step_iterations
        }
        return;
      }
      if (s.step_iterations) {  // computeHessian at the accepted point
        double x[6];
#pragma unroll
        for (int k = 0; k < 6; k++) x[k] = s.x_t[k];
        write_evaluation<true, COH>(st, hdr, s, c, x, (STRICT && c.hessian_double) ? 2 : 1, false, writer);
        s.phase = PH_MT_HESSIAN;
        return;
      }
      iteration_open = true;
    } break;
    case PH_MT_HESSIAN:
      iteration_open = true;
      break;
    default:
      return;
  }
  break;
  }
  for (int guard = 0; guard < 4096; guard++) {
    if (iteration_open) {
      if (end_iteration(st, s, c, writer)) return;
    }
    if (STRICT && defer_solve) {   // the Newton step goes to the solve kernel
      s.phase = PH_SOLVE_PENDING;
      return;
    }
    if (STRICT && speculate) {
      bool ok = false;
      const int ph0 = s.phase, cv0 = s.converged;
      if (begin_iteration<STRICT, SVD_REGS, COH>(st, hdr, s, c, writer, true, &ok)) {   // evaluation queued from the speculated direction
        *speculated = true;
        return;
      }
      s.phase = ph0;
      s.converged = cv0;
      // ill-conditioned, or the fast step ends / skips the iteration: nothing was published that the exact step below does not overwrite
      // (its inputs -- p, score, gradient, Hessian -- are untouched)
    }
    if (begin_iteration<STRICT, SVD_REGS, COH>(st, hdr, s, c, writer)) return;  // evaluation queued
    if (s.phase == PH_DONE) return;
    iteration_open = true;                          // zero-step iteration: close it and try again
  }
  s.converged = 0;
  s.phase = PH_DONE;
}

// Sums a pair's partial rows in slice order and advances its optimiser by one evaluation; executed by one whole workgroup.
// launch >= 0: fused launches (the pair leaves through last_launch); launch < 0: ndt_solve_kernel (the pair leaves through active).
#ifdef DGS_CLOSE_STAMPS   // diagnostic build only (make dbg): 100 MHz wall-clock stamps of the closing phases into the pair's last trajectory rows
#define CLOSE_STAMP(k) if (threadIdx.x == 0 && st->s.nr_iterations == 1) st->traj[kTrajCap - 1][k] = (double)wall_clock64();
#else
#define CLOSE_STAMP(k)
#endif
// QUEUE: called inside the persistent queue kernel -- the pair's record was written by another workgroup of the SAME launch and will be
// read by others: coherent (agent-scope) loads and write-through stores for every word of it.  Returns (to the closing wave) whether
// the registration has ended.
// DONE_FLAG: `done_counter` is this pair's own flag in HOST memory (pinned, device-visible): a finished pair stores launch + 1 into it and the host
// counts the flags at every chunk boundary -- no copy command between the chunks of launches (each cost the stream ~8 us: a blit kernel
// and two barriers).  Otherwise a device counter that the host copies back.
template <bool QUEUE, bool DONE_FLAG>
__device__ __forceinline__ bool ndt_close_evaluation(NdtPair* st, const double* partials_of_pair, int blocks_per_pair, const NdtConsts& c, int* done_counter, int launch,
                                                     NdtPair* hdr_next, int need_h_in) {
  CLOSE_STAMP(0)
  __shared__ NdtSolver s_lds;   // the optimiser state lives in LDS: a register copy costs ~150 VGPRs
  NdtSolver& s = s_lds;
  // Everything read here comes from memory (the state from the previous launch, the rows from this one): issue it all at once --
  // the state word by word across the workgroup (one 8-byte load per thread instead of 38 dependent 16-byte loads in every lane
  // of one wave, which took 5 us of the 7 us this function used to take), the rows as before -- and pay ONE memory latency.
  static_assert(sizeof(NdtSolver) % 8 == 0 && sizeof(NdtSolver) / 8 <= kBlock, "state words");
  constexpr int kWords = (int)(sizeof(NdtSolver) / 8);
  double word = 0.0;
  if (threadIdx.x < kWords) word = QUEUE ? __hip_atomic_load(reinterpret_cast<const double*>(&st->s) + threadIdx.x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
                                         : reinterpret_cast<const double*>(&st->s)[threadIdx.x];
  const int need_h = need_h_in >= 0 ? need_h_in : st->need_hessian;   // queue kernel: the flag of the round being closed comes from its record slot
  // ---- finish the reduction: 8 strided groups x 32 columns, fixed order
  __shared__ double tot[kAccumPad];
  __shared__ double sm[kBlock / kAccumPad][kAccumPad];
  const int col = threadIdx.x % kAccumPad, grp = threadIdx.x / kAccumPad;
  constexpr int G = kBlock / kAccumPad;
  double v = 0.0;
  // four rows in flight per thread, added in slice order (a missing row adds +0.0, which changes nothing)
  for (int b0 = grp; b0 < blocks_per_pair; b0 += 4 * G) {
    double r[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const int b = b0 + k * G;
      const double* ptr = partials_of_pair + (size_t)min(b, blocks_per_pair - 1) * kAccumPad + col;
      // rows published inside this launch: agent-scope (sc1) loads, never a line this CU may hold from an earlier launch
      const double x = (launch >= 0) ? handoff_load_row(ptr) : *ptr;
      r[k] = (b < blocks_per_pair) ? x : 0.0;
    }
    v = (((v + r[0]) + r[1]) + r[2]) + r[3];
  }
  sm[grp][col] = v;
  if (threadIdx.x < kWords) reinterpret_cast<double*>(&s_lds)[threadIdx.x] = word;
  __syncthreads();
  if (threadIdx.x < kAccumPad) {
    double t = 0.0;
#pragma unroll
    for (int k = 0; k < G; k++) t += sm[k][threadIdx.x];
    tot[threadIdx.x] = t;
  }
  __syncthreads();
  CLOSE_STAMP(1)
  if (threadIdx.x >= kWave) return false;
  // ---- one wave advances the optimiser: every lane computes the same values, lane 0 writes the pair's record
  const bool writer = threadIdx.x == 0;
  // the totals into the optimiser state, one entry per lane: lanes 0..35 the symmetric Hessian (entry (i, j) <- upper-triangle slot of
  // (min, max)), 36..41 the gradient, 42 the score (all 64 lanes storing all 49 entries one after the other cost 0.7 us)
  {
    const int t = threadIdx.x;
    if (t < 36) {
      if (need_h) {
        const int i = t / 6, j = t % 6, lo = min(i, j), hi = max(i, j);
        s.hess[t] = tot[7 + lo * 6 - (lo * (lo - 1)) / 2 + (hi - lo)];
      }
    } else if (t < 42) {
      s.grad[t - 36] = tot[1 + t - 36];
    } else if (t == 42) {
      s.score = tot[0];
    }
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_s_waitcnt(0xc07f);   // lgkmcnt(0): the wave's LDS stores have landed
  }
  CLOSE_STAMP(2)
  ndt_advance<false, QUEUE>(st, hdr_next ? hdr_next : st, s, c, writer);
  CLOSE_STAMP(3)
  // write the state back word by word across the wave (lane 0 alone would issue 38 stores one after the other)
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_s_waitcnt(0xc07f);   // lgkmcnt(0): the wave's LDS stores have landed
  for (int w = threadIdx.x; w < kWords; w += kWave) {
    const double v = reinterpret_cast<const double*>(&s_lds)[w];
    if (QUEUE) __hip_atomic_store(reinterpret_cast<double*>(&st->s) + w, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else reinterpret_cast<double*>(&st->s)[w] = v;
  }
  if (writer && s.phase == PH_DONE) {
    st->active = 0;
    if (launch >= 0) st->last_launch = launch;
    if (DONE_FLAG) __hip_atomic_store(done_counter, launch + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);   // which launch ended it (ndt_align_pairs: early fitness)
    else atomicAdd(done_counter, 1);
  }
  CLOSE_STAMP(4)
  return s.phase == PH_DONE;
}

#ifndef DGS_NDT_PCL_DOUBLE
__global__ __launch_bounds__(kBlock) void ndt_solve_kernel(NdtPair* __restrict__ pairs, const double* __restrict__ partials, const int cap_blocks,
                                                           int* __restrict__ pair_blocks, const NdtConsts c, int* __restrict__ done_counter,
                                                           const double* __restrict__ strict_totals, const int strict_from_rows) {
  const int pair = blockIdx.x;
  NdtPair* st = pairs + pair;
  if (!st->active) return;
  if (!strict_totals) {
    ndt_close_evaluation(st, partials + (size_t)pair * cap_blocks * kAccumPad, pair_blocks[pair], c, done_counter, -1);
    return;
  }
  // validation modes: the sums of this evaluation were formed by ndt_strict_kernel's rows / ndt_strict_seqsum.  A pair that the
  // derivative launch in front of this one did not evaluate (the launch served the other evaluation kind, ndt_strict.h) has no rows.
  if (strict_from_rows) {
    if (pair_blocks[pair] == 0) return;
  }
  __shared__ NdtSolver s_lds;
  NdtSolver& s = s_lds;
  __shared__ double tot[kStrictPad];
  int need_h = 0;
  if (threadIdx.x < kWave) {
    s_lds = st->s;
    need_h = st->need_hessian;
  }
  if (threadIdx.x < kStrictPad) {
    if (strict_from_rows) {
      // order 1: the workgroups' rows added as the fused launch's closing adds them (ndt_close_strict, ndt_strict.h) -- five partial sums, sum
      // g over the rows g, g + 5, g + 10, ... in steps of four, (((v + r0) + r1) + r2) + r3 with 0.0 for a row the pair lacks, then the five
      // in order -- so that the two paths give the same bits whatever the row count (tests/test_strict_closing_rows_gpu.py).  It used to add
      // the rows one after the other in slice order: the same additions up to five rows, another association above (1-3 ulps of the score).
      const int nb = pair_blocks[pair];
      const double* base = partials + (size_t)pair * cap_blocks * kStrictPad + threadIdx.x;
      constexpr int G = kBlock / kStrictPad;
      double t = 0.0;
#pragma unroll 1
      for (int grp = 0; grp < G; grp++) {
        double v = 0.0;
        for (int b0 = grp; b0 < nb; b0 += 4 * G) {
          double r[4];
#pragma unroll
          for (int k = 0; k < 4; k++) {
            const int b = b0 + k * G;
            const double x = base[(size_t)min(b, nb - 1) * kStrictPad];
            r[k] = (b < nb) ? x : 0.0;
          }
          v = (((v + r[0]) + r[1]) + r[2]) + r[3];
        }
        t += v;
      }
      tot[threadIdx.x] = t;
    } else {
      tot[threadIdx.x] = strict_totals[(size_t)pair * kStrictPad + threadIdx.x];
    }
  }
  __syncthreads();
  if (threadIdx.x >= kWave) return;
  const bool writer = threadIdx.x == 0;
  if (need_h != 2) {   // kind 2 (computeHessian alone) leaves score and gradient as the last trial left them
    s.score = tot[0];
#pragma unroll
    for (int k = 0; k < 6; k++) s.grad[k] = tot[1 + k];
  }
  if (need_h) {
#pragma unroll
    for (int k = 0; k < 36; k++) s.hess[k] = tot[7 + k];  // upstream's full 6x6 (not exactly symmetric in float)
  }
  ndt_advance<true, false, true>(st, st, s, c, writer);
  if (writer) {
    if (strict_from_rows) pair_blocks[pair] = 0;   // consumed
    st->s = s;
    if (s.phase == PH_DONE) {
      st->active = 0;
      atomicAdd(done_counter, 1);
    }
  }
}
#endif
