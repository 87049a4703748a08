// K5 gicp_correspond, K6 gicp_linearize / gicp_error and the Levenberg-Marquardt driver on the device (K4 knn_covariance: gicp_cov.hip
// over knn_lists.hip).
//
// Replaces fast_gicp::FastGICP::computeTransformation (on fast_gicp::LsqRegistration), i.e. what
// registration->align(*aligned, guess) runs at /root/reference/apps/scan_matching_odometry_nodelet.cpp:218 and
// /root/reference/include/hdl_graph_slam/loop_detector.hpp:145 when registration_method is FAST_GICP (the value every
// shipped launch file sets; object configured at src/hdl_graph_slam/registrations.cpp:27-36).  Algorithm: SURVEY.md App. B.
//
// MI355X design
//   * No pointer kd-trees: both clouds get the implicit 8-ary AABB index of nn_bvh.hip (Hilbert ordered; the target of a large
//     batch k-d ordered).  k-NN covariances: one wave per index leaf (gicp_knn_leaf_kernel, knn_lists.hip); per-iteration 1-NN
//     correspondences: 8-lane groups (nn_group.h), exact and bounded by max_correspondence_distance.
//   * One linearisation = correspond (8 lanes / point) + linearize (1 lane / point, all double: RCR = C_B + R C_A R^T,
//     3x3 inverse, J = [skew(Tp) | -I], 21 + 6 + 1 sums) with the same wave-DPP -> LDS -> fixed-order partial rows as NDT,
//     so the sums are bit-reproducible (upstream's per-thread OpenMP partials are not).
//   * The optimiser step (LM / GN, se3_exp, the rho test, the convergence test) runs on one wave in the LAST workgroup of a pair's
//     linearize slice (gicp_close_round; gicp_solve_kernel is the same step as its own launch) and queues the next evaluation in
//     place: no host round trip per iteration.
#include <cfloat>
#include <cmath>
#include <cstddef>
#include <cstring>
#include <vector>

#include "batch_rounds.h"
#include "handle.h"
#include "nn_group.h"
#include "small_linalg.h"
#include "solve6.h"

namespace dgs {

// ================================================================================================ where a pair's target comes from
// The round kernels are written once and take their target from a policy, passed by value as the first kernel argument.  A batch against
// the handle's target carries it in the arguments (the index view for the search, points and covariances for the sums: two types, so
// each kernel's argument block holds what it reads and nothing more).  gicp_align_pairs -- pair i registers ITS source against ITS target,
// the loop detector's tick: every new keyframe is a target with a short candidate list of its own -- carries a device table with one
// 64-byte entry per distinct target, chosen by GicpItem::tgt.  deal_workgroup makes the pair index workgroup-uniform, so the entry's
// address is uniform too: it comes in through scalar loads, once per wave, and lives in SGPRs exactly where the other form keeps its
// arguments (load16_at's base, the walk's depth and first leaf).
struct GicpTarget {
  BvhView b;           // exact-NN index of the target cloud
  const float4* pts;   // its points in the caller's order
  const double* cov;   // its covariances, 6 doubles per point
  int n, pad;
};
static_assert(sizeof(GicpTarget) == 64, "one target is one 64-byte scalar load");

struct GicpBatchIndex {
  BvhView b;
  __device__ __forceinline__ const BvhView& index(const GicpItem&) const { return b; }
};
struct GicpBatchCloud {
  const float4* points;
  const double* covs;
  __device__ __forceinline__ const float4* pts(const GicpItem&) const { return points; }
  __device__ __forceinline__ const double* cov(const GicpItem&) const { return covs; }
};
struct GicpTargetTable {
  const GicpTarget* t;
  __device__ __forceinline__ const BvhView& index(const GicpItem& it) const { return t[it.tgt].b; }
  __device__ __forceinline__ const float4* pts(const GicpItem& it) const { return t[it.tgt].pts; }
  __device__ __forceinline__ const double* cov(const GicpItem& it) const { return t[it.tgt].cov; }
};

// ================================================================================================ K5 correspondences
// FastGICP::update_correspondences, search part: x' = float(T) * p in float, exact 1-NN in the target, accepted iff
// d^2 < corr_dist_threshold^2
template <class TGT>
__global__ __launch_bounds__(kBlock) void gicp_correspond_kernel(const TGT target, const GicpItem* __restrict__ items,
                                                                 const GicpPair* __restrict__ pairs, const int n_pairs, const int cap_blocks,
                                                                 const float max_sq) {
  // workgroups go to the pairs whose queued evaluation is a linearisation (an LM trial re-uses the stored correspondences)
  int pair, slice, bpp;
  if (!deal_workgroup(n_pairs, cap_blocks, [&](int pi) { return pairs[pi].active != 0 && pairs[pi].eval_kind == 0; }, pair, slice, bpp)) return;
  const GicpPair& st = pairs[pair];
  const GicpItem it = items[pair];
  const BvhView b = target.index(it);
  const int n = it.n;
  float T[12];
#pragma unroll
  for (int k = 0; k < 12; k++) T[k] = (float)st.Teval[k];
  const int sub = threadIdx.x & 7;
  constexpr int QPB = kBlock / 8;
  // every wave walks a contiguous stretch of the source in ITS index's (Hilbert) order (w = original index), 8 adjacent
  // points per round: the previous round's correspondences bound this round's searches (nn_warm_bound_round)
  const int run = (n + bpp * QPB - 1) / (bpp * QPB);
  const int first = (slice * (kBlock / kWave) + (threadIdx.x >> 6)) * (8 * run) + ((threadIdx.x & 63) >> 3);
  float px = 0.f, py = 0.f, pz = 0.f, prev_best = INFINITY;
  bool prev_found = false;
  for (int r = 0; r < run; r++) {
    const int pos = first + r * 8;
    const float4 p = (pos < n) ? it.src_sorted[pos] : make_float4(0.f, 0.f, 0.f, 0.f);
    const int i = (pos < n) ? (int)__float_as_uint(p.w) : -1;
    const bool alive = pos < n && i >= 0 && i < n;
    const float x = affine_row_rn(T[0], T[1], T[2], T[3], p.x, p.y, p.z);
    const float y = affine_row_rn(T[4], T[5], T[6], T[7], p.x, p.y, p.z);
    const float z = affine_row_rn(T[8], T[9], T[10], T[11], p.x, p.y, p.z);
    float best;
    int bi;
    // nothing farther than the threshold can be a correspondence
    const float bound = fminf(max_sq, nn_warm_bound_round(prev_best, prev_found, x, y, z, px, py, pz));
    nn_query_group(b, x, y, z, alive, bound, best, bi);
    prev_found = alive && bi != 0x7FFFFFFF;
    prev_best = best;
    px = x; py = y; pz = z;
    if (alive && sub == 0) {
      const bool ok = (bi != 0x7FFFFFFF) && (best < max_sq);
      it.corr[i] = ok ? bi : -1;
      it.corr_sq[i] = (bi != 0x7FFFFFFF) ? best : max_sq;
    }
  }
}

// One correspondence's contribution to E = sum w e^T M e, b = sum w J^T M e, H = sum w J^T M J with J = [skew(t) | -I]
// (t = T p, e = mean_B - t; FastGICP: w = 1, FastVGICP: w = sqrt(points in the voxel)).  acc: E, b[6], upper triangle of H.
template <bool WEIGHTED>
__device__ __forceinline__ void gicp_accumulate(double* acc, const double* M, const double e0, const double e1, const double e2, const double t0,
                                                const double t1, const double t2, const double w, const bool full) {
  double m0 = M[0] * e0 + M[1] * e1 + M[2] * e2;
  double m1 = M[1] * e0 + M[3] * e1 + M[4] * e2;
  double m2 = M[2] * e0 + M[4] * e1 + M[5] * e2;
  double err = e0 * m0 + e1 * m1 + e2 * m2;
  if (WEIGHTED) err *= w;
  acc[0] += err;
  if (full) {
    double Mw[6];
#pragma unroll
    for (int k = 0; k < 6; k++) Mw[k] = WEIGHTED ? w * M[k] : M[k];
    if (WEIGHTED) { m0 *= w; m1 *= w; m2 *= w; }
    // b = J^T M e = [ (Me) x t ; -Me ]
    acc[1] += m1 * t2 - m2 * t1;
    acc[2] += m2 * t0 - m0 * t2;
    acc[3] += m0 * t1 - m1 * t0;
    acc[4] += -m0;
    acc[5] += -m1;
    acc[6] += -m2;
    // H = J^T M J = [[S^T M S, -S^T M], [-M S, M]] with S = skew(t):  G = M S (3x3), then S^T G and -G^T
    const double Mf[9] = {Mw[0], Mw[1], Mw[2], Mw[1], Mw[3], Mw[4], Mw[2], Mw[4], Mw[5]};
    const double Sk[9] = {0, -t2, t1, t2, 0, -t0, -t1, t0, 0};
    double G[9];
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
      for (int c = 0; c < 3; c++) G[r * 3 + c] = Mf[r * 3 + 0] * Sk[0 * 3 + c] + Mf[r * 3 + 1] * Sk[1 * 3 + c] + Mf[r * 3 + 2] * Sk[2 * 3 + c];
    double Hrr[9];
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
      for (int c = 0; c < 3; c++) Hrr[r * 3 + c] = Sk[0 * 3 + r] * G[0 * 3 + c] + Sk[1 * 3 + r] * G[1 * 3 + c] + Sk[2 * 3 + r] * G[2 * 3 + c];
    // upper triangle, row-major: (0,0..5) (1,1..5) (2,2..5) (3,3..5) (4,4..5) (5,5)
    acc[7] += Hrr[0]; acc[8] += Hrr[1]; acc[9] += Hrr[2]; acc[10] += -G[0 * 3 + 0]; acc[11] += -G[1 * 3 + 0]; acc[12] += -G[2 * 3 + 0];
    acc[13] += Hrr[4]; acc[14] += Hrr[5]; acc[15] += -G[0 * 3 + 1]; acc[16] += -G[1 * 3 + 1]; acc[17] += -G[2 * 3 + 1];
    acc[18] += Hrr[8]; acc[19] += -G[0 * 3 + 2]; acc[20] += -G[1 * 3 + 2]; acc[21] += -G[2 * 3 + 2];
    acc[22] += Mw[0]; acc[23] += Mw[1]; acc[24] += Mw[2];
    acc[25] += Mw[3]; acc[26] += Mw[4];
    acc[27] += Mw[5];
  }
}

// Mahalanobis matrix of one correspondence: (C_B + R C_A R^T)^-1, symmetric 6-vector (3x3 block of upstream's 4x4)
__device__ __forceinline__ void gicp_mahalanobis(const double* T, const double* CA, const double* CB, double* M) {
  const double a0 = CA[0], a1 = CA[1], a2 = CA[2], a3 = CA[3], a4 = CA[4], a5 = CA[5];
  double RC[9];
#pragma unroll
  for (int r = 0; r < 3; r++) {
    const double r0 = T[r * 4 + 0], r1 = T[r * 4 + 1], r2 = T[r * 4 + 2];
    RC[r * 3 + 0] = r0 * a0 + r1 * a1 + r2 * a2;
    RC[r * 3 + 1] = r0 * a1 + r1 * a3 + r2 * a4;
    RC[r * 3 + 2] = r0 * a2 + r1 * a4 + r2 * a5;
  }
  double S[9];
#pragma unroll
  for (int r = 0; r < 3; r++)
#pragma unroll
    for (int c = 0; c < 3; c++) S[r * 3 + c] = RC[r * 3 + 0] * T[c * 4 + 0] + RC[r * 3 + 1] * T[c * 4 + 1] + RC[r * 3 + 2] * T[c * 4 + 2];
  S[0] += CB[0]; S[1] += CB[1]; S[2] += CB[2]; S[3] += CB[1]; S[4] += CB[3]; S[5] += CB[4]; S[6] += CB[2]; S[7] += CB[4]; S[8] += CB[5];
  double Mi[9];
  inv3_d(S, Mi);
  M[0] = Mi[0]; M[1] = Mi[1]; M[2] = Mi[2]; M[3] = Mi[4]; M[4] = Mi[5]; M[5] = Mi[8];
}

// wave DPP sums -> LDS -> one fixed-order row of kAccumPad doubles per workgroup
template <bool FUSED = false>
__device__ __forceinline__ void gicp_block_reduce(const double* acc, double* __restrict__ row) {
  __shared__ double sm[kBlock / kWave][kAccumPad];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < kAccum; k++) {
    const double v = wave_sum_to_lane63(acc[k]);
    if (lane == 63) sm[wave][k] = v;
  }
  __syncthreads();
  if (threadIdx.x < kAccumPad) {
    double v = 0.0;
    if (threadIdx.x < kAccum) v = ((sm[0][threadIdx.x] + sm[1][threadIdx.x]) + sm[2][threadIdx.x]) + sm[3][threadIdx.x];
    if (FUSED) {
      handoff_store_row(row + threadIdx.x, v);   // write-through: see gicp_close_round and common.h, "in-launch hand-off"
      handoff_drain_stores();
    } else {
      row[threadIdx.x] = v;
    }
  }
}

// ---- the optimiser (forced inline: inside the fused linearize kernels the launch bound of the linearize loop must govern, the
// tail spills what does not fit)
// ================================================================================================ solver
// so3_exp / se3_exp of fast_gicp (quaternion form); out = rows 0..2 of the 4x4, row-major 3x4
__device__ __forceinline__ void se3_exp_dev(const double* a, double* T) {
  const double wx = a[0], wy = a[1], wz = a[2];
  const double theta_sq = wx * wx + wy * wy + wz * wz;
  double imag, real;
  if (theta_sq < 1e-10) {
    const double tq = theta_sq * theta_sq;
    imag = 0.5 - 1.0 / 48.0 * theta_sq + 1.0 / 3840.0 * tq;
    real = 1.0 - 1.0 / 8.0 * theta_sq + 1.0 / 384.0 * tq;
  } else {
    const double theta = sqrt(theta_sq), half = 0.5 * theta;
    imag = sin(half) / theta;
    real = cos(half);
  }
  const double qw = real, qx = imag * wx, qy = imag * wy, qz = imag * wz;
  const double tx = 2 * qx, ty = 2 * qy, tz = 2 * qz;
  const double twx = tx * qw, twy = ty * qw, twz = tz * qw, txx = tx * qx, txy = ty * qx, txz = tz * qx, tyy = ty * qy, tyz = tz * qy, tzz = tz * qz;
  const double R[9] = {1 - (tyy + tzz), txy - twz, txz + twy, txy + twz, 1 - (txx + tzz), tyz - twx, txz - twy, tyz + twx, 1 - (txx + tyy)};
  const double theta = sqrt(theta_sq);
  double V[9];
  if (theta < 1e-10) {
    for (int i = 0; i < 9; i++) V[i] = R[i];
  } else {
    const double O[9] = {0, -wz, wy, wz, 0, -wx, -wy, wx, 0};
    double O2[9];
    for (int r = 0; r < 3; r++)
      for (int c = 0; c < 3; c++) O2[r * 3 + c] = O[r * 3 + 0] * O[0 * 3 + c] + O[r * 3 + 1] * O[1 * 3 + c] + O[r * 3 + 2] * O[2 * 3 + c];
    const double c1 = (1.0 - cos(theta)) / theta_sq, c2 = (theta - sin(theta)) / (theta_sq * theta);
    for (int i = 0; i < 9; i++) V[i] = ((i % 4 == 0) ? 1.0 : 0.0) + c1 * O[i] + c2 * O2[i];
  }
  for (int r = 0; r < 3; r++) {
    for (int c = 0; c < 3; c++) T[r * 4 + c] = R[r * 3 + c];
    T[r * 4 + 3] = V[r * 3 + 0] * a[3] + V[r * 3 + 1] * a[4] + V[r * 3 + 2] * a[5];
  }
}

__device__ __forceinline__ void iso_mul(const double* A, const double* B, double* C) {  // 3x4 isometries, C = A * B
  double T[12];
  for (int r = 0; r < 3; r++) {
    for (int c = 0; c < 4; c++) T[r * 4 + c] = A[r * 4 + 0] * B[0 * 4 + c] + A[r * 4 + 1] * B[1 * 4 + c] + A[r * 4 + 2] * B[2 * 4 + c];
    T[r * 4 + 3] += A[r * 4 + 3];
  }
  for (int k = 0; k < 12; k++) C[k] = T[k];
}

__device__ __forceinline__ bool gicp_is_converged(const double* delta, const GicpConsts& c) {
  double rmax = 0, tmax = 0;
  for (int r = 0; r < 3; r++) {
    for (int cc = 0; cc < 3; cc++) rmax = fmax(rmax, fabs(delta[r * 4 + cc] - (r == cc ? 1.0 : 0.0)) / c.rot_eps);
    tmax = fmax(tmax, fabs(delta[r * 4 + 3]) / c.trans_eps);
  }
  return fmax(rmax, tmax) < 1;
}

__device__ __forceinline__ void gicp_queue(GicpPair* st, const double* T, int kind, bool writer) {
  if (writer) {
    for (int k = 0; k < 12; k++) st->Teval[k] = T[k];
    st->eval_kind = kind;
  }
}

__device__ __forceinline__ void gicp_try_lm(GicpPair* st, GicpSolver& s, const GicpConsts& c, bool writer) {
  solve6_step(s.H, s.b, s.lambda, s.d);
  se3_exp_dev(s.d, s.delta);
  iso_mul(s.delta, s.x0, s.xi);
  gicp_queue(st, s.xi, 1, writer);
  s.phase = GP_ERROR_WAIT;
}

// after a successful optimisation step: convergence test of LsqRegistration::computeTransformation
__device__ __forceinline__ void gicp_after_step(GicpPair* st, GicpSolver& s, const GicpConsts& c, bool writer) {
  const bool conv = gicp_is_converged(s.delta, c);
  s.converged = conv ? 1 : 0;
  if (!conv && s.iteration + 1 < c.max_iterations) {
    s.iteration++;
    gicp_queue(st, s.x0, 0, writer);
    s.phase = GP_LINEARIZE_WAIT;
  } else {
    s.phase = GP_DONE;
  }
}

__device__ __forceinline__ void gicp_advance(GicpPair* st, GicpSolver& s, const GicpConsts& c, bool writer) {
  s.evaluations++;
  if (s.phase == GP_PROBE) {
    s.phase = GP_DONE;
    return;
  }
  if (s.phase == GP_LINEARIZE_WAIT) {
    if (c.optimizer == DGS_GICP_OPT_GAUSS_NEWTON) {
      solve6_step(s.H, s.b, 0.0, s.d);
      se3_exp_dev(s.d, s.delta);
      iso_mul(s.delta, s.x0, s.x0);
      gicp_after_step(st, s, c, writer);
      return;
    }
    if (s.lambda < 0.0) {
      double m = 0;
      for (int k = 0; k < 6; k++) m = fmax(m, fabs(s.H[k * 6 + k]));
      s.lambda = c.lm_init_lambda_factor * m;
    }
    s.nu = 2.0;
    s.lm_try = 0;
    gicp_try_lm(st, s, c, writer);
    return;
  }
  if (s.phase == GP_ERROR_WAIT) {
    double denom = 0;
    for (int k = 0; k < 6; k++) denom += s.d[k] * (s.lambda * s.d[k] - s.b[k]);
    const double rho = (s.y0 - s.yi) / denom;
    if (rho < 0) {
      if (gicp_is_converged(s.delta, c)) {  // step_lm returns true without moving x0
        gicp_after_step(st, s, c, writer);
        return;
      }
      s.lambda = s.nu * s.lambda;
      s.nu = 2 * s.nu;
      s.lm_try++;
      if (s.lm_try < c.lm_max_iterations) {
        gicp_try_lm(st, s, c, writer);
      } else {  // "lm not converged!!": the outer loop breaks, converged_ stays false
        s.converged = 0;
        s.phase = GP_DONE;
      }
      return;
    }
    for (int k = 0; k < 12; k++) s.x0[k] = s.xi[k];
    const double t = 2 * rho - 1;
    s.lambda = s.lambda * fmax(1.0 / 3.0, 1 - t * t * t);
    s.y0 = s.yi;
    gicp_after_step(st, s, c, writer);
  }
}

// The optimiser step of a registration from its partial rows: gicp_solve_kernel's body, also run by the LAST workgroup of a
// pair inside the linearize launch (fused rounds).  Rows are summed in the same order either way (bit-identical results).
template <bool FUSED>
__device__ __forceinline__ void gicp_step_from_rows(GicpPair* st, const double* __restrict__ partials, const int nblocks, const GicpConsts& c,
                                                    int* __restrict__ done_counter, const int launch) {
  __shared__ double sm[kBlock / kAccumPad][kAccumPad];
  __shared__ double tot[kAccumPad];
  __shared__ GicpSolver s_lds;   // the state lives in LDS: in registers it would cost the linearize loop half its occupancy
  const int col = threadIdx.x % kAccumPad, grp = threadIdx.x / kAccumPad;
  constexpr int G = kBlock / kAccumPad;
  double v = 0.0;
  for (int b = grp; b < nblocks; b += G) {
    const double* r = partials + (size_t)b * kAccumPad + col;
    v += FUSED ? handoff_load_row(r) : *r;
  }
  sm[grp][col] = v;
  {  // state -> LDS, word by word, by the whole workgroup
    const int* src = reinterpret_cast<const int*>(&st->s);
    int* dst = reinterpret_cast<int*>(&s_lds);
    for (int w = threadIdx.x; w < (int)(sizeof(GicpSolver) / sizeof(int)); w += kBlock) dst[w] = src[w];
  }
  __syncthreads();
  if (threadIdx.x < kAccumPad) {
    double t = 0.0;
#pragma unroll
    for (int k = 0; k < G; k++) t += sm[k][threadIdx.x];
    tot[threadIdx.x] = t;
  }
  __syncthreads();
  if (threadIdx.x >= kWave) return;
  const bool writer = threadIdx.x == 0;
  GicpSolver& s = s_lds;
  if (st->eval_kind == 0) {
    if (writer) {
      s.y0 = tot[0];
      for (int k = 0; k < 6; k++) s.b[k] = tot[1 + k];
      int q = 7;
      for (int i = 0; i < 6; i++)
        for (int j = i; j < 6; j++) {
          s.H[i * 6 + j] = tot[q];
          s.H[j * 6 + i] = tot[q];
          q++;
        }
    }
  } else if (writer) {
    s.yi = tot[0];
  }
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_s_waitcnt(0xc07f);
  gicp_advance(st, s, c, writer);
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_s_waitcnt(0xc07f);
  {
    const int* src = reinterpret_cast<const int*>(&s_lds);
    int* dst = reinterpret_cast<int*>(&st->s);
    for (int w = threadIdx.x; w < (int)(sizeof(GicpSolver) / sizeof(int)); w += kWave) dst[w] = src[w];
  }
  if (writer) {
    for (int r = 0; r < 3; r++)
      for (int cc = 0; cc < 4; cc++) st->final_T[cc * 4 + r] = (float)s.x0[r * 4 + cc];
    st->final_T[3] = st->final_T[7] = st->final_T[11] = 0.f;
    st->final_T[15] = 1.f;
    if (s.phase == GP_DONE) {
      st->active = 0;
      if (FUSED) st->last_launch = launch;
      atomicAdd(done_counter, 1);
    }
  }
}

// Fused rounds: after its row is published (write-through stores, drained) a workgroup takes a ticket of its pair; the one that
// takes the last ticket runs the pair's optimiser step -- the scheme of ndt_derivatives_kernel<.., fused> (ndt_align.hip).
// n_tickets: workgroups of the pair in this launch; n_rows: rows of the pair (the same number unless the slices are fixed).
__device__ __forceinline__ void gicp_close_round(GicpPair* pairs, const int pair, const int n_tickets, const int n_rows,
                                                 const double* __restrict__ partials_of_pair, const GicpConsts& c, int* __restrict__ done_counter,
                                                 const int launch) {
  __shared__ int s_last;
  __syncthreads();
  if (threadIdx.x == 0) {
    s_last = handoff_take_ticket(&pairs[pair].ticket, n_tickets) ? 1 : 0;
  }
  __syncthreads();
  if (!s_last) return;
  gicp_step_from_rows<true>(pairs + pair, partials_of_pair, n_rows, c, done_counter, launch);
}

// ================================================================================================ K6 linearize / error
// How a pair's sums are cut into rows.  FIXED = false: as many slices as the launch leaves the pair (deal_workgroup's blocks_per_pair),
// one per workgroup, so the association of its double sums follows the batch.  FIXED = true (dgs_set_batch_independent): the slices follow
// the pair's own size, S(n) = clamp(ceil(n / kBlock), 1, 512), point i in slice (i / kBlock) % S(n), the rows added by
// gicp_step_from_rows over S(n) rows -- the layout a LONE default align gets from gicp_choose_launch(1, n) and deal_workgroup, so a pair in
// any batch is bit-equal to its own single align.  A workgroup is still dealt (pair, slice, blocks_per_pair); it takes the slices slice,
// slice + blocks_per_pair, ... of the pair one after the other and ONE ticket after the last (a workgroup dealt no slice takes its
// ticket all the same: the count is blocks_per_pair, as in pcl_ndt.hip); the last ticket closes over S(n) rows.
// Both forms are one slice loop, which the first leaves after its only pass, over one point loop.  The point loop is spelled in the
// kernel and must stay there: reached through a device function that takes the item or the pair by reference, the compiler contracted
// a * b + c differently and the score left the lone align's by 1-4 ulp.
__device__ __forceinline__ int gicp_fixed_slices_of(const int n) { return max(1, min((n + kBlock - 1) / kBlock, 512)); }

// fused: the linearize loop keeps its 4 waves per SIMD; the optimiser tail (one workgroup per pair and launch) spills what does not fit
template <bool FUSED, bool FIXED, class TGT>
__global__ __launch_bounds__(kBlock, FUSED ? 4 : 1) void gicp_linearize_kernel(const TGT target, const GicpItem* __restrict__ items,
                                                                GicpPair* __restrict__ pairs, double* __restrict__ partials, const int n_pairs,
                                                                const int cap_blocks, int* __restrict__ pair_blocks, const GicpConsts consts,
                                                                int* __restrict__ done_counter, const int launch) {
  int pair, slice, nblocks;
  if (!deal_workgroup(n_pairs, cap_blocks, [&](int pi) { return FUSED ? (launch <= pairs[pi].last_launch) : (pairs[pi].active != 0); }, pair, slice, nblocks)) return;
  const GicpPair& st = pairs[pair];
  const GicpItem it = items[pair];
  const int n = it.n;
  const int n_rows = FIXED ? min(gicp_fixed_slices_of(n), cap_blocks) : nblocks;   // cap_blocks = S(largest source) >= S(n): the min only guards the rows
  if (slice == 0 && threadIdx.x == 0) pair_blocks[pair] = n_rows;
  const float4* __restrict__ src = it.src;
  const double* __restrict__ cov_s = it.cov_s;
  const int* __restrict__ corr = it.corr;
  double* __restrict__ mahal = it.mahal;
  const float4* __restrict__ tgt = target.pts(it);
  const double* __restrict__ cov_t = target.cov(it);
  const bool full = st.eval_kind == 0;
  double T[12];
#pragma unroll
  for (int k = 0; k < 12; k++) T[k] = st.Teval[k];
  double* __restrict__ rows_of_pair = partials + (size_t)pair * cap_blocks * kAccumPad;
  for (int q = slice; q < n_rows; q += nblocks) {
    double acc[kAccum];
#pragma unroll
    for (int k = 0; k < kAccum; k++) acc[k] = 0.0;

    for (int i = q * kBlock + threadIdx.x; i < n; i += n_rows * kBlock) {
      const int j = corr[i];
      if (j < 0) continue;
      const float4 pa = src[i], pb = tgt[j];
      double M[6];
      if (full) {
        gicp_mahalanobis(T, cov_s + (size_t)i * 6, cov_t + (size_t)j * 6, M);
        double* mo = mahal + (size_t)i * 6;
#pragma unroll
        for (int k = 0; k < 6; k++) mo[k] = M[k];
      } else {
        const double* mo = mahal + (size_t)i * 6;
#pragma unroll
        for (int k = 0; k < 6; k++) M[k] = mo[k];
      }
      const double ax = pa.x, ay = pa.y, az = pa.z;
      const double t0 = T[0] * ax + T[1] * ay + T[2] * az + T[3];
      const double t1 = T[4] * ax + T[5] * ay + T[6] * az + T[7];
      const double t2 = T[8] * ax + T[9] * ay + T[10] * az + T[11];
      gicp_accumulate<false>(acc, M, (double)pb.x - t0, (double)pb.y - t1, (double)pb.z - t2, t0, t1, t2, 1.0, full);
    }
    gicp_block_reduce<FUSED>(acc, rows_of_pair + (size_t)q * kAccumPad);
    if (!FIXED) break;
    __syncthreads();   // the row has been read out of gicp_block_reduce's LDS before the next slice's sums land there
  }
  if (FUSED) gicp_close_round(pairs, pair, nblocks, n_rows, rows_of_pair, consts, done_counter, launch);
}

// ================================================================================================ FAST_VGICP linearize / error
// FastVGICP::update_correspondences + linearize (eval_kind 0) or compute_error (eval_kind 1) in one pass: the voxel of T p
// (double) and its DIRECT1 / 7 / 27 neighbours are looked up in the dense cell table -- no tree, no distance gate --, every hit is
// a correspondence with Mahalanobis (cov_voxel + R cov_p R^T)^-1 and weight sqrt(points in the voxel).  An error-only
// evaluation re-uses the voxel ids and Mahalanobis matrices stored by the last linearisation, as upstream does.
// Rows and slice loop as in gicp_linearize_kernel; the point loop stays spelled here for the same reason.
template <bool FUSED, bool FIXED>
__global__ __launch_bounds__(kBlock, FUSED ? 3 : 1) void vgicp_linearize_kernel(const VgicpMap m, const GicpItem* __restrict__ items,
                                                                 GicpPair* __restrict__ pairs, double* __restrict__ partials,
                                                                 const int n_pairs, const int cap_blocks, int* __restrict__ pair_blocks,
                                                                 const GicpConsts consts, int* __restrict__ done_counter, const int launch) {
  int pair, slice, nblocks;
  if (!deal_workgroup(n_pairs, cap_blocks, [&](int pi) { return FUSED ? (launch <= pairs[pi].last_launch) : (pairs[pi].active != 0); }, pair, slice, nblocks)) return;
  const GicpPair& st = pairs[pair];
  const GicpItem it = items[pair];
  const int n = it.n, no = m.n_offsets;
  const int n_rows = FIXED ? min(gicp_fixed_slices_of(n), cap_blocks) : nblocks;
  if (slice == 0 && threadIdx.x == 0) pair_blocks[pair] = n_rows;
  double* __restrict__ rows_of_pair = partials + (size_t)pair * cap_blocks * kAccumPad;
  const bool full = st.eval_kind == 0;
  double T[12];
#pragma unroll
  for (int k = 0; k < 12; k++) T[k] = st.Teval[k];
  for (int q = slice; q < n_rows; q += nblocks) {
    double acc[kAccum];
#pragma unroll
    for (int k = 0; k < kAccum; k++) acc[k] = 0.0;
    for (int i = q * kBlock + threadIdx.x; i < n; i += n_rows * kBlock) {
      const float4 pa = it.src[i];
      const double ax = pa.x, ay = pa.y, az = pa.z;
      const double t0 = T[0] * ax + T[1] * ay + T[2] * az + T[3];
      const double t1 = T[4] * ax + T[5] * ay + T[6] * az + T[7];
      const double t2 = T[8] * ax + T[9] * ay + T[10] * az + T[11];
      // GaussianVoxelMap::voxel_coord: floor(x / resolution - 0.5), relative to the table's first cell
      const int c0 = (int)floor(t0 / m.resolution - 0.5) - m.min_c[0];
      const int c1 = (int)floor(t1 / m.resolution - 0.5) - m.min_c[1];
      const int c2 = (int)floor(t2 / m.resolution - 0.5) - m.min_c[2];
      for (int k = 0; k < no; k++) {
        const size_t slot = (size_t)i * no + k;
        int v;
        if (full) {
          int dx = 0, dy = 0, dz = 0;
          if (m.search == DGS_VGICP_DIRECT7) {  // (0,0,0) (1,0,0) (-1,0,0) (0,1,0) (0,-1,0) (0,0,1) (0,0,-1)
            dx = (k == 1) - (k == 2);
            dy = (k == 3) - (k == 4);
            dz = (k == 5) - (k == 6);
          } else if (m.search == DGS_VGICP_DIRECT27) {
            dx = k / 9 - 1;
            dy = (k / 3) % 3 - 1;
            dz = k % 3 - 1;
          }
          const int x = c0 + dx, y = c1 + dy, z = c2 + dz;
          v = -1;
          if (x >= 0 && x < m.div[0] && y >= 0 && y < m.div[1] && z >= 0 && z < m.div[2]) v = m.cell2vox[x + y * m.mul1 + z * m.mul2];
          it.corr[slot] = v;
        } else {
          v = it.corr[slot];
        }
        if (v < 0) continue;
        const VgicpVoxel* vx = m.vox + v;
        double M[6];
        if (full) {
          gicp_mahalanobis(T, it.cov_s + (size_t)i * 6, vx->cov, M);
#pragma unroll
          for (int a = 0; a < 6; a++) it.mahal[slot * 6 + a] = M[a];
        } else {
#pragma unroll
          for (int a = 0; a < 6; a++) M[a] = it.mahal[slot * 6 + a];
        }
        gicp_accumulate<true>(acc, M, vx->mean[0] - t0, vx->mean[1] - t1, vx->mean[2] - t2, t0, t1, t2, vx->w, full);
      }
    }
    gicp_block_reduce<FUSED>(acc, rows_of_pair + (size_t)q * kAccumPad);
    if (!FIXED) break;
    __syncthreads();   // the row has been read out of gicp_block_reduce's LDS before the next slice's sums land there
  }
  if (FUSED) gicp_close_round(pairs, pair, nblocks, n_rows, rows_of_pair, consts, done_counter, launch);
}

__global__ __launch_bounds__(kBlock) void gicp_solve_kernel(GicpPair* __restrict__ pairs, const double* __restrict__ all_partials,
                                                            const int* __restrict__ pair_blocks, const int cap_blocks, const GicpConsts c,
                                                            int* __restrict__ done_counter) {
  GicpPair* st = pairs + blockIdx.x;  // one workgroup per registration of the batch
  if (!st->active) return;
  gicp_step_from_rows<false>(st, all_partials + (size_t)blockIdx.x * cap_blocks * kAccumPad, pair_blocks[blockIdx.x], c, done_counter, -1);
}

struct GicpInit {
  double x0[12];
  int probe_kind;  // -1: normal align; 0 / 1: probe a linearisation / an error evaluation
  int n;           // source size: an empty source never becomes active (PCL's initCompute refuses it)
};

__global__ void gicp_init_kernel(GicpPair* __restrict__ pairs, const GicpInit* __restrict__ inits, const int n_pairs) {
  const int pi = blockIdx.x * blockDim.x + threadIdx.x;
  if (pi >= n_pairs) return;
  GicpPair* st = pairs + pi;
  const GicpInit* init = inits + pi;
  GicpSolver s;
  s.phase = (init->n <= 0) ? GP_DONE : (init->probe_kind >= 0) ? GP_PROBE : GP_LINEARIZE_WAIT;
  s.iteration = 0;
  s.evaluations = 0;
  s.converged = 0;
  s.lm_try = 0;
  s.pad = 0;
  for (int k = 0; k < 12; k++) { s.x0[k] = init->x0[k]; s.xi[k] = init->x0[k]; s.delta[k] = (k % 5 == 0) ? 1.0 : 0.0; st->Teval[k] = init->x0[k]; }
  for (int k = 0; k < 36; k++) s.H[k] = 0;
  for (int k = 0; k < 6; k++) { s.b[k] = 0; s.d[k] = 0; }
  s.y0 = s.yi = 0;
  s.lambda = -1.0;
  s.nu = 2.0;
  st->s = s;
  st->eval_kind = (init->probe_kind > 0) ? 1 : 0;
  st->active = (init->n > 0) ? 1 : 0;
  st->last_launch = (init->n > 0) ? 0x7FFFFFFF : -1;
  st->ticket = 0;
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 4; c++) st->final_T[c * 4 + r] = (float)init->x0[r * 4 + c];
  st->final_T[3] = st->final_T[7] = st->final_T[11] = 0.f;
  st->final_T[15] = 1.f;
}

// ================================================================================================ host side
static void fill_gconsts(dgs_handle* h) {
  GicpConsts& c = h->gconsts;
  const dgs_params& p = h->prm;
  c.trans_eps = p.transformation_epsilon;
  c.rot_eps = p.gicp_rotation_epsilon;
  c.lm_init_lambda_factor = p.gicp_lm_init_lambda_factor;
  const float dmax = (float)p.gicp_max_correspondence_distance;
  c.max_corr_sq = dmax * dmax;
  c.max_iterations = p.maximum_iterations;
  c.optimizer = p.gicp_optimizer;
  c.lm_max_iterations = p.gicp_lm_max_iterations;
  c.k = p.gicp_correspondence_randomness;
  c.regularization = p.gicp_regularization;
}

// Launch shape of one batch: per-pair caps (what a lone registration gets) and grids dealt over the active pairs.
struct GicpLaunch {
  int n_pairs, cap_c, cap_l, grid_c, grid_l;
};

static GicpLaunch gicp_choose_launch(int n_pairs, int64_t max_n) {
  GicpLaunch L;
  L.n_pairs = n_pairs;
  L.cap_c = (int)std::max<int64_t>(1, std::min<int64_t>((max_n * 8 + kBlock - 1) / kBlock, 4096));
  L.cap_l = (int)std::max<int64_t>(1, std::min<int64_t>((max_n + kBlock - 1) / kBlock, 512));
  L.grid_c = (int)std::max<int64_t>(n_pairs, std::min<int64_t>((int64_t)n_pairs * L.cap_c, 8192));
  L.grid_l = (int)std::max<int64_t>(n_pairs, std::min<int64_t>((int64_t)n_pairs * L.cap_l, 2048));
  return L;
}

// One round of a batch: correspond (FAST_GICP), linearize, and the solve launch unless the rounds are fused.  per_pair: the targets come
// from the handle's GicpTarget table (gicp_align_pairs) instead of the handle's target; such a batch is FAST_GICP whatever the method.
template <bool FUSED, bool FIXED>
static void gicp_launch_round_as(dgs_handle* h, const GicpLaunch& L, const int launch, const bool per_pair) {
  const bool vgicp = !per_pair && h->prm.method == DGS_METHOD_VGICP;
  if (!vgicp) {
    const int slot = prof_begin(h, DGS_K_NN_SEARCH);
    if (per_pair)
      hipLaunchKernelGGL(gicp_correspond_kernel<GicpTargetTable>, dim3(L.grid_c), dim3(kBlock), 0, h->stream, GicpTargetTable{h->gtargets.ptr}, h->gitems.ptr,
                         h->gpairs.ptr, L.n_pairs, L.cap_c, h->gconsts.max_corr_sq);
    else
      hipLaunchKernelGGL(gicp_correspond_kernel<GicpBatchIndex>, dim3(L.grid_c), dim3(kBlock), 0, h->stream, GicpBatchIndex{make_bvh_view(h->tgt->bvh)}, h->gitems.ptr,
                         h->gpairs.ptr, L.n_pairs, L.cap_c, h->gconsts.max_corr_sq);
    prof_end(h, DGS_K_NN_SEARCH, slot);
  }
  const int slot = prof_begin(h, DGS_K_GICP_LINEARIZE);
  const auto linearize = [&](auto kernel, const auto target) {
    hipLaunchKernelGGL(kernel, dim3(L.grid_l), dim3(kBlock), 0, h->stream, target, h->gitems.ptr, h->gpairs.ptr, h->partials.ptr, L.n_pairs, L.cap_l,
                       h->pair_blocks.ptr, h->gconsts, h->done_counter.ptr, launch);
  };
  if (vgicp)
    linearize(vgicp_linearize_kernel<FUSED, FIXED>, h->vmap);
  else if (per_pair)
    linearize(gicp_linearize_kernel<FUSED, FIXED, GicpTargetTable>, GicpTargetTable{h->gtargets.ptr});
  else
    linearize(gicp_linearize_kernel<FUSED, FIXED, GicpBatchCloud>, GicpBatchCloud{h->tgt->pts.ptr, h->tgt->cov.ptr});
  prof_end(h, DGS_K_GICP_LINEARIZE, slot);
  if (!FUSED)
    hipLaunchKernelGGL(gicp_solve_kernel, dim3(L.n_pairs), dim3(kBlock), 0, h->stream, h->gpairs.ptr, h->partials.ptr, h->pair_blocks.ptr, L.cap_l,
                       h->gconsts, h->done_counter.ptr);
}

// fused rounds (default; DGS_GICP_FUSED=0 restores the separate solve launch): the optimiser step of a pair runs in the last
// workgroup of its linearize slice -- two dependent launches per evaluation instead of three (VGICP: one instead of two).
// batch_independent: slices that follow the pair's own size (the FIXED kernels).
static void gicp_launch_round(dgs_handle* h, const GicpLaunch& L, const int launch, const bool per_pair) {
  switch ((h->gicp_fused ? 2 : 0) | (h->batch_independent ? 1 : 0)) {
    case 3: gicp_launch_round_as<true, true>(h, L, launch, per_pair); break;
    case 2: gicp_launch_round_as<true, false>(h, L, launch, per_pair); break;
    case 1: gicp_launch_round_as<false, true>(h, L, launch, per_pair); break;
    default: gicp_launch_round_as<false, false>(h, L, launch, per_pair); break;
  }
}

using GicpStaging = BatchStaging<GicpInit, GicpItem, GicpPair>;

// Covariances and indices of every cloud, work arrays, per-pair state: everything a batch needs before its first round.
// tgt_of (gicp_align_pairs): pair i's entry of the target table, < 0 for a pair without a target (it never becomes active); the caller has
// seen to the targets' covariances.  nullptr: every pair registers against the handle's target.
static int gicp_start(dgs_handle* h, int n, CloudState* const* srcs, const double* x0_rows, int probe_kind, GicpLaunch* L_out, int* n_live,
                      const int* tgt_of = nullptr) {
  hipStream_t st = h->stream;
  fill_gconsts(h);
  int rc = tgt_of ? DGS_OK : ensure_covariance(h, *h->tgt);
  if (rc) return rc;
  const bool vgicp = !tgt_of && h->prm.method == DGS_METHOD_VGICP;
  if (vgicp && !h->vmap_valid) {
    rc = vgicp_build_map(h);
    if (rc) return rc;
  }
  const int64_t per_point = vgicp ? h->vmap.n_offsets : 1;  // correspondences per source point
  int64_t total = 0, max_n = 1;
  *n_live = 0;
  std::vector<CloudState*> live;
  for (int i = 0; i < n; i++) {
    if (srcs[i]->n <= 0 || (tgt_of && tgt_of[i] < 0)) continue;
    live.push_back(srcs[i]);
    total += srcs[i]->n;
    max_n = std::max<int64_t>(max_n, srcs[i]->n);
    (*n_live)++;
  }
  // the sources' covariances: one batched pass (cov_batch.hip), a lone source on the single pass; gicp_align_pairs has made them with its targets'
  if (!tgt_of) {
    rc = live.size() == 1 ? ensure_covariance(h, *live[0]) : ensure_covariances(h, (int)live.size(), live.data(), covplan::kFast);
    if (rc) return rc;
  }
  const GicpLaunch L = gicp_choose_launch(n, max_n);
  *L_out = L;
  DGS_HIP_TRY(h, h->corr.reserve((size_t)std::max<int64_t>(total, 1) * per_point));
  DGS_HIP_TRY(h, h->corr_sq.reserve((size_t)std::max<int64_t>(total, 1)));
  DGS_HIP_TRY(h, h->mahal.reserve((size_t)std::max<int64_t>(total, 1) * per_point * 6));
  DGS_HIP_TRY(h, h->gpairs.reserve(n));
  DGS_HIP_TRY(h, h->gitems.reserve(n));
  DGS_HIP_TRY(h, h->inits.reserve(n));  // sizeof(NdtInit) >= sizeof(GicpInit)
  static_assert(sizeof(NdtInit) >= sizeof(GicpInit), "init staging buffer is shared with NDT");
  DGS_HIP_TRY(h, h->pair_blocks.reserve(n));
  DGS_HIP_TRY(h, h->done_counter.reserve(16));
  DGS_HIP_TRY(h, h->partials.reserve((size_t)n * L.cap_l * kAccumPad + 64));
  const GicpStaging stg(h, n);
  if (stg.ensure() != DGS_OK) return DGS_ERR_HIP;
  GicpInit* hin = stg.inits();
  GicpItem* hit = stg.items();
  int64_t off = 0;
  for (int i = 0; i < n; i++) {
    const CloudState& c = *srcs[i];
    for (int k = 0; k < 12; k++) hin[i].x0[k] = x0_rows[12 * i + k];
    hin[i].probe_kind = probe_kind;
    // a pair without a target is dead: the sizing loop above left its source out of `total`, so it gets a zero-length slot here
    const int64_t live_n = (tgt_of && tgt_of[i] < 0) ? 0 : c.n;
    hin[i].n = (int)live_n;
    hit[i].src = c.pts.ptr;
    hit[i].src_sorted = c.bvh.sorted.ptr;
    hit[i].cov_s = c.cov.ptr;
    hit[i].corr = h->corr.ptr + off * per_point;
    hit[i].corr_sq = h->corr_sq.ptr + off;
    hit[i].mahal = h->mahal.ptr + off * per_point * 6;
    hit[i].n = (int)live_n;
    hit[i].tgt = tgt_of ? std::max(tgt_of[i], 0) : 0;
    off += live_n;
  }
  DGS_HIP_TRY(h, hipMemcpyAsync(h->inits.ptr, hin, (size_t)n * sizeof(GicpInit), hipMemcpyHostToDevice, st));
  DGS_HIP_TRY(h, hipMemcpyAsync(h->gitems.ptr, hit, (size_t)n * sizeof(GicpItem), hipMemcpyHostToDevice, st));
  DGS_HIP_TRY(h, hipMemsetAsync(h->done_counter.ptr, 0, 16 * sizeof(int), st));
  DGS_HIP_TRY(h, hipMemsetAsync(h->pair_blocks.ptr, 0, (size_t)n * sizeof(int), st));
  hipLaunchKernelGGL(gicp_init_kernel, dim3((n + 63) / 64), dim3(64), 0, st, h->gpairs.ptr, reinterpret_cast<const GicpInit*>(h->inits.ptr), n);
  return DGS_OK;
}

// FastGICP::align for every source of a batch against the handle's target; the LM loops of all pairs advance together,
// one (correspond, linearize, solve) launch triple per round, and pairs that finish hand their workgroups to the rest.
static std::vector<double> gicp_guess_rows(int n, const float* guesses16) {
  std::vector<double> x0((size_t)n * 12);
  for (int i = 0; i < n; i++) {
    const float* G = guesses16 ? guesses16 + 16 * i : kIdentity16;
    for (int r = 0; r < 3; r++)
      for (int c = 0; c < 4; c++) x0[(size_t)i * 12 + r * 4 + c] = (double)G[c * 4 + r];  // Eigen::Isometry3d(guess.cast<double>())
  }
  return x0;
}

// whole chunks of 4 rounds: the bound rounded up
static long gicp_max_rounds(const dgs_handle* h) { return ((long)h->prm.maximum_iterations * (h->prm.gicp_lm_max_iterations + 1) + 4 + 3) / 4 * 4; }

static int gicp_read_results(dgs_handle* h, int n, CloudState* const* srcs, dgs_result* out);

int gicp_align_batch(dgs_handle* h, int n, CloudState* const* srcs, const float* guesses16, dgs_result* out) {
  const std::vector<double> x0 = gicp_guess_rows(n, guesses16);
  GicpLaunch L;
  int n_live = 0;
  int rc = gicp_start(h, n, srcs, x0.data(), -1, &L, &n_live);
  if (rc) return rc;

  if (n_live > 0) {
    int launch_no = 0;
    rc = run_rounds_polled(h, n_live, gicp_max_rounds(h), 4, [&] { gicp_launch_round(h, L, launch_no++, false); });
    if (rc != DGS_OK) return rc;
  }
  return gicp_read_results(h, n, srcs, out);
}

// the pair states of the batch that has just run -> results
static int gicp_read_results(dgs_handle* h, int n, CloudState* const* srcs, dgs_result* out) {
  const GicpStaging stg(h, n);
  int rc = stg.read_back(h->gpairs, n, "GICP optimiser state");
  if (rc) return rc;
  const GicpPair* hp = stg.pairs();
  long evals = 0;
  for (int i = 0; i < n; i++) {
    std::memcpy(out[i].final_transformation, hp[i].final_T, sizeof(float) * 16);
    const bool empty = srcs[i]->n <= 0;
    out[i].converged = (!empty && hp[i].s.phase == GP_DONE) ? hp[i].s.converged : 0;
    out[i].iterations = hp[i].s.iteration;
    out[i].evaluations = hp[i].s.evaluations;
    out[i].status = empty ? DGS_ERR_NO_SOURCE : DGS_OK;
    out[i].score = hp[i].s.y0;
    out[i].fitness = NAN;
    evals += hp[i].s.evaluations;
  }
  h->last_evaluations = evals;
  return DGS_OK;
}

// ---- per-pair targets: pair i = (tgts[i], srcs[i], guess i), all LM loops advancing together in the same rounds (the kernels take
// their targets from GicpTargetTable).  The handle's own target, source and last result are not touched.  A pair whose target or source is empty never
// becomes active: its status is the caller's business (dgs_align_pairs_clouds).
int gicp_align_pairs(dgs_handle* h, int n, dgs_cloud* const* tgts, dgs_cloud* const* srcs, const float* guesses16, dgs_result* out) {
  // the distinct non-empty targets, by pointer, in order of first appearance; tgt_of[i] < 0: pair i has no target
  std::vector<dgs_cloud*> uniq;
  std::vector<int> tgt_of((size_t)n);
  for (int i = 0; i < n; i++) {
    tgt_of[i] = -1;
    if (tgts[i]->st.n <= 0) continue;
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
  // (k, regularisation): shared with every other path that uses the cloud
  std::vector<CloudState*> cs((size_t)n), need;
  for (dgs_cloud* c : uniq) need.push_back(&c->st);
  for (int i = 0; i < n; i++) {
    cs[i] = &srcs[i]->st;
    if (tgt_of[i] >= 0 && cs[i]->n > 0) need.push_back(cs[i]);
  }
  rc = ensure_covariances(h, (int)need.size(), need.data(), covplan::kFast);
  h->cb.counts8[7] = build.built;
  if (rc) return rc;
  const std::vector<double> x0 = gicp_guess_rows(n, guesses16);
  // the target table travels from the pinned block, behind the batch's own staging (gicp_start sizes the block for that alone)
  const size_t tab_off = (GicpStaging(h, n).bytes + 63) & ~(size_t)63, tab_bytes = std::max<size_t>(uniq.size(), 1) * sizeof(GicpTarget);
  if (ensure_pinned(h, tab_off + tab_bytes) != DGS_OK) return DGS_ERR_HIP;
  GicpLaunch L;
  int n_live = 0;
  rc = gicp_start(h, n, cs.data(), x0.data(), -1, &L, &n_live, tgt_of.data());
  if (rc) return rc;
  if (n_live > 0) {
    DGS_HIP_TRY(h, h->gtargets.reserve(uniq.size()));
    GicpTarget* tab = reinterpret_cast<GicpTarget*>(reinterpret_cast<char*>(h->pinned) + tab_off);
    for (size_t t = 0; t < uniq.size(); t++) {
      const CloudState& c = uniq[t]->st;
      tab[t] = GicpTarget{make_bvh_view(c.bvh), c.pts.ptr, c.cov.ptr, (int)c.n, 0};
    }
    DGS_HIP_TRY(h, hipMemcpyAsync(h->gtargets.ptr, tab, uniq.size() * sizeof(GicpTarget), hipMemcpyHostToDevice, h->stream));
    int launch_no = 0;
    rc = run_rounds_polled(h, n_live, gicp_max_rounds(h), 4, [&] { gicp_launch_round(h, L, launch_no++, true); });
    if (rc != DGS_OK) return rc;
  }
  const int64_t own_evaluations = h->last_evaluations;   // dgs_get_counts keeps reporting the handle's own last align / batch
  rc = gicp_read_results(h, n, cs.data(), out);
  h->last_evaluations = own_evaluations;
  return rc;
}

int gicp_align(dgs_handle* h, const float* guess16, dgs_result* out) {
  CloudState* one[1] = {h->src};
  return gicp_align_batch(h, 1, one, guess16, out);
}

// device pointer and stride of the batch's final transforms (column-major float[16] per pair) for the fitness kernel
const float* gicp_final_transforms(dgs_handle* h, size_t* stride_bytes) {
  *stride_bytes = sizeof(GicpPair);
  return reinterpret_cast<const float*>(reinterpret_cast<const char*>(h->gpairs.ptr) + offsetof(GicpPair, final_T));
}


// Test hook: one linearize (error_only = 0: fresh correspondences at T) or compute_error (1: stored correspondences).
int gicp_probe(dgs_handle* h, const double* T16, int error_only, double* err, double* H36, double* b6) {
  GicpLaunch L;
  int n_live = 0;
  CloudState* one[1] = {h->src};
  int rc = gicp_start(h, 1, one, T16, error_only ? 1 : 0, &L, &n_live);
  if (rc) return rc;
  if (n_live == 0) return DGS_ERR_NO_SOURCE;
  gicp_launch_round(h, L, 0, false);
  const GicpStaging stg(h, 1);
  rc = stg.read_back(h->gpairs, 1, "GICP optimiser state");
  if (rc) return rc;
  const GicpPair* hp = stg.pairs();
  *err = error_only ? hp->s.yi : hp->s.y0;
  if (!error_only) {
    for (int k = 0; k < 36; k++) H36[k] = hp->s.H[k];
    for (int k = 0; k < 6; k++) b6[k] = hp->s.b[k];
  }
  return DGS_OK;
}

}  // namespace dgs
