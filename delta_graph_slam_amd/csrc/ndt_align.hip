// K2 ndt_derivatives + K3 ndt_solve: the NDT align() loop on the device.  This file is the host driver, init / export and the test
// hooks; the kernels are templates launched from here, so they are headers of this one translation unit, one role each:
//   ndt_fast.h        the default order's derivative kernel          ndt_optimiser.h   More-Thuente, Newton step, ndt_advance, the solve kernel
//   ndt_strict.h      the upstream order, fused (ndt_strict_order 1)   ndt_sequential.h  the upstream order summed in index order (ndt_strict_order 2)
//   ndt_queue.h       the persistent queue kernel (experiments build)  ndt_plan.h        the launch plan of an align (host, pure)
//
// Replaces pclomp::NormalDistributionsTransform::computeTransformation, i.e. what
// registration->align(*aligned, guess) runs at apps/scan_matching_odometry_nodelet.cpp:218 and
// include/hdl_graph_slam/loop_detector.hpp:145 of the reference (object configured at
// src/hdl_graph_slam/registrations.cpp:105-119).  Algorithm: SURVEY.md App. A.
//
// MI355X design
//   * One launch of ndt_derivatives covers EVERY still-active pair of a batch and every source point (its ~1024
//     workgroups are re-dealt to the active pairs at each launch, on the device):
//     coalesced 16-B loads of XYZ1 points, 7 (1/27) dependent 4-B cell lookups, 48-B voxel records from L2,
//     float per-point math, double accumulation, wave shuffle -> LDS -> one 28-double partial row per block.
//     No atomics: the rows are summed in a fixed order by ndt_solve, so results are bit-reproducible.
//   * Per point the 7 voxels are folded first into b = sum w C q and N = sum w C - sum w d2 (Cq)(Cq)^T and then
//     projected once through the point Jacobian:  g = J^T b,  H = J^T N J + b . d2T/dp2  -- algebraically
//     the upstream per-voxel update (eq. 6.12/6.13) at ~1/3 of the flops.
//   * ndt_solve (one workgroup per pair) finishes the reduction and runs Newton + the More-Thuente state
//     machine on lane 0, then writes the next evaluation's float transform and angle tables in place, so an
//     iteration is two dependent launches and NO host round trip; finished pairs turn their blocks into
//     immediate returns.  The host only polls a "pairs done" counter once per chunk of iterations.
#include <cfloat>
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "handle.h"
#include "ndt_plan.h"
#include "solve6.h"

namespace dgs {

#include "ndt_fast.h"   // the default order's derivative kernel: the only code here compiled with contraction allowed

// Everything below this line -- the validation-mode evaluation, the optimiser (Newton step, More-Thuente state machine,
// transform / angle tables of the next evaluation) and the host code -- is compiled with floating-point contraction OFF: each
// operation is rounded on its own, as in a CPU build of upstream without FMA, so the optimiser's double arithmetic follows the
// CPU checker operation for operation.  Only the default derivative kernel above lets the compiler fuse multiply-adds.
#pragma clang fp contract(off)

#include "ndt_exp_tables.h"
#include "ndt_optimiser.h"   // write_evaluation ... ndt_advance, ndt_close_evaluation, ndt_solve_kernel
#include "ndt_strict.h"      // ndt_strict_order 1: the upstream-order evaluation as a fused launch (uses ndt_advance)
#include "ndt_sequential.h"  // ndt_strict_order 2

// ================================================================================================ queue layout
// Shared by the init kernel, the host driver (DGS_NDT_SCHEDULE cuts the rounds like the queue would) and the queue kernel itself (ndt_queue.h).
__host__ __device__ inline int ndt_queue_slices(int round, int base, int cap) {
  const int f = round < 12 ? 1 : (round < 24 ? 2 : 4);
  return min(base * f, cap);
}
constexpr int kQueueHdrWords = 82;                    // NdtPair: T[12], jang[8][3], hang[15][3], need_hessian
static_assert(offsetof(NdtPair, need_hessian) == 81 * 4, "header layout");
// What a round's derivative pass reads of the pair's record (transform, angle tables, need_hessian: the first 82 words of NdtPair) has
// ONE SLOT PER ROUND, each in its own 128-byte lines: the closing workgroup of round r writes slot r + 1 through to memory before it
// publishes round r + 1, and no cache of any XCD can hold an older copy of an address that nobody has read in this launch yet -- so the
// workers read a slot with ordinary scalar loads, exactly like the launch-per-evaluation kernel reads the record after a kernel
// boundary (keeping the 81 table entries in scalar registers read back through v_readlane cost 58 more instructions per point).
constexpr size_t kQueueSlotBytes = 384;
__host__ __device__ inline NdtPair* queue_slot(char* ring, int ring_rounds, int pair, int round) {
  return reinterpret_cast<NdtPair*>(ring + ((size_t)pair * ring_rounds + round) * kQueueSlotBytes);
}
// Queue memory: 64-bit words, contiguous -- word 0 = control ([31:0] pairs still iterating, bit 32 abort), word 1 + p = pair p.  A worker
// looking for work reads control and up to 63 pairs with ONE wave-wide load of four 128-byte lines (one line per pair made every
// idle poll 34 line requests to the same memory channel: measured 110 polls per us by 768 workers, items three times slower).
__device__ __forceinline__ unsigned long long* queue_word(int* queue, int pair) { return reinterpret_cast<unsigned long long*>(queue) + 1 + pair; }
__device__ __forceinline__ unsigned long long* queue_ctl(int* queue) { return reinterpret_cast<unsigned long long*>(queue); }
constexpr int kQueueStatInts = 16;   // diagnostic build: counters behind the words

// ================================================================================================ init / export
__global__ void ndt_init_kernel(NdtPair* __restrict__ pairs, const NdtInit* __restrict__ inits, int n_pairs, const NdtConsts c, int probe,
                                int* __restrict__ done_counter, const float4* const* __restrict__ stage_ptrs, const int* __restrict__ stage_sizes,
                                const float4** __restrict__ src_ptrs, int* __restrict__ src_sizes, int* __restrict__ queue, const int queue_slices0,
                                char* __restrict__ ring, const int ring_rounds) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < 16) done_counter[i] = 0;   // the first block has 64 threads: the counter block is cleared here, not by a fill command
  if (queue && i == 0) *queue_ctl(queue) = (unsigned long long)n_pairs;   // queue kernel: pairs still iterating, abort bit clear
  if (queue && i < kQueueStatInts) queue[2 * (n_pairs + 2) + i] = 0;
  if (i >= n_pairs) return;
  if (queue) *queue_word(queue, i) = (unsigned long long)queue_slices0 << 32;   // round 0, nothing claimed
  src_ptrs[i] = stage_ptrs[i];
  src_sizes[i] = stage_sizes[i];
  NdtPair* st = pairs + i;
  const NdtInit& in = inits[i];
  NdtSolver s;
  s.phase = probe ? PH_PROBE : PH_INIT_EVAL;
  s.nr_iterations = 0;
  s.trial_n = 0;
  s.trial_next = 0;
  s.trial_hits = 0;
  s.trial_pad = 0;
  s.evaluations = 0;
  s.converged = 0;
  s.step_iterations = 0;
  s.interval_converged = 0;
  s.open_interval = 1;
  s.traj_len = 1;
  s.score = 0;
  s.phi_0 = s.d_phi_0 = s.a_t = s.a_l = s.f_l = s.g_l = s.a_u = s.f_u = s.g_u = s.step_init = 0;
  for (int k = 0; k < 6; k++) { s.p[k] = in.p0[k]; s.grad[k] = 0; s.dir[k] = 0; st->traj[0][k] = in.p0[k]; }
  for (int k = 0; k < 36; k++) s.hess[k] = 0;
  double x[6];
  for (int k = 0; k < 6; k++) x[k] = in.p0[k];
  write_evaluation<false>(st, st, s, c, x, probe == 2 ? 2 : (probe == 3 ? 0 : 1), false, true);   // probe 2: the test hook of the double-precision computeHessian pass; 3: a score + gradient evaluation (PCL_NDT_HIP)
  // the first evaluation transforms the cloud by the GUESS matrix itself (computeTransformation)
  const float* G = in.guess;
  st->T[0] = G[0]; st->T[1] = G[4]; st->T[2] = G[8];  st->T[3] = G[12];
  st->T[4] = G[1]; st->T[5] = G[5]; st->T[6] = G[9];  st->T[7] = G[13];
  st->T[8] = G[2]; st->T[9] = G[6]; st->T[10] = G[10]; st->T[11] = G[14];
  for (int k = 0; k < 16; k++) st->final_T[k] = G[k];
  st->s = s;
  st->active = 1;
  st->last_launch = 0x7FFFFFFF;
  st->ticket = 0;
  st->serve[0] = 0;    // upstream order, fused: the first evaluation (kind 1) is served by round 0's first kernel
  st->serve[1] = -1;
  st->serve[2] = -1;
  st->serve[3] = st->need_hessian & 3;   // round 0's kind (NdtPair::serve)
  st->spec_pending = 0;
  st->spec_result = 0;
  if (queue) {   // queue kernel: the record slot of round 0
    const int* from = reinterpret_cast<const int*>(st);
    int* to = reinterpret_cast<int*>(queue_slot(ring, ring_rounds, i, 0));
    for (int k = 0; k < kQueueHdrWords; k++) to[k] = from[k];
  }
}

struct NdtOut {
  float T[16];
  int converged, iterations, evaluations, reused;   // evaluations: upstream's count; reused: those of them answered from the trial cache (NdtSolver::trial_hits)
  double score;
};

__global__ void ndt_export_kernel(const NdtPair* __restrict__ pairs, int n_pairs, NdtOut* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_pairs) return;
  const NdtPair& st = pairs[i];
  NdtOut o;
  for (int k = 0; k < 16; k++) o.T[k] = st.final_T[k];
  o.converged = (st.s.phase == PH_DONE) ? st.s.converged : 0;
  o.iterations = st.s.nr_iterations;
  o.evaluations = st.s.evaluations;
  o.reused = st.s.trial_hits;
  o.score = st.s.score;
  out[i] = o;
}

// ================================================================================================ host side
// Eigen 3.3 Matrix3f::eulerAngles(0,1,2) on the rotation block of a column-major float 4x4
// (computeTransformation: "convert initial guess matrix to 6 element transformation vector").
static void euler_angles_012(const float* T, float res[3]) {
  auto m = [&](int r, int c) { return T[c * 4 + r]; };
  const float kPi = 3.14159265358979323846f;
  res[0] = std::atan2(m(1, 2), m(2, 2));
  const float c2 = std::sqrt(m(0, 0) * m(0, 0) + m(0, 1) * m(0, 1));
  if (res[0] > 0.0f) {
    res[0] -= kPi;
    res[1] = std::atan2(-m(0, 2), -c2);
  } else {
    res[1] = std::atan2(-m(0, 2), c2);
  }
  const float s1 = std::sin(res[0]), c1 = std::cos(res[0]);
  res[2] = std::atan2(s1 * m(2, 0) - c1 * m(1, 0), c1 * m(1, 1) - s1 * m(2, 1));
  res[0] = -res[0];
  res[1] = -res[1];
  res[2] = -res[2];
}

// Eigen::Transform<float, 3, Affine>::rotation() of the guess (dgs_params.ndt_guess_rotation_polar): computeRotationScaling, i.e. a
// 3 x 3 float JacobiSVD (Eigen 3.3's two-sided Jacobi: the sequence of solve6.h's jsvd, here in float on the host, once per align),
// x = det(U V^T), U.col(0) /= x, R = U V^T.  Every operation individually rounded (contraction is off in this part of the file).
// [UPSTREAM-RECALL: Eigen/src/Geometry/Transform.h, Eigen/src/SVD/JacobiSVD.h; the CPU checker carries its own statement.]  R: row-major.
static void affine_rotation_f32(const float* T_colmajor16, float* R) {
  constexpr int N = 3;
  const float precision = 2.f * FLT_EPSILON, tiny = FLT_MIN;
  float W[9], U[9], V[9];
  float scale = 0.f;
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 3; c++) { W[r * 3 + c] = T_colmajor16[c * 4 + r]; scale = std::fabs(W[r * 3 + c]) > scale ? std::fabs(W[r * 3 + c]) : scale; }
  if (scale == 0.f) scale = 1.f;
  for (int i = 0; i < 9; i++) { W[i] = W[i] / scale; U[i] = V[i] = (i % 4 == 0) ? 1.f : 0.f; }
  float max_diag = 0.f;
  for (int i = 0; i < N; i++) { const float a = std::fabs(W[i * 4]); if (a > max_diag) max_diag = a; }
  bool finished = false;
  for (int sweep = 0; sweep < 64 && !finished; sweep++) {
    finished = true;
    for (int p = 1; p < N; p++)
      for (int q = 0; q < p; q++) {
        const float pm = precision * max_diag;
        const float threshold = tiny > pm ? tiny : pm;
        if (!(std::fabs(W[p * N + q]) > threshold || std::fabs(W[q * N + p]) > threshold)) continue;
        finished = false;
        float m00 = W[p * N + p], m01 = W[p * N + q], m10 = W[q * N + p], m11 = W[q * N + q];
        const float t = m00 + m11, d = m10 - m01;
        float r1c, r1s;
        if (std::fabs(d) < tiny) { r1s = 0.f; r1c = 1.f; }
        else {
          const float u = t / d;
          const float tmp = std::sqrt(1.f + u * u);
          r1s = 1.f / tmp;
          r1c = u / tmp;
        }
        if (!(r1c == 1.f && r1s == 0.f)) {
          const float x0 = m00, y0 = m10, x1 = m01, y1 = m11;
          m00 = r1c * x0 + r1s * y0; m10 = -r1s * x0 + r1c * y0;
          m01 = r1c * x1 + r1s * y1; m11 = -r1s * x1 + r1c * y1;
        }
        float jrc, jrs;
        {
          const float deno = 2.f * std::fabs(m01);
          if (deno < tiny) { jrc = 1.f; jrs = 0.f; }
          else {
            const float tau = (m00 - m11) / deno;
            const float w = std::sqrt(tau * tau + 1.f);
            const float tt = (tau > 0.f) ? 1.f / (tau + w) : 1.f / (tau - w);
            const float sign_t = tt > 0.f ? 1.f : -1.f;
            const float nn = 1.f / std::sqrt(tt * tt + 1.f);
            jrs = -sign_t * (m01 / std::fabs(m01)) * std::fabs(tt) * nn;
            jrc = nn;
          }
        }
        const float jtc = jrc, jts = -jrs;
        const float jlc = r1c * jtc - r1s * jts;
        const float jls = r1c * jts + r1s * jtc;
        if (!(jlc == 1.f && jls == 0.f)) {
          for (int i = 0; i < N; i++) {
            const float xi = W[p * N + i], yi = W[q * N + i];
            W[p * N + i] = jlc * xi + jls * yi;
            W[q * N + i] = -jls * xi + jlc * yi;
          }
          for (int i = 0; i < N; i++) {
            const float xi = U[i * N + p], yi = U[i * N + q];
            U[i * N + p] = jlc * xi + jls * yi;
            U[i * N + q] = -jls * xi + jlc * yi;
          }
        }
        if (!(jrc == 1.f && -jrs == 0.f)) {
          const float c = jrc, s = -jrs;
          for (int i = 0; i < N; i++) {
            const float xi = W[i * N + p], yi = W[i * N + q];
            W[i * N + p] = c * xi + s * yi;
            W[i * N + q] = -s * xi + c * yi;
          }
          for (int i = 0; i < N; i++) {
            const float xi = V[i * N + p], yi = V[i * N + q];
            V[i * N + p] = c * xi + s * yi;
            V[i * N + q] = -s * xi + c * yi;
          }
        }
        const float app = std::fabs(W[p * N + p]), aqq = std::fabs(W[q * N + q]);
        const float mx = app < aqq ? aqq : app;
        if (max_diag < mx) max_diag = mx;
      }
  }
  float sv[3];
  for (int i = 0; i < N; i++) {
    const float a = W[i * 4];
    sv[i] = std::fabs(a) * scale;
    if (a < 0.f) for (int k = 0; k < N; k++) U[k * N + i] = -U[k * N + i];
  }
  for (int i = 0; i < N; i++) {   // descending order: first maximum of the tail, column swaps
    int pos = 0;
    float best = sv[i];
    for (int k = 1; k < N - i; k++) if (sv[i + k] > best) { best = sv[i + k]; pos = k; }
    if (best == 0.f) break;
    if (pos) {
      pos += i;
      std::swap(sv[i], sv[pos]);
      for (int k = 0; k < N; k++) { std::swap(U[k * N + i], U[k * N + pos]); std::swap(V[k * N + i], V[k * N + pos]); }
    }
  }
  auto prod = [&](const float* M, int i, int j) { return M[i * 3 + 0] * V[j * 3 + 0] + M[i * 3 + 1] * V[j * 3 + 1] + M[i * 3 + 2] * V[j * 3 + 2]; };
  float UVt[9];
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) UVt[i * 3 + j] = prod(U, i, j);
  auto det3h = [&](int a, int b, int c) { return UVt[0 * 3 + a] * (UVt[1 * 3 + b] * UVt[2 * 3 + c] - UVt[1 * 3 + c] * UVt[2 * 3 + b]); };
  const float x = det3h(0, 1, 2) - det3h(1, 0, 2) + det3h(2, 0, 1);
  for (int k = 0; k < 3; k++) U[k * 3 + 0] /= x;
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) R[i * 3 + j] = prod(U, i, j);
}

static void fill_consts(dgs_handle* h) {
  const dgs_params& p = h->prm;
  const double c1 = 10.0 * (1.0 - p.ndt_outlier_ratio);
  const double c2 = p.ndt_outlier_ratio / std::pow(p.ndt_resolution, 3);
  const double d3 = -std::log(c2);
  NdtConsts& c = h->consts;
  c.gauss_d1 = -std::log(c1 + c2) - d3;
  c.gauss_d2 = -2.0 * std::log((-std::log(c1 * std::exp(-0.5) + c2) - d3) / c.gauss_d1);
  c.step_size = p.ndt_step_size;
  c.trans_eps = p.transformation_epsilon;
  c.max_iterations = p.maximum_iterations;
  c.line_search = p.ndt_line_search;
  c.mt_max_step_iterations = p.ndt_mt_max_step_iterations;
  c.fix_hessian_d1 = p.ndt_fix_hessian_d1;
  c.search_method = p.ndt_search_method;
  c.strict_order = p.ndt_strict_order;
  c.newton_solver = p.ndt_newton_solver;
  c.hessian_double = (p.ndt_strict_order != DGS_NDT_ORDER_FAST && p.ndt_hessian_recompute_double) ? 1 : 0;
  c.exp_libm = p.ndt_exp_glibc ? 1 : 0;
  c.reuse_trials = (DGS_NDT_REUSE_TRIALS != 0 && h->ndt_reuse_trials && p.ndt_strict_order != DGS_NDT_ORDER_FAST) ? 1 : 0;
}

struct NdtLaunch {
  int n_pairs;
  int cap_blocks;    // most slices one pair can get (= rows reserved per pair in `partials`)
  int total_blocks;  // workgroups per derivative launch
  int max_n;         // largest source of the batch (row length of the ndt_strict_order 2 per-point table)
  int queue_workers; // queue kernel: persistent workgroups; 0 = launch-per-evaluation path
  int queue_base;    // queue kernel: slices of a pair's first rounds (ndt_queue_slices)
};

// per-pair stride (doubles) of the ndt_strict_order 2 table: 43 per-point totals, or -- with the double-precision computeHessian pass --
// 36 entries x (point, voxel slot) terms
static size_t strict_rows_pair_stride(const dgs_handle* h, const NdtLaunch& L) {
  size_t s = (size_t)kStrictAccum * L.max_n;
  if (h->consts.hessian_double) {
    const int nb = (h->consts.search_method == DGS_NDT_DIRECT1) ? 1 : (h->consts.search_method == DGS_NDT_DIRECT7 ? 7 : 27);
    s = std::max(s, (size_t)36 * L.max_n * nb);
  }
  return s;
}

// ---- the plan of this align (ndt_plan.h), from the handle as ndt_setup has left it
static NdtPlan plan_align(const dgs_handle* h) {
  NdtPlanIn in;
  in.strict_order = h->consts.strict_order;
  in.search_method = h->consts.search_method;
  in.strict_kernel = h->strict_kernel;
  in.exp_libm = h->consts.exp_libm;
  in.hessian_double = h->consts.hessian_double;
  in.newton_solver = h->consts.newton_solver;
  in.n_occupied_bound = h->n_occupied_bound;
  in.ndt_fused = h->ndt_fused;
  in.hd_overlap = h->hd_overlap;
  in.has_hd_stream = h->hd_stream != nullptr;
  in.ndt_speculate = h->ndt_speculate;
  in.ndt_fixed_slices = h->ndt_fixed_slices;
  in.solve_min_active = h->solve_min_active;
  NdtPlan p = plan_align(in);
  if (is_pcl_ndt(h)) {
    // PCL_NDT_HIP: the upstream order's driver with pcl_ndt.hip's kernel -- one launch per round serves every evaluation kind, the Newton
    // step stays in the pair's closing workgroup and nothing is speculated (a pair's doubles must not depend on its batch)
    p.item_kernel = true;
    p.two_kinds = p.solve_beside = p.speculate = false;
    p.fixed_slices = true;
    p.fused = true;   // (DGS_NDT_FUSED=0 is the other methods' test hook: the stand-alone solve kernel leaves no double angle vectors)
    p.evals_factor = 1;
  }
  return p;
}

static hipStream_t launch_stream(const dgs_handle* h, const NdtPlan& P, int launch, bool hd) { return plan_on_hd_stream(P, launch, hd) ? h->hd_stream : h->stream; }

// ndt_strict_order 2: per-point totals / per-term table to HBM (round 2's kernel), then the sequential sums
template <int SEARCH>
static void launch_strict_rows(dgs_handle* h, const NdtLaunch& L, const dim3 grid, const int leaf_pow2, hipStream_t st) {
  const double gd1 = h->consts.gauss_d1;
  const float gd2 = (float)h->consts.gauss_d2;
  static const bool literal = std::getenv("DGS_NDT_STRICT_LITERAL") && std::atoi(std::getenv("DGS_NDT_STRICT_LITERAL")) != 0;
  const size_t stride = strict_rows_pair_stride(h, L);
  with_bool(literal, [&](auto LIT) {
    hipLaunchKernelGGL((ndt_derivatives_strict_kernel<SEARCH, true, decltype(LIT)::value>), grid, dim3(kBlock), 0, st, h->src_ptrs.ptr, h->src_sizes.ptr, h->pairs.ptr, h->grid,
                       h->vox_dbg.ptr, gd1, gd2, leaf_pow2, h->partials.ptr, h->strict_rows.ptr, L.max_n, L.n_pairs, L.cap_blocks, h->pair_blocks.ptr,
                       h->consts.gauss_d2, stride, h->consts.exp_libm);
  });
  hipLaunchKernelGGL(ndt_strict_seqsum_kernel, dim3(L.n_pairs), dim3(kWave), 0, st, h->pairs.ptr, h->src_sizes.ptr, h->strict_rows.ptr, L.max_n,
                     h->strict_totals.ptr, stride, Offsets<SEARCH>::N);
}

// ndt_strict_order 1 (ndt_strict.h).  FUSED: launch number `launch` >= 0 of this align, derivatives + closing workgroups, a pair's
// "finished" flag in pinned memory; otherwise derivatives only and the device counter.
// The item-compacted kernel, one launch per round for every evaluation kind (NdtPlan::item_kernel; dgs_handle::strict_kernel 3, the default).
// (Measured and dropped: the item-compacted kernel for the float kinds alone -- 64-point tiles, a third of the LDS, meant for three waves
// per SIMD -- with the lane-per-point computeHessian kernel as the round's second launch: the register allocator spilled the double
// accumulators, 47 ms per step.)
// (It carries ONE exponential -- glibc's, the default: with both compiled in it went from 4 to 27 spilled registers; ndt_exp_glibc = 0,
//  the rounds 1-3 polynomial, is served by the lane-per-point kernels.)
#ifdef DGS_DEAL_STAMPS
// Stamp build (make stamps): the item-kernel launches number DGS_DEAL_STAMPS_AT .. + kStampLaunches - 1 of this handle are recorded; the
// launch after them waits for the stream and writes the records to DGS_DEAL_STAMPS_FILE (raw, kStampLaunches x kStampGrid x kStampWords
// 64-bit words).  Returns 1 + the slot of the launch about to be issued, or 0.
static int deal_stamp_slot(dgs_handle* h, hipStream_t st) {
  static const char* file = std::getenv("DGS_DEAL_STAMPS_FILE");
  static const long long at = std::getenv("DGS_DEAL_STAMPS_AT") ? std::atoll(std::getenv("DGS_DEAL_STAMPS_AT")) : 2200;
  if (!file) return 0;
  const size_t words = (size_t)kStampLaunches * kStampGrid * kStampWords;
  const long long seq = h->deal_stamp_seq++;
  if (seq == at) {
    if (hipMalloc(reinterpret_cast<void**>(&h->deal_stamps), words * 8) != hipSuccess) { h->deal_stamps = nullptr; return 0; }
    (void)hipMemsetAsync(h->deal_stamps, 0, words * 8, st);
    (void)hipMemcpyToSymbolAsync(HIP_SYMBOL(g_deal_stamps), &h->deal_stamps, sizeof(h->deal_stamps), 0, hipMemcpyHostToDevice, st);
    (void)hipStreamSynchronize(st);
  }
  if (!h->deal_stamps || seq < at) return 0;
  if (seq < at + kStampLaunches) return (int)(seq - at) + 1;
  if (seq == at + kStampLaunches) {
    (void)hipStreamSynchronize(st);
    std::vector<unsigned long long> host(words);
    if (hipMemcpy(host.data(), h->deal_stamps, words * 8, hipMemcpyDeviceToHost) == hipSuccess) {
      if (FILE* f = std::fopen(file, "wb")) {
        std::fwrite(host.data(), 8, words, f);
        std::fclose(f);
      }
    }
  }
  return 0;
}
#endif

template <int SEARCH, bool FUSED, bool FIXED>
static void launch_strict_items(dgs_handle* h, const NdtPlan& P, const NdtLaunch& L, const dim3 grid, const int leaf_pow2, const int launch, hipStream_t st) {
  const int spec = (FUSED && P.speculate) ? 1 : 0;
  const dim3 grid_s(grid.x + (spec ? L.n_pairs : 0));   // + one solver workgroup per pair, in front (ndt_strict.h)
  int flags = (spec ? kStrictSpeculate : 0) | (h->ndt_deal_by_cost ? kStrictDealByCost : 0);
#ifdef DGS_DEAL_STAMPS
  flags |= deal_stamp_slot(h, st) << kStrictStampShift;
#endif
  hipLaunchKernelGGL((ndt_strict3_kernel<SEARCH, FUSED, true, FIXED>), grid_s, dim3(kBlock), 0, st, h->src_ptrs.ptr, h->src_sizes.ptr, h->pairs.ptr, h->grid, h->vox_strict.ptr,
                     h->vox_dbg.ptr, h->consts.gauss_d1, h->consts.gauss_d2, leaf_pow2, h->partials.ptr, L.n_pairs, L.cap_blocks, h->pair_blocks.ptr, h->consts,
                     FUSED ? h->done_flags : h->done_counter.ptr, launch, (FUSED && P.solve_beside) ? h->solve_min_active : 0, flags);
}

// The lane-per-point kernels, two launches per round.  HD: the instantiation for the pairs waiting for the double-precision
// computeHessian pass (evaluation kind 2); with overlap it runs on the third stream beside the next round's first launch (lag 2).
template <int SEARCH, bool FUSED, bool HD>
static void launch_strict_lanes(dgs_handle* h, const NdtPlan& P, const NdtLaunch& L, const dim3 grid, const int leaf_pow2, const int launch, hipStream_t st) {
  const int hd_lag = (FUSED && P.hd_overlap) ? 2 : 1;
  hipLaunchKernelGGL((ndt_strict_kernel<SEARCH, FUSED, HD>), grid, dim3(kBlock), 0, st, h->src_ptrs.ptr, h->src_sizes.ptr, h->pairs.ptr, h->grid, h->vox_strict.ptr,
                     h->vox_dbg.ptr, h->consts.gauss_d1, h->consts.gauss_d2, leaf_pow2, h->partials.ptr, L.n_pairs, L.cap_blocks, h->pair_blocks.ptr, h->consts,
                     FUSED ? h->done_flags : h->done_counter.ptr, launch, hd_lag);
}

// the default order (ndt_fast.h); PACK: two points per lane on packed FP32 (experiments build, DGS_NDT_PACK2, DIRECT7 only)
template <int SEARCH, bool FUSED, bool PACK>
static void launch_fast(dgs_handle* h, const NdtLaunch& L, const dim3 grid, const int leaf_pow2, const int launch, hipStream_t st) {
  hipLaunchKernelGGL((ndt_derivatives_kernel<SEARCH, FUSED, PACK>), grid, dim3(kBlock), 0, st, h->src_ptrs.ptr, h->src_sizes.ptr, h->pairs.ptr, h->grid, h->consts.gauss_d1,
                     (float)h->consts.gauss_d2, leaf_pow2, h->partials.ptr, L.n_pairs, L.cap_blocks, h->pair_blocks.ptr, h->consts,
                     FUSED ? h->done_flags : h->done_counter.ptr, launch);
}

// The derivative launch of one evaluation.  launch >= 0: fused launch number `launch` of this align (derivatives + closing workgroups);
// < 0: derivatives only.  hd: the launch for the pairs waiting for the double computeHessian pass.
static void launch_derivatives(dgs_handle* h, const NdtPlan& P, const NdtLaunch& L, int launch = -1, bool hd = false) {
  const dim3 grid(L.total_blocks);
  int fe = 0;
  const int leaf_pow2 = (std::frexp(h->grid.leaf, &fe) == 0.5f) ? 1 : 0;
  const hipStream_t st = launch_stream(h, P, launch, hd);
  int slot = prof_begin(h, DGS_K_NDT_DERIVATIVES, st);
  if (is_pcl_ndt(h)) {
    if (!(hd && launch >= 0)) pcl_ndt_launch(h, L.n_pairs, L.cap_blocks, L.total_blocks, launch, st);   // (hd with launch < 0: the test hook asks for the kind it has set up)
    prof_end(h, DGS_K_NDT_DERIVATIVES, slot, st);
    return;
  }
  with_search(P.search, [&](auto S) {
    constexpr int SEARCH = decltype(S)::value;
    if (P.order == DGS_NDT_ORDER_UPSTREAM_SEQUENTIAL) {
      launch_strict_rows<SEARCH>(h, L, grid, leaf_pow2, st);
    } else if (P.order == DGS_NDT_ORDER_UPSTREAM && P.item_kernel) {
      if (hd && launch >= 0) return;   // one kernel serves every kind (launch < 0: the test hook asks for the kind it has set up)
      with_bool(launch >= 0, [&](auto FUSED) {
        with_bool(P.fixed_slices, [&](auto FIXED) { launch_strict_items<SEARCH, decltype(FUSED)::value, decltype(FIXED)::value>(h, P, L, grid, leaf_pow2, launch, st); });
      });
    } else if (P.order == DGS_NDT_ORDER_UPSTREAM) {
      with_bool(launch >= 0, [&](auto FUSED) {
        with_bool(hd, [&](auto HD) { launch_strict_lanes<SEARCH, decltype(FUSED)::value, decltype(HD)::value>(h, P, L, grid, leaf_pow2, launch, st); });
      });
    } else {
      with_bool(launch >= 0, [&](auto FUSED) {
        if constexpr (kExperiments && SEARCH == DGS_NDT_DIRECT7) {
          if (h->ndt_pack2) {
            launch_fast<SEARCH, decltype(FUSED)::value, true>(h, L, grid, leaf_pow2, launch, st);
            return;
          }
        }
        launch_fast<SEARCH, decltype(FUSED)::value, false>(h, L, grid, leaf_pow2, launch, st);
      });
    }
  });
  prof_end(h, DGS_K_NDT_DERIVATIVES, slot, st);
}

static void launch_solve(dgs_handle* h, const NdtPlan& P, const NdtLaunch& L) {
  int slot = prof_begin(h, DGS_K_NDT_SOLVE);
  hipLaunchKernelGGL(ndt_solve_kernel, dim3(L.n_pairs), dim3(kBlock), 0, h->stream, h->pairs.ptr, h->partials.ptr, L.cap_blocks, h->pair_blocks.ptr, h->consts,
                     h->done_counter.ptr, P.order != DGS_NDT_ORDER_FAST ? h->strict_totals.ptr : nullptr, P.order == DGS_NDT_ORDER_UPSTREAM ? 1 : 0);
  prof_end(h, DGS_K_NDT_SOLVE, slot);
}

static NdtLaunch choose_launch(int n_pairs, int max_n) {
  NdtLaunch L;
  L.n_pairs = n_pairs;
  // tuning knobs (sweeps only; the defaults are the measured winners: profiles/r03/launch_shape_sweep.jsonl)
  static const int env_cap = std::getenv("DGS_NDT_CAP") ? std::atoi(std::getenv("DGS_NDT_CAP")) : 1024;
  static const int env_total = std::getenv("DGS_NDT_BLOCKS") ? std::atoi(std::getenv("DGS_NDT_BLOCKS")) : 1024;
  static const int env_ppt = std::getenv("DGS_NDT_PPT") ? std::max(1, std::atoi(std::getenv("DGS_NDT_PPT"))) : 2;
  // Slices (= partial rows) one pair can get: sized by the cloud, >= env_ppt points per thread -- 128 workgroups for a 65,536-point
  // scan as before, 391 for the 200,000-point indoor scan (which a fixed cap of 128 held on half of the 256 CUs), never more rows
  // than the closing workgroup's row sum was laid out for.
  static const int env_min = std::getenv("DGS_NDT_MIN_BLOCKS") ? std::max(1, std::atoi(std::getenv("DGS_NDT_MIN_BLOCKS"))) : 64;
  const int by_points = (max_n + kBlock * env_ppt - 1) / (kBlock * env_ppt);
  const int at_least = std::min(env_min, (max_n + kBlock - 1) / kBlock);   // small clouds: 64 workgroups while every thread still has a point (16,384 points: 13.3 against 15.1 us per evaluation)
  L.cap_blocks = std::max(1, std::min({std::max(by_points, at_least), env_cap, kMaxPartialBlocks}));
  L.total_blocks = (int)std::max<int64_t>(n_pairs, std::min<int64_t>((int64_t)n_pairs * L.cap_blocks, env_total));  // ~4 workgroups per CU
  L.max_n = std::max(max_n, 1);
  L.queue_workers = 0;
  L.queue_base = 0;
  return L;
}

// Shape of the persistent queue kernel for this batch: workers (3 workgroups per CU by default: the fourth slot of every CU stays free
// for the side stream's index build), and the slices of a pair's first rounds.
static void choose_queue(dgs_handle* h, NdtLaunch& L) {
  static const int env_workers = std::getenv("DGS_NDT_QUEUE_WORKERS") ? std::atoi(std::getenv("DGS_NDT_QUEUE_WORKERS")) : 768;
  static const int env_base = std::getenv("DGS_NDT_QUEUE_BASE") ? std::atoi(std::getenv("DGS_NDT_QUEUE_BASE")) : 0;
  const int64_t most = (int64_t)L.n_pairs * L.cap_blocks;
  L.queue_workers = (int)std::max<int64_t>(1, std::min<int64_t>(env_workers, most));
  L.queue_base = env_base > 0 ? std::min(env_base, L.cap_blocks) : std::max(1, std::min(L.cap_blocks, L.queue_workers / std::max(1, L.n_pairs)));
  (void)h;
}

// Uploads pointers / sizes / initial poses, runs init, returns the launch shape.
static int ndt_setup(dgs_handle* h, int n_pairs, const float4* const* src_ptrs_host, const int* sizes_host, const float* guesses16,
                     const double* probe_p6, NdtLaunch* launch_out, bool use_queue = false, int probe_kind = 1) {
  hipStream_t st = h->stream;
  fill_consts(h);
  int max_n = 0;
  for (int i = 0; i < n_pairs; i++) max_n = std::max(max_n, sizes_host[i]);
  NdtLaunch L = choose_launch(n_pairs, max_n);
  if (use_queue) {
    choose_queue(h, L);
    DGS_HIP_TRY(h, h->ndt_queue.reserve(2 * ((size_t)n_pairs + 2) + kQueueStatInts));
    // one record slot per pair and round; a registration ends within (max_iterations + 2) x (line-search trials + 2) evaluations
    const int per_iter_q = (h->prm.ndt_line_search == DGS_NDT_LS_FIXED_STEP && h->prm.ndt_step_size - h->prm.transformation_epsilon / 2 > 0) ? 1 : (h->prm.ndt_mt_max_step_iterations + 2);
    h->ndt_ring_rounds = (h->prm.maximum_iterations + 3) * per_iter_q + 8;
    DGS_HIP_TRY(h, h->ndt_ring.reserve((size_t)n_pairs * h->ndt_ring_rounds * kQueueSlotBytes));
  }
  *launch_out = L;
  DGS_HIP_TRY(h, h->pairs.reserve(n_pairs));
  DGS_HIP_TRY(h, h->inits.reserve(n_pairs));
  DGS_HIP_TRY(h, h->src_ptrs.reserve(n_pairs));
  DGS_HIP_TRY(h, h->src_sizes.reserve(n_pairs));
  DGS_HIP_TRY(h, h->partials.reserve((size_t)n_pairs * L.cap_blocks * (h->consts.strict_order ? kStrictPad : kAccumPad)));
  if (h->consts.strict_order) DGS_HIP_TRY(h, h->strict_totals.reserve((size_t)n_pairs * kStrictPad));
  if (h->consts.strict_order == DGS_NDT_ORDER_UPSTREAM_SEQUENTIAL) DGS_HIP_TRY(h, h->strict_rows.reserve((size_t)n_pairs * strict_rows_pair_stride(h, L)));
  DGS_HIP_TRY(h, h->pair_blocks.reserve(n_pairs));
  if (h->consts.strict_order == DGS_NDT_ORDER_UPSTREAM) DGS_HIP_TRY(h, hipMemsetAsync(h->pair_blocks.ptr, 0, sizeof(int) * n_pairs, st));   // "rows present" marks of the unfused upstream order
  DGS_HIP_TRY(h, h->done_counter.reserve(16));
  const size_t off_init = 256;
  const size_t off_ptr = off_init + sizeof(NdtInit) * n_pairs;
  const size_t off_size = off_ptr + sizeof(void*) * n_pairs;
  const size_t off_out = (off_size + sizeof(int) * n_pairs + 255) & ~(size_t)255;
  const size_t total = off_out + sizeof(NdtOut) * n_pairs + sizeof(NdtPair) + 256;
  if (ensure_pinned(h, total) != DGS_OK) return DGS_ERR_HIP;
  char* base = reinterpret_cast<char*>(h->pinned);
  NdtInit* hin = reinterpret_cast<NdtInit*>(base + off_init);
  const float ident[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  for (int i = 0; i < n_pairs; i++) {
    const float* G = guesses16 ? guesses16 + 16 * i : ident;
    std::memcpy(hin[i].guess, G, sizeof(float) * 16);
    if (probe_p6) {
      for (int k = 0; k < 6; k++) hin[i].p0[k] = probe_p6[k];
    } else {
      float e[3];
      if (h->prm.ndt_guess_rotation_polar) {   // eig_transformation.rotation().eulerAngles(0, 1, 2): Affine3f::rotation() is the polar factor
        float R[9], Gp[16];
        affine_rotation_f32(G, R);
        std::memcpy(Gp, G, sizeof(Gp));
        for (int r = 0; r < 3; r++)
          for (int c = 0; c < 3; c++) Gp[c * 4 + r] = R[r * 3 + c];
        euler_angles_012(Gp, e);
      } else {
        euler_angles_012(G, e);
      }
      hin[i].p0[0] = G[12]; hin[i].p0[1] = G[13]; hin[i].p0[2] = G[14];
      hin[i].p0[3] = e[0]; hin[i].p0[4] = e[1]; hin[i].p0[5] = e[2];
    }
  }
  std::memcpy(base + off_ptr, src_ptrs_host, sizeof(void*) * n_pairs);
  std::memcpy(base + off_size, sizes_host, sizeof(int) * n_pairs);
  // ONE copy of (initial poses | source pointers | sizes), contiguous in the pinned block as in the device staging buffer; the init
  // kernel hands the pointers and sizes on to the arrays the other kernels read
  const size_t stage_bytes = off_size + sizeof(int) * n_pairs - off_init;
  DGS_HIP_TRY(h, h->inits.reserve((stage_bytes + sizeof(NdtInit) - 1) / sizeof(NdtInit)));
  DGS_HIP_TRY(h, hipMemcpyAsync(h->inits.ptr, hin, stage_bytes, hipMemcpyHostToDevice, st));
  const char* dstage = reinterpret_cast<const char*>(h->inits.ptr);
  hipLaunchKernelGGL(ndt_init_kernel, dim3((n_pairs + 63) / 64), dim3(64), 0, st, h->pairs.ptr, h->inits.ptr, n_pairs, h->consts, probe_p6 ? probe_kind : 0,
                     h->done_counter.ptr, reinterpret_cast<const float4* const*>(dstage + (off_ptr - off_init)),
                     reinterpret_cast<const int*>(dstage + (off_size - off_init)), h->src_ptrs.ptr, h->src_sizes.ptr,
                     L.queue_workers > 0 ? h->ndt_queue.ptr : nullptr, L.queue_workers > 0 ? ndt_queue_slices(0, L.queue_base, L.cap_blocks) : 0,
                     reinterpret_cast<char*>(h->ndt_ring.ptr), h->ndt_ring_rounds);
  if (is_pcl_ndt(h)) pcl_ndt_init_tables(h, n_pairs, st);   // the first evaluation's double angle vectors
  return DGS_OK;
}

#ifdef DGS_EXPERIMENTS
#include "ndt_queue.h"   // ndt_queue_kernel, launch_queue
#else
static void launch_queue(dgs_handle*, const NdtLaunch&) {}
#endif

static int ndt_export(dgs_handle* h, int n_pairs, dgs_result* results);

int ndt_align_pairs(dgs_handle* h, int n_pairs, const float4* const* src_ptrs_host, const int* sizes_host, const float* guesses16,
                    dgs_result* results) {
  hipStream_t st = h->stream;
  NdtLaunch L{};
  // the persistent queue kernel serves the default evaluation order (the validation orders keep their launch-per-evaluation kernels)
  const bool use_queue = kExperiments && h->ndt_queue_mode != 0 && h->ndt_fused && (h->consts.strict_order == DGS_NDT_ORDER_FAST) && n_pairs >= h->ndt_queue_min_pairs;
  int rc = ndt_setup(h, n_pairs, src_ptrs_host, sizes_host, guesses16, nullptr, &L, use_queue);
  if (rc != DGS_OK) return rc;
  const NdtPlan P = plan_align(h);
  if (use_queue) {
    launch_queue(h, L);
    // the queue kernel leaves one workgroup slot per CU free: the side stream's index build (dgs_align_batch) runs beside it
    if ((rc = side_build_now(h)) != DGS_OK) return rc;
    int* hq = reinterpret_cast<int*>(h->pinned);   // control word: [0] pairs unfinished, [1] abort bit
    DGS_HIP_TRY(h, hipMemcpyAsync(hq, h->ndt_queue.ptr, sizeof(int) * 2, hipMemcpyDeviceToHost, st));
    rc = ndt_export(h, n_pairs, results);
    if (rc != DGS_OK) return rc;
#ifdef DGS_QUEUE_STATS
    {
      int q[8];
      (void)hipMemcpy(q, h->ndt_queue.ptr + 2 * (n_pairs + 2), sizeof(q), hipMemcpyDeviceToHost);
      int q2[8];
      (void)hipMemcpy(q2, h->ndt_queue.ptr + 2 * (n_pairs + 2) + 8, sizeof(q2), hipMemcpyDeviceToHost);
      const double it = std::max(1, q[4]);
      std::fprintf(stderr, "[queue] workers %d base %d: polls %d failed_claims %d claims %d closings %d; per worker: looking for work %.1f us, in items %.1f us; per item: %.2f us = record %.2f + "
                   "points %.2f + row %.2f + ticket %.2f; per closing %.2f us\n",
                   L.queue_workers, L.queue_base, q[2], q[3], q[4], q[7], q[5] * 0.01 / L.queue_workers, q[6] * 0.01 / L.queue_workers, q[6] * 0.01 / it, q2[0] * 0.01 / it,
                   q2[1] * 0.01 / it, q2[2] * 0.01 / it, q2[3] * 0.01 / it, q2[4] * 0.01 / std::max(1, q[7]));
    }
#endif
    if (hq[1] != 0 || hq[0] != 0) {
      h->err = "ndt_queue_kernel gave up (poll guard): " + std::to_string(hq[0]) + " registrations unfinished";
      return DGS_ERR_HIP;
    }
    return DGS_OK;
  }

  if (h->early_fit.on && (rc = nn_fitness_prepare(h, n_pairs, h->early_fit.max_n, false)) != DGS_OK) return rc;
  // ---- iterate: chunks of (derivatives, solve) launches; the host looks at the done counter one chunk behind
  volatile int* flags = reinterpret_cast<volatile int*>(h->pinned);  // [0], [1]: done counts of alternating chunks
  flags[0] = flags[1] = 0;
  if (ensure_poll_events(h) != DGS_OK) return DGS_ERR_HIP;
  const bool fused_flags = P.fused;   // the default order and the upstream order close inside the launch
  if (fused_flags) {   // fused launches: every pair has a "finished" flag in pinned host memory that its closing workgroup sets
    if (h->done_flags_cap < n_pairs) {
      if (h->done_flags) (void)hipHostFree(h->done_flags);
      h->done_flags = nullptr;
      h->done_flags_cap = 0;
      DGS_HIP_TRY(h, hipHostMalloc(reinterpret_cast<void**>(&h->done_flags), sizeof(int) * (size_t)(n_pairs + 64), hipHostMallocDefault));
      h->done_flags_cap = n_pairs + 64;
    }
    for (int i = 0; i < n_pairs; i++) h->done_flags[i] = 0;   // nothing of this handle is in flight: the previous align has been synchronised
  }
  hipEvent_t* ev = h->ev_poll;
  // evaluations one iteration can take.  The fixed-step form initialises its interval as converged only while step_size > epsilon / 2; at or
  // below that (a nonsensical but legal parameter set: the soak drew step_size 0.05 with epsilon 0.1) it runs the trial loop like More-Thuente,
  // and a budget of one evaluation per iteration cut such pairs off unfinished
  const bool fixed_one = h->prm.ndt_line_search == DGS_NDT_LS_FIXED_STEP && h->prm.ndt_step_size - h->prm.transformation_epsilon / 2 > 0;
  const int per_iter = fixed_one ? 1 : (h->prm.ndt_mt_max_step_iterations + 2);
  // (upstream order with speculated Newton steps: an evaluation whose header the exact step refuses is made again -- at most twice the launches)
  const long max_evals = ((long)(h->prm.maximum_iterations + 3) * per_iter + 2) * P.evals_factor;
  const int chunk = 4;  // (derivatives, solve) launches between two looks at the done counter
  long queued = 0;
  int launch_no = 0;
  // DGS_NDT_SCHEDULE=1 (tests): every launch cuts the pairs into the slices the queue kernel would give that round, so that the two
  // paths sum the same partitions and can be compared bit for bit
  const bool schedule = h->ndt_schedule;
  NdtLaunch Lq = L;
  if (schedule) choose_queue(h, Lq);
  int round_no = 0;
  int launches_upto[2] = {0, 0};   // launches enqueued up to the end of the chunk of either slot
  int hd_rounds = 0;               // rounds whose computeHessian launch went to its own stream
  // A round whose second half goes to the third stream: round r's derivative launch on the main stream, `beside` -- the lane-per-point
  // kernels' computeHessian launch, or the Newton steps the item-compacted kernel's closings left behind -- on the third stream beside the
  // first launch of round r + 1; the first launch of round r + 2 waits for it (NdtPair::serve, lag 2)
  auto chained_round = [&](const NdtLaunch& Lr, auto&& beside) -> int {
    constexpr int R = dgs_handle::kHdEvents;
    if (launch_no >= 2) DGS_HIP_TRY(h, hipStreamWaitEvent(st, h->ev_hd_b[(launch_no - 2) % R], 0));
    launch_derivatives(h, P, Lr, launch_no);
    DGS_HIP_TRY(h, hipEventRecord(h->ev_hd_a[launch_no % R], st));
    DGS_HIP_TRY(h, hipStreamWaitEvent(h->hd_stream, h->ev_hd_a[launch_no % R], 0));
    beside();
    DGS_HIP_TRY(h, hipEventRecord(h->ev_hd_b[launch_no % R], h->hd_stream));
    hd_rounds = launch_no + 1;
    return DGS_OK;
  };
  auto enqueue_chunk = [&](int slot, int launches) -> int {
    for (int e = 0; e < launches; e++) {
      NdtLaunch Lr = L;
      if (schedule) {
        Lr.cap_blocks = ndt_queue_slices(round_no, Lq.queue_base, L.cap_blocks);
        Lr.total_blocks = n_pairs * Lr.cap_blocks;
      }
      round_no++;
      if (P.fused) {
        int rc_round = DGS_OK;
        if (P.two_kinds && P.hd_overlap) {
          rc_round = chained_round(Lr, [&] { launch_derivatives(h, P, Lr, launch_no, true); });
        } else if (P.solve_beside) {
          rc_round = chained_round(Lr, [&] {
            hipLaunchKernelGGL(ndt_strict_solve_kernel, dim3(n_pairs), dim3(kWave), 0, h->hd_stream, h->pairs.ptr, n_pairs, h->consts, h->done_flags, launch_no, 2);
          });
        } else {
          launch_derivatives(h, P, Lr, launch_no);
          if (P.two_kinds) launch_derivatives(h, P, Lr, launch_no, true);   // same round number: NdtPair::serve
        }
        if (rc_round != DGS_OK) return rc_round;
        launch_no++;
      } else {
        launch_derivatives(h, P, Lr);
        launch_solve(h, P, Lr);
        if (P.two_kinds) {
          launch_derivatives(h, P, Lr, -1, true);
          launch_solve(h, P, Lr);
        }
      }
    }
    queued += launches;
    launches_upto[slot] = launch_no;
    if (!fused_flags) DGS_HIP_TRY(h, hipMemcpyAsync(const_cast<int*>(&flags[slot]), h->done_counter.ptr, sizeof(int), hipMemcpyDeviceToHost, st));
    DGS_HIP_TRY(h, hipEventRecord(ev[slot], st));
    return DGS_OK;
  };
  auto pairs_done = [&](int slot) -> int {
    if (!fused_flags) return flags[slot];
    int n = 0;
    for (int i = 0; i < n_pairs; i++) n += reinterpret_cast<volatile int*>(h->done_flags)[i] != 0;
    return n;
  };
  // ---- early fitness (dgs_align_batch, compute_fitness): the nearest-neighbour walk of a candidate needs only its final transform, and
  // the tail of a batch -- a few pairs still iterating, 11 us of latency per launch -- leaves most of the chip idle.  At every chunk
  // boundary the pairs whose closing launch is KNOWN to have completed (flag = launch + 1 <= the launches the synchronised event covers:
  // their state is in memory, not in some XCD's L2) get their walk on the low-priority side stream, behind the target's index build.
  // Whatever is left at the end goes on the main stream.  A pair's rows and their order do not depend on which launch walked it.
  const bool early = h->early_fit.on && fused_flags;
  std::vector<char> walked(early ? n_pairs : 0, 0);
  const float* fit_T = reinterpret_cast<const float*>(reinterpret_cast<const char*>(h->pairs.ptr) + offsetof(NdtPair, final_T));
  std::vector<int> ready;
  auto walk_finished = [&](int completed, bool rest) -> int {
    ready.clear();
    for (int i = 0; i < n_pairs; i++) {
      if (walked[i]) continue;
      const int f = reinterpret_cast<volatile int*>(h->done_flags)[i];
      if (rest || (f != 0 && f <= completed)) ready.push_back(i);
    }
    // a walk's workgroups live ~100 us whatever the number of pairs: few large launches, not one per finished pair
    if (ready.empty() || (!rest && ((int)ready.size() < h->early_fit.min_pairs || n_pairs - pairs_done(0) > h->early_fit.max_active))) return DGS_OK;
    for (int i : ready) walked[i] = 1;
    nn_fitness_enqueue(h, rest ? st : h->side_stream, h->tgt->bvh, ready.data(), (int)ready.size(), h->src_ptrs.ptr, h->src_sizes.ptr, fit_T, sizeof(NdtPair),
                       h->early_fit.max_range, 0.0, rest ? 0 : h->early_fit.lds_kb);
    if (!rest) {
      DGS_HIP_TRY(h, hipEventRecord(h->ev_join, h->side_stream));
      h->side_pending = true;
    }
    return DGS_OK;
  };
  int cur = 0;
  // with a build waiting for the side stream the first chunk is twice as long: the host needs ~0.1 ms to enqueue that build, and
  // the main stream must not run dry meanwhile.  (Also tried: the fused launches writing the count of finished pairs into pinned
  // host memory themselves instead of a copy command per chunk -- the one more kernel argument pushed the derivative loop over its
  // 128 VGPRs (4 spilled registers, 34 -> 40 us per launch): the copies stay.)
  rc = enqueue_chunk(0, h->side_build_deferred ? 2 * chunk : chunk);
  bool finished = false;
  bool first = true;
  while (rc == DGS_OK) {
    const bool more = queued < max_evals;
    if (more) rc = enqueue_chunk(cur ^ 1, chunk);
    if (rc != DGS_OK) break;
    // two chunks are in flight: now the host has time to enqueue what dgs_align_batch left for the side stream
    if (first && (rc = side_build_now(h)) != DGS_OK) break;
    first = false;
    hipError_t e = hipEventSynchronize(ev[cur]);
    if (e != hipSuccess) { h->err = std::string("hipEventSynchronize: ") + hipGetErrorString(e); rc = DGS_ERR_HIP; break; }
    if (early && (rc = walk_finished(launches_upto[cur], false)) != DGS_OK) break;
    if (pairs_done(cur) >= n_pairs) { finished = true; break; }
    if (!more) break;
    cur ^= 1;
  }
  if (hd_rounds > 0) {   // the main stream takes the computeHessian stream's launches in (they are in order: the last one covers them all)
    hipError_t e = hipStreamWaitEvent(st, h->ev_hd_b[(hd_rounds - 1) % dgs_handle::kHdEvents], 0);
    if (e != hipSuccess && rc == DGS_OK) { h->err = std::string("hipStreamWaitEvent: ") + hipGetErrorString(e); rc = DGS_ERR_HIP; }
  }
  if (rc != DGS_OK) return rc;
  (void)finished;  // pairs that did not finish inside max_evals export converged = 0
  if (early) {
    // the main stream waits for the side stream (index build, early walks), walks the rest, totals everything and copies it out: the
    // export's synchronisation below covers all of it
    if (side_join(h) != DGS_OK) return DGS_ERR_HIP;
    if ((rc = walk_finished(0, true)) != DGS_OK) return rc;
    if ((rc = nn_fitness_totals_enqueue(h, n_pairs)) != DGS_OK) return rc;
    h->early_fit.enqueued = true;
  }
  return ndt_export(h, n_pairs, results);
}

// ---- export: final transforms / flags / counts of every pair to the caller's result array
static int ndt_export(dgs_handle* h, int n_pairs, dgs_result* results) {
  hipStream_t st = h->stream;
  char* base = reinterpret_cast<char*>(h->pinned);
  const size_t off_out = ((256 + sizeof(NdtInit) * n_pairs + sizeof(void*) * n_pairs + sizeof(int) * n_pairs) + 255) & ~(size_t)255;
  NdtOut* hout = reinterpret_cast<NdtOut*>(base + off_out);
  NdtOut* dout = reinterpret_cast<NdtOut*>(h->partials.ptr);  // partial rows are dead now; reuse (>= 32 doubles per pair)
  hipLaunchKernelGGL(ndt_export_kernel, dim3((n_pairs + 63) / 64), dim3(64), 0, st, h->pairs.ptr, n_pairs, dout);
  DGS_HIP_TRY(h, hipMemcpyAsync(hout, dout, sizeof(NdtOut) * n_pairs, hipMemcpyDeviceToHost, st));
  DGS_HIP_TRY(h, hipStreamSynchronize(st));
  DGS_HIP_TRY(h, hipGetLastError());
  int64_t evals = 0, reused = 0;
  for (int i = 0; i < n_pairs; i++) {
    std::memcpy(results[i].final_transformation, hout[i].T, sizeof(float) * 16);
    results[i].converged = hout[i].converged;
    results[i].iterations = hout[i].iterations;
    results[i].evaluations = hout[i].evaluations;
    results[i].status = DGS_OK;
    results[i].score = hout[i].score;
    results[i].fitness = NAN;
    evals += hout[i].evaluations;
    reused += hout[i].reused;
  }
  // what ran on the device: with the reuse on, a cached trial pose is counted by upstream and the records, and launches nothing
  h->last_evaluations = evals - (h->consts.reuse_trials ? reused : 0);
  h->last_reused = reused;
  return DGS_OK;
}

// Test hook: poses after every outer iteration of pair `pair` of the last align / batch.
int ndt_trajectory(dgs_handle* h, int pair, double* out, int* len) {
  std::vector<char> buf(sizeof(NdtPair));
  DGS_HIP_TRY(h, hipStreamSynchronize(h->stream));
  DGS_HIP_TRY(h, hipMemcpy(buf.data(), h->pairs.ptr + pair, sizeof(NdtPair), hipMemcpyDeviceToHost));
  const NdtPair* st = reinterpret_cast<const NdtPair*>(buf.data());
#ifdef DGS_CLOSE_STAMPS
  const int n = kTrajCap;
#else
  const int n = std::min(st->s.traj_len, kTrajCap);
#endif
  for (int i = 0; i < n; i++)
    for (int k = 0; k < 6; k++) out[i * 6 + k] = st->traj[i][k];
  *len = n;
  return DGS_OK;
}

// Test hook: one computeDerivatives evaluation on the device.
int ndt_probe(dgs_handle* h, const double* p6, const float* T16, double* score, double* g6, double* H36, int kind) {
  hipStream_t st = h->stream;
  NdtLaunch L{};
  const float4* src = h->src->pts.ptr;
  const int n = (int)h->ns;
  float T[16];
  if (T16) {
    std::memcpy(T, T16, sizeof(T));
  } else {  // pose_to_matrix in float, as the solver builds it
    const float rx = (float)p6[3], ry = (float)p6[4], rz = (float)p6[5];
    const float cx = (float)std::cos((double)rx), sx = (float)std::sin((double)rx), cy = (float)std::cos((double)ry), sy = (float)std::sin((double)ry),
                cz = (float)std::cos((double)rz), sz = (float)std::sin((double)rz);
    auto mul = [](float a, float b) { volatile float r = a * b; return (float)r; };  // keep host products un-fused
    T[0] = mul(cy, cz); T[4] = mul(-cy, sz); T[8] = sy; T[12] = (float)p6[0];
    { volatile float a = mul(cx, sz), b = mul(mul(sx, sy), cz); T[1] = a + b; }
    { volatile float a = mul(cx, cz), b = mul(mul(sx, sy), sz); T[5] = a - b; }
    T[9] = mul(-sx, cy); T[13] = (float)p6[1];
    { volatile float a = mul(sx, sz), b = mul(mul(cx, sy), cz); T[2] = a - b; }
    { volatile float a = mul(sx, cz), b = mul(mul(cx, sy), sz); T[6] = a + b; }
    T[10] = mul(cx, cy); T[14] = (float)p6[2];
    T[3] = T[7] = T[11] = 0.f; T[15] = 1.f;
  }
  int rc = ndt_setup(h, 1, &src, &n, T, p6, &L, false, kind == 0 ? 3 : kind);   // kind 0 (PCL_NDT_HIP): score + gradient
  if (rc != DGS_OK) return rc;
  const NdtPlan P = plan_align(h);
  launch_derivatives(h, P, L, -1, kind == 2);
  launch_solve(h, P, L);
  char* base = reinterpret_cast<char*>(h->pinned);
  NdtPair* hp = reinterpret_cast<NdtPair*>(base + ((h->pinned_bytes - sizeof(NdtPair) - 64) & ~(size_t)63));
  DGS_HIP_TRY(h, hipMemcpyAsync(hp, h->pairs.ptr, sizeof(NdtPair), hipMemcpyDeviceToHost, st));
  DGS_HIP_TRY(h, hipStreamSynchronize(st));
  DGS_HIP_TRY(h, hipGetLastError());
  *score = hp->s.score;
  for (int k = 0; k < 6; k++) g6[k] = hp->s.grad[k];
  for (int k = 0; k < 36; k++) H36[k] = hp->s.hess[k];
  return DGS_OK;
}

// Test hook (dgs_strict_row_probe): one workgroup reduces a [kBlock][kStrictAccum] matrix of per-thread totals twice -- as the item-compacted
// kernel's timed instantiation does, in passes as wide as its wave's table region allows, and in the stand-alone form's passes of 11 columns.
__global__ __launch_bounds__(kBlock) void strict_row_probe_kernel(const double* __restrict__ totals, const int ncol, double* __restrict__ rows2) {
  constexpr int kBytes = StrictTile<DGS_NDT_DIRECT7, true, true>::kTableBytes;
  __shared__ __attribute__((aligned(16))) unsigned char s_tab[kBlock / kWave][kBytes];
  double acc[kStrictAccum];
#pragma unroll
  for (int k = 0; k < kStrictAccum; k++) acc[k] = totals[(size_t)threadIdx.x * kStrictAccum + k];
  strict_block_row<false, false, kBytes>(acc, ncol, rows2, reinterpret_cast<double*>(s_tab[threadIdx.x >> 6]));
  __syncthreads();
  strict_block_row<false, true>(acc, ncol, rows2 + kStrictPad);
}
int strict_row_probe(dgs_handle* h, const double* totals, int ncol, double* rows2) {
  DevBuf<double> d;   // the matrix, then the two rows
  const size_t n_in = (size_t)kBlock * kStrictAccum, n_out = 2 * (size_t)kStrictPad;
  hipError_t e = d.reserve(n_in + n_out);
  if (e == hipSuccess) e = hipMemcpyAsync(d.ptr, totals, sizeof(double) * n_in, hipMemcpyHostToDevice, h->stream);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(strict_row_probe_kernel, dim3(1), dim3(kBlock), 0, h->stream, d.ptr, ncol, d.ptr + n_in);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(rows2, d.ptr + n_in, sizeof(double) * n_out, hipMemcpyDeviceToHost, h->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
  d.release();
  if (e != hipSuccess) {
    h->err = std::string("dgs_strict_row_probe: ") + hipGetErrorString(e);
    return DGS_ERR_HIP;
  }
  return DGS_OK;
}

}  // namespace dgs
