// ICP_HIP: pcl::IterativeClosestPoint<PointXYZ, PointXYZ>::computeTransformation with DefaultConvergenceCriteria (point to point), the
// object the reference's factory builds for "ICP" (src/hdl_graph_slam/registrations.cpp:59-64).  Behaviour: DESIGN.md "ICP_HIP".
//
// MI355X design
//   * One launch per ICP iteration for the whole batch (icp_iterate_kernel).  Every pair owns a FIXED number of workgroups (slices), a
//     function of its own size only: workgroup -> (pair, slice) comes from a host-built table, so a pair's sums -- and with them its
//     result -- do not depend on which other pairs share the batch.  Workgroups of finished pairs return at once.
//   * A slice walks kIcpSlicePoints source points in the source index's spatial order (w = original index), one 8-lane group per
//     point: apply the previous iteration's T_k to the stored working copy and write it back, gated exact 1-NN in the target
//     (nn_query_group, warm bounds from the wave's previous round), gather q, accumulate count, sum d2, sum p, sum q, sum p q^T in
//     double, about an origin o = the target's first finite point.  Wave DPP sums -> LDS -> one fixed-order row per slice.
//   * The last workgroup of a pair (ticket, write-through rows: common.h "in-launch hand-off") sums the rows in slice order and runs
//     Kabsch (jacobi_svd3_d in double), the float update of final_transformation_ and the convergence criteria on one lane.
//   * Reciprocal mode (setUseReciprocalCorrespondences): correctness first.  The host sequences one round at a time: apply T_k
//     (icp_apply_kernel), build an index over every working copy (bvh_build), then the same iteration launch with the reverse query.
#include <cfloat>
#include <cmath>
#include <cstddef>
#include <cstring>
#include <vector>

#include "batch_rounds.h"
#include "handle.h"
#include "nn_group.h"
#include "slice_rows.h"
#include "small_linalg.h"

namespace dgs {

struct IcpPair {
  float Tk[12];        // row-major 3x4: the last incremental transform, applied to the working copy at the start of the next launch
                       // (the guess before the first iteration)
  float final_T[16];   // column-major, = final_transformation_
  double prev_mse;     // DefaultConvergenceCriteria::correspondences_prev_mse_ (DBL_MAX before the first iteration)
  double mse;          // MSE of the last iteration's kept pairs (DBL_MAX before the first iteration)
  int active;          // 0: every workgroup of this pair returns at once
  int iterations;      // nr_iterations_
  int evaluations;     // correspondence passes run
  int converged;
  int ticket;          // slices of this pair that have published their row in the running launch
  int last_corr;       // kept pairs of the last correspondence pass
  int pad[2];
};

struct IcpItem {             // one registration of a batch
  const float4* src;         // source points in the caller's order
  const float4* src_sorted;  // the same points in their own index's order (Hilbert / k-d), w = original index
  float4* W;                 // the working copy (input_transformed), caller's order
  BvhView wv;                // reciprocal mode: index over W of this round
  int n, slice0, n_slices, pad;
};

struct IcpConsts {
  double max_sq;       // max_correspondence_distance^2, squared in double (PCL's max_dist_sqr)
  double trans_thr, rot_thr, mse_abs, mse_rel;
  float gate;          // largest float f with (double) f <= max_sq: d2 <= gate <=> (double) d2 <= max_sq
  int max_iterations, reciprocal, traj_cap;
};

constexpr int kIcpRun = 8;                                   // points per 8-lane group and slice
constexpr int kIcpSlicePoints = (kBlock / 8) * kIcpRun;      // 256 points per workgroup
constexpr int kIcpAccum = 17;                                // count, sum d2, sum p (3), sum q (3), sum p q^T (9, row-major)
constexpr int kIcpPad = 32;                                  // row stride (doubles)

// ================================================================================================ device
__device__ __forceinline__ double icp_det3(const double* A) {   // row-major 3 x 3
  return A[0] * (A[4] * A[8] - A[5] * A[7]) - A[1] * (A[3] * A[8] - A[5] * A[6]) + A[2] * (A[3] * A[7] - A[4] * A[6]);
}

// Kabsch / Umeyama without scale (pcl::registration::TransformationEstimationSVD) from the pair's totals, then the update and
// DefaultConvergenceCriteria::hasConverged.  One lane.  tot: about the origin o (p' = p - o, q' = q - o).
__device__ __noinline__ void icp_close_pair(IcpPair* st, const double* tot, const double* o, const IcpConsts c, int* done_counter, float* traj_T,
                                            double* traj_mse, int* traj_n, const int pair) {
#pragma clang fp contract(off)
  const double n = tot[0];
  st->evaluations += 1;
  st->last_corr = (int)n;
  if (n < 3.0) {   // "Not enough correspondences found": converged_ = false, the loop ends, nr_iterations_ unchanged
    st->converged = 0;
    st->active = 0;
    atomicAdd(done_counter, 1);
    return;
  }
  double cp[3], cq[3];
  for (int a = 0; a < 3; a++) { cp[a] = tot[2 + a] / n; cq[a] = tot[5 + a] / n; }
  // H = sum (p - cp)(q - cq)^T = sum p' q'^T - (sum p') cq'^T
  double H[9];
  for (int a = 0; a < 3; a++)
    for (int b = 0; b < 3; b++) H[a * 3 + b] = tot[8 + a * 3 + b] - tot[2 + a] * cq[b];
  double U[9], V[9], sv[3];
  jacobi_svd3_d(H, U, V, sv);   // H = U diag(sv) V^T, row-major factors
  const double dU = icp_det3(U), dV = icp_det3(V);
  if (dU * dV < 0.0)
    for (int r = 0; r < 3; r++) V[r * 3 + 2] = -V[r * 3 + 2];
  double R[9];
  for (int r = 0; r < 3; r++)
    for (int k = 0; k < 3; k++) R[r * 3 + k] = (V[r * 3 + 0] * U[k * 3 + 0] + V[r * 3 + 1] * U[k * 3 + 1]) + V[r * 3 + 2] * U[k * 3 + 2];
  float T[12];
  for (int r = 0; r < 3; r++) {
    const double pr = cp[0] + o[0], pg = cp[1] + o[1], pb = cp[2] + o[2];
    const double t = (cq[r] + o[r]) - ((R[r * 3 + 0] * pr + R[r * 3 + 1] * pg) + R[r * 3 + 2] * pb);
    for (int k = 0; k < 3; k++) T[r * 4 + k] = (float)R[r * 3 + k];
    T[r * 4 + 3] = (float)t;
  }
  // final = T_k * final: float 4 x 4 product, each entry ((T0 F0 + T1 F1) + T2 F2) + T3 F3, every operation rounded; T_k's row 3 is (0, 0, 0, 1)
  float F[16];
  for (int k = 0; k < 16; k++) F[k] = st->final_T[k];
  for (int cc = 0; cc < 4; cc++) {
    for (int r = 0; r < 3; r++)
      st->final_T[cc * 4 + r] = add_rn(add_rn(add_rn(mul_rn(T[r * 4 + 0], F[cc * 4 + 0]), mul_rn(T[r * 4 + 1], F[cc * 4 + 1])), mul_rn(T[r * 4 + 2], F[cc * 4 + 2])),
                                       mul_rn(T[r * 4 + 3], F[cc * 4 + 3]));
    st->final_T[cc * 4 + 3] = add_rn(add_rn(add_rn(mul_rn(0.f, F[cc * 4 + 0]), mul_rn(0.f, F[cc * 4 + 1])), mul_rn(0.f, F[cc * 4 + 2])), mul_rn(1.f, F[cc * 4 + 3]));
  }
  for (int k = 0; k < 12; k++) st->Tk[k] = T[k];
  const int it = st->iterations + 1;
  st->iterations = it;
  const double mse = tot[1] / n;
  st->mse = mse;
  if (it - 1 < c.traj_cap) {
    const size_t e = (size_t)pair * c.traj_cap + (it - 1);
    float* Tt = traj_T + e * 16;
    for (int r = 0; r < 3; r++)
      for (int k = 0; k < 4; k++) Tt[k * 4 + r] = T[r * 4 + k];
    Tt[3] = Tt[7] = Tt[11] = 0.f;
    Tt[15] = 1.f;
    traj_mse[e] = mse;
    traj_n[e] = (int)n;
  }
  // DefaultConvergenceCriteria::hasConverged (max_iterations_similar_transforms_ = 0), on T_k read as double
  bool conv = it >= c.max_iterations;
  if (!conv) {
    const double cos_angle = 0.5 * ((((double)T[0] + (double)T[5]) + (double)T[10]) - 1.0);
    const double t0 = T[3], t1 = T[7], t2 = T[11];
    const double tsq = (t0 * t0 + t1 * t1) + t2 * t2;
    conv = cos_angle >= c.rot_thr && tsq <= c.trans_thr;
  }
  if (!conv) {
    const double d = fabs(mse - st->prev_mse);
    conv = d < c.mse_abs || d / st->prev_mse < c.mse_rel;
  }
  if (conv) {
    st->converged = 1;
    st->active = 0;
    atomicAdd(done_counter, 1);
  } else {
    st->prev_mse = mse;
  }
}

// One ICP iteration of every active pair.  RECIPROCAL: icp_apply_kernel has already moved the working copies, the kept pairs need the
// reverse query as well.
template <bool RECIPROCAL>
__global__ __launch_bounds__(kBlock, 4) void icp_iterate_kernel(const BvhView tv, const float4* __restrict__ tgt, const int* __restrict__ origin, const int nt,
                                                             const IcpItem* __restrict__ items,
                                                             IcpPair* __restrict__ pairs, const int* __restrict__ blk_pair, double* __restrict__ rows,
                                                             const IcpConsts c, int* __restrict__ done_counter, float* __restrict__ traj_T,
                                                             double* __restrict__ traj_mse, int* __restrict__ traj_n) {
  const int pair = blk_pair[blockIdx.x];
  IcpPair* st = pairs + pair;
  if (!st->active) return;   // uniform per pair: the closing workgroup clears it after every slice of this launch has read it
  const IcpItem it = items[pair];
  const int slice = (int)blockIdx.x - it.slice0;
  const int n = it.n;
  constexpr bool apply = !RECIPROCAL;
  const bool from_src = st->evaluations == 0;
  float T[12];
#pragma unroll
  for (int k = 0; k < 12; k++) T[k] = st->Tk[k];
  // the origin of the moment sums: the target's first finite point (none: no correspondence can be kept either)
  const int oi = *origin;
  const float4 o4 = (oi >= 0 && oi < nt) ? tgt[oi] : make_float4(0.f, 0.f, 0.f, 0.f);
  const double ox = o4.x, oy = o4.y, oz = o4.z;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, sub = lane & 7;
  const int first = (slice * (kBlock / kWave) + wave) * (8 * kIcpRun) + (lane >> 3);
  double acc[kIcpAccum];
#pragma unroll
  for (int k = 0; k < kIcpAccum; k++) acc[k] = 0.0;
  float px = 0.f, py = 0.f, pz = 0.f, prev_best = INFINITY;
  bool prev_found = false;
  for (int r = 0; r < kIcpRun; r++) {
    const int pos = first + r * 8;
    const float4 s = (pos < n) ? it.src_sorted[pos] : make_float4(0.f, 0.f, 0.f, 0.f);
    const int i = (pos < n) ? (int)__float_as_uint(s.w) : -1;
    const bool alive = pos < n && i >= 0 && i < n;
    float x = 0.f, y = 0.f, z = 0.f;
    if (alive) {
      const float4 w = (apply && from_src) ? it.src[i] : it.W[i];
      if (apply) {   // input_transformed = T_k * input_transformed (the guess * input_ before the first iteration)
        x = affine_row_rn(T[0], T[1], T[2], T[3], w.x, w.y, w.z);
        y = affine_row_rn(T[4], T[5], T[6], T[7], w.x, w.y, w.z);
        z = affine_row_rn(T[8], T[9], T[10], T[11], w.x, w.y, w.z);
        if (sub == 0) it.W[i] = make_float4(x, y, z, 0.f);
      } else {
        x = w.x; y = w.y; z = w.z;
      }
    }
    float best;
    int bi;
    const float bound = fminf(c.gate, nn_warm_bound_round(prev_best, prev_found, x, y, z, px, py, pz));
    nn_query_group(tv, x, y, z, alive, bound, best, bi);
    prev_found = alive && bi != 0x7FFFFFFF;
    prev_best = best;
    px = x; py = y; pz = z;
    bool keep = alive && bi != 0x7FFFFFFF;   // found within the bound: d2 <= gate
    float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
    if (keep) q = tgt[bi];
    if (RECIPROCAL) {   // the 1-NN of target[j] among the working copy must be i, within the gate as well
      float best2;
      int bi2;
      nn_query_group(it.wv, q.x, q.y, q.z, keep, c.gate, best2, bi2);
      keep = keep && bi2 == i;
    }
    if (keep && sub == 0) {
      const double a0 = (double)x - ox, a1 = (double)y - oy, a2 = (double)z - oz;
      const double b0 = (double)q.x - ox, b1 = (double)q.y - oy, b2 = (double)q.z - oz;
      acc[0] += 1.0;
      acc[1] += (double)best;
      acc[2] += a0; acc[3] += a1; acc[4] += a2;
      acc[5] += b0; acc[6] += b1; acc[7] += b2;
      acc[8] += a0 * b0; acc[9] += a0 * b1; acc[10] += a0 * b2;
      acc[11] += a1 * b0; acc[12] += a1 * b1; acc[13] += a1 * b2;
      acc[14] += a2 * b0; acc[15] += a2 * b1; acc[16] += a2 * b2;
    }
  }
  // this slice's row, the pair's ticket; in the pair's closing workgroup the rows summed in slice order (slice_rows.h)
  __shared__ double tot[kIcpPad];
  if (!slice_rows_close(acc, kIcpAccum, rows, it.slice0, it.n_slices, &st->ticket, tot)) return;
  if (threadIdx.x == 0) {
    const double o[3] = {ox, oy, oz};
    icp_close_pair(st, tot, o, c, done_counter, traj_T, traj_mse, traj_n, pair);
  }
}

// Index of the first point of the target with three finite coordinates -> *out (preset to a value >= n).  One atomic per wave.
__global__ __launch_bounds__(kBlock) void icp_origin_kernel(const float4* __restrict__ pts, const int n, int* __restrict__ out) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  bool ok = false;
  if (i < n) {
    const float4 p = pts[i];
    ok = isfinite(p.x) && isfinite(p.y) && isfinite(p.z);
  }
  const unsigned long long m = __ballot(ok);
  if (m != 0ull && (threadIdx.x & 63) == 0) atomicMin(out, (int)(blockIdx.x * kBlock + (threadIdx.x & ~63)) + __ffsll((long long)m) - 1);
}

// Reciprocal mode, first step of a round: input_transformed = T_k * input_transformed for every active pair (same workgroup table).
__global__ __launch_bounds__(kBlock) void icp_apply_kernel(const IcpItem* __restrict__ items, const IcpPair* __restrict__ pairs, const int* __restrict__ blk_pair) {
  const int pair = blk_pair[blockIdx.x];
  const IcpPair* st = pairs + pair;
  if (!st->active) return;
  const IcpItem it = items[pair];
  const int slice = (int)blockIdx.x - it.slice0;
  float T[12];
#pragma unroll
  for (int k = 0; k < 12; k++) T[k] = st->Tk[k];
  const bool from_src = st->evaluations == 0;
  for (int i = slice * kIcpSlicePoints + (int)threadIdx.x; i < min(it.n, (slice + 1) * kIcpSlicePoints); i += kBlock) {
    const float4 w = from_src ? it.src[i] : it.W[i];
    it.W[i] = make_float4(affine_row_rn(T[0], T[1], T[2], T[3], w.x, w.y, w.z), affine_row_rn(T[4], T[5], T[6], T[7], w.x, w.y, w.z),
                          affine_row_rn(T[8], T[9], T[10], T[11], w.x, w.y, w.z), 0.f);
  }
}

struct IcpInit {
  float guess[16];   // column-major
  int n;
};

__global__ void icp_init_kernel(IcpPair* __restrict__ pairs, const IcpInit* __restrict__ inits, const int n_pairs) {
  const int pi = blockIdx.x * blockDim.x + threadIdx.x;
  if (pi >= n_pairs) return;
  IcpPair* st = pairs + pi;
  const IcpInit* in = inits + pi;
  for (int r = 0; r < 3; r++)
    for (int cc = 0; cc < 4; cc++) st->Tk[r * 4 + cc] = in->guess[cc * 4 + r];
  for (int k = 0; k < 16; k++) st->final_T[k] = in->guess[k];
  st->prev_mse = DBL_MAX;
  st->mse = DBL_MAX;
  st->active = in->n > 0 ? 1 : 0;   // an empty source never starts (PCL's initCompute refuses it)
  st->iterations = 0;
  st->evaluations = 0;
  st->converged = 0;
  st->ticket = 0;
  st->last_corr = 0;
  st->pad[0] = st->pad[1] = 0;
}

// ================================================================================================ host
static IcpConsts icp_consts(const dgs_handle* h) {
  IcpConsts c;
  const double d = h->prm.gicp_max_correspondence_distance;
  c.max_sq = d * d;
  float g = (float)c.max_sq;   // round to nearest, then step down until (double) g <= max_sq
  if (!(c.max_sq >= 0.0)) g = -1.f;
  else if (c.max_sq >= (double)FLT_MAX) g = FLT_MAX;
  else if ((double)g > c.max_sq) g = std::nextafter(g, 0.f);
  c.gate = g;
  c.trans_thr = h->prm.transformation_epsilon;
  c.rot_thr = h->icp_opt.rotation_epsilon > 0 ? h->icp_opt.rotation_epsilon : 1.0 - h->prm.transformation_epsilon;
  c.mse_abs = 1e-12;
  c.mse_rel = h->icp_opt.euclidean_fitness_epsilon;
  c.max_iterations = h->prm.maximum_iterations;
  c.reciprocal = h->icp_opt.use_reciprocal_correspondences ? 1 : 0;
  c.traj_cap = std::max(1, h->prm.maximum_iterations);
  return c;
}

using IcpStaging = BatchStaging<IcpInit, IcpItem, IcpPair>;

// IterativeClosestPoint::align for every source of a batch against the handle's target.  The target needs its exact-NN index only;
// every source its own index (for the spatial order of the correspondence walk).  No covariances anywhere.
int icp_align_batch(dgs_handle* h, int n, CloudState* const* srcs, const float* guesses16, dgs_result* out) {
  hipStream_t st = h->stream;
  const IcpConsts c = icp_consts(h);
  int rc = ensure_target_index(h);
  if (rc) return rc;
  int64_t total = 0;
  int n_live = 0;
  SliceTable slices(n, srcs, kIcpSlicePoints);
  const int total_slices = slices.total_slices;
  for (int i = 0; i < n; i++) {
    CloudState& s = *srcs[i];
    total += s.n;
    if (s.n <= 0) continue;
    n_live++;
    rc = ensure_walk_order(h, s);
    if (rc) return rc;
  }
  DGS_HIP_TRY(h, h->ipairs.reserve(n));
  DGS_HIP_TRY(h, h->iitems.reserve(n));
  DGS_HIP_TRY(h, h->icp_w.reserve((size_t)std::max<int64_t>(total, 1)));
  DGS_HIP_TRY(h, h->icp_traj_T.reserve((size_t)n * c.traj_cap * 16));
  DGS_HIP_TRY(h, h->icp_traj_mse.reserve((size_t)n * c.traj_cap));
  DGS_HIP_TRY(h, h->icp_traj_n.reserve((size_t)n * c.traj_cap));
  DGS_HIP_TRY(h, h->done_counter.reserve(16));
  DGS_HIP_TRY(h, h->icp_origin.reserve(1));
  if (c.reciprocal && h->icp_w_bvh.size() < (size_t)n) h->icp_w_bvh.resize(n);
  const IcpStaging stg(h, n);
  if (stg.ensure() != DGS_OK) return DGS_ERR_HIP;
  IcpInit* hin = stg.inits();
  IcpItem* hit = stg.items();
  int64_t off = 0;
  for (int i = 0; i < n; i++) {
    const CloudState& s = *srcs[i];
    std::memcpy(hin[i].guess, guesses16 ? guesses16 + 16 * i : kIdentity16, sizeof(float) * 16);
    hin[i].n = (int)s.n;
    hit[i].src = s.pts.ptr;
    hit[i].src_sorted = walk_sorted(s);
    hit[i].W = h->icp_w.ptr + off;
    std::memset(&hit[i].wv, 0, sizeof(BvhView));
    hit[i].n = (int)s.n;
    hit[i].slice0 = slices.slice0[i];
    hit[i].n_slices = slices.n_slices[i];
    hit[i].pad = 0;
    off += s.n;
  }
  rc = slices.upload(h, kIcpPad);
  if (rc) return rc;
  DGS_HIP_TRY(h, h->inits.reserve((size_t)n));   // staging shared with NDT / GICP
  static_assert(sizeof(NdtInit) >= sizeof(IcpInit), "init staging buffer is shared with NDT");
  DGS_HIP_TRY(h, hipMemcpyAsync(h->inits.ptr, hin, (size_t)n * sizeof(IcpInit), hipMemcpyHostToDevice, st));
  DGS_HIP_TRY(h, hipMemcpyAsync(h->iitems.ptr, hit, (size_t)n * sizeof(IcpItem), hipMemcpyHostToDevice, st));
  DGS_HIP_TRY(h, hipMemsetAsync(h->done_counter.ptr, 0, 16 * sizeof(int), st));
  DGS_HIP_TRY(h, hipMemsetAsync(h->icp_origin.ptr, 0x7F, sizeof(int), st));   // 0x7F7F7F7F >= any cloud size: "no finite point"
  const int nt = (int)h->nt;
  if (nt > 0) hipLaunchKernelGGL(icp_origin_kernel, dim3((nt + kBlock - 1) / kBlock), dim3(kBlock), 0, st, h->tgt->pts.ptr, nt, h->icp_origin.ptr);
  hipLaunchKernelGGL(icp_init_kernel, dim3((n + 63) / 64), dim3(64), 0, st, h->ipairs.ptr, reinterpret_cast<const IcpInit*>(h->inits.ptr), n);
  DGS_HIP_TRY(h, hipStreamSynchronize(st));   // slices.blk is pageable host memory
  const BvhView tv = make_bvh_view(h->tgt->bvh);
  const long max_rounds = std::max(1, h->prm.maximum_iterations);
  auto launch_round = [&](bool reciprocal) {
    int slot = prof_begin(h, DGS_K_NN_SEARCH);
    if (reciprocal)
      hipLaunchKernelGGL(icp_iterate_kernel<true>, dim3(total_slices), dim3(kBlock), 0, st, tv, h->tgt->pts.ptr, h->icp_origin.ptr, nt, h->iitems.ptr, h->ipairs.ptr, h->slice_blk_pair.ptr,
                         h->slice_rows.ptr, c, h->done_counter.ptr, h->icp_traj_T.ptr, h->icp_traj_mse.ptr, h->icp_traj_n.ptr);
    else
      hipLaunchKernelGGL(icp_iterate_kernel<false>, dim3(total_slices), dim3(kBlock), 0, st, tv, h->tgt->pts.ptr, h->icp_origin.ptr, nt, h->iitems.ptr, h->ipairs.ptr, h->slice_blk_pair.ptr,
                         h->slice_rows.ptr, c, h->done_counter.ptr, h->icp_traj_T.ptr, h->icp_traj_mse.ptr, h->icp_traj_n.ptr);
    prof_end(h, DGS_K_NN_SEARCH, slot);
  };
  if (n_live > 0 && !c.reciprocal) {
    rc = run_rounds_polled(h, n_live, max_rounds, 4, [&] { launch_round(false); });
    if (rc != DGS_OK) return rc;
  } else if (n_live > 0) {
    // reciprocal mode: one round at a time -- move the working copies, index them, then the iteration launch with the reverse query
    for (long r = 0; r < max_rounds; r++) {
      rc = stg.read_back(h->ipairs, n, "ICP state");
      if (rc) return rc;
      const IcpPair* hp = stg.pairs();
      std::vector<char> act(n);
      int live = 0;
      for (int i = 0; i < n; i++) { act[i] = hp[i].active != 0; live += act[i]; }
      if (live == 0) break;
      hipLaunchKernelGGL(icp_apply_kernel, dim3(total_slices), dim3(kBlock), 0, st, h->iitems.ptr, h->ipairs.ptr, h->slice_blk_pair.ptr);
      DGS_HIP_TRY(h, hipGetLastError());
      for (int i = 0; i < n; i++) {
        if (!act[i]) continue;
        rc = bvh_build(h, h->icp_w_bvh[i], hit[i].W, hit[i].n);
        if (rc) return rc;
        hit[i].wv = make_bvh_view(h->icp_w_bvh[i]);
      }
      DGS_HIP_TRY(h, hipMemcpyAsync(h->iitems.ptr, hit, (size_t)n * sizeof(IcpItem), hipMemcpyHostToDevice, st));
      launch_round(true);
      DGS_HIP_TRY(h, hipGetLastError());
    }
  }
  rc = stg.read_back(h->ipairs, n, "ICP state");
  if (rc) return rc;
  const IcpPair* hp = stg.pairs();
  long evals = 0;
  h->icp_last_iters.assign(n, 0);
  h->icp_traj_cap = c.traj_cap;
  for (int i = 0; i < n; i++) {
    std::memcpy(out[i].final_transformation, hp[i].final_T, sizeof(float) * 16);
    const bool empty = srcs[i]->n <= 0;
    out[i].converged = (!empty && !hp[i].active) ? hp[i].converged : 0;
    out[i].iterations = hp[i].iterations;
    out[i].evaluations = hp[i].evaluations;
    out[i].status = empty ? DGS_ERR_NO_SOURCE : DGS_OK;
    out[i].score = hp[i].mse;
    out[i].fitness = NAN;
    evals += hp[i].evaluations;
    h->icp_last_iters[i] = hp[i].iterations;
  }
  h->last_evaluations = evals;
  return DGS_OK;
}

int icp_align(dgs_handle* h, const float* guess16, dgs_result* out) {
  CloudState* one[1] = {h->src};
  return icp_align_batch(h, 1, one, guess16, out);
}

// device pointer and stride of the batch's final transforms (column-major float[16] per pair) for the fitness kernel
const float* icp_final_transforms(dgs_handle* h, size_t* stride_bytes) {
  *stride_bytes = sizeof(IcpPair);
  return reinterpret_cast<const float*>(reinterpret_cast<const char*>(h->ipairs.ptr) + offsetof(IcpPair, final_T));
}

int icp_trajectory(dgs_handle* h, int pair, float* T16s, double* mse, int32_t* n_corr, int capacity, int* len) {
  int m;
  size_t e;
  int rc = traj_window(h->icp_last_iters, h->icp_traj_cap, pair, capacity, len, &m, &e);
  if (rc || m == 0) return rc;
  DGS_HIP_TRY(h, hipStreamSynchronize(h->stream));
  if (T16s) DGS_HIP_TRY(h, hipMemcpy(T16s, h->icp_traj_T.ptr + e * 16, (size_t)m * 16 * sizeof(float), hipMemcpyDeviceToHost));
  if (mse) DGS_HIP_TRY(h, hipMemcpy(mse, h->icp_traj_mse.ptr + e, (size_t)m * sizeof(double), hipMemcpyDeviceToHost));
  if (n_corr) DGS_HIP_TRY(h, hipMemcpy(n_corr, h->icp_traj_n.ptr + e, (size_t)m * sizeof(int), hipMemcpyDeviceToHost));
  return DGS_OK;
}

void icp_release(dgs_handle* h) {
  h->ipairs.release(); h->iitems.release(); h->icp_w.release(); h->icp_origin.release();
  h->icp_traj_T.release(); h->icp_traj_mse.release(); h->icp_traj_n.release();
  for (auto& b : h->icp_w_bvh) b.release();
  h->icp_w_bvh.clear();
}

}  // namespace dgs
