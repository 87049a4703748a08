// LineBasedScanmatcher::line_extraction (upstream src/hdl_graph_slam/line_based_scanmatcher.cpp:299-457) on the device: while at
// least min_cluster_size points remain, a RANSAC line fit (pcl::SACSegmentation, SACMODEL_LINE, optimised coefficients), a Euclidean
// clustering of the inliers, the statistics of the biggest cluster and its removal.
//
// MI355X design, one round over the n remaining points
//   * The RANSAC is sac.h's, shared with the floor detection, over LnModel (the line's sample test, point and unit direction, inlier
//     test).  The draw stream does not depend on any count, so the host builds the round's draw list from n alone (the generator
//     restarts every round) and uploads it; sac_prepare_kernel<LnModel> turns it into hypotheses and sac_score_kernel<LnModel, 512>
//     scores every hypothesis against every point in one launch.
//   * ln_walk_kernel replays RandomSampleConsensus::computeModel's sequential walk (SacWalk) over the (count, draw) records: the winner
//     is the sequential loop's winner.
//   * Inliers, cluster members and the removal are keep flags and the shared stable compaction (compact.h: pf_count_kernel,
//     pf_scan_kernel, pf_scatter_kernel); ln_scatter_index_kernel is the scatter that also writes a point's position.
//   * The refit and the statistics keep upstream's sequential sums: a workgroup stages 256 terms at a time in LDS, one lane adds them
//     in order.  Everything that is order-independent (minimum, maximum, first extreme projection) is a reduction.
//   * Clustering: the inliers lie within the threshold of a line, so they are sorted by their projection on it and every inlier tests
//     the exact 3-D distance to the ones that follow inside a window of the tolerance plus a rounding margin; linked pairs are united
//     in a lock-free union-find whose root is the lowest sorted position.  Exact components for any tolerance.
//   * One host wait per round: the round record and the three counts come back together.  Launches that depend on the inlier count
//     are shaped for n and read the count on the device.
// Semantics and the PCL 1.10 details recalled from upstream: DESIGN.md §6e.
#include <algorithm>
#include <cfloat>
#include <climits>
#include <cmath>
#include <cstring>

#include <hipcub/hipcub.hpp>

#include "compact.h"
#include "eigen33.h"
#include "handle.h"
#include "nn_group.h"
#include "sac.h"

namespace dgs {

constexpr int kLnHypChunk = 512;         // hypotheses per workgroup of sac_score_kernel (blockIdx.y)
constexpr int kLnBadRun = 1000;          // SampleConsensusModel::max_sample_checks_
constexpr int kLnPickBlock = 1024;       // ln_pick_kernel: one workgroup

struct LnHyp {
  float p0[3];
  float dir[3];
  int draw, i0, i1;
  int pad[3];
};

struct LnRound {
  int status, draws, iterations, i0, i1;
  int n_inliers, n_cluster, chosen, emitted, pad;
  float p0[3], dir[3];       // the winner's sample model
  double line[2], d[2];      // the model the statistics use: (x, y) of point and direction, the direction renormalised in double
  double A[3], B[3], mean, sigma, maxe, mine;
};

// (line_pt - p).cross3(line_dir).squaredNorm() < threshold^2, the norm's terms associated as `order` says (the fourth term is 0)
__device__ __forceinline__ bool ln_is_inlier(const float4 p, const float p0x, const float p0y, const float p0z, const float dx, const float dy,
                                             const float dz, const int order, const double thr2) {
  const float ax = sub_rn(p0x, p.x), ay = sub_rn(p0y, p.y), az = sub_rn(p0z, p.z);
  const float cx = sub_rn(mul_rn(ay, dz), mul_rn(az, dy));
  const float cy = sub_rn(mul_rn(az, dx), mul_rn(ax, dz));
  const float cz = sub_rn(mul_rn(ax, dy), mul_rn(ay, dx));
  const float xx = mul_rn(cx, cx), yy = mul_rn(cy, cy), zz = mul_rn(cz, cz);
  const float sq = order == DGS_PF_NORM_PAIRS_XY_ZW   ? add_rn(add_rn(xx, yy), add_rn(zz, 0.f))
                   : order == DGS_PF_NORM_PAIRS_XZ_YW ? add_rn(add_rn(xx, zz), add_rn(yy, 0.f))
                                                      : add_rn(add_rn(add_rn(xx, yy), zz), 0.f);
  return (double)sq < thr2;
}

// ================================================================================================ hypotheses
// pcl::SampleConsensusModelLine for sac.h's kernels: isSampleGood, computeModelCoefficients and the countWithinDistance predicate
struct LnModel {
  static constexpr int kSample = 2;
  using Hyp = LnHyp;
  struct Params {
    int any_axis, order;   // sample_good_any_axis, sqnorm_order
    double thr2;           // sac_distance_threshold squared
  };
  struct Coef {
    float p0x, p0y, p0z, dx, dy, dz;
  };
  static __device__ __forceinline__ int bad_run(const Params&) { return kLnBadRun; }
  static __device__ __forceinline__ bool good(const Params& prm, const float4 (&p)[2]) {
    const float4 a = p[0], b = p[1];
    return prm.any_axis ? (a.x != b.x || a.y != b.y || a.z != b.z) : (a.x != b.x && a.y != b.y && a.z != b.z);
  }
  static __device__ __forceinline__ LnHyp make(const Params&, const float4 (&p)[2], const int d, const int (&idx)[2]) {
    const float4 a = p[0], b = p[1];
    LnHyp hy;
    hy.p0[0] = a.x; hy.p0[1] = a.y; hy.p0[2] = a.z;
    // model_coefficients.tail<3>() = p1 - p0, normalize(): divided by sqrt(squaredNorm) when that is > 0
    float ux = sub_rn(b.x, a.x), uy = sub_rn(b.y, a.y), uz = sub_rn(b.z, a.z);
    const float n2 = add_rn(add_rn(mul_rn(ux, ux), mul_rn(uy, uy)), mul_rn(uz, uz));
    if (n2 > 0.f) {
      const float s = sqrtf(n2);
      ux = ux / s; uy = uy / s; uz = uz / s;
    }
    hy.dir[0] = ux; hy.dir[1] = uy; hy.dir[2] = uz;
    hy.draw = d; hy.i0 = idx[0]; hy.i1 = idx[1];
    hy.pad[0] = hy.pad[1] = hy.pad[2] = 0;
    return hy;
  }
  static __device__ __forceinline__ Coef coef(const LnHyp* hy) { return {hy->p0[0], hy->p0[1], hy->p0[2], hy->dir[0], hy->dir[1], hy->dir[2]}; }
  static __device__ __forceinline__ bool inlier(const Params& prm, const float4 p, const Coef& c) {
    return ln_is_inlier(p, c.p0x, c.p0y, c.p0z, c.dx, c.dy, c.dz, prm.order, prm.thr2);
  }
  // computeModel's w^2 for SacWalk::step, which runs on the device
  static __device__ __forceinline__ double ratio_power(const double w) {
#pragma clang fp contract(off)
    return w * w;
  }
};

// RandomSampleConsensus::computeModel's walk over the counts (one lane)
__global__ void ln_walk_kernel(const LnHyp* __restrict__ hyps, const int* __restrict__ counts, const int* __restrict__ meta, const int n, const int D,
                               const int max_hyp, const int max_iterations, const double log_one_minus_p, LnRound* __restrict__ R) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const int H = min(meta[0], max_hyp), fail_at = meta[1];
  SacWalk wk;
  while (wk.open()) {
    if (wk.it >= H) {
      wk.end_of_list(fail_at, D);
      break;
    }
    if (!wk.next(hyps[wk.it].draw, fail_at)) break;
    if (!wk.step(counts[wk.it], n, max_iterations, log_one_minus_p, LnModel::ratio_power)) break;
  }
  const int win = wk.win;
  const int status = (wk.status == SAC_OK && win < 0) ? SAC_FAILED : wk.status;
  R->status = status;
  R->draws = wk.draws;
  R->iterations = wk.it;
  R->i0 = R->i1 = -1;
  R->n_inliers = R->n_cluster = R->emitted = 0;
  R->chosen = -1;
  for (int a = 0; a < 3; a++) { R->p0[a] = 0.f; R->dir[a] = 0.f; R->A[a] = 0.0; R->B[a] = 0.0; }
  R->line[0] = R->line[1] = R->d[0] = R->d[1] = 0.0;
  R->mean = R->sigma = R->maxe = R->mine = 0.0;
  if (status == SAC_OK) {
    R->i0 = hyps[win].i0;
    R->i1 = hyps[win].i1;
    for (int a = 0; a < 3; a++) { R->p0[a] = hyps[win].p0[a]; R->dir[a] = hyps[win].dir[a]; }
  }
}

// selectWithinDistance of the winner
__global__ __launch_bounds__(kBlock) void ln_flag_kernel(const float4* __restrict__ pts, const int n, const LnRound* __restrict__ R, const int order,
                                                         const double thr2, unsigned char* __restrict__ flags) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  flags[i] = (R->status == SAC_OK && ln_is_inlier(pts[i], R->p0[0], R->p0[1], R->p0[2], R->dir[0], R->dir[1], R->dir[2], order, thr2)) ? 1 : 0;
}

// pf_scatter_kernel that writes the point's position into the fourth float
__global__ __launch_bounds__(kBlock) void ln_scatter_index_kernel(const float4* __restrict__ in, const unsigned char* __restrict__ flags, const int n,
                                                                  const int* __restrict__ blk, float4* __restrict__ out) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  int off;
  if (!compact_slot(flags, i, n, blk, &off)) return;
  float4 p = in[i];
  p.w = __int_as_float(i);
  out[off] = p;   // off < number of flagged points <= n: `out` holds n points
}

// ================================================================================================ refit
// SampleConsensusModelLine::optimizeModelCoefficients: compute3DCentroid and computeCovarianceMatrix (sequential float sums in inlier
// order, un-normalised), pcl::eigen33's eigenvalues, computeCorrespondingEigenVector of the largest.  line_extraction then takes x and y
// of point and direction and renormalises the direction in double (:360-364).  Two or fewer inliers keep the sample's model.
__global__ __launch_bounds__(kBlock) void ln_refit_kernel(const float4* __restrict__ inl, const int* __restrict__ cnt, LnRound* __restrict__ R) {
#pragma clang fp contract(off)
  __shared__ float s_x[kBlock], s_y[kBlock], s_z[kBlock];
  __shared__ float s_c[3];
  const int m = cnt[0];
  float px = R->p0[0], py = R->p0[1], vx = R->dir[0], vy = R->dir[1];
  if (m > 2 && R->status == SAC_OK) {
    float cx = 0.f, cy = 0.f, cz = 0.f;
    for (int base = 0; base < m; base += kBlock) {
      const int j = base + threadIdx.x;
      if (j < m) {
        const float4 p = inl[j];
        s_x[threadIdx.x] = p.x; s_y[threadIdx.x] = p.y; s_z[threadIdx.x] = p.z;
      }
      __syncthreads();
      if (threadIdx.x == 0) {
        const int e = min(kBlock, m - base);
        for (int t = 0; t < e; t++) { cx += s_x[t]; cy += s_y[t]; cz += s_z[t]; }
      }
      __syncthreads();
    }
    if (threadIdx.x == 0) {
      const float fm = (float)m;
      s_c[0] = cx / fm; s_c[1] = cy / fm; s_c[2] = cz / fm;
    }
    __syncthreads();
    cx = s_c[0]; cy = s_c[1]; cz = s_c[2];
    float xx = 0.f, xy = 0.f, xz = 0.f, yy = 0.f, yz = 0.f, zz = 0.f;
    for (int base = 0; base < m; base += kBlock) {
      const int j = base + threadIdx.x;
      if (j < m) {
        const float4 p = inl[j];
        s_x[threadIdx.x] = p.x - cx; s_y[threadIdx.x] = p.y - cy; s_z[threadIdx.x] = p.z - cz;
      }
      __syncthreads();
      if (threadIdx.x == 0) {
        const int e = min(kBlock, m - base);
        for (int t = 0; t < e; t++) {
          const float x = s_x[t], y = s_y[t], z = s_z[t];
          yy += y * y; yz += y * z; zz += z * z;
          xx += x * x; xy += x * y; xz += x * z;
        }
      }
      __syncthreads();
    }
    if (threadIdx.x == 0) {
      const float cov[9] = {xx, xy, xz, xy, yy, yz, xz, yz, zz};
      float scale = 0.f;
      for (int a = 0; a < 9; a++) scale = fmaxf(scale, fabsf(cov[a]));
      if (scale <= FLT_MIN) scale = 1.f;
      float sm[9], r[3], ev[3];
      for (int a = 0; a < 9; a++) sm[a] = cov[a] / scale;
      pf_compute_roots(sm, r);
      const float largest = r[2] * scale;          // eigen33(mat, evals): evals = roots * scale
      const float shift = largest / scale;         // computeCorrespondingEigenVector: scaledMat.diagonal() -= eigenvalue / scale
      sm[0] -= shift; sm[4] -= shift; sm[8] -= shift;
      pf_eigen33_vector(sm, ev);
      px = cx; py = cy; vx = ev[0]; vy = ev[1];
    }
  }
  if (threadIdx.x == 0) {
    R->n_inliers = m;
    double dx = (double)vx, dy = (double)vy;
    const double z = dx * dx + dy * dy;
    if (z > 0.0) {
      const double s = sqrt(z);
      dx = dx / s; dy = dy / s;
    }
    R->line[0] = (double)px; R->line[1] = (double)py;
    R->d[0] = dx; R->d[1] = dy;
  }
}

// ================================================================================================ clustering
__device__ __forceinline__ uint32_t ln_float_key(float f) {
  const uint32_t b = __float_as_uint(f);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

// one lane per slot of an n-sized array: the first cnt[0] slots are inliers (key = projection on the sample's line), the rest sort last
__global__ __launch_bounds__(kBlock) void ln_key_kernel(const float4* __restrict__ inl, const int* __restrict__ cnt, const int n,
                                                        const LnRound* __restrict__ R, uint32_t* __restrict__ keys, uint32_t* __restrict__ vals,
                                                        int* __restrict__ parent, int* __restrict__ csize, int* __restrict__ cminpos,
                                                        unsigned char* __restrict__ cflags) {
  const int j = blockIdx.x * kBlock + threadIdx.x;
  if (j >= n) return;
  uint32_t key = 0xFFFFFFFFu;
  if (j < cnt[0]) {
    const float4 p = inl[j];
    const float t = (p.x - R->p0[0]) * R->dir[0] + (p.y - R->p0[1]) * R->dir[1] + (p.z - R->p0[2]) * R->dir[2];
    key = min(ln_float_key(t), 0xFFFFFFFEu);
  }
  keys[j] = key;
  vals[j] = (uint32_t)j;
  parent[j] = j;
  csize[j] = 0;
  cminpos[j] = INT_MAX;
  cflags[j] = 0;
}

__global__ __launch_bounds__(kBlock) void ln_gather_kernel(const float4* __restrict__ inl, const int* __restrict__ cnt, const uint32_t* __restrict__ vals,
                                                           const LnRound* __restrict__ R, float4* __restrict__ sorted, float* __restrict__ sproj) {
  const int q = blockIdx.x * kBlock + threadIdx.x;
  const int m = cnt[0];
  if (q >= m) return;
  const uint32_t j = vals[q];
  if (j >= (uint32_t)m) return;   // cannot happen: the first m sorted slots are the m inliers
  const float4 p = inl[j];
  sorted[q] = p;
  sproj[q] = (p.x - R->p0[0]) * R->dir[0] + (p.y - R->p0[1]) * R->dir[1] + (p.z - R->p0[2]) * R->dir[2];
}

__device__ __forceinline__ int ln_find(int* parent, int x) {
  int p = __hip_atomic_load(&parent[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  while (p != x) {
    x = p;
    p = __hip_atomic_load(&parent[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  return x;
}

// A projection on a unit direction never grows a distance, so two inliers farther apart along the line than the tolerance (plus the
// rounding of the float projections) cannot be linked: every later inlier inside that window gets the exact test of pf_radius_kernel.
__global__ __launch_bounds__(kBlock) void ln_link_kernel(const float4* __restrict__ sorted, const float* __restrict__ sproj, const int* __restrict__ cnt,
                                                         const float tol, const double tol2, const int inclusive, int* __restrict__ parent) {
  const int q = blockIdx.x * kBlock + threadIdx.x;
  const int m = cnt[0];
  if (q >= m) return;
  const float tmax = fmaxf(fabsf(sproj[0]), fabsf(sproj[m - 1]));
  const float window = tol * 1.0001f + 2e-5f * tmax + 1e-6f;
  const float4 p = sorted[q];
  const float tq = sproj[q];
  for (int r = q + 1; r < m; r++) {
    if (sproj[r] - tq > window) break;
    const float4 o = sorted[r];
    const double d2 = (double)sqdist_rn(p.x, p.y, p.z, o.x, o.y, o.z);
    if (!(inclusive ? d2 <= tol2 : d2 < tol2)) continue;
    int a = q, b = r;
    for (;;) {   // unite: the higher root points at the lower one
      a = ln_find(parent, a);
      b = ln_find(parent, b);
      if (a == b) break;
      if (a > b) { const int t = a; a = b; b = t; }
      if (atomicCAS(&parent[b], b, a) == b) break;
    }
  }
}

__global__ __launch_bounds__(kBlock) void ln_component_kernel(const float4* __restrict__ sorted, const int* __restrict__ cnt, int* __restrict__ parent,
                                                              int* __restrict__ label, int* __restrict__ csize, int* __restrict__ cminpos) {
  const int q = blockIdx.x * kBlock + threadIdx.x;
  if (q >= cnt[0]) return;
  const int root = ln_find(parent, q);
  label[q] = root;
  atomicAdd(&csize[root], 1);
  atomicMin(&cminpos[root], __float_as_int(sorted[q].w));
}

// the biggest component of at most max_cluster members; ties to the one that holds the lowest position (one workgroup)
__global__ __launch_bounds__(kLnPickBlock) void ln_pick_kernel(const int* __restrict__ label, const int* __restrict__ csize, const int* __restrict__ cminpos,
                                                              const int* __restrict__ cnt, const int max_cluster, LnRound* __restrict__ R) {
  __shared__ unsigned long long s_best;
  if (threadIdx.x == 0) s_best = 0ull;
  __syncthreads();
  const int m = cnt[0];
  unsigned long long best = 0ull;
  for (int q = threadIdx.x; q < m; q += kLnPickBlock) {
    if (label[q] != q) continue;
    const int sz = csize[q];
    if (sz < 1 || sz > max_cluster) continue;
    const unsigned long long key = ((unsigned long long)(unsigned)sz << 32) | (unsigned)(INT_MAX - cminpos[q]);
    best = best > key ? best : key;
  }
  if (best) atomicMax(&s_best, best);
  __syncthreads();
  const unsigned long long top = s_best;
  if (threadIdx.x == 0 && top == 0ull) R->chosen = -1;
  if (top == 0ull) return;
  for (int q = threadIdx.x; q < m; q += kLnPickBlock) {
    if (label[q] != q) continue;
    const int sz = csize[q];
    if (sz < 1 || sz > max_cluster) continue;
    if ((((unsigned long long)(unsigned)sz << 32) | (unsigned)(INT_MAX - cminpos[q])) == top) R->chosen = q;   // one root has this key
  }
}

__global__ __launch_bounds__(kBlock) void ln_cluster_flag_kernel(const float4* __restrict__ sorted, const int* __restrict__ label, const int* __restrict__ cnt,
                                                                 const int n, const LnRound* __restrict__ R, unsigned char* __restrict__ cflags) {
  const int q = blockIdx.x * kBlock + threadIdx.x;
  if (q >= cnt[0]) return;
  const int pos = __float_as_int(sorted[q].w);
  if (label[q] == R->chosen && pos >= 0 && pos < n) cflags[pos] = 1;
}

// ================================================================================================ statistics
// :383-442.  d = point_to_line_distance (the direction normalised once more, :771), mean and sigma as upstream's sequential double sums,
// max from 0 and min from 100000, A / B the first member with the strictly smallest / largest projection.
struct LnStat {
  double d, t, v[3];
};

__device__ __forceinline__ LnStat ln_stat_point(const float4 p, const double lx, const double ly, const double dx, const double dy) {
#pragma clang fp contract(off)
  LnStat s;
  const double x = (double)p.x, y = (double)p.y, z = (double)p.z;
  // point_to_line_distance
  double nx = dx, ny = dy;
  const double n2 = (nx * nx + ny * ny) + 0.0 * 0.0;
  if (n2 > 0.0) {
    const double nn = sqrt(n2);
    nx = nx / nn; ny = ny / nn;
  }
  const double tn = ((x - lx) * nx + (y - ly) * ny) + (z - 0.0) * 0.0;
  const double qx = lx + nx * tn, qy = ly + ny * tn, qz = 0.0 + 0.0 * tn;
  const double ex = x - qx, ey = y - qy, ez = z - qz;
  s.d = sqrt((ex * ex + ey * ey) + ez * ez);
  // vt = vt_line + vt_direction * ((vt - vt_line).dot(vt_direction)); its own projection (vt - vt_line).dot(vt_direction)
  const double t0 = ((x - lx) * dx + (y - ly) * dy) + (z - 0.0) * 0.0;
  s.v[0] = lx + dx * t0; s.v[1] = ly + dy * t0; s.v[2] = 0.0 + 0.0 * t0;
  s.t = ((s.v[0] - lx) * dx + (s.v[1] - ly) * dy) + (s.v[2] - 0.0) * 0.0;
  return s;
}

__global__ __launch_bounds__(kBlock) void ln_stats_kernel(const float4* __restrict__ clu, const int* __restrict__ cnt, const int min_cluster,
                                                          const double merror, const double min_length, LnRound* __restrict__ R) {
#pragma clang fp contract(off)
  __shared__ double s_d[kBlock];
  __shared__ double s_mean;
  __shared__ double s_lo[kBlock], s_hi[kBlock], s_mn[kBlock], s_mx[kBlock];
  __shared__ int s_ilo[kBlock], s_ihi[kBlock];
  const int c = cnt[1];
  if (threadIdx.x == 0) R->n_cluster = c;
  if (c < min_cluster || c < 1) return;
  const double lx = R->line[0], ly = R->line[1], dx = R->d[0], dy = R->d[1];
  double sum = 0.0;
  double lo = 0.0, hi = 0.0, mn = 100000.0, mx = 0.0;
  int ilo = INT_MAX, ihi = INT_MAX;
  for (int base = 0; base < c; base += kBlock) {
    const int j = base + threadIdx.x;
    if (j < c) {
      const LnStat s = ln_stat_point(clu[j], lx, ly, dx, dy);
      s_d[threadIdx.x] = s.d;
      if (s.d > mx) mx = s.d;
      if (s.d < mn) mn = s.d;
      if (ilo == INT_MAX || s.t < lo) { lo = s.t; ilo = j; }   // j ascends per lane: the first of equal values stays
      if (ihi == INT_MAX || s.t > hi) { hi = s.t; ihi = j; }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      const int e = min(kBlock, c - base);
      for (int t = 0; t < e; t++) sum += s_d[t];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) s_mean = sum / (double)c;
  s_lo[threadIdx.x] = lo; s_hi[threadIdx.x] = hi; s_mn[threadIdx.x] = mn; s_mx[threadIdx.x] = mx;
  s_ilo[threadIdx.x] = ilo; s_ihi[threadIdx.x] = ihi;
  __syncthreads();
  const double mean = s_mean;
  double sig = 0.0;
  for (int base = 0; base < c; base += kBlock) {
    const int j = base + threadIdx.x;
    if (j < c) {
      const double e = ln_stat_point(clu[j], lx, ly, dx, dy).d - mean;
      s_d[threadIdx.x] = e * e;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      const int e = min(kBlock, c - base);
      for (int t = 0; t < e; t++) sig += s_d[t];
    }
    __syncthreads();
  }
  if (threadIdx.x != 0) return;
  for (int t = 1; t < kBlock; t++) {
    if (s_ilo[t] != INT_MAX && (s_lo[t] < lo || (s_lo[t] == lo && s_ilo[t] < ilo))) { lo = s_lo[t]; ilo = s_ilo[t]; }
    if (s_ihi[t] != INT_MAX && (s_hi[t] > hi || (s_hi[t] == hi && s_ihi[t] < ihi))) { hi = s_hi[t]; ihi = s_ihi[t]; }
    if (s_mn[t] < mn) mn = s_mn[t];
    if (s_mx[t] > mx) mx = s_mx[t];
  }
  const LnStat a = ln_stat_point(clu[ilo], lx, ly, dx, dy), b = ln_stat_point(clu[ihi], lx, ly, dx, dy);   // ilo, ihi < c
  for (int k = 0; k < 3; k++) { R->A[k] = a.v[k]; R->B[k] = b.v[k]; }
  R->mean = mean;
  R->sigma = sqrt(sig / (double)c);
  R->maxe = mx;
  R->mine = mn;
  const double ux = a.v[0] - b.v[0], uy = a.v[1] - b.v[1], uz = a.v[2] - b.v[2];
  const double len = sqrt((ux * ux + uy * uy) + uz * uz);
  R->emitted = (mean < merror && len > min_length) ? 1 : 0;
}

// extract.setNegative(true): everything but the cluster stays, in order
__global__ __launch_bounds__(kBlock) void ln_keep_kernel(const unsigned char* __restrict__ cflags, const int n, unsigned char* __restrict__ flags) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  flags[i] = cflags[i] ? 0 : 1;
}

// ================================================================================================ host side
namespace {

struct LnBack {   // what comes back once per round
  LnRound r;
  int cnt[4];
};
constexpr size_t kLnDrawOffset = 4096;   // the draw list sits behind the read-back block in the pinned staging
static_assert(sizeof(LnBack) <= kLnDrawOffset, "the read-back block must fit in front of the draw list");

// count + scan + scatter of `flags` over n points; the total lands in cnt[slot]
template <class Scatter>
void ln_compact(dgs_handle* h, int64_t n, const unsigned char* flags, int slot, Scatter scatter) {
  LnScratch& ln = h->ln;
  compact_offsets(h->stream, flags, n, ln.blk.ptr, ln.cnt.ptr + slot);
  scatter(compact_blocks(n));
  ln.counts4[0] += 3;
}

int ln_reserve(dgs_handle* h, int64_t n, int max_hyp) {
  LnScratch& ln = h->ln;
  const size_t m = (size_t)std::max<int64_t>(n, 1);
  for (DevBuf<float4>* b : {&ln.a, &ln.b, &ln.inl, &ln.clu, &ln.sorted}) DGS_HIP_TRY(h, b->reserve(m));
  DGS_HIP_TRY(h, ln.flags.reserve(m));
  DGS_HIP_TRY(h, ln.cflags.reserve(m));
  DGS_HIP_TRY(h, ln.blk.reserve(compact_blocks(m)));
  DGS_HIP_TRY(h, ln.cnt.reserve(4));
  DGS_HIP_TRY(h, ln.hyps.reserve((size_t)max_hyp));
  DGS_HIP_TRY(h, ln.sac.counts.reserve((size_t)max_hyp));
  DGS_HIP_TRY(h, ln.sac.meta.reserve(4));
  DGS_HIP_TRY(h, ln.round.reserve(1));
  for (DevBuf<uint32_t>* b : {&ln.keys, &ln.keys_alt, &ln.vals, &ln.vals_alt}) DGS_HIP_TRY(h, b->reserve(m));
  DGS_HIP_TRY(h, ln.sproj.reserve(m));
  for (DevBuf<int>* b : {&ln.parent, &ln.csize, &ln.cminpos}) DGS_HIP_TRY(h, b->reserve(m));
  return DGS_OK;
}

// one round over `cur` (n points): everything up to the removal into `next`; the record and the counts are in the pinned block after
// the wait.  label[] of the components reuses keys (the sort's input is dead by then).
int ln_round(dgs_handle* h, const dgs_line_extraction_params& p, const float4* cur, float4* next, int64_t n, const uint32_t* raw, int D, int max_hyp,
             LnBack* back) {
  LnScratch& ln = h->ln;
  SacScratch& sac = ln.sac;
  const unsigned nb = compact_blocks(n);
  const double thr2 = (double)p.sac_distance_threshold * (double)p.sac_distance_threshold;
  const double tol2 = (double)p.cluster_tolerance * (double)p.cluster_tolerance;
  DGS_HIP_TRY(h, sac.draws.reserve((size_t)D * 2));
  if (ensure_pinned(h, kLnDrawOffset + (size_t)D * 2 * sizeof(int)) != DGS_OK) return DGS_ERR_HIP;
  int* hd = reinterpret_cast<int*>(static_cast<char*>(h->pinned) + kLnDrawOffset);
  sac_draws<2>(sac.perm, raw, n, D, hd);
  DGS_HIP_TRY(h, hipMemcpyAsync(sac.draws.ptr, hd, (size_t)D * 2 * sizeof(int), hipMemcpyHostToDevice, h->stream));
  const LnModel::Params prm{p.sample_good_any_axis ? 1 : 0, p.sqnorm_order, thr2};
  hipLaunchKernelGGL(sac_prepare_kernel<LnModel>, dim3(1), dim3(kSacPrepareBlock), 0, h->stream, cur, (int)n, sac.draws.ptr, D, prm, max_hyp,
                     ln.hyps.ptr, sac.counts.ptr, sac.meta.ptr);
  hipLaunchKernelGGL((sac_score_kernel<LnModel, kLnHypChunk>),
                     dim3((unsigned)((n + kSacTile - 1) / kSacTile), (unsigned)((max_hyp + kLnHypChunk - 1) / kLnHypChunk)), dim3(kBlock), 0, h->stream, cur,
                     (int)n, ln.hyps.ptr, sac.meta.ptr, max_hyp, 0, max_hyp, prm, sac.counts.ptr);
  hipLaunchKernelGGL(ln_walk_kernel, dim3(1), dim3(kWave), 0, h->stream, ln.hyps.ptr, sac.counts.ptr, sac.meta.ptr, (int)n, D, max_hyp, p.max_iterations,
                     std::log(1.0 - 0.99), ln.round.ptr);
  hipLaunchKernelGGL(ln_flag_kernel, dim3(nb), dim3(kBlock), 0, h->stream, cur, (int)n, ln.round.ptr, p.sqnorm_order, thr2, ln.flags.ptr);
  ln.counts4[0] += 4;
  ln_compact(h, n, ln.flags.ptr, 0, [&](unsigned b) {
    hipLaunchKernelGGL(ln_scatter_index_kernel, dim3(b), dim3(kBlock), 0, h->stream, cur, ln.flags.ptr, (int)n, ln.blk.ptr, ln.inl.ptr);
  });
  hipLaunchKernelGGL(ln_refit_kernel, dim3(1), dim3(kBlock), 0, h->stream, ln.inl.ptr, ln.cnt.ptr, ln.round.ptr);
  hipLaunchKernelGGL(ln_key_kernel, dim3(nb), dim3(kBlock), 0, h->stream, ln.inl.ptr, ln.cnt.ptr, (int)n, ln.round.ptr, ln.keys.ptr, ln.vals.ptr,
                     ln.parent.ptr, ln.csize.ptr, ln.cminpos.ptr, ln.cflags.ptr);
  size_t tb = 0;
  (void)hipcub::DeviceRadixSort::SortPairs(nullptr, tb, ln.keys.ptr, ln.keys_alt.ptr, ln.vals.ptr, ln.vals_alt.ptr, (int)n, 0, 32, h->stream);
  DGS_HIP_TRY(h, ln.temp.reserve(tb + 16));
  DGS_HIP_TRY(h, hipcub::DeviceRadixSort::SortPairs(ln.temp.ptr, tb, ln.keys.ptr, ln.keys_alt.ptr, ln.vals.ptr, ln.vals_alt.ptr, (int)n, 0, 32, h->stream));
  ln.counts4[3] += 1;
  int* label = reinterpret_cast<int*>(ln.keys.ptr);
  hipLaunchKernelGGL(ln_gather_kernel, dim3(nb), dim3(kBlock), 0, h->stream, ln.inl.ptr, ln.cnt.ptr, ln.vals_alt.ptr, ln.round.ptr, ln.sorted.ptr,
                     ln.sproj.ptr);
  hipLaunchKernelGGL(ln_link_kernel, dim3(nb), dim3(kBlock), 0, h->stream, ln.sorted.ptr, ln.sproj.ptr, ln.cnt.ptr, p.cluster_tolerance, tol2,
                     p.cluster_inclusive ? 1 : 0, ln.parent.ptr);
  hipLaunchKernelGGL(ln_component_kernel, dim3(nb), dim3(kBlock), 0, h->stream, ln.sorted.ptr, ln.cnt.ptr, ln.parent.ptr, label, ln.csize.ptr,
                     ln.cminpos.ptr);
  hipLaunchKernelGGL(ln_pick_kernel, dim3(1), dim3(kLnPickBlock), 0, h->stream, label, ln.csize.ptr, ln.cminpos.ptr, ln.cnt.ptr, p.max_cluster_size,
                     ln.round.ptr);
  hipLaunchKernelGGL(ln_cluster_flag_kernel, dim3(nb), dim3(kBlock), 0, h->stream, ln.sorted.ptr, label, ln.cnt.ptr, (int)n, ln.round.ptr, ln.cflags.ptr);
  ln.counts4[0] += 7;
  ln_compact(h, n, ln.cflags.ptr, 1, [&](unsigned b) {
    hipLaunchKernelGGL(ln_scatter_index_kernel, dim3(b), dim3(kBlock), 0, h->stream, cur, ln.cflags.ptr, (int)n, ln.blk.ptr, ln.clu.ptr);
  });
  hipLaunchKernelGGL(ln_stats_kernel, dim3(1), dim3(kBlock), 0, h->stream, ln.clu.ptr, ln.cnt.ptr, p.min_cluster_size, (double)p.merror_threshold,
                     (double)p.line_length_threshold, ln.round.ptr);
  hipLaunchKernelGGL(ln_keep_kernel, dim3(nb), dim3(kBlock), 0, h->stream, ln.cflags.ptr, (int)n, ln.flags.ptr);
  ln.counts4[0] += 2;
  ln_compact(h, n, ln.flags.ptr, 2, [&](unsigned b) {
    hipLaunchKernelGGL(pf_scatter_kernel, dim3(b), dim3(kBlock), 0, h->stream, cur, ln.flags.ptr, (int)n, ln.blk.ptr, next, 0);
  });
  DGS_HIP_TRY(h, hipGetLastError());
  LnBack* hb = reinterpret_cast<LnBack*>(h->pinned);
  DGS_HIP_TRY(h, hipMemcpyAsync(&hb->r, ln.round.ptr, sizeof(LnRound), hipMemcpyDeviceToHost, h->stream));
  DGS_HIP_TRY(h, hipMemcpyAsync(hb->cnt, ln.cnt.ptr, 3 * sizeof(int), hipMemcpyDeviceToHost, h->stream));
  DGS_HIP_TRY(h, hipStreamSynchronize(h->stream));
  ln.counts4[1] += 1;
  ln.counts4[2] += 1;
  *back = *hb;
  return DGS_OK;
}

// record_lists: the fourth float of the first m points of a list, as positions
int ln_read_list(dgs_handle* h, const float4* list, int m, std::vector<int32_t>* out) {
  out->assign((size_t)m, 0);
  if (m == 0) return DGS_OK;
  std::vector<float4> tmp((size_t)m);
  DGS_HIP_TRY(h, hipMemcpyAsync(tmp.data(), list, (size_t)m * sizeof(float4), hipMemcpyDeviceToHost, h->stream));
  DGS_HIP_TRY(h, hipStreamSynchronize(h->stream));
  h->ln.counts4[1] += 1;
  for (int j = 0; j < m; j++) std::memcpy(&(*out)[j], &tmp[j].w, sizeof(int32_t));
  return DGS_OK;
}

const char* ln_bad_params(const dgs_line_extraction_params* p) {
  if (!p) return "line extraction: params is NULL";
  if (p->struct_size != sizeof(dgs_line_extraction_params)) return "line extraction: wrong struct_size";
  if (p->sac_method_type != 0) return "line extraction: only SAC_RANSAC (sac_method_type 0) is served";
  if (p->sqnorm_order < DGS_PF_NORM_PAIRS_XY_ZW || p->sqnorm_order > DGS_PF_NORM_SEQUENTIAL) return "line extraction: unknown sqnorm_order";
  if (p->max_iterations < 0 || p->max_iterations > (1 << 20)) return "line extraction: max_iterations must lie in 0..1048576";
  if (p->max_rounds < 0) return "line extraction: max_rounds must not be negative";
  return nullptr;
}

int ln_extract(dgs_handle* h, const dgs_line_extraction_params& p, const float* in_xyz16, int64_t n0, int32_t in_on_device, const uint32_t* rng_raw,
               int64_t rng_len, dgs_line_feature* lines, int64_t capacity, int64_t* n_lines, int32_t* status_out) {
  LnScratch& ln = h->ln;
  ln.rounds.clear();
  ln.inlier_lists.clear();
  ln.cluster_lists.clear();
  for (int a = 0; a < 4; a++) ln.counts4[a] = 0;
  int status = DGS_LE_DONE;
  const int max_hyp = p.max_iterations + 1;
  const int64_t min_cluster = p.min_cluster_size;
  int64_t n = n0;
  if (n >= min_cluster && n > 0) {
    if (int rc = ln_reserve(h, n, max_hyp)) return rc;
    DGS_HIP_TRY(h, hipMemcpyAsync(ln.a.ptr, in_xyz16, (size_t)n * sizeof(float4), in_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, h->stream));
    if (!in_on_device) {   // the caller's array may go away after the call: wait for the copy
      DGS_HIP_TRY(h, hipStreamSynchronize(h->stream));
      ln.counts4[1] += 1;
    }
    sac_grow_perm(ln.sac.perm, n);
  }
  float4* cur = ln.a.ptr;
  float4* next = ln.b.ptr;
  const int64_t avail_draws = rng_raw ? rng_len / 2 : INT32_MAX;
  while (n >= min_cluster && n > 0) {
    if ((int64_t)ln.rounds.size() >= p.max_rounds) { status = DGS_LE_MAX_ROUNDS; break; }
    dgs_line_extraction_round rec{};
    rec.n_before = (int32_t)n;
    rec.sample0 = rec.sample1 = -1;
    if (n < 2) {   // no two points to draw
      status = DGS_LE_RANSAC_FAILED;
      ln.rounds.push_back(rec);
      break;
    }
    SacDrawPlan plan(avail_draws, max_hyp, kLnBadRun);
    LnBack back{};
    bool exhausted = false;
    for (;;) {
      if (plan.empty()) { exhausted = true; break; }
      const uint32_t* raw = rng_raw;
      if (!rng_raw) {   // every round restarts the generator at the seed
        sac_grow_mt(ln.sac.mt_raw, 2 * plan.D);
        raw = ln.sac.mt_raw.data();
      }
      if (int rc = ln_round(h, p, cur, next, n, raw, (int)plan.D, max_hyp, &back)) return rc;
      if (back.r.status != SAC_NEED_DRAWS) break;
      if (!plan.grow()) { exhausted = true; break; }
    }
    if (exhausted) {
      status = DGS_LE_RNG_EXHAUSTED;
      rec.draws = (int32_t)std::max<int64_t>(plan.D, 0);
      rec.iterations = back.r.iterations;
      ln.rounds.push_back(rec);
      break;
    }
    rec.draws = back.r.draws;
    rec.iterations = back.r.iterations;
    if (back.r.status == SAC_FAILED) {
      status = DGS_LE_RANSAC_FAILED;
      ln.rounds.push_back(rec);
      break;
    }
    rec.sample0 = back.r.i0;
    rec.sample1 = back.r.i1;
    rec.inliers = back.cnt[0];
    rec.cluster = back.cnt[1];
    rec.emitted = (rec.cluster >= min_cluster && rec.cluster >= 1) ? back.r.emitted : 0;
    ln.rounds.push_back(rec);
    if (p.record_lists) {
      ln.inlier_lists.emplace_back();
      ln.cluster_lists.emplace_back();
      if (int rc = ln_read_list(h, ln.inl.ptr, rec.inliers, &ln.inlier_lists.back())) return rc;
      if (int rc = ln_read_list(h, ln.clu.ptr, rec.cluster, &ln.cluster_lists.back())) return rc;
    }
    if (rec.cluster < 1) { status = DGS_LE_STALL; break; }
    if (rec.emitted) {
      if (*n_lines >= capacity) {
        h->err = "line extraction: more lines than the output holds";
        return DGS_ERR_INVALID_ARGUMENT;
      }
      dgs_line_feature& f = lines[*n_lines];
      for (int a = 0; a < 3; a++) { f.point_a[a] = back.r.A[a]; f.point_b[a] = back.r.B[a]; }
      f.mean_error = back.r.mean;
      f.std_sigma = back.r.sigma;
      f.max_error = back.r.maxe;
      f.min_error = back.r.mine;
      ++*n_lines;
    }
    std::swap(cur, next);
    n = back.cnt[2];
  }
  if (status_out) *status_out = status;
  return DGS_OK;
}

}  // namespace

void line_extraction_release(dgs_handle* h) {
  LnScratch& ln = h->ln;
  for (DevBuf<float4>* b : {&ln.a, &ln.b, &ln.inl, &ln.clu, &ln.sorted}) b->release();
  ln.flags.release(); ln.cflags.release(); ln.blk.release(); ln.cnt.release(); ln.sac.release(); ln.hyps.release();
  ln.round.release(); ln.keys.release(); ln.keys_alt.release(); ln.vals.release(); ln.vals_alt.release(); ln.sproj.release();
  ln.parent.release(); ln.csize.release(); ln.cminpos.release(); ln.temp.release();
  ln.rounds.clear(); ln.inlier_lists.clear(); ln.cluster_lists.clear();
}

}  // namespace dgs

using namespace dgs;

extern "C" {

int dgs_line_extraction_params_init(dgs_line_extraction_params* p) {
  if (!p) return DGS_ERR_INVALID_ARGUMENT;
  std::memset(p, 0, sizeof(*p));
  p->struct_size = sizeof(*p);
  p->min_cluster_size = 25;
  p->max_cluster_size = 25000;
  p->cluster_tolerance = 1.0f;
  p->sac_distance_threshold = 0.1f;
  p->max_iterations = 500;
  p->merror_threshold = 150.f;
  p->line_length_threshold = 1.0f;
  p->sac_method_type = 0;
  p->sample_good_any_axis = 1;
  p->sqnorm_order = DGS_PF_NORM_PAIRS_XY_ZW;
  p->cluster_inclusive = 1;
  p->max_rounds = 4096;
  p->record_lists = 0;
  return DGS_OK;
}

int dgs_line_extraction(dgs_handle* h, const dgs_line_extraction_params* params, const float* in_xyz16, int64_t n, int32_t in_on_device,
                        const uint32_t* rng_raw, int64_t rng_len, dgs_line_feature* lines, int64_t capacity, int64_t* n_lines, int32_t* status_out) {
  if (const char* why = ln_bad_params(params)) {   // before anything touches a device
    if (h) h->err = why;
    return DGS_ERR_INVALID_ARGUMENT;
  }
  if (!h || !n_lines || n < 0 || n > INT32_MAX || (n > 0 && !in_xyz16) || capacity < 0 || (capacity > 0 && !lines) || rng_len < 0 ||
      (rng_len > 0 && !rng_raw))
    return DGS_ERR_INVALID_ARGUMENT;
  *n_lines = 0;
  if (status_out) *status_out = DGS_LE_DONE;
  h->err.clear();
  DGS_HIP_TRY(h, hipSetDevice(h->device));
  const int rc = ln_extract(h, *params, in_xyz16, n, in_on_device, rng_len > 0 ? rng_raw : nullptr, rng_len, lines, capacity, n_lines, status_out);
  if (rc != DGS_OK) (void)hipStreamSynchronize(h->stream);
  return rc;
}

int dgs_line_extraction_get_rounds(dgs_handle* h, dgs_line_extraction_round* rounds, int64_t capacity, int64_t* n_rounds, int32_t list_round,
                                   int32_t* inlier_idx, int32_t* cluster_idx, int64_t* counts4) {
  if (!h || !n_rounds || capacity < 0) return DGS_ERR_INVALID_ARGUMENT;
  const LnScratch& ln = h->ln;
  *n_rounds = (int64_t)ln.rounds.size();
  if (rounds)
    for (int64_t r = 0; r < std::min<int64_t>(capacity, *n_rounds); r++) rounds[r] = ln.rounds[(size_t)r];
  if (counts4)
    for (int a = 0; a < 4; a++) counts4[a] = ln.counts4[a];
  if (inlier_idx || cluster_idx) {
    if (list_round < 0 || (size_t)list_round >= ln.inlier_lists.size()) {
      h->err = "line extraction: no index lists for that round (record_lists off, or the round failed)";
      return DGS_ERR_INVALID_ARGUMENT;
    }
    const std::vector<int32_t>&il = ln.inlier_lists[(size_t)list_round], &cl = ln.cluster_lists[(size_t)list_round];
    if (inlier_idx && !il.empty()) std::memcpy(inlier_idx, il.data(), il.size() * sizeof(int32_t));
    if (cluster_idx && !cl.empty()) std::memcpy(cluster_idx, cl.data(), cl.size() * sizeof(int32_t));
  }
  return DGS_OK;
}

}  // extern "C"
