// The prefilter's per-point passes as __device__ bodies: the raw-scan head, the predicates, the k-NN passes.  Two kernels call each of
// them: the single-scan kernel of prefilter.hip, whose workgroup `blk` is blockIdx.x, and the segment-table kernel of
// prefilter_batch.hip, where a workgroup first finds its scan and `blk` is its number inside that scan -- the same body, the same local
// index, the same arguments, so a scan of a batch gets the bits of the single call.  (The pattern of knn_leaf.h and gicp_cov_body.h.)
#pragma once
#include <cfloat>
#include <cmath>
#include <cstring>

#include "eigen33.h"
#include "handle.h"
#include "nn_group.h"

namespace dgs {

constexpr int kPfNormalK = 10;             // normal_filtering: ne.setKSearch(10) (:227)
constexpr float kPfNormalThresh = 0.2f;    // normal_filter_thresh (:235)
constexpr int kPfStatsBlock = 1024;        // pf_sor_stats_body: one workgroup

// ================================================================================================ predicates
// distance_filter: d = p.getVector3fMap().norm() in float, (x*x + y*y) + z*z without FMA; kept iff d > near && d < far in double.
// A non-finite point gives a NaN or infinite d and fails one of the two comparisons.
__device__ __forceinline__ void pf_distance_body(const float4* __restrict__ in, const int n, const double near_t, const double far_t,
                                                 unsigned char* __restrict__ flags, const int blk) {
  const int i = blk * kBlock + threadIdx.x;
  if (i >= n) return;
  const float4 p = in[i];
  const float d = sqrtf(add_rn(add_rn(mul_rn(p.x, p.x), mul_rn(p.y, p.y)), mul_rn(p.z, p.z)));
  const double dd = (double)d;
  flags[i] = (dd > near_t && dd < far_t) ? 1 : 0;
}

// height_filtering: kept iff cloud->at(i).z > lidar_position.z(), compared in double
__device__ __forceinline__ void pf_height_body(const float4* __restrict__ in, const int n, const double lz, unsigned char* __restrict__ flags, const int blk) {
  const int i = blk * kBlock + threadIdx.x;
  if (i >= n) return;
  flags[i] = ((double)in[i].z > lz) ? 1 : 0;
}

// ================================================================================================ raw-scan head
// What the head does to a point; by value in the kernel arguments, or a record of the batch's head table.
struct PfHead {
  int deskew;          // an angular velocity was given (the IMU queue was not empty, :295-297)
  int transform;       // a base_link transform was given (:123)
  int norm_order;      // dgs_prefilter_scan_params::deskew_norm_order
  int sets_w;          // dgs_prefilter_scan_params::transform_sets_w
  float ang_v[3];      // (float)angular_velocity * -1.0f (:330-331)
  double scan_period;  // :340
  double m[12];        // rows 0..2 of the 4 x 4 double matrix (:146)
};

// deskewing (:345-350) then pcl::transformPointCloud (:146) of point i of n.  Float where upstream is float, double where it is double,
// operation for operation, no contraction.  DESIGN.md 6c restates every line.
__device__ __forceinline__ float4 pf_head_point(float4 p, const long long i, const long long n, const PfHead& hd) {
#pragma clang fp contract(off)
  if (hd.deskew) {
    // double delta_t = scan_period * static_cast<double>(i) / cloud->size();
    const double half_t = hd.scan_period * (double)i / (double)n / 2.0;
    // Eigen::Quaternionf delta_q(1, delta_t / 2.0 * ang_v[0], ...): the double products narrowed to float
    const float qw = 1.0f;
    const float qx = (float)(half_t * (double)hd.ang_v[0]);
    const float qy = (float)(half_t * (double)hd.ang_v[1]);
    const float qz = (float)(half_t * (double)hd.ang_v[2]);
    // delta_q.inverse(): conjugate / squaredNorm when that is > 0, else the zero quaternion
    const float xx = qx * qx, yy = qy * qy, zz = qz * qz, ww = qw * qw;
    const float n2 = hd.norm_order == 0 ? (xx + yy) + (zz + ww) : hd.norm_order == 1 ? (xx + zz) + (yy + ww) : ((xx + yy) + zz) + ww;
    float ix = 0.f, iy = 0.f, iz = 0.f, iw = 0.f;
    if (n2 > 0.f) {
      ix = -qx / n2;
      iy = -qy / n2;
      iz = -qz / n2;
      iw = qw / n2;
    }
    // q * v, Eigen's _transformVector: uv = q.vec x v; uv += uv; v + w * uv + q.vec x uv
    float ux = iy * p.z - iz * p.y;
    float uy = iz * p.x - ix * p.z;
    float uz = ix * p.y - iy * p.x;
    ux = ux + ux;
    uy = uy + uy;
    uz = uz + uz;
    const float rx = (p.x + iw * ux) + (iy * uz - iz * uy);
    const float ry = (p.y + iw * uy) + (iz * ux - ix * uz);
    const float rz = (p.z + iw * uz) + (ix * uy - iy * ux);
    p.x = rx;
    p.y = ry;
    p.z = rz;   // the fourth float is copied (:349)
  }
  // the non-dense branch of transformPointCloud copies a non-finite point as it is
  if (hd.transform && isfinite(p.x) && isfinite(p.y) && isfinite(p.z)) {
    const double x = (double)p.x, y = (double)p.y, z = (double)p.z;
    p.x = (float)(((hd.m[0] * x + hd.m[1] * y) + hd.m[2] * z) + hd.m[3]);
    p.y = (float)(((hd.m[4] * x + hd.m[5] * y) + hd.m[6] * z) + hd.m[7]);
    p.z = (float)(((hd.m[8] * x + hd.m[9] * y) + hd.m[10] * z) + hd.m[11]);
    if (hd.sets_w) p.w = 1.0f;
  }
  return p;
}

// head + distance_filter's decision (pf_distance_body's, on the transformed point)
__device__ __forceinline__ void pf_head_flag_body(const float4* __restrict__ in, const long long n, const PfHead& hd, const double near_t, const double far_t,
                                                  unsigned char* __restrict__ flags, const int blk) {
  const long long i = (long long)blk * kBlock + threadIdx.x;
  if (i >= n) return;
  const float4 p = pf_head_point(in[i], i, n, hd);
  const float d = sqrtf(add_rn(add_rn(mul_rn(p.x, p.x), mul_rn(p.y, p.y)), mul_rn(p.z, p.z)));
  const double dd = (double)d;
  flags[i] = (dd > near_t && dd < far_t) ? 1 : 0;
}

// the scatter over the raw cloud: kept point i is recomputed from the raw one and written at its compacted place `off`
__device__ __forceinline__ void pf_head_scatter_body(const float4* __restrict__ in, const long long n, const PfHead& hd, const long long i, const int off,
                                                     float4* __restrict__ out) {
  out[off] = pf_head_point(in[i], i, n, hd);
}

// dgs_prefilter_scan_params -> the head's kernel argument and lidar_position (:113, :143)
inline bool pf_make_head(const dgs_prefilter_scan_params* sp, PfHead* head, double* lidar) {
  if (!sp || sp->struct_size != sizeof(dgs_prefilter_scan_params) || sp->deskew_norm_order < DGS_PF_NORM_PAIRS_XY_ZW ||
      sp->deskew_norm_order > DGS_PF_NORM_SEQUENTIAL)
    return false;
  std::memset(head, 0, sizeof(*head));
  head->deskew = sp->has_angular_velocity ? 1 : 0;
  head->transform = sp->has_transform ? 1 : 0;
  head->norm_order = sp->deskew_norm_order;
  head->sets_w = sp->transform_sets_w ? 1 : 0;
  for (int a = 0; a < 3; a++) head->ang_v[a] = (float)sp->angular_velocity[a] * -1.0f;   // Eigen::Vector3f ang_v(...); ang_v *= -1 (:330-331)
  head->scan_period = sp->scan_period;
  for (int a = 0; a < 12; a++) head->m[a] = sp->transform[a];
  lidar[0] = lidar[1] = lidar[2] = 0.0;   // Eigen::Vector3d::Zero() (:113)
  if (sp->has_transform) { lidar[0] = sp->transform[3]; lidar[1] = sp->transform[7]; lidar[2] = sp->transform[11]; }   // .translation() (:143)
  return true;
}

// ================================================================================================ k-NN passes
// The list of query `pos` (index order) as sorted keys (float distance bits << 32 | index), empty slots last.
template <int N>
__device__ __forceinline__ int pf_sorted_list(const float4* __restrict__ pts, const int n, const int k, const int* __restrict__ nbr, const int pos,
                                              const float4 q, unsigned long long (&key)[N]) {
  int found = 0;
#pragma unroll
  for (int s = 0; s < N; s++) {
    const int j = (s < k) ? nbr[(size_t)pos * kKnnMax + s] : -1;
    if (j >= 0 && j < n) {
      const float4 p = pts[j];
      const float d = sqdist_rn(q.x, q.y, q.z, p.x, p.y, p.z);   // FLANN L2_Simple: (dx*dx + dy*dy) + dz*dz in float
      key[s] = ((unsigned long long)__float_as_uint(d) << 32) | (unsigned)j;
      found++;
    } else {
      key[s] = ~0ull;
    }
  }
  // bitonic sorting network: constant indices only, the keys stay in registers
#pragma unroll
  for (int size = 2; size <= N; size <<= 1)
#pragma unroll
    for (int stride = size >> 1; stride > 0; stride >>= 1)
#pragma unroll
      for (int a = 0; a < N; a++) {
        const int b = a ^ stride;
        if (b > a) {
          const unsigned long long x = key[a], y = key[b];
          const bool up = (a & size) == 0;
          if ((x > y) == up) { key[a] = y; key[b] = x; }
        }
      }
  return found;
}

__device__ __forceinline__ float pf_key_dist(unsigned long long key) { return __uint_as_float((unsigned)(key >> 32)); }

// RadiusOutlierRemoval (PCL 1.10, dense input): nearestKSearch with k = min_neighbors + 1 (the query counts); kept iff k points were
// found and the k-th smallest squared distance is <= r^2 (inclusive) or < r^2, compared in double.  The k-th smallest distance of the
// exact k-set is its largest: no sort needed.
__device__ __forceinline__ void pf_radius_body(const BvhView& b, const float4* __restrict__ pts, const int n, const int k, const int* __restrict__ nbr,
                                               const double r2, const int inclusive, unsigned char* __restrict__ flags, const int blk) {
  const int pos = blk * kBlock + threadIdx.x;
  if (pos >= n) return;
  const int i = (int)__float_as_uint(b.sorted[pos].w);
  if (i < 0 || i >= n) return;
  const float4 q = pts[i];
  int found = 0;
  float dmax = 0.f;
  for (int s = 0; s < k; s++) {
    const int j = nbr[(size_t)pos * kKnnMax + s];
    if (j >= 0 && j < n) {
      const float4 p = pts[j];
      dmax = fmaxf(dmax, sqdist_rn(q.x, q.y, q.z, p.x, p.y, p.z));
      found++;
    }
  }
  const double dk = (double)dmax;
  const bool keep = found == k && (inclusive ? dk <= r2 : dk < r2);
  flags[i] = keep ? 1 : 0;
}

// StatisticalOutlierRemoval, first pass: nearestKSearch(mean_k + 1), index 0 is the query; dist_sum (double) += sqrt(d^2) over
// j = 1..mean_k in ascending order; distances[i] = (float)(dist_sum / mean_k).
__device__ __forceinline__ void pf_sor_distance_body(const BvhView& b, const float4* __restrict__ pts, const int n, const int k, const int* __restrict__ nbr,
                                                     const int sqrt_float, float* __restrict__ mean_d, const int blk) {
  const int pos = blk * kBlock + threadIdx.x;
  if (pos >= n) return;
  const int i = (int)__float_as_uint(b.sorted[pos].w);
  if (i < 0 || i >= n) return;
  unsigned long long key[kKnnMax];
  pf_sorted_list<kKnnMax>(pts, n, k, nbr, pos, pts[i], key);
  double dist_sum = 0.0;
#pragma unroll
  for (int s = 1; s < kKnnMax; s++) {
    if (s < k) {
      const float d2 = pf_key_dist(key[s]);
      dist_sum += sqrt_float ? (double)sqrtf(d2) : sqrt((double)d2);
    }
  }
  mean_d[i] = (float)(dist_sum / (double)(k - 1));
}

// mean / stddev / threshold: sum and sq_sum as double sums (sq_sum adds the float product d*d), reduced in a fixed order in one
// workgroup; variance = (sq_sum - sum*sum/n) / (n-1), threshold = mean + mul * sqrt(variance).
__device__ __forceinline__ void pf_sor_stats_body(const float* __restrict__ mean_d, const int n, const double mul, double* __restrict__ stats) {
#pragma clang fp contract(off)
  __shared__ double s_s[kPfStatsBlock], s_q[kPfStatsBlock];
  double s = 0.0, q = 0.0;
  for (int i = threadIdx.x; i < n; i += kPfStatsBlock) {
    const float d = mean_d[i];
    s += (double)d;
    q += (double)mul_rn(d, d);
  }
  s_s[threadIdx.x] = s;
  s_q[threadIdx.x] = q;
  __syncthreads();
  for (int h = kPfStatsBlock / 2; h > 0; h >>= 1) {
    if ((int)threadIdx.x < h) {
      s_s[threadIdx.x] += s_s[threadIdx.x + h];
      s_q[threadIdx.x] += s_q[threadIdx.x + h];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const double sum = s_s[0], sq_sum = s_q[0], nn = (double)n;
    const double mean = sum / nn;
    const double variance = (sq_sum - sum * sum / nn) / (nn - 1.0);
    const double stddev = sqrt(variance);
    stats[0] = mean;
    stats[1] = stddev;
    stats[2] = mean + mul * stddev;
    stats[3] = variance;
  }
}

// second pass: removed iff distances[i] > threshold (a NaN threshold removes nothing, as upstream)
__device__ __forceinline__ void pf_sor_flag_body(const float* __restrict__ mean_d, const int n, const double* __restrict__ stats,
                                                 unsigned char* __restrict__ flags, const int blk) {
  const int i = blk * kBlock + threadIdx.x;
  if (i >= n) return;
  flags[i] = ((double)mean_d[i] > stats[2]) ? 0 : 1;
}

// ---- pcl::eigen33 in float: pf_compute_roots and pf_eigen33_vector (eigen33.h)
// eigenvector of the smallest eigenvalue
__device__ inline void pf_eigen33(const float* mat, float* ev) {
#pragma clang fp contract(off)
  float scale = 0.f;
#pragma unroll
  for (int a = 0; a < 9; a++) scale = fmaxf(scale, fabsf(mat[a]));
  if (scale <= FLT_MIN) scale = 1.f;
  float m[9];
#pragma unroll
  for (int a = 0; a < 9; a++) m[a] = mat[a] / scale;
  float r[3];
  pf_compute_roots(m, r);
  m[0] -= r[0]; m[4] -= r[0]; m[8] -= r[0];
  pf_eigen33_vector(m, ev);
}

// normal_filtering: NormalEstimation (k = 10 on this cloud) -> computeMeanAndCovarianceMatrix (9-float raw moments in neighbour order,
// divided by the float count, cov = E[ab] - mean_a * mean_b) -> eigen33 -> flipNormalTowardsViewpoint -> .normalized(); kept iff
// |n.z| < 0.2f.  Fewer than 3 neighbours: NaN normal, dropped.
__device__ __forceinline__ void pf_normal_body(const BvhView& b, const float4* __restrict__ pts, const int n, const int k, const int* __restrict__ nbr,
                                               const float vx, const float vy, const float vz, unsigned char* __restrict__ flags,
                                               float4* __restrict__ normals, float* __restrict__ cov9, const int blk) {
#pragma clang fp contract(off)
  const int pos = blk * kBlock + threadIdx.x;
  if (pos >= n) return;
  const int i = (int)__float_as_uint(b.sorted[pos].w);
  if (i < 0 || i >= n) return;
  const float4 q = pts[i];
  unsigned long long key[16];
  const int found = pf_sorted_list<16>(pts, n, k, nbr, pos, q, key);
  float* C = cov9 + (size_t)i * 9;
  const float qnan = __int_as_float(0x7fc00000);
  if (found < 3) {
#pragma unroll
    for (int a = 0; a < 9; a++) C[a] = qnan;
    normals[i] = make_float4(qnan, qnan, qnan, qnan);
    flags[i] = 0;
    return;
  }
  float acc[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int s = 0; s < 16; s++) {
    if (s < found) {
      const float4 p = pts[(int)(unsigned)(key[s] & 0xffffffffull)];
      acc[0] += p.x * p.x; acc[1] += p.x * p.y; acc[2] += p.x * p.z;
      acc[3] += p.y * p.y; acc[4] += p.y * p.z; acc[5] += p.z * p.z;
      acc[6] += p.x; acc[7] += p.y; acc[8] += p.z;
    }
  }
  const float cnt = (float)found;
#pragma unroll
  for (int a = 0; a < 9; a++) acc[a] = acc[a] / cnt;
  float m[9];
  m[0] = acc[0] - acc[6] * acc[6];
  m[1] = acc[1] - acc[6] * acc[7];
  m[2] = acc[2] - acc[6] * acc[8];
  m[4] = acc[3] - acc[7] * acc[7];
  m[5] = acc[4] - acc[7] * acc[8];
  m[8] = acc[5] - acc[8] * acc[8];
  m[3] = m[1]; m[6] = m[2]; m[7] = m[5];
#pragma unroll
  for (int a = 0; a < 9; a++) C[a] = m[a];
  float nv[3];
  pf_eigen33(m, nv);
  // flipNormalTowardsViewpoint: (vp - p) . n < 0 -> n = -n
  const float cos_theta = ((vx - q.x) * nv[0] + (vy - q.y) * nv[1]) + (vz - q.z) * nv[2];
  if (cos_theta < 0.f) { nv[0] = -nv[0]; nv[1] = -nv[1]; nv[2] = -nv[2]; }
  // Eigen's normalized(): n / sqrt(squaredNorm) when squaredNorm > 0
  const float z = (nv[0] * nv[0] + nv[1] * nv[1]) + nv[2] * nv[2];
  if (z > 0.f) {
    const float s = sqrtf(z);
    nv[0] = nv[0] / s; nv[1] = nv[1] / s; nv[2] = nv[2] / s;
  }
  normals[i] = make_float4(nv[0], nv[1], nv[2], 0.f);
  flags[i] = (fabsf(nv[2]) < kPfNormalThresh) ? 1 : 0;
}

}  // namespace dgs
