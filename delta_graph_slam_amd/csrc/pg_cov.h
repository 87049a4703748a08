// pcl::GeneralizedIterativeClosestPoint::computeCovariances as device bodies, written once: pg_cov_kernel / pg_cov_wide_kernel
// (pcl_gicp.hip) run them over one cloud, cov_pcl_batch_kernel / cov_pcl_batch_wide_kernel (cov_batch.hip) over every cloud of a chunk.
#pragma once
#include <climits>
#include <cmath>
#include <cstdint>

#include "handle.h"
#include "nn_group.h"
#include "small_linalg.h"

namespace dgs {

// Sorting network (odd-even transposition) over kKnnMax register slots; compile-time indices only.
__device__ __forceinline__ void pg_sort32(int* v) {
#pragma unroll
  for (int r = 0; r < kKnnMax; r++) {
#pragma unroll
    for (int i = (r & 1); i + 1 < kKnnMax; i += 2) {
      const int lo = min(v[i], v[i + 1]), hi = max(v[i], v[i + 1]);
      v[i] = lo;
      v[i + 1] = hi;
    }
  }
}

// The neighbours' sums, one point after another in ascending index order, and what computeCovariances makes of them.
struct PgCovSums {
  double mx = 0, my = 0, mz = 0, sxx = 0, syx = 0, syy = 0, szx = 0, szy = 0, szz = 0;
  __device__ __forceinline__ void add(const float4 p) {
#pragma clang fp contract(off)
    mx += (double)p.x; my += (double)p.y; mz += (double)p.z;
    sxx += (double)(p.x * p.x);
    syx += (double)(p.y * p.x); syy += (double)(p.y * p.y);
    szx += (double)(p.z * p.x); szy += (double)(p.z * p.y); szz += (double)(p.z * p.z);
  }
  __device__ __forceinline__ void finish(const int k, const double eps, double* out) {
#pragma clang fp contract(off)
    const double kk = (double)k;
    mx /= kk; my /= kk; mz /= kk;
    double C[9];
    C[0] = sxx / kk - mx * mx;
    C[3] = syx / kk - my * mx; C[4] = syy / kk - my * my;
    C[6] = szx / kk - mz * mx; C[7] = szy / kk - mz * my; C[8] = szz / kk - mz * mz;
    C[1] = C[3]; C[2] = C[6]; C[5] = C[7];
    double U[9], V[9], sv[3];
    jacobi_svd3_d(C, U, V, sv);
    const double val[3] = {1.0, 1.0, eps};
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
      for (int c = 0; c < 3; c++)
        out[r * 3 + c] = ((val[0] * U[r * 3 + 0]) * U[c * 3 + 0] + (val[1] * U[r * 3 + 1]) * U[c * 3 + 1]) + (val[2] * U[r * 3 + 2]) * U[c * 3 + 2];
  }
};

// computeCovariances for one point per lane.  nbr: slot lists in index order (pos), -1 = nothing found (a zero column, as upstream's
// matrix); out: 9 doubles per point in the caller's order.  Non-finite points get NaN (they never pair, never are a neighbour).
// blk: the workgroup's index among the workgroups of this cloud (blockIdx.x for a launch over one cloud).
__device__ __forceinline__ void pg_cov_body(const BvhView& b, const float4* __restrict__ pts, const int n, const int k, const double eps,
                                            const int* __restrict__ nbr, double* __restrict__ cov9, const int blk) {
#pragma clang fp contract(off)
  const int pos = blk * kBlock + threadIdx.x;
  if (pos >= n) return;
  const int i = (int)__float_as_uint(b.sorted[pos].w);
  if (i < 0 || i >= n) return;
  const float4 q = pts[i];
  double* out = cov9 + (size_t)i * 9;
  if (!(isfinite(q.x) && isfinite(q.y) && isfinite(q.z))) {
    for (int a = 0; a < 9; a++) out[a] = NAN;
    return;
  }
  int v[kKnnMax];
#pragma unroll
  for (int s = 0; s < kKnnMax; s++) {
    const int j = (s < k) ? nbr[(size_t)pos * kKnnMax + s] : -1;
    v[s] = (j >= 0 && j < n) ? j : INT_MAX;
  }
  pg_sort32(v);
  PgCovSums sums;
#pragma unroll
  for (int s = 0; s < kKnnMax; s++) {
    if (v[s] != INT_MAX) sums.add(pts[v[s]]);
  }
  sums.finish(k, eps, out);
}

// 32 < k <= 64, table stride kKnnMaxWide.  A 64-slot sorting network in registers is 2,016 compare-exchanges of straight-line code per
// lane (the compiler did not finish it); the list is sorted in LDS instead: lane t owns column t of s_v (consecutive lanes, consecutive
// banks: no conflict) and inserts its neighbours one by one.  Same sums in the same (ascending index) order as the narrow kernel.
// 128 lanes per workgroup: 32 KiB of LDS.
constexpr int kPgWideBlock = 128;
__device__ __forceinline__ void pg_cov_wide_body(const BvhView& b, const float4* __restrict__ pts, const int n, const int k, const double eps,
                                                 const int* __restrict__ nbr, double* __restrict__ cov9, const int blk) {
#pragma clang fp contract(off)
  __shared__ int s_v[kKnnMaxWide][kPgWideBlock];
  const int tid = threadIdx.x;
  const int pos = blk * kPgWideBlock + tid;
  if (pos >= n) return;   // no barrier below: every lane works on its own column
  const int i = (int)__float_as_uint(b.sorted[pos].w);
  if (i < 0 || i >= n) return;
  const float4 q = pts[i];
  double* out = cov9 + (size_t)i * 9;
  if (!(isfinite(q.x) && isfinite(q.y) && isfinite(q.z))) {
    for (int a = 0; a < 9; a++) out[a] = NAN;
    return;
  }
  const int kc = min(k, kKnnMaxWide);
  int m = 0;   // neighbours found so far, s_v[0 .. m)[tid] ascending
#pragma unroll 1
  for (int s = 0; s < kc; s++) {
    const int j = nbr[(size_t)pos * kKnnMaxWide + s];
    if (j < 0 || j >= n) continue;
    int t = m;
#pragma unroll 1
    for (; t > 0 && s_v[t - 1][tid] > j; t--) s_v[t][tid] = s_v[t - 1][tid];
    s_v[t][tid] = j;
    m++;
  }
  PgCovSums sums;
#pragma unroll 1
  for (int s = 0; s < m; s++) sums.add(pts[s_v[s][tid]]);
  sums.finish(k, eps, out);
}

}  // namespace dgs
