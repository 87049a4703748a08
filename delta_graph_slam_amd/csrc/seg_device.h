// Device pieces of the launches that run over a table of segments (clouds, scans, edges), written once: which segment owns a workgroup
// (cov_batch.hip, prefilter_batch.hip, fitness_batch.hip) and the boxes of the finite points, for one cloud (ndt_voxel.hip) or per
// segment (voxel_batch.hip, fitness_batch.hip).  Nothing of the k-NN search in here.
#pragma once
#include <cfloat>
#include <cmath>

#include "common.h"

namespace dgs {

// A launch in which segment c owns the workgroups [first[c], first[c + 1]): the segment of workgroup `blk` is the largest c with
// first[c] <= blk (first[0] = 0, ascending, blk < first[m]).  A segment may own no workgroup: it shares its successor's first, and the
// largest such c is the successor, never the empty one.  Uniform: scalar loads.
__device__ __forceinline__ int seg_find(const int* __restrict__ first, const int m, const int blk) {
  int lo = 0, hi = m;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (first[mid] <= blk) lo = mid; else hi = mid;
  }
  return lo;
}

// ---- boxes of the finite points: min and max are exact, so the order of the folds does not show in the result
__device__ __forceinline__ void box_add_finite(const float4 p, float (&mn)[3], float (&mx)[3]) {
  if (isfinite(p.x) && isfinite(p.y) && isfinite(p.z)) {
    mn[0] = fminf(mn[0], p.x); mn[1] = fminf(mn[1], p.y); mn[2] = fminf(mn[2], p.z);
    mx[0] = fmaxf(mx[0], p.x); mx[1] = fmaxf(mx[1], p.y); mx[2] = fmaxf(mx[2], p.z);
  }
}
// per-lane mn / mx of a workgroup of kBlock lanes -> out[at .. at + 6) = its min xyz, max xyz (lanes 0..5 write one float each)
template <class Index>
__device__ __forceinline__ void box_fold_block(float (&mn)[3], float (&mx)[3], float* __restrict__ out, const Index at) {
  __shared__ float sm[kBlock / kWave][6];
#pragma unroll
  for (int a = 0; a < 3; a++) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      mn[a] = fminf(mn[a], __shfl_down(mn[a], off, 64));
      mx[a] = fmaxf(mx[a], __shfl_down(mx[a], off, 64));
    }
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0)
    for (int a = 0; a < 3; a++) { sm[wave][a] = mn[a]; sm[wave][3 + a] = mx[a]; }
  __syncthreads();
  if (threadIdx.x < 6) {
    float v = sm[0][threadIdx.x];
    for (int w = 1; w < kBlock / kWave; w++) v = (threadIdx.x < 3) ? fminf(v, sm[w][threadIdx.x]) : fmaxf(v, sm[w][threadIdx.x]);
    out[at + threadIdx.x] = v;
  }
}
// six per-lane values folded through one wave into lane 0: min for 0..2, max for 3..5
__device__ __forceinline__ void box_fold_wave(float (&v)[6]) {
#pragma unroll
  for (int a = 0; a < 6; a++) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const float o = __shfl_down(v[a], off, 64);
      v[a] = (a < 3) ? fminf(v[a], o) : fmaxf(v[a], o);
    }
  }
}

// ---- per segment (minmax_kernel / minmax_final_kernel of ndt_voxel.hip): blockIdx.y = segment, kSegBoxBlocks partial boxes each
constexpr int kSegBoxBlocks = kWave;   // partial boxes per segment = lanes of the wave that folds them
// grid (kSegBoxBlocks, segments) x kBlock
__device__ __forceinline__ void seg_box_partial_body(const float4* __restrict__ pts, const int n, float* __restrict__ partial) {
  float mn[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, mx[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
  for (int i = blockIdx.x * kBlock + threadIdx.x; i < n; i += kSegBoxBlocks * kBlock) box_add_finite(pts[i], mn, mx);
  box_fold_block(mn, mx, partial, ((size_t)blockIdx.y * kSegBoxBlocks + blockIdx.x) * 6);
}
// grid (segments) x kWave: one partial box per lane
__device__ __forceinline__ void seg_box_final_body(const float* __restrict__ partial, float* __restrict__ boxes) {
  const float* p = partial + ((size_t)blockIdx.x * kSegBoxBlocks + threadIdx.x) * 6;
  float v[6];
#pragma unroll
  for (int a = 0; a < 6; a++) v[a] = p[a];
  box_fold_wave(v);
  if (threadIdx.x == 0)
    for (int a = 0; a < 6; a++) boxes[(size_t)blockIdx.x * 6 + a] = v[a];
}

}  // namespace dgs
