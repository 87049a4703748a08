// What the structures keyed by voxel cell have in common, written once: the cell key of a point in pcl::VoxelGrid's grid and the
// centroid of a run (ndt_voxel.hip for one cloud, voxel_batch.hip per segment), and the chain from keys to runs over a KeyRuns
// (handle.h) that ndt_build_target, voxel_grid_filter, vgicp_build_map and voxelgrid_batch run.  The grid itself: voxel_grid_plan.h.
#pragma once
#include <hipcub/hipcub.hpp>

#include <algorithm>

#include "handle.h"

namespace dgs {

constexpr uint32_t kNonFiniteCell = 0xFFFFFFFFu;   // the key of a point that is not finite: its run sorts last

// VoxelGrid / VoxelGridCovariance first pass: the index arithmetic is in float as upstream, floor(p * inv_leaf) - (float)min_b per axis
__device__ __forceinline__ uint32_t voxel_cell_key(const float4 p, const float inv_leaf, const int (&min_b)[3], const int mul1, const int mul2) {
  if (!(isfinite(p.x) && isfinite(p.y) && isfinite(p.z))) return kNonFiniteCell;
  const int i0 = (int)(floorf(p.x * inv_leaf) - (float)min_b[0]);
  const int i1 = (int)(floorf(p.y * inv_leaf) - (float)min_b[1]);
  const int i2 = (int)(floorf(p.z * inv_leaf) - (float)min_b[2]);
  return (uint32_t)(i0 + i1 * mul1 + i2 * mul2);
}

// pcl::VoxelGrid's and pcl::ApproximateVoxelGrid's centroid of a run of cnt points: float sums in point-index order, divided by the
// float count.  point(j) fetches the j-th point of the run.
template <class Point>
__device__ __forceinline__ float4 run_centroid(const int cnt, const Point point) {
  float sx = 0.f, sy = 0.f, sz = 0.f;
  for (int j = 0; j < cnt; j++) {
    const float4 p = point(j);
    sx += p.x; sy += p.y; sz += p.z;
  }
  const float fn = (float)cnt;
  return make_float4(sx / fn, sy / fn, sz / fn, 1.f);
}

// ---- host: R.keys / R.vals -> stable sort -> runs -> offsets, on h->cub_temp ------------------------------------------------------
// Like DevBuf's methods these return hipError_t and the caller wraps them in DGS_HIP_TRY.  The library calls take the size of the
// temporary block by reference: every call starts from the block's capacity.
template <class Key>
size_t key_runs_sort_temp(KeyRuns<Key>& R, const int n, const int end_bit, hipStream_t st) {
  size_t t = 0;
  (void)hipcub::DeviceRadixSort::SortPairs(nullptr, t, R.keys.ptr, R.sorted_keys.ptr, R.vals.ptr, R.sorted_vals.ptr, n, 0, end_bit, st);
  return t;
}
// the temporary block of key_runs_chain: the three size queries, one reserve
template <class Key>
hipError_t key_runs_reserve_temp(dgs_handle* h, KeyRuns<Key>& R, RunTable<Key>& t, const int n, const int end_bit, hipStream_t st) {
  size_t t2 = 0, t3 = 0;
  (void)hipcub::DeviceRunLengthEncode::Encode(nullptr, t2, R.sorted_keys.ptr, t.keys.ptr, R.run_counts.ptr, t.scalars.ptr, n, st);
  (void)hipcub::DeviceScan::ExclusiveSum(nullptr, t3, R.run_counts.ptr, R.run_offsets.ptr, n, st);
  return h->cub_temp.reserve(std::max(key_runs_sort_temp(R, n, end_bit, st), std::max(t2, t3)) + 256);
}
template <class Key>
hipError_t key_runs_sort(dgs_handle* h, KeyRuns<Key>& R, const int n, const int end_bit, hipStream_t st) {
  size_t tb = h->cub_temp.cap;
  return hipcub::DeviceRadixSort::SortPairs(h->cub_temp.ptr, tb, R.keys.ptr, R.sorted_keys.ptr, R.vals.ptr, R.sorted_vals.ptr, n, 0, end_bit, st);
}
// three library calls: the sort, the run keys and the number of runs into `t`, the run lengths and their exclusive scan into R
template <class Key>
hipError_t key_runs_chain(dgs_handle* h, KeyRuns<Key>& R, RunTable<Key>& t, const int n, const int end_bit, hipStream_t st) {
  hipError_t e = key_runs_sort(h, R, n, end_bit, st);
  if (e != hipSuccess) return e;
  size_t tb = h->cub_temp.cap;
  e = hipcub::DeviceRunLengthEncode::Encode(h->cub_temp.ptr, tb, R.sorted_keys.ptr, t.keys.ptr, R.run_counts.ptr, t.scalars.ptr, n, st);
  if (e != hipSuccess) return e;
  tb = h->cub_temp.cap;
  return hipcub::DeviceScan::ExclusiveSum(h->cub_temp.ptr, tb, R.run_counts.ptr, R.run_offsets.ptr, n, st);
}

}  // namespace dgs
