// dgs_cloud_assign_batch: n inputs down-sampled into n resident clouds by ONE chain of launches (the frame loop of several odometry
// streams: ScanMatchingOdometryNodelet::downsample, apps/scan_matching_odometry_nodelet.cpp:155-165 of the reference, once per stream).
//
// VOXELGRID is voxel_grid_filter (ndt_voxel.hip) over segments: both run the grid of voxel_grid_plan.h and the key, the centroid and the
// chain of voxel_cells.h.  Cloud i receives, bit for bit and in the same order, what the single call gives input i alone:
//   1. per-cloud boxes of the finite points (min / max: exact in any order)                      -> host wait 1: grids and PCL's overflow test
//   2. one key per point, (cloud number << 32) | cell index in the cloud's OWN grid (voxel_cell_key); a point that is not finite gets
//      cell 0xFFFFFFFF, which sorts last inside its cloud
//   3. one stable radix sort of all keys (values = index of the point in its cloud, so the order inside a cell is point-index order),
//      one run-length pass, one scan of the run lengths (key_runs_chain)
//   4. per cloud its first run and the end of its emitted runs (the run of non-finite points is dropped)
//   5. one lane per emitted cell sums its points in float in point-index order and divides by the float count (run_centroid; the
//      points are read through the sorted values, so no gathered copy is made)                       -> host wait 2: the n sizes
// The same cell index in two clouds never merges: the cloud number stands above it in the key.  A workgroup of the box, key and centroid
// kernels belongs to one cloud (blockIdx.y), so the cloud's record is read by scalar loads and its grid sits in SGPRs.
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstring>
#include <vector>

#include "seg_device.h"
#include "voxel_cells.h"
#include "voxel_grid_plan.h"

namespace dgs {

struct VbSeg {
  const float4* in;    // the input points (the caller's device array, or its place in the staged slab)
  float4* out;         // the resident cloud's buffer: at least n points
  int n, off;          // points; first slot of this cloud in the shared key / value arrays
  int min_b[3];        // VoxelGrid::min_b, mul1, mul2, inv_leaf of the cloud's own grid
  int mul1, mul2;
  float inv_leaf;
  int pad[4];
};
static_assert(sizeof(VbSeg) == 64, "one cloud is one 64-byte scalar load");

// ---- 1. boxes: the per-segment bodies of seg_device.h over this file's records ----------------------------------------------------
__global__ __launch_bounds__(kBlock) void vb_minmax_kernel(const VbSeg* __restrict__ segs, float* __restrict__ partial) {
  const VbSeg& S = segs[blockIdx.y];
  seg_box_partial_body(S.in, S.n, partial);
}
__global__ __launch_bounds__(kWave) void vb_minmax_final_kernel(const float* __restrict__ partial, float* __restrict__ boxes) { seg_box_final_body(partial, boxes); }

// ---- 2. keys (voxel_cell_key per segment, the cloud's number above the 32 bits of the cell) --------------------------------------
__global__ __launch_bounds__(kBlock) void vb_key_kernel(const VbSeg* __restrict__ segs, unsigned long long* __restrict__ keys, uint32_t* __restrict__ vals) {
  const VbSeg& S = segs[blockIdx.y];
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= S.n) return;
  const uint32_t key = voxel_cell_key(S.in[i], S.inv_leaf, S.min_b, S.mul1, S.mul2);
  keys[(size_t)S.off + i] = ((unsigned long long)blockIdx.y << 32) | key;
  vals[(size_t)S.off + i] = (uint32_t)i;
}

// ---- 4. per cloud: bounds[2 c] = its first run, bounds[2 c + 1] = the end of its emitted runs (both 0 for a cloud without points) ----
__global__ __launch_bounds__(kBlock) void vb_bounds_kernel(const unsigned long long* __restrict__ run_keys, const int* __restrict__ scalars, int* __restrict__ bounds) {
  const int r = blockIdx.x * kBlock + threadIdx.x;
  const int nr = scalars[0];
  if (r >= nr) return;
  const unsigned long long k = run_keys[r];
  const int c = (int)(k >> 32);
  if (r == 0 || (int)(run_keys[r - 1] >> 32) != c) bounds[2 * c] = r;
  if (r == nr - 1 || (int)(run_keys[r + 1] >> 32) != c) bounds[2 * c + 1] = ((uint32_t)k == kNonFiniteCell) ? r : r + 1;   // the run of non-finite points sorts last: not emitted
}

// ---- 5. centroids (run_centroid per segment): one lane per emitted cell --------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void vb_centroid_kernel(const VbSeg* __restrict__ segs, const uint32_t* __restrict__ order, const int* __restrict__ run_counts,
                                                             const int* __restrict__ run_offsets, const int* __restrict__ bounds) {
  const VbSeg& S = segs[blockIdx.y];
  const int first = bounds[2 * blockIdx.y], cells = bounds[2 * blockIdx.y + 1] - first;
  const int c = blockIdx.x * kBlock + threadIdx.x;
  if (c >= cells) return;
  const int off = run_offsets[first + c];
  S.out[c] = run_centroid(run_counts[first + c], [&](const int j) { return S.in[order[off + j]]; });
}

// ---- host --------------------------------------------------------------------------------------------------------------------
// inputs: device pointers (host inputs have been staged by the caller).  On DGS_ERR_GRID_TOO_LARGE no cloud has been touched.
// The outputs are cloud states: those of dgs_cloud objects (`owners`, dgs_cloud_assign_batch) or a handle's own (prefilter_batch.hip).
int voxelgrid_batch(dgs_handle* h, int n, const float4* const* d_in, const int64_t* sizes, float leaf, CloudState* const* states, dgs_cloud* const* owners,
                    int64_t* out_sizes, StageCounts* sink) {
  VbScratch& V = h->vb;
  hipStream_t st = h->stream;
  int64_t total = 0;
  int max_n = 0;
  for (int i = 0; i < n; i++) {
    total += sizes[i];
    max_n = std::max<int>(max_n, (int)sizes[i]);
  }
  if (total > INT32_MAX) { h->err = "dgs_cloud_assign_batch: more than 2^31 points in one call"; return DGS_ERR_UNSUPPORTED; }
  for (int i = 0; i < n; i++) out_sizes[i] = 0;
  if (total == 0) {   // nothing to launch: every cloud becomes empty
    for (int i = 0; i < n; i++) {
      if (owners) cloud_detach_users(owners[i]);
      states[i]->invalidate();
      states[i]->n = 0;
    }
    return DGS_OK;
  }
  // pinned block: [cloud records | boxes | bounds]
  const size_t seg_bytes = sizeof(VbSeg) * (size_t)n, box_bytes = sizeof(float) * 6 * (size_t)n, bnd_bytes = sizeof(int) * 2 * (size_t)n;
  if (ensure_pinned(h, seg_bytes + box_bytes + bnd_bytes) != DGS_OK) return DGS_ERR_HIP;
  VbSeg* segs = reinterpret_cast<VbSeg*>(h->pinned);
  float* boxes_h = reinterpret_cast<float*>(reinterpret_cast<char*>(h->pinned) + seg_bytes);
  int* bounds_h = reinterpret_cast<int*>(reinterpret_cast<char*>(h->pinned) + seg_bytes + box_bytes);
  DGS_HIP_TRY(h, V.segs.reserve((size_t)n));
  DGS_HIP_TRY(h, V.mm.reserve((size_t)n * (kSegBoxBlocks + 1) * 6));
  KeyRuns<unsigned long long>& R = V.runs;
  DGS_HIP_TRY(h, R.reserve((size_t)total, R.table));
  DGS_HIP_TRY(h, V.bounds.reserve((size_t)n * 2));
  int seg_bits = 0;
  while ((1 << seg_bits) < n) seg_bits++;
  DGS_HIP_TRY(h, key_runs_reserve_temp(h, R, R.table, (int)total, 32 + seg_bits, st));

  // 1. boxes
  std::memset(segs, 0, seg_bytes);
  int off = 0;
  for (int i = 0; i < n; i++) {
    segs[i].in = d_in[i];
    segs[i].n = (int)sizes[i];
    segs[i].off = off;
    off += (int)sizes[i];
  }
  const int slot = prof_begin(h, DGS_K_NDT_VOXEL_BUILD);
  float* boxes_d = V.mm.ptr + (size_t)n * kSegBoxBlocks * 6;
  DGS_HIP_TRY(h, hipMemcpyAsync(V.segs.ptr, segs, seg_bytes, hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(vb_minmax_kernel, dim3(kSegBoxBlocks, n), dim3(kBlock), 0, st, V.segs.ptr, V.mm.ptr);
  hipLaunchKernelGGL(vb_minmax_final_kernel, dim3(n), dim3(kWave), 0, st, V.mm.ptr, boxes_d);
  DGS_HIP_TRY(h, hipMemcpyAsync(boxes_h, boxes_d, box_bytes, hipMemcpyDeviceToHost, st));
  DGS_HIP_TRY(h, hipStreamSynchronize(st));
  sink->launches += 2;
  sink->waits++;

  // grids (voxel_grid_plan.h) and PCL's overflow test, per cloud, before anything is written
  const float inv_leaf = 1.0f / leaf;
  for (int i = 0; i < n; i++) {
    segs[i].inv_leaf = inv_leaf;
    int div_b[3];
    // a cloud without points has the start values as its box; with no finite point every key is the non-finite one, nothing is emitted
    if (vgplan::plan(boxes_h + (size_t)i * 6, inv_leaf, segs[i].min_b, div_b, segs[i].mul1, segs[i].mul2) == vgplan::kTooLarge) {
      prof_end(h, DGS_K_NDT_VOXEL_BUILD, slot);
      h->err = std::string(vgplan::kTooLargeText) + " (cloud " + std::to_string(i) + " of the batch)";
      return DGS_ERR_GRID_TOO_LARGE;
    }
  }
  // from here on the clouds change: whoever borrowed one loses it, buffers grow to the input size (the steady state allocates nothing)
  for (int i = 0; i < n; i++) {
    if (owners) cloud_detach_users(owners[i]);
    states[i]->invalidate();
    states[i]->n = 0;
    if (sizes[i] > 0) DGS_HIP_TRY(h, states[i]->pts.reserve((size_t)sizes[i]));
    segs[i].out = states[i]->pts.ptr;
  }

  // 2. - 5.
  const int nb_max = (max_n + kBlock - 1) / kBlock, nb_total = (int)((total + kBlock - 1) / kBlock);
  DGS_HIP_TRY(h, hipMemcpyAsync(V.segs.ptr, segs, seg_bytes, hipMemcpyHostToDevice, st));
  DGS_HIP_TRY(h, hipMemsetAsync(V.bounds.ptr, 0, bnd_bytes, st));
  hipLaunchKernelGGL(vb_key_kernel, dim3(nb_max, n), dim3(kBlock), 0, st, V.segs.ptr, R.keys.ptr, R.vals.ptr);
  DGS_HIP_TRY(h, key_runs_chain(h, R, R.table, (int)total, 32 + seg_bits, st));
  hipLaunchKernelGGL(vb_bounds_kernel, dim3(nb_total), dim3(kBlock), 0, st, R.table.keys.ptr, R.table.scalars.ptr, V.bounds.ptr);
  hipLaunchKernelGGL(vb_centroid_kernel, dim3(nb_max, n), dim3(kBlock), 0, st, V.segs.ptr, R.sorted_vals.ptr, R.run_counts.ptr, R.run_offsets.ptr, V.bounds.ptr);
  DGS_HIP_TRY(h, hipMemcpyAsync(bounds_h, V.bounds.ptr, bnd_bytes, hipMemcpyDeviceToHost, st));
  prof_end(h, DGS_K_NDT_VOXEL_BUILD, slot);
  DGS_HIP_TRY(h, hipStreamSynchronize(st));
  DGS_HIP_TRY(h, hipGetLastError());
  sink->launches += 6;   // keys, sort, run lengths, scan, bounds, centroids
  sink->waits++;
  for (int i = 0; i < n; i++) {
    out_sizes[i] = bounds_h[2 * i + 1] - bounds_h[2 * i];
    states[i]->n = out_sizes[i];
  }
  return DGS_OK;
}

static int assign_voxelgrid(dgs_handle* h, int n, const float4* const* d_in, const int64_t* sizes, float leaf, dgs_cloud* const* clouds, int64_t* out_sizes) {
  std::vector<CloudState*> states((size_t)n);
  for (int i = 0; i < n; i++) states[i] = &clouds[i]->st;
  StageCounts sc;
  const int rc = voxelgrid_batch(h, n, d_in, sizes, leaf, states.data(), clouds, out_sizes, &sc);
  h->vb.counts8[0] += sc.launches;
  h->vb.counts8[1] += sc.waits;
  return rc;
}

int cloud_assign_batch(dgs_handle* h, int n, const float* const* inputs, const int64_t* sizes, int on_device, int filter, float leaf, dgs_cloud* const* clouds,
                       int64_t* out_sizes) {
  VbScratch& V = h->vb;
  std::fill(V.counts8, V.counts8 + 8, 0);
  V.counts8[2] = n;
  hipStream_t st = h->stream;
  std::vector<const float4*> d_in((size_t)n);
  if (!on_device && filter != 0) {
    if (int rc = stage_host_inputs(h, V.in, n, inputs, sizes, d_in.data())) return rc;
  } else {
    for (int i = 0; i < n; i++) d_in[i] = reinterpret_cast<const float4*>(inputs[i]);
  }
  if (filter == 1) return assign_voxelgrid(h, n, d_in.data(), sizes, leaf, clouds, out_sizes);

  // NONE: a copy.  APPROX_VOXELGRID: the single-cloud routine per cloud (its waits number n times as many)
  for (int i = 0; i < n; i++) {
    CloudState& C = clouds[i]->st;
    cloud_detach_users(clouds[i]);
    C.invalidate();
    C.n = 0;
    out_sizes[i] = 0;
    if (sizes[i] == 0) continue;
    DGS_HIP_TRY(h, C.pts.reserve((size_t)sizes[i]));
    if (filter == 0) {
      DGS_HIP_TRY(h, hipMemcpyAsync(C.pts.ptr, inputs[i], (size_t)sizes[i] * sizeof(float4), on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st));
      out_sizes[i] = sizes[i];
    } else {
      const int rc = approx_voxel_grid_filter(h, d_in[i], sizes[i], leaf, C.pts.ptr, sizes[i], &out_sizes[i]);
      if (rc != DGS_OK) return rc;
      V.counts8[0] += 8;
      V.counts8[1]++;
    }
    C.n = out_sizes[i];
  }
  if (filter == 0) {   // the caller's arrays are not read after return
    DGS_HIP_TRY(h, hipStreamSynchronize(st));
    V.counts8[1]++;
  }
  return DGS_OK;
}

void voxel_batch_release(dgs_handle* h) {
  VbScratch& V = h->vb;
  V.in.release(); V.segs.release(); V.mm.release(); V.runs.release(); V.bounds.release();
}

}  // namespace dgs
