// dgs_cloud_assign_batch: n inputs down-sampled into n resident clouds by ONE chain of launches (the frame loop of several odometry
// streams: ScanMatchingOdometryNodelet::downsample, apps/scan_matching_odometry_nodelet.cpp:155-165 of the reference, once per stream).
//
// VOXELGRID is voxel_grid_filter (ndt_voxel.hip) restated over segments.  Cloud i receives, bit for bit and in the same order, what the
// single call gives input i alone:
//   1. per-cloud boxes of the finite points (min / max: exact in any order)                      -> host wait 1: grids and PCL's overflow test
//   2. one key per point, (cloud number << 32) | cell index in the cloud's OWN grid (voxel_key_kernel's float arithmetic); a point that
//      is not finite gets cell 0xFFFFFFFF, which sorts last inside its cloud
//   3. one stable radix sort of all keys (values = index of the point in its cloud, so the order inside a cell is point-index order),
//      one run-length pass, one scan of the run lengths
//   4. per cloud its first run and the end of its emitted runs (the run of non-finite points is dropped)
//   5. one lane per emitted cell sums its points in float in point-index order and divides by the float count (voxel_centroid_kernel's
//      expressions; the points are read through the sorted values, so no gathered copy is made)      -> host wait 2: the n sizes
// The same cell index in two clouds never merges: the cloud number stands above it in the key.  A workgroup of the box, key and centroid
// kernels belongs to one cloud (blockIdx.y), so the cloud's record is read by scalar loads and its grid sits in SGPRs.
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstring>
#include <vector>

#include "handle.h"
#include "seg_device.h"

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

// ---- 2. keys (voxel_key_kernel per segment, the cloud's number above the 32 bits of the cell) ------------------------------------
__global__ __launch_bounds__(kBlock) void vb_key_kernel(const VbSeg* __restrict__ segs, unsigned long long* __restrict__ keys, uint32_t* __restrict__ vals) {
  const VbSeg& S = segs[blockIdx.y];
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= S.n) return;
  const float4 p = S.in[i];
  uint32_t key = 0xFFFFFFFFu;
  if (isfinite(p.x) && isfinite(p.y) && isfinite(p.z)) {
    const int i0 = (int)(floorf(p.x * S.inv_leaf) - (float)S.min_b[0]);
    const int i1 = (int)(floorf(p.y * S.inv_leaf) - (float)S.min_b[1]);
    const int i2 = (int)(floorf(p.z * S.inv_leaf) - (float)S.min_b[2]);
    key = (uint32_t)(i0 + i1 * S.mul1 + i2 * S.mul2);
  }
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
  if (r == nr - 1 || (int)(run_keys[r + 1] >> 32) != c) bounds[2 * c + 1] = ((uint32_t)k == 0xFFFFFFFFu) ? r : r + 1;   // the run of non-finite points sorts last: not emitted
}

// ---- 5. centroids (voxel_centroid_kernel per segment): one lane per emitted cell, float sums in point-index order -----------------
__global__ __launch_bounds__(kBlock) void vb_centroid_kernel(const VbSeg* __restrict__ segs, const uint32_t* __restrict__ order, const int* __restrict__ run_counts,
                                                             const int* __restrict__ run_offsets, const int* __restrict__ bounds) {
  const VbSeg& S = segs[blockIdx.y];
  const int first = bounds[2 * blockIdx.y], cells = bounds[2 * blockIdx.y + 1] - first;
  const int c = blockIdx.x * kBlock + threadIdx.x;
  if (c >= cells) return;
  const int off = run_offsets[first + c], cnt = run_counts[first + c];
  float sx = 0.f, sy = 0.f, sz = 0.f;
  for (int j = 0; j < cnt; j++) {
    const float4 p = S.in[order[off + j]];
    sx += p.x; sy += p.y; sz += p.z;
  }
  const float fn = (float)cnt;
  S.out[c] = make_float4(sx / fn, sy / fn, sz / fn, 1.f);
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
  DGS_HIP_TRY(h, V.keys.reserve((size_t)total));
  DGS_HIP_TRY(h, V.keys_alt.reserve((size_t)total));
  DGS_HIP_TRY(h, V.run_keys.reserve((size_t)total));
  DGS_HIP_TRY(h, V.vals.reserve((size_t)total));
  DGS_HIP_TRY(h, V.vals_alt.reserve((size_t)total));
  DGS_HIP_TRY(h, V.run_counts.reserve((size_t)total));
  DGS_HIP_TRY(h, V.run_offsets.reserve((size_t)total));
  DGS_HIP_TRY(h, V.scalars.reserve(8));
  DGS_HIP_TRY(h, V.bounds.reserve((size_t)n * 2));
  int seg_bits = 0;
  while ((1 << seg_bits) < n) seg_bits++;
  size_t t1 = 0, t2 = 0, t3 = 0;
  (void)hipcub::DeviceRadixSort::SortPairs(nullptr, t1, V.keys.ptr, V.keys_alt.ptr, V.vals.ptr, V.vals_alt.ptr, (int)total, 0, 32 + seg_bits, st);
  (void)hipcub::DeviceRunLengthEncode::Encode(nullptr, t2, V.keys_alt.ptr, V.run_keys.ptr, V.run_counts.ptr, V.scalars.ptr, (int)total, st);
  (void)hipcub::DeviceScan::ExclusiveSum(nullptr, t3, V.run_counts.ptr, V.run_offsets.ptr, (int)total, st);
  DGS_HIP_TRY(h, h->cub_temp.reserve(std::max(t1, std::max(t2, t3)) + 256));

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

  // grids (voxel_grid_filter's arithmetic) and PCL's overflow test, per cloud, before anything is written
  const float inv_leaf = 1.0f / leaf;
  for (int i = 0; i < n; i++) {
    const float* hmm = boxes_h + (size_t)i * 6;
    segs[i].inv_leaf = inv_leaf;
    if (sizes[i] == 0 || !(hmm[0] <= hmm[3])) continue;   // no finite point: every key is the non-finite one, nothing is emitted
    int div_b[3];
    int64_t cells = 1;
    for (int a = 0; a < 3; a++) {
      segs[i].min_b[a] = (int)std::floor(hmm[a] * inv_leaf);
      div_b[a] = (int)std::floor(hmm[3 + a] * inv_leaf) - segs[i].min_b[a] + 1;
      cells *= (int64_t)((hmm[3 + a] - hmm[a]) * inv_leaf) + 1;
    }
    if (cells > INT32_MAX || (int64_t)div_b[0] * div_b[1] * div_b[2] > INT32_MAX) {
      prof_end(h, DGS_K_NDT_VOXEL_BUILD, slot);
      h->err = "Leaf size is too small for the input dataset. Integer indices would overflow. (cloud " + std::to_string(i) + " of the batch)";
      return DGS_ERR_GRID_TOO_LARGE;
    }
    segs[i].mul1 = div_b[0];
    segs[i].mul2 = div_b[0] * div_b[1];
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
  hipLaunchKernelGGL(vb_key_kernel, dim3(nb_max, n), dim3(kBlock), 0, st, V.segs.ptr, V.keys.ptr, V.vals.ptr);
  size_t tb = h->cub_temp.cap;
  DGS_HIP_TRY(h, hipcub::DeviceRadixSort::SortPairs(h->cub_temp.ptr, tb, V.keys.ptr, V.keys_alt.ptr, V.vals.ptr, V.vals_alt.ptr, (int)total, 0, 32 + seg_bits, st));
  tb = h->cub_temp.cap;
  DGS_HIP_TRY(h, hipcub::DeviceRunLengthEncode::Encode(h->cub_temp.ptr, tb, V.keys_alt.ptr, V.run_keys.ptr, V.run_counts.ptr, V.scalars.ptr, (int)total, st));
  tb = h->cub_temp.cap;
  DGS_HIP_TRY(h, hipcub::DeviceScan::ExclusiveSum(h->cub_temp.ptr, tb, V.run_counts.ptr, V.run_offsets.ptr, (int)total, st));
  hipLaunchKernelGGL(vb_bounds_kernel, dim3(nb_total), dim3(kBlock), 0, st, V.run_keys.ptr, V.scalars.ptr, V.bounds.ptr);
  hipLaunchKernelGGL(vb_centroid_kernel, dim3(nb_max, n), dim3(kBlock), 0, st, V.segs.ptr, V.vals_alt.ptr, V.run_counts.ptr, V.run_offsets.ptr, V.bounds.ptr);
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
  V.in.release(); V.segs.release(); V.mm.release(); V.keys.release(); V.keys_alt.release(); V.run_keys.release(); V.vals.release(); V.vals_alt.release();
  V.run_counts.release(); V.run_offsets.release(); V.scalars.release(); V.bounds.release();
}

}  // namespace dgs
