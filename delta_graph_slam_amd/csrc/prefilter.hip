// PrefilteringNodelet::cloud_callback (/root/reference/apps/prefiltering_nodelet.cpp:111-164) from the distance filter to flatten,
// and, through dgs_prefilter_scan, from the raw scan: deskewing (:293-354) and the base_link transform (:122-150) in front of it.
//
//   deskewing (:340-351) -> base_link transform (:137-149) -> [the raw-scan head, fused into the distance filter's pass]
//   distance filter (:275-291) -> down-sampling (:249-260) -> outlier removal (:262-273)   = /filtered_points
//   height filter (:192-212) -> normal filter (:217-245) -> flatten (:166-188)            = /flat_filtered_points
//
// MI355X design
//   * Every pass-through filter is a keep flag per point followed by one stable compaction: a count pass (wave ballot + popcount per
//     workgroup), one workgroup scanning the counts, and a scatter pass (ballot prefix inside the wave, the wave totals of the
//     workgroup, the scanned workgroup offset).  The whole 16-byte point is copied, pad lane included.
//   * Down-sampling is dgs_voxel_grid_filter's / dgs_approx_voxel_grid_filter's code path, unchanged (ndt_voxel.hip).
//   * The outlier passes and the normal pass run on knn_lists.hip's exact k-NN lists (knn_lists, k <= 32) over an index of the
//     prefilter's own (PfScratch::cloud).  A list is the k smallest (float FLANN distance, index) keys, ties to the lower index; each
//     lane sorts its list (bitonic network in registers) before any order-dependent sum.
//   * StatisticalOutlierRemoval's mean and standard deviation are a fixed-order reduction in one workgroup; the threshold is
//     compared on the device.
//   * The raw-scan head is two kernels over the raw cloud: pf_head_flag_kernel deskews, transforms and takes the distance decision per
//     point, and pf_head_scatter_kernel recomputes the point and writes it at its compacted place.  No cloud-sized deskewed or
//     transformed intermediate exists; the count and scan kernels between the two are the compaction's own.
//   * The host reads a count back after each compaction that a later pass needs as a size (the NN index and the voxel filters are
//     shaped on the host), and once at the end.
// Semantics and the PCL 1.10 details recalled from upstream: DESIGN.md §6c.
#include <cfloat>
#include <climits>
#include <cmath>
#include <cstring>

#include "compact.h"
#include "handle.h"
#include "nn_group.h"
#include "prefilter_body.h"

namespace dgs {

// ================================================================================================ stable compaction
__global__ __launch_bounds__(kBlock) void pf_count_kernel(const unsigned char* __restrict__ flags, const int n, int* __restrict__ blk) {
  __shared__ int s_w[kBlock / kWave];
  const int i = blockIdx.x * kBlock + threadIdx.x;
  const bool f = i < n && flags[i] != 0;
  const unsigned long long m = __ballot(f);
  if ((threadIdx.x & (kWave - 1)) == 0) s_w[threadIdx.x / kWave] = __popcll(m);
  __syncthreads();
  if (threadIdx.x == 0) {
    int t = 0;
#pragma unroll
    for (int w = 0; w < kBlock / kWave; w++) t += s_w[w];
    blk[blockIdx.x] = t;
  }
}

// One workgroup: exclusive scan of the nb workgroup counts in place, total -> *total.  Chunks of 1024 in order, so the result is the
// same whatever the hardware schedule.
__global__ __launch_bounds__(kCompactScanBlock) void pf_scan_kernel(int* __restrict__ blk, const int nb, int* __restrict__ total) {
  __shared__ int s_w[kCompactScanBlock / kWave];
  __shared__ int s_carry;
  const int lane = threadIdx.x & (kWave - 1), wv = threadIdx.x / kWave;
  if (threadIdx.x == 0) s_carry = 0;
  __syncthreads();
  for (int base = 0; base < nb; base += kCompactScanBlock) {
    const int i = base + threadIdx.x;
    const int v = i < nb ? blk[i] : 0;
    int x = v;
#pragma unroll
    for (int o = 1; o < kWave; o <<= 1) {
      const int y = __shfl_up(x, o, kWave);
      if (lane >= o) x += y;
    }
    if (lane == kWave - 1) s_w[wv] = x;
    __syncthreads();
    if (wv == 0) {
      int w = lane < kCompactScanBlock / kWave ? s_w[lane] : 0;
#pragma unroll
      for (int o = 1; o < kCompactScanBlock / kWave; o <<= 1) {
        const int y = __shfl_up(w, o, kWave);
        if (lane >= o) w += y;
      }
      if (lane < kCompactScanBlock / kWave) s_w[lane] = w;
    }
    __syncthreads();
    const int carry = s_carry;
    const int before = carry + (wv ? s_w[wv - 1] : 0) + x - v;
    if (i < nb) blk[i] = before;
    __syncthreads();
    if (threadIdx.x == kCompactScanBlock - 1) s_carry = before + v;
    __syncthreads();
  }
  if (threadIdx.x == 0) *total = s_carry;
}

__global__ __launch_bounds__(kBlock) void pf_scatter_kernel(const float4* __restrict__ in, const unsigned char* __restrict__ flags, const int n,
                                                            const int* __restrict__ blk, float4* __restrict__ out, const int flatten) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  int off;
  if (!compact_slot(flags, i, n, blk, &off)) return;
  float4 p = in[i];
  if (flatten) p.z = 0.f;   // flatten (:181): point.z = 0
  out[off] = p;             // off < number of kept points <= n: `out` holds n points
}

// ================================================================================================ the passes over one scan
// Their bodies are prefilter_body.h's, shared with the segment-table kernels of prefilter_batch.hip; here the workgroup is blockIdx.x.
__global__ __launch_bounds__(kBlock) void pf_distance_kernel(const float4* __restrict__ in, const int n, const double near_t, const double far_t,
                                                             unsigned char* __restrict__ flags) {
  pf_distance_body(in, n, near_t, far_t, flags, (int)blockIdx.x);
}

__global__ __launch_bounds__(kBlock) void pf_height_kernel(const float4* __restrict__ in, const int n, const double lz, unsigned char* __restrict__ flags) {
  pf_height_body(in, n, lz, flags, (int)blockIdx.x);
}

// head + distance_filter's decision
__global__ __launch_bounds__(kBlock) void pf_head_flag_kernel(const float4* __restrict__ in, const long long n, const PfHead hd, const double near_t,
                                                              const double far_t, unsigned char* __restrict__ flags) {
  pf_head_flag_body(in, n, hd, near_t, far_t, flags, (int)blockIdx.x);
}

// pf_scatter_kernel over the raw cloud: the kept point is recomputed from the raw one and written at its compacted place
__global__ __launch_bounds__(kBlock) void pf_head_scatter_kernel(const float4* __restrict__ in, const unsigned char* __restrict__ flags, const long long n,
                                                                 const PfHead hd, const int* __restrict__ blk, float4* __restrict__ out) {
  const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
  int off;
  if (!compact_slot(flags, i, n, blk, &off)) return;
  pf_head_scatter_body(in, n, hd, i, off, out);   // off < number of kept points <= n: `out` holds n points
}

// the two steps alone (dgs_prefilter_deskew): every point, non-finite ones included, at its own place
__global__ __launch_bounds__(kBlock) void pf_head_apply_kernel(const float4* __restrict__ in, const long long n, const PfHead hd, float4* __restrict__ out) {
  const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  out[i] = pf_head_point(in[i], i, n, hd);
}

__global__ __launch_bounds__(kBlock) void pf_radius_kernel(const BvhView b, const float4* __restrict__ pts, const int n, const int k,
                                                           const int* __restrict__ nbr, const double r2, const int inclusive,
                                                           unsigned char* __restrict__ flags) {
  pf_radius_body(b, pts, n, k, nbr, r2, inclusive, flags, (int)blockIdx.x);
}

__global__ __launch_bounds__(kBlock) void pf_sor_distance_kernel(const BvhView b, const float4* __restrict__ pts, const int n, const int k,
                                                                 const int* __restrict__ nbr, const int sqrt_float, float* __restrict__ mean_d) {
  pf_sor_distance_body(b, pts, n, k, nbr, sqrt_float, mean_d, (int)blockIdx.x);
}

__global__ __launch_bounds__(kPfStatsBlock) void pf_sor_stats_kernel(const float* __restrict__ mean_d, const int n, const double mul,
                                                                    double* __restrict__ stats) {
  pf_sor_stats_body(mean_d, n, mul, stats);
}

__global__ __launch_bounds__(kBlock) void pf_sor_flag_kernel(const float* __restrict__ mean_d, const int n, const double* __restrict__ stats,
                                                             unsigned char* __restrict__ flags) {
  pf_sor_flag_body(mean_d, n, stats, flags, (int)blockIdx.x);
}

__global__ __launch_bounds__(kBlock) void pf_normal_kernel(const BvhView b, const float4* __restrict__ pts, const int n, const int k,
                                                           const int* __restrict__ nbr, const float vx, const float vy, const float vz,
                                                           unsigned char* __restrict__ flags, float4* __restrict__ normals,
                                                           float* __restrict__ cov9) {
  pf_normal_body(b, pts, n, k, nbr, vx, vy, vz, flags, normals, cov9, (int)blockIdx.x);
}

// ================================================================================================ host side
namespace {

// compact `in` (n points) by pf.flags into `out` (reserved for n points); *m = kept points (read back: the host waits here).
// With a head, `in` is the raw cloud and the scatter writes the deskewed, transformed point.
int pf_compact(dgs_handle* h, const float4* in, int64_t n, DevBuf<float4>& out, bool flatten, int64_t* m, const PfHead* head = nullptr) {
  PfScratch& pf = h->pf;
  if (!head) return compact_points(h, in, pf.flags.ptr, n, pf.blk, pf.cnt, out, flatten, m);
  return compact_scatter(h, pf.flags.ptr, n, pf.blk, pf.cnt, out, m, [&](unsigned nb) {
    hipLaunchKernelGGL(pf_head_scatter_kernel, dim3(nb), dim3(kBlock), 0, h->stream, in, pf.flags.ptr, (long long)n, *head, pf.blk.ptr, out.ptr);
  });
}

int pf_reserve_flags(dgs_handle* h, int64_t n) {
  DGS_HIP_TRY(h, h->pf.flags.reserve((size_t)std::max<int64_t>(n, 1)));
  return DGS_OK;
}

// the cloud of a k-NN pass: a copy in PfScratch::cloud with a fresh index, and its k-NN lists in PfScratch::nbr
int pf_knn(dgs_handle* h, const float4* in, int64_t n, int k) {
  CloudState& c = h->pf.cloud;
  DGS_HIP_TRY(h, c.pts.reserve((size_t)n));
  DGS_HIP_TRY(h, hipMemcpyAsync(c.pts.ptr, in, (size_t)n * sizeof(float4), hipMemcpyDeviceToDevice, h->stream));
  c.n = n;
  c.invalidate();
  return knn_lists(h, c, k, &h->pf.nbr);
}

int pf_distance(dgs_handle* h, const float4* in, int64_t n, double near_t, double far_t, DevBuf<float4>& out, int64_t* m) {
  *m = 0;
  if (n == 0) return DGS_OK;
  if (int rc = pf_reserve_flags(h, n)) return rc;
  hipLaunchKernelGGL(pf_distance_kernel, dim3(compact_blocks(n)), dim3(kBlock), 0, h->stream, in, (int)n, near_t, far_t, h->pf.flags.ptr);
  return pf_compact(h, in, n, out, false, m);
}

// the raw-scan head in front of the distance filter: one flag pass and one compaction over the raw cloud, as pf_distance
int pf_head_distance(dgs_handle* h, const float4* in, int64_t n, const PfHead& head, double near_t, double far_t, DevBuf<float4>& out, int64_t* m) {
  *m = 0;
  if (n == 0) return DGS_OK;
  if (int rc = pf_reserve_flags(h, n)) return rc;
  hipLaunchKernelGGL(pf_head_flag_kernel, dim3(compact_blocks(n)), dim3(kBlock), 0, h->stream, in, (long long)n, head, near_t, far_t, h->pf.flags.ptr);
  return pf_compact(h, in, n, out, false, m, &head);
}

int pf_radius(dgs_handle* h, const float4* in, int64_t n, double radius, int min_neighbors, int inclusive, DevBuf<float4>& out, int64_t* m) {
  *m = 0;
  const int k = min_neighbors + 1;
  if (min_neighbors < 0 || k > kKnnMax) {
    h->err = "RadiusOutlierRemoval: min_neighbors + 1 must lie in 1..32 (the k-NN of the HIP index)";
    return DGS_ERR_INVALID_ARGUMENT;
  }
  if (n == 0) return DGS_OK;
  if (n < k) return DGS_OK;   // fewer than k points: no point finds k neighbours, all are removed
  if (int rc = pf_reserve_flags(h, n)) return rc;
  if (int rc = pf_knn(h, in, n, k)) return rc;
  const CloudState& c = h->pf.cloud;
  hipLaunchKernelGGL(pf_radius_kernel, dim3(compact_blocks(n)), dim3(kBlock), 0, h->stream, make_bvh_view(c.bvh), c.pts.ptr, (int)n, k, h->pf.nbr.ptr,
                     radius * radius, inclusive, h->pf.flags.ptr);
  return pf_compact(h, in, n, out, false, m);
}

int pf_statistical(dgs_handle* h, const float4* in, int64_t n, int mean_k, double mul, int sqrt_float, DevBuf<float4>& out, int64_t* m) {
  *m = 0;
  PfScratch& pf = h->pf;
  if (mean_k < 1 || mean_k + 1 > kKnnMax) {
    h->err = "StatisticalOutlierRemoval: mean_k + 1 must lie in 2..32 (the k-NN of the HIP index)";
    return DGS_ERR_INVALID_ARGUMENT;
  }
  pf.stat_n = 0;
  if (n == 0) return DGS_OK;
  if (n <= mean_k) {
    h->err = "StatisticalOutlierRemoval: the cloud has no more points than mean_k (upstream reads past its neighbour lists)";
    return DGS_ERR_INVALID_ARGUMENT;
  }
  if (int rc = pf_reserve_flags(h, n)) return rc;
  DGS_HIP_TRY(h, pf.mean_d.reserve((size_t)n));
  DGS_HIP_TRY(h, pf.stats.reserve(4));
  const int k = mean_k + 1;
  if (int rc = pf_knn(h, in, n, k)) return rc;
  const CloudState& c = pf.cloud;
  hipLaunchKernelGGL(pf_sor_distance_kernel, dim3(compact_blocks(n)), dim3(kBlock), 0, h->stream, make_bvh_view(c.bvh), c.pts.ptr, (int)n, k, pf.nbr.ptr,
                     sqrt_float, pf.mean_d.ptr);
  hipLaunchKernelGGL(pf_sor_stats_kernel, dim3(1), dim3(kPfStatsBlock), 0, h->stream, pf.mean_d.ptr, (int)n, mul, pf.stats.ptr);
  hipLaunchKernelGGL(pf_sor_flag_kernel, dim3(compact_blocks(n)), dim3(kBlock), 0, h->stream, pf.mean_d.ptr, (int)n, pf.stats.ptr, pf.flags.ptr);
  pf.stat_n = n;
  return pf_compact(h, in, n, out, false, m);
}

int pf_normal(dgs_handle* h, const float4* in, int64_t n, const double* lidar, DevBuf<float4>& out, bool flatten, int64_t* m) {
  *m = 0;
  PfScratch& pf = h->pf;
  pf.normal_n = 0;
  if (n == 0) return DGS_OK;
  if (int rc = pf_reserve_flags(h, n)) return rc;
  DGS_HIP_TRY(h, pf.normals.reserve((size_t)n));
  DGS_HIP_TRY(h, pf.cov9.reserve((size_t)n * 9));
  const int k = (int)std::min<int64_t>(kPfNormalK, n);   // FLANN returns min(k, n) neighbours
  if (int rc = pf_knn(h, in, n, k)) return rc;
  const CloudState& c = pf.cloud;
  // ne.setViewPoint(float, float, float)
  hipLaunchKernelGGL(pf_normal_kernel, dim3(compact_blocks(n)), dim3(kBlock), 0, h->stream, make_bvh_view(c.bvh), c.pts.ptr, (int)n, k, pf.nbr.ptr,
                     (float)lidar[0], (float)lidar[1], (float)lidar[2], pf.flags.ptr, pf.normals.ptr, pf.cov9.ptr);
  pf.normal_n = n;
  return pf_compact(h, in, n, out, flatten, m);
}

int pf_begin(dgs_handle* h) {
  h->err.clear();
  DGS_HIP_TRY(h, hipSetDevice(h->device));
  return DGS_OK;
}

// the input on the device: the caller's pointer, or a copy of the host array in PfScratch::in
int pf_input(dgs_handle* h, const float* in_xyz16, int64_t n, int32_t on_device, const float4** d) {
  *d = reinterpret_cast<const float4*>(in_xyz16);
  if (on_device || n == 0) return DGS_OK;
  DGS_HIP_TRY(h, h->pf.in.reserve((size_t)n));
  DGS_HIP_TRY(h, hipMemcpyAsync(h->pf.in.ptr, in_xyz16, (size_t)n * sizeof(float4), hipMemcpyHostToDevice, h->stream));
  *d = h->pf.in.ptr;
  return DGS_OK;
}

// result of a stage / the chain to the caller's buffer; the host waits for the stream before returning
int pf_output(dgs_handle* h, const float4* src, int64_t m, float* out_xyz16, int64_t cap, int32_t on_device) {
  if (m > cap) {
    h->err = "output buffer too small for the filtered cloud";
    return DGS_ERR_INVALID_ARGUMENT;
  }
  if (m > 0)
    DGS_HIP_TRY(h, hipMemcpyAsync(out_xyz16, src, (size_t)m * sizeof(float4), on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, h->stream));
  return DGS_OK;
}

int pf_finish(dgs_handle* h, int rc) {
  if (rc != DGS_OK) {
    (void)hipStreamSynchronize(h->stream);
    return rc;
  }
  DGS_HIP_TRY(h, hipStreamSynchronize(h->stream));
  DGS_HIP_TRY(h, hipGetLastError());
  return DGS_OK;
}

bool pf_bad_io(const float* in_xyz16, int64_t n, const float* out, const int64_t* n_out, int64_t cap) {
  return !n_out || n < 0 || n > INT32_MAX || (n > 0 && !in_xyz16) || cap < 0 || (cap > 0 && !out);
}

// cloud_callback from :120 (with a head) or from :153 (without) to :160
int pf_chain(dgs_handle* h, const dgs_prefilter_params* p, const PfHead* head, const float* in_xyz16, int64_t n, int32_t in_on_device,
             const double* lidar_xyz, float* out3d, int64_t cap3d, float* out2d, int64_t cap2d, int32_t out_on_device, int64_t* n3d_out, int64_t* n2d_out) {
  if (!h || !p || p->struct_size != sizeof(dgs_prefilter_params) || pf_bad_io(in_xyz16, n, out3d, n3d_out, cap3d) || !n2d_out || cap2d < 0 ||
      (cap2d > 0 && !out2d))
    return DGS_ERR_INVALID_ARGUMENT;
  if (p->downsample_method < DGS_PF_DOWNSAMPLE_NONE || p->downsample_method > DGS_PF_DOWNSAMPLE_APPROX_VOXELGRID ||
      p->outlier_removal_method < DGS_PF_OUTLIER_NONE || p->outlier_removal_method > DGS_PF_OUTLIER_RADIUS ||
      (p->downsample_method != DGS_PF_DOWNSAMPLE_NONE && !(p->downsample_resolution > 0)))
    return DGS_ERR_INVALID_ARGUMENT;
  *n3d_out = 0;
  *n2d_out = 0;
  if (int rc = pf_begin(h)) return rc;
  const double zero3[3] = {0.0, 0.0, 0.0};
  const double* lidar = lidar_xyz ? lidar_xyz : zero3;
  PfScratch& pf = h->pf;
  pf.stat_n = pf.normal_n = 0;
  if (n == 0) return DGS_OK;   // cloud_callback returns on an empty cloud (:116-118): nothing is published
  const float4* in = nullptr;
  int rc = pf_input(h, in_xyz16, n, in_on_device, &in);
  // 1. distance filter (applied whatever use_distance_filter says, :153), behind the raw-scan head when there is one
  int64_t n1 = 0;
  if (rc == DGS_OK)
    rc = head ? pf_head_distance(h, in, n, *head, p->distance_near_thresh, p->distance_far_thresh, pf.a, &n1)
              : pf_distance(h, in, n, p->distance_near_thresh, p->distance_far_thresh, pf.a, &n1);
  // 2. down-sampling: the voxel filters' own code paths (ndt_voxel.hip)
  const float4* s2 = pf.a.ptr;
  int64_t n2 = n1;
  if (rc == DGS_OK && n1 > 0 && p->downsample_method != DGS_PF_DOWNSAMPLE_NONE) {
    if (pf.b.reserve((size_t)n1) != hipSuccess) { h->err = "hipMalloc failed"; return pf_finish(h, DGS_ERR_HIP); }
    const float leaf = (float)p->downsample_resolution;   // setLeafSize(float, float, float)
    rc = p->downsample_method == DGS_PF_DOWNSAMPLE_VOXELGRID ? voxel_grid_filter(h, pf.a.ptr, n1, leaf, pf.b.ptr, n1, &n2)
                                                             : approx_voxel_grid_filter(h, pf.a.ptr, n1, leaf, pf.b.ptr, n1, &n2);
    s2 = pf.b.ptr;
  }
  // 3. outlier removal -> /filtered_points
  const float4* s3 = s2;
  int64_t n3 = n2;
  if (rc == DGS_OK && p->outlier_removal_method == DGS_PF_OUTLIER_STATISTICAL) {
    rc = pf_statistical(h, s2, n2, p->statistical_mean_k, p->statistical_stddev, p->statistical_sqrt_float, pf.c, &n3);
    s3 = pf.c.ptr;
  } else if (rc == DGS_OK && p->outlier_removal_method == DGS_PF_OUTLIER_RADIUS) {
    rc = pf_radius(h, s2, n2, p->radius_radius, p->radius_min_neighbors, p->radius_inclusive, pf.c, &n3);
    s3 = pf.c.ptr;
  }
  // 4. height filter, 5. normal filter + 6. flatten (the scatter of the normal pass writes z = 0)
  int64_t n4 = 0, n5 = 0;
  if (rc == DGS_OK && n3 > 0) {
    if ((rc = pf_reserve_flags(h, n3)) == DGS_OK) {
      hipLaunchKernelGGL(pf_height_kernel, dim3(compact_blocks(n3)), dim3(kBlock), 0, h->stream, s3, (int)n3, lidar[2], pf.flags.ptr);
      rc = pf_compact(h, s3, n3, pf.d, false, &n4);
    }
  }
  if (rc == DGS_OK && n4 > 0) rc = pf_normal(h, pf.d.ptr, n4, lidar, pf.e, true, &n5);
  if (rc == DGS_OK) {
    *n3d_out = n3;
    *n2d_out = n5;
    rc = pf_output(h, s3, n3, out3d, cap3d, out_on_device);
    if (rc == DGS_OK) rc = pf_output(h, pf.e.ptr, n5, out2d, cap2d, out_on_device);
  }
  return pf_finish(h, rc);
}

}  // namespace

void prefilter_release(dgs_handle* h) {
  PfScratch& pf = h->pf;
  for (DevBuf<float4>* b : {&pf.in, &pf.a, &pf.b, &pf.c, &pf.d, &pf.e, &pf.normals}) b->release();
  pf.flags.release(); pf.blk.release(); pf.cnt.release(); pf.nbr.release(); pf.mean_d.release(); pf.stats.release(); pf.cov9.release();
  pf.cloud.release();
  pf.stat_n = pf.normal_n = 0;
}

}  // namespace dgs

using namespace dgs;

extern "C" {

int dgs_prefilter_params_init(dgs_prefilter_params* p) {
  if (!p) return DGS_ERR_INVALID_ARGUMENT;
  std::memset(p, 0, sizeof(*p));
  p->struct_size = sizeof(*p);
  p->downsample_method = DGS_PF_DOWNSAMPLE_VOXELGRID;
  p->downsample_resolution = 0.1;
  p->outlier_removal_method = DGS_PF_OUTLIER_STATISTICAL;
  p->statistical_mean_k = 20;
  p->statistical_stddev = 1.0;
  p->radius_radius = 0.8;
  p->radius_min_neighbors = 2;
  p->use_distance_filter = 1;
  p->distance_near_thresh = 1.0;
  p->distance_far_thresh = 100.0;
  p->radius_inclusive = 1;
  p->statistical_sqrt_float = 1;
  return DGS_OK;
}

int dgs_prefilter(dgs_handle* h, const dgs_prefilter_params* p, const float* in_xyz16, int64_t n, int32_t in_on_device, const double* lidar_xyz,
                  float* out3d, int64_t cap3d, float* out2d, int64_t cap2d, int32_t out_on_device, int64_t* n3d_out, int64_t* n2d_out) {
  return pf_chain(h, p, nullptr, in_xyz16, n, in_on_device, lidar_xyz, out3d, cap3d, out2d, cap2d, out_on_device, n3d_out, n2d_out);
}

int dgs_prefilter_scan_params_init(dgs_prefilter_scan_params* p) {
  if (!p) return DGS_ERR_INVALID_ARGUMENT;
  std::memset(p, 0, sizeof(*p));
  p->struct_size = sizeof(*p);
  p->scan_period = 0.1;
  for (int a = 0; a < 4; a++) p->transform[5 * a] = 1.0;
  p->deskew_norm_order = DGS_PF_NORM_PAIRS_XY_ZW;
  p->transform_sets_w = 1;
  return DGS_OK;
}

int dgs_prefilter_scan(dgs_handle* h, const dgs_prefilter_params* p, const dgs_prefilter_scan_params* sp, const float* in_xyz16, int64_t n,
                       int32_t in_on_device, float* out3d, int64_t cap3d, float* out2d, int64_t cap2d, int32_t out_on_device, int64_t* n3d_out,
                       int64_t* n2d_out, double* lidar_xyz_out) {
  PfHead head;
  double lidar[3];
  if (!pf_make_head(sp, &head, lidar)) return DGS_ERR_INVALID_ARGUMENT;
  if (lidar_xyz_out) std::memcpy(lidar_xyz_out, lidar, sizeof(lidar));
  return pf_chain(h, p, &head, in_xyz16, n, in_on_device, lidar, out3d, cap3d, out2d, cap2d, out_on_device, n3d_out, n2d_out);
}

int dgs_prefilter_deskew(dgs_handle* h, const dgs_prefilter_scan_params* sp, const float* in_xyz16, int64_t n, int32_t in_on_device, float* out_xyz16,
                         int64_t cap, int32_t out_on_device, int64_t* n_out) {
  PfHead head;
  double lidar[3];
  if (!h || !pf_make_head(sp, &head, lidar) || pf_bad_io(in_xyz16, n, out_xyz16, n_out, cap)) return DGS_ERR_INVALID_ARGUMENT;
  *n_out = 0;
  if (int rc = pf_begin(h)) return rc;
  if (n == 0) return DGS_OK;
  const float4* in = nullptr;
  int rc = pf_input(h, in_xyz16, n, in_on_device, &in);
  if (rc == DGS_OK && h->pf.a.reserve((size_t)n) != hipSuccess) { h->err = "hipMalloc failed"; rc = DGS_ERR_HIP; }
  if (rc == DGS_OK) {
    hipLaunchKernelGGL(pf_head_apply_kernel, dim3(compact_blocks(n)), dim3(kBlock), 0, h->stream, in, (long long)n, head, h->pf.a.ptr);
    *n_out = n;
    rc = pf_output(h, h->pf.a.ptr, n, out_xyz16, cap, out_on_device);
  }
  return pf_finish(h, rc);
}

int dgs_prefilter_distance(dgs_handle* h, const float* in_xyz16, int64_t n, int32_t in_on_device, double near_t, double far_t, float* out_xyz16,
                           int64_t cap, int32_t out_on_device, int64_t* n_out) {
  if (!h || pf_bad_io(in_xyz16, n, out_xyz16, n_out, cap)) return DGS_ERR_INVALID_ARGUMENT;
  *n_out = 0;
  if (int rc = pf_begin(h)) return rc;
  const float4* in = nullptr;
  int64_t m = 0;
  int rc = pf_input(h, in_xyz16, n, in_on_device, &in);
  if (rc == DGS_OK) rc = pf_distance(h, in, n, near_t, far_t, h->pf.a, &m);
  if (rc == DGS_OK) { *n_out = m; rc = pf_output(h, h->pf.a.ptr, m, out_xyz16, cap, out_on_device); }
  return pf_finish(h, rc);
}

int dgs_prefilter_radius(dgs_handle* h, const float* in_xyz16, int64_t n, int32_t in_on_device, double radius, int32_t min_neighbors, int32_t inclusive,
                         float* out_xyz16, int64_t cap, int32_t out_on_device, int64_t* n_out) {
  if (!h || pf_bad_io(in_xyz16, n, out_xyz16, n_out, cap)) return DGS_ERR_INVALID_ARGUMENT;
  *n_out = 0;
  if (int rc = pf_begin(h)) return rc;
  const float4* in = nullptr;
  int64_t m = 0;
  int rc = pf_input(h, in_xyz16, n, in_on_device, &in);
  if (rc == DGS_OK) rc = pf_radius(h, in, n, radius, min_neighbors, inclusive, h->pf.c, &m);
  if (rc == DGS_OK) { *n_out = m; rc = pf_output(h, h->pf.c.ptr, m, out_xyz16, cap, out_on_device); }
  return pf_finish(h, rc);
}

int dgs_prefilter_statistical(dgs_handle* h, const float* in_xyz16, int64_t n, int32_t in_on_device, int32_t mean_k, double stddev_mul,
                              int32_t sqrt_float, float* out_xyz16, int64_t cap, int32_t out_on_device, int64_t* n_out) {
  if (!h || pf_bad_io(in_xyz16, n, out_xyz16, n_out, cap)) return DGS_ERR_INVALID_ARGUMENT;
  *n_out = 0;
  if (int rc = pf_begin(h)) return rc;
  const float4* in = nullptr;
  int64_t m = 0;
  int rc = pf_input(h, in_xyz16, n, in_on_device, &in);
  if (rc == DGS_OK) rc = pf_statistical(h, in, n, mean_k, stddev_mul, sqrt_float, h->pf.c, &m);
  if (rc == DGS_OK) { *n_out = m; rc = pf_output(h, h->pf.c.ptr, m, out_xyz16, cap, out_on_device); }
  return pf_finish(h, rc);
}

int dgs_prefilter_normal(dgs_handle* h, const float* in_xyz16, int64_t n, int32_t in_on_device, const double* lidar_xyz, float* out_xyz16,
                         int64_t cap, int32_t out_on_device, int64_t* n_out) {
  if (!h || pf_bad_io(in_xyz16, n, out_xyz16, n_out, cap)) return DGS_ERR_INVALID_ARGUMENT;
  *n_out = 0;
  if (int rc = pf_begin(h)) return rc;
  const double zero3[3] = {0.0, 0.0, 0.0};
  const float4* in = nullptr;
  int64_t m = 0;
  int rc = pf_input(h, in_xyz16, n, in_on_device, &in);
  if (rc == DGS_OK) rc = pf_normal(h, in, n, lidar_xyz ? lidar_xyz : zero3, h->pf.e, false, &m);
  if (rc == DGS_OK) { *n_out = m; rc = pf_output(h, h->pf.e.ptr, m, out_xyz16, cap, out_on_device); }
  return pf_finish(h, rc);
}

int dgs_prefilter_get_statistics(dgs_handle* h, float* mean_distances, int64_t capacity, double* stats4, int64_t* n) {
  if (!h || !n || capacity < 0) return DGS_ERR_INVALID_ARGUMENT;
  if (int rc = pf_begin(h)) return rc;
  const int64_t m = h->pf.stat_n;
  *n = m;
  if (m == 0) return DGS_OK;
  if (mean_distances && capacity >= m)
    DGS_HIP_TRY(h, hipMemcpyAsync(mean_distances, h->pf.mean_d.ptr, (size_t)m * sizeof(float), hipMemcpyDeviceToHost, h->stream));
  if (stats4) {
    DGS_HIP_TRY(h, hipMemcpyAsync(stats4, h->pf.stats.ptr, 3 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    stats4[3] = (double)m;
  }
  DGS_HIP_TRY(h, hipStreamSynchronize(h->stream));
  return DGS_OK;
}

int dgs_prefilter_get_normals(dgs_handle* h, float* normals4, float* cov9, int64_t capacity, int64_t* n) {
  if (!h || !n || capacity < 0) return DGS_ERR_INVALID_ARGUMENT;
  if (int rc = pf_begin(h)) return rc;
  const int64_t m = h->pf.normal_n;
  *n = m;
  if (m == 0 || capacity < m) return DGS_OK;
  if (normals4) DGS_HIP_TRY(h, hipMemcpyAsync(normals4, h->pf.normals.ptr, (size_t)m * sizeof(float4), hipMemcpyDeviceToHost, h->stream));
  if (cov9) DGS_HIP_TRY(h, hipMemcpyAsync(cov9, h->pf.cov9.ptr, (size_t)m * 9 * sizeof(float), hipMemcpyDeviceToHost, h->stream));
  DGS_HIP_TRY(h, hipStreamSynchronize(h->stream));
  return DGS_OK;
}

}  // extern "C"
