// Exact k-NN lists of every point of a cloud in the cloud itself (knn_lists): the search half of FastGICP::calculate_covariances
// (gicp_cov.hip, gicp_cov_ordered.hip), of GICP_HIP's covariances (pcl_gicp.hip), of the prefilter's outlier and normal passes
// (prefilter.hip) and of floor detection's normals (floor_detection.hip).  Two searches over the 8-ary AABB index of nn_bvh.hip, the same
// sets from either: one wave per index leaf (gicp_knn_leaf_kernel, its body in knn_leaf.h) and the per-query walk with warm bounds
// (gicp_knn_kernel).  The same search over many clouds in one launch: cov_batch.hip.
#include <algorithm>
#include <cmath>
#include <cstdint>

#include "cov_batch_plan.h"
#include "handle.h"
#include "knn_leaf.h"
#include "nn_group.h"

namespace dgs {

// The per-query walk.  The search alone, so its registers are the k-NN set and the walk, nothing of the covariance; every wave takes a
// contiguous stretch of the cloud in the index's own (Hilbert) order, 8 adjacent points per round (the 8 groups walk nearly the same
// nodes), and each round's searches start from a bound on the k-th distance taken from the previous round: all k neighbours of q' lie
// within r_k(q') + |q - q'| of q (pruning only: same sets).  It writes the set of every point to `nbr` (knn_write_list).
// SLOTS = 4: k <= 32, table stride kKnnMax; SLOTS = 8: k <= 64, table stride kKnnMaxWide (the wide kernels below).
template <int SLOTS>
__device__ __forceinline__ void gicp_knn_body(const BvhView& b, const int n, const int k, const int run, int* __restrict__ nbr) {
  const int sub = threadIdx.x & 7;
  const int wave = blockIdx.x * (kBlock / kWave) + (threadIdx.x >> 6);
  const int first = wave * (8 * run) + ((threadIdx.x & 63) >> 3);
  float px = 0.f, py = 0.f, pz = 0.f, prev_kth = INFINITY;
  bool prev_found = false;
  for (int r = 0; r < run; r++) {
    const int pos = first + r * 8;
    if (__all(pos >= n)) break;   // wave-uniform: the stretch is past the end of the cloud
    const float4 q = (pos < n) ? b.sorted[pos] : make_float4(0.f, 0.f, 0.f, 0.f);
    const int i = (pos < n) ? (int)__float_as_uint(q.w) : -1;
    const bool alive = pos < n && i >= 0 && i < n;
    const float bound = nn_warm_bound_round(prev_kth, prev_found, q.x, q.y, q.z, px, py, pz);
    KnnListT<SLOTS> L;
    knn_query_group(b, q.x, q.y, q.z, alive, k, L, bound);
    const unsigned long long worst = knn_largest(L);
    prev_kth = __uint_as_float((unsigned)(worst >> 32));
    prev_found = alive && prev_kth < INFINITY;
    px = q.x; py = q.y; pz = q.z;
    if (alive) knn_write_list(L, pos, sub, k, nbr);
  }
}
__global__ __launch_bounds__(kBlock) void gicp_knn_kernel(const BvhView b, const int n, const int k, const int run, int* __restrict__ nbr) {
  gicp_knn_body<kKnnSlots>(b, n, k, run, nbr);
}
__global__ __launch_bounds__(kBlock) void gicp_knn_wide_kernel(const BvhView b, const int n, const int k, const int run, int* __restrict__ nbr) {
  gicp_knn_body<kKnnSlotsWide>(b, n, k, run, nbr);
}

// The wave-per-leaf search over one cloud (knn_leaf.h).
__global__ __launch_bounds__(kBlock, DGS_KNN_WAVES) void gicp_knn_leaf_kernel(const BvhView b, const int n, const int k, const int parts, int* __restrict__ nbr, int* __restrict__ stats) {
  gicp_knn_leaf_body<kKnnSlots>(b, n, k, parts, nbr, stats, (int)blockIdx.x);
}
// 32 < k <= 64.  The window of step (a) stays 8 leaves = 64 points, one per lane: it bounds the k-th distance of a query by its k-th
// smallest distance to those 64 points, which for k near 64 is the far edge of the window -- a loose bound, more gathered leaves, more
// retries with a scaled bound (the sets do not depend on it).  Whether this or the per-query walk serves wide k: knn_lists.
// The narrow kernel's occupancy bound on purpose: under 4 waves per SIMD (128 registers) this form spills 24 registers (100 bytes of scratch
// per lane), under 3 waves it needs 151 registers and spills nothing -- and is 9 to 16 % slower at every k measured (33 .. 60, both bench
// clouds: 0.136 against 0.118 ms per 65,536-point cloud at k = 33, 0.178 against 0.154 ms at k = 60).
__global__ __launch_bounds__(kBlock, DGS_KNN_WAVES) void gicp_knn_leaf_wide_kernel(const BvhView b, const int n, const int k, const int parts, int* __restrict__ nbr, int* __restrict__ stats) {
  gicp_knn_leaf_body<kKnnSlotsWide>(b, n, k, parts, nbr, stats, (int)blockIdx.x);
}

// Exact k-NN of every point of `c` in `c` itself (the point included) -> h->knn_nbr (nbr[pos * stride + slot], pos in c.bvh's order).
// Shared by FAST_GICP's covariances, GICP_HIP's (pcl_gicp.hip), the prefilter (prefilter.hip) and floor detection (floor_detection.hip),
// the last two with a buffer of their own.
// Two widths.  A caller that passes `stride` reads the table at the stride it gets back: kKnnMax (32) for k <= 32 -- the kernels every
// earlier release ran, unchanged -- and kKnnMaxWide (64) for 32 < k <= 64, the wide kernels.  Only the GICP family's covariance passes do
// (ensure_covariance in gicp_cov.hip, ensure_pcov in pcl_gicp.hip).  A caller that does not -- the prefilter's pf_radius / pf_statistical / normals and
// floor detection -- keeps k <= 32 and stride 32: their limits, messages and kernels are as they were.
// Which search makes the lists: the wave-per-leaf search at either width (measured 10 to 13 times faster than the per-query walk with
// warm bounds at every k in 33 .. 64 on both bench clouds); DGS_KNN_LEAF=0 selects the walk for every k,
// DGS_KNN_LEAF_WIDE=0 for wide k only.
// The shape of a cloud's search -- waves per leaf, rounds per wave -- is cov_batch_plan.h's, shared with the batched pass (cov_batch.hip).
bool knn_uses_leaf_search(const dgs_handle* h, const int k) { return h->knn_leaf && (k <= kKnnMax || h->knn_leaf_wide); }
int knn_lists(dgs_handle* h, CloudState& c, int k, DevBuf<int>* out, int* stride) {
  DevBuf<int>& nbr = out ? *out : h->knn_nbr;
  if (k > (stride ? kKnnMaxWide : kKnnMax)) {
    h->err = stride ? kKnnTooWide : "reg_correspondence_randomness > 32 is not supported by the HIP k-NN";
    return DGS_ERR_UNSUPPORTED;
  }
  const bool wide = k > kKnnMax;
  const int width = wide ? kKnnMaxWide : kKnnMax;
  if (stride) *stride = width;
  if (!c.bvh.valid) {
    // the target of a batch is searched by every candidate at every linearisation: worth the slower k-d ordered build (nn_bvh.hip)
    int rc = bvh_build(h, c.bvh, c.pts.ptr, c.n, nullptr, h->batch_kd && &c == h->tgt);
    if (rc) return rc;
  }
  const BvhView v = make_bvh_view(c.bvh);
  DGS_HIP_TRY(h, nbr.reserve((size_t)c.n * width));
  DGS_HIP_TRY(h, h->knn_stats.reserve(8));
  if (knn_uses_leaf_search(h, k)) {
    const int parts = covplan::knn_leaf_parts(c.n, h->knn_parts);
#ifdef DGS_KNN_STATS
    (void)hipMemsetAsync(h->knn_stats.ptr, 0, 8 * sizeof(int), h->stream);
#endif
    const dim3 grid((unsigned)covplan::knn_leaf_blocks(c.n, parts));
    if (wide)
      hipLaunchKernelGGL(gicp_knn_leaf_wide_kernel, grid, dim3(kBlock), 0, h->stream, v, (int)c.n, k, parts, nbr.ptr, h->knn_stats.ptr);
    else
      hipLaunchKernelGGL(gicp_knn_leaf_kernel, grid, dim3(kBlock), 0, h->stream, v, (int)c.n, k, parts, nbr.ptr, h->knn_stats.ptr);
  } else {
    const int run = covplan::knn_walk_run(c.n, h->knn_rounds, h->knn_min_waves);
    const dim3 grid((unsigned)covplan::knn_walk_blocks(c.n, run));
    if (wide)
      hipLaunchKernelGGL(gicp_knn_wide_kernel, grid, dim3(kBlock), 0, h->stream, v, (int)c.n, k, run, nbr.ptr);
    else
      hipLaunchKernelGGL(gicp_knn_kernel, grid, dim3(kBlock), 0, h->stream, v, (int)c.n, k, run, nbr.ptr);
  }
  return DGS_OK;
}

}  // namespace dgs
