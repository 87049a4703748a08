// K4 knn_covariance.  FastGICP::calculate_covariances for FAST_GICP / FAST_VGICP: the exact k-NN sets of every point in its own cloud
// (knn_lists.hip), the covariance of the neighbours in double, regularised (gicp_cov_from_knn_kernel; in upstream's operation order:
// gicp_cov_ordered.hip).  Cached on the cloud under (k, regularisation): ensure_covariance.  The kernels' body: gicp_cov_body.h; the same
// pass over many clouds in one pair of launches: cov_batch.hip.
#include <cmath>
#include <cstdint>
#include <vector>

#include "gicp_cov_body.h"
#include "handle.h"
#include "nn_group.h"
#include "small_linalg.h"

namespace dgs {

__global__ __launch_bounds__(kBlock) void gicp_cov_from_knn_kernel(const BvhView b, const float4* __restrict__ pts, const int n, const int k, const int method,
                                                                   const int* __restrict__ nbr, double* __restrict__ cov6) {
  gicp_cov_from_knn_body<kKnnSlots>(b, pts, n, k, method, nbr, cov6, (int)blockIdx.x);
}
// 32 < k <= 64: 8 slots per lane, table stride kKnnMaxWide; the same sums in the same order per lane (slot q * 8 + sub, q ascending), then the same tree
__global__ __launch_bounds__(kBlock) void gicp_cov_from_knn_wide_kernel(const BvhView b, const float4* __restrict__ pts, const int n, const int k, const int method,
                                                                        const int* __restrict__ nbr, double* __restrict__ cov6) {
  gicp_cov_from_knn_body<kKnnSlotsWide>(b, pts, n, k, method, nbr, cov6, (int)blockIdx.x);
}

// The covariances of `c` under the handle's (k, regularisation), computed unless the cloud holds them already.
int ensure_covariance(dgs_handle* h, CloudState& c) {
  const int k = h->prm.gicp_correspondence_randomness, reg = h->prm.gicp_regularization;
  if (c.cov_valid && c.cov_k == k && c.cov_reg == reg) return DGS_OK;
  if (k > kKnnMaxWide) {
    h->err = kKnnTooWide;
    return DGS_ERR_UNSUPPORTED;
  }
  if (!c.bvh.valid) {
    int rc = bvh_build(h, c.bvh, c.pts.ptr, c.n, nullptr, h->batch_kd && &c == h->tgt);
    if (rc) return rc;
  }
  DGS_HIP_TRY(h, c.cov.reserve((size_t)c.n * 6));
  const BvhView v = make_bvh_view(c.bvh);
  int slot = prof_begin(h, DGS_K_GICP_COVARIANCE);
  int stride = 0;
  int rc = knn_lists(h, c, k, nullptr, &stride);
  if (rc) return rc;
  const dim3 cov_grid((unsigned)(((int64_t)c.n + kCovPerBlock - 1) / kCovPerBlock));
  const int cov_method = reg | (h->prm.gicp_cov_jacobi_svd ? 0x100 : 0);
  if (h->prm.gicp_cov_jacobi_svd == DGS_GICP_COV_UPSTREAM_ORDER)   // ordered lists, sequential sums, JacobiSVD: gicp_cov_ordered.hip
    gicp_cov_upstream_order(h, v, c, k, reg, h->knn_nbr.ptr, stride);
  else if (stride == kKnnMaxWide)
    hipLaunchKernelGGL(gicp_cov_from_knn_wide_kernel, cov_grid, dim3(kBlock), 0, h->stream, v, c.pts.ptr, (int)c.n, k, cov_method, h->knn_nbr.ptr, c.cov.ptr);
  else
    hipLaunchKernelGGL(gicp_cov_from_knn_kernel, cov_grid, dim3(kBlock), 0, h->stream, v, c.pts.ptr, (int)c.n, k, cov_method, h->knn_nbr.ptr, c.cov.ptr);
  prof_end(h, DGS_K_GICP_COVARIANCE, slot);
  DGS_HIP_TRY(h, hipGetLastError());
#ifdef DGS_KNN_STATS
  if (knn_uses_leaf_search(h, k)) {
    int st[8];
    (void)hipMemcpyAsync(st, h->knn_stats.ptr, sizeof(st), hipMemcpyDeviceToHost, h->stream);
    (void)hipStreamSynchronize(h->stream);
    const double w = std::max(st[0], 1);
    fprintf(stderr, "[knn] n %lld waves %d answered cooperatively %d (%.2f %%) gather rounds per wave %.3f waves that retried %d; per wave (us): window bounds %.2f, "
            "leaf walk %.2f, selection %.2f, whole %.2f\n", (long long)c.n, st[0], st[1], 100.0 * st[1] / w, (double)st[2] / w, st[3], st[4] * 0.01 / w, st[5] * 0.01 / w,
            st[6] * 0.01 / w, st[7] * 0.01 / w);
  }
#endif
  c.cov_valid = true;
  c.cov_k = k;
  c.cov_reg = reg;
  return DGS_OK;
}

// Test hook: regularised covariances (9 doubles per point, row-major) of the source (which = 0) or target (1) cloud.
int gicp_covariances(dgs_handle* h, int which, double* host_out9, int64_t n) {
  int rc = which ? ensure_covariance(h, *h->tgt) : ensure_covariance(h, *h->src);
  if (rc) return rc;
  std::vector<double> c6((size_t)n * 6);
  DGS_HIP_TRY(h, hipStreamSynchronize(h->stream));
  DGS_HIP_TRY(h, hipMemcpy(c6.data(), which ? h->tgt->cov.ptr : h->src->cov.ptr, c6.size() * sizeof(double), hipMemcpyDeviceToHost));
  for (int64_t i = 0; i < n; i++) {
    const double* c = c6.data() + i * 6;
    double* o = host_out9 + i * 9;
    o[0] = c[0]; o[1] = c[1]; o[2] = c[2]; o[3] = c[1]; o[4] = c[3]; o[5] = c[4]; o[6] = c[2]; o[7] = c[4]; o[8] = c[5];
  }
  return DGS_OK;
}

}  // namespace dgs
