// K4 in upstream order: dgs_params.gicp_cov_jacobi_svd = DGS_GICP_COV_UPSTREAM_ORDER.
//
// fast_gicp::FastGICP::calculate_covariances sums a point's k neighbours one after another, in the order its kd-tree returns them
// (ascending squared distance), and hands the 3 x 3 result to Eigen::JacobiSVD.  On a rank-deficient neighbourhood (duplicated points,
// points on a line) JacobiSVD's 2 eps maxDiag rotation threshold turns the last bit of that matrix into another basis of the null
// space, so the regularised covariance is upstream's only if the sums are upstream's bit for bit.  gicp_cov_from_knn_kernel (gicp_cov.hip)
// reduces over 8 lanes in a tree; this kernel restates the sequence of the CPU restatement of calculate_covariances (the test suite's
// checker) operation for operation, every one individually rounded: the whole file is compiled without contraction (Makefile).
//
// One wave takes kOrdPerWave points, two phases.
//  (1) rounds of 8 points, 8 lanes per point: every lane gathers its <= 4 neighbours (slots s * 8 + sub of the k-NN list), recomputes the
//      float squared distance as the kd-tree does ((dx dx + dy dy) + dz dz), and ranks its (distance, index) keys among the group's 32 by
//      counting the smaller ones -- the keys are distinct because the indices are, so the ranks of the k used slots are 0 .. k - 1.  The
//      coordinates go to LDS at their rank: [coordinate][rank][point], so that phase 2's lanes read consecutive words (no bank conflict).
//      Slots that found nothing (a cloud smaller than k) sort last and hold zeros: upstream's 4 x k matrix keeps zero columns there.
//  (2) lane t takes point t: mean and the nine products summed over the k columns in order, all double, read from LDS (k dependent
//      gathers from L2 per lane otherwise), then the regularisation.
#include "handle.h"
#include "nn_group.h"
#include "small_linalg.h"

namespace dgs {

// The regularisation of calc_covariances in its operation order: std::max(a, b) = (a < b) ? b : a, U diag V^T summed left to right from 0.
__device__ static void regularize_cov_upstream(const double* cov9, const int method, double* out6) {
  double C[9];
  if (method == DGS_GICP_REG_NONE) {
    for (int a = 0; a < 9; a++) C[a] = cov9[a];
  } else if (method == DGS_GICP_REG_FROBENIUS) {
    const double lambda = 1e-3;
    double A[9], Ai[9];
    for (int a = 0; a < 9; a++) A[a] = cov9[a] + ((a % 4 == 0) ? lambda : 0.0);
    inv3_d(A, Ai);
    double nrm = 0;
    for (int a = 0; a < 9; a++) nrm += Ai[a] * Ai[a];
    nrm = sqrt(nrm);
    for (int a = 0; a < 9; a++) Ai[a] /= nrm;
    inv3_d(Ai, C);
  } else {
    double U[9], V[9], sv[3], vals[3];
    jacobi_svd3_d(cov9, U, V, sv);
    if (method == DGS_GICP_REG_PLANE) {
      vals[0] = 1; vals[1] = 1; vals[2] = 1e-3;
    } else if (method == DGS_GICP_REG_MIN_EIG) {
      for (int a = 0; a < 3; a++) vals[a] = (sv[a] < 1e-3) ? 1e-3 : sv[a];
    } else {
      for (int a = 0; a < 3; a++) { const double s = sv[a] / sv[0]; vals[a] = (s < 1e-3) ? 1e-3 : s; }
    }
    for (int r = 0; r < 3; r++)
      for (int c = r; c < 3; c++) {
        double s = 0;
        for (int a = 0; a < 3; a++) s += U[r * 3 + a] * vals[a] * V[c * 3 + a];
        C[r * 3 + c] = s;
      }
  }
  out6[0] = C[0]; out6[1] = C[1]; out6[2] = C[2]; out6[3] = C[4]; out6[4] = C[5]; out6[5] = C[8];
}

// Points per wave = rounds * 8.  As in gicp_cov_from_knn_kernel, 8 rounds would fill every lane of phase 2 but leave a 65,536-point cloud
// with one wave per SIMD; 4 rounds keep two, and a wave's LDS at 3 * 32 * 32 * 4 = 12 KiB for k = 32 (7.5 KiB for k = 20): 48 KiB per
// workgroup at most, under the 64 KiB a launch may ask for without an attribute, three to five workgroups per CU.
#ifndef DGS_COV_ORDERED_ROUNDS
#define DGS_COV_ORDERED_ROUNDS 4
#endif
constexpr int kOrdRounds = DGS_COV_ORDERED_ROUNDS, kOrdPerWave = kOrdRounds * 8, kOrdPerBlock = kOrdPerWave * (kBlock / kWave);
static_assert(kOrdPerWave <= kWave, "phase 2 takes one lane per point");
// The wide form (32 < k <= 64: 8 slots per lane, table stride kKnnMaxWide) takes 2 rounds = 16 points per wave: 3 * 64 * 16 * 4 = 12 KiB of
// LDS per wave at k = 64, the 48 KiB per workgroup of the narrow form at k = 32 (4 rounds would ask for 96 KiB).
constexpr int kOrdRoundsWide = 2, kOrdPerWaveWide = kOrdRoundsWide * 8, kOrdPerBlockWide = kOrdPerWaveWide * (kBlock / kWave);

// SLOTS slots per lane (table stride SLOTS * 8), ROUNDS rounds of 8 points per wave
template <int SLOTS, int ROUNDS>
__device__ __forceinline__ void gicp_cov_ordered_body(const BvhView& b, const float4* __restrict__ pts, const int n, const int k, const int method,
                                                      const int* __restrict__ nbr, double* __restrict__ cov6) {
  constexpr int kPerWave = ROUNDS * 8;                // points of a wave in this instantiation
  extern __shared__ float s_xyz[];                    // [wave][coordinate][rank < k][point of the wave]
  __shared__ int s_i[kBlock / kWave][kPerWave];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, sub = lane & 7, grp = lane >> 3;
  const int wave_base = (blockIdx.x * (kBlock / kWave) + wv) * kPerWave;   // first point (position in index order) of this wave
  if (wave_base >= n) return;   // wave-uniform; the kernel has no workgroup barrier
  float* __restrict__ sw = s_xyz + (size_t)wv * 3 * k * kPerWave;
  float* __restrict__ sx = sw, * __restrict__ sy = sw + k * kPerWave, * __restrict__ sz = sw + 2 * k * kPerWave;
#pragma unroll 1
  for (int r = 0; r < ROUNDS; r++) {
    const int pt = r * 8 + grp, pos = wave_base + pt;
    const float4 q = (pos < n) ? b.sorted[pos] : make_float4(0.f, 0.f, 0.f, 0.f);
    const int i = (pos < n) ? (int)__float_as_uint(q.w) : -1;
    const bool live = i >= 0 && i < n;
    unsigned long long key[SLOTS];
    float cx[SLOTS], cy[SLOTS], cz[SLOTS];
#pragma unroll
    for (int s = 0; s < SLOTS; s++) {
      const int slot = s * 8 + sub;
      const bool used = slot < k;
      int j = (live && used) ? nbr[(size_t)pos * (SLOTS * 8) + slot] : -1;
      if ((unsigned)j >= (unsigned)n) j = -1;
      const float4 p = (j >= 0) ? pts[j] : make_float4(0.f, 0.f, 0.f, 0.f);
      cx[s] = p.x; cy[s] = p.y; cz[s] = p.z;
      const float dx = q.x - p.x, dy = q.y - p.y, dz = q.z - p.z;
      const float d = (dx * dx + dy * dy) + dz * dz;   // the kd-tree's distance: every step rounded to float
      // unused slots: the largest key, below nothing; slots that found nothing: after every distance, in slot order
      key[s] = !used ? ~0ull : ((unsigned long long)((j >= 0) ? __float_as_uint(d) : 0xFFFFFFFFu) << 32) | (unsigned)((j >= 0) ? j : slot);
    }
    int rank[SLOTS];
#pragma unroll
    for (int s = 0; s < SLOTS; s++) rank[s] = 0;
#pragma unroll
    for (int l = 0; l < 8; l++)
#pragma unroll
      for (int t = 0; t < SLOTS; t++) {
        const unsigned long long o = __shfl(key[t], l, 8);
#pragma unroll
        for (int s = 0; s < SLOTS; s++) rank[s] += (o < key[s]) ? 1 : 0;
      }
#pragma unroll
    for (int s = 0; s < SLOTS; s++)
      if (s * 8 + sub < k && rank[s] < k) {   // rank < k always (k distinct keys below every unused one); the test keeps a store inside the wave's LDS whatever nbr holds
        const int at = rank[s] * kPerWave + pt;
        sx[at] = cx[s]; sy[at] = cy[s]; sz[at] = cz[s];
      }
    if (sub == 0) s_i[wv][pt] = live ? i : -1;
  }
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_s_waitcnt(0xc07f);   // lgkmcnt(0): the wave's LDS stores have landed
  if (lane >= kPerWave) return;
  const int i = s_i[wv][lane];
  if (i < 0) return;
  const double kk = (double)k;
  double m0 = 0, m1 = 0, m2 = 0;
#pragma unroll 4
  for (int j = 0; j < k; j++) {   // columns that found nothing add +0: the same bits as leaving them out
    m0 += (double)sx[j * kPerWave + lane];
    m1 += (double)sy[j * kPerWave + lane];
    m2 += (double)sz[j * kPerWave + lane];
  }
  m0 /= kk; m1 /= kk; m2 /= kk;
  double c[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll 4
  for (int j = 0; j < k; j++) {
    const double d[3] = {(double)sx[j * kPerWave + lane] - m0, (double)sy[j * kPerWave + lane] - m1, (double)sz[j * kPerWave + lane] - m2};
#pragma unroll
    for (int a = 0; a < 3; a++)
#pragma unroll
      for (int e = 0; e < 3; e++) c[a * 3 + e] += d[a] * d[e];
  }
#pragma unroll
  for (int a = 0; a < 9; a++) c[a] /= kk;
  double out6[6];
  regularize_cov_upstream(c, method, out6);
#pragma unroll
  for (int a = 0; a < 6; a++) cov6[(size_t)i * 6 + a] = out6[a];
}
__global__ __launch_bounds__(kBlock) void gicp_cov_ordered_kernel(const BvhView b, const float4* __restrict__ pts, const int n, const int k, const int method,
                                                                  const int* __restrict__ nbr, double* __restrict__ cov6) {
  gicp_cov_ordered_body<kKnnSlots, kOrdRounds>(b, pts, n, k, method, nbr, cov6);
}
__global__ __launch_bounds__(kBlock) void gicp_cov_ordered_wide_kernel(const BvhView b, const float4* __restrict__ pts, const int n, const int k, const int method,
                                                                       const int* __restrict__ nbr, double* __restrict__ cov6) {
  gicp_cov_ordered_body<kKnnSlotsWide, kOrdRoundsWide>(b, pts, n, k, method, nbr, cov6);
}

// c.cov of every point of `c` from the k-NN lists in `nbr` (knn_lists, a table of stride `stride`), in upstream's operation order.
int gicp_cov_upstream_order(dgs_handle* h, const BvhView& v, CloudState& c, int k, int regularization, const int* nbr, int stride) {
  if (stride == kKnnMaxWide) {
    const size_t lds = (size_t)(kBlock / kWave) * 3 * (size_t)k * kOrdPerWaveWide * sizeof(float);
    hipLaunchKernelGGL(gicp_cov_ordered_wide_kernel, dim3((unsigned)(((int64_t)c.n + kOrdPerBlockWide - 1) / kOrdPerBlockWide)), dim3(kBlock), lds, h->stream, v, c.pts.ptr,
                       (int)c.n, k, regularization, nbr, c.cov.ptr);
    return DGS_OK;
  }
  const size_t lds = (size_t)(kBlock / kWave) * 3 * (size_t)k * kOrdPerWave * sizeof(float);
  hipLaunchKernelGGL(gicp_cov_ordered_kernel, dim3((unsigned)(((int64_t)c.n + kOrdPerBlock - 1) / kOrdPerBlock)), dim3(kBlock), lds, h->stream, v, c.pts.ptr, (int)c.n, k,
                     regularization, nbr, c.cov.ptr);
  return DGS_OK;
}

}  // namespace dgs
