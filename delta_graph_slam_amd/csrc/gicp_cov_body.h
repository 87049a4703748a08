// FastGICP::calculate_covariances' arithmetic as device bodies, written once: gicp_cov_from_knn_kernel / gicp_cov_from_knn_wide_kernel
// (gicp_cov.hip) run them over one cloud, cov_fast_batch_kernel / cov_fast_batch_wide_kernel (cov_batch.hip) over every cloud of a chunk.
#pragma once
#include <cmath>
#include <cstdint>

#include "handle.h"
#include "nn_group.h"
#include "small_linalg.h"

namespace dgs {

__device__ inline void regularize_cov(const double* cov9, int method_and_flag, double* out6) {
  const bool jacobi_svd = (method_and_flag & 0x100) != 0;   // dgs_params.gicp_cov_jacobi_svd rides on the method word
  const int method = method_and_flag & 0xff;
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
    // Eigen::JacobiSVD<Matrix3d> svd(cov, ComputeFullU | ComputeFullV); cov = U values.asDiagonal() V^T (singular values descending) -- or, rounds
    // 1-3's stand-in, the eigen-decomposition of the symmetric PSD matrix (the same factors up to rounding, U = V)
    double U[9], V[9], sv[3];
    if (jacobi_svd) {
      jacobi_svd3_d(cov9, U, V, sv);
    } else {
      double ev[3], E[9];
      sym_eig3_d(cov9, ev, E);
      for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) U[r * 3 + c] = V[r * 3 + c] = E[r * 3 + (2 - c)];   // descending order: column c <- eigenvector 2 - c
      sv[0] = fabs(ev[2]); sv[1] = fabs(ev[1]); sv[2] = fabs(ev[0]);
    }
    double vals[3];
    if (method == DGS_GICP_REG_PLANE) {
      vals[0] = 1; vals[1] = 1; vals[2] = 1e-3;
    } else if (method == DGS_GICP_REG_MIN_EIG) {
      for (int a = 0; a < 3; a++) vals[a] = fmax(sv[a], 1e-3);
    } else {
      for (int a = 0; a < 3; a++) vals[a] = fmax(sv[a] / sv[0], 1e-3);
    }
    for (int r = 0; r < 3; r++)
      for (int c = 0; c < 3; c++) C[r * 3 + c] = U[r * 3 + 0] * vals[0] * V[c * 3 + 0] + U[r * 3 + 1] * vals[1] * V[c * 3 + 1] + U[r * 3 + 2] * vals[2] * V[c * 3 + 2];
  }
  out6[0] = C[0]; out6[1] = C[1]; out6[2] = C[2]; out6[3] = C[4]; out6[4] = C[5]; out6[5] = C[8];
}

// One wave per 64 points, two phases.  (1) eight rounds of 8 points, 8 lanes per point: gather the neighbours, mean and covariance in
// double, reduced inside the 8-lane group; the six covariance entries of every point go to LDS.  (2) lane t regularises point t.
// (Regularising in phase 1's layout left 56 of 64 lanes idle through the 3x3 decomposition, which is most of this kernel's
// instructions: 1,964 VALU instructions per wave of 8 points.)  Same arithmetic per point as before, bit for bit.
#ifndef DGS_COV_ROUNDS
#define DGS_COV_ROUNDS 4
#endif
// A wave takes kCovRounds * 8 points: rounds of 8 points (8 lanes each) for the sums, then one lane per point for the regularisation.
// 8 rounds fill every lane of the second phase but leave a 65,536-point cloud with one wave per SIMD and nothing to hide its gathers
// behind; measured 8 / 4 / 2 rounds: 23.6 / 20.8 / 25.4 us per 65,536-point cloud, 21.5 / 14.6 / 15.2 us per 26,668 points.
constexpr int kCovRounds = DGS_COV_ROUNDS, kCovPerWave = kCovRounds * 8, kCovPerBlock = kCovPerWave * (kBlock / kWave);
// blk: the workgroup's index among the workgroups of this cloud (blockIdx.x for a launch over one cloud).
template <int SLOTS>
__device__ __forceinline__ void gicp_cov_from_knn_body(const BvhView& b, const float4* __restrict__ pts, const int n, const int k, const int method,
                                                       const int* __restrict__ nbr, double* __restrict__ cov6, const int blk) {
  __shared__ double s_c[kBlock / kWave][kCovPerWave][6];
  __shared__ int s_i[kBlock / kWave][kCovPerWave];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, sub = lane & 7, grp = lane >> 3;
  const int wave_base = (blk * (kBlock / kWave) + wv) * kCovPerWave;   // first point (position in index order) of this wave
  if (wave_base >= n) return;
  const double kk = (double)k;
#pragma unroll 2
  for (int r = 0; r < kCovRounds; r++) {
    const int pos = wave_base + r * 8 + grp;
    int i = -1;
    if (pos < n) i = (int)__float_as_uint(b.sorted[pos].w);
    const bool live = i >= 0 && i < n;
    // neighbours of this lane (slots q * 8 + sub < k); slots that found nothing are zero columns, as upstream's matrix
    double px[SLOTS], py[SLOTS], pz[SLOTS];
    bool use[SLOTS];
    double sx = 0, sy = 0, sz = 0;
#pragma unroll
    for (int q = 0; q < SLOTS; q++) {
      use[q] = (q * 8 + sub) < k;
      const int j = (live && use[q]) ? nbr[(size_t)pos * (SLOTS * 8) + q * 8 + sub] : -1;
      const float4 p = (j >= 0) ? pts[j] : make_float4(0.f, 0.f, 0.f, 0.f);
      px[q] = p.x; py[q] = p.y; pz[q] = p.z;
      if (use[q]) { sx += px[q]; sy += py[q]; sz += pz[q]; }
    }
    const double mx = group8_sum_f64(sx) / kk, my = group8_sum_f64(sy) / kk, mz = group8_sum_f64(sz) / kk;
    double c[6] = {0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int q = 0; q < SLOTS; q++) {
      if (use[q]) {
        const double dx = px[q] - mx, dy = py[q] - my, dz = pz[q] - mz;
        c[0] += dx * dx; c[1] += dx * dy; c[2] += dx * dz; c[3] += dy * dy; c[4] += dy * dz; c[5] += dz * dz;
      }
    }
#pragma unroll
    for (int a = 0; a < 6; a++) c[a] = group8_sum_f64(c[a]) / kk;
    if (sub == 0) {
#pragma unroll
      for (int a = 0; a < 6; a++) s_c[wv][r * 8 + grp][a] = c[a];
      s_i[wv][r * 8 + grp] = live ? i : -1;
    }
  }
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_s_waitcnt(0xc07f);   // lgkmcnt(0): the wave's LDS stores have landed
  if (lane >= kCovPerWave) return;
  const int i = s_i[wv][lane];
  if (i < 0) return;
  const double* c = s_c[wv][lane];
  const double cov9[9] = {c[0], c[1], c[2], c[1], c[3], c[4], c[2], c[4], c[5]};
  double out6[6];
  regularize_cov(cov9, method, out6);
#pragma unroll
  for (int a = 0; a < 6; a++) cov6[(size_t)i * 6 + a] = out6[a];
}

}  // namespace dgs
