// FloorDetectionNodelet::detect's device pieces, written once for the single call (floor_detection.hip) and the call over many scans
// (floor_detection_batch.hip): the float arithmetic both share with the host (fd_dot4, fd_is_inlier), the bodies of the three per-point
// passes, which take the workgroup's number inside its own scan (blockIdx.x of the single launch), and the plane model of sac.h's
// kernels.  Both files compile under the same flags (no contraction); every body keeps its own pragma as well.
#pragma once
#include "common.h"
#include "sac.h"

namespace dgs {

constexpr int kFdHypSub = 64;            // hypotheses per workgroup of sac_score_kernel (blockIdx.y)
constexpr int kFdNormalK = 10;           // ne.setKSearch(10) (:219)

struct FdHyp {
  float c[4];
  int draw, i0, i1, i2;
};

struct FdMat {
  float m[16];   // row-major
};
inline FdMat fd_mat(const float* col16) {
  FdMat M;
  for (int r = 0; r < 4; r++)
    for (int c = 0; c < 4; c++) M.m[4 * r + c] = col16[4 * c + r];
  return M;
}

// a four-term float dot product, the terms associated as plane_dot_order says
__host__ __device__ __forceinline__ float fd_dot4(const float a0, const float a1, const float a2, const float a3, const float b0, const float b1,
                                                  const float b2, const float b3, const int order) {
#pragma clang fp contract(off)
  const float x = a0 * b0, y = a1 * b1, z = a2 * b2, w = a3 * b3;
  return order == 0 ? (x + y) + (z + w) : order == 1 ? (x + z) + (y + w) : ((x + y) + z) + w;
}

// countWithinDistance / selectWithinDistance: |dot4(coefficients, (x, y, z, 1))| < threshold, compared in double
__host__ __device__ __forceinline__ bool fd_is_inlier(const float4 p, const float a, const float b, const float c, const float d, const int order,
                                                      const double thr) {
  return (double)fabsf(fd_dot4(a, b, c, d, p.x, p.y, p.z, 1.0f, order)) < thr;
}

// pcl::transformPointCloud(Matrix4f): a non-finite point goes through the arithmetic, the fourth float becomes 1
__device__ __forceinline__ float4 fd_transform(const float4 p, const FdMat& M, const int order) {
#pragma clang fp contract(off)
  float4 q;
  const float* m = M.m;
  if (order == 0) {
    q.x = p.x * m[0] + (p.y * m[1] + (p.z * m[2] + m[3]));
    q.y = p.x * m[4] + (p.y * m[5] + (p.z * m[6] + m[7]));
    q.z = p.x * m[8] + (p.y * m[9] + (p.z * m[10] + m[11]));
  } else {
    q.x = ((m[0] * p.x + m[1] * p.y) + m[2] * p.z) + m[3];
    q.y = ((m[4] * p.x + m[5] * p.y) + m[6] * p.z) + m[7];
    q.z = ((m[8] * p.x + m[9] * p.y) + m[10] * p.z) + m[11];
  }
  q.w = 1.0f;
  return q;
}

// ================================================================================================ filter stage
// tilt, then plane_clip twice (:117-119): PlaneClipper3D keeps a point whose float distance ((0*x + 0*y) + 1*z) + d is >= 0; the second
// clip is negated
__device__ __forceinline__ void fd_tilt_clip_body(const float4* __restrict__ in, const int n, const FdMat& M, const int order, const float hi, const float lo,
                                                  float4* __restrict__ out, unsigned char* __restrict__ flags, const int blk) {
#pragma clang fp contract(off)
  const int i = blk * kBlock + threadIdx.x;
  if (i >= n) return;
  const float4 q = fd_transform(in[i], M, order);
  const float base = (0.0f * q.x + 0.0f * q.y) + 1.0f * q.z;
  const float dhi = base + hi, dlo = base + lo;
  out[i] = q;
  flags[i] = (dhi >= 0.0f && !(dlo >= 0.0f)) ? 1 : 0;
}

// normal_filtering's rule (:227-228) over the normals pf_normal_kernel wrote: kept iff |n.z| > cos(normal_filter_thresh) in double; a NaN
// normal fails the comparison
__device__ __forceinline__ void fd_normal_flag_body(const float4* __restrict__ normals, const int n, const double cos_thr, unsigned char* __restrict__ flags,
                                                    const int blk) {
  const int i = blk * kBlock + threadIdx.x;
  if (i >= n) return;
  flags[i] = ((double)fabsf(normals[i].z) > cos_thr) ? 1 : 0;
}

__device__ __forceinline__ void fd_transform_body(const float4* __restrict__ in, const int n, const FdMat& M, const int order, float4* __restrict__ out,
                                                  const int blk) {
  const int i = blk * kBlock + threadIdx.x;
  if (i >= n) return;
  out[i] = fd_transform(in[i], M, order);
}

// ================================================================================================ hypotheses
// pcl::SampleConsensusModelPlane for sac.h's kernels: isSampleGood, computeModelCoefficients and the countWithinDistance predicate
struct FdModel {
  static constexpr int kSample = 3;
  using Hyp = FdHyp;
  struct Params {
    int order, bad_run;   // plane_dot_order, max_sample_checks
    double thr;           // distance_threshold
  };
  struct Coef {
    float a, b, c, d;
  };
  static __device__ __forceinline__ int bad_run(const Params& prm) { return prm.bad_run; }
  // computeModel's w^3 for SacWalk::step, which runs on the host: upstream's own libm
  static double ratio_power(double w) { return std::pow(w, 3.0); }
  // dy1dy2 = (p1 - p0) / (p2 - p0), component-wise; good iff its x, y, z are not all equal (NaN compares unequal)
  static __device__ __forceinline__ bool good(const Params&, const float4 (&p)[3]) {
#pragma clang fp contract(off)
    const float rx = (p[1].x - p[0].x) / (p[2].x - p[0].x), ry = (p[1].y - p[0].y) / (p[2].y - p[0].y), rz = (p[1].z - p[0].z) / (p[2].z - p[0].z);
    return rx != ry || rz != ry;
  }
  static __device__ __forceinline__ FdHyp make(const Params& prm, const float4 (&p)[3], const int d, const int (&idx)[3]) {
#pragma clang fp contract(off)
    const float ux = p[1].x - p[0].x, uy = p[1].y - p[0].y, uz = p[1].z - p[0].z;
    const float vx = p[2].x - p[0].x, vy = p[2].y - p[0].y, vz = p[2].z - p[0].z;
    float a = uy * vz - uz * vy;
    float b = uz * vx - ux * vz;
    float c = ux * vy - uy * vx;
    // model_coefficients.normalize(): divided by sqrt(squaredNorm) when that is > 0
    const float s2 = fd_dot4(a, b, c, 0.f, a, b, c, 0.f, prm.order);
    if (s2 > 0.f) {
      const float s = sqrtf(s2);
      a = a / s; b = b / s; c = c / s;
    }
    FdHyp hy;
    hy.c[0] = a; hy.c[1] = b; hy.c[2] = c;
    hy.c[3] = -1.0f * fd_dot4(a, b, c, 0.f, p[0].x, p[0].y, p[0].z, p[0].w, prm.order);
    hy.draw = d; hy.i0 = idx[0]; hy.i1 = idx[1]; hy.i2 = idx[2];
    return hy;
  }
  static __device__ __forceinline__ Coef coef(const FdHyp* hy) { return {hy->c[0], hy->c[1], hy->c[2], hy->c[3]}; }
  static __device__ __forceinline__ bool inlier(const Params& prm, const float4 p, const Coef& c) {
    return fd_is_inlier(p, c.a, c.b, c.c, c.d, prm.order, prm.thr);
  }
};

}  // namespace dgs
