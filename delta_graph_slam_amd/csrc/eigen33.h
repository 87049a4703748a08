// pcl::eigen33 (common/impl/eigen.hpp) in float, operation for operation, no contraction: the roots of the characteristic polynomial
// and the cross-product selection of an eigenvector.  Shared by the prefilter's normal pass (smallest root) and the line refit of
// line_extraction.hip (largest root).
#pragma once
#include <cfloat>

#include "common.h"

namespace dgs {

__device__ inline void pf_compute_roots2(const float b, const float c, float* r) {
#pragma clang fp contract(off)
  r[0] = 0.f;
  float d = (float)((double)(b * b) - 4.0 * (double)c);   // Scalar (b * b - 4.0 * c): the double literal promotes the difference
  if (d < 0.f) d = 0.f;
  const float sd = sqrtf(d);
  r[2] = 0.5f * (b + sd);
  r[1] = 0.5f * (b - sd);
}

__device__ inline void pf_compute_roots(const float* m, float* r) {   // m row-major 3 x 3, symmetric
#pragma clang fp contract(off)
  const float m00 = m[0], m01 = m[1], m02 = m[2], m11 = m[4], m12 = m[5], m22 = m[8];
  const float c0 = m00 * m11 * m22 + 2.f * m01 * m02 * m12 - m00 * m12 * m12 - m11 * m02 * m02 - m22 * m01 * m01;
  const float c1 = m00 * m11 - m01 * m01 + m00 * m22 - m02 * m02 + m11 * m22 - m12 * m12;
  const float c2 = m00 + m11 + m22;
  if (fabsf(c0) < FLT_EPSILON) {
    pf_compute_roots2(c2, c1, r);
    return;
  }
  const float s_inv3 = (float)(1.0 / 3.0);
  const float s_sqrt3 = sqrtf(3.f);
  const float c2_over_3 = c2 * s_inv3;
  float a_over_3 = (c1 - c2 * c2_over_3) * s_inv3;
  if (a_over_3 > 0.f) a_over_3 = 0.f;
  const float half_b = 0.5f * (c0 + c2_over_3 * (2.f * c2_over_3 * c2_over_3 - c1));
  float q = half_b * half_b + a_over_3 * a_over_3 * a_over_3;
  if (q > 0.f) q = 0.f;
  const float rho = sqrtf(-a_over_3);
  const float theta = atan2f(sqrtf(-q), half_b) * s_inv3;
  const float cos_theta = cosf(theta);
  const float sin_theta = sinf(theta);
  r[0] = c2_over_3 + 2.f * rho * cos_theta;
  r[1] = c2_over_3 - rho * (cos_theta + s_sqrt3 * sin_theta);
  r[2] = c2_over_3 - rho * (cos_theta - s_sqrt3 * sin_theta);
  float t;
  if (r[0] >= r[1]) { t = r[0]; r[0] = r[1]; r[1] = t; }
  if (r[1] >= r[2]) {
    t = r[1]; r[1] = r[2]; r[2] = t;
    if (r[0] >= r[1]) { t = r[0]; r[0] = r[1]; r[1] = t; }
  }
  if (r[0] <= 0.f) pf_compute_roots2(c2, c1, r);
}

// m: the scaled matrix with the chosen root subtracted from its diagonal.  The largest of the three row cross products, normalised.
__device__ inline void pf_eigen33_vector(const float* m, float* ev) {
#pragma clang fp contract(off)
  auto cross = [](const float* u, const float* v, float* o) {
#pragma clang fp contract(off)
    o[0] = u[1] * v[2] - u[2] * v[1];
    o[1] = u[2] * v[0] - u[0] * v[2];
    o[2] = u[0] * v[1] - u[1] * v[0];
  };
  auto sq = [](const float* u) {
#pragma clang fp contract(off)
    return (u[0] * u[0] + u[1] * u[1]) + u[2] * u[2];
  };
  float v1[3], v2[3], v3[3];
  cross(m + 0, m + 3, v1);
  cross(m + 0, m + 6, v2);
  cross(m + 3, m + 6, v3);
  const float l1 = sq(v1), l2 = sq(v2), l3 = sq(v3);
  const float* v = v3;
  float l = l3;
  if (l1 >= l2 && l1 >= l3) { v = v1; l = l1; }
  else if (l2 >= l1 && l2 >= l3) { v = v2; l = l2; }
  const float sl = sqrtf(l);
  ev[0] = v[0] / sl; ev[1] = v[1] / sl; ev[2] = v[2] / sl;
}

}  // namespace dgs
