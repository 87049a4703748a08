// PCL_NDT_HIP (DGS_METHOD_PCL_NDT): the per-point and per-(point, voxel) arithmetic of pcl::NormalDistributionsTransform's
// computeDerivatives / updateDerivatives / computeHessian / updateHessian (PCL 1.10, ndt.hpp), everything in double, stated ONCE as
// host + device code: pcl_ndt.hip runs it in the derivative kernel, tests/cpp/pcl_ndt_driver.cpp compiles the same text for the CPU and
// replays it against the numpy restatement (tests/pcl_ndt_reference.py) bit for bit.  Plain C++: no HIP type, no include of the
// project's other headers.  Every operation is rounded on its own: build with -ffp-contract=off (csrc/Makefile, the CPU test).
// [UPSTREAM-RECALL: pcl/registration/impl/ndt.hpp, pcl/filters/voxel_grid_covariance.h, pcl/kdtree/impl/kdtree_flann.hpp; DESIGN.md 6i.]
#pragma once
#include <cmath>
#include <cstddef>

#if defined(__HIPCC__)
#define PN_HD __host__ __device__ __forceinline__
#else
#define PN_HD inline
#endif

namespace dgs {
namespace pn {

constexpr int kSlots = 27;                 // cells of the walk around a transformed point: a centroid within `resolution` lies in one of them
constexpr int kAccum = 43;                 // score, gradient 0..5, Hessian 0..35 row-major
constexpr int kPointsPerWorkgroup = 256;   // one point per lane and pass
constexpr int kPointsPerSlice = 512;       // a slice is the unit whose sums make one row (pcl_ndt.hip slices_of)

// The target's voxel grid as the neighbourhood reads it (a view of dgs::VoxelGrid; the CPU driver fills one from a file).
struct Grid {
  int min_b[3], max_b[3];
  int mul1, mul2;          // cell (a0, a1, a2) -> (a0 - min0) + (a1 - min1) * mul1 + (a2 - min2) * mul2
  float leaf, inv_leaf;
  int leaf_pow2;           // the leaf is a power of two: x * inv_leaf and x / leaf are the same float
  const int* cell2vox;     // dense; a VALID voxel's number or -1 (an under-populated voxel is no entry of upstream's k-d tree)
  const float* centroid;   // four floats per voxel: VoxelGridCovariance's float centroid, w unused here
};

// slot k of the walk, k = 9 (dx + 1) + 3 (dy + 1) + (dz + 1)
PN_HD void slot_offset(const int k, int& dx, int& dy, int& dz) {
  dx = k / 9 - 1;
  dy = (k / 3) % 3 - 1;
  dz = k % 3 - 1;
}

// pcl::transformPointCloud's row in float: ((m0 x + m1 y) + m2 z) + m3
PN_HD float affine_row(const float m0, const float m1, const float m2, const float m3, const float x, const float y, const float z) {
  const float a = m0 * x, b = m1 * y, c = m2 * z;
  const float ab = a + b;
  const float abc = ab + c;
  return abc + m3;
}
// T: row-major 3 x 4
PN_HD void transform_point(const float* T, const float x, const float y, const float z, float (&xt)[3]) {
  xt[0] = affine_row(T[0], T[1], T[2], T[3], x, y, z);
  xt[1] = affine_row(T[4], T[5], T[6], T[7], x, y, z);
  xt[2] = affine_row(T[8], T[9], T[10], T[11], x, y, z);
}

// the voxel in slot k around cell c, or -1
PN_HD int slot_voxel(const Grid& g, const int (&c)[3], const int k) {
  int dx, dy, dz;
  slot_offset(k, dx, dy, dz);
  const int a0 = c[0] + dx, a1 = c[1] + dy, a2 = c[2] + dz;
  const bool inb = a0 >= g.min_b[0] && a0 <= g.max_b[0] && a1 >= g.min_b[1] && a1 <= g.max_b[1] && a2 >= g.min_b[2] && a2 <= g.max_b[2];
  if (!inb) return -1;
  return g.cell2vox[(a0 - g.min_b[0]) + (a1 - g.min_b[1]) * g.mul1 + (a2 - g.min_b[2]) * g.mul2];
}

// radiusSearch(x_trans, resolution): FLANN's L2_Simple in float, a strict <, the radius squared in float
PN_HD bool within_radius(const Grid& g, const int vid, const float (&xt)[3]) {
  const float* ce = g.centroid + (size_t)vid * 4;
  const float ex = ce[0] - xt[0], ey = ce[1] - xt[1], ez = ce[2] - xt[2];
  const float r2 = g.leaf * g.leaf;
  const float d2 = (ex * ex + ey * ey) + ez * ez;
  return d2 < r2;
}

// Bit k of the result: slot k holds a valid voxel whose centroid is within `resolution` of xt.  c receives the point's cell.  A point
// that is not finite (or lies 2^30 cells out) has no neighbours.
PN_HD unsigned neighbourhood(const Grid& g, const float (&xt)[3], int (&c)[3]) {
  c[0] = c[1] = c[2] = 0;
  float f[3];
  bool ok = true;
  for (int r = 0; r < 3; r++) {
    f[r] = floorf(g.leaf_pow2 ? xt[r] * g.inv_leaf : xt[r] / g.leaf);
    ok = ok && (fabsf(f[r]) < 1073741824.f);   // false for NaN
  }
  if (!ok) return 0u;
  for (int r = 0; r < 3; r++) c[r] = (int)f[r];
  unsigned mask = 0;
#pragma unroll
  for (int k = 0; k < kSlots; k++) {
    const int vid = slot_voxel(g, c, k);
    if (vid >= 0 && within_radius(g, vid, xt)) mask |= 1u << k;
  }
  return mask;
}

// computeAngleDerivatives: the double vectors j_ang_a_ .. j_ang_h_ and h_ang_a2_ .. h_ang_f3_ of pose p (its three angles), with
// upstream's small-angle cases; fix_d1: the exact z entry of h_ang_d1_ (-sy) instead of upstream's +sy (dgs_params.ndt_fix_hessian_d1).
// The device takes its tables from the optimiser (ndt_optimiser.h write_evaluation: the same expressions); this copy serves the CPU.
struct Tables {
  double j[8][3];
  double h[15][3];
};
inline void angle_tables(const double rx, const double ry, const double rz, const int fix_d1, Tables& t) {
  double cx, cy, cz, sx, sy, sz;
  if (std::fabs(rx) < 10e-5) { cx = 1.0; sx = 0.0; } else { cx = std::cos(rx); sx = std::sin(rx); }
  if (std::fabs(ry) < 10e-5) { cy = 1.0; sy = 0.0; } else { cy = std::cos(ry); sy = std::sin(ry); }
  if (std::fabs(rz) < 10e-5) { cz = 1.0; sz = 0.0; } else { cz = std::cos(rz); sz = std::sin(rz); }
  double (*J)[3] = t.j;
  J[0][0] = (-sx * sz + cx * sy * cz); J[0][1] = (-sx * cz - cx * sy * sz); J[0][2] = (-cx * cy);
  J[1][0] = (cx * sz + sx * sy * cz);  J[1][1] = (cx * cz - sx * sy * sz);  J[1][2] = (-sx * cy);
  J[2][0] = (-sy * cz);                J[2][1] = (sy * sz);                 J[2][2] = (cy);
  J[3][0] = (sx * cy * cz);            J[3][1] = (-sx * cy * sz);           J[3][2] = (sx * sy);
  J[4][0] = (-cx * cy * cz);           J[4][1] = (cx * cy * sz);            J[4][2] = (-cx * sy);
  J[5][0] = (-cy * sz);                J[5][1] = (-cy * cz);                J[5][2] = 0.0;
  J[6][0] = (cx * cz - sx * sy * sz);  J[6][1] = (-cx * sz - sx * sy * cz); J[6][2] = 0.0;
  J[7][0] = (sx * cz + cx * sy * sz);  J[7][1] = (cx * sy * cz - sx * sz);  J[7][2] = 0.0;
  double (*H)[3] = t.h;
  H[0][0] = (-cx * sz - sx * sy * cz); H[0][1] = (-cx * cz + sx * sy * sz); H[0][2] = (sx * cy);
  H[1][0] = (-sx * sz + cx * sy * cz); H[1][1] = (-cx * sy * sz - sx * cz); H[1][2] = (-cx * cy);
  H[2][0] = (cx * cy * cz);            H[2][1] = (-cx * cy * sz);           H[2][2] = (cx * sy);
  H[3][0] = (sx * cy * cz);            H[3][1] = (-sx * cy * sz);           H[3][2] = (sx * sy);
  H[4][0] = (-sx * cz - cx * sy * sz); H[4][1] = (sx * sz - cx * sy * cz);  H[4][2] = 0.0;
  H[5][0] = (cx * cz - sx * sy * sz);  H[5][1] = (-sx * sy * cz - cx * sz); H[5][2] = 0.0;
  H[6][0] = (-cy * cz);                H[6][1] = (cy * sz);                 H[6][2] = (fix_d1 ? -sy : sy);
  H[7][0] = (-sx * sy * cz);           H[7][1] = (sx * sy * sz);            H[7][2] = (sx * cy);
  H[8][0] = (cx * sy * cz);            H[8][1] = (-cx * sy * sz);           H[8][2] = (-cx * cy);
  H[9][0] = (sy * sz);                 H[9][1] = (sy * cz);                 H[9][2] = 0.0;
  H[10][0] = (-sx * cy * sz);          H[10][1] = (-sx * cy * cz);          H[10][2] = 0.0;
  H[11][0] = (cx * cy * sz);           H[11][1] = (cx * cy * cz);           H[11][2] = 0.0;
  H[12][0] = (-cy * cz);               H[12][1] = (cy * sz);                H[12][2] = 0.0;
  H[13][0] = (-cx * sz - sx * sy * cz); H[13][1] = (-cx * cz + sx * sy * sz); H[13][2] = 0.0;
  H[14][0] = (-sx * sz + cx * sy * cz); H[14][1] = (-cx * sy * sz - sx * cz); H[14][2] = 0.0;
}

// computePointDerivatives: the point's products with the angle vectors.  x: the double of the UNtransformed float point.
// xj: point_gradient_ (1,3) (2,3) (0,4) (1,4) (2,4) (0,5) (1,5) (2,5); xh: a2 a3 b2 b3 c2 c3 d1 d2 d3 e1 e2 e3 f1 f2 f3.
template <bool NEED_H>
PN_HD void point_tables(const double (&x)[3], const double (*J)[3], const double (*H)[3], double (&xj)[8], double (&xh)[15]) {
#pragma unroll
  for (int i = 0; i < 8; i++) xj[i] = x[0] * J[i][0] + x[1] * J[i][1] + x[2] * J[i][2];
#pragma unroll
  for (int i = 0; i < 15; i++) xh[i] = NEED_H ? (x[0] * H[i][0] + x[1] * H[i][1] + x[2] * H[i][2]) : 0.0;
}

// One (point, voxel) item.  KIND 0: updateDerivatives without the Hessian (a More-Thuente trial), 1: with it, 2: updateHessian alone
// (the closing computeHessian).  xt: the float-transformed point; rec: the voxel's mean[3] and inverse covariance [9] row-major;
// expd: std::exp(double).  acc[0] score, acc[1..6] gradient, acc[7..42] Hessian: the item's increments are ADDED.
// A voxel whose weight fails upstream's test adds nothing, the score included (updateDerivatives returns 0 there).
template <int KIND, class EXP>
PN_HD void item(const float (&xt)[3], const double (&xj)[8], const double (&xh)[15], const double* rec, const double gauss_d1, const double gauss_d2,
                double (&acc)[kAccum], EXP&& expd) {
  const double pg13 = xj[0], pg23 = xj[1];
  const double pg4[3] = {xj[2], xj[3], xj[4]}, pg5[3] = {xj[5], xj[6], xj[7]};
  double q[3], C[3][3];
#pragma unroll
  for (int r = 0; r < 3; r++) q[r] = (double)xt[r] - rec[r];
#pragma unroll
  for (int r = 0; r < 3; r++)
#pragma unroll
    for (int c = 0; c < 3; c++) C[r][c] = rec[3 + r * 3 + c];
  double Cq[3];
#pragma unroll
  for (int r = 0; r < 3; r++) Cq[r] = C[r][0] * q[0] + C[r][1] * q[1] + C[r][2] * q[2];
  const double e_arg = -gauss_d2 * (q[0] * Cq[0] + q[1] * Cq[1] + q[2] * Cq[2]) / 2;
  double e = expd(e_arg);
  const double score_inc = -gauss_d1 * e;
  e = gauss_d2 * e;
  if (e > 1 || e < 0 || e != e) return;
  e *= gauss_d1;
  // cov_dxd_pi = c_inv * point_gradient_.col(i): column i of c_inv for i < 3; column 3 of the point gradient has a zero first entry
  double cd[6][3];
#pragma unroll
  for (int r = 0; r < 3; r++) {
    cd[0][r] = C[r][0]; cd[1][r] = C[r][1]; cd[2][r] = C[r][2];
    cd[3][r] = C[r][1] * pg13 + C[r][2] * pg23;
    cd[4][r] = C[r][0] * pg4[0] + C[r][1] * pg4[1] + C[r][2] * pg4[2];
    cd[5][r] = C[r][0] * pg5[0] + C[r][1] * pg5[1] + C[r][2] * pg5[2];
  }
  double A[6];   // x_trans . cov_dxd_pi
#pragma unroll
  for (int i = 0; i < 6; i++) A[i] = q[0] * cd[i][0] + q[1] * cd[i][1] + q[2] * cd[i][2];
  if (KIND != 2) {
    acc[0] += score_inc;
#pragma unroll
    for (int i = 0; i < 6; i++) acc[1 + i] += A[i] * e;
  }
  if (KIND != 0) {
    // x_trans . (c_inv * point_hessian_ block) for the six distinct vectors a = (0, xh0, xh1) b c, d = xh6..8 e f
    double xch[6];
#pragma unroll
    for (int v = 0; v < 6; v++) {
      double Ch[3];
#pragma unroll
      for (int r = 0; r < 3; r++)
        Ch[r] = (v < 3) ? (C[r][1] * xh[v < 3 ? 2 * v : 0] + C[r][2] * xh[v < 3 ? 2 * v + 1 : 0])
                        : (C[r][0] * xh[v < 3 ? 0 : 3 * v - 3] + C[r][1] * xh[v < 3 ? 0 : 3 * v - 2] + C[r][2] * xh[v < 3 ? 0 : 3 * v - 1]);
      xch[v] = q[0] * Ch[0] + q[1] * Ch[1] + q[2] * Ch[2];
    }
#pragma unroll
    for (int i = 0; i < 6; i++) {
      const double nA = -gauss_d2 * A[i];
#pragma unroll
      for (int j = 0; j < 6; j++) {
        double t = nA * A[j];
        if (i >= 3 && j >= 3) {
          const int lo = (i < j ? i : j) - 3, hi = (i < j ? j : i) - 3;
          t = t + xch[lo == 0 ? hi : (lo == 1 ? 2 + hi : 5)];
        }
        // point_gradient_.col(j) . cov_dxd_pi
        const double D = (j < 3) ? cd[i][j < 3 ? j : 0] : (j == 3) ? (pg13 * cd[i][1] + pg23 * cd[i][2])
                       : (j == 4) ? (pg4[0] * cd[i][0] + pg4[1] * cd[i][1] + pg4[2] * cd[i][2]) : (pg5[0] * cd[i][0] + pg5[1] * cd[i][1] + pg5[2] * cd[i][2]);
        acc[7 + i * 6 + j] += e * (t + D);
      }
    }
  }
}

}  // namespace pn
}  // namespace dgs
