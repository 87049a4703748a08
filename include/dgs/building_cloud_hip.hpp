// dgs::HipBuildingClouds -- interpolate (src/hdl_graph_slam/ros_utils.cpp:146-165), BuildingTools::buildPointCloud's cloud
// (building_tools.cpp:166-196) and Building::getCloud (building.cpp:7-22) over libdgs_reg.so (include/dgs_reg.h,
// dgs_building_cloud_generate).  INTEGRATION.md 4j shows the patches to the nodelet.
// Header-only; needs pcl::PointCloud at the user's build.  Vectors and matrices are anything with (row, column) access (Eigen's); a
// line is anything with ->pointA and ->pointB (LineFeature::Ptr).  The handle is created at the first call.  Any error returns a
// null pointer and never throws (last_error() has the text): the caller falls back to interpolate.
#pragma once

#include <cmath>
#include <cstdint>
#include <vector>

#include <pcl/point_cloud.h>

#include "../dgs_reg.h"

namespace dgs {

// The matrix Building::getCloud builds (building.cpp:11-15) from the building's pose and its node's estimate, both 3 x 3 double
// (Eigen::Isometry2d::matrix()), then transform2Dto3D (ros_utils.cpp:105-126) -> 16 floats, COLUMN-major.  Scalar host arithmetic;
// [UPSTREAM-RECALL] Eigen 3.3: an Isometry's inverse() is (R^T, -(R^T t)), the product of two is (Ra Rb, Ra tb + ta).
template <typename Pose, typename Estimate>
inline void building_transform16(const Pose& P, const Estimate& E, float out16[16]) {
  const double r00 = P(0, 0), r01 = P(1, 0), r10 = P(0, 1), r11 = P(1, 1);   // the inverse's rotation: the transpose
  const double px = P(0, 2), py = P(1, 2);
  const double ix = -(r00 * px + r01 * py), iy = -(r10 * px + r11 * py);
  const double t00 = r00 * E(0, 0) + r01 * E(1, 0), t01 = r00 * E(0, 1) + r01 * E(1, 1);
  const double t10 = r10 * E(0, 0) + r11 * E(1, 0), t11 = r10 * E(0, 1) + r11 * E(1, 1);
  double tx = (r00 * E(0, 2) + r01 * E(1, 2)) + ix, ty = (r10 * E(0, 2) + r11 * E(1, 2)) + iy;
  tx += px - (t00 * px + t01 * py);
  ty += py - (t10 * px + t11 * py);
  const float ang = std::atan2((float)t10, (float)t00);   // Eigen::Rotation2Df(mat).angle()
  const float c = std::cos(ang), s = std::sin(ang);
  for (int i = 0; i < 16; i++) out16[i] = 0.f;
  out16[0] = c;        // (0, 0)
  out16[1] = s;        // (1, 0)
  out16[4] = -s;       // (0, 1)
  out16[5] = c;        // (1, 1)
  out16[10] = 1.f;
  out16[12] = (float)tx;
  out16[13] = (float)ty;
  out16[15] = 1.f;
}

template <typename PointT>
class HipBuildingClouds {
 public:
  using Cloud = pcl::PointCloud<PointT>;
  using CloudPtr = typename Cloud::Ptr;

  explicit HipBuildingClouds(int device = 0) : device_(device) { dgs_building_cloud_params_init(&p_); }
  ~HipBuildingClouds() {
    if (h_) dgs_destroy(h_);
  }
  HipBuildingClouds(const HipBuildingClouds&) = delete;
  HipBuildingClouds& operator=(const HipBuildingClouds&) = delete;

  dgs_building_cloud_params& params() { return p_; }
  const char* last_error() const { return dgs_last_error(h_); }

  // interpolate(a, b): Eigen::Vector3f end points
  template <typename Vec3>
  CloudPtr interpolate(const Vec3& a, const Vec3& b) {
    begin();
    push(a, b);
    end_item();
    return run(nullptr, nullptr, nullptr);
  }
  // the cloud buildPointCloud accumulates over a building's lines, in order
  template <typename Lines>
  CloudPtr buildPointCloud(const Lines& lines) {
    begin();
    for (const auto& l : lines) push(l->pointA, l->pointB);
    end_item();
    return run(nullptr, nullptr, nullptr);
  }
  // Building::getCloud: that cloud through pcl::transformPointCloud(trans3D), an Eigen::Matrix4f
  template <typename Lines, typename Mat4>
  CloudPtr getCloud(const Lines& lines, const Mat4& trans3D) {
    begin();
    for (const auto& l : lines) push(l->pointA, l->pointB);
    end_item();
    float m[16];
    for (int c = 0; c < 4; c++)
      for (int r = 0; r < 4; r++) m[c * 4 + r] = (float)trans3D(r, c);
    return run(m, nullptr, nullptr);
  }
  // Many items in one call: items[i] is a range of lines; transforms16 (nullable): column-major 4 x 4 floats, transform_index (nullable)
  // per item the matrix it goes through or -1, as dgs_building_cloud_generate takes them.  point_offsets (nullable) receives
  // items + 1 offsets into the returned cloud.
  template <typename Items>
  CloudPtr clouds(const Items& items, const float* transforms16, const int32_t* transform_index, std::vector<int64_t>* point_offsets) {
    begin();
    for (const auto& lines : items) {
      for (const auto& l : lines) push(l->pointA, l->pointB);
      end_item();
    }
    return run(transforms16, transform_index, point_offsets);
  }

 private:
  void begin() {
    lines_.clear();
    offsets_.assign(1, 0);
  }
  template <typename Vec3>
  void push(const Vec3& a, const Vec3& b) {
    dgs_line_feature f{};
    for (int c = 0; c < 3; c++) {
      f.point_a[c] = (double)a(c, 0);
      f.point_b[c] = (double)b(c, 0);
    }
    lines_.push_back(f);
  }
  void end_item() { offsets_.push_back((int64_t)lines_.size()); }

  CloudPtr run(const float* transforms16, const int32_t* transform_index, std::vector<int64_t>* point_offsets) {
    if (!ensure_handle()) return nullptr;
    const int64_t n_items = (int64_t)offsets_.size() - 1;
    int64_t m = 0;
    if (dgs_building_cloud_generate(h_, &p_, lines_.data(), offsets_.data(), n_items, transforms16, transform_index, &m) != DGS_OK) return nullptr;
    out_.resize(4 * (size_t)(m ? m : 1));
    if (point_offsets) point_offsets->assign((size_t)n_items + 1, 0);
    if (dgs_building_cloud_get(h_, out_.data(), m, 0, point_offsets ? point_offsets->data() : nullptr, &m, nullptr) != DGS_OK) return nullptr;
    CloudPtr cloud(new Cloud());
    cloud->points.resize((size_t)m);
    for (int64_t i = 0; i < m; i++) {
      cloud->points[(size_t)i].x = out_[4 * (size_t)i];
      cloud->points[(size_t)i].y = out_[4 * (size_t)i + 1];
      cloud->points[(size_t)i].z = out_[4 * (size_t)i + 2];
    }
    cloud->width = (uint32_t)m;
    cloud->height = 1;
    return cloud;
  }
  bool ensure_handle() {
    if (h_) return true;
    dgs_params prm;
    if (dgs_params_init(&prm, DGS_METHOD_NDT) != DGS_OK) return false;
    prm.device = device_;
    return dgs_create(&prm, &h_) == DGS_OK;
  }

  dgs_building_cloud_params p_{};
  dgs_handle* h_ = nullptr;
  int device_ = 0;
  std::vector<dgs_line_feature> lines_;
  std::vector<int64_t> offsets_;
  std::vector<float> out_;
};

}  // namespace dgs
