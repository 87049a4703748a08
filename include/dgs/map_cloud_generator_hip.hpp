// dgs::HipMapCloudGenerator -- hdl_graph_slam::MapCloudGenerator::generate (src/hdl_graph_slam/map_cloud_generator.cpp:13-50) over
// libdgs_reg.so (include/dgs_reg.h, dgs_map_cloud_generate).  INTEGRATION.md shows the patch to the nodelet.
// Header-only; needs pcl::PointCloud at the user's build.  generate(keyframes, resolution) has upstream's shape over any range of
// snapshot pointers with ->pose (anything with .matrix(), e.g. Eigen::Isometry3d, or 16 doubles in column-major order) and ->cloud
// (a pointer to a pcl::PointCloud): the voxel centres of the octree in its depth-first order, or the concatenation when
// resolution <= 0.  The handle is created at the first call; an empty list or a failure of any kind returns a null pointer and
// never throws (last_error() has the text).
#pragma once

#include <cstring>
#include <vector>

#include <pcl/point_cloud.h>

#include "../dgs_reg.h"

namespace dgs {

template <typename PointT>
class HipMapCloudGenerator {
 public:
  explicit HipMapCloudGenerator(int device = 0) : device_(device) { dgs_map_cloud_params_init(&p_); }
  ~HipMapCloudGenerator() {
    if (h_) dgs_destroy(h_);
  }
  HipMapCloudGenerator(const HipMapCloudGenerator&) = delete;
  HipMapCloudGenerator& operator=(const HipMapCloudGenerator&) = delete;

  dgs_map_cloud_params& params() { return p_; }
  const char* last_error() const { return dgs_last_error(h_); }

  template <typename Keyframes>
  typename pcl::PointCloud<PointT>::Ptr generate(const Keyframes& keyframes, double resolution) {
    size_t n = 0, total = 0;
    for (const auto& kf : keyframes) {
      n++;
      total += kf->cloud->points.size();
    }
    if (n == 0 || !ensure_handle()) return nullptr;   // "warning: keyframes empty!!" (:14-17)
    in_.resize(4 * total);
    poses_.resize(16 * n);
    ptrs_.resize(n);
    sizes_.resize(n);
    size_t k = 0, off = 0;
    for (const auto& kf : keyframes) {
      pose16(kf->pose, &poses_[16 * k], 0);
      const auto& pts = kf->cloud->points;
      for (size_t i = 0; i < pts.size(); i++) {   // pcl::PointXYZ: x, y, z and the pad lane
        std::memcpy(&in_[4 * (off + i)], &pts[i], 3 * sizeof(float));
        in_[4 * (off + i) + 3] = 1.f;
      }
      ptrs_[k] = pts.empty() ? nullptr : &in_[4 * off];
      sizes_[k] = (int64_t)pts.size();
      off += pts.size();
      k++;
    }
    int64_t m = 0;
    if (dgs_map_cloud_generate(h_, &p_, (int32_t)n, ptrs_.data(), sizes_.data(), 0, poses_.data(), resolution, &m) != DGS_OK) return nullptr;
    out_.resize(4 * (size_t)(m ? m : 1));
    if (dgs_map_cloud_get(h_, out_.data(), m, 0, &m) != DGS_OK) return nullptr;
    typename pcl::PointCloud<PointT>::Ptr cloud(new pcl::PointCloud<PointT>());
    cloud->points.resize((size_t)m);
    for (int64_t i = 0; i < m; i++) {
      cloud->points[i].x = out_[4 * i];
      cloud->points[i].y = out_[4 * i + 1];
      cloud->points[i].z = out_[4 * i + 2];
    }
    cloud->width = (uint32_t)m;
    cloud->height = 1;
    cloud->is_dense = false;
    return cloud;
  }

 private:
  // pose.matrix() (row, column) -> 16 doubles, column-major; or 16 doubles that already are
  template <typename Pose>
  static auto pose16(const Pose& pose, double* o, int) -> decltype(pose.matrix(), void()) {
    const auto& m = pose.matrix();
    for (int c = 0; c < 4; c++)
      for (int r = 0; r < 4; r++) o[c * 4 + r] = (double)m(r, c);
  }
  template <typename Pose>
  static void pose16(const Pose& pose, double* o, long) {
    for (int i = 0; i < 16; i++) o[i] = (double)pose[i];
  }
  bool ensure_handle() {
    if (h_) return true;
    dgs_params prm;
    if (dgs_params_init(&prm, DGS_METHOD_NDT) != DGS_OK) return false;
    prm.device = device_;
    return dgs_create(&prm, &h_) == DGS_OK;
  }

  dgs_map_cloud_params p_{};
  dgs_handle* h_ = nullptr;
  int device_ = 0;
  std::vector<float> in_, out_;
  std::vector<double> poses_;
  std::vector<const float*> ptrs_;
  std::vector<int64_t> sizes_;
};

}  // namespace dgs
