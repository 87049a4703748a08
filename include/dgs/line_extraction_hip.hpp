// dgs::HipLineExtractor -- LineBasedScanmatcher::line_extraction (src/hdl_graph_slam/line_based_scanmatcher.cpp:336-457) over
// libdgs_reg.so (include/dgs_reg.h, dgs_line_extraction).  INTEGRATION.md 4d shows the one-line patch to align_global.
// Header-only; needs pcl::PointCloud at the user's build and nothing of the matcher: LineFeatureT is any struct with upstream's six
// fields (pointA, pointB: anything indexable by 0..2 and assignable from double; mean_error, std_sigma, max_error, min_error).
// Built from the nodelet's private parameters (apps/delta_graph_slam_nodelet.cpp:79-96, same names and defaults).  The handle is
// created at the first extract call.  A failure of any kind never throws: extract() returns an empty vector (last_error() says why)
// and the caller falls back to line_extraction.  An unserved delta_SACMethodType is such a failure.
#pragma once

#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include <pcl/point_cloud.h>

#include "../dgs_reg.h"

namespace dgs {

template <typename PointT, typename LineFeatureT>
class HipLineExtractor {
 public:
  // NodeHandle: anything with param<T>(name, default), e.g. ros::NodeHandle (private_nh)
  template <typename NodeHandle>
  explicit HipLineExtractor(NodeHandle& private_nh, int device = 0) : device_(device) {
    dgs_line_extraction_params_init(&p_);
    p_.min_cluster_size = private_nh.template param<int>("delta_MinClusterSize", 25);
    p_.max_cluster_size = private_nh.template param<int>("delta_MaxClusterSize", 25000);
    p_.cluster_tolerance = private_nh.template param<float>("delta_ClusterTolerance", 1.0f);
    p_.sac_distance_threshold = private_nh.template param<float>("delta_SACDistanceThreshold", 0.1f);
    p_.max_iterations = private_nh.template param<int>("delta_Max_iterations", 500);
    p_.merror_threshold = private_nh.template param<float>("delta_Merror_threshold", 150.f);
    p_.line_length_threshold = private_nh.template param<float>("delta_lenght_threshold", 1.f);
    // an unknown name keeps SAC_RANSAC, as the nodelet's loop does (:87-96)
    const std::string method = private_nh.template param<std::string>("delta_SACMethodType", "SAC_RANSAC");
    static const char* const kMethods[] = {"SAC_RANSAC", "SAC_LMEDS", "SAC_MSAC", "SAC_RRANSAC", "SAC_RMSAC", "SAC_MLESAC", "SAC_PROSAC"};
    p_.sac_method_type = 0;
    for (int i = 0; i < 7; i++)
      if (method == kMethods[i]) p_.sac_method_type = i;
  }
  ~HipLineExtractor() {
    if (h_) dgs_destroy(h_);
  }
  HipLineExtractor(const HipLineExtractor&) = delete;
  HipLineExtractor& operator=(const HipLineExtractor&) = delete;

  dgs_line_extraction_params& params() { return p_; }
  const char* last_error() const { return dgs_last_error(h_); }
  int status() const { return status_; }   // dgs_line_extraction_status of the last extract

  std::vector<std::shared_ptr<LineFeatureT>> extract(const pcl::PointCloud<PointT>& cloud) {
    std::vector<std::shared_ptr<LineFeatureT>> lines;
    const size_t n = cloud.points.size();
    if (!ensure_handle()) return lines;
    in_.resize(4 * n);
    for (size_t i = 0; i < n; i++) {   // pcl::PointXYZ: x, y, z and the pad lane
      std::memcpy(&in_[4 * i], &cloud.points[i], 3 * sizeof(float));
      in_[4 * i + 3] = 1.f;
    }
    out_.resize(n / (size_t)(p_.min_cluster_size > 0 ? p_.min_cluster_size : 1) + 1);
    int64_t m = 0;
    int32_t st = 0;
    if (dgs_line_extraction(h_, &p_, in_.data(), (int64_t)n, 0, nullptr, 0, out_.data(), (int64_t)out_.size(), &m, &st) != DGS_OK) return lines;
    status_ = st;
    for (int64_t i = 0; i < m; i++) {
      auto line = std::make_shared<LineFeatureT>();
      for (int a = 0; a < 3; a++) {
        line->pointA[a] = out_[(size_t)i].point_a[a];
        line->pointB[a] = out_[(size_t)i].point_b[a];
      }
      line->mean_error = out_[(size_t)i].mean_error;
      line->std_sigma = out_[(size_t)i].std_sigma;
      line->max_error = out_[(size_t)i].max_error;
      line->min_error = out_[(size_t)i].min_error;
      lines.push_back(line);
    }
    return lines;
  }

 private:
  bool ensure_handle() {
    if (h_) return true;
    dgs_params prm;
    if (dgs_params_init(&prm, DGS_METHOD_NDT) != DGS_OK) return false;
    prm.device = device_;
    return dgs_create(&prm, &h_) == DGS_OK;
  }

  dgs_line_extraction_params p_{};
  dgs_handle* h_ = nullptr;
  int device_ = 0;
  int status_ = 0;
  std::vector<float> in_;
  std::vector<dgs_line_feature> out_;
};

}  // namespace dgs
