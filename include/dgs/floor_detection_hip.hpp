// dgs::HipFloorDetector -- FloorDetectionNodelet::detect (apps/floor_detection_nodelet.cpp:110-180) over libdgs_reg.so
// (include/dgs_reg.h, dgs_floor_detection).  INTEGRATION.md 4h shows the patch to the nodelet.
// Header-only; needs Eigen, boost::optional and pcl::PointCloud at the user's build, as the nodelet does.  Built from the nodelet's
// private parameters (:57-63, same names and defaults).  The tilt matrix and its inverse are built here exactly as detect() builds
// them (Eigen's AngleAxisf and .inverse()), so they carry the bits of the user's Eigen.  The handle is created at the first detect
// call.  On anything but DGS_FD_DETECTED -- a failure of any kind included, which never throws -- detect() returns boost::none;
// status() and last_error() say why.
#pragma once

#include <cmath>
#include <cstring>
#include <vector>

#include <boost/optional.hpp>

#include <Eigen/Core>
#include <Eigen/Geometry>
#include <Eigen/LU>

#include <pcl/point_cloud.h>

#include "../dgs_reg.h"

namespace dgs {

template <typename PointT>
class HipFloorDetector {
 public:
  // NodeHandle: anything with param<T>(name, default), e.g. ros::NodeHandle (private_nh)
  template <typename NodeHandle>
  explicit HipFloorDetector(NodeHandle& private_nh, int device = 0) : device_(device) {
    dgs_floor_detection_params_init(&p_);
    p_.tilt_deg = private_nh.template param<double>("tilt_deg", 0.0);
    p_.sensor_height = private_nh.template param<double>("sensor_height", 2.0);
    p_.height_clip_range = private_nh.template param<double>("height_clip_range", 1.0);
    p_.floor_pts_thresh = private_nh.template param<int>("floor_pts_thresh", 512);
    p_.floor_normal_thresh = private_nh.template param<double>("floor_normal_thresh", 10.0);
    p_.use_normal_filtering = private_nh.template param<bool>("use_normal_filtering", true) ? 1 : 0;
    p_.normal_filter_thresh = private_nh.template param<double>("normal_filter_thresh", 20.0);
  }
  ~HipFloorDetector() {
    if (h_) dgs_destroy(h_);
  }
  HipFloorDetector(const HipFloorDetector&) = delete;
  HipFloorDetector& operator=(const HipFloorDetector&) = delete;

  dgs_floor_detection_params& params() { return p_; }
  const char* last_error() const { return dgs_last_error(h_); }
  int status() const { return status_; }   // dgs_floor_detection_status of the last detect

  boost::optional<Eigen::Vector4f> detect(const pcl::PointCloud<PointT>& cloud) {
    status_ = DGS_FD_TOO_FEW_POINTS;
    const size_t n = cloud.points.size();
    if (!ensure_handle()) return boost::none;
    // :112-113 and :125, :152
    Eigen::Matrix4f tilt = Eigen::Matrix4f::Identity();
    tilt.topLeftCorner(3, 3) = Eigen::AngleAxisf(p_.tilt_deg * M_PI / 180.0f, Eigen::Vector3f::UnitY()).toRotationMatrix();
    const Eigen::Matrix4f tilt_inv = static_cast<Eigen::Matrix4f>(tilt.inverse());
    in_.resize(4 * n);
    for (size_t i = 0; i < n; i++) {   // x, y, z; the fourth float is overwritten by the transform
      std::memcpy(&in_[4 * i], &cloud.points[i], 3 * sizeof(float));
      in_[4 * i + 3] = 1.f;
    }
    float coeffs[4] = {0.f, 0.f, 0.f, 0.f};
    int32_t st = 0;
    if (dgs_floor_detection(h_, &p_, tilt.data(), tilt_inv.data(), in_.data(), (int64_t)n, 0, nullptr, 0, coeffs, &st) != DGS_OK) return boost::none;
    status_ = st;
    if (st != DGS_FD_DETECTED) return boost::none;
    return Eigen::Vector4f(coeffs[0], coeffs[1], coeffs[2], coeffs[3]);
  }

  // detect() over many clouds -- the frames of several streams -- in one device call (dgs_floor_detection_batch): floors[i] is what
  // detect(*clouds[i]) returns, statuses (nullable) receives every scan's dgs_floor_detection_status.  -> false when the call itself
  // failed (last_error() says why); floors then holds boost::none for every scan.
  bool detectBatch(const std::vector<const pcl::PointCloud<PointT>*>& clouds, std::vector<boost::optional<Eigen::Vector4f>>& floors,
                   std::vector<int>* statuses = nullptr) {
    const size_t n = clouds.size();
    floors.assign(n, boost::none);
    if (statuses) statuses->assign(n, DGS_FD_TOO_FEW_POINTS);
    if (!ensure_handle()) return false;
    Eigen::Matrix4f tilt = Eigen::Matrix4f::Identity();
    tilt.topLeftCorner(3, 3) = Eigen::AngleAxisf(p_.tilt_deg * M_PI / 180.0f, Eigen::Vector3f::UnitY()).toRotationMatrix();
    const Eigen::Matrix4f tilt_inv = static_cast<Eigen::Matrix4f>(tilt.inverse());
    std::vector<int64_t> sizes(n);
    size_t total = 0;
    for (size_t s = 0; s < n; s++) {
      if (!clouds[s]) return false;
      sizes[s] = (int64_t)clouds[s]->points.size();
      total += clouds[s]->points.size();
    }
    in_.resize(4 * total + 4);
    std::vector<const float*> ptrs(n);
    size_t off = 0;
    for (size_t s = 0; s < n; s++) {
      ptrs[s] = in_.data() + 4 * off;
      for (const auto& q : clouds[s]->points) {
        std::memcpy(&in_[4 * off], &q, 3 * sizeof(float));
        in_[4 * off + 3] = 1.f;
        off++;
      }
    }
    std::vector<float> coeffs(4 * n + 4, 0.f);
    std::vector<int32_t> st(n + 1, DGS_FD_TOO_FEW_POINTS);
    if (dgs_floor_detection_batch(h_, &p_, tilt.data(), tilt_inv.data(), (int32_t)n, ptrs.data(), sizes.data(), 0, nullptr, nullptr, coeffs.data(), st.data()) !=
        DGS_OK)
      return false;
    for (size_t s = 0; s < n; s++) {
      if (statuses) (*statuses)[s] = st[s];
      if (st[s] == DGS_FD_DETECTED) floors[s] = Eigen::Vector4f(coeffs[4 * s], coeffs[4 * s + 1], coeffs[4 * s + 2], coeffs[4 * s + 3]);
    }
    return true;
  }
  // /floor_detection/floor_filtered_points and /floor_detection/floor_points of scan `i` of the last detectBatch
  template <typename CloudT>
  void batchFiltered(int i, CloudT& out) {
    int64_t m = 0;
    if (!h_ || dgs_floor_detection_batch_get_filtered(h_, i, nullptr, 0, 0, &m) != DGS_OK) m = 0;
    buf_.resize(4 * (size_t)m);
    if (m > 0 && dgs_floor_detection_batch_get_filtered(h_, i, buf_.data(), m, 0, &m) != DGS_OK) m = 0;
    fill(out, m);
  }
  template <typename CloudT>
  void batchFloorPoints(int i, CloudT& out) {
    int64_t m = 0;
    if (!h_ || dgs_floor_detection_batch_get_inliers(h_, i, nullptr, nullptr, 0, &m) != DGS_OK) m = 0;
    buf_.resize(4 * (size_t)m);
    if (m > 0 && dgs_floor_detection_batch_get_inliers(h_, i, nullptr, buf_.data(), m, &m) != DGS_OK) m = 0;
    fill(out, m);
  }

  // /floor_detection/floor_filtered_points and /floor_detection/floor_points of the last detect: x, y, z of every point
  template <typename CloudT>
  void filtered(CloudT& out) {
    int64_t m = 0;
    if (!h_ || dgs_floor_detection_get_filtered(h_, nullptr, 0, 0, &m) != DGS_OK) m = 0;
    buf_.resize(4 * (size_t)m);
    if (m > 0 && dgs_floor_detection_get_filtered(h_, buf_.data(), m, 0, &m) != DGS_OK) m = 0;
    fill(out, m);
  }
  template <typename CloudT>
  void floor_points(CloudT& out) {
    int64_t m = 0;
    if (!h_ || dgs_floor_detection_get_inliers(h_, nullptr, nullptr, 0, &m) != DGS_OK) m = 0;
    buf_.resize(4 * (size_t)m);
    if (m > 0 && dgs_floor_detection_get_inliers(h_, nullptr, buf_.data(), m, &m) != DGS_OK) m = 0;
    fill(out, m);
  }

 private:
  template <typename CloudT>
  void fill(CloudT& out, int64_t m) {
    out.points.resize((size_t)m);
    for (int64_t i = 0; i < m; i++) {
      auto& p = out.points[(size_t)i];
      p.x = buf_[4 * (size_t)i];
      p.y = buf_[4 * (size_t)i + 1];
      p.z = buf_[4 * (size_t)i + 2];
    }
    out.width = (uint32_t)m;
    out.height = 1;
    out.is_dense = false;
  }
  bool ensure_handle() {
    if (h_) return true;
    dgs_params prm;
    if (dgs_params_init(&prm, DGS_METHOD_NDT) != DGS_OK) return false;
    prm.device = device_;
    return dgs_create(&prm, &h_) == DGS_OK;
  }

  dgs_floor_detection_params p_{};
  dgs_handle* h_ = nullptr;
  int device_ = 0;
  int status_ = DGS_FD_TOO_FEW_POINTS;
  std::vector<float> in_, buf_;
};

}  // namespace dgs
