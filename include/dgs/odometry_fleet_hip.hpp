// dgs::HipOdometryFleet -- B independent ScanMatchingOdometryNodelet::matching streams (apps/scan_matching_odometry_nodelet.cpp:173-270)
// advanced by one frame each in one chain of device calls over libdgs_reg.so (include/dgs_reg.h): dgs_cloud_assign_batch
// down-samples all frames into resident clouds, dgs_align_pairs_clouds registers every (keyframe, frame) pair together, and
// dgs_calc_inlier_fraction_batch_clouds counts the inliers of publish_scan_matching_status (:321-332) when somebody listens.  Launches
// and host waits of a step do not grow with B.
// Header-only and free of ROS and PCL: a frame is n 16-byte x, y, z, pad points (pcl::PointXYZ's layout), a pose an Eigen::Matrix4f (anything
// with column-major data() and operator()(row, col) will do).  Every stream owns two resident clouds, keyframe and frame; at a keyframe
// switch they are swapped, so the new keyframe keeps the index and covariances it made as a source (fast_gicp's swapSourceAndTarget case).
// The registration must be one dgs_align_pairs_clouds serves (FAST_GICP, GICP_HIP); the library names any other method in lastError().
// A failure never throws: step() returns false, lastError() says why, and no stream has advanced past its down-sampling.
#pragma once

#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include <Eigen/Core>

#include "../dgs_reg.h"

namespace dgs {

struct OdometryStreamParams {   // initialize_params (:64-106); the defaults are the nodelet's
  double keyframe_delta_trans = 0.25, keyframe_delta_angle = 0.15, keyframe_delta_time = 1.0;
  bool transform_thresholding = false;
  double max_acceptable_trans = 1.0, max_acceptable_angle = 1.0;
  template <class Params>
  void load(Params& pnh) {
    keyframe_delta_trans = pnh.template param<double>("keyframe_delta_trans", 0.25);
    keyframe_delta_angle = pnh.template param<double>("keyframe_delta_angle", 0.15);
    keyframe_delta_time = pnh.template param<double>("keyframe_delta_time", 1.0);
    transform_thresholding = pnh.template param<bool>("transform_thresholding", false);
    max_acceptable_trans = pnh.template param<double>("max_acceptable_trans", 1.0);
    max_acceptable_angle = pnh.template param<double>("max_acceptable_angle", 1.0);
  }
};

class HipOdometryFleet {
 public:
  using Matrix4 = Eigen::Matrix4f;
  enum Downsample { NONE = 0, VOXELGRID = 1, APPROX_VOXELGRID = 2 };   // dgs_cloud_assign_batch's filter
  struct Frame {            // one stream's input of a step; points == nullptr: the stream is not touched
    const float* points = nullptr;   // n x (x, y, z, pad), host memory
    int64_t n = 0;
    double stamp = 0.0;
  };
  struct Status {           // msg/ScanMatchingStatus.msg, the fields the registration feeds
    bool has_converged = false;
    double matching_error = 0.0, inlier_fraction = 0.0;
    Matrix4 relative_pose;
  };

  HipOdometryFleet(const dgs_params& registration, const std::vector<OdometryStreamParams>& streams, Downsample method = VOXELGRID, float resolution = 0.1f,
                   bool batch_independent = false)
      : params_(registration), method_(method), resolution_(resolution), batch_independent_(batch_independent), streams_(streams.size()) {
    for (size_t i = 0; i < streams.size(); i++) streams_[i].prm = streams[i];
  }
  ~HipOdometryFleet() {
    for (Stream& s : streams_) {
      if (s.key) dgs_cloud_destroy(s.key);
      if (s.frame) dgs_cloud_destroy(s.frame);
    }
    if (h_) dgs_destroy(h_);
  }
  HipOdometryFleet(const HipOdometryFleet&) = delete;
  HipOdometryFleet& operator=(const HipOdometryFleet&) = delete;

  size_t size() const { return streams_.size(); }
  std::string lastError() const { return error_.empty() ? std::string(dgs_last_error(h_)) : error_; }
  dgs_handle* handle() { return h_; }
  int keyframes(size_t stream) const { return streams_[stream].n_keyframes; }
  const Matrix4& odom(size_t stream) const { return streams_[stream].odom; }
  const Status& status(size_t stream) const { return streams_[stream].status; }   // of the stream's last registered frame, after a step with want_status

  // One frame per stream.  (*odoms)[i]: the pose of stream i's frame in its odometry frame (its last one for an untouched stream).
  bool step(const std::vector<Frame>& frames, std::vector<Matrix4>* odoms, bool want_status = false, const std::vector<Matrix4>* msf_deltas = nullptr) {
    error_.clear();
    const size_t B = streams_.size();
    if (!odoms || frames.size() != B || (msf_deltas && msf_deltas->size() != B)) { error_ = "HipOdometryFleet::step: one frame (and delta) per stream"; return false; }
    if (!ensure_handle()) return false;
    std::vector<size_t> live;
    for (size_t i = 0; i < B; i++)
      if (frames[i].points) live.push_back(i);
    // 1. every live frame into its stream's frame cloud
    in_.clear(); sizes_.clear(); c1_.clear();
    for (size_t i : live) {
      in_.push_back(frames[i].points);
      sizes_.push_back(frames[i].n);
      c1_.push_back(streams_[i].frame);
    }
    out_sizes_.assign(live.size() + 1, 0);
    if (dgs_cloud_assign_batch(h_, (int32_t)live.size(), in_.data(), sizes_.data(), 0, (int32_t)method_, resolution_, c1_.data(), out_sizes_.data()) != DGS_OK) return false;
    // 2. first frames become keyframes (:174-183)
    std::vector<size_t> rest;
    for (size_t i : live) {
      Stream& s = streams_[i];
      if (s.n_keyframes == 0) {
        std::swap(s.key, s.frame);
        s.prev_trans = s.keyframe_pose = s.odom = Matrix4::Identity();
        s.keyframe_stamp = frames[i].stamp;
        s.n_keyframes = 1;
      } else {
        rest.push_back(i);
      }
    }
    if (!rest.empty()) {
      // 3. one registration of all (keyframe, frame) pairs from prev_trans * msf_delta (:189-207)
      const size_t n = rest.size();
      c1_.clear(); c2_.clear();
      guess_.assign(n * 16, 0.f);
      for (size_t k = 0; k < n; k++) {
        const Stream& s = streams_[rest[k]];
        c1_.push_back(s.key);
        c2_.push_back(s.frame);
        const Matrix4 g = msf_deltas ? mul(s.prev_trans, (*msf_deltas)[rest[k]]) : s.prev_trans;
        std::memcpy(&guess_[k * 16], g.data(), sizeof(float) * 16);
      }
      res_.resize(n);
      if (dgs_align_pairs_clouds(h_, (int32_t)n, c1_.data(), c2_.data(), guess_.data(), want_status ? 1 : 0, 1.7976931348623157e308, res_.data()) != DGS_OK) return false;
      // 4. the inlier fractions under the final transforms (:321-332: d^2 < 0.5 * 0.5)
      if (want_status) {
        for (size_t k = 0; k < n; k++) std::memcpy(&guess_[k * 16], res_[k].final_transformation, sizeof(float) * 16);
        frac_.assign(n, 0.0);
        if (dgs_calc_inlier_fraction_batch_clouds(h_, (int32_t)n, c1_.data(), c2_.data(), guess_.data(), 0.5 * 0.5, frac_.data(), nullptr) != DGS_OK) return false;
      }
      // 5. / 6. the decisions of matching per stream (:222-260); a keyframe switch swaps the stream's two clouds
      for (size_t k = 0; k < n; k++) {
        Stream& s = streams_[rest[k]];
        Matrix4 trans;
        std::memcpy(trans.data(), res_[k].final_transformation, sizeof(float) * 16);
        const bool converged = res_[k].converged != 0 && res_[k].status == DGS_OK;
        if (want_status) s.status = Status{converged, res_[k].fitness, frac_[k], trans};
        s.odom = decide(s, frames[rest[k]].stamp, converged, trans);
      }
    }
    odoms->resize(B);
    for (size_t i = 0; i < B; i++) (*odoms)[i] = streams_[i].odom;
    return true;
  }

 private:
  struct Stream {
    OdometryStreamParams prm;
    dgs_cloud* key = nullptr;
    dgs_cloud* frame = nullptr;
    Matrix4 keyframe_pose = Matrix4::Identity(), prev_trans = Matrix4::Identity(), odom = Matrix4::Identity();
    double keyframe_stamp = 0.0;
    int n_keyframes = 0;
    Status status;
  };

  static Matrix4 mul(const Matrix4& a, const Matrix4& b) {   // float products summed in k order, as Eigen's 4 x 4 product rounds them
    Matrix4 c;
    for (int r = 0; r < 4; r++)
      for (int col = 0; col < 4; col++) {
        float s = a(r, 0) * b(0, col);
        for (int k = 1; k < 4; k++) s += a(r, k) * b(k, col);
        c(r, col) = s;
      }
    return c;
  }
  static Matrix4 rigid_inverse_times(const Matrix4& a, const Matrix4& b) {   // a^-1 * b for a rigid a
    Matrix4 ai = Matrix4::Identity();
    for (int r = 0; r < 3; r++) {
      for (int c = 0; c < 3; c++) ai(r, c) = a(c, r);
      ai(r, 3) = -(a(0, r) * a(0, 3) + a(1, r) * a(1, 3) + a(2, r) * a(2, 3));
    }
    return mul(ai, b);
  }
  static double translation(const Matrix4& t) { return std::sqrt((double)t(0, 3) * t(0, 3) + (double)t(1, 3) * t(1, 3) + (double)t(2, 3) * t(2, 3)); }
  static double angle(const Matrix4& t) {   // acos(Quaternionf(R).w())
    const double tr = (double)t(0, 0) + t(1, 1) + t(2, 2);
    double w;
    if (tr > 0) {
      w = 0.5 * std::sqrt(tr + 1.0);
    } else {
      int i = 0;
      if (t(1, 1) > t(0, 0)) i = 1;
      if (t(2, 2) > t(i, i)) i = 2;
      const int j = (i + 1) % 3, k = (i + 2) % 3;
      const double s = std::sqrt((double)t(i, i) - t(j, j) - t(k, k) + 1.0);
      w = ((double)t(k, j) - t(j, k)) * 0.5 / s;
    }
    return std::acos(w < -1.0 ? -1.0 : w > 1.0 ? 1.0 : w);
  }

  Matrix4 decide(Stream& s, double stamp, bool converged, const Matrix4& trans) {
    if (!converged) return mul(s.keyframe_pose, s.prev_trans);   // "ignore this frame"
    const Matrix4 odom = mul(s.keyframe_pose, trans);
    if (s.prm.transform_thresholding) {
      const Matrix4 d = rigid_inverse_times(s.prev_trans, trans);
      if (translation(d) > s.prm.max_acceptable_trans || angle(d) > s.prm.max_acceptable_angle) return mul(s.keyframe_pose, s.prev_trans);   // "too large transform"
    }
    s.prev_trans = trans;
    if (translation(trans) > s.prm.keyframe_delta_trans || angle(trans) > s.prm.keyframe_delta_angle || stamp - s.keyframe_stamp > s.prm.keyframe_delta_time) {
      std::swap(s.key, s.frame);
      s.keyframe_pose = odom;
      s.keyframe_stamp = stamp;
      s.prev_trans = Matrix4::Identity();
      s.n_keyframes++;
    }
    return odom;
  }

  bool ensure_handle() {
    if (h_) return true;
    if (dgs_create(&params_, &h_) != DGS_OK) { error_ = dgs_last_error(nullptr); h_ = nullptr; return false; }
    if (batch_independent_ && dgs_set_batch_independent(h_, 1) != DGS_OK) return false;
    for (Stream& s : streams_)
      if (dgs_cloud_create(h_, nullptr, 0, 0, &s.key) != DGS_OK || dgs_cloud_create(h_, nullptr, 0, 0, &s.frame) != DGS_OK) return false;
    return true;
  }

  dgs_params params_;
  Downsample method_;
  float resolution_;
  bool batch_independent_;
  std::vector<Stream> streams_;
  dgs_handle* h_ = nullptr;
  std::string error_;
  std::vector<const float*> in_;
  std::vector<int64_t> sizes_, out_sizes_;
  std::vector<dgs_cloud*> c1_, c2_;
  std::vector<float> guess_;
  std::vector<double> frac_;
  std::vector<dgs_result> res_;
};

}  // namespace dgs
