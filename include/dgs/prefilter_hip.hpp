// dgs::HipPrefilter -- PrefilteringNodelet::cloud_callback (apps/prefiltering_nodelet.cpp:111-164) over libdgs_reg.so
// (include/dgs_reg.h): filterScan from the raw scan (deskewing, the base_link transform, then the chain; dgs_prefilter_scan), filter
// from the distance filter to flatten (dgs_prefilter).  INTEGRATION.md shows the patch to the nodelet.
// Header-only; needs pcl::PointCloud at the user's build.  Built from the nodelet's private parameters (initialize_params,
// :55-109, same names and defaults); filter(src, lidar_position, filtered3d, filtered2d) gives what cloud_callback publishes on
// /filtered_points and /flat_filtered_points; filterScan(src, angular_velocity, base_link_matrix, ...) does the same from the scan
// the driver delivers, with dgs::select_imu as the nodelet's search of its IMU queue.  The handle is created at the first filter
// call; a failure of any kind never throws: filter() / filterScan() return false and leave both outputs empty.
// The node handle given to the constructor is read again at every filterScan ("scan_period", :340): it must outlive the filter.
#pragma once

#include <cstring>
#include <functional>
#include <string>
#include <vector>

#include <pcl/point_cloud.h>

#include "../dgs_reg.h"

namespace dgs {

// deskewing's search of the IMU queue (:318-328): the first message stamped after `stamp` (strictly), else the last one; everything
// before the position where the search stopped is erased, so a queue with no later message is emptied.  Queue: any sequence of
// pointers whose elements have ->header.stamp (std::vector / std::deque of sensor_msgs::ImuConstPtr).  Empty queue: a null pointer
// (deskewing returns the cloud as it is, :295-297).
template <typename Queue, typename Stamp>
typename Queue::value_type select_imu(Queue& queue, const Stamp& stamp) {
  if (queue.empty()) return typename Queue::value_type();
  typename Queue::value_type imu_msg = queue.front();
  auto loc = queue.begin();
  for (; loc != queue.end(); loc++) {
    imu_msg = (*loc);
    if ((*loc)->header.stamp > stamp) break;
  }
  queue.erase(queue.begin(), loc);
  return imu_msg;
}

template <typename PointT>
class HipPrefilter {
 public:
  // NodeHandle: anything with param<T>(name, default), e.g. ros::NodeHandle (private_nh)
  template <typename NodeHandle>
  explicit HipPrefilter(NodeHandle& private_nh, int device = 0) : device_(device) {
    dgs_prefilter_params_init(&p_);
    const std::string ds = private_nh.template param<std::string>("downsample_method", "VOXELGRID");
    p_.downsample_method = ds == "VOXELGRID" ? DGS_PF_DOWNSAMPLE_VOXELGRID : ds == "APPROX_VOXELGRID" ? DGS_PF_DOWNSAMPLE_APPROX_VOXELGRID : DGS_PF_DOWNSAMPLE_NONE;
    p_.downsample_resolution = private_nh.template param<double>("downsample_resolution", 0.1);
    const std::string om = private_nh.template param<std::string>("outlier_removal_method", "STATISTICAL");
    p_.outlier_removal_method = om == "STATISTICAL" ? DGS_PF_OUTLIER_STATISTICAL : om == "RADIUS" ? DGS_PF_OUTLIER_RADIUS : DGS_PF_OUTLIER_NONE;
    p_.statistical_mean_k = private_nh.template param<int>("statistical_mean_k", 20);
    p_.statistical_stddev = private_nh.template param<double>("statistical_stddev", 1.0);
    p_.radius_radius = private_nh.template param<double>("radius_radius", 0.8);
    p_.radius_min_neighbors = private_nh.template param<int>("radius_min_neighbors", 2);
    p_.use_distance_filter = private_nh.template param<bool>("use_distance_filter", true) ? 1 : 0;   // read and ignored, as upstream (:153)
    p_.distance_near_thresh = private_nh.template param<double>("distance_near_thresh", 1.0);
    p_.distance_far_thresh = private_nh.template param<double>("distance_far_thresh", 100.0);
    dgs_prefilter_scan_params_init(&sp_);
    NodeHandle* nh = &private_nh;
    scan_period_ = [nh]() { return nh->template param<double>("scan_period", 0.1); };
  }
  ~HipPrefilter() {
    if (h_) dgs_destroy(h_);
  }
  HipPrefilter(const HipPrefilter&) = delete;
  HipPrefilter& operator=(const HipPrefilter&) = delete;

  const dgs_prefilter_params& params() const { return p_; }
  dgs_prefilter_scan_params& scan_params() { return sp_; }   // deskew_norm_order, transform_sets_w; the rest is set per call
  const char* last_error() const { return dgs_last_error(h_); }

  bool filter(const pcl::PointCloud<PointT>& src, const double lidar_position[3], pcl::PointCloud<PointT>& filtered3d, pcl::PointCloud<PointT>& filtered2d) {
    filtered3d.points.clear();
    filtered2d.points.clear();
    const size_t n = src.points.size();
    if (!ensure_handle()) return false;
    pack(src);
    int64_t n3 = 0, n2 = 0;
    if (dgs_prefilter(h_, &p_, in_.data(), (int64_t)n, 0, lidar_position, out3_.data(), (int64_t)n, out2_.data(), (int64_t)n, 0, &n3, &n2) != DGS_OK)
      return false;
    unpack(out3_, n3, filtered3d);
    unpack(out2_, n2, filtered2d);
    return true;
  }

  // cloud_callback from :120 to :160.  angular_velocity: imu_msg->angular_velocity x, y, z of the message select_imu chose, null when
  // the queue was empty (no deskewing).  base_link_matrix16: transform_isometry.matrix() row-major (tf::transformTFToEigen, :138), null
  // when base_link_frame is empty; m(0,3) and m(1,3) are zeroed here (:141-142).  lidar_position_out (3 doubles, nullable) receives
  // lidar_position (:113, :143).
  bool filterScan(const pcl::PointCloud<PointT>& src, const double* angular_velocity, const double* base_link_matrix16,
                  pcl::PointCloud<PointT>& filtered3d, pcl::PointCloud<PointT>& filtered2d, double* lidar_position_out) {
    filtered3d.points.clear();
    filtered2d.points.clear();
    const size_t n = src.points.size();
    if (!ensure_handle()) return false;
    pack(src);
    sp_.has_angular_velocity = angular_velocity ? 1 : 0;
    for (int a = 0; a < 3; a++) sp_.angular_velocity[a] = angular_velocity ? angular_velocity[a] : 0.0;
    sp_.scan_period = scan_period_();
    sp_.has_transform = base_link_matrix16 ? 1 : 0;
    for (int a = 0; a < 16; a++) sp_.transform[a] = base_link_matrix16 ? base_link_matrix16[a] : (a % 5 == 0 ? 1.0 : 0.0);
    sp_.transform[3] = 0.0;   // lidar scans should be centered in base_link
    sp_.transform[7] = 0.0;
    int64_t n3 = 0, n2 = 0;
    if (dgs_prefilter_scan(h_, &p_, &sp_, in_.data(), (int64_t)n, 0, out3_.data(), (int64_t)n, out2_.data(), (int64_t)n, 0, &n3, &n2,
                           lidar_position_out) != DGS_OK)
      return false;
    unpack(out3_, n3, filtered3d);
    unpack(out2_, n2, filtered2d);
    return true;
  }

  // filterScan over many scans in one device call (dgs_prefilter_scan_batch): the frames of several streams.  srcs / filtered3d /
  // filtered2d: one cloud per scan; angular_velocities / base_link_matrices16: one pointer per scan (a null entry: none for that scan)
  // or null for all; lidar_positions_out (3 doubles per scan, nullable); statuses_out (nullable): what filterScan's device call would
  // have returned for each scan.  Scan i receives the bits filterScan gives it alone.  false: the call itself failed, every output empty;
  // a scan whose status is not DGS_OK has empty outputs and does not fail the call.
  bool filterScanBatch(const std::vector<const pcl::PointCloud<PointT>*>& srcs, const double* const* angular_velocities,
                       const double* const* base_link_matrices16, std::vector<pcl::PointCloud<PointT>>& filtered3d,
                       std::vector<pcl::PointCloud<PointT>>& filtered2d, double* lidar_positions_out, std::vector<int>* statuses_out) {
    const size_t n = srcs.size();
    filtered3d.assign(n, pcl::PointCloud<PointT>());
    filtered2d.assign(n, pcl::PointCloud<PointT>());
    if (statuses_out) statuses_out->assign(n, DGS_OK);
    if (!ensure_handle()) return false;
    if (n == 0) return true;
    std::vector<std::vector<float>> in(n), o3(n), o2(n);
    std::vector<const float*> in_p(n);
    std::vector<float*> o3_p(n), o2_p(n);
    std::vector<int64_t> sizes(n), n3(n, 0), n2(n, 0);
    std::vector<int32_t> status(n, 0);
    std::vector<dgs_prefilter_scan_params> sps(n, sp_);
    const double period = scan_period_();
    for (size_t s = 0; s < n; s++) {
      const pcl::PointCloud<PointT>& src = *srcs[s];
      const size_t m = src.points.size();
      in[s].resize(4 * (m ? m : 1));
      for (size_t i = 0; i < m; i++) {
        std::memcpy(&in[s][4 * i], &src.points[i], 3 * sizeof(float));
        in[s][4 * i + 3] = 1.f;
      }
      o3[s].resize(4 * (m ? m : 1));
      o2[s].resize(4 * (m ? m : 1));
      in_p[s] = in[s].data();
      o3_p[s] = o3[s].data();
      o2_p[s] = o2[s].data();
      sizes[s] = (int64_t)m;
      const double* av = angular_velocities ? angular_velocities[s] : nullptr;
      const double* m16 = base_link_matrices16 ? base_link_matrices16[s] : nullptr;
      dgs_prefilter_scan_params& sp = sps[s];
      sp.has_angular_velocity = av ? 1 : 0;
      for (int a = 0; a < 3; a++) sp.angular_velocity[a] = av ? av[a] : 0.0;
      sp.scan_period = period;
      sp.has_transform = m16 ? 1 : 0;
      for (int a = 0; a < 16; a++) sp.transform[a] = m16 ? m16[a] : (a % 5 == 0 ? 1.0 : 0.0);
      sp.transform[3] = 0.0;   // lidar scans should be centered in base_link
      sp.transform[7] = 0.0;
    }
    if (dgs_prefilter_scan_batch(h_, &p_, (int32_t)n, sps.data(), in_p.data(), sizes.data(), 0, o3_p.data(), sizes.data(), o2_p.data(), sizes.data(), 0, n3.data(),
                                 n2.data(), lidar_positions_out, status.data()) != DGS_OK)
      return false;
    for (size_t s = 0; s < n; s++) {
      if (statuses_out) (*statuses_out)[s] = status[s];
      if (status[s] != DGS_OK) continue;
      unpack(o3[s], n3[s], filtered3d[s]);
      unpack(o2[s], n2[s], filtered2d[s]);
    }
    return true;
  }

 private:
  bool ensure_handle() {
    if (h_) return true;
    dgs_params prm;
    if (dgs_params_init(&prm, DGS_METHOD_NDT) != DGS_OK) return false;
    prm.device = device_;
    return dgs_create(&prm, &h_) == DGS_OK;
  }
  void pack(const pcl::PointCloud<PointT>& src) {
    const size_t n = src.points.size();
    in_.resize(4 * n);
    for (size_t i = 0; i < n; i++) {   // pcl::PointXYZ: x, y, z and the pad lane
      std::memcpy(&in_[4 * i], &src.points[i], 3 * sizeof(float));
      in_[4 * i + 3] = 1.f;
    }
    out3_.resize(4 * (n ? n : 1));
    out2_.resize(4 * (n ? n : 1));
  }
  static void unpack(const std::vector<float>& buf, int64_t m, pcl::PointCloud<PointT>& out) {
    out.points.resize((size_t)m);
    for (int64_t i = 0; i < m; i++) {
      out.points[i].x = buf[4 * i];
      out.points[i].y = buf[4 * i + 1];
      out.points[i].z = buf[4 * i + 2];
    }
    out.width = (uint32_t)m;
    out.height = 1;
    out.is_dense = false;
  }

  dgs_prefilter_params p_{};
  dgs_prefilter_scan_params sp_{};
  std::function<double()> scan_period_;
  dgs_handle* h_ = nullptr;
  int device_ = 0;
  std::vector<float> in_, out3_, out2_;
};

}  // namespace dgs
