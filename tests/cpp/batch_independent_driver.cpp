// HipRegistration::setBatchIndependent and the factory's dgs_batch_independent parameter (include/dgs/registrations_hip.hpp) against the
// PCL-shape stubs.  No device is needed: the switch is remembered by the object and applied to every handle it makes; without a device no
// handle is ever made and align() fails soft, switch or not.  Prints one JSON line.
#include <cstdio>
#include <map>
#include <string>

#include <dgs/registrations_hip.hpp>

struct Params {   // stands in for ros::NodeHandle::param<T>(name, default)
  std::map<std::string, std::string> s;
  template <class T>
  T param(const std::string& k, const T& d) {
    auto it = s.find(k);
    if (it == s.end()) return d;
    if constexpr (std::is_same<T, std::string>::value) return it->second;
    else if constexpr (std::is_integral<T>::value) return (T)std::stol(it->second);
    else return (T)std::stod(it->second);
  }
};

int main() {
  using PointT = pcl::PointXYZ;
  using Reg = dgs::HipRegistration<PointT, PointT>;
  const char* methods[] = {"FAST_GICP_HIP", "FAST_VGICP_HIP", "ICP_HIP", "GICP_HIP", "PCL_NDT_HIP", "NDT_HIP"};
  int on_count = 0, off_count = 0, served = 0;
  for (const char* m : methods) {
    Params on, off;
    on.s["dgs_batch_independent"] = "1";
    auto a = dgs::select_hip_registration<PointT>(std::string(m), on);
    auto b = dgs::select_hip_registration<PointT>(std::string(m), off);
    if (!a || !b) continue;
    served++;
    on_count += static_cast<Reg*>(a.get())->getBatchIndependent() ? 1 : 0;
    off_count += static_cast<Reg*>(b.get())->getBatchIndependent() ? 0 : 1;
  }
  Params on;
  on.s["dgs_batch_independent"] = "1";
  auto other = dgs::select_hip_registration<PointT>(std::string("GICP"), on);   // the reference's own branch: not served, nothing to switch
  Reg reg(DGS_METHOD_GICP);
  const bool initial = reg.getBatchIndependent();
  reg.setBatchIndependent(true);
  const bool after_on = reg.getBatchIndependent();
  // an align with the switch on: with a device it registers, without one it fails soft (no exception, not converged) -- and keeps the switch
  pcl::PointCloud<PointT>::Ptr cloud(new pcl::PointCloud<PointT>());
  cloud->points.resize(64);
  for (int i = 0; i < 64; i++) { cloud->points[i].x = 0.1f * (i % 8); cloud->points[i].y = 0.1f * (i / 8); cloud->points[i].z = 0.01f * (i % 5); }
  cloud->width = 64;
  cloud->height = 1;
  reg.setInputTarget(cloud);
  reg.setInputSource(cloud);
  pcl::PointCloud<PointT> aligned;
  reg.align(aligned);
  const bool after_align = reg.getBatchIndependent();
  int32_t on_handle = -1;
  if (reg.handle()) dgs_get_batch_independent(reg.handle(), &on_handle);
  reg.setBatchIndependent(false);
  int32_t off_handle = -1;
  if (reg.handle()) dgs_get_batch_independent(reg.handle(), &off_handle);
  std::printf("{\"served\": %d, \"factory_on\": %d, \"factory_default_off\": %d, \"unserved_is_null\": %d, \"initial\": %d, \"after_on\": %d, "
              "\"after_align\": %d, \"after_off\": %d, \"has_handle\": %d, \"handle_on\": %d, \"handle_off\": %d}\n",
              served, on_count, off_count, other ? 0 : 1, initial ? 1 : 0, after_on ? 1 : 0, after_align ? 1 : 0, reg.getBatchIndependent() ? 1 : 0,
              reg.handle() ? 1 : 0, (int)on_handle, (int)off_handle);
  return 0;
}
