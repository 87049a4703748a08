// PCL_NDT_HIP through the C++ factory branch (include/dgs/registrations_hip.hpp) against the PCL-shape stubs: select_hip_registration
// gives a dgs::HipRegistration<PCL_NDT> configured from the three rosparams of registrations.cpp:97-99, and PCL's own setters
// (setResolution, setStepSize, setOulierRatio) reach dgs_params.  No device is touched: the handle is made at the first align.
// Prints one JSON line.
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
  Params defaults, pnh;
  pnh.s["reg_transformation_epsilon"] = "0.001";
  pnh.s["reg_maximum_iterations"] = "32";
  pnh.s["reg_resolution"] = "1.5";
  pnh.s["reg_num_threads"] = "7";                  // not read by this branch
  pnh.s["reg_nn_search_method"] = "DIRECT1";       // nor this
  auto d = dgs::select_hip_registration<PointT>(std::string("PCL_NDT_HIP"), defaults);
  auto reg = dgs::select_hip_registration<PointT>(std::string("PCL_NDT_HIP"), pnh);
  if (!d || !reg) { std::printf("{\"error\": \"no registration\"}\n"); return 3; }
  const dgs_params pd = static_cast<Reg*>(d.get())->params();
  Reg* ndt = static_cast<Reg*>(reg.get());
  const dgs_params p = ndt->params();
  ndt->setResolution(2.0f);
  ndt->setStepSize(0.2);
  ndt->setOulierRatio(0.4);
  const dgs_params q = ndt->params();
  auto plain = dgs::select_hip_registration<PointT>(std::string("NDT"), pnh);   // the reference's own branch: not served here
  auto foo = dgs::select_hip_registration<PointT>(std::string("FOO"), pnh);
  std::printf("{\"name\": \"%s\", \"method\": %d, \"default_resolution\": %g, \"default_epsilon\": %g, \"default_iterations\": %d, "
              "\"default_step_size\": %g, \"default_outlier_ratio\": %g, \"resolution\": %g, \"transformation_epsilon\": %g, "
              "\"maximum_iterations\": %d, \"num_threads\": %d, \"set_resolution\": %g, \"set_step_size\": %g, \"set_outlier_ratio\": %g, "
              "\"plain_ndt_served\": %d, \"foo_served\": %d}\n",
              ndt->registrationName().c_str(), (int)p.method, pd.ndt_resolution, pd.transformation_epsilon, pd.maximum_iterations, pd.ndt_step_size,
              pd.ndt_outlier_ratio, p.ndt_resolution, p.transformation_epsilon, p.maximum_iterations, p.num_threads, q.ndt_resolution, q.ndt_step_size,
              q.ndt_outlier_ratio, plain ? 1 : 0, foo ? 1 : 0);
  return 0;
}
