// GICP_HIP / GICP_OMP_HIP through the C++ factory branch (include/dgs/registrations_hip.hpp) against the PCL-shape stubs:
// select_hip_registration gives a dgs::HipRegistration<PCL_GICP> configured from rosparam-style values (registrations.cpp:65-87).
// No device is touched: the handle is made at the first align.  Prints one JSON line.
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

int main(int argc, char** argv) {
  using PointT = pcl::PointXYZ;
  using Reg = dgs::HipRegistration<PointT, PointT>;
  Params pnh;
  pnh.s["reg_transformation_epsilon"] = "0.001";
  pnh.s["reg_maximum_iterations"] = "32";
  pnh.s["reg_max_correspondence_distance"] = "1.5";
  pnh.s["reg_correspondence_randomness"] = "15";
  pnh.s["reg_max_optimizer_iterations"] = "9";
  pnh.s["reg_use_reciprocal_correspondences"] = "1";
  const std::string name = argc > 1 ? argv[1] : "GICP_HIP";
  auto reg = dgs::select_hip_registration<PointT>(name, pnh);
  if (!reg) { std::printf("{\"error\": \"no registration\"}\n"); return 3; }
  Reg* gicp = static_cast<Reg*>(reg.get());
  const dgs_pcl_gicp_options& o = gicp->pclGicpOptions();
  const dgs_params p = gicp->params();
  auto plain = dgs::select_hip_registration<PointT>(std::string("GICP"), pnh);       // the reference's own branches: not served here
  auto omp = dgs::select_hip_registration<PointT>(std::string("GICP_OMP"), pnh);
  std::printf("{\"name\": \"%s\", \"method\": %d, \"transformation_epsilon\": %g, \"maximum_iterations\": %d, \"max_correspondence_distance\": %g, "
              "\"k\": %d, \"max_optimizer_iterations\": %d, \"reciprocal\": %d, \"rotation_epsilon\": %g, \"gicp_epsilon\": %g, "
              "\"plain_gicp_served\": %d, \"gicp_omp_served\": %d}\n",
              gicp->registrationName().c_str(), (int)p.method, p.transformation_epsilon, p.maximum_iterations, p.gicp_max_correspondence_distance,
              p.gicp_correspondence_randomness, o.max_optimizer_iterations, o.use_reciprocal_correspondences, o.rotation_epsilon, o.gicp_epsilon,
              plain ? 1 : 0, omp ? 1 : 0);
  return 0;
}
