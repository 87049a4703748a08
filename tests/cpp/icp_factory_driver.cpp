// ICP_HIP through the C++ factory branch (include/dgs/registrations_hip.hpp) against the PCL-shape stubs: select_hip_registration gives a
// dgs::HipRegistration<ICP> configured from rosparam-style values (registrations.cpp:59-64).  No device is touched: the handle is made at
// the first align.  Prints one JSON line.
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
  pnh.s["reg_use_reciprocal_correspondences"] = (argc > 1 && std::string(argv[1]) == "false") ? "0" : "1";
  auto reg = dgs::select_hip_registration<PointT>(std::string("ICP_HIP"), pnh);
  if (!reg) { std::printf("{\"error\": \"no registration\"}\n"); return 3; }
  Reg* icp = static_cast<Reg*>(reg.get());
  const dgs_icp_options& o = icp->icpOptions();
  auto icp_ref = dgs::select_hip_registration<PointT>(std::string("ICP"), pnh);   // the reference's own branch: not served here
  std::printf("{\"name\": \"%s\", \"reciprocal\": %d, \"fitness_eps\": %g, \"rotation_eps\": %g, \"plain_icp_served\": %d}\n",
              icp->registrationName().c_str(), o.use_reciprocal_correspondences, o.euclidean_fitness_epsilon, o.rotation_epsilon, icp_ref ? 1 : 0);
  return 0;
}
