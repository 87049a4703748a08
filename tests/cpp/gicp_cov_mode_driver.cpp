// The covariance mode of FAST_GICP_HIP / FAST_VGICP_HIP through the C++ adapter against the PCL-shape stubs: the factory branch reads the optional
// reg_covariance_upstream_order parameter (default false), HipRegistration::setCovarianceMode writes dgs_params.gicp_cov_jacobi_svd.
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
  const std::string name = argc > 1 ? argv[1] : "FAST_GICP_HIP";
  Params plain, upstream, off;
  plain.s["reg_correspondence_randomness"] = "15";
  upstream.s["reg_correspondence_randomness"] = "15";
  upstream.s["reg_covariance_upstream_order"] = "1";
  off.s["reg_covariance_upstream_order"] = "0";
  auto a = dgs::select_hip_registration<PointT>(name, plain);
  auto b = dgs::select_hip_registration<PointT>(name, upstream);
  auto c = dgs::select_hip_registration<PointT>(name, off);
  if (!a || !b || !c) { std::printf("{\"error\": \"no registration\"}\n"); return 3; }
  const dgs_params pa = static_cast<Reg*>(a.get())->params(), pb = static_cast<Reg*>(b.get())->params(), pc = static_cast<Reg*>(c.get())->params();
  Reg* set = static_cast<Reg*>(a.get());
  set->setCovarianceMode(DGS_GICP_COV_JACOBI_SVD);
  const int after_1 = set->params().gicp_cov_jacobi_svd;
  set->setCovarianceMode(DGS_GICP_COV_UPSTREAM_ORDER);
  const int after_2 = set->params().gicp_cov_jacobi_svd;
  set->setCovarianceMode(DGS_GICP_COV_SYM_EIG);
  const int after_0 = set->params().gicp_cov_jacobi_svd;
  std::printf("{\"method\": %d, \"k\": %d, \"default\": %d, \"with_parameter\": %d, \"parameter_false\": %d, \"set_1\": %d, \"set_2\": %d, \"set_0\": %d, "
              "\"enum\": [%d, %d, %d]}\n",
              (int)pb.method, pb.gicp_correspondence_randomness, pa.gicp_cov_jacobi_svd, pb.gicp_cov_jacobi_svd, pc.gicp_cov_jacobi_svd, after_1, after_2, after_0,
              (int)DGS_GICP_COV_SYM_EIG, (int)DGS_GICP_COV_JACOBI_SVD, (int)DGS_GICP_COV_UPSTREAM_ORDER);
  return 0;
}
