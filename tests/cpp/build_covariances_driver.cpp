// dgs::HipRegistration::buildCovariances (include/dgs/hip_registration.hpp) against the PCL-shape stubs (tests/stub_pcl): the covariances
// of a few clouds made ahead of the registrations that use them, in one call.
//   build_covariances_driver <method> <clouds> <points per cloud>
// Prints {"ok", "clouds", "counts", "error"}; ok = false without a GPU or for a method that keeps no covariances (the adapter's soft
// failure: no throw), exit code 0 either way; 3 for a method name the factory does not know.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <string>
#include <type_traits>
#include <vector>

#include <dgs/registrations_hip.hpp>

using PointT = pcl::PointXYZ;
using Reg = dgs::HipRegistration<PointT, PointT>;

struct Params {   // stands in for ros::NodeHandle::param<T>(name, default)
  std::map<std::string, double> d;
  template <class T>
  T param(const std::string& k, const T& def) const {
    if constexpr (std::is_arithmetic<T>::value) {
      auto it = d.find(k);
      return it == d.end() ? def : (T)it->second;
    } else {
      return def;
    }
  }
};

int main(int argc, char** argv) {
  if (argc < 4) return 2;
  Params pnh;
  pcl::Registration<PointT, PointT>::Ptr registration = dgs::select_hip_registration<PointT>(argv[1], pnh);
  Reg* hip = dynamic_cast<Reg*>(registration.get());
  if (!hip) { std::printf("{\"error\": \"unknown method\"}\n"); return 3; }
  const int n_clouds = std::atoi(argv[2]), n_points = std::atoi(argv[3]);
  std::vector<pcl::PointCloud<PointT>::ConstPtr> clouds;
  unsigned state = 12345u;
  for (int c = 0; c < n_clouds; c++) {
    pcl::PointCloud<PointT>::Ptr cloud(new pcl::PointCloud<PointT>());
    cloud->points.resize((size_t)n_points);
    for (auto& p : cloud->points) {
      float v[3];
      for (float& x : v) { state = state * 1664525u + 1013904223u; x = (float)(state >> 8) / (float)(1u << 24) * 10.f; }
      p.x = v[0]; p.y = v[1]; p.z = 0.1f * v[2];
    }
    cloud->width = (std::uint32_t)n_points;
    clouds.push_back(cloud);
  }
  clouds.push_back(clouds.front());   // a cloud listed twice is fine
  const bool ok = hip->buildCovariances(clouds);
  std::string err = ok ? "" : hip->lastError();
  for (char& ch : err)
    if (ch == '"' || ch == '\\' || ch == '\n') ch = ' ';
  int64_t counts[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (ok) (void)dgs_cloud_covariances_get_counts(hip->handle(), counts);
  std::printf("{\"ok\": %s, \"clouds\": %d, \"counts\": [%lld, %lld, %lld, %lld, %lld, %lld, %lld, %lld], \"error\": \"%s\"}\n", ok ? "true" : "false", n_clouds,
              (long long)counts[0], (long long)counts[1], (long long)counts[2], (long long)counts[3], (long long)counts[4], (long long)counts[5],
              (long long)counts[6], (long long)counts[7], err.c_str());
  return 0;
}
