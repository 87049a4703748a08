// dgs::HipFloorDetector::detectBatch (include/dgs/floor_detection_hip.hpp) against the PCL-shape stubs and the stand-ins of
// tests/stub_eigen.
//   floor_detection_batch_driver n {in.bin filtered.bin floor.bin} x n [name=value ...]
//       -> runs detect() over n clouds of float32 [N,4] points in one device call, writes x, y, z, 1 of every scan's filtered cloud and
//          floor points; one JSON line with the statuses and coefficients (null: boost::none)
#include <cstdio>
#include <cstdlib>
#include <map>
#include <string>
#include <vector>

#include <dgs/floor_detection_hip.hpp>
#include <pcl/point_types.h>

struct Params {   // stands in for ros::NodeHandle::param<T>(name, default)
  std::map<std::string, std::string> s;
  template <class T>
  T param(const std::string& k, const T& d) {
    auto it = s.find(k);
    if (it == s.end()) return d;
    if constexpr (std::is_same<T, bool>::value) return it->second == "true" || it->second == "1";
    else if constexpr (std::is_integral<T>::value) return (T)std::stol(it->second);
    else return (T)std::stod(it->second);
  }
};

static bool write_cloud(const char* path, const pcl::PointCloud<pcl::PointXYZ>& c) {
  FILE* f = std::fopen(path, "wb");
  if (!f) return false;
  for (const auto& p : c.points) {
    const float v[4] = {p.x, p.y, p.z, 1.f};
    std::fwrite(v, sizeof(float), 4, f);
  }
  std::fclose(f);
  return true;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  const int n = std::atoi(argv[1]);
  if (n < 0 || argc < 2 + 3 * n) return 2;
  Params pnh;
  for (int a = 2 + 3 * n; a < argc; a++) {
    const std::string kv = argv[a];
    const size_t eq = kv.find('=');
    if (eq != std::string::npos) pnh.s[kv.substr(0, eq)] = kv.substr(eq + 1);
  }
  dgs::HipFloorDetector<pcl::PointXYZ> det(pnh);
  std::vector<pcl::PointCloud<pcl::PointXYZ>> src((size_t)n);
  std::vector<const pcl::PointCloud<pcl::PointXYZ>*> srcs((size_t)n);
  for (int s = 0; s < n; s++) {
    FILE* f = std::fopen(argv[2 + 3 * s], "rb");
    if (!f) return 3;
    float v[4];
    while (std::fread(v, sizeof(float), 4, f) == 4) {
      pcl::PointXYZ p;
      p.x = v[0];
      p.y = v[1];
      p.z = v[2];
      src[s].points.push_back(p);
    }
    std::fclose(f);
    srcs[s] = &src[s];
  }
  std::vector<boost::optional<Eigen::Vector4f>> floors;
  std::vector<int> status;
  if (!det.detectBatch(srcs, floors, &status)) {
    std::fprintf(stderr, "detectBatch failed: %s\n", det.last_error() ? det.last_error() : "");
    return 1;
  }
  for (int s = 0; s < n; s++) {
    pcl::PointCloud<pcl::PointXYZ> filtered, floor;
    det.batchFiltered(s, filtered);
    det.batchFloorPoints(s, floor);
    if (!write_cloud(argv[2 + 3 * s + 1], filtered) || !write_cloud(argv[2 + 3 * s + 2], floor)) return 4;
  }
  std::printf("{\"status\": [");
  for (int s = 0; s < n; s++) std::printf("%s%d", s ? ", " : "", status[s]);
  std::printf("], \"coeffs\": [");
  for (int s = 0; s < n; s++) {
    if (floors[s]) std::printf("%s[%.9g, %.9g, %.9g, %.9g]", s ? ", " : "", (*floors[s])[0], (*floors[s])[1], (*floors[s])[2], (*floors[s])[3]);
    else std::printf("%snull", s ? ", " : "");
  }
  std::printf("]}\n");
  return 0;
}
