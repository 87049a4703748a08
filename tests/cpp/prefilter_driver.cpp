// dgs::HipPrefilter (include/dgs/prefilter_hip.hpp) against the PCL-shape stubs.
//   prefilter_driver params [name=value ...]                     -> one JSON line with the parsed parameters (no device touched)
//   prefilter_driver run in.bin lz out3d.bin out2d.bin [name=value ...] -> runs the chain on float32 [N,4] points, writes x, y, z, 1
#include <cstdio>
#include <cstdlib>
#include <map>
#include <string>
#include <vector>

#include <dgs/prefilter_hip.hpp>
#include <pcl/point_types.h>

struct Params {   // stands in for ros::NodeHandle::param<T>(name, default)
  std::map<std::string, std::string> s;
  template <class T>
  T param(const std::string& k, const T& d) {
    auto it = s.find(k);
    if (it == s.end()) return d;
    if constexpr (std::is_same<T, std::string>::value) return it->second;
    else if constexpr (std::is_same<T, bool>::value) return it->second == "true" || it->second == "1";
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
  const std::string mode = argv[1];
  const int first_kv = mode == "run" ? 6 : 2;
  if (argc < first_kv) return 2;
  Params pnh;
  for (int a = first_kv; a < argc; a++) {
    const std::string kv = argv[a];
    const size_t eq = kv.find('=');
    if (eq != std::string::npos) pnh.s[kv.substr(0, eq)] = kv.substr(eq + 1);
  }
  dgs::HipPrefilter<pcl::PointXYZ> pf(pnh);
  const dgs_prefilter_params& p = pf.params();
  if (mode == "params") {
    std::printf("{\"downsample_method\": %d, \"downsample_resolution\": %.17g, \"outlier_removal_method\": %d, \"statistical_mean_k\": %d, "
                "\"statistical_stddev\": %.17g, \"radius_radius\": %.17g, \"radius_min_neighbors\": %d, \"use_distance_filter\": %d, "
                "\"distance_near_thresh\": %.17g, \"distance_far_thresh\": %.17g}\n",
                p.downsample_method, p.downsample_resolution, p.outlier_removal_method, p.statistical_mean_k, p.statistical_stddev, p.radius_radius,
                p.radius_min_neighbors, p.use_distance_filter, p.distance_near_thresh, p.distance_far_thresh);
    return 0;
  }
  FILE* f = std::fopen(argv[2], "rb");
  if (!f) return 3;
  std::vector<float> buf;
  float v[4];
  while (std::fread(v, sizeof(float), 4, f) == 4) buf.insert(buf.end(), v, v + 4);
  std::fclose(f);
  pcl::PointCloud<pcl::PointXYZ> src, out3, out2;
  src.points.resize(buf.size() / 4);
  for (size_t i = 0; i < src.points.size(); i++) {
    src.points[i].x = buf[4 * i];
    src.points[i].y = buf[4 * i + 1];
    src.points[i].z = buf[4 * i + 2];
  }
  const double lidar[3] = {0.0, 0.0, std::atof(argv[3])};
  if (!pf.filter(src, lidar, out3, out2)) {
    std::fprintf(stderr, "filter failed: %s\n", pf.last_error() ? pf.last_error() : "");
    return 1;
  }
  if (!write_cloud(argv[4], out3) || !write_cloud(argv[5], out2)) return 4;
  std::printf("{\"n3d\": %zu, \"n2d\": %zu}\n", out3.points.size(), out2.points.size());
  return 0;
}
