// dgs::HipPrefilter::filterScanBatch (include/dgs/prefilter_hip.hpp) against the PCL-shape stubs.
//   prefilter_batch_driver n {in.bin out3d.bin out2d.bin wx,wy,wz|none m0,...,m15|none} x n [name=value ...]
//       -> runs cloud_callback from the raw scan over n scans of float32 [N,4] points in one device call, writes x, y, z, 1 per scan;
//          one JSON line with the statuses, counts and lidar positions
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

static bool parse_list(const std::string& s, size_t want, std::vector<double>* out) {
  out->clear();
  if (s == "none") return true;
  size_t pos = 0;
  while (pos <= s.size()) {
    const size_t c = s.find(',', pos);
    out->push_back(std::stod(s.substr(pos, c == std::string::npos ? std::string::npos : c - pos)));
    if (c == std::string::npos) break;
    pos = c + 1;
  }
  return out->size() == want;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  const int n = std::atoi(argv[1]);
  if (n < 0 || argc < 2 + 5 * n) return 2;
  Params pnh;
  for (int a = 2 + 5 * n; a < argc; a++) {
    const std::string kv = argv[a];
    const size_t eq = kv.find('=');
    if (eq != std::string::npos) pnh.s[kv.substr(0, eq)] = kv.substr(eq + 1);
  }
  dgs::HipPrefilter<pcl::PointXYZ> pf(pnh);
  pf.scan_params().deskew_norm_order = pnh.param<int>("deskew_norm_order", 0);
  pf.scan_params().transform_sets_w = pnh.param<int>("transform_sets_w", 1);
  std::vector<pcl::PointCloud<pcl::PointXYZ>> src((size_t)n), out3, out2;
  std::vector<std::vector<double>> av((size_t)n), m16((size_t)n);
  std::vector<const pcl::PointCloud<pcl::PointXYZ>*> srcs((size_t)n);
  std::vector<const double*> avs((size_t)n), ms((size_t)n);
  for (int s = 0; s < n; s++) {
    char** a = argv + 2 + 5 * s;
    if (!parse_list(a[3], 3, &av[s]) || !parse_list(a[4], 16, &m16[s])) return 2;
    FILE* f = std::fopen(a[0], "rb");
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
    avs[s] = av[s].empty() ? nullptr : av[s].data();
    ms[s] = m16[s].empty() ? nullptr : m16[s].data();
  }
  std::vector<double> lidar((size_t)n * 3, -1.0);
  std::vector<int> status;
  if (!pf.filterScanBatch(srcs, avs.data(), ms.data(), out3, out2, lidar.data(), &status)) {
    std::fprintf(stderr, "filterScanBatch failed: %s\n", pf.last_error() ? pf.last_error() : "");
    return 1;
  }
  for (int s = 0; s < n; s++)
    if (!write_cloud(argv[2 + 5 * s + 1], out3[s]) || !write_cloud(argv[2 + 5 * s + 2], out2[s])) return 4;
  std::printf("{\"status\": [");
  for (int s = 0; s < n; s++) std::printf("%s%d", s ? ", " : "", status[s]);
  std::printf("], \"n3d\": [");
  for (int s = 0; s < n; s++) std::printf("%s%zu", s ? ", " : "", out3[s].points.size());
  std::printf("], \"n2d\": [");
  for (int s = 0; s < n; s++) std::printf("%s%zu", s ? ", " : "", out2[s].points.size());
  std::printf("], \"lidar\": [");
  for (int s = 0; s < n; s++) std::printf("%s[%.17g, %.17g, %.17g]", s ? ", " : "", lidar[3 * s], lidar[3 * s + 1], lidar[3 * s + 2]);
  std::printf("]}\n");
  return 0;
}
