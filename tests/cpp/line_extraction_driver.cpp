// dgs::HipLineExtractor (include/dgs/line_extraction_hip.hpp) against the PCL-shape stubs.
//   line_extraction_driver params [name=value ...]            -> one JSON line with the parsed parameters (no device touched)
//   line_extraction_driver run in.bin out.bin [name=value ...] -> extracts from float32 [N,4] points, writes 10 doubles per line
//                                                                 (A, B, mean, sigma, max, min) and prints {"lines", "status"}
#include <cstdio>
#include <cstdlib>
#include <map>
#include <string>
#include <vector>

#include <dgs/line_extraction_hip.hpp>
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

struct Line {   // upstream's LineFeature without Eigen
  double pointA[3], pointB[3];
  double mean_error, std_sigma, max_error, min_error;
};

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  const std::string mode = argv[1];
  const int first_kv = mode == "run" ? 4 : 2;
  if (argc < first_kv) return 2;
  Params pnh;
  for (int a = first_kv; a < argc; a++) {
    const std::string kv = argv[a];
    const size_t eq = kv.find('=');
    if (eq != std::string::npos) pnh.s[kv.substr(0, eq)] = kv.substr(eq + 1);
  }
  dgs::HipLineExtractor<pcl::PointXYZ, Line> ex(pnh);
  const dgs_line_extraction_params& p = ex.params();
  if (mode == "params") {
    std::printf("{\"min_cluster_size\": %d, \"max_cluster_size\": %d, \"cluster_tolerance\": %.9g, \"sac_distance_threshold\": %.9g, "
                "\"max_iterations\": %d, \"merror_threshold\": %.9g, \"line_length_threshold\": %.9g, \"sac_method_type\": %d}\n",
                p.min_cluster_size, p.max_cluster_size, p.cluster_tolerance, p.sac_distance_threshold, p.max_iterations, p.merror_threshold,
                p.line_length_threshold, p.sac_method_type);
    return 0;
  }
  FILE* f = std::fopen(argv[2], "rb");
  if (!f) return 3;
  std::vector<float> buf;
  float v[4];
  while (std::fread(v, sizeof(float), 4, f) == 4) buf.insert(buf.end(), v, v + 4);
  std::fclose(f);
  pcl::PointCloud<pcl::PointXYZ> src;
  src.points.resize(buf.size() / 4);
  for (size_t i = 0; i < src.points.size(); i++) {
    src.points[i].x = buf[4 * i];
    src.points[i].y = buf[4 * i + 1];
    src.points[i].z = buf[4 * i + 2];
  }
  const auto lines = ex.extract(src);
  const char* err = ex.last_error();
  FILE* o = std::fopen(argv[3], "wb");
  if (!o) return 4;
  for (const auto& l : lines) {
    const double rec[10] = {l->pointA[0], l->pointA[1], l->pointA[2], l->pointB[0], l->pointB[1], l->pointB[2], l->mean_error, l->std_sigma,
                            l->max_error, l->min_error};
    std::fwrite(rec, sizeof(double), 10, o);
  }
  std::fclose(o);
  std::printf("{\"lines\": %zu, \"status\": %d, \"error\": \"%s\"}\n", lines.size(), ex.status(), err ? err : "");
  return 0;
}
