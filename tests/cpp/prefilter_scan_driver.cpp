// dgs::HipPrefilter::filterScan and dgs::select_imu (include/dgs/prefilter_hip.hpp) against the PCL-shape stubs.
//   prefilter_scan_driver select scan_stamp [stamp ...]
//       -> one JSON line: the stamp select_imu chose (null on an empty queue) and the stamps left in the queue (no device touched)
//   prefilter_scan_driver run in.bin out3d.bin out2d.bin wx,wy,wz|none m0,...,m15|none [name=value ...]
//       -> runs cloud_callback from the raw scan on float32 [N,4] points, writes x, y, z, 1; one JSON line with counts and lidar_position
#include <cstdio>
#include <cstdlib>
#include <deque>
#include <map>
#include <memory>
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

struct Imu {   // the shape of sensor_msgs::Imu that deskewing reads
  struct Header { double stamp; } header;
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
  const std::string mode = argv[1];
  if (mode == "select") {
    if (argc < 3) return 2;
    std::deque<std::shared_ptr<const Imu>> queue;
    for (int a = 3; a < argc; a++) queue.push_back(std::make_shared<const Imu>(Imu{{std::atof(argv[a])}}));
    const std::shared_ptr<const Imu> chosen = dgs::select_imu(queue, std::atof(argv[2]));
    if (chosen) std::printf("{\"chosen\": %.17g, \"left\": [", chosen->header.stamp);
    else std::printf("{\"chosen\": null, \"left\": [");
    for (size_t i = 0; i < queue.size(); i++) std::printf("%s%.17g", i ? ", " : "", queue[i]->header.stamp);
    std::printf("]}\n");
    return 0;
  }
  if (mode != "run" || argc < 7) return 2;
  Params pnh;
  for (int a = 7; a < argc; a++) {
    const std::string kv = argv[a];
    const size_t eq = kv.find('=');
    if (eq != std::string::npos) pnh.s[kv.substr(0, eq)] = kv.substr(eq + 1);
  }
  std::vector<double> av, m16;
  if (!parse_list(argv[5], 3, &av) || !parse_list(argv[6], 16, &m16)) return 2;
  dgs::HipPrefilter<pcl::PointXYZ> pf(pnh);
  pf.scan_params().deskew_norm_order = pnh.param<int>("deskew_norm_order", 0);
  pf.scan_params().transform_sets_w = pnh.param<int>("transform_sets_w", 1);
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
  double lidar[3] = {-1.0, -1.0, -1.0};
  if (!pf.filterScan(src, av.empty() ? nullptr : av.data(), m16.empty() ? nullptr : m16.data(), out3, out2, lidar)) {
    std::fprintf(stderr, "filterScan failed: %s\n", pf.last_error() ? pf.last_error() : "");
    return 1;
  }
  if (!write_cloud(argv[3], out3) || !write_cloud(argv[4], out2)) return 4;
  std::printf("{\"n3d\": %zu, \"n2d\": %zu, \"lidar\": [%.17g, %.17g, %.17g]}\n", out3.points.size(), out2.points.size(), lidar[0], lidar[1], lidar[2]);
  return 0;
}
