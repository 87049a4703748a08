// dgs::HipMapCloudGenerator (include/dgs/map_cloud_generator_hip.hpp) against the PCL-shape stubs.
//   map_cloud_driver run in.bin resolution out.bin [matrix]
// in.bin: int32 keyframes, then per keyframe int32 points, 16 doubles (the pose, column-major), points x 4 floats.  Writes x, y, z, 1
// per map point and prints one JSON line; a null result prints {"null": true}.  With `matrix` the snapshots carry a pose object with
// .matrix() (Eigen::Isometry3d's shape) instead of double[16].
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <string>
#include <vector>

#include <Eigen/Core>
#include <dgs/map_cloud_generator_hip.hpp>
#include <pcl/point_types.h>

using Cloud = pcl::PointCloud<pcl::PointXYZ>;

struct Isometry3d {   // stands in for Eigen::Isometry3d
  Eigen::Matrix<double, 4, 4> m;
  const Eigen::Matrix<double, 4, 4>& matrix() const { return m; }
};
struct SnapshotArray {   // stands in for hdl_graph_slam::KeyFrameSnapshot
  double pose[16];
  Cloud::ConstPtr cloud;
};
struct SnapshotMatrix {
  Isometry3d pose;
  Cloud::ConstPtr cloud;
};

template <class Snapshots>
static int run(const Snapshots& snaps, double resolution, const char* out_path) {
  dgs::HipMapCloudGenerator<pcl::PointXYZ> gen;
  Cloud::Ptr map = gen.generate(snaps, resolution);
  if (!map) {
    const char* e = gen.last_error();
    std::printf("{\"null\": true, \"error\": \"%s\"}\n", e ? e : "");
    return 0;
  }
  FILE* f = std::fopen(out_path, "wb");
  if (!f) return 4;
  for (const auto& p : map->points) {
    const float v[4] = {p.x, p.y, p.z, 1.f};
    std::fwrite(v, sizeof(float), 4, f);
  }
  std::fclose(f);
  std::printf("{\"n\": %zu, \"width\": %u, \"height\": %u, \"is_dense\": %d}\n", map->points.size(), map->width, map->height, map->is_dense ? 1 : 0);
  return 0;
}

int main(int argc, char** argv) {
  if (argc < 5 || std::string(argv[1]) != "run") return 2;
  const bool matrix = argc > 5 && std::string(argv[5]) == "matrix";
  FILE* f = std::fopen(argv[2], "rb");
  if (!f) return 3;
  int32_t n_kf = 0;
  if (std::fread(&n_kf, sizeof(n_kf), 1, f) != 1) return 3;
  std::vector<std::shared_ptr<SnapshotArray>> a;
  std::vector<std::shared_ptr<SnapshotMatrix>> m;
  for (int k = 0; k < n_kf; k++) {
    int32_t n = 0;
    double pose[16];
    if (std::fread(&n, sizeof(n), 1, f) != 1 || std::fread(pose, sizeof(double), 16, f) != 16) return 3;
    std::vector<float> buf(4 * (size_t)n);
    if (n > 0 && std::fread(buf.data(), sizeof(float), buf.size(), f) != buf.size()) return 3;
    std::shared_ptr<Cloud> c(new Cloud());
    c->points.resize((size_t)n);
    for (int i = 0; i < n; i++) {
      c->points[i].x = buf[4 * i];
      c->points[i].y = buf[4 * i + 1];
      c->points[i].z = buf[4 * i + 2];
    }
    if (matrix) {
      std::shared_ptr<SnapshotMatrix> s(new SnapshotMatrix());
      for (int col = 0; col < 4; col++)
        for (int r = 0; r < 4; r++) s->pose.m(r, col) = pose[col * 4 + r];
      s->cloud = c;
      m.push_back(s);
    } else {
      std::shared_ptr<SnapshotArray> s(new SnapshotArray());
      for (int i = 0; i < 16; i++) s->pose[i] = pose[i];
      s->cloud = c;
      a.push_back(s);
    }
  }
  std::fclose(f);
  const double resolution = std::atof(argv[3]);
  return matrix ? run(m, resolution, argv[4]) : run(a, resolution, argv[4]);
}
