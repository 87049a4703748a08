// dgs::HipBuildingClouds (include/dgs/building_cloud_hip.hpp) against the PCL-shape stubs.
//   building_cloud_driver interpolate|build|getcloud in.bin out.bin
//   building_cloud_driver matrix in.bin out.bin
// in.bin: int32 lines, 6 doubles per line (pointA, pointB), then 16 floats (trans3D, row-major; read by getcloud).  Writes x, y, z, 1 per
// point and prints one JSON line; a null result prints {"null": true, "error": ...}.  interpolate samples the first line alone, from
// float end points as upstream's free function takes them.
// matrix: in.bin is 9 + 9 doubles (the building's pose and the node's estimate, row-major 3 x 3); writes building_transform16's 16
// floats.  No device is touched.
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <string>
#include <vector>

#include <Eigen/Core>
#include <dgs/building_cloud_hip.hpp>
#include <pcl/point_types.h>

using Cloud = pcl::PointCloud<pcl::PointXYZ>;
using Vector3d = Eigen::Matrix<double, 3, 1>;
using Vector3f = Eigen::Matrix<float, 3, 1>;

struct LineFeature {   // stands in for hdl_graph_slam::LineFeature
  Vector3d pointA, pointB;
};

static int write_cloud(const Cloud::Ptr& c, const dgs::HipBuildingClouds<pcl::PointXYZ>& bc, const char* path) {
  if (!c) {
    const char* e = bc.last_error();
    std::printf("{\"null\": true, \"error\": \"%s\"}\n", e ? e : "");
    return 0;
  }
  FILE* f = std::fopen(path, "wb");
  if (!f) return 4;
  for (const auto& p : c->points) {
    const float v[4] = {p.x, p.y, p.z, 1.f};
    std::fwrite(v, sizeof(float), 4, f);
  }
  std::fclose(f);
  std::printf("{\"n\": %zu, \"width\": %u, \"height\": %u}\n", c->points.size(), c->width, c->height);
  return 0;
}

int main(int argc, char** argv) {
  if (argc < 4) return 2;
  const std::string mode = argv[1];
  FILE* f = std::fopen(argv[2], "rb");
  if (!f) return 3;
  if (mode == "matrix") {
    double v[18];
    if (std::fread(v, sizeof(double), 18, f) != 18) return 3;
    std::fclose(f);
    Eigen::Matrix<double, 3, 3> pose, est;
    for (int r = 0; r < 3; r++)
      for (int c = 0; c < 3; c++) {
        pose(r, c) = v[r * 3 + c];
        est(r, c) = v[9 + r * 3 + c];
      }
    float m[16];
    dgs::building_transform16(pose, est, m);
    FILE* o = std::fopen(argv[3], "wb");
    if (!o) return 4;
    std::fwrite(m, sizeof(float), 16, o);
    std::fclose(o);
    std::printf("{\"ok\": true}\n");
    return 0;
  }
  int32_t n = 0;
  if (std::fread(&n, sizeof(n), 1, f) != 1 || n < 0) return 3;
  std::vector<std::shared_ptr<LineFeature>> lines;
  for (int i = 0; i < n; i++) {
    double v[6];
    if (std::fread(v, sizeof(double), 6, f) != 6) return 3;
    std::shared_ptr<LineFeature> l(new LineFeature());
    for (int c = 0; c < 3; c++) {
      l->pointA(c, 0) = v[c];
      l->pointB(c, 0) = v[3 + c];
    }
    lines.push_back(l);
  }
  float m[16];
  if (std::fread(m, sizeof(float), 16, f) != 16) return 3;
  std::fclose(f);
  dgs::HipBuildingClouds<pcl::PointXYZ> bc;
  if (mode == "interpolate") {
    if (lines.empty()) return 3;
    Vector3f a, b;
    for (int c = 0; c < 3; c++) {
      a(c, 0) = (float)lines[0]->pointA(c, 0);
      b(c, 0) = (float)lines[0]->pointB(c, 0);
    }
    return write_cloud(bc.interpolate(a, b), bc, argv[3]);
  }
  if (mode == "build") return write_cloud(bc.buildPointCloud(lines), bc, argv[3]);
  if (mode == "getcloud") {
    Eigen::Matrix4f t;
    for (int r = 0; r < 4; r++)
      for (int c = 0; c < 4; c++) t(r, c) = m[r * 4 + c];
    return write_cloud(bc.getCloud(lines, t), bc, argv[3]);
  }
  return 2;
}
