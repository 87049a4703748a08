// InformationMatrixCalculator without Eigen, PCL or ROS: dgs::HipInformationMatrixCalculator (include/dgs/information_matrix_hip.hpp) over
// libdgs_reg.so, against tests/stub_pcl.
//   information_matrix_driver in.bin out.bin [key=value ...]          key: any parameter of information_matrix_calculator.cpp:28-48
// in.bin: int64 C; per cloud int64 n, then n x 4 floats; int64 E; per edge int64 cloud1, int64 cloud2, 16 doubles (relpose, row-major);
// then 4 doubles: fitness_score of the global building form; avg_distance, coverage_percentage, isEdgeAligned of the local one.
// out.bin, all doubles, 9 per matrix (row-major): the global building form, the local one (host arithmetic: written with or without a
// device), then -- when the device calls succeed -- calc_information_matrices over all edges, calc_information_matrix edge by edge,
// and all edges once more after forget() of every cloud.
// Prints {"ok", "edges", "error"}; ok = false without a GPU (the adapter's soft failure), exit code 0 either way.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include <Eigen/Core>
#include <pcl/point_cloud.h>
#include <pcl/point_types.h>

#include <dgs/information_matrix_hip.hpp>

struct Params {   // stands in for ros::NodeHandle::param<T>(name, default)
  std::map<std::string, std::string> s;
  template <class T>
  T param(const std::string& k, const T& d) {
    auto it = s.find(k);
    if (it == s.end()) return d;
    if (std::is_same<T, bool>::value) return (T)(it->second == "1" || it->second == "true");
    return (T)std::stod(it->second);
  }
};
using Pose = Eigen::Matrix<double, 4, 4>;
using Mat3 = Eigen::Matrix<double, 3, 3>;
using Calc = dgs::HipInformationMatrixCalculator<pcl::PointXYZ, Pose, Mat3>;
struct Fitness {
  double real_avg_distance = 0, avg_distance = 0, coverage = 0, coverage_percentage = 0;
};
struct Alignment {   // the fields of upstream's BestFitAlignment that are read
  Fitness fitness_score;
  bool isEdgeAligned = false;
};

static bool read_all(FILE* f, void* p, size_t bytes) { return bytes == 0 || std::fread(p, 1, bytes, f) == bytes; }
static void put(std::vector<double>* out, const Mat3& m) {
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 3; c++) out->push_back(m(r, c));
}

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  Params pnh;
  for (int a = 3; a < argc; a++) {
    const std::string kv = argv[a];
    const size_t eq = kv.find('=');
    if (eq != std::string::npos) pnh.s[kv.substr(0, eq)] = kv.substr(eq + 1);
  }
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 3;
  int64_t C = 0, E = 0;
  if (!read_all(f, &C, 8) || C < 0) return 3;
  std::vector<pcl::PointCloud<pcl::PointXYZ>::Ptr> clouds;
  for (int64_t i = 0; i < C; i++) {
    int64_t n = 0;
    if (!read_all(f, &n, 8) || n < 0) return 3;
    auto c = std::make_shared<pcl::PointCloud<pcl::PointXYZ>>();
    c->points.resize((size_t)n);
    if (!read_all(f, c->points.data(), (size_t)n * 16)) return 3;
    clouds.push_back(c);
  }
  if (!read_all(f, &E, 8) || E < 0) return 3;
  std::vector<Calc::Edge> edges;
  for (int64_t e = 0; e < E; e++) {
    int64_t ij[2];
    double T[16];
    if (!read_all(f, ij, 16) || !read_all(f, T, 128) || ij[0] < 0 || ij[0] >= C || ij[1] < 0 || ij[1] >= C) return 3;
    Calc::Edge ed;
    ed.cloud1 = clouds[(size_t)ij[0]];
    ed.cloud2 = clouds[(size_t)ij[1]];
    for (int r = 0; r < 4; r++)
      for (int c = 0; c < 4; c++) ed.relpose(r, c) = T[4 * r + c];
    edges.push_back(ed);
  }
  double tail[4];
  if (!read_all(f, tail, 32)) return 3;
  std::fclose(f);

  Calc calc(pnh);
  std::vector<double> out;
  put(&out, calc.calc_information_matrix_buildings_global(tail[0]));
  Alignment al;
  al.fitness_score.avg_distance = tail[1];
  al.fitness_score.coverage_percentage = tail[2];
  al.isEdgeAligned = tail[3] != 0.0;
  put(&out, calc.calc_information_matrix_buildings_local(al));

  std::vector<Mat3> infs;
  bool ok = calc.calc_information_matrices(edges, &infs);
  std::string err;
  if (ok) {
    for (const Mat3& m : infs) put(&out, m);
    for (size_t e = 0; ok && e < edges.size(); e++) {
      Mat3 m;
      ok = calc.calc_information_matrix(edges[e].cloud1, edges[e].cloud2, edges[e].relpose, &m);
      if (ok) put(&out, m);
    }
    for (const auto& c : clouds) calc.forget(c.get());
    ok = ok && calc.calc_information_matrices(edges, &infs);
    if (ok)
      for (const Mat3& m : infs) put(&out, m);
  }
  if (!ok) err = calc.last_error() ? calc.last_error() : "";
  for (char& ch : err)
    if (ch == '"' || ch == '\\' || ch == '\n') ch = ' ';
  FILE* o = std::fopen(argv[2], "wb");
  if (!o) return 4;
  std::fwrite(out.data(), sizeof(double), out.size(), o);
  std::fclose(o);
  std::printf("{\"ok\": %s, \"edges\": %lld, \"error\": \"%s\"}\n", ok ? "true" : "false", (long long)E, err.c_str());
  return 0;
}
