// dgs::HipLineAligner::edgeExtractionBatch / edgeExtraction (include/dgs/line_align_hip.hpp) without Eigen, PCL or ROS:
//   line_edges_driver segments.bin out.bin
// segments.bin: int64 n, n + 1 int64 line offsets, n int64 only_angular_edges, n doubles max_dist_angular_edge, then 6 doubles (A, B) per line.
// out.bin, all doubles: the n + 1 edge offsets, then 9 per edge (edgePoint, pointA, pointB) of all segments back to back; then the same 9
// per edge of segment 0 from the single-segment call.  Prints {"ok", "segments", "edges", "error"}.
#include <cstdint>
#include <cstdio>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include <dgs/line_align_hip.hpp>

struct Params {   // stands in for ros::NodeHandle::param<T>(name, default)
  template <class T>
  T param(const std::string&, const T& d) { return d; }
};
struct Line {   // upstream's LineFeature without Eigen
  double pointA[3], pointB[3];
  double mean_error = 0, std_sigma = 0, max_error = 0, min_error = 0;
};
struct Edge {   // upstream's EdgeFeature without Eigen
  double edgePoint[3], pointA[3], pointB[3];
};
struct Mat4 {
  double m[16];
  double& operator()(int r, int c) { return m[4 * r + c]; }
};
struct Fitness {
  double real_avg_distance, avg_distance, coverage, coverage_percentage;
};
struct Alignment {
  std::vector<std::shared_ptr<Line>> not_aligned_lines, aligned_lines;
  Mat4 transformation;
  Fitness fitness_score;
  bool isEdgeAligned = false;
};
using Aligner = dgs::HipLineAligner<Line, Alignment>;

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  int64_t n = 0;
  if (std::fread(&n, 8, 1, f) != 1) return 2;
  std::vector<int64_t> off((size_t)n + 1), only((size_t)n);
  std::vector<double> dist((size_t)n);
  if (std::fread(off.data(), 8, off.size(), f) != off.size()) return 2;
  if (n && (std::fread(only.data(), 8, only.size(), f) != only.size() || std::fread(dist.data(), 8, dist.size(), f) != dist.size())) return 2;
  std::vector<std::vector<std::shared_ptr<Line>>> lines((size_t)n);
  for (int64_t b = 0; b < n; b++)
    for (int64_t k = off[b]; k < off[b + 1]; k++) {
      auto l = std::make_shared<Line>();
      if (std::fread(l->pointA, 8, 3, f) != 3 || std::fread(l->pointB, 8, 3, f) != 3) return 2;
      lines[(size_t)b].push_back(l);
    }
  std::fclose(f);
  Params nh;
  Aligner al(nh);
  std::vector<Aligner::EdgeItem> items;
  for (int64_t b = 0; b < n; b++) items.push_back(Aligner::EdgeItem{&lines[(size_t)b], only[(size_t)b] != 0, dist[(size_t)b]});
  std::vector<std::vector<std::shared_ptr<Edge>>> edges;
  std::vector<std::shared_ptr<Edge>> first;
  bool ok = al.edgeExtractionBatch<Edge>(items, &edges);
  if (ok && n) ok = al.edgeExtraction<Edge>(lines[0], only[0] != 0, dist[0], &first);
  size_t total = 0;
  if (ok) {
    std::vector<double> out(1, 0.0);
    for (const auto& e : edges) out.push_back(out.back() + (double)e.size());
    auto put = [&out](const Edge& e) {
      out.insert(out.end(), e.edgePoint, e.edgePoint + 3);
      out.insert(out.end(), e.pointA, e.pointA + 3);
      out.insert(out.end(), e.pointB, e.pointB + 3);
    };
    for (const auto& seg : edges)
      for (const auto& e : seg) put(*e);
    for (const auto& e : first) put(*e);
    total = (size_t)out[(size_t)n];
    FILE* o = std::fopen(argv[2], "wb");
    if (!o || std::fwrite(out.data(), 8, out.size(), o) != out.size()) return 2;
    std::fclose(o);
  }
  std::string err = al.last_error();
  for (char& c : err)
    if (c == '"' || c == '\\') c = '\'';
  std::printf("{\"ok\": %s, \"segments\": %lld, \"edges\": %zu, \"error\": \"%s\"}\n", ok ? "true" : "false", (long long)n, total, err.c_str());
  return 0;
}
