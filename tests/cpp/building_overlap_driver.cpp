// are_buildings_overlapped over all pairs and align_overlapped_buildings without Eigen, PCL or ROS, two ways:
//   building_overlap_driver host pairs|align in.bin out.bin [repeat=N] [angle_gate_float_chain=0|1]
//       the shared header (delta_graph_slam_amd/csrc/building_overlap.h) compiled for the host: bo::overlapped_pairs, or bo::align_overlapped
//       per item; no library call and no device.
//   building_overlap_driver device pairs|align in.bin out.bin [repeat=N]
//       dgs::HipBuildingOverlap::overlappedPairs (include/dgs/building_overlap_hip.hpp) or dgs::HipLineAligner::alignOverlappedBatch
//       (include/dgs/line_align_hip.hpp) over libdgs_reg.so, the hypothesis records through the C ABI's test hook.
// pairs, in.bin: int64 B, B + 1 int64 line offsets, 6 doubles (A, B) per line, 3 doubles per centre.  out.bin: int32 i, j per pair.
// align, in.bin: int64 n, n + 1 int64 source offsets, n + 1 int64 target offsets, 6 doubles per source line, 6 per target line, 3 per
// source centre, 3 per target centre.  out.bin, per item, all doubles: transformation 16, translation_norm, winner, n_hypotheses_edge,
// n_hypotheses_line, n_angle_passed, n_not_overlapped, Es, Et, is_identity; then 6 per aligned line; then 9 per hypothesis: gate,
// rotation 4, translation 3, translation.norm().
// Prints {"ok", "n", "count", "ms_per_call", "error"}: buildings and pairs, or items and hypotheses; the median over `repeat` calls.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include <dgs/building_overlap_hip.hpp>
#include <dgs/line_align_hip.hpp>

#include "../../delta_graph_slam_amd/csrc/building_overlap.h"

namespace la = dgs::la;
namespace bo = dgs::bo;

struct Params {   // stands in for ros::NodeHandle::param<T>(name, default)
  std::map<std::string, std::string> s;
  template <class T>
  T param(const std::string& k, const T& d) {
    auto it = s.find(k);
    if (it == s.end()) return d;
    if constexpr (std::is_integral<T>::value) return (T)std::stol(it->second);
    else return (T)std::stod(it->second);
  }
};
struct Line {   // upstream's LineFeature without Eigen
  double pointA[3], pointB[3];
  double mean_error = 0, std_sigma = 0, max_error = 0, min_error = 0;
};
struct Mat4 {
  double m[16];
  double& operator()(int r, int c) { return m[4 * r + c]; }
};
struct Fitness {
  double real_avg_distance, avg_distance, coverage, coverage_percentage;
};
struct Alignment {   // upstream's BestFitAlignment
  std::vector<std::shared_ptr<Line>> not_aligned_lines, aligned_lines;
  Mat4 transformation;
  Fitness fitness_score;
  bool isEdgeAligned = false;
};

static bool read_all(FILE* f, void* p, size_t bytes) { return bytes == 0 || std::fread(p, 1, bytes, f) == bytes; }
static la::Line line_at(const std::vector<double>& v, int64_t i) {
  la::Line l;
  l.a = la::v3(v[6 * i], v[6 * i + 1], v[6 * i + 2]);
  l.b = la::v3(v[6 * i + 3], v[6 * i + 4], v[6 * i + 5]);
  return l;
}
static void fill(const std::vector<double>& v, int64_t first, int64_t last, std::vector<std::shared_ptr<Line>>* o) {
  for (int64_t i = first; i < last; i++) {
    auto l = std::make_shared<Line>();
    for (int a = 0; a < 3; a++) { l->pointA[a] = v[6 * i + a]; l->pointB[a] = v[6 * i + 3 + a]; }
    l->mean_error = 0.1 * (double)i;
    o->push_back(l);
  }
}

int main(int argc, char** argv) {
  if (argc < 5) return 2;
  const std::string mode = argv[1], what = argv[2];
  Params pnh;
  for (int a = 5; a < argc; a++) {
    const std::string kv = argv[a];
    const size_t eq = kv.find('=');
    if (eq != std::string::npos) pnh.s[kv.substr(0, eq)] = kv.substr(eq + 1);
  }
  const int repeat = std::max(1, pnh.param<int>("repeat", 1));
  const int float_chain = pnh.param<int>("angle_gate_float_chain", 1);
  FILE* f = std::fopen(argv[3], "rb");
  if (!f) return 3;
  int64_t n = 0;
  if (std::fread(&n, 8, 1, f) != 1 || n < 0) return 3;
  std::vector<double> times;
  std::vector<double> out;
  std::vector<int32_t> pairs_out;
  bool ok = true;
  std::string err;
  long long count = 0;
  if (what == "pairs") {
    std::vector<int64_t> off((size_t)n + 1);
    if (!read_all(f, off.data(), off.size() * 8)) return 3;
    std::vector<double> ll((size_t)off[(size_t)n] * 6), ce((size_t)n * 3);
    if (!read_all(f, ll.data(), ll.size() * 8) || !read_all(f, ce.data(), ce.size() * 8)) return 3;
    std::fclose(f);
    if (mode == "host") {
      std::vector<std::vector<la::Line>> buildings((size_t)n);
      std::vector<la::V3> centers;
      for (int64_t b = 0; b < n; b++) {
        for (int64_t i = off[(size_t)b]; i < off[(size_t)b + 1]; i++) buildings[(size_t)b].push_back(line_at(ll, i));
        centers.push_back(la::v3(ce[3 * b], ce[3 * b + 1], ce[3 * b + 2]));
      }
      for (int rep = 0; rep < repeat; rep++) {
        const auto t0 = std::chrono::steady_clock::now();
        bo::overlapped_pairs(buildings, centers, &pairs_out);
        times.push_back(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
      }
    } else {
      dgs::HipBuildingOverlap<Line> ov;
      std::vector<std::vector<std::shared_ptr<Line>>> buildings((size_t)n);
      std::vector<std::array<double, 3>> centers;
      for (int64_t b = 0; b < n; b++) {
        fill(ll, off[(size_t)b], off[(size_t)b + 1], &buildings[(size_t)b]);
        centers.push_back({ce[3 * b], ce[3 * b + 1], ce[3 * b + 2]});
      }
      std::vector<std::pair<int, int>> pr;
      for (int rep = 0; rep < repeat && ok; rep++) {
        const auto t0 = std::chrono::steady_clock::now();
        ok = ov.overlappedPairs(buildings, centers, &pr);
        times.push_back(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
      }
      if (!ok) err = ov.last_error() ? ov.last_error() : "";
      for (const auto& p : pr) { pairs_out.push_back(p.first); pairs_out.push_back(p.second); }
    }
    count = (long long)pairs_out.size() / 2;
  } else {
    std::vector<int64_t> so((size_t)n + 1), to((size_t)n + 1);
    if (!read_all(f, so.data(), so.size() * 8) || !read_all(f, to.data(), to.size() * 8)) return 3;
    std::vector<double> sl((size_t)so[(size_t)n] * 6), tl((size_t)to[(size_t)n] * 6), cs((size_t)n * 3), ct((size_t)n * 3);
    if (!read_all(f, sl.data(), sl.size() * 8) || !read_all(f, tl.data(), tl.size() * 8) || !read_all(f, cs.data(), cs.size() * 8) ||
        !read_all(f, ct.data(), ct.size() * 8))
      return 3;
    std::fclose(f);
    const auto put_hyp = [&out](double gate, const double* r4, const double* t3, double tn) {
      out.push_back(gate);
      out.insert(out.end(), r4, r4 + 4);
      out.insert(out.end(), t3, t3 + 3);
      out.push_back(tn);
    };
    if (mode == "host") {
      for (int rep = 0; rep < repeat; rep++) {
        out.clear();
        count = 0;
        const auto t0 = std::chrono::steady_clock::now();
        for (int64_t b = 0; b < n; b++) {
          std::vector<la::Line> src, trg, aligned;
          for (int64_t i = so[(size_t)b]; i < so[(size_t)b + 1]; i++) src.push_back(line_at(sl, i));
          for (int64_t j = to[(size_t)b]; j < to[(size_t)b + 1]; j++) trg.push_back(line_at(tl, j));
          bo::OverlapResult r;
          std::vector<bo::OverlapHyp> hy;
          bo::align_overlapped(src, trg, la::v3(cs[3 * b], cs[3 * b + 1], cs[3 * b + 2]), la::v3(ct[3 * b], ct[3 * b + 1], ct[3 * b + 2]), float_chain, &r,
                               &aligned, &hy);
          double T[16];
          la::matrix(r.t, T);
          out.insert(out.end(), T, T + 16);
          for (const double v : {r.tn, (double)r.winner, (double)r.n_edge, (double)r.n_line, (double)r.n_angle_passed, (double)r.n_not_overlapped,
                                 (double)r.n_edges_source, (double)r.n_edges_target, (double)r.is_identity})
            out.push_back(v);
          for (const la::Line& l : aligned)
            for (const double v : {l.a.x, l.a.y, l.a.z, l.b.x, l.b.y, l.b.z}) out.push_back(v);
          for (const bo::OverlapHyp& h : hy) {
            const double r4[4] = {h.t.r00, h.t.r01, h.t.r10, h.t.r11}, t3[3] = {h.t.tx, h.t.ty, h.t.tz};
            put_hyp((double)h.gate, r4, t3, h.tn);
          }
          count += (long long)hy.size();
        }
        times.push_back(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
      }
    } else {
      dgs::HipLineAligner<Line, Alignment> al(pnh);
      al.params().angle_gate_float_chain = float_chain;
      std::vector<std::vector<std::shared_ptr<Line>>> src((size_t)n), trg((size_t)n);
      std::vector<dgs::HipLineAligner<Line, Alignment>::OverlapItem> items;
      for (int64_t b = 0; b < n; b++) {
        fill(sl, so[(size_t)b], so[(size_t)b + 1], &src[(size_t)b]);
        fill(tl, to[(size_t)b], to[(size_t)b + 1], &trg[(size_t)b]);
        items.push_back({&src[(size_t)b], &trg[(size_t)b], {cs[3 * b], cs[3 * b + 1], cs[3 * b + 2]}, {ct[3 * b], ct[3 * b + 1], ct[3 * b + 2]}});
      }
      std::vector<Alignment> res;
      for (int rep = 0; rep < repeat && ok; rep++) {
        const auto t0 = std::chrono::steady_clock::now();
        ok = al.alignOverlappedBatch(items, &res);
        times.push_back(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
      }
      for (size_t b = 0; ok && b < res.size(); b++) {
        const dgs_line_overlap_alignment& r = al.lastOverlapped()[b];
        out.insert(out.end(), res[b].transformation.m, res[b].transformation.m + 16);
        for (const double v : {r.translation_norm, (double)r.winner, (double)r.n_hypotheses_edge, (double)r.n_hypotheses_line, (double)r.n_angle_passed,
                               (double)r.n_not_overlapped, (double)r.n_edges_source, (double)r.n_edges_target, (double)r.is_identity})
          out.push_back(v);
        for (const auto& l : res[b].aligned_lines) {
          ok = ok && l->mean_error == src[b][&l - &res[b].aligned_lines[0]]->mean_error;   // the statistics are carried through
          out.insert(out.end(), l->pointA, l->pointA + 3);
          out.insert(out.end(), l->pointB, l->pointB + 3);
        }
        const int64_t H = r.n_hypotheses_edge + r.n_hypotheses_line;
        std::vector<dgs_line_align_overlapped_hypothesis> hy((size_t)std::max<int64_t>(H, 1));
        ok = ok && dgs_line_align_overlapped_get_hypotheses(al.handle(), (int64_t)b, 0, H, hy.data()) == DGS_OK;
        for (int64_t k = 0; ok && k < H; k++) put_hyp((double)hy[(size_t)k].gate, hy[(size_t)k].rotation, hy[(size_t)k].translation, hy[(size_t)k].translation_norm);
        count += (long long)H;
      }
      if (!ok) err = al.last_error() ? al.last_error() : "";
    }
  }
  if (ok) {
    FILE* o = std::fopen(argv[4], "wb");
    if (!o) return 4;
    if (what == "pairs" && !pairs_out.empty()) std::fwrite(pairs_out.data(), sizeof(int32_t), pairs_out.size(), o);
    if (what != "pairs" && !out.empty()) std::fwrite(out.data(), sizeof(double), out.size(), o);
    std::fclose(o);
  }
  std::sort(times.begin(), times.end());
  std::printf("{\"ok\": %s, \"n\": %lld, \"count\": %lld, \"ms_per_call\": %.6f, \"error\": \"%s\"}\n", ok ? "true" : "false", (long long)n, count,
              times.empty() ? 0.0 : times[times.size() / 2], err.c_str());
  return 0;
}
