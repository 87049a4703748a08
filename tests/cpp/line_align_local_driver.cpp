// LineBasedScanmatcher::align_local without Eigen, PCL or ROS, two ways:
//   line_align_local_driver host items.bin out.bin max_range [repeat=N] [name=value ...]
//       the shared header (delta_graph_slam_amd/csrc/line_align.h) compiled for the host: la::align_local per item, no library call and
//       no device.  Names: the l_* members, l_max_distance, l_max_angle, angle_gate_float_chain, nn_tie_highest_index, refine_three_nearest.
//   line_align_local_driver run items.bin out.bin max_range [repeat=N] [name=value ...]
//       dgs::HipLineAligner::alignLocalBatch (include/dgs/line_align_hip.hpp) over libdgs_reg.so; names: the nodelet's delta_local_*.
//       single=1: the same items as one alignLocal call each (what is timed then; the output is the same).
// items.bin: int64 n, n + 1 int64 source offsets, n + 1 int64 target offsets, then 6 doubles (A, B) per source line and per target line.
// out.bin, per item, all doubles: transformation 16, fitness 4, score; then (host only) the edge phase's 16 + 4 + 1, the baseline's
// 4 + 1, winner_edge, winner_line, survivors_edge, survivors_line, Es, Et, H1, H2; then 6 per aligned line; then (host only) 16 per
// hypothesis of both phases: gate, target, rotation 4, translation 3, translation.norm(), fitness 4, score, 0.
// Prints {"ok", "items", "ms_per_call", "error"}; ms_per_call is the median over `repeat` calls.
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

#include <dgs/line_align_hip.hpp>

#include "../../delta_graph_slam_amd/csrc/line_align.h"

namespace la = dgs::la;

struct Params {   // stands in for ros::NodeHandle::param<T>(name, default)
  std::map<std::string, std::string> s;
  template <class T>
  T param(const std::string& k, const T& d) {
    auto it = s.find(k);
    if (it == s.end()) return d;
    if constexpr (std::is_same<T, std::string>::value) return it->second;
    else if constexpr (std::is_integral<T>::value) return (T)std::stol(it->second);
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

static void put_tf(const la::Tf t, std::vector<double>* o) {
  const double m[16] = {t.r00, t.r01, 0.0, t.tx, t.r10, t.r11, 0.0, t.ty, 0.0, 0.0, 1.0, t.tz, 0.0, 0.0, 0.0, 1.0};
  o->insert(o->end(), m, m + 16);
}
static double num(const std::string& v) { return v == "inf" ? INFINITY : std::stod(v); }

int main(int argc, char** argv) {
  if (argc < 5) return 2;
  const std::string mode = argv[1];
  Params pnh;
  for (int a = 5; a < argc; a++) {
    const std::string kv = argv[a];
    const size_t eq = kv.find('=');
    if (eq != std::string::npos) pnh.s[kv.substr(0, eq)] = kv.substr(eq + 1);
  }
  const double max_range = num(argv[4]);
  const int repeat = std::max(1, pnh.param<int>("repeat", 1));
  FILE* f = std::fopen(argv[2], "rb");
  if (!f) return 3;
  int64_t n = 0;
  if (std::fread(&n, 8, 1, f) != 1 || n < 0) return 3;
  std::vector<int64_t> so((size_t)n + 1), to((size_t)n + 1);
  if (std::fread(so.data(), 8, so.size(), f) != so.size() || std::fread(to.data(), 8, to.size(), f) != to.size()) return 3;
  std::vector<double> sl((size_t)so[(size_t)n] * 6), tl((size_t)to[(size_t)n] * 6);
  if (std::fread(sl.data(), 8, sl.size(), f) != sl.size() || std::fread(tl.data(), 8, tl.size(), f) != tl.size()) return 3;
  std::fclose(f);
  const auto line_at = [](const std::vector<double>& v, int64_t i) {
    la::Line l;
    l.a = la::v3(v[6 * i], v[6 * i + 1], v[6 * i + 2]);
    l.b = la::v3(v[6 * i + 3], v[6 * i + 4], v[6 * i + 5]);
    return l;
  };
  std::vector<double> out, times;
  bool ok = true;
  std::string err;
  if (mode == "host") {
    la::LocalParams P;
    P.w.avg_distance_weight = num(pnh.param<std::string>("l_avg_distance_weight", "0.6"));
    P.w.coverage_weight = num(pnh.param<std::string>("l_coverage_weight", "1.0"));
    P.w.transform_weight = num(pnh.param<std::string>("l_transform_weight", "0.2"));
    P.w.max_score_distance = pnh.param<double>("l_max_score_distance", 5.0);
    P.w.max_score_translation = pnh.param<double>("l_max_score_translation", 5.0);
    P.max_distance = pnh.param<double>("l_max_distance", 2.5);
    P.cos_max_angle = std::cos(pnh.param<double>("l_max_angle", M_PI / 9.0));
    P.max_range = max_range;
    P.float_chain = pnh.param<int>("angle_gate_float_chain", 1);
    P.tie_highest = pnh.param<int>("nn_tie_highest_index", 0);
    P.three_nearest = pnh.param<int>("refine_three_nearest", 0);
    for (int rep = 0; rep < repeat; rep++) {
      out.clear();
      const auto t0 = std::chrono::steady_clock::now();
      for (int64_t b = 0; b < n; b++) {
        std::vector<la::Line> src, trg, aligned;
        for (int64_t i = so[(size_t)b]; i < so[(size_t)b + 1]; i++) src.push_back(line_at(sl, i));
        for (int64_t j = to[(size_t)b]; j < to[(size_t)b + 1]; j++) trg.push_back(line_at(tl, j));
        la::LocalResult r;
        std::vector<la::LocalHyp> h1, h2;
        la::align_local(src, trg, P, &r, &aligned, &h1, &h2);
        put_tf(r.t, &out);
        out.insert(out.end(), r.fit, r.fit + 5);
        put_tf(r.t_edge, &out);
        out.insert(out.end(), r.fit_edge, r.fit_edge + 5);
        out.insert(out.end(), r.fit_base, r.fit_base + 5);
        for (const double v : {(double)r.winner_edge, (double)r.winner_line, (double)r.survivors_edge, (double)r.survivors_line,
                               (double)r.n_edges_source, (double)r.n_edges_target, (double)h1.size(), (double)h2.size()})
          out.push_back(v);
        for (const la::Line& l : aligned)
          for (const double v : {l.a.x, l.a.y, l.a.z, l.b.x, l.b.y, l.b.z}) out.push_back(v);
        for (const std::vector<la::LocalHyp>* hv : {&h1, &h2})
          for (const la::LocalHyp& h : *hv) {
            for (const double v : {(double)h.gate, (double)h.target, h.t.r00, h.t.r01, h.t.r10, h.t.r11, h.t.tx, h.t.ty, h.t.tz, h.tn}) out.push_back(v);
            out.insert(out.end(), h.fit, h.fit + 5);
            out.push_back(0.0);
          }
      }
      times.push_back(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    }
  } else {
    dgs::HipLineAligner<Line, Alignment> al(pnh);
    std::vector<std::vector<std::shared_ptr<Line>>> src((size_t)n), trg((size_t)n);
    std::vector<dgs::HipLineAligner<Line, Alignment>::LocalItem> items;
    const auto fill = [](const std::vector<double>& v, int64_t first, int64_t last, std::vector<std::shared_ptr<Line>>* o) {
      for (int64_t i = first; i < last; i++) {
        auto l = std::make_shared<Line>();
        for (int a = 0; a < 3; a++) { l->pointA[a] = v[6 * i + a]; l->pointB[a] = v[6 * i + 3 + a]; }
        l->mean_error = 0.1 * (double)i;
        o->push_back(l);
      }
    };
    for (int64_t b = 0; b < n; b++) {
      fill(sl, so[(size_t)b], so[(size_t)b + 1], &src[(size_t)b]);
      fill(tl, to[(size_t)b], to[(size_t)b + 1], &trg[(size_t)b]);
      items.push_back({&src[(size_t)b], &trg[(size_t)b]});
    }
    std::vector<Alignment> res;
    const bool single = pnh.param<int>("single", 0) != 0;
    for (int rep = 0; rep < repeat && ok; rep++) {
      const auto t0 = std::chrono::steady_clock::now();
      if (single) {
        Alignment one;
        for (size_t b = 0; b < items.size() && ok; b++) ok = al.alignLocal(src[b], trg[b], max_range, &one);
      } else {
        ok = al.alignLocalBatch(items, max_range, &res);
      }
      times.push_back(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    }
    if (ok && single) ok = al.alignLocalBatch(items, max_range, &res);   // the output
    if (!ok) err = al.last_error() ? al.last_error() : "";
    for (size_t b = 0; ok && b < res.size(); b++) {
      out.insert(out.end(), res[b].transformation.m, res[b].transformation.m + 16);
      for (const double v : {res[b].fitness_score.real_avg_distance, res[b].fitness_score.avg_distance, res[b].fitness_score.coverage,
                             res[b].fitness_score.coverage_percentage, al.lastLocal()[b].score})
        out.push_back(v);
      for (const auto& l : res[b].aligned_lines) {
        ok = ok && l->mean_error == src[b][&l - &res[b].aligned_lines[0]]->mean_error;   // the statistics are carried through
        out.insert(out.end(), l->pointA, l->pointA + 3);
        out.insert(out.end(), l->pointB, l->pointB + 3);
      }
    }
  }
  if (ok) {
    FILE* o = std::fopen(argv[3], "wb");
    if (!o) return 4;
    std::fwrite(out.data(), sizeof(double), out.size(), o);
    std::fclose(o);
  }
  std::sort(times.begin(), times.end());
  std::printf("{\"ok\": %s, \"items\": %lld, \"ms_per_call\": %.6f, \"error\": \"%s\"}\n", ok ? "true" : "false", (long long)n,
              times.empty() ? 0.0 : times[times.size() / 2], err.c_str());
  return 0;
}
