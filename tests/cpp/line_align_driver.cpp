// dgs::HipLineAligner (include/dgs/line_align_hip.hpp) without Eigen, PCL or ROS.
//   line_align_driver params [name=value ...]                      -> one JSON line with the parsed parameters (no device touched)
//   line_align_driver run src.bin trg.bin out.bin constrain max_range [name=value ...]
//       src.bin / trg.bin: 6 doubles per line (A, B); out.bin: 16 doubles of the transformation, 4 of the fitness score, then 6 per
//       aligned line; prints {"ok", "winner", "refine_steps", "status", "hypotheses", "survivors", "error"}
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include <dgs/line_align_hip.hpp>

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
};

static std::vector<std::shared_ptr<Line>> read_lines(const char* path) {
  std::vector<std::shared_ptr<Line>> out;
  FILE* f = std::fopen(path, "rb");
  if (!f) return out;
  double v[6];
  while (std::fread(v, sizeof(double), 6, f) == 6) {
    auto l = std::make_shared<Line>();
    for (int a = 0; a < 3; a++) { l->pointA[a] = v[a]; l->pointB[a] = v[3 + a]; }
    out.push_back(l);
  }
  std::fclose(f);
  return out;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  const std::string mode = argv[1];
  const int first_kv = mode == "run" ? 7 : 2;
  if (argc < first_kv) return 2;
  Params pnh;
  for (int a = first_kv; a < argc; a++) {
    const std::string kv = argv[a];
    const size_t eq = kv.find('=');
    if (eq != std::string::npos) pnh.s[kv.substr(0, eq)] = kv.substr(eq + 1);
  }
  dgs::HipLineAligner<Line, Alignment> al(pnh);
  const dgs_line_align_params& p = al.params();
  if (mode == "params") {
    std::printf("{\"g_avg_distance_weight\": %.17g, \"g_coverage_weight\": %.17g, \"g_transform_weight\": %.17g, \"g_max_score_distance\": %.17g, "
                "\"g_max_score_translation\": %.17g, \"max_distance\": %.17g, \"max_angle\": %.17g}\n",
                p.g_avg_distance_weight, p.g_coverage_weight, p.g_transform_weight, p.g_max_score_distance, p.g_max_score_translation, p.max_distance,
                p.max_angle);
    return 0;
  }
  const auto src = read_lines(argv[2]), trg = read_lines(argv[3]);
  const bool constrain = std::atoi(argv[5]) != 0;
  const std::string mr = argv[6];
  const double max_range = mr == "inf" ? std::numeric_limits<double>::infinity() : std::stod(mr);
  Alignment res;
  const bool ok = al.alignGlobal(src, trg, constrain, max_range, &res);
  const char* err = al.last_error();
  if (ok) {
    FILE* o = std::fopen(argv[4], "wb");
    if (!o) return 4;
    std::fwrite(res.transformation.m, sizeof(double), 16, o);
    std::fwrite(&res.fitness_score, sizeof(double), 4, o);
    for (const auto& l : res.aligned_lines) {
      std::fwrite(l->pointA, sizeof(double), 3, o);
      std::fwrite(l->pointB, sizeof(double), 3, o);
    }
    std::fclose(o);
  }
  std::printf("{\"ok\": %s, \"winner\": %lld, \"refine_steps\": %d, \"status\": %d, \"hypotheses\": %lld, \"survivors\": %lld, \"error\": \"%s\"}\n",
              ok ? "true" : "false", (long long)al.last().winner, al.last().refine_steps, al.last().status, (long long)al.last().n_hypotheses,
              (long long)al.last().n_survivors, err ? err : "");
  return 0;
}
