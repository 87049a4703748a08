// dgs::HipRegistration::alignPairs (include/dgs/hip_registration.hpp) against the PCL-shape stubs (tests/stub_pcl): n registrations that each
// name their own target, in one device call, the way a patched LoopDetector::detect would issue a tick's candidates.
//   align_pairs_driver <method> in.bin out.bin [max_correspondence_distance]
// in.bin: int64 C; per cloud int64 n, then n x 4 floats; int64 P; per pair int64 target, int64 source, 16 floats (guess, column-major).
// out.bin: P x dgs_result, as the C ABI lays it out.  The call is made twice (the second one on the clouds the first left resident); the
// second answer is written, and "repeat_equal" says whether the two agree byte for byte.
// Prints {"ok", "pairs", "repeat_equal", "own_untouched", "error"}; ok = false without a GPU (the adapter's soft failure), exit code 0 either way.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <string>
#include <type_traits>
#include <vector>

#include <dgs/registrations_hip.hpp>

using PointT = pcl::PointXYZ;
using Reg = dgs::HipRegistration<PointT, PointT>;

struct Params {   // stands in for ros::NodeHandle::param<T>(name, default)
  std::map<std::string, double> d;
  template <class T>
  T param(const std::string& k, const T& def) const {
    if constexpr (std::is_arithmetic<T>::value) {
      auto it = d.find(k);
      return it == d.end() ? def : (T)it->second;
    } else {
      return def;
    }
  }
};

static bool read_all(FILE* f, void* p, size_t bytes) { return bytes == 0 || std::fread(p, 1, bytes, f) == bytes; }

int main(int argc, char** argv) {
  if (argc < 4) return 2;
  Params pnh;
  pnh.d["reg_max_correspondence_distance"] = argc > 4 ? std::atof(argv[4]) : 2.0;
  pcl::Registration<PointT, PointT>::Ptr registration = dgs::select_hip_registration<PointT>(argv[1], pnh);
  Reg* hip = dynamic_cast<Reg*>(registration.get());
  if (!hip) { std::printf("{\"error\": \"unknown method\"}\n"); return 3; }

  FILE* f = std::fopen(argv[2], "rb");
  if (!f) return 3;
  int64_t C = 0, P = 0;
  if (!read_all(f, &C, 8) || C < 0) return 3;
  std::vector<pcl::PointCloud<PointT>::Ptr> clouds;
  for (int64_t i = 0; i < C; i++) {
    int64_t n = 0;
    if (!read_all(f, &n, 8) || n < 0) return 3;
    pcl::PointCloud<PointT>::Ptr c(new pcl::PointCloud<PointT>());
    c->points.resize((size_t)n);
    if (!read_all(f, c->points.data(), (size_t)n * 16)) return 3;
    c->width = (std::uint32_t)n;
    clouds.push_back(c);
  }
  if (!read_all(f, &P, 8) || P < 0) return 3;
  std::vector<Reg::PointCloudTargetConstPtr> targets;
  std::vector<Reg::PointCloudSourceConstPtr> sources;
  std::vector<Reg::Matrix4> guesses;
  for (int64_t p = 0; p < P; p++) {
    int64_t ts[2];
    float g[16];
    if (!read_all(f, ts, 16) || !read_all(f, g, 64) || ts[0] < 0 || ts[0] >= C || ts[1] < 0 || ts[1] >= C) return 3;
    targets.push_back(clouds[(size_t)ts[0]]);
    sources.push_back(clouds[(size_t)ts[1]]);
    Reg::Matrix4 G;
    std::memcpy(G.data(), g, sizeof(g));
    guesses.push_back(G);
  }
  std::fclose(f);

  const Reg::Matrix4 own_before = hip->getFinalTransformation();
  std::vector<dgs_result> first, second;
  bool ok = hip->alignPairs(targets, sources, guesses, true, DBL_MAX, &first);
  ok = ok && hip->alignPairs(targets, sources, guesses, true, DBL_MAX, &second);
  std::string err = ok ? "" : hip->lastError();
  for (char& ch : err)
    if (ch == '"' || ch == '\\' || ch == '\n') ch = ' ';
  const bool repeat_equal = ok && first.size() == second.size() && (first.empty() || std::memcmp(first.data(), second.data(), first.size() * sizeof(dgs_result)) == 0);
  const bool own_untouched = !hip->hasConverged() && std::memcmp(own_before.data(), hip->getFinalTransformation().data(), sizeof(float) * 16) == 0;
  FILE* o = std::fopen(argv[3], "wb");
  if (!o) return 4;
  if (ok) std::fwrite(second.data(), sizeof(dgs_result), second.size(), o);
  std::fclose(o);
  std::printf("{\"ok\": %s, \"pairs\": %lld, \"repeat_equal\": %s, \"own_untouched\": %s, \"error\": \"%s\"}\n", ok ? "true" : "false", (long long)P,
              repeat_equal ? "true" : "false", own_untouched ? "true" : "false", err.c_str());
  return 0;
}
