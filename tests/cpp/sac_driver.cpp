// Host pieces of delta_graph_slam_amd/csrc/sac.h driven from a command file on stdin, one answer line per command (tests/test_sac_cpu.py):
//   draws K n D R r0 .. r(R-1)     sac_draws<K> over R raw values (R = 0: the built-in generator) -> the K * D indices, then 1 when the
//                                  permutation, kept across commands and grown on demand like a handle's, is the identity again
//   walk K n max_iterations probability M c0 .. c(M-1)
//                                  SacWalk::step over the counts while the loop is open -> winner, iterations, 1 when it ran past the counts
//   next draw fail_at              SacWalk::next -> its return value, status, draws
//   end fail_at D                  SacWalk::end_of_list -> status, draws
//   plan avail max_hyp bad_run G   SacDrawPlan -> empty(), D, then G times: grow()'s return value, D
// Plain C++17, no device.
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>

#include "../../delta_graph_slam_amd/csrc/sac.h"

using namespace dgs;

namespace {

std::vector<int> g_perm;

template <int K>
void draws(std::istringstream& in) {
  long long n, D, R;
  in >> n >> D >> R;
  std::vector<uint32_t> raw((size_t)R);
  for (uint32_t& v : raw) in >> v;
  if (R == 0) sac_grow_mt(raw, K * D);
  if ((long long)raw.size() < K * D) { std::puts("short raw"); std::exit(2); }
  sac_grow_perm(g_perm, n);
  std::vector<int> out((size_t)(K * D));
  sac_draws<K>(g_perm, raw.data(), n, D, out.data());
  for (int v : out) std::printf("%d ", v);
  bool identity = true;
  for (size_t i = 0; i < g_perm.size(); i++) identity = identity && g_perm[i] == (int)i;
  std::printf("%d\n", identity ? 1 : 0);
}

template <class Power>
void walk(std::istringstream& in, Power power) {
  long long n, M;
  int max_iterations;
  double probability;
  in >> n >> max_iterations >> probability >> M;
  std::vector<int> counts((size_t)M);
  for (int& c : counts) in >> c;
  SacWalk wk;
  const double log_one_minus_p = std::log(1.0 - probability);
  bool broke = false;
  while (wk.open() && wk.it < M) {
    if (!wk.step(counts[(size_t)wk.it], n, max_iterations, log_one_minus_p, power)) { broke = true; break; }
  }
  std::printf("%d %d %d\n", wk.win, wk.it, (!broke && wk.open()) ? 1 : 0);
}

}  // namespace

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string cmd;
    if (!(in >> cmd)) continue;
    if (cmd == "draws" || cmd == "walk") {
      int K;
      in >> K;
      if (K != 2 && K != 3) { std::puts("bad K"); return 2; }
      if (cmd == "draws") {
        K == 2 ? draws<2>(in) : draws<3>(in);
      } else if (K == 2) {
        walk(in, [](double w) { return w * w; });             // the line model's power, as line_extraction.hip writes it
      } else {
        walk(in, [](double w) { return std::pow(w, 3.0); });  // the plane model's, as floor_detection.hip writes it
      }
    } else if (cmd == "next") {
      int draw, fail_at;
      in >> draw >> fail_at;
      SacWalk wk;
      const bool ok = wk.next(draw, fail_at);
      std::printf("%d %d %d\n", ok ? 1 : 0, wk.status, wk.draws);
    } else if (cmd == "end") {
      int fail_at, D;
      in >> fail_at >> D;
      SacWalk wk;
      wk.end_of_list(fail_at, D);
      std::printf("%d %d\n", wk.status, wk.draws);
    } else if (cmd == "plan") {
      long long avail;
      int max_hyp, bad_run, G;
      in >> avail >> max_hyp >> bad_run >> G;
      SacDrawPlan plan(avail, max_hyp, bad_run);
      std::printf("%d %lld", plan.empty() ? 1 : 0, (long long)plan.D);
      for (int g = 0; g < G; g++) {
        const bool ok = plan.grow();
        std::printf(" %d %lld", ok ? 1 : 0, (long long)plan.D);
      }
      std::printf("\n");
    } else {
      std::puts("bad command");
      return 2;
    }
  }
  return 0;
}
