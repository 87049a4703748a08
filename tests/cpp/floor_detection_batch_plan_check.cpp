// The host plan of floor detection over many scans (delta_graph_slam_amd/csrc/floor_detection_batch_plan.h) on its own, against
// expectations written by hand: first-workgroup tables at the sizes around a workgroup and a score tile, dead scans between live ones,
// chunk boundaries, the walks of scans that close in different rounds with the round tables and their y extent, the status mapping.
// No device, no library: built with g++ -fsanitize=address,undefined by tests/test_floor_detection_batch_cpu.py.  Prints "ok" and
// exits 0, or names the first failed check.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "floor_detection_batch_plan.h"

using namespace dgs::fdbplan;

static int failures = 0;
#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) {                                                         \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);        \
      failures++;                                                          \
    }                                                                      \
  } while (0)

struct Hyp {
  int draw;
};
static double cube(double w) { return std::pow(w, 3.0); }

int main() {
  // ---- first-workgroup tables of a filter stage at 0 / 1 / 256 / 257 / 1,023 / 1,024 / 1,025 points
  {
    const int64_t sizes[7] = {0, 1, 256, 257, 1023, 1024, 1025};
    const Stage S = make_stage(7, sizes);
    CHECK(S.items.size() == 6 && S.blocks == 1 + 1 + 2 + 4 + 4 + 5 && S.knn_blocks == 0 && S.points == 3586);
    CHECK((S.first() == std::vector<int>{0, 1, 2, 4, 8, 12, 17}));
    CHECK(S.items[0].scan == 1 && S.items[5].scan == 6 && S.items[3].point0 == 514 && S.items[5].point0 == 2561);
    const Stage E = make_stage(0, nullptr);
    CHECK(E.items.empty() && E.blocks == 0 && E.first() == std::vector<int>{0});
  }

  // ---- dead scans between live ones own nothing and shift nothing; every workgroup falls into exactly one scan
  {
    const int64_t sizes[7] = {300, 0, 0, 5, 0, 512, 0};
    const Stage S = make_stage(7, sizes);
    CHECK(S.items.size() == 3 && S.items[0].scan == 0 && S.items[1].scan == 3 && S.items[2].scan == 5);
    CHECK((S.first() == std::vector<int>{0, 2, 3, 5}));
    CHECK(S.items[1].point0 == 300 && S.items[2].point0 == 305 && S.points == 817);
    const std::vector<int> first = S.first();
    for (int blk = 0; blk < S.blocks; blk++) {
      int lo = 0, hi = (int)S.items.size();
      while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (first[mid] <= blk) lo = mid; else hi = mid;
      }
      CHECK(S.items[lo].blk0 <= blk && blk < S.items[lo].blk0 + S.items[lo].blocks);
    }
  }

  // ---- chunks: a budget of 300 raw points over 129, 200, 64, 0, 500, 0, 10
  {
    const int64_t sizes[7] = {129, 200, 64, 0, 500, 0, 10};
    const std::vector<Chunk> C = make_chunks(7, sizes, 300);
    CHECK(C.size() == 4);
    CHECK(C[0].first == 0 && C[0].count == 1 && C[0].points == 129);
    CHECK(C[1].first == 1 && C[1].count == 3 && C[1].points == 264);   // the empty scan rides along
    CHECK(C[2].first == 4 && C[2].count == 2 && C[2].points == 500);   // above the budget: a chunk of its own
    CHECK(C[3].first == 6 && C[3].count == 1 && C[3].points == 10);
    CHECK(make_chunks(7, sizes, kBatchPoints).size() == 1 && kBatchPoints == 4194304);
    CHECK(make_chunks(0, nullptr, 300).empty());
  }

  // ---- a round's table: tiles at 1 / 1,023 / 1,024 / 1,025 / 2,049 points, the y extent is the longest chunk's
  {
    Round R;
    round_add(R, 0, 1, 0, 64);
    round_add(R, 2, 1023, 64, 576);
    round_add(R, 3, 1024, 0, 64);
    round_add(R, 5, 1025, 576, 1001);
    round_add(R, 6, 2049, 64, 65);
    CHECK(R.tiles == 1 + 1 + 1 + 2 + 3 && (R.first() == std::vector<int>{0, 1, 2, 3, 5, 8}));
    CHECK(R.groups == 8);                                              // 512 hypotheses in groups of 64
    CHECK(R.h_lo == 0 && R.h_hi == 1001);
    CHECK(R.items[3].scan == 5 && R.items[3].tile0 == 3 && R.items[3].tiles == 2 && R.items[3].h_first == 576 && R.items[3].h_end == 1001);
    Round One;
    round_add(One, 0, 5000, 0, 65);
    CHECK(One.tiles == 5 && One.groups == 2 && One.h_lo == 0 && One.h_hi == 65);
  }

  // ---- walks that close in different rounds.  max_iterations 1000, chunks of 64 then 512, 100 points, every draw good.
  {
    const int max_it = 1000, max_hyp = 1001;
    const double log1p = std::log(1.0 - 0.99);
    std::vector<Hyp> hyps(max_hyp);
    for (int i = 0; i < max_hyp; i++) hyps[i].draw = i;
    // scan A: 90 of 100 inliers at rank 2 -> k = log(0.01) / log(1 - 0.729) = 3.5: closes at it = 4, in round 1
    // scan B: 90 inliers at rank 70 -> open after the first 64, closes in round 2
    // scan C: 3 inliers everywhere -> k stays huge: runs to it = 1001 > max_iterations, in round 3
    std::vector<int> ca(max_hyp, 3), cb(max_hyp, 3), cc(max_hyp, 3);
    ca[2] = 90;
    cb[70] = 90;
    ScanWalk A, B, C;
    A.n = B.n = C.n = 100;
    A.D = B.D = C.D = max_hyp + 64;
    ScanWalk* W[3] = {&A, &B, &C};
    const std::vector<int>* cnt[3] = {&ca, &cb, &cc};
    int closed_in[3] = {0, 0, 0}, rounds = 0;
    bool open[3] = {true, true, true};
    for (;;) {
      Round R;
      for (int j = 0; j < 3; j++) {
        if (!open[j]) continue;
        open[j] = W[j]->advance(hyps.data(), cnt[j]->data(), max_it, 64, 512, log1p, cube);
        if (open[j]) round_add(R, j, W[j]->n, W[j]->h_first, W[j]->h_end);
        else closed_in[j] = rounds;
      }
      if (R.items.empty()) break;
      rounds++;
      if (rounds == 1) CHECK(R.items.size() == 3 && R.groups == 1 && R.h_lo == 0 && R.h_hi == 64);
      if (rounds == 2) CHECK(R.items.size() == 2 && R.items[0].scan == 1 && R.groups == 8 && R.h_lo == 64 && R.h_hi == 576 && R.tiles == 2);
      if (rounds == 3) CHECK(R.items.size() == 1 && R.items[0].scan == 2 && R.groups == 7 && R.h_lo == 576 && R.h_hi == 1001);
      for (const RoundItem& it : R.items) W[it.scan]->scored_round(max_hyp + 64, INT_MAX, max_hyp);   // every draw of the list is good
    }
    CHECK(rounds == 3 && closed_in[0] == 1 && closed_in[1] == 2 && closed_in[2] == 3);
    CHECK(A.wk.win == 2 && A.wk.it == 4 && A.chunks == 1 && A.scored == 64 && A.wk.status == dgs::SAC_OK && A.wk.draws == 4);
    CHECK(B.wk.win == 70 && B.wk.it == 71 && B.chunks == 2 && B.scored == 576);
    CHECK(C.wk.win == 0 && C.wk.it == 1001 && C.chunks == 3 && C.scored == 1001 && C.wk.status == dgs::SAC_OK);
  }

  // ---- a list that ends: 30 good draws, then bad ones.  A completed run of bad draws fails the walk; a list that is merely too short
  // asks for more draws
  {
    const int max_it = 40;
    std::vector<Hyp> hyps(41);
    for (int i = 0; i < 41; i++) hyps[i].draw = i;
    const std::vector<int> c(41, 3);
    for (int failed = 0; failed < 2; failed++) {
      ScanWalk S;
      S.n = 100;
      S.D = 105;
      CHECK(S.advance(hyps.data(), c.data(), max_it, 64, 512, std::log(0.01), cube) && S.h_first == 0 && S.h_end == 41);
      S.scored_round(30, failed ? 100 : INT_MAX, 41);
      CHECK(S.scored == 30 && S.H == 30);
      CHECK(!S.advance(hyps.data(), c.data(), max_it, 64, 512, std::log(0.01), cube));
      CHECK(S.wk.it == 30 && S.wk.status == (failed ? dgs::SAC_FAILED : dgs::SAC_NEED_DRAWS) && S.wk.draws == (failed ? 101 : 105));
    }
  }

  // ---- the status mapping
  CHECK(!reaches_ransac(0, 0, 0));                                     // an empty scan returns at once, whatever the threshold
  CHECK(reaches_ransac(5, 0, 0) && !reaches_ransac(600, 511, 512) && reaches_ransac(600, 512, 512));
  CHECK(decide(511, 512, 1.0, 0.98) == kTooFewInliers && decide(512, 512, 1.0, 0.98) == kDetected);
  CHECK(decide(0, 0, 0.0, 0.98) == kNotVertical);                       // no model, threshold 0: the zero normal fails the verticality check
  CHECK(decide(900, 512, 0.97, 0.98) == kNotVertical && decide(900, 512, 0.98, 0.98) == kDetected);
  CHECK(kDetected == 0 && kTooFewPoints == 1 && kTooFewInliers == 2 && kNotVertical == 3 && kRngExhausted == 4);

  if (failures) return 1;
  std::printf("ok\n");
  return 0;
}
