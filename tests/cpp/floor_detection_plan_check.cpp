// The host plan of floor detection (delta_graph_slam_amd/csrc/floor_detection_plan.h) on its own, against
// expectations written by hand: first-workgroup tables at the sizes around a workgroup and a score tile, dead scans between live ones,
// chunk boundaries, the walks of scans that close in different rounds with the round tables and their y extent, the status mapping,
// the verdict's status, dot product and coefficients at its edges.
// No device, no library: built with g++ -fsanitize=address,undefined by tests/test_floor_detection_batch_cpu.py.  Prints "ok" and
// exits 0, or names the first failed check.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "floor_detection_plan.h"

using namespace dgs::fdplan;

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

// verdict() into outputs that start at 0
struct V {
  int status;
  float raw[4], dot, out[4];
};
static V run(const float* win, int64_t inliers, const float* tilt_inv16, int floor_pts_thresh, double floor_normal_thresh) {
  V v{};
  v.status = verdict(win, inliers, tilt_inv16, floor_pts_thresh, floor_normal_thresh, v.raw, &v.dot, v.out);
  return v;
}
static bool same4(const float* got, float a, float b, float c, float d) {   // bit for bit: -0.0f is not 0.0f
  const float want[4] = {a, b, c, d};
  return std::memcmp(got, want, sizeof(want)) == 0;
}

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

  // ---- the verdict: status, dot and coefficients as both calls store them (outputs start at 0, as a reset record's do)
  {
    const float eye[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};   // column-major: the reference is (0, 0, 1)
    const float up[4] = {0.f, 0.f, 1.f, -2.f};
    // no model: all-zero coefficients.  floor_pts_thresh 0 lets the count pass and the zero normal fails the verticality check
    V v = run(nullptr, 0, eye, 0, 10.0);
    CHECK(v.status == kNotVertical && v.dot == 0.f && same4(v.raw, 0.f, 0.f, 0.f, 0.f) && same4(v.out, 0.f, 0.f, 0.f, 0.f));
    v = run(nullptr, 0, eye, 1, 10.0);
    CHECK(v.status == kTooFewInliers && v.dot == 0.f && same4(v.raw, 0.f, 0.f, 0.f, 0.f) && same4(v.out, 0.f, 0.f, 0.f, 0.f));
    // one inlier below floor_pts_thresh: no dot product yet, the raw coefficients are the winner's all the same; exactly at it
    v = run(up, 511, eye, 512, 10.0);
    CHECK(v.status == kTooFewInliers && v.dot == 0.f && same4(v.raw, 0.f, 0.f, 1.f, -2.f) && same4(v.out, 0.f, 0.f, 0.f, 0.f));
    v = run(up, 512, eye, 512, 10.0);
    CHECK(v.status == kDetected && v.dot == 1.f && same4(v.raw, 0.f, 0.f, 1.f, -2.f) && same4(v.out, 0.f, 0.f, 1.f, -2.f));
    // |dot| == cos(floor_normal_thresh) exactly (0 degrees: cos = 1): the comparison is <, so DETECTED; one float below 1: NOT_VERTICAL
    v = run(up, 600, eye, 512, 0.0);
    CHECK(v.status == kDetected && v.dot == 1.f && same4(v.out, 0.f, 0.f, 1.f, -2.f));
    const float below[4] = {0.f, 0.f, 0.99999994f, -2.f};
    v = run(below, 600, eye, 512, 0.0);
    CHECK(v.status == kNotVertical && v.dot == 0.99999994f && same4(v.raw, 0.f, 0.f, 0.99999994f, -2.f) && same4(v.out, 0.f, 0.f, 0.f, 0.f));
    // a downward normal: all four come back times -1, the signs of zeros included
    const float down[4] = {0.f, 0.25f, -1.f, 0.f};
    v = run(down, 600, eye, 512, 10.0);
    CHECK(v.status == kDetected && v.dot == -1.f && same4(v.raw, 0.f, 0.25f, -1.f, 0.f) && same4(v.out, -0.f, -0.25f, 1.f, -0.f));
    const float down_neg0[4] = {-0.f, 0.f, -1.f, -0.f};
    v = run(down_neg0, 600, eye, 512, 10.0);
    CHECK(v.status == kDetected && v.dot == -1.f && same4(v.raw, -0.f, 0.f, -1.f, -0.f) && same4(v.out, 0.f, -0.f, 1.f, 0.f));
    // a tilted sensor: the reference is the third COLUMN (0.5, 0.25, 0.75), not the third row (9, 9, 0.75)
    float tilt[16] = {1, 0, 9, 0, 0, 1, 9, 0, 0.5f, 0.25f, 0.75f, 0, 0, 0, 0, 1};
    const float plane[4] = {0.5f, 0.5f, 0.75f, -2.f};   // (0.25 + 0.125) + 0.5625 = 0.9375; cos 10 deg = 0.98..., cos 25 deg = 0.90...
    v = run(plane, 600, tilt, 512, 10.0);
    CHECK(v.status == kNotVertical && v.dot == 0.9375f && same4(v.raw, 0.5f, 0.5f, 0.75f, -2.f) && same4(v.out, 0.f, 0.f, 0.f, 0.f));
    v = run(plane, 600, tilt, 512, 25.0);
    CHECK(v.status == kDetected && v.dot == 0.9375f && same4(v.out, 0.5f, 0.5f, 0.75f, -2.f));
  }

  if (failures) return 1;
  std::printf("ok\n");
  return 0;
}
