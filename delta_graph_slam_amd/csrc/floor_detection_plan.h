// The host plan of floor detection, for one scan (floor_detection.hip) and for many (floor_detection_batch.hip): the state of a scan's
// walk between score launches of the RANSAC and what a scan's condition means for its status and coefficients, which both calls run;
// for the batch besides, the chunks a call's scans go in and the live scans of a filter stage with their first workgroups and point
// offsets (both prefilter_batch_plan.h's, used as they are) and the table of a round's score launch.
// No HIP in here: a CPU program can include this header and check the plan on its own (tests/cpp/floor_detection_plan_check.cpp).
#pragma once
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>
#include <vector>

#include "prefilter_batch_plan.h"
#include "sac.h"

namespace dgs {
namespace fdplan {

using pfbplan::Chunk;
using pfbplan::Item;
using pfbplan::Stage;
using pfbplan::make_chunks;

// Raw points per chunk of a call: the neighbour table of the normal stage is at most this many points * 32 ints (512 MiB).
// DGS_FLOOR_BATCH_POINTS in the environment of dgs_create overrides it.
constexpr int64_t kBatchPoints = (int64_t)4 << 20;
constexpr int kTile = 1024;      // points per workgroup of the score launch (sac.h kSacTile; floor_detection_batch.hip asserts it)
constexpr int kHypGroup = 64;    // hypotheses per workgroup of the score launch (floor_detection_body.h kFdHypSub)
// dgs_floor_detection_status (dgs_reg.h; floor_detection_batch.hip asserts them)
constexpr int kDetected = 0, kTooFewPoints = 1, kTooFewInliers = 2, kNotVertical = 3, kRngExhausted = 4;

// a filter stage without a search: every live scan owns ceil(n / 256) workgroups
inline Stage make_stage(const int n_scans, const int64_t* sizes) { return pfbplan::make_stage(n_scans, sizes, false, 0); }

// ---- the RANSAC of one scan between score launches: the single call's loop (floor_detection.hip fd_ransac) and a scan's part of the
// batch's rounds.  advance() walks the counts the host holds until the walk closes (-> false) or needs hypotheses nobody scored yet
// (-> true, [h_first, h_end) is the chunk to score: the first holds chunk_first hypotheses, every further one `chunk`);
// scored_round() takes what the launch brought back: meta[0] good draws, meta[1] the draw that completes a run of bad ones.
struct ScanWalk {
  SacWalk wk;
  int64_t n = 0, D = 0;            // points of the filtered cloud, draws of the list
  int scored = 0, chunks = 0, H = 0, fail_at = INT_MAX;
  int h_first = 0, h_end = 0;      // the chunk of the round it is open in
  template <class Hyp, class Power>
  bool advance(const Hyp* hyps, const int* counts, const int max_iterations, const int chunk_first, const int chunk, const double log_one_minus_p, Power power) {
    const int max_hyp = max_iterations + 1;
    while (wk.open()) {
      if (wk.it >= scored) {
        if (chunks > 0 && scored >= H) {
          wk.end_of_list(fail_at, (int)D);
          break;
        }
        h_first = scored;
        h_end = (int)std::min<int64_t>(max_hyp, (int64_t)scored + (chunks == 0 ? chunk_first : chunk));
        return true;
      }
      if (!wk.next(hyps[wk.it].draw, fail_at)) break;
      if (!wk.step(counts[wk.it], n, max_iterations, log_one_minus_p, power)) break;
    }
    return false;
  }
  void scored_round(const int meta0, const int meta1, const int max_hyp) {
    chunks++;
    H = std::min(meta0, max_hyp);
    fail_at = meta1;
    scored = std::min(h_end, H);
  }
};

// ---- a round's score launch: x = the 1,024-point tiles of the open scans back to back, y = the hypothesis groups of the longest chunk
struct RoundItem {
  int scan;          // number among the scans that reached the RANSAC
  int64_t n;
  int tile0, tiles;
  int h_first, h_end;
};
struct Round {
  std::vector<RoundItem> items;
  int tiles = 0, groups = 0;   // gridDim.x, gridDim.y
  int h_lo = 0, h_hi = 0;      // the hypotheses the round's download covers: [min h_first, max h_end)
  std::vector<int> first() const { return segtab::first_array(items.data(), items.size(), &RoundItem::tile0, tiles); }
};
inline void round_add(Round& R, const int scan, const int64_t n, const int h_first, const int h_end) {
  RoundItem it{};
  it.scan = scan;
  it.n = n;
  it.tile0 = R.tiles;
  it.tiles = (int)((n + kTile - 1) / kTile);
  it.h_first = h_first;
  it.h_end = h_end;
  R.h_lo = R.items.empty() ? h_first : std::min(R.h_lo, h_first);
  R.h_hi = R.items.empty() ? h_end : std::max(R.h_hi, h_end);
  R.tiles += it.tiles;
  R.groups = std::max(R.groups, (h_end - h_first + kHypGroup - 1) / kHypGroup);
  R.items.push_back(it);
}

// ---- per-scan conditions -> the status the single call gives that scan
// before the RANSAC: an empty scan returns at once (cloud_callback, :76-78), whatever floor_pts_thresh; fewer filtered points than
// floor_pts_thresh is TOO_FEW_POINTS (:133)
inline bool reaches_ransac(const int64_t n, const int64_t n_filtered, const int floor_pts_thresh) { return n > 0 && n_filtered >= (int64_t)floor_pts_thresh; }
// behind it (:147, :157-158), the integer and threshold core of verdict(): `inliers` is the winner's count (0 without a model), abs_dot the verticality check's |dot product|
inline int decide(const int64_t inliers, const int floor_pts_thresh, const double abs_dot, const double cos_thresh) {
  if (inliers < (int64_t)floor_pts_thresh) return kTooFewInliers;
  if (abs_dot < cos_thresh) return kNotVertical;
  return kDetected;
}
// The checks behind the RANSAC with their arithmetic (:147-166), for the single call and every scan of a batch.  `win`: the winner's
// four coefficients, or nullptr without a model (all zero); `inliers`: its inlier count.  -> the status.  raw_coeffs: the coefficients
// as the RANSAC gave them; *dot, written once the count passed: their float dot product with the reference; coeffs_out, written when
// the floor is DETECTED: the plane with its normal upward.
inline int verdict(const float* win, const int64_t inliers, const float* tilt_inv16, const int floor_pts_thresh, const double floor_normal_thresh,
                   float* raw_coeffs, float* dot_out, float* coeffs_out) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  float coeffs[4];
  for (int a = 0; a < 4; a++) raw_coeffs[a] = coeffs[a] = win ? win[a] : 0.f;
  if (decide(inliers, floor_pts_thresh, 1.0, 0.0) != kDetected) return kTooFewInliers;   // :147, before the dot product exists
  // reference = tilt_matrix.inverse() * UnitZ: the third column (:152); the dot product in float, compared in double (:157-158)
  const float rx = tilt_inv16[8], ry = tilt_inv16[9], rz = tilt_inv16[10];
  const float dot = (coeffs[0] * rx + coeffs[1] * ry) + coeffs[2] * rz;
  *dot_out = dot;
  const int status = decide(inliers, floor_pts_thresh, std::abs((double)dot), std::cos(floor_normal_thresh * M_PI / 180.0));
  if (status != kDetected) return status;
  // make the normal upward (:164-166)
  const float up = (0.0f * coeffs[0] + 0.0f * coeffs[1]) + 1.0f * coeffs[2];
  for (int a = 0; a < 4; a++) coeffs_out[a] = up < 0.0f ? coeffs[a] * -1.0f : coeffs[a];
  return kDetected;
}

}  // namespace fdplan
}  // namespace dgs
