// The host plan of the prefilter over many scans (prefilter_batch.hip): the chunks a call's scans go in, for every stage which scans
// are still live and the workgroups each owns in the stage's launches, and what a scan's condition means for its status.  No HIP in
// here: a CPU program can include this header and check the plan on its own (tests/cpp/prefilter_batch_plan_check.cpp).
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

#include "cov_batch_plan.h"
#include "seg_table.h"

namespace dgs {
namespace pfbplan {

constexpr int kPlanBlock = 256;   // points per workgroup of the per-point passes and of the compaction (common.h kBlock)
// Raw points per chunk of a call: the neighbour table of a k-NN stage is at most this many points * 32 ints (512 MiB).
// DGS_PREFILTER_BATCH_POINTS in the environment of dgs_create overrides it.
constexpr int64_t kBatchPoints = (int64_t)4 << 20;
constexpr int kOk = 0, kInvalidArgument = 1;   // DGS_OK, DGS_ERR_INVALID_ARGUMENT (dgs_reg.h; prefilter_batch.hip asserts it)

// ---- chunks: the scans of a call in order, greedily up to `budget` raw points; a scan above the budget gets a chunk of its own, an
// empty scan rides along.  Each chunk runs the whole chain.
struct Chunk {
  int first, count;   // scans [first, first + count)
  int64_t points;
};
inline std::vector<Chunk> make_chunks(const int n_scans, const int64_t* sizes, const int64_t budget) {
  std::vector<Chunk> chunks;
  for (int s = 0; s < n_scans; s++) {
    if (chunks.empty() || (sizes[s] > 0 && chunks.back().points > 0 && chunks.back().points + sizes[s] > budget)) chunks.push_back(Chunk{s, 0, 0});
    chunks.back().count++;
    chunks.back().points += sizes[s];
  }
  return chunks;
}

// ---- a stage: the live scans (size > 0) in order.  Every live scan owns whole workgroups: ceil(n / 256) of the per-point launches from
// blk0 on, and (k-NN stages) the workgroups knn_lists would launch for it alone, with the `parts` it would get alone, from knn_blk0 on.
// point0: the live points before it -- where its slices of the per-point arrays (neighbour lists, mean distances, normals) begin.
struct Item {
  int scan;   // number of the scan inside its chunk
  int64_t n;
  int blk0, blocks;
  int knn_blk0, knn_blocks, parts;
  int64_t point0;
};
struct Stage {
  std::vector<Item> items;
  int blocks = 0, knn_blocks = 0;   // workgroups of the per-point launches / of the search launch
  int64_t points = 0;
  // first workgroup per item and, behind the last, the number of workgroups: what the launch bisects
  std::vector<int> first() const { return segtab::first_array(items.data(), items.size(), &Item::blk0, blocks); }
  std::vector<int> knn_first() const { return segtab::first_array(items.data(), items.size(), &Item::knn_blk0, knn_blocks); }
};
inline Stage make_stage(const int n_scans, const int64_t* sizes, const bool knn, const int override_parts) {
  Stage S;
  for (int s = 0; s < n_scans; s++) {
    if (sizes[s] <= 0) continue;   // a dead scan owns no workgroup
    Item it{};
    it.scan = s;
    it.n = sizes[s];
    it.blk0 = S.blocks;
    it.blocks = (int)((sizes[s] + kPlanBlock - 1) / kPlanBlock);
    it.knn_blk0 = S.knn_blocks;
    if (knn) {
      it.parts = covplan::knn_leaf_parts(sizes[s], override_parts);
      it.knn_blocks = (int)covplan::knn_leaf_blocks(sizes[s], it.parts);
    }
    it.point0 = S.points;
    S.blocks += it.blocks;
    S.knn_blocks += it.knn_blocks;
    S.points += sizes[s];
    S.items.push_back(it);
  }
  return S;
}

// ---- per-scan conditions -> what the single call would have returned for that scan
// StatisticalOutlierRemoval reads mean_k + 1 neighbours: 0 < points <= mean_k is the single call's DGS_ERR_INVALID_ARGUMENT; the scan
// is dead from there on and its counts are 0.  An empty scan stays DGS_OK.
inline int statistical_status(const int64_t n, const int mean_k) { return (n > 0 && n <= mean_k) ? kInvalidArgument : kOk; }
// RadiusOutlierRemoval with fewer than k = min_neighbors + 1 points: no point finds k neighbours, all are removed, DGS_OK
inline bool radius_removes_all(const int64_t n, const int k) { return n < k; }
// The outputs of a scan that finished the chain: the full counts are reported whatever the capacities; a count above its capacity is
// DGS_ERR_INVALID_ARGUMENT, and the single call stops at the first output that does not fit (the 3-D one goes first).
struct Outputs {
  int status;
  bool copy3d, copy2d;
};
inline Outputs output_status(const int64_t n3d, const int64_t cap3d, const int64_t n2d, const int64_t cap2d) {
  if (n3d > cap3d) return Outputs{kInvalidArgument, false, false};
  if (n2d > cap2d) return Outputs{kInvalidArgument, n3d > 0, false};
  return Outputs{kOk, n3d > 0, n2d > 0};
}

}  // namespace pfbplan
}  // namespace dgs
