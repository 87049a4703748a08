// The host plan of a batched k-NN covariance pass (cov_batch.hip): which of the listed clouds need the pass, in which chunks they go, and
// for every cloud the workgroups it owns in the two launches of its chunk.  No HIP in here: a CPU program can include this header and
// check the plan on its own (tests/cpp/cov_batch_plan_check.cpp).
//
// Also the one place that says how knn_lists (knn_lists.hip) shapes the search of a cloud: waves per leaf (`parts`) of the wave-per-leaf
// search, rounds per wave (`run`) of the per-query walk.  The slot order of a neighbour list depends on which queries a wave has open, and
// so on `parts`; gicp_cov_from_knn_body sums in slot order.  The batched pass therefore gives every cloud the shape it would get alone --
// both paths call the functions below -- and every wave of the batched launch does what its wave of the single launch does.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

namespace dgs {
namespace covplan {

constexpr int kPlanLeaf = 8;            // points per leaf of the index (nn_group.h kLeaf)
constexpr int kPlanWavesPerBlock = 4;   // waves per workgroup of the search (kBlock / kWave)
// Points per chunk of a batched pass: the neighbour table of a chunk is points * 32 (k <= 32) or * 64 ints, 512 MiB or 1 GiB at this
// budget.  DGS_COV_BATCH_POINTS in the environment of dgs_create overrides it.
constexpr int64_t kCovBatchPoints = (int64_t)4 << 20;

// Waves per leaf of the wave-per-leaf search (each answers 8 / parts of the leaf's queries after its own walk, whose loops run over ITS
// queries only): measured 1 / 2 / 4 / 8 waves per leaf: 0.168 / 0.148 / 0.143 / 0.160 ms per 65,536-point cloud, 0.099 / 0.076 / 0.065 /
// 0.069 ms per 26,668 points.  override_parts: DGS_KNN_PARTS (0 = by cloud size).
inline int knn_leaf_parts(const int64_t n, const int override_parts) {
  const int64_t n_leaves = (n + kPlanLeaf - 1) / kPlanLeaf;
  int parts = 1;
  while (parts < 4 && n_leaves * parts < 32768) parts *= 2;
  if (override_parts > 0) parts = override_parts;
  return parts;
}
inline int64_t knn_leaf_blocks(const int64_t n, const int parts) {
  const int64_t n_leaves = (n + kPlanLeaf - 1) / kPlanLeaf;
  return (n_leaves * parts + kPlanWavesPerBlock - 1) / kPlanWavesPerBlock;
}
// Rounds per wave of the per-query walk: enough waves to fill the chip several times over, and stretches long enough for the warm bounds
// to pay.  rounds: DGS_KNN_ROUNDS, min_waves: DGS_KNN_MIN_WAVES.
inline int knn_walk_run(const int64_t n, const int rounds, const int min_waves) {
  return (int)std::max<int64_t>(1, std::min<int64_t>(rounds, (n + 8 * (int64_t)min_waves - 1) / (8 * (int64_t)min_waves)));
}
inline int64_t knn_walk_blocks(const int64_t n, const int run) {
  const int64_t waves = (n + 8 * (int64_t)run - 1) / (8 * (int64_t)run);
  return (waves + kPlanWavesPerBlock - 1) / kPlanWavesPerBlock;
}

// The two covariance caches of a cloud.  kFast: FAST_GICP / FAST_VGICP, 6 doubles per point under (k, regularisation); kPcl: GICP_HIP /
// GICP_OMP_HIP, 9 doubles per point under (k, epsilon).
enum Kind { kFast = 0, kPcl = 1 };
struct Key {
  int kind;
  int k;
  int reg;      // kFast
  double eps;   // kPcl
};
// What the plan needs to know of a listed cloud: who it is, how large, and the key its cache of this kind holds.
struct CloudInfo {
  const void* id;
  int64_t n;
  bool cached;
  int cached_k, cached_reg;
  double cached_eps;
};
inline bool cache_hit(const Key& key, const CloudInfo& c) {
  if (!c.cached || c.cached_k != key.k) return false;
  return key.kind == kFast ? c.cached_reg == key.reg : c.cached_eps == key.eps;
}

struct Item {
  int input;          // index into the caller's list (first appearance)
  int64_t n;
  int parts;          // what knn_lists would give the cloud alone
  int knn_blk0, knn_blocks;   // first workgroup and workgroups in the chunk's search launch
  int cov_blk0, cov_blocks;   // ... and in its covariance launch
  int64_t nbr_point0;         // points of the chunk before this cloud: where its slice of the neighbour table begins
};
struct Chunk {
  int first, count;   // items [first, first + count)
  int64_t points;
  int knn_blocks, cov_blocks;
};
struct Plan {
  std::vector<Item> items;
  std::vector<Chunk> chunks;
  int listed = 0, cached = 0, duplicates = 0, empty = 0, too_small = 0;
  int64_t max_chunk_points = 0;
};

// Listed clouds -> the work.  Dropped: a cloud seen before in the list, an empty cloud, a cloud whose cache answers the key, and (kPcl) a
// cloud of fewer than k points -- computeCovariances refuses it, it stays without covariances.  The rest keep the order of the list and
// fill chunks greedily up to `budget` points; a cloud above the budget gets a chunk of its own.
inline Plan make_plan(const Key& key, const int n, const CloudInfo* clouds, const int64_t budget, const int override_parts, const int cov_points_per_block) {
  Plan P;
  P.listed = n;
  std::vector<const void*> seen;
  for (int i = 0; i < n; i++) {
    const CloudInfo& c = clouds[i];
    if (std::find(seen.begin(), seen.end(), c.id) != seen.end()) { P.duplicates++; continue; }
    seen.push_back(c.id);
    if (c.n <= 0) { P.empty++; continue; }
    if (cache_hit(key, c)) { P.cached++; continue; }
    if (key.kind == kPcl && (int64_t)key.k > c.n) { P.too_small++; continue; }
    Item it{};
    it.input = i;
    it.n = c.n;
    it.parts = knn_leaf_parts(c.n, override_parts);
    it.knn_blocks = (int)knn_leaf_blocks(c.n, it.parts);
    it.cov_blocks = (int)((c.n + cov_points_per_block - 1) / cov_points_per_block);
    if (P.chunks.empty() || P.chunks.back().points + c.n > budget) P.chunks.push_back(Chunk{(int)P.items.size(), 0, 0, 0, 0});
    Chunk& ch = P.chunks.back();
    it.knn_blk0 = ch.knn_blocks;
    it.cov_blk0 = ch.cov_blocks;
    it.nbr_point0 = ch.points;
    ch.count++;
    ch.points += c.n;
    ch.knn_blocks += it.knn_blocks;
    ch.cov_blocks += it.cov_blocks;
    P.max_chunk_points = std::max(P.max_chunk_points, ch.points);
    P.items.push_back(it);
  }
  return P;
}

}  // namespace covplan
}  // namespace dgs
