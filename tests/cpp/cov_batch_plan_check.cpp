// The host plan of the batched covariance pass (delta_graph_slam_amd/csrc/cov_batch_plan.h) on its own, against expectations written by
// hand: cache filtering by key, de-duplication, chunking, workgroup prefixes, `parts` per size.  No device, no library: built with
// g++ -fsanitize=address,undefined by tests/test_cov_batch_cpu.py.  Prints "ok" and exits 0, or names the first failed check.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "cov_batch_plan.h"

using namespace dgs::covplan;

static int failures = 0;
#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) {                                                         \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);        \
      failures++;                                                          \
    }                                                                      \
  } while (0)

static CloudInfo fresh(const void* id, int64_t n) { return CloudInfo{id, n, false, 0, -1, 0.0}; }

int main() {
  // ---- parts: what knn_lists gives a cloud alone.  Fewer than 32,768 (leaves x parts) doubles parts, up to 4.
  CHECK(knn_leaf_parts(1, 0) == 4);
  CHECK(knn_leaf_parts(1000, 0) == 4);
  CHECK(knn_leaf_parts(65536, 0) == 4);       // 8,192 leaves: x 4 = 32,768 reached at 4
  CHECK(knn_leaf_parts(131064, 0) == 4);      // 16,383 leaves: x 2 = 32,766, one more doubling
  CHECK(knn_leaf_parts(131065, 0) == 2);      // 16,384 leaves
  CHECK(knn_leaf_parts(131072, 0) == 2);      // 16,384 leaves: x 2 = 32,768
  CHECK(knn_leaf_parts(131073, 0) == 2);      // 16,385 leaves
  CHECK(knn_leaf_parts(131080, 0) == 2);
  CHECK(knn_leaf_parts(262136, 0) == 2);      // 32,767 leaves: one short of 32,768
  CHECK(knn_leaf_parts(262137, 0) == 1);      // 32,768 leaves
  CHECK(knn_leaf_parts(262144, 0) == 1);
  CHECK(knn_leaf_parts(262144, 8) == 8);      // DGS_KNN_PARTS overrides whatever the size
  CHECK(knn_leaf_parts(1000, 1) == 1);
  // workgroups of the search: ceil(leaves * parts / 4 waves)
  CHECK(knn_leaf_blocks(1, 4) == 1);
  CHECK(knn_leaf_blocks(8, 4) == 1);
  CHECK(knn_leaf_blocks(9, 4) == 2);
  CHECK(knn_leaf_blocks(1000, 4) == 125);
  CHECK(knn_leaf_blocks(3001, 4) == 376);
  CHECK(knn_leaf_blocks(262144, 1) == 8192);
  CHECK(knn_leaf_blocks(131080, 2) == 8193);  // 16,385 leaves x 2 = 32,770 waves
  // the per-query walk's shape (defaults: 8 rounds, 4,096 waves)
  CHECK(knn_walk_run(1000, 8, 4096) == 1);
  CHECK(knn_walk_run(65536, 8, 4096) == 2);
  CHECK(knn_walk_run(1 << 20, 8, 4096) == 8);
  CHECK(knn_walk_blocks(1000, 1) == 32);      // 125 waves
  CHECK(knn_walk_blocks(65536, 2) == 1024);

  // ---- cache filtering by key
  {
    const Key fast{kFast, 20, 2, 0.0}, pcl{kPcl, 20, 0, 1e-3};
    const CloudInfo hit{nullptr, 100, true, 20, 2, 1e-3};
    CHECK(cache_hit(fast, hit));
    CHECK(cache_hit(pcl, hit));
    CloudInfo c = hit;
    c.cached = false;
    CHECK(!cache_hit(fast, c) && !cache_hit(pcl, c));
    c = hit; c.cached_k = 19;
    CHECK(!cache_hit(fast, c) && !cache_hit(pcl, c));
    c = hit; c.cached_reg = 3;
    CHECK(!cache_hit(fast, c) && cache_hit(pcl, c));      // the regularisation is FAST_GICP's key only
    c = hit; c.cached_eps = 2e-3;
    CHECK(cache_hit(fast, c) && !cache_hit(pcl, c));      // epsilon is GICP_HIP's key only
  }

  // ---- an empty list
  {
    const Plan P = make_plan(Key{kFast, 20, 2, 0.0}, 0, nullptr, kCovBatchPoints, 0, 128);
    CHECK(P.listed == 0 && P.items.empty() && P.chunks.empty() && P.max_chunk_points == 0);
  }

  // ---- the sizes at the edges of every unit, scrambled, one chunk, FAST_GICP (128 points per covariance workgroup)
  {
    const int64_t sizes[] = {257, 1, 1000, 64, 9, 3001, 128, 7, 255, 65, 8, 129, 63, 256, 127};
    const int n = (int)(sizeof(sizes) / sizeof(sizes[0]));
    int ids[16];
    std::vector<CloudInfo> in;
    for (int i = 0; i < n; i++) in.push_back(fresh(&ids[i], sizes[i]));
    const Plan P = make_plan(Key{kFast, 20, 2, 0.0}, n, in.data(), kCovBatchPoints, 0, 128);
    CHECK(P.listed == n && (int)P.items.size() == n && P.chunks.size() == 1 && P.cached == 0 && P.duplicates == 0 && P.empty == 0 && P.too_small == 0);
    //                       257  1 1000 64  9 3001 128  7 255 65  8 129 63 256 127
    const int knn_blocks[] = {33, 1, 125, 8, 2, 376, 16, 1, 32, 9, 1, 17, 8, 32, 16};
    const int cov_blocks[] = {3, 1, 8, 1, 1, 24, 1, 1, 2, 1, 1, 2, 1, 2, 1};
    int knn0 = 0, cov0 = 0;
    int64_t pts = 0;
    for (int i = 0; i < n && i < (int)P.items.size(); i++) {
      const Item& it = P.items[i];
      CHECK(it.input == i && it.n == sizes[i] && it.parts == 4);
      CHECK(it.knn_blocks == knn_blocks[i] && it.cov_blocks == cov_blocks[i]);
      CHECK(it.knn_blk0 == knn0 && it.cov_blk0 == cov0 && it.nbr_point0 == pts);
      knn0 += knn_blocks[i]; cov0 += cov_blocks[i]; pts += sizes[i];
    }
    CHECK(P.chunks[0].first == 0 && P.chunks[0].count == n && P.chunks[0].points == pts && P.chunks[0].knn_blocks == knn0 && P.chunks[0].cov_blocks == cov0);
    CHECK(knn0 == 677 && cov0 == 50 && pts == 5370 && P.max_chunk_points == 5370);
    // GICP_HIP at k = 20 (256 points per covariance workgroup): the clouds of 1, 9, 7 and 8 points stay out
    const Plan Q = make_plan(Key{kPcl, 20, 0, 1e-3}, n, in.data(), kCovBatchPoints, 0, 256);
    CHECK(Q.too_small == 4 && (int)Q.items.size() == n - 4 && Q.chunks.size() == 1);
    CHECK(Q.items[0].input == 0 && Q.items[0].cov_blocks == 2 && Q.items[1].input == 2 && Q.items[1].cov_blocks == 4 && Q.items[1].cov_blk0 == 2);
    CHECK(Q.items[1].knn_blk0 == 33 && Q.items[1].nbr_point0 == 257);   // the dropped cloud of 1 point owns nothing
  }

  // ---- the `parts` case: 262,144 (1), 131,080 (2), 1,000 (4) points in one chunk
  {
    int ids[3];
    const CloudInfo in[3] = {fresh(&ids[0], 262144), fresh(&ids[1], 131080), fresh(&ids[2], 1000)};
    const Plan P = make_plan(Key{kFast, 20, 2, 0.0}, 3, in, kCovBatchPoints, 0, 128);
    CHECK(P.items.size() == 3 && P.chunks.size() == 1);
    CHECK(P.items[0].parts == 1 && P.items[1].parts == 2 && P.items[2].parts == 4);
    CHECK(P.items[0].knn_blk0 == 0 && P.items[1].knn_blk0 == 8192 && P.items[2].knn_blk0 == 8192 + 8193 && P.chunks[0].knn_blocks == 8192 + 8193 + 125);
    CHECK(P.items[1].cov_blk0 == 2048 && P.items[2].cov_blk0 == 2048 + 1025 && P.chunks[0].cov_blocks == 2048 + 1025 + 8);
    const Plan O = make_plan(Key{kFast, 20, 2, 0.0}, 3, in, kCovBatchPoints, 2, 128);   // DGS_KNN_PARTS=2
    CHECK(O.items[0].parts == 2 && O.items[1].parts == 2 && O.items[2].parts == 2 && O.items[0].knn_blocks == 16384 && O.items[2].knn_blocks == 63);
  }

  // ---- chunks: a budget of 300 points over 129, 200, 64, 500, 10
  {
    int ids[5];
    const CloudInfo in[5] = {fresh(&ids[0], 129), fresh(&ids[1], 200), fresh(&ids[2], 64), fresh(&ids[3], 500), fresh(&ids[4], 10)};
    const Plan P = make_plan(Key{kFast, 20, 2, 0.0}, 5, in, 300, 0, 128);
    CHECK(P.chunks.size() == 4 && P.items.size() == 5);
    CHECK(P.chunks[0].first == 0 && P.chunks[0].count == 1 && P.chunks[0].points == 129);
    CHECK(P.chunks[1].first == 1 && P.chunks[1].count == 2 && P.chunks[1].points == 264);
    CHECK(P.chunks[2].first == 3 && P.chunks[2].count == 1 && P.chunks[2].points == 500);   // above the budget: a chunk of its own
    CHECK(P.chunks[3].first == 4 && P.chunks[3].count == 1 && P.chunks[3].points == 10);
    CHECK(P.max_chunk_points == 500);
    // every chunk counts its workgroups and its points from zero
    CHECK(P.items[1].knn_blk0 == 0 && P.items[1].nbr_point0 == 0 && P.items[2].knn_blk0 == 25 && P.items[2].cov_blk0 == 2 && P.items[2].nbr_point0 == 200);
    CHECK(P.items[3].knn_blk0 == 0 && P.items[3].cov_blk0 == 0 && P.items[3].nbr_point0 == 0 && P.items[4].knn_blk0 == 0 && P.items[4].nbr_point0 == 0);
    CHECK(P.chunks[1].knn_blocks == 25 + 8 && P.chunks[1].cov_blocks == 2 + 1 && P.chunks[2].knn_blocks == 63 && P.chunks[2].cov_blocks == 4);
    // exactly the budget still fits
    const CloudInfo fit[2] = {fresh(&ids[0], 100), fresh(&ids[1], 200)};
    CHECK(make_plan(Key{kFast, 20, 2, 0.0}, 2, fit, 300, 0, 128).chunks.size() == 1);
    const CloudInfo over[2] = {fresh(&ids[0], 100), fresh(&ids[1], 201)};
    CHECK(make_plan(Key{kFast, 20, 2, 0.0}, 2, over, 300, 0, 128).chunks.size() == 2);
  }

  // ---- duplicates, empty clouds, valid caches
  {
    int ids[4];
    CloudInfo cached = fresh(&ids[2], 300);
    cached.cached = true; cached.cached_k = 20; cached.cached_reg = 2;
    CloudInfo stale = fresh(&ids[3], 400);
    stale.cached = true; stale.cached_k = 10; stale.cached_reg = 2;
    const CloudInfo in[7] = {fresh(&ids[0], 100), fresh(&ids[1], 0), fresh(&ids[0], 100), cached, stale, cached, fresh(&ids[1], 0)};
    const Plan P = make_plan(Key{kFast, 20, 2, 0.0}, 7, in, kCovBatchPoints, 0, 128);
    CHECK(P.listed == 7 && P.duplicates == 3 && P.empty == 1 && P.cached == 1 && P.items.size() == 2);
    CHECK(P.items[0].input == 0 && P.items[1].input == 4 && P.items[1].n == 400 && P.items[1].nbr_point0 == 100);
    // everything cached: nothing to do
    const CloudInfo all[2] = {cached, cached};
    const Plan Q = make_plan(Key{kFast, 20, 2, 0.0}, 2, all, kCovBatchPoints, 0, 128);
    CHECK(Q.items.empty() && Q.chunks.empty() && Q.cached == 1 && Q.duplicates == 1);
  }

  if (failures) return 1;
  std::printf("ok\n");
  return 0;
}
