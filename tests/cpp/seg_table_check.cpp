// The layout helper of the batched calls (delta_graph_slam_amd/csrc/seg_table.h) on its own, against offsets written out by hand: the
// stage block of the prefilter over many scans (entries of 144 bytes, heads of 136) and the per-chunk sections of the batched covariance
// pass (entries of 96 bytes) for m = 0, 1 and 3, the offset allocator at its alignments, and the first-workgroup array of a stage with
// an empty item in the middle.  No device, no library: built with g++ -fsanitize=address,undefined by tests/test_prefilter_batch_cpu.py.
// Prints "ok" and exits 0, or names the first failed check.
#include <cstdio>
#include <vector>

#include "prefilter_batch_plan.h"
#include "seg_table.h"

using namespace dgs::segtab;

static int failures = 0;
#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) {                                                         \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);        \
      failures++;                                                          \
    }                                                                      \
  } while (0)

static bool same(const StageTable& t, size_t entries, size_t heads, size_t first, size_t knn_first, size_t up, size_t totals, size_t stats, size_t all) {
  return t.entries == entries && t.heads == heads && t.first == first && t.knn_first == knn_first && t.up == up && t.totals == totals && t.stats == stats &&
         t.all == all;
}
static bool same(const ChunkTable& t, size_t entries, size_t knn_first, size_t cov_first, size_t end) {
  return t.entries == entries && t.knn_first == knn_first && t.cov_first == cov_first && t.end == end;
}

int main() {
  constexpr size_t kSeg = 144, kHead = 136, kEntry = 96;   // sizeof(PfbSeg), sizeof(PfHead), sizeof(CovBatchEntry)

  // ---- the allocator: places are multiples of the alignment, the end is not rounded, an empty take still aligns
  {
    Layout L;
    CHECK(L.take(5, 128) == 0 && L.end == 5);
    CHECK(L.take(3, 8) == 8 && L.end == 11);
    CHECK(L.take(0, 64) == 64 && L.end == 64);
    CHECK(L.take(1, 4) == 64 && L.end == 65);
    CHECK(L.take(4, 4) == 68 && L.end == 72);
    CHECK(L.take(0, 8) == 72 && L.take(16, 128) == 128 && L.end == 144);
  }

  // ---- the stage block: entries | heads | first (m + 1 ints) | knn first (m + 1 ints) go up; totals (m ints) | stats (4 m doubles) stay
  // m = 0: two one-entry arrays, each in a 64-byte line of its own
  CHECK(same(stage_table(0, kSeg, 0), 0, 0, 0, 64, 128, 128, 128, 128));
  CHECK(same(stage_table(0, kSeg, kHead), 0, 0, 0, 64, 128, 128, 128, 128));
  // m = 1 without heads: 144 -> 192; 8 bytes of firsts -> 256; 8 -> 320 = up; 4 -> 384; 32 -> 416
  CHECK(same(stage_table(1, kSeg, 0), 0, 192, 192, 256, 320, 320, 384, 416));
  // m = 1 with heads: 144 -> 192; 192 + 136 = 328 -> 384; 392 -> 448; 456 -> 512 = up; 516 -> 576; + 32
  CHECK(same(stage_table(1, kSeg, kHead), 0, 192, 384, 448, 512, 512, 576, 608));
  // m = 3 without heads: 432 -> 448; 464 -> 512; 528 -> 576 = up; 588 -> 640; + 96
  CHECK(same(stage_table(3, kSeg, 0), 0, 448, 448, 512, 576, 576, 640, 736));
  // m = 3 with heads: 432 -> 448; 448 + 408 = 856 -> 896; 912 -> 960; 976 -> 1024 = up; 1036 -> 1088; + 96
  CHECK(same(stage_table(3, kSeg, kHead), 0, 448, 896, 960, 1024, 1024, 1088, 1184));

  // ---- chunk sections: entries | knn first (count + 1 ints) | cov first (count + 1 ints), packed; the next chunk from a multiple of 64
  {
    Layout L;
    CHECK(same(chunk_table(L, 0, kEntry), 0, 0, 4, 8) && L.end == 64);
    CHECK(same(chunk_table(L, 1, kEntry), 64, 160, 168, 176) && L.end == 192);
    CHECK(same(chunk_table(L, 3, kEntry), 192, 480, 496, 512) && L.end == 512);   // 512 is a multiple of 64 already
    CHECK(same(chunk_table(L, 1, kEntry), 512, 608, 616, 624) && L.end == 640);
    Layout one;
    CHECK(same(chunk_table(one, 3, kEntry), 0, 288, 304, 320) && one.end == 320);
  }

  // ---- the first-workgroup array: the items' firsts, then the total; an item without workgroups repeats its successor's first, and the
  // bisection of the launches never lands on it
  {
    struct It { int blk0, blocks, other; };
    const std::vector<It> items = {{0, 2, 7}, {2, 0, 8}, {2, 3, 9}};   // the one in the middle is empty
    const std::vector<int> f = first_array(items.data(), items.size(), &It::blk0, 5);
    CHECK((f == std::vector<int>{0, 2, 2, 5}));
    CHECK((first_array(items.data(), items.size(), &It::other, 10) == std::vector<int>{7, 8, 9, 10}));
    CHECK((first_array(items.data(), 0, &It::blk0, 0) == std::vector<int>{0}));
    CHECK((first_array(items.data() + 1, 2, &It::blk0, 5) == std::vector<int>{2, 2, 5}));   // a chunk's items are a slice of the plan's
    for (int blk = 0; blk < 5; blk++) {
      int lo = 0, hi = (int)items.size();
      while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (f[mid] <= blk) lo = mid; else hi = mid;
      }
      CHECK(lo != 1 && items[lo].blk0 <= blk && blk < items[lo].blk0 + items[lo].blocks);
    }
    // empty items first and last
    const std::vector<It> edge = {{0, 0, 0}, {0, 1, 0}, {1, 0, 0}};
    const std::vector<int> g = first_array(edge.data(), edge.size(), &It::blk0, 1);
    int lo = 0, hi = 3;
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (g[mid] <= 0) lo = mid; else hi = mid;
    }
    CHECK((g == std::vector<int>{0, 0, 1, 1}) && lo == 1);
  }

  // ---- a stage of the plan goes through the same function
  {
    const int64_t sizes[4] = {300, 0, 5, 512};
    const dgs::pfbplan::Stage S = dgs::pfbplan::make_stage(4, sizes, true, 0);
    CHECK((S.first() == first_array(S.items.data(), S.items.size(), &dgs::pfbplan::Item::blk0, S.blocks)));
    CHECK((S.first() == std::vector<int>{0, 2, 3, 5}) && (S.knn_first() == std::vector<int>{0, 38, 39, 103}));
  }

  if (failures) return 1;
  std::printf("ok\n");
  return 0;
}
