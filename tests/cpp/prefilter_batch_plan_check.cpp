// The host plan of the batched prefilter (delta_graph_slam_amd/csrc/prefilter_batch_plan.h) on its own, against expectations written by
// hand: first-workgroup tables at the sizes around a workgroup, dead scans between live ones, chunk boundaries, the status mapping.
// No device, no library: built with g++ -fsanitize=address,undefined by tests/test_prefilter_batch_cpu.py.  Prints "ok" and exits 0, or
// names the first failed check.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "prefilter_batch_plan.h"

using namespace dgs::pfbplan;

static int failures = 0;
#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) {                                                         \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);        \
      failures++;                                                          \
    }                                                                      \
  } while (0)

int main() {
  // ---- no scans, and scans that are all dead: no workgroup, tables of one entry
  {
    const Stage E = make_stage(0, nullptr, true, 0);
    CHECK(E.items.empty() && E.blocks == 0 && E.knn_blocks == 0 && E.points == 0);
    CHECK(E.first() == std::vector<int>{0} && E.knn_first() == std::vector<int>{0});
    const int64_t dead[3] = {0, 0, 0};
    const Stage D = make_stage(3, dead, false, 0);
    CHECK(D.items.empty() && D.blocks == 0 && D.first() == std::vector<int>{0});
  }

  // ---- first-workgroup tables at 0 / 1 / 256 / 257 points, without and with the search
  {
    const int64_t sizes[4] = {0, 1, 256, 257};
    const Stage S = make_stage(4, sizes, false, 0);
    CHECK(S.items.size() == 3 && S.blocks == 4 && S.knn_blocks == 0 && S.points == 514);
    CHECK(S.items[0].scan == 1 && S.items[0].blk0 == 0 && S.items[0].blocks == 1 && S.items[0].point0 == 0);
    CHECK(S.items[1].scan == 2 && S.items[1].blk0 == 1 && S.items[1].blocks == 1 && S.items[1].point0 == 1);
    CHECK(S.items[2].scan == 3 && S.items[2].blk0 == 2 && S.items[2].blocks == 2 && S.items[2].point0 == 257);
    CHECK((S.first() == std::vector<int>{0, 1, 2, 4}));
    CHECK((S.knn_first() == std::vector<int>{0, 0, 0, 0}));         // no search in this stage
    const Stage K = make_stage(4, sizes, true, 0);
    // leaves 1 / 32 / 33, four waves per leaf, four waves per workgroup: 1 / 32 / 33 workgroups
    CHECK(K.items[0].parts == 4 && K.items[1].parts == 4 && K.items[2].parts == 4);
    CHECK(K.items[0].knn_blocks == 1 && K.items[1].knn_blocks == 32 && K.items[2].knn_blocks == 33 && K.knn_blocks == 66);
    CHECK((K.knn_first() == std::vector<int>{0, 1, 33, 66}));
    CHECK((K.first() == std::vector<int>{0, 1, 2, 4}));             // the per-point launches are the same
    const Stage O = make_stage(4, sizes, true, 2);                   // DGS_KNN_PARTS=2
    CHECK(O.items[2].parts == 2 && O.items[2].knn_blocks == 17 && (O.knn_first() == std::vector<int>{0, 1, 17, 34}));
  }

  // ---- the `parts` a scan would get alone follow its own size, whatever its neighbours
  {
    const int64_t sizes[3] = {262144, 1000, 131080};
    const Stage K = make_stage(3, sizes, true, 0);
    CHECK(K.items[0].parts == 1 && K.items[1].parts == 4 && K.items[2].parts == 2);
    CHECK(K.items[0].knn_blocks == 8192 && K.items[1].knn_blocks == 125 && K.items[2].knn_blocks == 8193);
    CHECK(K.items[1].blk0 == 1024 && K.items[2].blk0 == 1028 && K.blocks == 1028 + 513);
  }

  // ---- dead scans between live ones own nothing and shift nothing
  {
    const int64_t sizes[7] = {300, 0, 0, 5, 0, 512, 0};
    const Stage S = make_stage(7, sizes, true, 0);
    CHECK(S.items.size() == 3 && S.items[0].scan == 0 && S.items[1].scan == 3 && S.items[2].scan == 5);
    CHECK((S.first() == std::vector<int>{0, 2, 3, 5}));
    CHECK(S.items[1].point0 == 300 && S.items[2].point0 == 305 && S.points == 817);
    CHECK((S.knn_first() == std::vector<int>{0, 38, 39, 103}));     // 38 / 1 / 64 leaves
    // every workgroup of the launch falls into exactly one scan, by the bisection the kernels run
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
    CHECK(C[2].first == 4 && C[2].count == 2 && C[2].points == 500);   // above the budget: a chunk of its own (and the empty scan behind it)
    CHECK(C[3].first == 6 && C[3].count == 1 && C[3].points == 10);
    const int64_t fit[2] = {100, 200}, over[2] = {100, 201}, empties[3] = {0, 0, 0};
    CHECK(make_chunks(2, fit, 300).size() == 1);                     // exactly the budget still fits
    CHECK(make_chunks(2, over, 300).size() == 2);
    CHECK(make_chunks(3, empties, 300).size() == 1 && make_chunks(3, empties, 300)[0].count == 3);
    CHECK(make_chunks(0, nullptr, 300).empty());
    CHECK(make_chunks(7, sizes, kBatchPoints).size() == 1);
  }

  // ---- the status mapping
  CHECK(statistical_status(0, 20) == kOk);                           // an empty scan stays ok
  CHECK(statistical_status(1, 20) == kInvalidArgument && statistical_status(20, 20) == kInvalidArgument);
  CHECK(statistical_status(21, 20) == kOk);
  CHECK(statistical_status(1, 1) == kInvalidArgument && statistical_status(2, 1) == kOk);
  CHECK(radius_removes_all(0, 1) && !radius_removes_all(1, 1) && radius_removes_all(2, 3) && !radius_removes_all(3, 3));
  {
    Outputs o = output_status(10, 10, 5, 5);
    CHECK(o.status == kOk && o.copy3d && o.copy2d);
    o = output_status(0, 0, 0, 0);
    CHECK(o.status == kOk && !o.copy3d && !o.copy2d);
    o = output_status(10, 9, 5, 5);                                  // the 3-D output goes first: nothing is copied
    CHECK(o.status == kInvalidArgument && !o.copy3d && !o.copy2d);
    o = output_status(10, 10, 5, 4);                                 // the 3-D output has been written when the 2-D one fails
    CHECK(o.status == kInvalidArgument && o.copy3d && !o.copy2d);
    o = output_status(10, 10, 0, 0);
    CHECK(o.status == kOk && o.copy3d && !o.copy2d);
  }

  if (failures) return 1;
  std::printf("ok\n");
  return 0;
}
