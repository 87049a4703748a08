// pcl::VoxelGrid's grid from a box (delta_graph_slam_amd/csrc/voxel_grid_plan.h) on its own, against numbers written out by hand and
// worked out in float32: negative and positive ends, an inverse leaf size that is not exact, the largest cube that still fits a 32-bit
// index and the first that does not, a single point, the start values of the box fold and a NaN.  No device, no library: built with
// g++ -fsanitize=address,undefined by tests/test_voxel_grid_plan_cpu.py.  Prints "ok" and exits 0, or names every failed check.
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstring>

#include "voxel_grid_plan.h"

using namespace dgs::vgplan;

static int failures = 0;
#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) {                                                         \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);        \
      failures++;                                                          \
    }                                                                      \
  } while (0)

struct Out {
  int min_b[3] = {77, 77, 77}, div_b[3] = {77, 77, 77}, mul1 = 77, mul2 = 77;   // 77: "not written"
  State state = kOk;
};
static Out run(const float (&box)[6], const float leaf) {
  Out o;
  o.state = plan(box, 1.0f / leaf, o.min_b, o.div_b, o.mul1, o.mul2);   // the inverse in float, as the callers make it
  return o;
}
static bool is3(const int (&v)[3], int a, int b, int c) { return v[0] == a && v[1] == b && v[2] == c; }
static bool untouched(const Out& o) { return is3(o.min_b, 77, 77, 77) && is3(o.div_b, 77, 77, 77) && o.mul1 == 77 && o.mul2 == 77; }

int main() {
  CHECK(std::strcmp(kTooLargeText, "Leaf size is too small for the input dataset. Integer indices would overflow.") == 0);

  {  // both signs, a flat axis, an axis that is one point: inv_leaf = 2 exactly; -2.5 floors to -3, 0.98 to 0, 1.0 to 1
    const Out o = run({-1.25f, 0.f, 0.5f, 1.0f, 0.49f, 0.5f}, 0.5f);
    CHECK(o.state == kOk);
    CHECK(is3(o.min_b, -3, 0, 1));
    CHECK(is3(o.div_b, 6, 1, 1));
    CHECK(o.mul1 == 6 && o.mul2 == 6);
  }
  {  // 1 / 0.1f is 9.99999985..., which rounds to 10.0f; 0.3f * 10.0f = 3.00000012 is a tie between 3.0f and 3.00000024f and goes to 3.0f
    CHECK(1.0f / 0.1f == 10.0f && 0.3f * 10.0f == 3.0f);
    const Out o = run({-0.3f, -0.3f, -0.3f, 0.3f, 0.3f, 0.3f}, 0.1f);
    CHECK(o.state == kOk);
    CHECK(is3(o.min_b, -3, -3, -3));
    CHECK(is3(o.div_b, 7, 7, 7));
    CHECK(o.mul1 == 7 && o.mul2 == 49);
  }
  {  // the largest cube that fits: div_b 1290 each, 1290^3 = 2,146,689,000 <= 2,147,483,647 (the truncated extents give 1289^3)
    const Out o = run({0.5f, 0.5f, 0.5f, 1289.4f, 1289.4f, 1289.4f}, 1.0f);
    CHECK(o.state == kOk);
    CHECK(is3(o.min_b, 0, 0, 0));
    CHECK(is3(o.div_b, 1290, 1290, 1290));
    CHECK(o.mul1 == 1290 && o.mul2 == 1664100);
  }
  {  // one cell more per axis: too large by the dense product alone (truncated extents 1290^3 fits, div_b gives 1291^3 = 2,151,685,171)
    const Out o = run({0.5f, 0.5f, 0.5f, 1290.4f, 1290.4f, 1290.4f}, 1.0f);
    CHECK(o.state == kTooLarge);
    CHECK(is3(o.min_b, 0, 0, 0));
    CHECK(is3(o.div_b, 1291, 1291, 1291));
    CHECK((int64_t)1290 * 1290 * 1290 <= INT32_MAX && (int64_t)1291 * 1291 * 1291 > INT32_MAX);
  }
  {  // the product of the truncated extents alone is over: 2001^3 (leaf 1), and the same cells at leaf 0.1 in a tenth of the box
    CHECK(run({0.f, 0.f, 0.f, 2000.f, 2000.f, 2000.f}, 1.0f).state == kTooLarge);
    CHECK(run({0.f, 0.f, 0.f, 200.f, 200.f, 200.f}, 0.1f).state == kTooLarge);
    CHECK(run({-1000.f, -1000.f, -1000.f, 1000.f, 1000.f, 1000.f}, 1.0f).state == kTooLarge);
    // one long axis is not too large: 100,001 x 1 x 1
    const Out o = run({0.f, 0.f, 0.f, 100000.f, 0.f, 0.f}, 1.0f);
    CHECK(o.state == kOk && is3(o.div_b, 100001, 1, 1) && o.mul1 == 100001 && o.mul2 == 100001);
  }
  {  // a single point: one cell, at any leaf; floor(1.7 * 2) = 3, floor(-2.3 * 2) = -5, floor(17.0) = 17, floor(-23.0) = -23
    const Out a = run({1.7f, -2.3f, 0.f, 1.7f, -2.3f, 0.f}, 0.5f);
    CHECK(a.state == kOk && is3(a.min_b, 3, -5, 0) && is3(a.div_b, 1, 1, 1) && a.mul1 == 1 && a.mul2 == 1);
    const Out b = run({1.7f, -2.3f, 0.f, 1.7f, -2.3f, 0.f}, 0.1f);
    CHECK(1.7f * 10.0f == 17.0f && -2.3f * 10.0f == -23.0f);
    CHECK(b.state == kOk && is3(b.min_b, 17, -23, 0) && is3(b.div_b, 1, 1, 1) && b.mul1 == 1 && b.mul2 == 1);
  }
  {  // the start values of the box fold (a cloud without a finite point): empty, nothing written
    const float leaves[4] = {0.1f, 0.5f, 1.0f, 1000.0f};
    for (const float leaf : leaves) {
      const Out o = run({FLT_MAX, FLT_MAX, FLT_MAX, -FLT_MAX, -FLT_MAX, -FLT_MAX}, leaf);
      CHECK(o.state == kEmpty && untouched(o));
    }
  }
  {  // a NaN anywhere in the box: empty, since !(min <= max); no NaN reaches a cast (UBSan would stop the program)
    const float nan = std::nanf("");
    for (int k = 0; k < 6; k++) {
      float box[6] = {-1.f, -1.f, -1.f, 1.f, 1.f, 1.f};
      box[k] = nan;
      const Out o = run(box, 0.5f);
      CHECK(o.state == kEmpty && untouched(o));
    }
    CHECK(run({nan, nan, nan, nan, nan, nan}, 0.5f).state == kEmpty);
  }
  if (failures) return 1;
  std::printf("ok\n");
  return 0;
}
