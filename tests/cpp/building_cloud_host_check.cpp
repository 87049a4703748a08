// The host-only helpers of the building cloud stage in a program of their own, for a sanitizer build (g++ -fsanitize=address,undefined):
// the table builder and the offset logic (delta_graph_slam_amd/csrc/building_cloud.h) and the adapter's matrix helper
// (include/dgs/building_cloud_hip.hpp).  Links nothing of the library.  Prints "ok" and returns 0, or says what failed.
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

#include <Eigen/Core>
#include <dgs/building_cloud_hip.hpp>

#include "building_cloud.h"

#define CHECK(cond)                                             \
  do {                                                          \
    if (!(cond)) {                                              \
      std::printf("failed at line %d: %s\n", __LINE__, #cond);  \
      return 1;                                                 \
    }                                                           \
  } while (0)

int main() {
  using namespace dgs::bc;
  // ---- the table
  StepTable t;
  t.reset(0.02f);
  CHECK(t.extend(0.0, 1 << 20) == kTableChunk && (int64_t)t.v.size() == kTableChunk && t.v[0] == 0.f && t.v[1] == 0.02f);
  CHECK(t.extend(0.0, 1 << 20) == 0);                                   // long enough already
  CHECK(t.extend(100.0, 1 << 20) == kTableChunk && t.v.back() > 100.f);
  CHECK(t.extend(1.0e9, 1 << 20) == (1 << 20) - 2 * kTableChunk && (int64_t)t.v.size() == (1 << 20) && !t.stalled);
  CHECK(t.extend(1.0e9, 1 << 20) == 0 && t.usable(64) == 64 && t.usable(1 << 21) == (1 << 20));
  for (size_t k = 1; k < t.v.size(); k++) CHECK(t.v[k] > t.v[k - 1]);   // strictly increasing over 2^20 entries
  int first = -1;
  for (int k = 0; k < 64 && first < 0; k++)
    if (t.v[k] != (float)(k * 0.02)) first = k;
  CHECK(first == 5);
  CHECK(count_points(t.v.data(), (int64_t)t.v.size(), 20.f) == 1000 && count_points(t.v.data(), (int64_t)t.v.size(), 1000.f) == 49983);
  CHECK(count_points(t.v.data(), (int64_t)t.v.size(), 100.f) == 5001 && count_points(t.v.data(), 64, 100.f) == 64);
  CHECK(count_points(t.v.data(), 64, 0.f) == 1 && count_points(t.v.data(), 64, -1.f) == 0 && count_points(t.v.data(), 64, std::nanf("")) == 0);
  CHECK(count_points(t.v.data(), 64, std::numeric_limits<float>::infinity()) == 64);
  StepTable small;   // a table that ends at max_entries below a chunk, then goes on
  small.reset(0.02f);
  CHECK(small.extend(5.0, 64) == 64 && small.extend(5.0, 64) == 0 && small.extend(0.5, 1 << 20) == kTableChunk - 64);
  for (int k = 0; k < 64; k++) CHECK(small.v[k] == t.v[k]);
  StepTable coarse;   // the second step would leave the finite floats: the sequence ends after two entries and extend() with it
  coarse.reset(3.0e38f);
  CHECK(coarse.extend(1.0e39, 1 << 20) == 2 && coarse.stalled && coarse.v[1] == 3.0e38f && coarse.extend(1.0e39, 1 << 20) == 0);
  // ---- offsets
  const int64_t off[] = {0, 0, 3, 3, 3, 7, 7};   // items 0, 2, 3 and 5 are empty
  CHECK(first_bad_offset(off, 6) == -1);
  const int64_t desc[] = {0, 4, 2}, late[] = {1, 2};
  CHECK(first_bad_offset(desc, 2) == 1 && first_bad_offset(late, 1) == 0 && first_bad_offset(off, 0) == -1);
  CHECK(item_of_line(off, 6, 0) == 1 && item_of_line(off, 6, 2) == 1 && item_of_line(off, 6, 3) == 4 && item_of_line(off, 6, 6) == 4);
  // ---- bounds
  const double a[3] = {0, 0, 0}, b[3] = {3, 4, 12}, inf[3] = {INFINITY, 0, 0}, nan[3] = {NAN, 0, 0}, huge[3] = {1e300, 0, 0};
  CHECK(norm_bound(a, b) >= 13.0 && norm_bound(a, b) < 13.0001 && norm_bound(a, a) == 0.0);
  CHECK(norm_bound(a, inf) == 0.0 && norm_bound(a, nan) == 0.0 && norm_bound(a, huge) == 0.0 && norm_bound(inf, inf) == 0.0);
  // ---- the adapter's matrix helper
  Eigen::Matrix<double, 3, 3> pose = Eigen::Matrix<double, 3, 3>::Identity(), est = pose;
  float m[16];
  dgs::building_transform16(pose, est, m);
  for (int i = 0; i < 16; i++) CHECK(m[i] == (i % 5 == 0 ? 1.f : 0.f));
  // estimate == pose: pose^-1 * pose is the identity whatever the pose, and the frame change adds t - I t = 0
  const double c = std::cos(0.3), s = std::sin(0.3);
  pose(0, 0) = c; pose(0, 1) = -s; pose(1, 0) = s; pose(1, 1) = c; pose(0, 2) = 12.5; pose(1, 2) = -7.25;
  dgs::building_transform16(pose, pose, m);
  CHECK(std::fabs(m[0] - 1.f) < 1e-6f && std::fabs(m[1]) < 1e-6f && std::fabs(m[12]) < 1e-5f && std::fabs(m[13]) < 1e-5f && m[10] == 1.f && m[15] == 1.f);
  std::printf("ok\n");
  return 0;
}
