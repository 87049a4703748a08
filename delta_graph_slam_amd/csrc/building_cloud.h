// Host pieces of the building cloud stage (building_cloud.hip) that need no device: the table of sample positions and the checks and
// bounds made over the caller's offsets and end points before anything is launched.  Plain C++, so that a stand-alone program can
// build them under a sanitizer (tests/cpp/building_cloud_host_check.cpp).  Compile without a*b+c contraction.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

namespace dgs {
namespace bc {

constexpr int64_t kTableChunk = 4096;   // the table grows to a multiple of this many entries (81.9 m at 0.02f)

// interpolate's loop variable (ros_utils.cpp:154): i_0 = 0, i_{k+1} = fl(i_k + step).  Point k of EVERY line sits at i_k, so one table
// serves all lines and a line's point count is the number of entries <= its norm.  The sequence ends where it no longer grows
// (i_{k+1} <= i_k: 2^19 m at 0.02f, where upstream's loop never ends) or would leave the finite floats.
struct StepTable {
  float step = 0.f;
  std::vector<float> v;
  bool stalled = false;   // v's last entry is the sequence's last: fl(last + step) <= last, or not finite

  void reset(float s) {
    step = s;
    v.clear();
    stalled = false;
  }
  // Extends the table until its last entry exceeds `need`, rounded up to whole chunks, but never past max_entries entries or the stall.
  // Returns the number of entries added.
  int64_t extend(double need, int64_t max_entries) {
    const int64_t before = (int64_t)v.size();
    if (v.empty()) v.push_back(0.f);
    while (!stalled && (int64_t)v.size() < max_entries && (!((double)v.back() > need) || (int64_t)v.size() % kTableChunk != 0)) {
      const float cur = v.back();
      volatile float rounded = cur + step;   // rounded to float here, whatever the host keeps in registers
      const float next = rounded;
      if (!(next > cur) || !std::isfinite(next)) {
        stalled = true;
        break;
      }
      v.push_back(next);
    }
    return (int64_t)v.size() - before;
  }
  // entries a call with this max_points_per_line may use
  int64_t usable(int64_t max_entries) const { return std::min<int64_t>((int64_t)v.size(), max_entries); }
};

// number of entries <= norm among the first n: the points of a line of that norm (0 for NaN)
inline int64_t count_points(const float* table, int64_t n, float norm) {
  if (!(norm == norm)) return 0;
  return (int64_t)(std::upper_bound(table, table + n, norm) - table);
}

// line_offsets: n_items + 1 entries, ascending from 0.  -> the item whose offsets are wrong, or -1
inline int64_t first_bad_offset(const int64_t* line_offsets, int64_t n_items) {
  if (line_offsets[0] != 0) return 0;
  for (int64_t i = 0; i < n_items; i++)
    if (line_offsets[i + 1] < line_offsets[i]) return i;
  return -1;
}

// item of line `l` (the last item whose first line is <= l and that is not empty)
inline int64_t item_of_line(const int64_t* line_offsets, int64_t n_items, int64_t l) {
  return (int64_t)(std::upper_bound(line_offsets, line_offsets + n_items + 1, l) - line_offsets) - 1;
}

// An upper bound of the float norm the device computes for a line from a to b (doubles, cast to float first as the device does): the
// exact length of the float difference in double, a little widened.  0 when it is not finite: such a line needs no table entry (NaN
// gives no point, +inf is refused on the device).
inline double norm_bound(const double a[3], const double b[3]) {
  double s = 0.0;
  for (int c = 0; c < 3; c++) {
    const float d = (float)b[c] - (float)a[c];
    s += (double)d * (double)d;
  }
  const double len = std::sqrt(s) * (1.0 + 1e-6);
  return std::isfinite(len) ? len : 0.0;
}

}  // namespace bc
}  // namespace dgs
