// pcl::VoxelGrid's grid from the box of the finite points (VoxelGrid::applyFilter, VoxelGridCovariance::applyFilter), written once:
// ndt_build_target and voxel_grid_filter (ndt_voxel.hip) and voxelgrid_batch (voxel_batch.hip) call it.  No HIP in here, like seg_table.h
// and the *_plan.h headers: a CPU program can include this header and check the numbers on its own (tests/cpp/voxel_grid_plan_check.cpp).
// vgicp_build_map's grid is another rule (vgicp_coord, in double) and stays in vgicp_voxel.hip.
#pragma once
#include <cmath>
#include <cstdint>

namespace dgs {
namespace vgplan {

// kEmpty: no finite point, !(min <= max), which a NaN in the box gives as well; kTooLarge: DGS_ERR_GRID_TOO_LARGE with kTooLargeText
enum State { kEmpty, kOk, kTooLarge };
// The one spelling of upstream's error; the batch appends which cloud it was.
constexpr const char* kTooLargeText = "Leaf size is too small for the input dataset. Integer indices would overflow.";

// box: min xyz, max xyz.  The index arithmetic is in float as upstream: both ends floor(box * inv_leaf), div_b their distance + 1,
// divb_mul = (1, mul1, mul2) = (1, div0, div0 * div1).  Too large by the product of the truncated extents (upstream's test) or by the
// product of div_b (the dense cell table is indexed by it).  Nothing is written for an empty box, everything otherwise.
inline State plan(const float box[6], const float inv_leaf, int (&min_b)[3], int (&div_b)[3], int& mul1, int& mul2) {
  // the box of a cloud's finite points is empty on all axes or on none (the callers looked at x alone before); all three are asked so
  // that no NaN reaches a cast
  if (!(box[0] <= box[3] && box[1] <= box[4] && box[2] <= box[5])) return kEmpty;
  int64_t cells = 1;
  for (int a = 0; a < 3; a++) {
    min_b[a] = (int)std::floor(box[a] * inv_leaf);
    div_b[a] = (int)std::floor(box[3 + a] * inv_leaf) - min_b[a] + 1;
    cells *= (int64_t)((box[3 + a] - box[a]) * inv_leaf) + 1;
  }
  mul1 = div_b[0];
  mul2 = (int)((int64_t)div_b[0] * div_b[1]);   // fits whenever the grid is ok
  return (cells > INT32_MAX || (int64_t)div_b[0] * div_b[1] * div_b[2] > INT32_MAX) ? kTooLarge : kOk;
}

}  // namespace vgplan
}  // namespace dgs
