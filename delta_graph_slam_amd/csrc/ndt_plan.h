// The launch plan of one NDT align: every scheduling decision of the host driver (ndt_align.hip), made once per align by a pure
// function and read by every launch.  Host code only, no HIP types and no environment: tests/cpp/ndt_plan_driver.cpp includes this
// file alone and checks every field against the expressions written out there.  Needs include/dgs_reg.h (the order / search enums).
#pragma once
#include <type_traits>

#include "../../include/dgs_reg.h"

namespace dgs {

// What the plan depends on: dgs_handle's knobs (DGS_NDT_* at dgs_create) and NdtConsts (dgs_params at the align); filled in one place.
struct NdtPlanIn {
  int strict_order, search_method;   // NdtConsts
  int strict_kernel;                 // dgs_handle::strict_kernel: 3 item-compacted, 2 lane-per-point
  int exp_libm, hessian_double, newton_solver;   // NdtConsts
  long long n_occupied_bound;
  bool ndt_fused, hd_overlap, has_hd_stream, ndt_speculate, ndt_fixed_slices;
  int solve_min_active;
};

struct NdtPlan {
  int order, search;   // dgs_ndt_strict_order, dgs_ndt_search
  // The item-compacted kernel (ndt_strict3_kernel) serves this handle: it carries ONE exponential, glibc's (ndt_exp_glibc = 0 and
  // DGS_NDT_STRICT_KERNEL=2 go to the lane-per-point kernels), and its queue entries hold a voxel number in 25 bits.
  bool item_kernel;
  bool two_kinds;      // upstream order, lane-per-point kernels, double computeHessian pass: kinds 0 / 1, then kind 2, two launches per round
  bool solve_beside;   // item-compacted kernel, fused: the closings' Newton steps go to ndt_strict_solve_kernel on the third stream
  bool hd_overlap;     // overlap asked for and the third stream exists
  bool speculate;      // item-compacted kernel, fused launches: speculated Newton steps, one more workgroup per pair in front of the grid
  bool fixed_slices;   // item-compacted kernel: DGS_NDT_FIXED_SLICES
  bool fused;          // the evaluation closes inside the derivative launch: per-pair "finished" flags in pinned memory, no solve launch
  int evals_factor;    // speculated steps: an evaluation whose header the exact step refuses is made again -- at most twice the launches
};

inline NdtPlan plan_align(const NdtPlanIn& in) {
  NdtPlan p;
  p.order = in.strict_order;
  p.search = in.search_method;
  const bool upstream = in.strict_order == DGS_NDT_ORDER_UPSTREAM;
  p.item_kernel = !(in.strict_kernel == 2 || !in.exp_libm) && in.n_occupied_bound < (1 << 25);
  p.two_kinds = upstream && in.hessian_double && !p.item_kernel;
  p.solve_beside = upstream && p.item_kernel && in.ndt_fused && in.solve_min_active > 0 && in.has_hd_stream;
  p.hd_overlap = in.hd_overlap && in.has_hd_stream;
  p.speculate = in.ndt_speculate && in.newton_solver && !p.solve_beside;
  p.fixed_slices = in.ndt_fixed_slices;
  p.fused = in.ndt_fused && in.strict_order != DGS_NDT_ORDER_UPSTREAM_SEQUENTIAL;
  p.evals_factor = (upstream && in.ndt_speculate) ? 2 : 1;
  return p;
}

// The one place that says which stream a derivative launch goes to (launch >= 0: fused launch number, < 0: derivatives only; hd:
// the launch for the pairs waiting for the double computeHessian pass): the third stream for the lane-per-point kernels' kind-2
// launch of a fused round with overlap, the handle's stream for everything else.
inline bool plan_on_hd_stream(const NdtPlan& p, int launch, bool hd) {
  return p.order == DGS_NDT_ORDER_UPSTREAM && !p.item_kernel && hd && launch >= 0 && p.hd_overlap;
}

// f(std::integral_constant<int, SEARCH>) for the search method of the align; unknown values run DIRECT7
template <class F>
inline void with_search(int method, F&& f) {
  switch (method) {
    case DGS_NDT_DIRECT1: f(std::integral_constant<int, DGS_NDT_DIRECT1>{}); break;
    case DGS_NDT_DIRECT26: f(std::integral_constant<int, DGS_NDT_DIRECT26>{}); break;
    case DGS_NDT_KDTREE: f(std::integral_constant<int, DGS_NDT_KDTREE>{}); break;
    default: f(std::integral_constant<int, DGS_NDT_DIRECT7>{}); break;
  }
}
template <class F>
inline void with_bool(bool b, F&& f) {
  if (b) f(std::true_type{});
  else f(std::false_type{});
}

}  // namespace dgs
