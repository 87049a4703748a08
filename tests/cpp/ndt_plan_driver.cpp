// Stand-alone check of the NDT launch plan (delta_graph_slam_amd/csrc/ndt_plan.h): the cross product of everything the plan depends on,
// each field against the expression the host driver used to write out at the place of use -- those expressions are the specification
// and are restated here literally, on the raw inputs.  Prints one JSON line; exit status 1 on the first mismatch.
#include <cstdio>
#include <initializer_list>

#include "../../delta_graph_slam_amd/csrc/ndt_plan.h"

using namespace dgs;

static long failures = 0;
#define CHECK(cond)                                                     \
  do {                                                                  \
    if (!(cond)) {                                                      \
      if (failures++ < 10) std::printf("FAIL line %d: %s\n", __LINE__, #cond); \
    }                                                                   \
  } while (0)

int main() {
  long cases = 0, stream_cases = 0, stream_disagree = 0, stream_disagree_launched = 0;
  const int orders[3] = {DGS_NDT_ORDER_FAST, DGS_NDT_ORDER_UPSTREAM, DGS_NDT_ORDER_UPSTREAM_SEQUENTIAL};
  const long long bounds[3] = {(1ll << 25) - 1, 1ll << 25, 100000};
  const int searches[5] = {DGS_NDT_KDTREE, DGS_NDT_DIRECT26, DGS_NDT_DIRECT7, DGS_NDT_DIRECT1, 17};
  for (int order : orders)
  for (int strict_kernel = 2; strict_kernel <= 3; strict_kernel++)
  for (int exp_libm = 0; exp_libm <= 1; exp_libm++)
  for (long long bound : bounds)
  for (int fused = 0; fused <= 1; fused++)
  for (int hd_param = 0; hd_param <= 1; hd_param++)
  for (int hd_overlap = 0; hd_overlap <= 1; hd_overlap++)
  for (int hd_stream = 0; hd_stream <= 1; hd_stream++)
  for (int solve_min_active : {0, 2})
  for (int speculate = 0; speculate <= 1; speculate++)
  for (int newton = 0; newton <= 1; newton++)
  for (int fixed = 0; fixed <= 1; fixed++) {
    NdtPlanIn in{};
    in.strict_order = order;
    in.search_method = searches[cases % 5];
    in.strict_kernel = strict_kernel;
    in.exp_libm = exp_libm;
    in.hessian_double = (order != DGS_NDT_ORDER_FAST && hd_param) ? 1 : 0;   // fill_consts: the fast order has no double pass
    in.newton_solver = newton;
    in.n_occupied_bound = bound;
    in.ndt_fused = fused;
    in.hd_overlap = hd_overlap;
    in.has_hd_stream = hd_stream;
    in.ndt_speculate = speculate;
    in.ndt_fixed_slices = fixed;
    in.solve_min_active = solve_min_active;
    const NdtPlan p = plan_align(in);
    cases++;

    // ---- the parent's expressions
    const int version = (strict_kernel == 2 || !exp_libm) ? 2 : 3;                                     // strict_kernel_version
    const bool item = version == 3 && bound < (1 << 25);                                               // launch_strict_sums
    const bool beside = version == 3 && bound < (1 << 25) && fused && solve_min_active > 0 && hd_stream && order == DGS_NDT_ORDER_UPSTREAM;   // strict_solve_beside
    const bool two_kinds = order == DGS_NDT_ORDER_UPSTREAM && in.hessian_double && !(version == 3 && bound < (1 << 25));
    CHECK(p.order == order && p.search == in.search_method);
    CHECK(p.item_kernel == item);
    CHECK(p.two_kinds == two_kinds);
    CHECK(p.solve_beside == beside);
    CHECK(p.hd_overlap == (hd_overlap && hd_stream));
    CHECK(p.fixed_slices == (fixed != 0));
    CHECK(p.fused == (fused && order != DGS_NDT_ORDER_UPSTREAM_SEQUENTIAL));
    CHECK(p.evals_factor == ((order == DGS_NDT_ORDER_UPSTREAM && speculate) ? 2 : 1));
    if (item) CHECK(p.speculate == (speculate && newton && !beside));   // read by the item-compacted kernel's fused launches alone
    // the two event-chained forms of a round never both apply
    CHECK(!(p.two_kinds && p.hd_overlap && p.solve_beside));

    // ---- the stream of a derivative launch: the parent's profiler stream (pst) and launch stream (lst)
    for (int launch : {-1, 0, 5})
    for (int hd = 0; hd <= 1; hd++) {
      const bool pst_hd = hd && launch >= 0 && hd_overlap && hd_stream && order == DGS_NDT_ORDER_UPSTREAM;
      // lst: the fast and the sequential order launch on the handle's stream; so does the item-compacted kernel, which makes no
      // launch at all for (hd, launch >= 0); the lane-per-point kernels go beside
      const bool launched = !(order == DGS_NDT_ORDER_UPSTREAM && item && hd && launch >= 0);
      const bool lst_hd = order == DGS_NDT_ORDER_UPSTREAM && !item && hd && launch >= 0 && hd_overlap && hd_stream;
      const bool got = plan_on_hd_stream(p, launch, hd != 0);
      stream_cases++;
      CHECK(got == lst_hd);
      if (pst_hd != lst_hd) {
        stream_disagree++;
        if (launched) stream_disagree_launched++;
        // the driver asks for (hd, launch >= 0) only with two_kinds, i.e. never where the two disagree
        CHECK(!p.two_kinds);
      } else {
        CHECK(got == pst_hd);
      }
    }
  }
  // with_search: each method reaches its own instantiation, anything else DIRECT7
  for (int m = -2; m < 8; m++) {
    int got = -100;
    with_search(m, [&](auto S) { got = decltype(S)::value; });
    const int want = (m == DGS_NDT_DIRECT1 || m == DGS_NDT_DIRECT26 || m == DGS_NDT_KDTREE) ? m : DGS_NDT_DIRECT7;
    CHECK(got == want);
  }
  for (int b = 0; b <= 1; b++) {
    int got = -1;
    with_bool(b != 0, [&](auto B) { got = decltype(B)::value ? 1 : 0; });
    CHECK(got == b);
  }
  std::printf("{\"cases\": %ld, \"stream_cases\": %ld, \"pst_lst_disagree\": %ld, \"pst_lst_disagree_launched\": %ld, \"failures\": %ld}\n", cases, stream_cases,
              stream_disagree, stream_disagree_launched, failures);
  return failures ? 1 : 0;
}
