// are_buildings_overlapped (upstream include/hdl_graph_slam/check_overlapping.hpp) and LineBasedScanmatcher::align_overlapped_buildings
// (src/hdl_graph_slam/line_based_scanmatcher.cpp:29-107, from the building-frame lines on), restated once for the host and the device on
// top of line_align.h.  Three sections, as there:
//   * host and device: shrinking, upstream's line intersection test, the angle gate and the arg-min order.
//   * device only: the wave arg-min.
//   * host only: bo::overlapped_pairs and bo::align_overlapped, the restatements building_overlap.hip is tested against and the CPU side
//     of scripts/bench_building_overlap.py.
// Everything is double and must not be contracted (the including file is built with -ffp-contract=off).  Only x and y take part in the
// overlap predicate.  Semantics and the deliberate non-differences from the geometric predicate: DESIGN.md 6h.
#pragma once

#include "line_align.h"

namespace dgs {
namespace bo {

constexpr double kShrinkRatio = 0.99;                        // shrink_polygon (:53)
constexpr double kMaxAngle = DGS_LA_OVERLAP_MAX_ANGLE;       // align_overlapped_buildings' max_angle = M_PI / 3.0 (:47)
enum { GATE_OVERLAP = 7 };                                   // after la::GATE_PASS .. la::GATE_RANK

struct Seg {   // the x and y of a line's two points
  double x1, y1, x2, y2;
};

// shrink_polygon (:51-70), per coordinate: center + shrink_ratio * (point - center)
LA_HD double shrink(const double p, const double c) { return c + kShrinkRatio * (p - c); }
LA_HD Seg shrink_line(const la::V3 a, const la::V3 b, const double cx, const double cy) {
  Seg s;
  s.x1 = shrink(a.x, cx); s.y1 = shrink(a.y, cy);
  s.x2 = shrink(b.x, cx); s.y2 = shrink(b.y, cy);
  return s;
}
LA_HD Seg load_seg(const double* p) { Seg s; s.x1 = p[0]; s.y1 = p[1]; s.x2 = p[2]; s.y2 = p[3]; return s; }
LA_HD void store_seg(double* p, const Seg s) { p[0] = s.x1; p[1] = s.y1; p[2] = s.x2; p[3] = s.y2; }
// is_point_on_the_line (:10-22): an OR of two half-open extents, kept as it is
LA_HD bool on_extent(const Seg l, const double x, const double y) { return ((x < l.x1) != (x < l.x2)) || ((y < l.y1) != (y < l.y2)); }
// are_lines_intersected (:24-49), operation for operation; a zero determinant (parallel or collinear lines) never intersects
LA_HD bool lines_intersected(const Seg l1, const Seg l2) {
  const double a1 = l1.y2 - l1.y1, b1 = l1.x1 - l1.x2, c1 = a1 * l1.x1 + b1 * l1.y1;
  const double a2 = l2.y2 - l2.y1, b2 = l2.x1 - l2.x2, c2 = a2 * l2.x1 + b2 * l2.y1;
  const double det = a1 * b2 - a2 * b1;
  if (det == 0.0) return false;
  const double x = (b2 * c1 - b1 * c2) / det;
  const double y = (a1 * c2 - a2 * c1) / det;
  return on_extent(l1, x, y) && on_extent(l2, x, y);
}
// the angle gate of :61 and :87: cos(angle) > cos(max_angle) passes; *tn receives translation.norm().  There is no distance gate.
LA_HD int gate_angle_only(const la::Tf t, const double cos_max_angle, const int float_chain, double* tn) {
  *tn = la::norm(la::v3(t.tx, t.ty, t.tz));
  return cos(la::gate_angle(t, float_chain)) > cos_max_angle ? (int)la::GATE_PASS : (int)la::GATE_ANGLE;
}
// upstream's running `translation.norm() < min_translation` from DBL_MAX is an arg-min: a strictly smaller norm takes over, equal
// norms go to the lower index, -1 (nothing took over, norm DBL_MAX) is the largest.  A norm that is NaN or not below DBL_MAX is no
// candidate: key() maps it to the start value.
LA_HD bool takes_under(const double tb, const int hb, const double ta, const int ha) {
  return tb < ta || (tb == ta && (unsigned)hb < (unsigned)ha);
}
LA_HD bool is_candidate(const int gate, const double tn) { return gate == la::GATE_PASS && tn < DBL_MAX; }

#if defined(__HIPCC__)
// ---- device only ---------------------------------------------------------------------------------------------------------------
// the arg-min of (norm, index) over a wavefront in takes_under's order (la::argmax_wave with <): afterwards every lane holds the winner
__device__ __forceinline__ void argmin_wave(double& best, int& bh) {
#pragma unroll
  for (int o = kWave / 2; o > 0; o >>= 1) {
    const double os = __shfl_xor(best, o, kWave);
    const int oh = __shfl_xor(bh, o, kWave);
    if (takes_under(os, oh, best, bh)) { best = os; bh = oh; }
  }
}
#endif

// ---- host only -----------------------------------------------------------------------------------------------------------------
inline std::vector<Seg> shrink_building(const std::vector<la::Line>& lines, const la::V3 c) {
  std::vector<Seg> out;
  out.reserve(lines.size());
  for (const la::Line& l : lines) out.push_back(shrink_line(l.a, l.b, c.x, c.y));
  return out;
}
// are_buildings_overlapped (:97-114) on shrunken polygons; the early return does not change the value
inline bool shrunken_overlapped(const std::vector<Seg>& a, const std::vector<Seg>& b) {
  for (const Seg& la_ : a)
    for (const Seg& lb : b)
      if (lines_intersected(la_, lb)) return true;
  return false;
}
inline bool buildings_overlapped(const std::vector<la::Line>& a, const la::V3 ca, const std::vector<la::Line>& b, const la::V3 cb) {
  return shrunken_overlapped(shrink_building(a, ca), shrink_building(b, cb));
}
// getOverlappedBuildings (apps/delta_graph_slam_nodelet.cpp:767-787): every pair i < j, i ascending, then j ascending.  A building is
// shrunk toward its own centre only, so once per building.
inline void overlapped_pairs(const std::vector<std::vector<la::Line>>& buildings, const std::vector<la::V3>& centers, std::vector<int32_t>* pairs) {
  std::vector<std::vector<Seg>> shr;
  for (size_t i = 0; i < buildings.size(); i++) shr.push_back(shrink_building(buildings[i], centers[i]));
  pairs->clear();
  for (size_t i = 0; i < shr.size(); i++)
    for (size_t j = i + 1; j < shr.size(); j++)
      if (shrunken_overlapped(shr[i], shr[j])) {
        pairs->push_back((int32_t)i);
        pairs->push_back((int32_t)j);
      }
}

struct OverlapHyp {
  int gate;   // la::GATE_PASS, la::GATE_ANGLE or GATE_OVERLAP
  la::Tf t;
  double tn;
};
struct OverlapResult {
  la::Tf t;
  double tn;                 // DBL_MAX without a winner
  long long winner, n_edge, n_line, n_angle_passed, n_not_overlapped;
  int n_edges_source, n_edges_target, is_identity;
};
// align_overlapped_buildings (:43-100) in the source building's frame.  Hypotheses in one index space: h = es * Et + et for the edge
// pairs of edge_extraction(src) x edge_extraction(trg), then Es * Et + i * Lt + j for the line pairs over the unmoved source lines.
// Every angle-passing hypothesis is tested for overlap (upstream skips the test when the norm is already no better, which only saves
// work); the source centre is not moved, as upstream.
inline void align_overlapped(const std::vector<la::Line>& src, const std::vector<la::Line>& trg, const la::V3 center_source, const la::V3 center_target,
                             const int float_chain, OverlapResult* r, std::vector<la::Line>* aligned, std::vector<OverlapHyp>* hyps) {
  std::vector<la::Edge> es, et;
  la::edge_extraction(src, es);
  la::edge_extraction(trg, et);
  const std::vector<Seg> target = shrink_building(trg, center_target);
  const double cos_max = std::cos(kMaxAngle);
  const long long n_edge = (long long)es.size() * (long long)et.size(), n_line = (long long)src.size() * (long long)trg.size();
  r->t = la::tf_identity();
  r->tn = DBL_MAX;
  r->winner = -1;
  r->n_edge = n_edge;
  r->n_line = n_line;
  r->n_angle_passed = r->n_not_overlapped = 0;
  r->n_edges_source = (int)es.size();
  r->n_edges_target = (int)et.size();
  if (hyps) hyps->clear();
  std::vector<la::Line> cand;
  for (long long h = 0; h < n_edge + n_line; h++) {
    OverlapHyp hy;
    if (h < n_edge) {
      hy.t = la::align_edges(es[(size_t)(h / (long long)et.size())], et[(size_t)(h % (long long)et.size())], nullptr);
    } else {
      const long long k = h - n_edge;
      hy.t = la::align_lines(src[(size_t)(k / (long long)trg.size())], trg[(size_t)(k % (long long)trg.size())]);
    }
    hy.gate = gate_angle_only(hy.t, cos_max, float_chain, &hy.tn);
    if (hy.gate == la::GATE_PASS) {
      r->n_angle_passed++;
      la::transform_lines(src, hy.t, &cand);
      if (shrunken_overlapped(shrink_building(cand, center_source), target)) hy.gate = GATE_OVERLAP;
      else r->n_not_overlapped++;
    }
    if (is_candidate(hy.gate, hy.tn) && hy.tn < r->tn) {   // ascending h: the first of equal norms stays
      r->t = hy.t;
      r->tn = hy.tn;
      r->winner = h;
    }
    if (hyps) hyps->push_back(hy);
  }
  if (r->winner >= 0) la::transform_lines(src, r->t, aligned);
  else *aligned = src;
  r->is_identity = la::is_identity(r->t) ? 1 : 0;
}

}  // namespace bo
}  // namespace dgs
