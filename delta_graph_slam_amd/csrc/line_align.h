// LineBasedScanmatcher::align_global's and align_local's pieces (upstream src/hdl_graph_slam/line_based_scanmatcher.cpp), restated once
// for the host and the device and shared by line_align.hip and line_align_local.hip.  Three sections:
//   * host and device: the scalar functions.  The kernels, the host-side merge / edge extraction, the refinement pass and la::align_local
//     all call them, so a value computed on either side has the same bits but for the trigonometric functions.
//   * device only: the one wave scorer (fitness_wave<LOCAL>, calc_fitness_score on a wavefront) and the wave arg-max both aligners use.
//   * host only: merge / edge extraction (the pair function itself, la::edge_pair, is in the first section: line_edges.hip runs it on the
//     device), calc_fitness<LOCAL>, la::align_local, and what both drivers need around the C ABI (feature to Line, the checks, the packing
//     of the upload, the segment table of a device edge extraction).
// Everything is double and must not be contracted (the including file is built with -ffp-contract=off); the float steps are
// LineFeature::lenght() and the angle gate's transform3Dto2D chain.  Eigen details recalled from memory are tagged [UPSTREAM-RECALL];
// DESIGN.md 6f lists them.
#pragma once

#include <cfloat>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/dgs_reg.h"

#if defined(__HIPCC__)
#include "common.h"   // kWave
#define LA_HD __host__ __device__ __forceinline__
#else
#define LA_HD inline
#endif

namespace dgs {
namespace la {

struct V3 {
  double x, y, z;
};
struct Line {
  V3 a, b;
};
struct Edge {
  V3 e, a, b;   // edgePoint, pointA, pointB
};
// a planar rigid transform: the upper-left 2 x 2 of the rotation (the rest of the 4 x 4 is the identity's) and the translation
struct Tf {
  double r00, r01, r10, r11, tx, ty, tz;
};
struct Fitness {
  double real_avg_distance, avg_distance, coverage, coverage_percentage;
};
struct Pair {   // line_to_line_distance's result as nearest_neighbor keeps it
  double real, dist, cov;
};
struct Weights {
  double avg_distance_weight, coverage_weight, transform_weight, max_score_distance, max_score_translation;
};

constexpr int kTableDoubles = 9;   // a target line in the table the scorer reads: A, B, (B - A).normalized()

LA_HD V3 v3(double x, double y, double z) { V3 r; r.x = x; r.y = y; r.z = z; return r; }
LA_HD V3 load3(const double* p) { return v3(p[0], p[1], p[2]); }
LA_HD void store3(double* p, const V3 v) { p[0] = v.x; p[1] = v.y; p[2] = v.z; }
LA_HD Edge load_edge(const double* p) { Edge e; e.e = load3(p); e.a = load3(p + 3); e.b = load3(p + 6); return e; }
// the five doubles kept per hypothesis and per record: the four fitness values and the score
LA_HD void store_fit(double* o, const Fitness f, const double score) {
  o[0] = f.real_avg_distance; o[1] = f.avg_distance; o[2] = f.coverage; o[3] = f.coverage_percentage; o[4] = score;
}
LA_HD V3 pick(const bool c, const V3 a, const V3 b) { return v3(c ? a.x : b.x, c ? a.y : b.y, c ? a.z : b.z); }   // c ? a : b by component: stays in registers on the device
LA_HD V3 sub(const V3 a, const V3 b) { return v3(a.x - b.x, a.y - b.y, a.z - b.z); }
LA_HD V3 add(const V3 a, const V3 b) { return v3(a.x + b.x, a.y + b.y, a.z + b.z); }
LA_HD V3 scale(const V3 a, const double s) { return v3(a.x * s, a.y * s, a.z * s); }
// Eigen's 3-term reductions: (x + y) + z [UPSTREAM-RECALL]
LA_HD double dot(const V3 a, const V3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
LA_HD double norm(const V3 a) { return sqrt(dot(a, a)); }
// MatrixBase::normalized(): divided by sqrt(squaredNorm) when that is > 0 [UPSTREAM-RECALL]
LA_HD V3 normalized(const V3 a) {
  const double z = dot(a, a);
  if (z > 0.0) {
    const double s = sqrt(z);
    return v3(a.x / s, a.y / s, a.z / s);
  }
  return a;
}
LA_HD float lenght(const V3 a, const V3 b) { return (float)norm(sub(a, b)); }   // LineFeature::lenght() returns float

LA_HD Tf tf_identity() { Tf t; t.r00 = 1.0; t.r01 = 0.0; t.r10 = 0.0; t.r11 = 1.0; t.tx = t.ty = t.tz = 0.0; return t; }
// Matrix3d * Vector3d with rows (r00 r01 0), (r10 r11 0), (0 0 1): ((m0 x + m1 y) + m2 z)
LA_HD V3 rotate(const Tf t, const V3 p) { return v3((t.r00 * p.x + t.r01 * p.y) + 0.0 * p.z, (t.r10 * p.x + t.r11 * p.y) + 0.0 * p.z, (0.0 * p.x + 0.0 * p.y) + 1.0 * p.z); }
// transform_lines (:985-1010): the last column of T * [I | p], (((m0 x + m1 y) + m2 z) + m3 * 1).  The third term is +-0 for every
// planar transform, so Eigen's other association ((m0 x + m1 y) + (m2 z + m3)) gives the same bits [UPSTREAM-RECALL].
LA_HD V3 apply(const Tf t, const V3 p) {
  return v3(((t.r00 * p.x + t.r01 * p.y) + 0.0 * p.z) + t.tx, ((t.r10 * p.x + t.r11 * p.y) + 0.0 * p.z) + t.ty, ((0.0 * p.x + 0.0 * p.y) + 1.0 * p.z) + t.tz);
}
// AngleAxisd(0, X) * AngleAxisd(0, Y) * AngleAxisd(angle, Z): the quaternion product (1,0,0,0) * (1,0,0,0) * (cos(a/2), 0, 0, sin(a/2)),
// exact, then Quaternion::toRotationMatrix() -- not cos / sin of the angle itself [UPSTREAM-RECALL]
LA_HD Tf rot_z(const double angle) {
  const double ha = 0.5 * angle;
  const double w = cos(ha), z = sin(ha);
  const double tz = 2.0 * z, twz = tz * w, tzz = tz * z;
  Tf t = tf_identity();
  t.r00 = 1.0 - (0.0 + tzz);
  t.r01 = 0.0 - twz;
  t.r10 = 0.0 + twz;
  t.r11 = 1.0 - (0.0 + tzz);
  return t;
}
// best_trans * transform of two planar 4 x 4 matrices (:196), every entry (((a0 b0 + a1 b1) + a2 b2) + a3 b3) with its zero terms
LA_HD Tf compose(const Tf a, const Tf b) {
  Tf r;
  r.r00 = ((a.r00 * b.r00 + a.r01 * b.r10) + 0.0) + 0.0;
  r.r01 = ((a.r00 * b.r01 + a.r01 * b.r11) + 0.0) + 0.0;
  r.r10 = ((a.r10 * b.r00 + a.r11 * b.r10) + 0.0) + 0.0;
  r.r11 = ((a.r10 * b.r01 + a.r11 * b.r11) + 0.0) + 0.0;
  r.tx = ((a.r00 * b.tx + a.r01 * b.ty) + 0.0 * b.tz) + a.tx;
  r.ty = ((a.r10 * b.tx + a.r11 * b.ty) + 0.0 * b.tz) + a.ty;
  r.tz = ((0.0 * b.tx + 0.0 * b.ty) + 1.0 * b.tz) + a.tz;
  return r;
}

// lines_intersection (:473-499); the parallel case yields DBL_MAX coordinates (and does not print)
LA_HD V3 lines_intersection(const V3 p1a, const V3 p1b, const V3 p2a, const V3 p2b) {
  const double a1 = p1b.y - p1a.y, b1 = p1a.x - p1b.x, c1 = a1 * p1a.x + b1 * p1a.y;
  const double a2 = p2b.y - p2a.y, b2 = p2a.x - p2b.x, c2 = a2 * p2a.x + b2 * p2a.y;
  const double det = a1 * b2 - a2 * b1;
  if (det != 0.0) return v3((b2 * c1 - b1 * c2) / det, (a1 * c2 - a2 * c1) / det, 0.0);
  return v3(DBL_MAX, DBL_MAX, 0.0);
}
// is_point_on_line (:800-809)
LA_HD bool is_point_on_line(const V3 p, const V3 a, const V3 b) {
  const double dot1 = dot(sub(p, a), sub(b, a));
  const double dot2 = dot(sub(p, b), sub(a, b));
  return dot1 >= 0.0 && dot2 >= 0.0;
}
// point_to_line_distance, the segment form (:776-798); `d` is (B - A).normalized().  Upstream falls off the end when a dot product is
// NaN; that case returns NaN here.
LA_HD double point_to_segment(const V3 p, const V3 a, const V3 b, const V3 d) {
  const V3 proj = add(a, scale(d, dot(sub(p, a), d)));
  const double dot1 = dot(sub(proj, a), sub(b, a));
  const double dot2 = dot(sub(proj, b), sub(a, b));
  if (dot1 >= 0.0 && dot2 >= 0.0) return norm(sub(p, proj));
  if (dot1 < 0.0) return norm(sub(p, a));
  if (dot2 < 0.0) return norm(sub(p, b));
  return NAN;
}
// line_to_line_distance (:811-903): source (sa, sb) of float length slen, target (ta, tb) with d = (tb - ta).normalized()
LA_HD Pair line_to_line(const V3 sa, const V3 sb, const float slen, const V3 ta, const V3 tb, const V3 d) {
  Pair r;
  double real = 0.0;
  real += point_to_segment(sa, ta, tb, d);
  real += point_to_segment(sb, ta, tb, d);
  r.real = real / 2.0;
  double distance1 = 0.0, distance2 = 0.0;
  V3 point1 = v3(0.0, 0.0, 0.0);
  bool found = false;
  V3 proj = add(ta, scale(d, dot(sub(sa, ta), d)));
  if (is_point_on_line(proj, ta, tb)) {
    point1 = sa;
    distance1 = norm(sub(sa, proj));
    found = true;
  }
  proj = add(ta, scale(d, dot(sub(sb, ta), d)));
  if (is_point_on_line(proj, ta, tb)) {
    if (!found) {
      point1 = sb;
      distance1 = norm(sub(sb, proj));
      found = true;
    } else {
      distance2 = norm(sub(sb, proj));
      r.dist = (distance1 + distance2) / 2.0;
      r.cov = norm(sub(sb, point1));
      return r;
    }
  }
  const V3 f = v3(d.y, -d.x, d.z);   // the direction turned by 90 degrees
  proj = lines_intersection(sa, sb, ta, add(ta, f));
  if (is_point_on_line(proj, sa, sb)) {
    if (!found) {
      point1 = proj;
      distance1 = norm(sub(ta, proj));
      found = true;
    } else {
      distance2 = norm(sub(ta, proj));
      r.dist = (distance1 + distance2) / 2.0;
      r.cov = norm(sub(proj, point1));
      return r;
    }
  }
  proj = lines_intersection(sa, sb, tb, add(tb, f));
  if (is_point_on_line(proj, sa, sb)) {
    if (found) {
      distance2 = norm(sub(tb, proj));
      r.dist = (distance1 + distance2) / 2.0;
      r.cov = norm(sub(proj, point1));
      return r;
    }
  }
  (void)slen;   // coverage_percentage = coverage / lenght() is computed upstream and never read by nearest_neighbor
  r.dist = DBL_MAX;
  r.cov = 0.0;
  return r;
}
// nearest_neighbor's order (:975-980): the smallest real_distance; equal ones go to the lowest (tie_highest: highest) target index
// [UPSTREAM-RECALL: std::sort is an insertion sort below 16 elements].  A NaN distance compares like +infinity.
LA_HD bool nn_better(const double key_b, const int jb, const double key_a, const int ja, const int tie_highest) {
  if (ja < 0) return jb >= 0;
  if (jb < 0) return false;
  if (key_b < key_a) return true;
  if (key_b > key_a) return false;
  return tie_highest ? jb > ja : jb < ja;
}
LA_HD double nn_key(const double real) { return real != real ? (double)INFINITY : real; }

// calc_fitness_score's running sums (:905-955).  LOCAL is upstream's is_local, and the comparison (:925) is all it selects: the global
// search takes a neighbour whose real_distance < max_range, the local one a neighbour whose distance < max_range.  A neighbour without
// coverage has distance DBL_MAX, so the local rule leaves it out of the four sums however small its real_distance; total_lenght always grows.
struct Sums {
  double real_distance, real_distance_lenght, distance, coverage_lenght, total_lenght;
};
LA_HD Sums sums_zero() { Sums s; s.real_distance = s.real_distance_lenght = s.distance = s.coverage_lenght = s.total_lenght = 0.0; return s; }
template <bool LOCAL>
LA_HD void sums_add(Sums& s, const bool has_nn, const Pair nn, const float slen, const double max_range) {
  if (has_nn && (LOCAL ? nn.dist : nn.real) < max_range) {
    s.real_distance += nn.real * (double)slen;
    s.real_distance_lenght += (double)slen;
    s.distance += nn.dist * nn.cov;
    s.coverage_lenght += nn.cov;
  }
  s.total_lenght += (double)slen;
}
LA_HD Fitness sums_finish(const Sums s) {
  Fitness f;
  f.coverage = s.coverage_lenght;
  f.real_avg_distance = s.real_distance_lenght > 0.0 ? s.real_distance / s.real_distance_lenght : DBL_MAX;
  f.avg_distance = s.coverage_lenght > 0.0 ? s.distance / s.coverage_lenght : DBL_MAX;
  f.coverage_percentage = s.total_lenght > 0.0 ? s.coverage_lenght / s.total_lenght * 100.0 : 0.0;
  return f;
}
LA_HD double min_std(const double a, const double b) { return b < a ? b : a; }   // std::min(a, b)
// weight_global and weight_local (line_based_scanmatcher.hpp:155-166) are this one expression: the global search passes its g_* members
// and real_avg_distance, the local one its l_* members and avg_distance
LA_HD double weight(const Weights w, const double avg_distance, const double coverage_percentage, const double translation_distance) {
  return -w.avg_distance_weight * (min_std(w.max_score_distance, avg_distance) / w.max_score_distance) * 100. + w.coverage_weight * coverage_percentage -
         w.transform_weight * (min_std(w.max_score_translation, translation_distance) / w.max_score_translation) * 100.;
}

// angle_between_vectors (:684-691)
LA_HD double angle_between(const V3 a, const V3 b) {
  const double dt = a.x * b.x + a.y * b.y;
  const double det = a.x * b.y - a.y * b.x;
  return atan2(det, dt);
}
// align_edges (:693-740); *used_rot1 says which of the two rotations was taken
LA_HD Tf align_edges(const Edge e1, const Edge e2, int* used_rot1) {
  const V3 side1A = sub(e1.a, e1.e), side1B = sub(e1.b, e1.e);
  V3 side2A = sub(e2.a, e2.e), side2B = sub(e2.b, e2.e);
  if (norm(side2A) < norm(side2B)) {
    const V3 t = side2A;
    side2A = side2B;
    side2B = t;
  }
  const double angle1 = angle_between(side1A, side2A);
  const double angle2 = angle_between(side1B, side2A);
  const Tf rot1 = rot_z(angle1), rot2 = rot_z(angle2);
  const double angle3 = angle_between(rotate(rot1, side1B), side2B);
  const double angle4 = angle_between(rotate(rot2, side1A), side2B);
  const bool first = fabs(angle3) < fabs(angle4);
  Tf t = first ? rot1 : rot2;
  const V3 tr = sub(e2.e, rotate(t, e1.e));
  t.tx = tr.x; t.ty = tr.y; t.tz = tr.z;
  if (used_rot1) *used_rot1 = first ? 1 : 0;
  return t;
}
// align_lines (:742-767)
LA_HD Tf align_lines(const Line l1, const Line l2) {
  double angle = angle_between(sub(l1.a, l1.b), sub(l2.a, l2.b));
  if (angle > M_PI / 2) angle -= M_PI;
  else if (angle < -M_PI / 2) angle += M_PI;
  const V3 d = normalized(sub(l2.a, l2.b));
  const V3 proj = add(l2.a, scale(d, dot(sub(l1.a, l2.a), d)));
  Tf t = rot_z(angle);
  const V3 tr = sub(proj, rotate(t, l1.a));
  t.tx = tr.x; t.ty = tr.y; t.tz = tr.z;
  return t;
}
LA_HD bool is_identity(const Tf t) { return t.r00 == 1.0 && t.r01 == 0.0 && t.r10 == 0.0 && t.r11 == 1.0 && t.tx == 0.0 && t.ty == 0.0 && t.tz == 0.0; }

// The angle gate's Rotation2Dd(transform3Dto2D(transform.cast<float>()).cast<double>().block<2,2>(0,0)).angle() (:139; ros_utils.cpp:95-144),
// the one place where the chain is restated [UPSTREAM-RECALL: Eigen 3.3's Quaternionf(Matrix3f), toRotationMatrix, eulerAngles(0,1,2),
// Rotation2D::fromRotationMatrix].  float_chain = 0 takes atan2(r10, r00) in double instead.
LA_HD double gate_angle(const Tf t, const int float_chain) {
  if (!float_chain) return atan2(t.r10, t.r00);
  const float m00 = (float)t.r00, m01 = (float)t.r01, m10 = (float)t.r10, m11 = (float)t.r11, m22 = 1.f;
  // Quaternionf(rotation matrix): x = y = 0 for a rotation about z
  float tr = (m00 + m11) + m22, qw, qz;
  if (tr > 0.f) {
    tr = sqrtf(tr + 1.f);
    qw = 0.5f * tr;
    tr = 0.5f / tr;
    qz = (m10 - m01) * tr;
  } else {   // m00 + m11 <= -1 < m22: the branch of the largest diagonal entry, i = 2
    tr = sqrtf(((m22 - m00) - m11) + 1.f);
    qz = 0.5f * tr;
    tr = 0.5f / tr;
    qw = (m10 - m01) * tr;
  }
  // toRotationMatrix()
  const float tz = 2.f * qz, twz = tz * qw, tzz = tz * qz;
  const float n00 = 1.f - (0.f + tzz), n01 = 0.f - twz, n10 = 0.f + twz, n11 = 1.f - (0.f + tzz);
  const float n02 = 0.f, n12 = 0.f, n20 = 0.f, n21 = 0.f, n22 = 1.f;
  // eulerAngles(0, 1, 2): odd = 0, i = 0, j = 1, k = 2
  float e0 = atan2f(n12, n22);
  const float c2 = sqrtf(n00 * n00 + n01 * n01);
  float e1;
  if (e0 > 0.f) {
    e0 -= (float)M_PI;
    e1 = atan2f(-n02, -c2);
  } else {
    e1 = atan2f(-n02, c2);
  }
  const float s1 = sinf(e0), c1 = cosf(e0);
  float e2 = atan2f(s1 * n20 - c1 * n10, c1 * n11 - s1 * n21);
  e0 = -e0; e1 = -e1; e2 = -e2;
  // normalize_euler_angs: float - double -> rounded to float
  const float g0 = (float)((double)e0 - M_PI * (e0 >= .0f ? 1 : -1));
  const float g1 = (float)((double)e1 - M_PI * (e1 >= .0f ? 1 : -1));
  const float g2 = (float)((double)e2 - M_PI * (e2 >= .0f ? 1 : -1));
  const float nn = sqrtf((g0 * g0 + g1 * g1) + g2 * g2), no = sqrtf((e0 * e0 + e1 * e1) + e2 * e2);
  const float yaw = nn < no ? g2 : e2;
  // Rotation2Df(yaw).toRotationMatrix() -> double -> Rotation2Dd(matrix).angle()
  const float s = sinf(yaw), c = cosf(yaw);
  return atan2((double)s, (double)c);
}

enum { GATE_PASS = 0, GATE_DISTANCE = 1, GATE_IDENTITY = 2, GATE_ANGLE = 3 };
// the three gates of :133-143 in upstream's order; *tn receives translation.norm()
LA_HD int gate(const Tf t, const double max_distance, const int constrain_angle, const double cos_max_angle, const int float_chain, double* tn) {
  *tn = norm(v3(t.tx, t.ty, t.tz));
  if (*tn > max_distance) return GATE_DISTANCE;
  if (is_identity(t)) return GATE_IDENTITY;
  if (constrain_angle && cos(gate_angle(t, float_chain)) < cos_max_angle) return GATE_ANGLE;
  return GATE_PASS;
}

// ---- align_local (:205-297) ----------------------------------------------------------------------------------------------------------
// GATE_LINE_*: the two gates of the line-pair phase (:270-280); GATE_RANK: a neighbour rank the walk does not visit (refine_three_nearest)
enum { GATE_LINE_DIRECTION = 4, GATE_LINE_DISTANCE = 5, GATE_RANK = 6 };
// the edge-pair phase's gates (:227-235) in upstream's order: the distance, then always the angle; there is no identity gate
LA_HD int gate_local(const Tf t, const double max_distance, const double cos_max_angle, const int float_chain, double* tn) {
  *tn = norm(v3(t.tx, t.ty, t.tz));
  if (*tn > max_distance) return GATE_DISTANCE;
  if (cos(gate_angle(t, float_chain)) < cos_max_angle) return GATE_ANGLE;
  return GATE_PASS;
}
// one line-pair hypothesis (:267-280): the direction gate, align_lines, the distance gate.  A gated hypothesis keeps the identity.
LA_HD int line_hypothesis(const Line ls, const Line lt, const double max_distance, const double cos_max_angle, Tf* t, double* tn) {
  *t = tf_identity();
  *tn = 0.0;
  const double cosine = dot(normalized(sub(ls.a, ls.b)), normalized(sub(lt.a, lt.b)));
  if (fabs(cosine) < cos_max_angle) return GATE_LINE_DIRECTION;
  *t = align_lines(ls, lt);
  *tn = norm(v3(t->tx, t->ty, t->tz));
  if (*tn > max_distance) return GATE_LINE_DISTANCE;
  return GATE_PASS;
}
// the neighbour order of the line-pair phase: all target lines by (nn_key(real_distance), target index), the index order flipped under
// tie_highest.  std::sort's order among equal keys above 16 elements is unspecified upstream; this is the project's definition.
LA_HD bool rank_before(const double key_a, const int ja, const double key_b, const int jb, const int tie_highest) {
  if (key_a < key_b) return true;
  if (key_a > key_b) return false;
  return tie_highest ? ja > jb : ja < jb;
}
// arg-max order: a strictly greater score takes over, equal scores go to the lower index, -1 (nothing took over) is the largest; NaN never wins
LA_HD bool takes_over(const double sb, const int hb, const double sa, const int ha) {
  return sb > sa || (sb == sa && (unsigned)hb < (unsigned)ha);
}

// get_edges (:501-682) of one pair of lines, for the host and for the device (line_edges.hip): up to four edges in the order of the four
// cases; returns how many.  EMIT = false only counts (`out` is not touched); EMIT = true writes at most `cap` edges (the device's emit
// pass hands in the count it stored for the pair, so a write can never pass the pair's own room).  only_angular_edges drops an edge whose lines end further
// than max_dist_angular_edge from the corner (cases 1, 2 and 3; case 4 has no such check upstream).  Only + - * /, sqrt, comparisons and
// fmin / fmax of ordered values: without contraction both sides produce the same bits.
template <bool EMIT>
LA_HD int edge_pair(const Line l1, const Line l2, const bool only_angular_edges, const double max_dist_angular_edge, Edge* out, const int cap) {
  const double cosine = dot(normalized(sub(l1.a, l1.b)), normalized(sub(l2.a, l2.b)));
  if (fabs(cosine) > 0.5) return 0;
  const double min_side = 1.0;
  const V3 ep = lines_intersection(l1.a, l1.b, l2.a, l2.b);
  const V3 s1a = sub(l1.a, ep), s1b = sub(l1.b, ep), s2a = sub(l2.a, ep), s2b = sub(l2.b, ep);
  const double n1a = norm(s1a), n1b = norm(s1b), n2a = norm(s2a), n2b = norm(s2b);
  const bool same1 = n1a < 0.01 || n1b < 0.01 || norm(sub(normalized(s1a), normalized(s1b))) < 1.;
  const bool same2 = n2a < 0.01 || n2b < 0.01 || norm(sub(normalized(s2a), normalized(s2b))) < 1.;
  int n = 0;
  Edge e;
  e.e = ep;
#define LA_EMIT_EDGE()        \
  do {                        \
    if (EMIT && n < cap) {    \
      out[n].e = e.e;         \
      out[n].a = e.a;         \
      out[n].b = e.b;         \
    }                         \
    n++;                      \
  } while (0)
  if (same1 && same2) {
    if (fmax(n1a, n1b) < min_side || fmax(n2a, n2b) < min_side) return 0;
    if (only_angular_edges && (fmin(n1a, n1b) > max_dist_angular_edge || fmin(n2a, n2b) > max_dist_angular_edge)) return 0;
    e.a = pick(n1a > n1b, l1.a, l1.b);
    e.b = pick(n2a > n2b, l2.a, l2.b);
    LA_EMIT_EDGE();
  } else if (same1 && !same2) {
    if (fmax(n1a, n1b) < min_side) return 0;
    if (only_angular_edges && fmin(n1a, n1b) > max_dist_angular_edge) return 0;
    e.a = pick(n1a > n1b, l1.a, l1.b);
    if (n2a > min_side) { e.b = l2.a; LA_EMIT_EDGE(); }
    if (n2b > min_side) { e.b = l2.b; LA_EMIT_EDGE(); }
  } else if (!same1 && same2) {
    if (fmax(n2a, n2b) < min_side) return 0;
    if (only_angular_edges && fmin(n2a, n2b) > max_dist_angular_edge) return 0;
    e.a = pick(n1a > n1b, l2.a, l2.b);   // upstream compares side1A with side1B here and takes the point from line2
    if (n1a > min_side) { e.b = l1.a; LA_EMIT_EDGE(); }
    if (n1b > min_side) { e.b = l1.b; LA_EMIT_EDGE(); }
  } else {
    if (n1a > min_side) {
      e.a = l1.a;
      if (n2a > min_side) { e.b = l2.a; LA_EMIT_EDGE(); }
      if (n2b > min_side) { e.b = l2.b; LA_EMIT_EDGE(); }
    }
    if (n1b > min_side) {
      e.a = l1.b;
      if (n2a > min_side) { e.b = l2.a; LA_EMIT_EDGE(); }
      if (n2b > min_side) { e.b = l2.b; LA_EMIT_EDGE(); }
    }
  }
#undef LA_EMIT_EDGE
  return n;
}

#if defined(__HIPCC__)
// ---- device only ---------------------------------------------------------------------------------------------------------------
// calc_fitness_score (:905-955) of `Ls` lines, moved by `t` or as they are, against the `Lt` rows of the target table in LDS, by one
// wavefront: lanes stride over the target lines, the arg-min of (real_distance, index) per source line is a butterfly of cross-lane
// shuffles, the owner lane's record is broadcast and the five sums are added in source order by every lane alike, so their association
// is upstream's whatever the launch shape.  Every lane returns the same value.
template <bool LOCAL>
__device__ __forceinline__ Fitness fitness_wave(const double* __restrict__ lines, const int Ls, const bool move, const Tf t, const double* s_t,
                                                const int Lt, const int lane, const int tie_highest, const double max_range) {
  Sums sums = sums_zero();
  for (int i = 0; i < Ls; i++) {
    V3 sa = load3(lines + 6 * i), sb = load3(lines + 6 * i + 3);
    if (move) {
      sa = apply(t, sa);
      sb = apply(t, sb);
    }
    const float sl = lenght(sa, sb);
    int bj = -1;
    double bkey = 0.0;
    Pair bp;
    bp.real = bp.dist = bp.cov = 0.0;
    for (int j = lane; j < Lt; j += kWave) {
      const double* tt = s_t + j * kTableDoubles;
      const Pair p = line_to_line(sa, sb, sl, load3(tt), load3(tt + 3), load3(tt + 6));
      const double key = nn_key(p.real);
      if (nn_better(key, j, bkey, bj, tie_highest)) {
        bj = j;
        bkey = key;
        bp = p;
      }
    }
    // arg-min of (key, index) over the wave: after the butterfly every lane holds the winner
    int wj = bj;
    double wkey = bkey;
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) {
      const int oj = __shfl_xor(wj, o, kWave);
      const double okey = __shfl_xor(wkey, o, kWave);
      if (nn_better(okey, oj, wkey, wj, tie_highest)) {
        wj = oj;
        wkey = okey;
      }
    }
    Pair nn;
    nn.real = nn.dist = nn.cov = 0.0;
    if (wj >= 0) {   // the lane that owns target wj holds its record as its own best
      const int owner = wj & (kWave - 1);
      nn.real = __shfl(bp.real, owner, kWave);
      nn.dist = __shfl(bp.dist, owner, kWave);
      nn.cov = __shfl(bp.cov, owner, kWave);
    }
    sums_add<LOCAL>(sums, wj >= 0, nn, sl, max_range);
  }
  return sums_finish(sums);
}
// the arg-max of (score, index) over a wavefront in takes_over's order: afterwards every lane holds the winner
__device__ __forceinline__ void argmax_wave(double& best, int& bh) {
#pragma unroll
  for (int o = kWave / 2; o > 0; o >>= 1) {
    const double os = __shfl_xor(best, o, kWave);
    const int oh = __shfl_xor(bh, o, kWave);
    if (takes_over(os, oh, best, bh)) { best = os; bh = oh; }
  }
}
#endif

// ---- host only -----------------------------------------------------------------------------------------------------------------
// are_lines_aligned (:1012-1084): 0 = no merge, 1 = line1 stays (identical lines), 2 = *merged
inline int are_lines_aligned(const Line l1, const Line l2, Line* merged) {
  const double cosine = dot(normalized(sub(l1.a, l1.b)), normalized(sub(l2.a, l2.b)));
  if (fabs(cosine) < 0.9995) return 0;
  const double thr = 0.3;
  const double aa = norm(sub(l1.a, l2.a)), bb = norm(sub(l1.b, l2.b)), ab = norm(sub(l1.a, l2.b)), ba = norm(sub(l1.b, l2.a));
  if ((aa < thr && bb < thr) || (ab < thr && ba < thr)) return 1;
  if (aa < thr) {
    if (is_point_on_line(l1.b, l2.a, l2.b) || is_point_on_line(l2.b, l1.a, l1.b)) return 0;
    merged->a = l1.b; merged->b = l2.b;
    return 2;
  } else if (ab < thr) {
    if (is_point_on_line(l1.b, l2.a, l2.b) || is_point_on_line(l2.a, l1.a, l1.b)) return 0;
    merged->a = l1.b; merged->b = l2.a;
    return 2;
  } else if (ba < thr) {
    if (is_point_on_line(l1.a, l2.a, l2.b) || is_point_on_line(l2.b, l1.a, l1.b)) return 0;
    merged->a = l1.a; merged->b = l2.b;
    return 2;
  } else if (bb < thr) {
    if (is_point_on_line(l1.a, l2.a, l2.b) || is_point_on_line(l2.a, l1.a, l1.b)) return 0;
    merged->a = l1.a; merged->b = l2.a;
    return 2;
  }
  return 0;
}
// merge_lines (:1086-1103): erase, i-- and break as upstream; `fresh[i]` marks a line that merging created (its statistics are not set)
inline void merge_lines(std::vector<Line>& lines, std::vector<int>& origin) {
  for (int i = 0; i < (int)lines.size(); i++) {
    for (int j = i + 1; j < (int)lines.size(); j++) {
      Line m;
      const int k = are_lines_aligned(lines[(size_t)i], lines[(size_t)j], &m);
      if (k) {
        lines.erase(lines.begin() + j);
        origin.erase(origin.begin() + j);
        if (k == 2) {
          lines[(size_t)i] = m;
          origin[(size_t)i] = -1;
        }
        i--;
        break;
      }
    }
  }
}
// get_edges on the host: edge_pair's edges appended to `out`.  The defaults are align_global's call.
inline void get_edges(const Line l1, const Line l2, std::vector<Edge>& out, const bool only_angular_edges = false,
                      const double max_dist_angular_edge = 7.0) {
  Edge e[4];
  const int n = edge_pair<true>(l1, l2, only_angular_edges, max_dist_angular_edge, e, 4);
  out.insert(out.end(), e, e + n);
}
// edge_extraction (:459-471); fewer than two lines give no edges (upstream's unsigned `size() - 1` reads out of bounds there)
inline void edge_extraction(const std::vector<Line>& lines, std::vector<Edge>& out, const bool only_angular_edges = false,
                            const double max_dist_angular_edge = 7.0) {
  const int n = (int)lines.size();
  for (int i = 0; i + 1 < n; i++)
    for (int j = i + 1; j < n; j++) get_edges(lines[(size_t)i], lines[(size_t)j], out, only_angular_edges, max_dist_angular_edge);
}
// nearest_neighbor's first entry: index of the nearest target (-1: none) and its record
inline int nearest(const V3 sa, const V3 sb, const std::vector<Line>& trg, const std::vector<V3>& dir, const int tie_highest, Pair* out) {
  int best = -1;
  double key = 0.0;
  const float sl = lenght(sa, sb);
  for (int j = 0; j < (int)trg.size(); j++) {
    const Pair p = line_to_line(sa, sb, sl, trg[(size_t)j].a, trg[(size_t)j].b, dir[(size_t)j]);
    if (nn_better(nn_key(p.real), j, key, best, tie_highest)) {
      best = j;
      key = nn_key(p.real);
      *out = p;
    }
  }
  return best;
}
// calc_fitness_score(is_local = LOCAL): what fitness_wave<LOCAL> computes on the device
template <bool LOCAL>
inline Fitness calc_fitness(const std::vector<Line>& src, const std::vector<Line>& trg, const std::vector<V3>& dir, const double max_range,
                            const int tie_highest) {
  Sums s = sums_zero();
  for (const Line& l : src) {
    Pair nn;
    nn.real = nn.dist = nn.cov = 0.0;
    const int j = nearest(l.a, l.b, trg, dir, tie_highest, &nn);
    sums_add<LOCAL>(s, j >= 0, nn, lenght(l.a, l.b), max_range);
  }
  return sums_finish(s);
}
inline void transform_lines(const std::vector<Line>& in, const Tf t, std::vector<Line>* out) {
  out->resize(in.size());
  for (size_t k = 0; k < in.size(); k++) {
    (*out)[k].a = apply(t, in[k].a);
    (*out)[k].b = apply(t, in[k].b);
  }
}
// the target table's third column
inline std::vector<V3> directions(const std::vector<Line>& trg) {
  std::vector<V3> dir;
  for (const Line& l : trg) dir.push_back(normalized(sub(l.b, l.a)));
  return dir;
}

// ---- host only, around the C ABI (include/dgs_reg.h): what dgs_line_align_global and dgs_line_align_local_batch both do
inline std::vector<Line> lines_of(const dgs_line_feature* f, const int64_t n) {
  std::vector<Line> out((size_t)n);
  for (int64_t i = 0; i < n; i++) {
    out[(size_t)i].a = load3(f[i].point_a);
    out[(size_t)i].b = load3(f[i].point_b);
  }
  return out;
}
inline bool all_finite(const dgs_line_feature* l, const int64_t n) {
  for (int64_t i = 0; i < n; i++)
    for (int a = 0; a < 3; a++)
      if (!std::isfinite(l[i].point_a[a]) || !std::isfinite(l[i].point_b[a])) return false;
  return true;
}
// edges_on_device of a struct that has the member (it took the place of `reserved2`, which dgs_line_align_params_init zeroes); the
// short struct is the host path
inline bool edges_on_device(const dgs_line_align_params* p) { return p->struct_size >= sizeof(dgs_line_align_params) && p->edges_on_device != 0; }
// what is wrong with the struct itself (nullptr: nothing): it ends before align_local's members were appended, or it is the whole of it
inline const char* params_guard(const dgs_line_align_params* p) {
  if (!p) return "line align: params is NULL";
  if (p->struct_size != offsetof(dgs_line_align_params, l_avg_distance_weight) && p->struct_size != sizeof(dgs_line_align_params))
    return "line align: wrong struct_size";
  return nullptr;
}
// the upload: 6 doubles per line, kTableDoubles per target line, 9 per edge; each returns the end of what it wrote
inline double* pack_lines(const std::vector<Line>& lines, double* o) {
  for (const Line& l : lines) { store3(o, l.a); store3(o + 3, l.b); o += 6; }
  return o;
}
inline double* pack_target_table(const std::vector<Line>& trg, const std::vector<V3>& dir, double* o) {
  for (size_t j = 0; j < trg.size(); j++) { store3(o, trg[j].a); store3(o + 3, trg[j].b); store3(o + 6, dir[j]); o += kTableDoubles; }
  return o;
}
inline double* pack_edges(const std::vector<Edge>& edges, double* o) {
  for (const Edge& e : edges) { store3(o, e.e); store3(o + 3, e.a); store3(o + 6, e.b); o += 9; }
  return o;
}
// the 4 x 4 row-major matrix of a planar transform
inline void matrix(const Tf t, double* T) {
  const double m[16] = {t.r00, t.r01, 0.0, t.tx, t.r10, t.r11, 0.0, t.ty, 0.0, 0.0, 1.0, t.tz, 0.0, 0.0, 0.0, 1.0};
  std::memcpy(T, m, sizeof(m));
}

// ---- the batched device edge extraction (line_edges.hip): what its callers hand it
}  // namespace la
// One segment: `n` lines from line `line_off` of the packed lines on.  Its pairs are indexed p = pair_off + i * n + j over the full square
// (j <= i yields nothing), so a segment takes n * n pair slots.
struct LeSeg {
  long long pair_off;
  int line_off, n, only_angular, pad;
  double max_dist;
};
namespace la {
inline void add_segment(std::vector<LeSeg>* segs, const int line_off, const int n, const bool only_angular, const double max_dist) {
  LeSeg g;
  g.pair_off = segs->empty() ? 0 : segs->back().pair_off + (long long)segs->back().n * segs->back().n;
  g.line_off = line_off; g.n = n; g.only_angular = only_angular ? 1 : 0; g.pad = 0; g.max_dist = max_dist;
  segs->push_back(g);
}
inline long long pair_slots(const std::vector<LeSeg>& segs) { return segs.empty() ? 0 : segs.back().pair_off + (long long)segs.back().n * segs.back().n; }

// ---- align_local (:205-297) on the host: the restatement the device path of line_align_local.hip is tested against, and the CPU side of
// scripts/bench_line_align_local.py.  The semantics are DESIGN.md 6g's.
struct LocalParams {
  Weights w;                 // the l_* members
  double max_distance, cos_max_angle, max_range;
  int float_chain, tie_highest, three_nearest;
};
struct LocalHyp {
  int gate, target;          // target: the target line of a line-pair hypothesis, -1 for an edge pair
  Tf t;
  double tn;
  double fit[5];             // the four fitness values and the score; zeros when gated
};
struct LocalResult {
  Tf t, t_edge;              // the final transformation and the edge-pair phase's (best_trans)
  double fit[5], fit_edge[5], fit_base[5];
  long long winner_edge, winner_line, survivors_edge, survivors_line;
  int n_edges_source, n_edges_target;
};
inline void align_local(const std::vector<Line>& src, const std::vector<Line>& trg, const LocalParams& P, LocalResult* r, std::vector<Line>* aligned,
                        std::vector<LocalHyp>* hyps_edge, std::vector<LocalHyp>* hyps_line) {
  const std::vector<V3> dir = directions(trg);
  std::vector<Edge> es, et;
  edge_extraction(src, es, true, 0.01);
  edge_extraction(trg, et, true);
  r->n_edges_source = (int)es.size();
  r->n_edges_target = (int)et.size();
  const Fitness fb = calc_fitness<true>(src, trg, dir, P.max_range, P.tie_highest);
  store_fit(r->fit_base, fb, weight(P.w, fb.avg_distance, fb.coverage_percentage, 0.0));
  for (int k = 0; k < 5; k++) r->fit_edge[k] = r->fit_base[k];
  r->t_edge = tf_identity();
  r->winner_edge = r->winner_line = -1;
  r->survivors_edge = r->survivors_line = 0;
  std::vector<Line> base = src, cand;
  if (hyps_edge) hyps_edge->clear();
  if (hyps_line) hyps_line->clear();
  // the edge pairs, h = es * Et + et
  for (size_t a = 0; a < es.size(); a++)
    for (size_t b = 0; b < et.size(); b++) {
      LocalHyp hy;
      hy.target = -1;
      for (int k = 0; k < 5; k++) hy.fit[k] = 0.0;
      hy.t = align_edges(es[a], et[b], nullptr);
      hy.gate = gate_local(hy.t, P.max_distance, P.cos_max_angle, P.float_chain, &hy.tn);
      if (hy.gate == GATE_PASS) {
        r->survivors_edge++;
        transform_lines(src, hy.t, &cand);
        const Fitness f = calc_fitness<true>(cand, trg, dir, P.max_range, P.tie_highest);
        store_fit(hy.fit, f, weight(P.w, f.avg_distance, f.coverage_percentage, hy.tn));
        if (hy.fit[4] > r->fit_edge[4]) {
          for (int k = 0; k < 5; k++) r->fit_edge[k] = hy.fit[k];
          r->t_edge = hy.t;
          r->winner_edge = (long long)(a * et.size() + b);
          base = cand;
        }
      }
      if (hyps_edge) hyps_edge->push_back(hy);
    }
  // the line pairs over the snapshot, k = i * Lt + r
  for (int k = 0; k < 5; k++) r->fit[k] = r->fit_edge[k];
  r->t = r->t_edge;
  *aligned = base;
  const int Lt = (int)trg.size();
  std::vector<double> key((size_t)Lt);
  std::vector<int> order((size_t)Lt);
  for (size_t i = 0; i < base.size(); i++) {
    const float sl = lenght(base[i].a, base[i].b);
    for (int j = 0; j < Lt; j++) key[(size_t)j] = nn_key(line_to_line(base[i].a, base[i].b, sl, trg[(size_t)j].a, trg[(size_t)j].b, dir[(size_t)j]).real);
    for (int j = 0; j < Lt; j++) {
      int rank = 0;
      for (int q = 0; q < Lt; q++) rank += rank_before(key[(size_t)q], q, key[(size_t)j], j, P.tie_highest) ? 1 : 0;
      order[(size_t)rank] = j;
    }
    for (int rk = 0; rk < Lt; rk++) {
      LocalHyp hy;
      hy.target = order[(size_t)rk];
      for (int k = 0; k < 5; k++) hy.fit[k] = 0.0;
      hy.t = tf_identity();
      hy.tn = 0.0;
      hy.gate = P.three_nearest && rk >= 3 ? (int)GATE_RANK : line_hypothesis(base[i], trg[(size_t)hy.target], P.max_distance, P.cos_max_angle, &hy.t, &hy.tn);
      if (hy.gate == GATE_PASS) {
        r->survivors_line++;
        transform_lines(base, hy.t, &cand);
        const Fitness f = calc_fitness<true>(cand, trg, dir, P.max_range, P.tie_highest);
        store_fit(hy.fit, f, weight(P.w, f.avg_distance, f.coverage_percentage, hy.tn));
        if (hy.fit[4] > r->fit[4]) {
          for (int k = 0; k < 5; k++) r->fit[k] = hy.fit[k];
          r->t = compose(r->t_edge, hy.t);
          r->winner_line = (long long)i * Lt + rk;
          *aligned = cand;
        }
      }
      if (hyps_line) hyps_line->push_back(hy);
    }
  }
}

}  // namespace la
}  // namespace dgs
