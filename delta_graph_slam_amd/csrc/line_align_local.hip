// LineBasedScanmatcher::align_local (upstream src/hdl_graph_slam/line_based_scanmatcher.cpp:205-297) on the device, for a batch of
// independent items (a keyframe's near buildings): per item the baseline, the edge-pair hypotheses h = es * Et + et with their two
// gates, the strict arg-max, then the line-pair hypotheses k = i * Lt + r over the snapshot of the first phase's result and the second
// arg-max.  Edge extraction runs on the host from the same functions (line_align.h), or with params->edges_on_device on the device
// (line_edges.hip): one batched extraction over all items' sources and targets, 2 * n_items segments, no per-item host loop.  That
// costs one more host wait (the edge offsets come back to build the item and workgroup tables, counts8[1] == 2), a second upload (those
// tables) and the extraction's launches, whose number does not depend on n_items either.  The scorer
// (la::fitness_wave), the wave arg-max and the host's checks and packing are line_align.h's, shared with line_align.hip.
//
// MI355X design
//   * One upload: the item table (sizes and offsets), the two workgroup tables, every item's source lines, target table (A, B,
//     (B - A).normalized() per line) and both edge lists.  One download: a record per item and the aligned lines.  One host wait.
//   * Seven launches whatever the number of items: lal_edge_hypothesis_kernel (a lane per edge pair of the batch), lal_score_kernel<0>,
//     lal_argmax_edge_kernel (a workgroup per item: the segmented arg-max, then the snapshot lines), lal_key_kernel and
//     lal_line_hypothesis_kernel (a lane per (snapshot line, target line): the real_distance keys, then the counting rank, O(Lt) per
//     lane, and the hypothesis at its rank), lal_score_kernel<1>, lal_argmax_line_kernel (a workgroup per item: the record and the
//     aligned lines).  The second phase reads the first phase's winner on the device.
//   * lal_score_kernel runs the scorer align_global runs, la::fitness_wave, with the local comparison: one wavefront per hypothesis.
//     Items have different target tables, so a workgroup serves one item: the host's table gives every workgroup its (item, first unit) and
//     the workgroup's four waves walk kLalUnits consecutive units of that item against one LDS copy of its table (72 bytes per line,
//     36 KiB at the limit of 512 lines).  A gated hypothesis costs its wave one load.  Nothing is accumulated across waves or with
//     atomics, so an item's results do not depend on what else is in the batch.
// Semantics, limits and the deliberate differences from upstream: DESIGN.md 6g.
#include <algorithm>
#include <cfloat>
#include <climits>
#include <cmath>
#include <cstddef>
#include <cstring>
#include <vector>

#include "handle.h"
#include "line_align.h"

namespace dgs {

constexpr int kLalUnits = 8;            // units (hypotheses; in phase 0 also the baseline) per workgroup of lal_score_kernel: two per wave
constexpr int kLalWaves = kBlock / kWave;

struct LalHyp {
  la::Tf t;
  double tn;            // translation.norm() of this hypothesis's own transform
  int gate, target;
};

struct LalItem {
  int Ls, Lt, Es, Et;
  int src_off, trg_off, es_off, et_off;   // first source line, target line, source edge and target edge of the item in the batch's arrays
  long long h1_off, h2_off;               // first hypothesis of the item in each phase; phase 1 starts after all of phase 0
};

struct LalRecord {
  la::Tf t, t_edge;
  double fit[5], fit_edge[5], fit_base[5];   // the four fitness values and the score
  long long winner_edge, winner_line, surv_edge, surv_line;
};

struct LalArgs {
  int n_items, float_chain, tie_highest, three_nearest;
  long long H1, H2;
  double max_distance, cos_max_angle, max_range;
  la::Weights w;
};

// the item that owns hypothesis g of a phase: the last item whose first hypothesis is <= g (empty items share their successor's offset).
// g < the phase's total, so the result's range holds g.
template <int PHASE>
__device__ __forceinline__ int lal_find_item(const LalItem* __restrict__ items, const int n, const long long g) {
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    const long long off = PHASE == 0 ? items[mid].h1_off : items[mid].h2_off;
    if (off <= g) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

// ================================================================================================ phase 0: edge pairs
__global__ __launch_bounds__(kBlock) void lal_edge_hypothesis_kernel(const LalItem* __restrict__ items, const double* __restrict__ es,
                                                                     const double* __restrict__ et, const LalArgs a, LalHyp* __restrict__ hyps,
                                                                     double* __restrict__ fit) {
  const long long g = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (g >= a.H1) return;
  const LalItem it = items[lal_find_item<0>(items, a.n_items, g)];
  const long long h = g - it.h1_off;                                  // 0 <= h < Es * Et of this item
  const int is = it.es_off + (int)(h / it.Et), ie = it.et_off + (int)(h % it.Et);
  LalHyp hy;
  hy.t = la::align_edges(la::load_edge(es + 9 * (long long)is), la::load_edge(et + 9 * (long long)ie), nullptr);
  hy.gate = la::gate_local(hy.t, a.max_distance, a.cos_max_angle, a.float_chain, &hy.tn);
  hy.target = -1;
  hyps[g] = hy;
#pragma unroll
  for (int k = 0; k < 5; k++) fit[5 * g + k] = 0.0;
}

// ================================================================================================ scores
// PHASE 0: unit 0 of an item is its baseline (the source lines as they are), unit u > 0 the edge pair h = u - 1 over the source lines.
// PHASE 1: unit u is the line pair k = u over the snapshot lines.
template <int PHASE>
__global__ __launch_bounds__(kBlock) void lal_score_kernel(const LalItem* __restrict__ items, const int2* __restrict__ wg, const int n_wg,
                                                           const double* __restrict__ lines, const double* __restrict__ tbl, const LalArgs a,
                                                           const LalHyp* __restrict__ hyps, double* __restrict__ fit, LalRecord* __restrict__ rec) {
  __shared__ double s_t[DGS_LA_MAX_LINES_TARGET * la::kTableDoubles];
  if ((int)blockIdx.x >= n_wg) return;                                // uniform: the grid is at least one workgroup
  const int2 w = wg[blockIdx.x];
  const LalItem it = items[w.x];
  const double* t = tbl + (long long)it.trg_off * la::kTableDoubles;
  for (int k = threadIdx.x; k < it.Lt * la::kTableDoubles; k += kBlock) s_t[k] = t[k];   // Lt <= DGS_LA_MAX_LINES_TARGET (checked on the host)
  __syncthreads();
  const int lane = threadIdx.x & (kWave - 1), wv = threadIdx.x / kWave;
  const long long units = PHASE == 0 ? (long long)it.Es * it.Et + 1 : (long long)it.Ls * it.Lt;
  const long long end = min((long long)w.y + kLalUnits, units);
  const double* src = lines + 6 * (long long)it.src_off;
  for (long long u = (long long)w.y + wv; u < end; u += kLalWaves) {  // uniform per wave
    const bool base = PHASE == 0 && u == 0;
    const long long idx = PHASE == 0 ? it.h1_off + u - 1 : it.h2_off + u;
    la::Tf tf = la::tf_identity();
    double tn = 0.0;
    if (!base) {
      const LalHyp hy = hyps[idx];
      if (hy.gate != la::GATE_PASS) continue;
      tf = hy.t;
      tn = hy.tn;
    }
    const la::Fitness f = la::fitness_wave<true>(src, it.Ls, !base, tf, s_t, it.Lt, lane, a.tie_highest, a.max_range);
    const double score = la::weight(a.w, f.avg_distance, f.coverage_percentage, tn);
    if (lane == 0) la::store_fit(base ? rec[w.x].fit_base : fit + 5 * idx, f, score);
  }
}

// ================================================================================================ arg-max
// One workgroup per item over hypotheses [off, off + H): strict > from `start`, the lowest index among the maxima, NaN never wins.
// Thread 0 returns the winner (-1: none) and the survivor count; the other threads' return values are not meaningful.
__device__ __forceinline__ long long lal_argmax_block(const LalHyp* __restrict__ hyps, const double* __restrict__ fit, const long long off,
                                                      const long long H, const double start, long long* surv_out) {
  __shared__ double s_s[kLalWaves];
  __shared__ int s_h[kLalWaves];
  __shared__ int s_n[kLalWaves];
  double best = start;
  int bh = -1, n = 0;
  for (long long h = threadIdx.x; h < H; h += kBlock) {               // h ascends per lane: the first of equal scores stays
    if (hyps[off + h].gate != la::GATE_PASS) continue;
    n++;
    const double sc = fit[5 * (off + h) + 4];
    if (sc > best) { best = sc; bh = (int)h; }
  }
  la::argmax_wave(best, bh);
#pragma unroll
  for (int o = kWave / 2; o > 0; o >>= 1) n += __shfl_xor(n, o, kWave);
  const int lane = threadIdx.x & (kWave - 1), wv = threadIdx.x / kWave;
  if (lane == 0) { s_s[wv] = best; s_h[wv] = bh; s_n[wv] = n; }
  __syncthreads();
  for (int w = 1; w < kLalWaves; w++) {
    if (la::takes_over(s_s[w], s_h[w], best, bh)) { best = s_s[w]; bh = s_h[w]; }
  }
  *surv_out = (long long)s_n[0] + s_n[1] + s_n[2] + s_n[3];
  return wv == 0 ? (long long)bh : -1;
}
static_assert(kLalWaves == 4, "lal_argmax_block adds four per-wave counts");

__global__ __launch_bounds__(kBlock) void lal_argmax_edge_kernel(const LalItem* __restrict__ items, const int n_items, const double* __restrict__ src,
                                                                 const LalHyp* __restrict__ hyps, const double* __restrict__ fit,
                                                                 LalRecord* __restrict__ rec, double* __restrict__ base) {
  __shared__ long long s_win;
  if ((int)blockIdx.x >= n_items) return;
  const LalItem it = items[blockIdx.x];
  LalRecord* r = rec + blockIdx.x;
  long long surv = 0;
  const long long win = lal_argmax_block(hyps, fit, it.h1_off, (long long)it.Es * it.Et, r->fit_base[4], &surv);
  if (threadIdx.x == 0) {
    r->winner_edge = win;
    r->surv_edge = surv;
    r->t_edge = win >= 0 ? hyps[it.h1_off + win].t : la::tf_identity();
    for (int k = 0; k < 5; k++) r->fit_edge[k] = win >= 0 ? fit[5 * (it.h1_off + win) + k] : r->fit_base[k];
    s_win = win;
  }
  __syncthreads();
  const long long w = s_win;
  la::Tf t = la::tf_identity();
  if (w >= 0) t = hyps[it.h1_off + w].t;
  // the snapshot (best_lines): transform_lines(linesSource, transform), or the source lines themselves
  for (int k = threadIdx.x; k < 2 * it.Ls; k += kBlock) {
    const long long p = 3 * (2 * (long long)it.src_off + k);
    la::V3 v = la::load3(src + p);
    if (w >= 0) v = la::apply(t, v);
    la::store3(base + p, v);
  }
}

__global__ __launch_bounds__(kBlock) void lal_argmax_line_kernel(const LalItem* __restrict__ items, const int n_items, const double* __restrict__ base,
                                                                 const LalHyp* __restrict__ hyps, const double* __restrict__ fit,
                                                                 LalRecord* __restrict__ rec, double* __restrict__ aligned) {
  __shared__ long long s_win;
  if ((int)blockIdx.x >= n_items) return;
  const LalItem it = items[blockIdx.x];
  LalRecord* r = rec + blockIdx.x;
  long long surv = 0;
  const long long win = lal_argmax_block(hyps, fit, it.h2_off, (long long)it.Ls * it.Lt, r->fit_edge[4], &surv);
  if (threadIdx.x == 0) {
    r->winner_line = win;
    r->surv_line = surv;
    r->t = win >= 0 ? la::compose(r->t_edge, hyps[it.h2_off + win].t) : r->t_edge;   // best_trans * transform
    for (int k = 0; k < 5; k++) r->fit[k] = win >= 0 ? fit[5 * (it.h2_off + win) + k] : r->fit_edge[k];
    s_win = win;
  }
  __syncthreads();
  const long long w = s_win;
  la::Tf t = la::tf_identity();
  if (w >= 0) t = hyps[it.h2_off + w].t;
  for (int k = threadIdx.x; k < 2 * it.Ls; k += kBlock) {              // transform_lines(best_lines, transform)
    const long long p = 3 * (2 * (long long)it.src_off + k);
    la::V3 v = la::load3(base + p);
    if (w >= 0) v = la::apply(t, v);
    la::store3(aligned + p, v);
  }
}

// ================================================================================================ phase 1: line pairs
// q = (the item's first line pair) + i * Lt + j: the real_distance key of snapshot line i against target line j
__global__ __launch_bounds__(kBlock) void lal_key_kernel(const LalItem* __restrict__ items, const double* __restrict__ base,
                                                         const double* __restrict__ tbl, const LalArgs a, double* __restrict__ keys) {
  const long long q = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (q >= a.H2) return;
  const LalItem it = items[lal_find_item<1>(items, a.n_items, a.H1 + q)];
  const long long local = a.H1 + q - it.h2_off;                       // 0 <= local < Ls * Lt of this item
  const int i = (int)(local / it.Lt), j = (int)(local % it.Lt);
  const double* s = base + 6 * ((long long)it.src_off + i);
  const double* t = tbl + la::kTableDoubles * ((long long)it.trg_off + j);
  const la::V3 sa = la::load3(s), sb = la::load3(s + 3);
  keys[q] = la::nn_key(la::line_to_line(sa, sb, la::lenght(sa, sb), la::load3(t), la::load3(t + 3), la::load3(t + 6)).real);
}

// the same lane layout: target j's rank r among the Lt keys of snapshot line i by counting, then hypothesis k = i * Lt + r.  The ranks
// of one line are a permutation of 0 .. Lt - 1, so every k is written exactly once.
__global__ __launch_bounds__(kBlock) void lal_line_hypothesis_kernel(const LalItem* __restrict__ items, const double* __restrict__ base,
                                                                     const double* __restrict__ tbl, const double* __restrict__ keys, const LalArgs a,
                                                                     LalHyp* __restrict__ hyps, double* __restrict__ fit) {
  const long long q = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (q >= a.H2) return;
  const LalItem it = items[lal_find_item<1>(items, a.n_items, a.H1 + q)];
  const long long local = a.H1 + q - it.h2_off;
  const int i = (int)(local / it.Lt), j = (int)(local % it.Lt);
  const double* row = keys + (q - j);
  const double key = row[j];
  int rank = 0;
  for (int o = 0; o < it.Lt; o++) rank += la::rank_before(row[o], o, key, j, a.tie_highest) ? 1 : 0;
  const double* s = base + 6 * ((long long)it.src_off + i);
  const double* t = tbl + la::kTableDoubles * ((long long)it.trg_off + j);
  la::Line ls, lt;
  ls.a = la::load3(s); ls.b = la::load3(s + 3);
  lt.a = la::load3(t); lt.b = la::load3(t + 3);
  LalHyp hy;
  hy.t = la::tf_identity();
  hy.tn = 0.0;
  hy.target = j;
  hy.gate = a.three_nearest && rank >= 3 ? (int)la::GATE_RANK : la::line_hypothesis(ls, lt, a.max_distance, a.cos_max_angle, &hy.t, &hy.tn);
  const long long idx = it.h2_off + (long long)i * it.Lt + rank;     // rank < Lt: inside the item's range
  hyps[idx] = hy;
#pragma unroll
  for (int k = 0; k < 5; k++) fit[5 * idx + k] = 0.0;
}

// ================================================================================================ host side
namespace {

inline size_t lal_align8(size_t b) { return (b + 7) & ~(size_t)7; }

// the l_* members of a struct that has them, upstream's defaults for one that ends before them
dgs_line_align_params lal_params(const dgs_line_align_params* p) {
  dgs_line_align_params q;
  dgs_line_align_params_init(&q);
  std::memcpy(&q, p, std::min<size_t>(p->struct_size, sizeof(q)));
  q.struct_size = sizeof(q);
  return q;
}
const char* lal_bad_params(const dgs_line_align_params* p) {
  if (const char* why = la::params_guard(p)) return why;
  const dgs_line_align_params q = lal_params(p);
  if (!(q.l_max_score_distance > 0.0) || !(q.l_max_score_translation > 0.0)) return "line align: the max_score values must be positive";
  for (const double w : {q.l_avg_distance_weight, q.l_coverage_weight, q.l_transform_weight})
    if (!(w >= 0.0)) return "line align: an l_* weight is negative or NaN";
  if (std::isnan(q.l_max_distance) || std::isnan(q.l_max_angle)) return "line align: l_max_distance / l_max_angle is NaN";
  return nullptr;
}

}  // namespace

void line_align_local_release(dgs_handle* h) {
  LalScratch& s = h->lal;
  s.in.release(); s.tab.release(); s.hyps.release(); s.fit.release(); s.keys.release(); s.base.release(); s.out.release();
  s.off1.clear();
  s.off2.clear();
}

}  // namespace dgs

using namespace dgs;

extern "C" {

int dgs_line_edges_angular(const dgs_line_feature* lines, int64_t n, int32_t only_angular_edges, double max_dist_angular_edge,
                           dgs_edge_feature* edges, int64_t capacity, int64_t* n_edges) {
  if (n < 0 || !n_edges || (n > 0 && !lines) || capacity < 0 || (capacity > 0 && !edges) || std::isnan(max_dist_angular_edge)) return DGS_ERR_INVALID_ARGUMENT;
  std::vector<la::Edge> e;
  la::edge_extraction(la::lines_of(lines, n), e, only_angular_edges != 0, max_dist_angular_edge);
  *n_edges = (int64_t)e.size();
  if (*n_edges > capacity) return DGS_ERR_INVALID_ARGUMENT;
  for (size_t i = 0; i < e.size(); i++) {
    la::store3(edges[i].edge_point, e[i].e);
    la::store3(edges[i].point_a, e[i].a);
    la::store3(edges[i].point_b, e[i].b);
  }
  return DGS_OK;
}

int dgs_line_align_local_batch(dgs_handle* h, const dgs_line_align_params* params, int64_t n_items, const dgs_line_feature* src_lines,
                               const int64_t* src_offsets, const dgs_line_feature* trg_lines, const int64_t* trg_offsets, double max_range,
                               dgs_line_feature* aligned_lines, dgs_line_local_alignment* alignments) {
  if (const char* why = lal_bad_params(params)) {   // before anything touches a device; without a handle the message is dgs_last_error(NULL)'s
    if (h) h->err = why;
    else set_handleless_error(why);
    return DGS_ERR_INVALID_ARGUMENT;
  }
  if (!h) set_handleless_error("line align: the handle is NULL");
  if (!h || n_items < 0 || (n_items > 0 && (!alignments || !src_offsets || !trg_offsets))) return DGS_ERR_INVALID_ARGUMENT;
  h->err.clear();
  LalScratch& s = h->lal;
  for (int k = 0; k < 8; k++) s.counts8[k] = 0;
  s.off1.assign(1, 0);
  s.off2.assign(1, 0);
  if (n_items == 0) return DGS_OK;
  const char* why = nullptr;
  if (n_items > DGS_LA_MAX_ITEMS) why = "line align: more than DGS_LA_MAX_ITEMS items";
  else if (std::isnan(max_range)) why = "line align: max_range is NaN";
  else if (src_offsets[0] != 0 || trg_offsets[0] != 0) why = "line align: the first offset is not 0";
  for (int64_t b = 0; b < n_items && !why; b++) {
    const int64_t ls = src_offsets[b + 1] - src_offsets[b], lt = trg_offsets[b + 1] - trg_offsets[b];
    if (ls < 0 || lt < 0) why = "line align: offsets are not ascending";
    else if (ls > DGS_LA_MAX_LINES_SOURCE) why = "line align: more than DGS_LA_MAX_LINES_SOURCE source lines in an item";
    else if (lt > DGS_LA_MAX_LINES_TARGET) why = "line align: more than DGS_LA_MAX_LINES_TARGET target lines in an item";
  }
  const int64_t n_src = why ? 0 : src_offsets[n_items], n_trg = why ? 0 : trg_offsets[n_items];
  if (!why && ((n_src > 0 && !src_lines) || (n_trg > 0 && !trg_lines))) why = "line align: a line array is NULL";
  if (!why && (!la::all_finite(src_lines, n_src) || !la::all_finite(trg_lines, n_trg))) why = "line align: a line coordinate is not finite";
  if (why) {
    h->err = why;
    return DGS_ERR_INVALID_ARGUMENT;
  }
  const dgs_line_align_params prm = lal_params(params);

  // ---- the host's share: edges (or, with edges_on_device, their offsets read back from the device), offsets, the workgroup tables
  const std::vector<la::Line> src = la::lines_of(src_lines, n_src), trg = la::lines_of(trg_lines, n_trg);
  const auto part = [](const std::vector<la::Line>& v, int first, int n) { return std::vector<la::Line>(v.begin() + first, v.begin() + first + n); };
  const bool dev_edges = la::edges_on_device(params);
  const size_t n_srcd = (size_t)n_src * 6, n_tbl = (size_t)n_trg * la::kTableDoubles, n_trg6 = dev_edges ? (size_t)n_trg * 6 : 0;
  const size_t b_lines = (n_srcd + n_trg6 + n_tbl) * sizeof(double);
  std::vector<LalItem> items((size_t)n_items);
  std::vector<la::Edge> es, et;
  std::vector<int2> wg1, wg2;
  const int* eoff = nullptr;
  if (dev_edges) {
    // segments 0 .. n_items - 1: the sources; n_items .. 2 n_items - 1: the targets, whose packed lines follow the sources'
    std::vector<LeSeg> segs;
    for (int64_t b = 0; b < n_items; b++) la::add_segment(&segs, (int)src_offsets[b], (int)(src_offsets[b + 1] - src_offsets[b]), true, 0.01);
    for (int64_t b = 0; b < n_items; b++) la::add_segment(&segs, (int)(n_src + trg_offsets[b]), (int)(trg_offsets[b + 1] - trg_offsets[b]), true, 7.0);
    if (la::pair_slots(segs) > DGS_LA_MAX_EDGE_PAIRS) {
      h->err = "line align: edges_on_device: more than DGS_LA_MAX_EDGE_PAIRS pairs (the squares of the items' line counts, summed)";
      return DGS_ERR_INVALID_ARGUMENT;
    }
    // the first upload: source lines, target lines, target tables
    DGS_HIP_TRY(h, hipSetDevice(h->device));
    DGS_HIP_TRY(h, s.in.reserve(std::max<size_t>(b_lines, 8)));
    if (ensure_pinned(h, b_lines) != DGS_OK) return DGS_ERR_HIP;
    double* o = la::pack_lines(src, static_cast<double*>(h->pinned));
    o = la::pack_lines(trg, o);
    la::pack_target_table(trg, la::directions(trg), o);
    if (b_lines) DGS_HIP_TRY(h, hipMemcpyAsync(s.in.ptr, h->pinned, b_lines, hipMemcpyHostToDevice, h->stream));
    const int rc = line_edges_run(h, reinterpret_cast<const double*>(s.in.ptr), segs, true);
    s.counts8[0] += h->le.counts4[0];
    s.counts8[1] += h->le.counts4[1];
    if (rc != DGS_OK) {
      (void)hipStreamSynchronize(h->stream);
      return rc;
    }
    eoff = h->le.eoff_host.data();                                     // 2 * n_items + 1 entries; this call's copies have completed
  }
  long long H1 = 0, H2 = 0;
  for (int64_t b = 0; b < n_items; b++) {
    LalItem& it = items[(size_t)b];
    it.Ls = (int)(src_offsets[b + 1] - src_offsets[b]);
    it.Lt = (int)(trg_offsets[b + 1] - trg_offsets[b]);
    it.src_off = (int)src_offsets[b];
    it.trg_off = (int)trg_offsets[b];
    if (dev_edges) {
      it.es_off = eoff[b];
      it.et_off = eoff[n_items + b] - eoff[n_items];
      it.Es = eoff[b + 1] - eoff[b];
      it.Et = eoff[n_items + b + 1] - eoff[n_items + b];
    } else {
      it.es_off = (int)es.size();
      it.et_off = (int)et.size();
      la::edge_extraction(part(src, it.src_off, it.Ls), es, true, 0.01);
      la::edge_extraction(part(trg, it.trg_off, it.Lt), et, true);
      it.Es = (int)es.size() - it.es_off;
      it.Et = (int)et.size() - it.et_off;
    }
    it.h1_off = H1;
    it.h2_off = H2;                                                    // made absolute below
    H1 += (long long)it.Es * it.Et;
    H2 += (long long)it.Ls * it.Lt;
    if (H1 + H2 > DGS_LA_MAX_HYPOTHESES) {
      h->err = "line align: more than DGS_LA_MAX_HYPOTHESES hypotheses in the batch (both phases, all items)";
      return DGS_ERR_INVALID_ARGUMENT;
    }
  }
  s.off1.clear();
  s.off2.clear();
  for (int64_t b = 0; b < n_items; b++) {
    LalItem& it = items[(size_t)b];
    it.h2_off += H1;
    s.off1.push_back(it.h1_off);
    s.off2.push_back(it.h2_off);
    const long long u1 = (long long)it.Es * it.Et + 1, u2 = (long long)it.Ls * it.Lt;
    for (long long u = 0; u < u1; u += kLalUnits) wg1.push_back(make_int2((int)b, (int)u));
    for (long long u = 0; u < u2; u += kLalUnits) wg2.push_back(make_int2((int)b, (int)u));
  }
  s.off1.push_back(H1);
  s.off2.push_back(H1 + H2);

  // ---- one upload (edges_on_device: the second, of the tables alone; the lines are on the device already)
  const size_t b_items = lal_align8(items.size() * sizeof(LalItem)), b_wg1 = lal_align8(wg1.size() * sizeof(int2)), b_wg2 = lal_align8(wg2.size() * sizeof(int2));
  const size_t n_es = es.size() * 9, n_et = et.size() * 9;
  const size_t b_tab = b_items + b_wg1 + b_wg2;
  const size_t b_in = dev_edges ? b_tab : b_tab + (n_srcd + n_tbl + n_es + n_et) * sizeof(double);
  const size_t b_rec = (size_t)n_items * sizeof(LalRecord), b_out = b_rec + n_srcd * sizeof(double);
  const size_t HH = (size_t)std::max<long long>(H1 + H2, 1);
  DGS_HIP_TRY(h, hipSetDevice(h->device));
  DGS_HIP_TRY(h, (dev_edges ? s.tab : s.in).reserve(b_in));
  DGS_HIP_TRY(h, s.hyps.reserve(HH));
  DGS_HIP_TRY(h, s.fit.reserve(HH * 5));
  DGS_HIP_TRY(h, s.keys.reserve((size_t)std::max<long long>(H2, 1)));
  DGS_HIP_TRY(h, s.base.reserve(std::max<size_t>(n_srcd, 1)));
  DGS_HIP_TRY(h, s.out.reserve(b_out));
  if (ensure_pinned(h, b_in + b_out) != DGS_OK) return DGS_ERR_HIP;
  char* up = static_cast<char*>(h->pinned);
  char* down = up + b_in;                                              // b_in is a multiple of 8
  std::memcpy(up, items.data(), items.size() * sizeof(LalItem));
  if (!wg1.empty()) std::memcpy(up + b_items, wg1.data(), wg1.size() * sizeof(int2));
  if (!wg2.empty()) std::memcpy(up + b_items + b_wg1, wg2.data(), wg2.size() * sizeof(int2));
  if (!dev_edges) {
    double* o = reinterpret_cast<double*>(up + b_tab);
    o = la::pack_lines(src, o);
    o = la::pack_target_table(trg, la::directions(trg), o);
    o = la::pack_edges(es, o);
    la::pack_edges(et, o);
  }
  unsigned char* d_tab = dev_edges ? s.tab.ptr : s.in.ptr;
  DGS_HIP_TRY(h, hipMemcpyAsync(d_tab, up, b_in, hipMemcpyHostToDevice, h->stream));
  const LalItem* d_items = reinterpret_cast<const LalItem*>(d_tab);
  const int2* d_wg1 = reinterpret_cast<const int2*>(d_tab + b_items);
  const int2* d_wg2 = reinterpret_cast<const int2*>(d_tab + b_items + b_wg1);
  const double* d_src = reinterpret_cast<const double*>(dev_edges ? s.in.ptr : s.in.ptr + b_tab);
  const double* d_tbl = d_src + n_srcd + n_trg6;
  // edges_on_device: the extraction's buffer, the sources' edges in front of the targets' (not read when the batch has no edge pair)
  const double* d_es = dev_edges ? h->le.edges.ptr : d_tbl + n_tbl;
  const double* d_et = dev_edges ? d_es + 9 * (size_t)eoff[n_items] : d_es + n_es;
  LalRecord* d_rec = reinterpret_cast<LalRecord*>(s.out.ptr);
  double* d_aligned = reinterpret_cast<double*>(s.out.ptr + b_rec);

  LalArgs a{};
  a.n_items = (int)n_items;
  a.float_chain = prm.angle_gate_float_chain ? 1 : 0;
  a.tie_highest = prm.nn_tie_highest_index ? 1 : 0;
  a.three_nearest = prm.refine_three_nearest ? 1 : 0;
  a.H1 = H1;
  a.H2 = H2;
  a.max_distance = prm.l_max_distance;
  a.cos_max_angle = std::cos(prm.l_max_angle);
  a.max_range = max_range;
  a.w.avg_distance_weight = prm.l_avg_distance_weight;
  a.w.coverage_weight = prm.l_coverage_weight;
  a.w.transform_weight = prm.l_transform_weight;
  a.w.max_score_distance = prm.l_max_score_distance;
  a.w.max_score_translation = prm.l_max_score_translation;

  // ---- seven launches whatever the batch holds (a grid is at least one workgroup; the kernels check their counts), counted where
  // they are issued
#define LAL_LAUNCH(...)                 \
  do {                                  \
    hipLaunchKernelGGL(__VA_ARGS__);    \
    s.counts8[0]++;                     \
  } while (0)
  const auto blocks = [](long long n) { return dim3((unsigned)std::max<long long>((n + kBlock - 1) / kBlock, 1)); };
  const dim3 g_items((unsigned)n_items), blk(kBlock);
  LAL_LAUNCH(lal_edge_hypothesis_kernel, blocks(H1), blk, 0, h->stream, d_items, d_es, d_et, a, s.hyps.ptr, s.fit.ptr);
  LAL_LAUNCH(lal_score_kernel<0>, dim3((unsigned)std::max<size_t>(wg1.size(), 1)), blk, 0, h->stream, d_items, d_wg1, (int)wg1.size(), d_src, d_tbl, a,
                     s.hyps.ptr, s.fit.ptr, d_rec);
  LAL_LAUNCH(lal_argmax_edge_kernel, g_items, blk, 0, h->stream, d_items, (int)n_items, d_src, s.hyps.ptr, s.fit.ptr, d_rec, s.base.ptr);
  LAL_LAUNCH(lal_key_kernel, blocks(H2), blk, 0, h->stream, d_items, s.base.ptr, d_tbl, a, s.keys.ptr);
  LAL_LAUNCH(lal_line_hypothesis_kernel, blocks(H2), blk, 0, h->stream, d_items, s.base.ptr, d_tbl, s.keys.ptr, a, s.hyps.ptr, s.fit.ptr);
  LAL_LAUNCH(lal_score_kernel<1>, dim3((unsigned)std::max<size_t>(wg2.size(), 1)), blk, 0, h->stream, d_items, d_wg2, (int)wg2.size(), s.base.ptr,
                     d_tbl, a, s.hyps.ptr, s.fit.ptr, d_rec);
  LAL_LAUNCH(lal_argmax_line_kernel, g_items, blk, 0, h->stream, d_items, (int)n_items, s.base.ptr, s.hyps.ptr, s.fit.ptr, d_rec, d_aligned);
#undef LAL_LAUNCH
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipMemcpyAsync(down, s.out.ptr, b_out, hipMemcpyDeviceToHost, h->stream);
  const hipError_t e2 = hipStreamSynchronize(h->stream);               // the one host wait, also on the error path
  s.counts8[1] += 1;
  DGS_HIP_TRY(h, e);
  DGS_HIP_TRY(h, e2);

  const LalRecord* rec = reinterpret_cast<const LalRecord*>(down);
  const double* al = reinterpret_cast<const double*>(down + b_rec);
  long long surv1 = 0, surv2 = 0;
  for (int64_t b = 0; b < n_items; b++) {
    const LalItem& it = items[(size_t)b];
    const LalRecord& r = rec[b];
    dgs_line_local_alignment& out = alignments[b];
    std::memset(&out, 0, sizeof(out));
    la::matrix(r.t, out.transformation);
    la::matrix(r.t_edge, out.edge_transformation);
    for (int k = 0; k < 4; k++) {
      out.fitness_score[k] = r.fit[k];
      out.edge_fitness_score[k] = r.fit_edge[k];
      out.baseline_fitness_score[k] = r.fit_base[k];
    }
    out.score = r.fit[4];
    out.edge_score = r.fit_edge[4];
    out.baseline_score = r.fit_base[4];
    out.winner_edge = r.winner_edge;
    out.winner_line = r.winner_line;
    out.n_hypotheses_edge = (int64_t)it.Es * it.Et;
    out.n_survivors_edge = r.surv_edge;
    out.n_hypotheses_line = (int64_t)it.Ls * it.Lt;
    out.n_survivors_line = r.surv_line;
    out.n_edges_source = it.Es;
    out.n_edges_target = it.Et;
    out.is_edge_aligned = r.winner_edge >= 0 ? 1 : 0;
    out.status = r.winner_edge >= 0 ? DGS_LA_ALIGNED
                 : r.winner_line >= 0 ? DGS_LA_LINE_ALIGNED
                 : out.n_hypotheses_edge + out.n_hypotheses_line == 0 ? DGS_LA_NO_HYPOTHESES
                 : r.surv_edge + r.surv_line == 0 ? DGS_LA_ALL_GATED
                                                  : DGS_LA_NONE_BETTER;
    surv1 += r.surv_edge;
    surv2 += r.surv_line;
  }
  if (aligned_lines)
    for (int64_t i = 0; i < n_src; i++) {
      aligned_lines[i] = src_lines[i];   // transform_lines copies the line and replaces its two points
      std::memcpy(aligned_lines[i].point_a, al + 6 * i, 24);
      std::memcpy(aligned_lines[i].point_b, al + 6 * i + 3, 24);
    }
  s.counts8[2] = n_items;
  s.counts8[3] = H1;
  s.counts8[4] = H2;
  s.counts8[5] = surv1;
  s.counts8[6] = surv2;
  s.counts8[7] = (int64_t)(wg1.size() + wg2.size());
  return DGS_OK;
}

int dgs_line_align_local(dgs_handle* h, const dgs_line_align_params* params, const dgs_line_feature* src_lines, int64_t n_src,
                         const dgs_line_feature* trg_lines, int64_t n_trg, double max_range, dgs_line_feature* aligned_lines,
                         dgs_line_local_alignment* alignment) {
  const int64_t so[2] = {0, n_src}, to[2] = {0, n_trg};
  return dgs_line_align_local_batch(h, params, 1, src_lines, so, trg_lines, to, max_range, aligned_lines, alignment);
}

int dgs_line_align_local_get_hypotheses(dgs_handle* h, int64_t item, int32_t phase, int64_t first, int64_t count,
                                        dgs_line_align_local_hypothesis* records, int64_t* counts8) {
  if (!h || first < 0 || count < 0) return DGS_ERR_INVALID_ARGUMENT;
  LalScratch& s = h->lal;
  if (counts8)
    for (int k = 0; k < 8; k++) counts8[k] = s.counts8[k];
  if (!records || count == 0) return DGS_OK;
  const std::vector<int64_t>& off = phase == 0 ? s.off1 : s.off2;
  if ((phase != 0 && phase != 1) || item < 0 || item + 1 >= (int64_t)off.size() || first + count > off[(size_t)item + 1] - off[(size_t)item]) {
    h->err = "line align: the range lies beyond the last call's hypotheses";
    return DGS_ERR_INVALID_ARGUMENT;
  }
  const size_t n = (size_t)count;
  const int64_t at = off[(size_t)item] + first;
  std::vector<LalHyp> hy(n);
  std::vector<double> f(n * 5);
  DGS_HIP_TRY(h, hipSetDevice(h->device));
  DGS_HIP_TRY(h, hipMemcpyAsync(hy.data(), s.hyps.ptr + at, n * sizeof(LalHyp), hipMemcpyDeviceToHost, h->stream));
  DGS_HIP_TRY(h, hipMemcpyAsync(f.data(), s.fit.ptr + at * 5, n * 5 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  DGS_HIP_TRY(h, hipStreamSynchronize(h->stream));
  for (size_t i = 0; i < n; i++) {
    dgs_line_align_local_hypothesis& r = records[i];
    r.gate = hy[i].gate;
    r.target = hy[i].target;
    r.rotation[0] = hy[i].t.r00; r.rotation[1] = hy[i].t.r01; r.rotation[2] = hy[i].t.r10; r.rotation[3] = hy[i].t.r11;
    r.translation[0] = hy[i].t.tx; r.translation[1] = hy[i].t.ty; r.translation[2] = hy[i].t.tz;
    for (int k = 0; k < 4; k++) r.fitness_score[k] = f[5 * i + k];
    r.score = f[5 * i + 4];
  }
  return DGS_OK;
}

}  // extern "C"
