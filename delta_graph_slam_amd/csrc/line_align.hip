// LineBasedScanmatcher::align_global (upstream src/hdl_graph_slam/line_based_scanmatcher.cpp:109-203) on the device: every
// (source edge, target edge) pair is a hypothesis h = es * Et + et; align_edges, the three gates, calc_fitness_score of the
// transformed source lines against the merged target lines and the strict arg-max run there.  merge_lines and the refinement pass are
// sequential and run on the host from the same functions (line_align.h); edge_extraction runs there too, or with
// params->edges_on_device on the device (line_edges.hip: the same pair function, the same bits), after the merge and the one upload of
// lines.  The device extraction costs one more host wait: the two edge counts are read back to size the hypothesis space and to check
// DGS_LA_MAX_HYPOTHESES, while the edges themselves stay in HBM for la_hypothesis_kernel.  The counters show it (counts4[1] == 2, and
// the extraction's launches in counts4[0]).  The scorer
// (la::fitness_wave), the wave arg-max and the host's checks and packing are line_align.h's, shared with line_align_local.hip.
//
// MI355X design
//   * One upload: source lines, the target table (A, B, (B - A).normalized() per merged line) and both edge lists (edges_on_device: the
//     merged target lines in place of the edge lists).
//   * la_hypothesis_kernel: one lane per h; transform, gate code, survivor flag.  Survivors are compacted in h order with the
//     shared stable compaction (compact.h: pf_count_kernel, pf_scan_kernel) and la_scatter_kernel.
//   * la_score_kernel: one wavefront per survivor (item 0 is the identity, the baseline) runs la::fitness_wave<false> against the
//     target table in LDS (72 bytes per line, 36 KiB at the limit of 512 lines).  FP64 throughout: the loop is bound by the FP64
//     divide and square-root sequences of line_to_line_distance, not by memory.
//   * la_argmax_kernel: one workgroup; a strictly greater score takes over, equal scores go to the lower h, NaN never wins.
//   * The grid of la_score_kernel is fixed and its waves stride over the survivor count read on the device: one host wait per call.
// Semantics and the Eigen details recalled from upstream: DESIGN.md §6f.
#include <algorithm>
#include <cfloat>
#include <climits>
#include <cmath>
#include <cstddef>
#include <cstring>
#include <vector>

#include "compact.h"
#include "handle.h"
#include "line_align.h"

namespace dgs {

constexpr int kLaArgmaxBlock = 1024;
constexpr int kLaScoreBlocks = 2048;    // la_score_kernel's fixed grid: 8192 waves, 8 per SIMD of 256 CUs
constexpr int kLaWavesPerBlock = kBlock / kWave;

struct LaHyp {
  la::Tf t;
  double tn;   // translation.norm()
};

struct LaResult {
  long long winner;        // h, -1: the baseline stays
  int survivors, pad;
  double fit[5];           // the winner's (or the baseline's) fitness and score
  double base[5];          // the baseline's
  LaHyp hyp;               // the winner's transform
};

struct LaArgs {
  int Ls, Lt, Es, Et;
  int constrain_angle, float_chain, tie_highest, pad;
  double max_distance, cos_max_angle, max_range;
  la::Weights w;
};

// ================================================================================================ hypotheses
__global__ __launch_bounds__(kBlock) void la_hypothesis_kernel(const double* __restrict__ es, const double* __restrict__ et, const LaArgs a,
                                                               LaHyp* __restrict__ hyps, unsigned char* __restrict__ keep,
                                                               unsigned char* __restrict__ gate, double* __restrict__ fit) {
  const long long h = (long long)blockIdx.x * kBlock + threadIdx.x;
  const long long H = (long long)a.Es * a.Et;
  if (h >= H) return;
  const int is = (int)(h / a.Et), it = (int)(h % a.Et);   // is < Es, it < Et: both edge lists are read inside their bounds
  LaHyp hy;
  hy.t = la::align_edges(la::load_edge(es + 9 * is), la::load_edge(et + 9 * it), nullptr);
  const int g = la::gate(hy.t, a.max_distance, a.constrain_angle, a.cos_max_angle, a.float_chain, &hy.tn);
  hyps[h] = hy;
  gate[h] = (unsigned char)g;
  keep[h] = g == la::GATE_PASS ? 1 : 0;
#pragma unroll
  for (int k = 0; k < 5; k++) fit[5 * h + k] = 0.0;
}

// the survivors' h in order, and every h's position in that list
__global__ __launch_bounds__(kBlock) void la_scatter_kernel(const unsigned char* __restrict__ keep, const int n, const int* __restrict__ blk,
                                                            int* __restrict__ surv, int* __restrict__ slot) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  int off;
  if (!compact_slot(keep, i, n, blk, &off)) {
    if (i < n) slot[i] = -1;
    return;
  }
  surv[off] = i;   // off < number of survivors <= n: `surv` holds n entries
  slot[i] = off;
}

// ================================================================================================ scores
// One wavefront per item: item 0 is the untransformed source (the baseline), item s + 1 the s-th survivor.
__global__ __launch_bounds__(kBlock) void la_score_kernel(const double* __restrict__ src, const double* __restrict__ tbl, const LaArgs a,
                                                          const LaHyp* __restrict__ hyps, const int* __restrict__ surv, const int* __restrict__ cnt,
                                                          double* __restrict__ fit, LaResult* __restrict__ res) {
  __shared__ double s_t[DGS_LA_MAX_LINES_TARGET * la::kTableDoubles];
  for (int k = threadIdx.x; k < a.Lt * la::kTableDoubles; k += kBlock) s_t[k] = tbl[k];   // Lt <= DGS_LA_MAX_LINES_TARGET (checked on the host)
  __syncthreads();
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = blockIdx.x * kLaWavesPerBlock + threadIdx.x / kWave;
  const int n_waves = gridDim.x * kLaWavesPerBlock;
  const int items = cnt[0] + 1;
  for (int item = wave; item < items; item += n_waves) {   // uniform per wave
    const bool base = item == 0;
    const int h = base ? -1 : surv[item - 1];
    LaHyp hy;
    hy.t = la::tf_identity();
    hy.tn = 0.0;
    if (!base) hy = hyps[h];
    const la::Fitness f = la::fitness_wave<false>(src, a.Ls, !base, hy.t, s_t, a.Lt, lane, a.tie_highest, a.max_range);
    const double score = la::weight(a.w, f.real_avg_distance, f.coverage_percentage, hy.tn);
    if (lane == 0) la::store_fit(base ? res->base : fit + 5 * (long long)h, f, score);
  }
}

// ================================================================================================ arg-max
// result_score starts at the identity's; a hypothesis takes over iff its score is strictly greater, in h order: the winner is the
// lowest h among the maxima above the baseline.  A NaN score compares false and never wins.
__global__ __launch_bounds__(kLaArgmaxBlock) void la_argmax_kernel(const int* __restrict__ surv, const int* __restrict__ cnt, const double* __restrict__ fit,
                                                                   const LaHyp* __restrict__ hyps, LaResult* __restrict__ res) {
  __shared__ double s_s[kLaArgmaxBlock / kWave];
  __shared__ int s_h[kLaArgmaxBlock / kWave];
  const int S = cnt[0];
  const double base = res->base[4];
  double best = base;
  int bh = -1;
  for (int s = threadIdx.x; s < S; s += kLaArgmaxBlock) {   // s ascends per lane, and so does h: the first of equal scores stays
    const int h = surv[s];
    const double sc = fit[5 * (long long)h + 4];
    if (sc > best) { best = sc; bh = h; }
  }
  la::argmax_wave(best, bh);
  const int lane = threadIdx.x & (kWave - 1), wv = threadIdx.x / kWave;
  if (lane == 0) { s_s[wv] = best; s_h[wv] = bh; }
  __syncthreads();
  if (threadIdx.x != 0) return;
  for (int w = 1; w < kLaArgmaxBlock / kWave; w++)
    if (la::takes_over(s_s[w], s_h[w], best, bh)) { best = s_s[w]; bh = s_h[w]; }
  res->winner = bh;
  res->survivors = S;
  res->pad = 0;
  LaHyp hy;
  hy.t = la::tf_identity();
  hy.tn = 0.0;
  if (bh >= 0) hy = hyps[bh];
  res->hyp = hy;
  for (int k = 0; k < 5; k++) res->fit[k] = bh >= 0 ? fit[5 * (long long)bh + k] : res->base[k];
}

// ================================================================================================ host side
namespace {

void la_merge(const dgs_line_feature* lines, int64_t n, std::vector<la::Line>* out, std::vector<int>* origin) {
  *out = la::lines_of(lines, n);
  origin->clear();
  for (int64_t i = 0; i < n; i++) origin->push_back((int)i);
  la::merge_lines(*out, *origin);
}

const char* la_bad_params(const dgs_line_align_params* p) {
  if (const char* why = la::params_guard(p)) return why;
  if (!(p->g_max_score_distance > 0.0) || !(p->g_max_score_translation > 0.0)) return "line align: the max_score values must be positive";
  // +infinity is a legal weight (that term alone decides); against a zero term it gives a NaN score, which never wins
  for (const double w : {p->g_avg_distance_weight, p->g_coverage_weight, p->g_transform_weight})
    if (!(w >= 0.0)) return "line align: a g_* weight is negative or NaN";
  if (std::isnan(p->max_distance) || std::isnan(p->max_angle)) return "line align: max_distance / max_angle is NaN";
  return nullptr;
}

struct LaOut {
  la::Tf t;
  la::Fitness fit;
  double score;
};

// phase 1 on the device: -> the winner (or the baseline) with one host wait.  dev_edges: es / et are empty, the edges are extracted on
// the device from the uploaded lines (a second wait, for the two counts) and a.Es / a.Et are set here.
int la_search(dgs_handle* h, LaArgs& a, const std::vector<la::Line>& src, const std::vector<la::Line>& trg, const std::vector<la::V3>& dir,
              const std::vector<la::Edge>& es, const std::vector<la::Edge>& et, const bool dev_edges, LaResult* out) {
  LaScratch& s = h->la;
  const size_t n_src = (size_t)a.Ls * 6, n_tbl = (size_t)a.Lt * la::kTableDoubles;
  // the upload: source lines, [dev_edges: target lines,] target table, [host edges: source edges, target edges]
  const size_t n_trg6 = dev_edges ? (size_t)a.Lt * 6 : 0, n_up_es = es.size() * 9, n_up_et = et.size() * 9;
  const size_t n_in = n_src + n_trg6 + n_tbl + n_up_es + n_up_et;
  DGS_HIP_TRY(h, s.in.reserve(std::max<size_t>(n_in, 1)));
  if (ensure_pinned(h, 4096 + n_in * sizeof(double)) != DGS_OK) return DGS_ERR_HIP;
  static_assert(sizeof(LaResult) <= 4096, "the read-back block must fit in front of the upload");
  {
    double* up = reinterpret_cast<double*>(static_cast<char*>(h->pinned) + 4096);
    double* o = la::pack_lines(src, up);
    if (dev_edges) o = la::pack_lines(trg, o);
    o = la::pack_target_table(trg, dir, o);
    o = la::pack_edges(es, o);
    la::pack_edges(et, o);
    if (n_in) DGS_HIP_TRY(h, hipMemcpyAsync(s.in.ptr, up, n_in * sizeof(double), hipMemcpyHostToDevice, h->stream));
  }
  const double* d_src = s.in.ptr;
  const double* d_tbl = d_src + n_src + n_trg6;
  const double* d_es = d_tbl + n_tbl;
  const double* d_et = d_es + n_up_es;
  if (dev_edges) {
    std::vector<LeSeg> segs;
    la::add_segment(&segs, 0, a.Ls, false, 7.0);        // get_edges' defaults: align_global's call
    la::add_segment(&segs, a.Ls, a.Lt, false, 7.0);
    const int rc = line_edges_run(h, d_src, segs, true);   // Ls <= 256, Lt <= 512: far below DGS_LA_MAX_EDGE_PAIRS
    s.counts4[0] += h->le.counts4[0];
    s.counts4[1] += h->le.counts4[1];
    if (rc != DGS_OK) return rc;
    a.Es = h->le.eoff_host[1];
    a.Et = h->le.eoff_host[2] - h->le.eoff_host[1];
    if ((int64_t)a.Es * a.Et > DGS_LA_MAX_HYPOTHESES) {
      h->err = "line align: more than DGS_LA_MAX_HYPOTHESES edge-pair hypotheses";
      return DGS_ERR_INVALID_ARGUMENT;
    }
    d_es = h->le.edges.ptr;                             // not read when there is no hypothesis
    d_et = d_es + 9 * (size_t)a.Es;
  }
  const int64_t H = (int64_t)a.Es * a.Et;
  const size_t hh = (size_t)std::max<int64_t>(H, 1);
  const unsigned nb = (unsigned)((hh + kBlock - 1) / kBlock);
  DGS_HIP_TRY(h, s.hyps.reserve(hh));
  DGS_HIP_TRY(h, s.keep.reserve(hh));
  DGS_HIP_TRY(h, s.gate.reserve(hh));
  DGS_HIP_TRY(h, s.blk.reserve(nb));
  DGS_HIP_TRY(h, s.cnt.reserve(4));
  DGS_HIP_TRY(h, s.surv.reserve(hh));
  DGS_HIP_TRY(h, s.slot.reserve(hh));
  DGS_HIP_TRY(h, s.fit.reserve(hh * 5));
  DGS_HIP_TRY(h, s.result.reserve(1));
  if (H > 0) {
    hipLaunchKernelGGL(la_hypothesis_kernel, dim3(nb), dim3(kBlock), 0, h->stream, d_es, d_et, a, s.hyps.ptr, s.keep.ptr, s.gate.ptr, s.fit.ptr);
    compact_offsets(h->stream, s.keep.ptr, H, s.blk.ptr, s.cnt.ptr);
    hipLaunchKernelGGL(la_scatter_kernel, dim3(nb), dim3(kBlock), 0, h->stream, s.keep.ptr, (int)H, s.blk.ptr, s.surv.ptr, s.slot.ptr);
    s.counts4[0] += 4;
  } else {
    DGS_HIP_TRY(h, hipMemsetAsync(s.cnt.ptr, 0, sizeof(int), h->stream));
  }
  const unsigned blocks = (unsigned)std::min<int64_t>(kLaScoreBlocks, (H + 1 + kLaWavesPerBlock - 1) / kLaWavesPerBlock);
  hipLaunchKernelGGL(la_score_kernel, dim3(blocks), dim3(kBlock), 0, h->stream, d_src, d_tbl, a, s.hyps.ptr, s.surv.ptr, s.cnt.ptr, s.fit.ptr, s.result.ptr);
  hipLaunchKernelGGL(la_argmax_kernel, dim3(1), dim3(kLaArgmaxBlock), 0, h->stream, s.surv.ptr, s.cnt.ptr, s.fit.ptr, s.hyps.ptr, s.result.ptr);
  s.counts4[0] += 2;
  DGS_HIP_TRY(h, hipGetLastError());
  DGS_HIP_TRY(h, hipMemcpyAsync(h->pinned, s.result.ptr, sizeof(LaResult), hipMemcpyDeviceToHost, h->stream));
  DGS_HIP_TRY(h, hipStreamSynchronize(h->stream));
  s.counts4[1] += 1;
  std::memcpy(out, h->pinned, sizeof(LaResult));
  s.n_hyp = H;
  s.counts4[2] = H;
  s.counts4[3] = out->survivors;
  return DGS_OK;
}

// the refinement pass (:160-200): the range-for walks the vector the body reassigns, so later iterations see the new lines while
// best_trans stays the first phase's transform [UPSTREAM-RECALL: vector assignment of equal size keeps the storage]
int la_refine(const dgs_line_align_params& p, const LaArgs& a, const std::vector<la::Line>& trg, const std::vector<la::V3>& dir,
              std::vector<la::Line>* aligned, LaOut* r) {
  const la::Tf best_trans = r->t;
  const double cos_max = a.cos_max_angle;
  int steps = 0;
  for (size_t i = 0; i < aligned->size(); i++) {
    const la::Line ls = (*aligned)[i];
    la::Pair nn;
    const int j = la::nearest(ls.a, ls.b, trg, dir, a.tie_highest, &nn);
    if (j < 0) continue;
    const la::V3 sd = la::normalized(la::sub(ls.a, ls.b)), td = la::normalized(la::sub(trg[(size_t)j].a, trg[(size_t)j].b));
    const double cosine = la::dot(sd, td);
    if (std::fabs(cosine) < cos_max) continue;
    const la::Tf tf = la::align_lines(ls, trg[(size_t)j]);
    const double tn = la::norm(la::v3(tf.tx, tf.ty, tf.tz));
    if (tn > p.max_distance) continue;
    std::vector<la::Line> cand;
    la::transform_lines(*aligned, tf, &cand);
    const la::Fitness f = la::calc_fitness<false>(cand, trg, dir, a.max_range, a.tie_highest);
    const double score = la::weight(a.w, f.real_avg_distance, f.coverage_percentage, tn);
    if (score > r->score) {
      *aligned = cand;
      r->t = la::compose(best_trans, tf);
      r->fit = f;
      r->score = score;
      steps++;
    }
  }
  return steps;
}

}  // namespace

void line_align_release(dgs_handle* h) {
  LaScratch& s = h->la;
  s.in.release(); s.hyps.release(); s.keep.release(); s.gate.release(); s.blk.release(); s.cnt.release(); s.surv.release(); s.slot.release();
  s.fit.release(); s.result.release();
  s.n_hyp = 0;
}

}  // namespace dgs

using namespace dgs;

extern "C" {

int dgs_line_align_params_init(dgs_line_align_params* p) {
  if (!p) return DGS_ERR_INVALID_ARGUMENT;
  std::memset(p, 0, sizeof(*p));
  p->struct_size = sizeof(*p);
  p->angle_gate_float_chain = 1;
  p->g_avg_distance_weight = 0.6;
  p->g_coverage_weight = 1.0;
  p->g_transform_weight = 0.2;
  p->g_max_score_distance = 5.0;
  p->g_max_score_translation = 5.0;
  p->max_distance = 2.0;
  p->max_angle = M_PI / 9.0;
  p->nn_tie_highest_index = 0;
  p->l_avg_distance_weight = 0.6;
  p->l_coverage_weight = 1.0;
  p->l_transform_weight = 0.2;
  p->l_max_score_distance = 5.0;
  p->l_max_score_translation = 5.0;
  p->l_max_distance = 2.5;
  p->l_max_angle = M_PI / 9.0;
  p->refine_three_nearest = 0;
  p->edges_on_device = 0;
  return DGS_OK;
}

int dgs_line_merge(const dgs_line_feature* lines, int64_t n, dgs_line_feature* out, int64_t* n_out) {
  if (n < 0 || !n_out || (n > 0 && (!lines || !out))) return DGS_ERR_INVALID_ARGUMENT;
  std::vector<la::Line> m;
  std::vector<int> origin;
  la_merge(lines, n, &m, &origin);
  for (size_t i = 0; i < m.size(); i++) {
    dgs_line_feature f{};
    if (origin[i] >= 0) f = lines[origin[i]];
    la::store3(f.point_a, m[i].a);
    la::store3(f.point_b, m[i].b);
    out[i] = f;
  }
  *n_out = (int64_t)m.size();
  return DGS_OK;
}

int dgs_line_edges(const dgs_line_feature* lines, int64_t n, dgs_edge_feature* edges, int64_t capacity, int64_t* n_edges) {
  return dgs_line_edges_angular(lines, n, 0, 7.0, edges, capacity, n_edges);   // get_edges' defaults: align_global's call
}

int dgs_line_align_global(dgs_handle* h, const dgs_line_align_params* params, const dgs_line_feature* src_lines, int64_t n_src,
                          const dgs_line_feature* trg_lines, int64_t n_trg, int32_t constrain_angle, double max_range,
                          dgs_line_feature* aligned_lines, dgs_line_alignment* alignment) {
  if (const char* why = la_bad_params(params)) {   // before anything touches a device; without a handle the message is dgs_last_error(NULL)'s
    if (h) h->err = why;
    else set_handleless_error(why);
    return DGS_ERR_INVALID_ARGUMENT;
  }
  if (!h) set_handleless_error("line align: the handle is NULL");
  if (!h || !alignment || n_src < 0 || n_trg < 0 || (n_src > 0 && !src_lines) || (n_trg > 0 && !trg_lines)) return DGS_ERR_INVALID_ARGUMENT;
  h->err.clear();
  std::memset(alignment, 0, sizeof(*alignment));
  const char* why = nullptr;
  if (n_src > DGS_LA_MAX_LINES_SOURCE) why = "line align: more than DGS_LA_MAX_LINES_SOURCE source lines";
  else if (n_trg > (1 << 20)) why = "line align: more than 2^20 target lines";
  else if (std::isnan(max_range)) why = "line align: max_range is NaN";
  else if (!la::all_finite(src_lines, n_src) || !la::all_finite(trg_lines, n_trg)) why = "line align: a line coordinate is not finite";
  if (why) {
    h->err = why;
    return DGS_ERR_INVALID_ARGUMENT;
  }
  const std::vector<la::Line> src = la::lines_of(src_lines, n_src);
  std::vector<la::Line> trg;
  std::vector<int> origin;
  la_merge(trg_lines, n_trg, &trg, &origin);
  if ((int64_t)trg.size() > DGS_LA_MAX_LINES_TARGET) {
    h->err = "line align: more than DGS_LA_MAX_LINES_TARGET target lines after merging";
    return DGS_ERR_INVALID_ARGUMENT;
  }
  const std::vector<la::V3> dir = la::directions(trg);
  const bool dev_edges = la::edges_on_device(params);
  std::vector<la::Edge> es, et;
  if (!dev_edges) {
    la::edge_extraction(src, es);
    la::edge_extraction(trg, et);
    if ((int64_t)es.size() * (int64_t)et.size() > DGS_LA_MAX_HYPOTHESES) {
      h->err = "line align: more than DGS_LA_MAX_HYPOTHESES edge-pair hypotheses";
      return DGS_ERR_INVALID_ARGUMENT;
    }
  }
  LaArgs a{};
  a.Ls = (int)src.size(); a.Lt = (int)trg.size(); a.Es = (int)es.size(); a.Et = (int)et.size();
  a.constrain_angle = constrain_angle ? 1 : 0;
  a.float_chain = params->angle_gate_float_chain ? 1 : 0;
  a.tie_highest = params->nn_tie_highest_index ? 1 : 0;
  a.max_distance = params->max_distance;
  a.cos_max_angle = std::cos(params->max_angle);
  a.max_range = max_range;
  a.w.avg_distance_weight = params->g_avg_distance_weight;
  a.w.coverage_weight = params->g_coverage_weight;
  a.w.transform_weight = params->g_transform_weight;
  a.w.max_score_distance = params->g_max_score_distance;
  a.w.max_score_translation = params->g_max_score_translation;
  for (int k = 0; k < 4; k++) h->la.counts4[k] = 0;
  DGS_HIP_TRY(h, hipSetDevice(h->device));
  LaResult res{};
  const int rc = la_search(h, a, src, trg, dir, es, et, dev_edges, &res);
  if (rc != DGS_OK) {
    (void)hipStreamSynchronize(h->stream);
    return rc;
  }
  const int64_t H = (int64_t)a.Es * a.Et;
  LaOut r;
  r.t = res.hyp.t;
  r.fit.real_avg_distance = res.fit[0]; r.fit.avg_distance = res.fit[1]; r.fit.coverage = res.fit[2]; r.fit.coverage_percentage = res.fit[3];
  r.score = res.fit[4];
  std::vector<la::Line> aligned = src;
  if (res.winner >= 0) la::transform_lines(src, r.t, &aligned);
  const int steps = la_refine(*params, a, trg, dir, &aligned, &r);
  la::matrix(r.t, alignment->transformation);
  alignment->fitness_score[0] = r.fit.real_avg_distance; alignment->fitness_score[1] = r.fit.avg_distance;
  alignment->fitness_score[2] = r.fit.coverage; alignment->fitness_score[3] = r.fit.coverage_percentage;
  alignment->score = r.score;
  alignment->winner = res.winner;
  alignment->n_hypotheses = H;
  alignment->n_survivors = res.survivors;
  alignment->n_edges_source = a.Es;
  alignment->n_edges_target = a.Et;
  alignment->n_lines_target = a.Lt;
  alignment->refine_steps = steps;
  alignment->status = res.winner >= 0 ? DGS_LA_ALIGNED : H == 0 ? DGS_LA_NO_HYPOTHESES : res.survivors == 0 ? DGS_LA_ALL_GATED : DGS_LA_NONE_BETTER;
  if (aligned_lines)
    for (size_t i = 0; i < aligned.size(); i++) {
      aligned_lines[i] = src_lines[i];   // transform_lines copies the line and replaces its two points
      la::store3(aligned_lines[i].point_a, aligned[i].a);
      la::store3(aligned_lines[i].point_b, aligned[i].b);
    }
  return DGS_OK;
}

int dgs_line_align_get_hypotheses(dgs_handle* h, int64_t first, int64_t count, dgs_line_align_hypothesis* records, int64_t* counts4) {
  if (!h || first < 0 || count < 0) return DGS_ERR_INVALID_ARGUMENT;
  LaScratch& s = h->la;
  if (counts4)
    for (int k = 0; k < 4; k++) counts4[k] = s.counts4[k];
  if (!records || count == 0) return DGS_OK;
  if (first + count > s.n_hyp) {
    h->err = "line align: the range lies beyond the last call's hypotheses";
    return DGS_ERR_INVALID_ARGUMENT;
  }
  const size_t n = (size_t)count;
  std::vector<LaHyp> hy(n);
  std::vector<unsigned char> g(n);
  std::vector<int> sl(n);
  std::vector<double> f(n * 5);
  DGS_HIP_TRY(h, hipSetDevice(h->device));
  DGS_HIP_TRY(h, hipMemcpyAsync(hy.data(), s.hyps.ptr + first, n * sizeof(LaHyp), hipMemcpyDeviceToHost, h->stream));
  DGS_HIP_TRY(h, hipMemcpyAsync(g.data(), s.gate.ptr + first, n, hipMemcpyDeviceToHost, h->stream));
  DGS_HIP_TRY(h, hipMemcpyAsync(sl.data(), s.slot.ptr + first, n * sizeof(int), hipMemcpyDeviceToHost, h->stream));
  DGS_HIP_TRY(h, hipMemcpyAsync(f.data(), s.fit.ptr + first * 5, n * 5 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  DGS_HIP_TRY(h, hipStreamSynchronize(h->stream));
  for (size_t i = 0; i < n; i++) {
    dgs_line_align_hypothesis& r = records[i];
    r.gate = g[i];
    r.slot = sl[i];
    r.rotation[0] = hy[i].t.r00; r.rotation[1] = hy[i].t.r01; r.rotation[2] = hy[i].t.r10; r.rotation[3] = hy[i].t.r11;
    r.translation[0] = hy[i].t.tx; r.translation[1] = hy[i].t.ty; r.translation[2] = hy[i].t.tz;
    for (int k = 0; k < 4; k++) r.fitness_score[k] = f[5 * i + k];
    r.score = f[5 * i + 4];
  }
  return DGS_OK;
}

}  // extern "C"
