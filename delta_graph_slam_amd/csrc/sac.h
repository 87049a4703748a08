// The parts of pcl::RandomSampleConsensus / pcl::SampleConsensusModel that do not depend on the model, restated once for the line
// extraction (SampleConsensusModelLine, 2-point samples) and the floor detection (SampleConsensusModelPlane, 3-point samples).
// Three sections:
//   * host, plain C++17: the draw stream (drawIndexSample over boost::mt19937(12345)() >> 1 or the caller's raw values) and the size
//     policy of a draw list.
//   * host and device: computeModel's walk over the inlier counts and its bookkeeping around a draw list (SacWalk).  The line
//     extraction runs it on the device, the floor detection on the host.
//   * device: the prepare kernel (draws -> hypotheses in order) and the score kernel (inliers per hypothesis) over a Model.
// A Model is a struct of the stage's own file with
//   kSample                       points per sample
//   Hyp                           the hypothesis record; Hyp::draw is the draw it came from
//   Params                        what both kernels pass through to the model
//   bad_run(prm)                  SampleConsensusModel::max_sample_checks_
//   good(prm, p)                  isSampleGood over the kSample sampled points
//   make(prm, p, d, idx)          computeModelCoefficients -> Hyp of draw d, sample indices idx
//   Coef, coef(hyp)               the coefficients the inlier test reads, in registers
//   inlier(prm, point, coef)      the countWithinDistance predicate
// All arithmetic on points and coefficients is the model's, under its own file's flags: the two kernels hold no floating point.
#pragma once

#include <algorithm>
#include <cfloat>
#include <climits>
#include <cmath>
#include <cstdint>
#include <random>
#include <vector>

#if defined(__HIPCC__)
#include "common.h"
#define SAC_HD __host__ __device__ __forceinline__
#else
#define SAC_HD inline
#endif

namespace dgs {

// ================================================================================================ draw stream (host)
// SampleConsensusModel::drawIndexSample for K-point samples, D times, on the identity permutation `perm` of at least n >= K entries that
// carries over between draws: for i < K, j = i + raw[K * d + i] % (n - i), swap.  -> K indices per draw in `out`; `perm` is the identity
// again on return.
template <int K>
inline void sac_draws(std::vector<int>& perm, const uint32_t* raw, int64_t n, int64_t D, int* out) {
  std::vector<int> touched;
  touched.reserve((size_t)D * K);
  for (int64_t d = 0; d < D; d++) {
    for (int i = 0; i < K; i++) {
      const int j = i + (int)(raw[K * d + i] % (uint32_t)(n - i));
      std::swap(perm[(size_t)i], perm[(size_t)j]);
      touched.push_back(j);
    }
    for (int i = 0; i < K; i++) out[K * d + i] = perm[(size_t)i];
  }
  for (int i = 0; i < K; i++) perm[(size_t)i] = i;
  for (int t : touched) perm[(size_t)t] = t;
}

inline void sac_grow_perm(std::vector<int>& perm, int64_t n) {
  if ((int64_t)perm.size() >= n) return;
  const size_t old = perm.size();
  perm.resize((size_t)n);
  for (size_t i = old; i < (size_t)n; i++) perm[i] = (int)i;
}

inline void sac_grow_mt(std::vector<uint32_t>& v, int64_t count) {   // boost::mt19937(12345)() >> 1 from the seed on
  if ((int64_t)v.size() >= count) return;
  std::mt19937 gen(12345u);
  v.resize((size_t)count);
  for (uint32_t& x : v) x = (uint32_t)gen() >> 1;
}

// The size of a draw list.  The walk needs at most max_hyp = max_iterations + 1 good draws, so the first list holds max_hyp + 64 draws;
// a list the walk ran past grows fourfold, up to max_hyp * bad_run + bad_run (a full run of bad draws in front of every hypothesis and
// one behind); `avail` draws of the caller's stream bound both.
struct SacDrawPlan {
  int64_t avail, cap, D;
  SacDrawPlan(int64_t avail_, int max_hyp, int bad_run)
      : avail(avail_), cap((int64_t)max_hyp * bad_run + bad_run), D(std::min<int64_t>(avail_, (int64_t)max_hyp + 64)) {}
  bool empty() const { return D < 1; }   // the caller's stream holds no draw at all
  bool grow() {                          // -> false: the caller's stream is exhausted
    if (D >= avail) return false;
    D = std::min<int64_t>(avail, std::min<int64_t>(D * 4, cap));
    return true;
  }
};

// ================================================================================================ computeModel's walk (host and device)
enum { SAC_OK = 0, SAC_FAILED = 1, SAC_NEED_DRAWS = 2 };

// RandomSampleConsensus::computeModel over the hypotheses of a draw list in order: k = 1, best = -INT_MAX, while it < k; a strictly
// greater count takes over and resets k; after ++it the loop stops once it > max_iterations.  A hypothesis goes through next() and then
// step(); `fail_at` is the draw that completes bad_run bad ones in a row (INT_MAX: none).
struct SacWalk {
  int it = 0, best = -INT_MAX, win = -1;
  int status = SAC_OK, draws = 0;   // draws: how many draws upstream's loop consumed
  double k = 1.0;
  SAC_HD bool open() const { return (double)it < k; }
  // the list of D draws holds no further hypothesis: a run of bad ones completed, or the list is too short
  SAC_HD void end_of_list(int fail_at, int D) {
    status = fail_at < D ? SAC_FAILED : SAC_NEED_DRAWS;
    draws = fail_at < D ? fail_at + 1 : D;
  }
  // the next hypothesis came from draw `draw` -> false when getSamples returned an empty selection before it: the loop breaks
  SAC_HD bool next(int draw, int fail_at) {
    if (draw > fail_at) {
      status = SAC_FAILED;
      draws = fail_at + 1;
      return false;
    }
    draws = draw + 1;
    return true;
  }
  // its inlier count -> false when the loop broke at it > max_iterations.  power(w) is the model's w^kSample as upstream writes it.
  template <class Power>
  SAC_HD bool step(int count, int64_t n, int max_iterations, double log_one_minus_p, Power power) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    if (count > best) {
      best = count;
      win = it;
      const double w = (double)count / (double)n;
      double p_no_outliers = 1.0 - power(w);
      p_no_outliers = p_no_outliers < DBL_EPSILON ? DBL_EPSILON : p_no_outliers;                  // (std::max)(epsilon, p)
      p_no_outliers = p_no_outliers > 1.0 - DBL_EPSILON ? 1.0 - DBL_EPSILON : p_no_outliers;      // (std::min)(1 - epsilon, p)
      k = log_one_minus_p / std::log(p_no_outliers);
    }
    ++it;
    return !(it > max_iterations);
  }
};

#if defined(__HIPCC__)
// ================================================================================================ scratch
struct SacScratch {
  DevBuf<int> draws;                   // kSample point indices per draw
  DevBuf<int> counts, meta;            // inliers per hypothesis; [0] good draws, [1] draw that completes bad_run bad ones in a row
  std::vector<uint32_t> mt_raw;        // mt19937(12345)() >> 1, extended on demand
  std::vector<int> perm;               // identity between calls: shuffled_indices_
  void release() { draws.release(); counts.release(); meta.release(); }
};

// ================================================================================================ kernels
constexpr int kSacPrepareBlock = 1024;   // sac_prepare_kernel's workgroup and chunk
constexpr int kSacTilePoints = 4;        // points per lane of sac_score_kernel
constexpr int kSacTile = kSacTilePoints * kBlock;

// One workgroup over the D draws in chunks of 1024, in order: good flag, rank among the good ones, distance to the last good one.  The
// good draws become hyps[0 .. min(good draws, max_hyp)) in order; counts[0 .. max_hyp) = 0; meta[0] = good draws, meta[1] = the first draw
// that completes bad_run bad ones in a row (INT_MAX: none).
// The body: the whole workgroup of a launch over one list, or of a launch with one workgroup per list (floor_detection_batch.hip).
template <class Model>
__device__ __forceinline__ void sac_prepare_body(const float4* __restrict__ pts, const int n, const int* __restrict__ draws, const int D,
                                                 const typename Model::Params& prm, const int max_hyp, typename Model::Hyp* __restrict__ hyps,
                                                 int* __restrict__ counts, int* __restrict__ meta) {
  constexpr int K = Model::kSample;
  __shared__ int s_w[kSacPrepareBlock / kWave], s_l[kSacPrepareBlock / kWave];
  __shared__ int s_rank, s_last, s_fail;
  const int lane = threadIdx.x & (kWave - 1), wv = threadIdx.x / kWave;
  if (threadIdx.x == 0) { s_rank = 0; s_last = -1; s_fail = INT_MAX; }
  for (int j = threadIdx.x; j < max_hyp; j += kSacPrepareBlock) counts[j] = 0;
  __syncthreads();
  for (int base = 0; base < D; base += kSacPrepareBlock) {
    const int d = base + threadIdx.x;
    bool good = false;
    int idx[K];
    float4 p[K];
#pragma unroll
    for (int i = 0; i < K; i++) { idx[i] = 0; p[i] = make_float4(0.f, 0.f, 0.f, 0.f); }
    if (d < D) {
      bool inside = true;
#pragma unroll
      for (int i = 0; i < K; i++) {
        idx[i] = draws[K * d + i];
        inside = inside && idx[i] >= 0 && idx[i] < n;
      }
      if (inside) {
#pragma unroll
        for (int i = 0; i < K; i++) p[i] = pts[idx[i]];
        good = Model::good(prm, p);
      }
    }
    // rank among the good draws, and the last good draw at or before this one (inclusive max scan)
    const unsigned long long m = __ballot(good);
    const int below = __popcll(m & ((1ull << lane) - 1ull));
    int last = good ? d : -1;
#pragma unroll
    for (int o = 1; o < kWave; o <<= 1) {
      const int y = __shfl_up(last, o, kWave);
      if (lane >= o) last = max(last, y);
    }
    if (lane == kWave - 1) { s_w[wv] = __popcll(m); s_l[wv] = last; }
    __syncthreads();
    int rank = s_rank + below, prev = s_last;
    for (int w = 0; w < wv; w++) { rank += s_w[w]; prev = max(prev, s_l[w]); }
    last = max(last, prev);
    if (d < D && !good && d - last == Model::bad_run(prm)) atomicMin(&s_fail, d);
    if (good && rank < max_hyp) hyps[rank] = Model::make(prm, p, d, idx);   // rank < max_hyp: `hyps` holds max_hyp records
    __syncthreads();
    if (threadIdx.x == kSacPrepareBlock - 1) {
      s_rank = rank + (good ? 1 : 0);
      s_last = last;
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    meta[0] = s_rank;
    meta[1] = s_fail;
  }
}
template <class Model>
__global__ __launch_bounds__(kSacPrepareBlock) void sac_prepare_kernel(const float4* __restrict__ pts, const int n, const int* __restrict__ draws,
                                                                      const int D, const typename Model::Params prm, const int max_hyp,
                                                                      typename Model::Hyp* __restrict__ hyps, int* __restrict__ counts,
                                                                      int* __restrict__ meta) {
  sac_prepare_body<Model>(pts, n, draws, D, prm, max_hyp, hyps, counts, meta);
}

// grid (tiles of 1024 points, groups of kHypPerGroup hypotheses of the chunk [h_first, h_end)).  A workgroup holds its tile in registers
// and walks its hypotheses, whose coefficients sit at wave-uniform addresses; an inlier count is one ballot and popcount per wave,
// gathered per workgroup in LDS and added to the hypothesis' global count with one atomic.
// The body takes the workgroup's tile inside its own cloud and its group of hypotheses inside its own chunk: blockIdx.x and blockIdx.y
// of the launch over one cloud, or what a launch over the tiles of many clouds finds for the workgroup (floor_detection_batch.hip).
template <class Model, int kHypPerGroup>
__device__ __forceinline__ void sac_score_body(const float4* __restrict__ pts, const int n, const typename Model::Hyp* __restrict__ hyps,
                                               const int* __restrict__ meta, const int max_hyp, const int h_first, const int h_end,
                                               const typename Model::Params& prm, int* __restrict__ counts, const int tile, const int group) {
  __shared__ int s_cnt[kHypPerGroup];
  const int H = min(min(meta[0], max_hyp), h_end);
  const int h0 = h_first + group * kHypPerGroup;
  if (h0 >= H) return;   // uniform per workgroup
  const int h1 = min(h0 + kHypPerGroup, H);
  for (int j = threadIdx.x; j < kHypPerGroup; j += kBlock) s_cnt[j] = 0;
  float4 p[kSacTilePoints];
  bool ok[kSacTilePoints];
#pragma unroll
  for (int k = 0; k < kSacTilePoints; k++) {
    const long long i = (long long)tile * kSacTile + k * kBlock + threadIdx.x;
    ok[k] = i < n;
    p[k] = ok[k] ? pts[i] : make_float4(0.f, 0.f, 0.f, 0.f);
  }
  __syncthreads();
  const int lane = threadIdx.x & (kWave - 1);
  for (int hh = h0; hh < h1; hh++) {
    const typename Model::Coef c = Model::coef(hyps + hh);   // the same address in every lane
    int cnt = 0;
#pragma unroll
    for (int k = 0; k < kSacTilePoints; k++) cnt += __popcll(__ballot(ok[k] && Model::inlier(prm, p[k], c)));
    if (lane == 0 && cnt) atomicAdd(&s_cnt[hh - h0], cnt);
  }
  __syncthreads();
  for (int j = threadIdx.x; j < h1 - h0; j += kBlock)
    if (s_cnt[j]) atomicAdd(&counts[h0 + j], s_cnt[j]);   // h0 + j < h1 <= max_hyp
}
template <class Model, int kHypPerGroup>
__global__ __launch_bounds__(kBlock) void sac_score_kernel(const float4* __restrict__ pts, const int n, const typename Model::Hyp* __restrict__ hyps,
                                                           const int* __restrict__ meta, const int max_hyp, const int h_first, const int h_end,
                                                           const typename Model::Params prm, int* __restrict__ counts) {
  sac_score_body<Model, kHypPerGroup>(pts, n, hyps, meta, max_hyp, h_first, h_end, prm, counts, (int)blockIdx.x, (int)blockIdx.y);
}
#endif  // __HIPCC__

}  // namespace dgs
