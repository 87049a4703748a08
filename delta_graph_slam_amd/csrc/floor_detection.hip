// FloorDetectionNodelet::detect (upstream apps/floor_detection_nodelet.cpp:110-238) on the device: the tilt transform, the two plane
// clips, the k = 10 normal filter, the back-transform, a RANSAC plane fit (pcl::RandomSampleConsensus over
// pcl::SampleConsensusModelPlane, driven directly: PCL's defaults, no refit) and the nodelet's three checks.
//
// MI355X design
//   * fd_tilt_clip_kernel transforms a point and takes both clip decisions in one pass; the kept points are compacted in order by the
//     prefilter's stable compaction (pf_count_kernel, pf_scan_kernel, pf_scatter_kernel).
//   * The normal pass is the prefilter's: an index of the detector's own over the clipped cloud, gicp.hip's exact k-NN lists and
//     pf_normal_kernel, unchanged.  fd_normal_flag_kernel applies the floor rule to the normals it wrote.
//   * The draw stream does not depend on any count, so the host builds the draw list from n alone and uploads it.  fd_prepare_kernel (one
//     workgroup) tests every draw, compacts the good ones in order into hypotheses (four plane coefficients) and finds the draw that
//     completes max_sample_checks bad ones in a row, if any.
//   * fd_score_kernel scores a chunk of hypotheses against every point: a workgroup holds a tile of 1024 points in registers and walks
//     64 hypotheses, whose four floats sit at wave-uniform addresses; an inlier count is one ballot and popcount per wave, gathered per
//     workgroup in LDS and added to the hypothesis' global count with one vector atomic.
//   * RandomSampleConsensus::computeModel's walk runs on the host over the counts that come back (upstream's own libm for pow and log).
//     With a floor in view it ends after a handful of hypotheses, so the first launch scores hyp_chunk_first of them and further chunks
//     of hyp_chunk are launched only while the walk is open: one host wait per chunk, one in the common case.
//   * The filtered cloud comes back with the first chunk; the winner's inlier list and the checks are host work.
// Semantics and the PCL 1.10 details recalled from upstream: DESIGN.md §6j.
#include <algorithm>
#include <cfloat>
#include <climits>
#include <cmath>
#include <cstring>
#include <random>

#include "handle.h"
#include "nn_group.h"

namespace dgs {

// the prefilter's stable compaction and its normal pass (prefilter.hip)
__global__ void pf_count_kernel(const unsigned char* __restrict__ flags, const int n, int* __restrict__ blk);
__global__ void pf_scan_kernel(int* __restrict__ blk, const int nb, int* __restrict__ total);
__global__ void pf_scatter_kernel(const float4* __restrict__ in, const unsigned char* __restrict__ flags, const int n, const int* __restrict__ blk,
                                  float4* __restrict__ out, const int flatten);
__global__ void pf_normal_kernel(const BvhView b, const float4* __restrict__ pts, const int n, const int k, const int* __restrict__ nbr, const float vx,
                                 const float vy, const float vz, unsigned char* __restrict__ flags, float4* __restrict__ normals, float* __restrict__ cov9);

constexpr int kFdTilePoints = 4;         // points per lane of fd_score_kernel
constexpr int kFdTile = kFdTilePoints * kBlock;
constexpr int kFdHypSub = 64;            // hypotheses per workgroup of fd_score_kernel (blockIdx.y)
constexpr int kFdOneBlock = 1024;
constexpr int kFdNormalK = 10;           // ne.setKSearch(10) (:219)
constexpr int kFdDrawSlack = 64;         // draws beyond max_iterations + 1 in the first list

struct FdHyp {
  float c[4];
  int draw, i0, i1, i2;
};

struct FdMat {
  float m[16];   // row-major
};

// a four-term float dot product, the terms associated as plane_dot_order says
__host__ __device__ __forceinline__ float fd_dot4(const float a0, const float a1, const float a2, const float a3, const float b0, const float b1,
                                                  const float b2, const float b3, const int order) {
#pragma clang fp contract(off)
  const float x = a0 * b0, y = a1 * b1, z = a2 * b2, w = a3 * b3;
  return order == 0 ? (x + y) + (z + w) : order == 1 ? (x + z) + (y + w) : ((x + y) + z) + w;
}

// countWithinDistance / selectWithinDistance: |dot4(coefficients, (x, y, z, 1))| < threshold, compared in double
__host__ __device__ __forceinline__ bool fd_is_inlier(const float4 p, const float a, const float b, const float c, const float d, const int order,
                                                      const double thr) {
  return (double)fabsf(fd_dot4(a, b, c, d, p.x, p.y, p.z, 1.0f, order)) < thr;
}

// pcl::transformPointCloud(Matrix4f): a non-finite point goes through the arithmetic, the fourth float becomes 1
__device__ __forceinline__ float4 fd_transform(const float4 p, const FdMat& M, const int order) {
#pragma clang fp contract(off)
  float4 q;
  const float* m = M.m;
  if (order == 0) {
    q.x = p.x * m[0] + (p.y * m[1] + (p.z * m[2] + m[3]));
    q.y = p.x * m[4] + (p.y * m[5] + (p.z * m[6] + m[7]));
    q.z = p.x * m[8] + (p.y * m[9] + (p.z * m[10] + m[11]));
  } else {
    q.x = ((m[0] * p.x + m[1] * p.y) + m[2] * p.z) + m[3];
    q.y = ((m[4] * p.x + m[5] * p.y) + m[6] * p.z) + m[7];
    q.z = ((m[8] * p.x + m[9] * p.y) + m[10] * p.z) + m[11];
  }
  q.w = 1.0f;
  return q;
}

// ================================================================================================ filter stage
// tilt, then plane_clip twice (:117-119): PlaneClipper3D keeps a point whose float distance ((0*x + 0*y) + 1*z) + d is >= 0; the second
// clip is negated
__global__ __launch_bounds__(kBlock) void fd_tilt_clip_kernel(const float4* __restrict__ in, const int n, const FdMat M, const int order, const float hi,
                                                              const float lo, float4* __restrict__ out, unsigned char* __restrict__ flags) {
#pragma clang fp contract(off)
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const float4 q = fd_transform(in[i], M, order);
  const float base = (0.0f * q.x + 0.0f * q.y) + 1.0f * q.z;
  const float dhi = base + hi, dlo = base + lo;
  out[i] = q;
  flags[i] = (dhi >= 0.0f && !(dlo >= 0.0f)) ? 1 : 0;
}

// normal_filtering's rule (:227-228) over the normals pf_normal_kernel wrote: kept iff |n.z| > cos(normal_filter_thresh) in double; a NaN
// normal fails the comparison
__global__ __launch_bounds__(kBlock) void fd_normal_flag_kernel(const float4* __restrict__ normals, const int n, const double cos_thr,
                                                                unsigned char* __restrict__ flags) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  flags[i] = ((double)fabsf(normals[i].z) > cos_thr) ? 1 : 0;
}

__global__ __launch_bounds__(kBlock) void fd_transform_kernel(const float4* __restrict__ in, const int n, const FdMat M, const int order,
                                                              float4* __restrict__ out) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  out[i] = fd_transform(in[i], M, order);
}

// ================================================================================================ hypotheses
// One workgroup over the D draws in chunks of 1024, in order: good flag, rank among the good ones, distance to the last good one
// (ln_prepare_kernel's scheme).  SampleConsensusModelPlane::isSampleGood and computeModelCoefficients.
__global__ __launch_bounds__(kFdOneBlock) void fd_prepare_kernel(const float4* __restrict__ pts, const int n, const int* __restrict__ draws, const int D,
                                                                 const int bad_run, const int order, const int max_hyp, FdHyp* __restrict__ hyps,
                                                                 int* __restrict__ counts, int* __restrict__ meta) {
#pragma clang fp contract(off)
  __shared__ int s_w[kFdOneBlock / kWave], s_l[kFdOneBlock / kWave];
  __shared__ int s_rank, s_last, s_fail;
  const int lane = threadIdx.x & (kWave - 1), wv = threadIdx.x / kWave;
  if (threadIdx.x == 0) { s_rank = 0; s_last = -1; s_fail = INT_MAX; }
  for (int j = threadIdx.x; j < max_hyp; j += kFdOneBlock) counts[j] = 0;
  __syncthreads();
  for (int base = 0; base < D; base += kFdOneBlock) {
    const int d = base + threadIdx.x;
    bool good = false;
    int i0 = 0, i1 = 0, i2 = 0;
    float4 p0 = make_float4(0.f, 0.f, 0.f, 0.f), p1 = p0, p2 = p0;
    if (d < D) {
      i0 = draws[3 * d];
      i1 = draws[3 * d + 1];
      i2 = draws[3 * d + 2];
      if (i0 >= 0 && i0 < n && i1 >= 0 && i1 < n && i2 >= 0 && i2 < n) {
        p0 = pts[i0];
        p1 = pts[i1];
        p2 = pts[i2];
        // dy1dy2 = (p1 - p0) / (p2 - p0), component-wise; good iff its x, y, z are not all equal (NaN compares unequal)
        const float rx = (p1.x - p0.x) / (p2.x - p0.x), ry = (p1.y - p0.y) / (p2.y - p0.y), rz = (p1.z - p0.z) / (p2.z - p0.z);
        good = rx != ry || rz != ry;
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
    if (d < D && !good && d - last == bad_run) atomicMin(&s_fail, d);
    if (good && rank < max_hyp) {
      const float ux = p1.x - p0.x, uy = p1.y - p0.y, uz = p1.z - p0.z;
      const float vx = p2.x - p0.x, vy = p2.y - p0.y, vz = p2.z - p0.z;
      float a = uy * vz - uz * vy;
      float b = uz * vx - ux * vz;
      float c = ux * vy - uy * vx;
      // model_coefficients.normalize(): divided by sqrt(squaredNorm) when that is > 0
      const float s2 = fd_dot4(a, b, c, 0.f, a, b, c, 0.f, order);
      if (s2 > 0.f) {
        const float s = sqrtf(s2);
        a = a / s; b = b / s; c = c / s;
      }
      FdHyp hy;
      hy.c[0] = a; hy.c[1] = b; hy.c[2] = c;
      hy.c[3] = -1.0f * fd_dot4(a, b, c, 0.f, p0.x, p0.y, p0.z, p0.w, order);
      hy.draw = d; hy.i0 = i0; hy.i1 = i1; hy.i2 = i2;
      hyps[rank] = hy;   // rank < max_hyp: `hyps` holds max_hyp records
    }
    __syncthreads();
    if (threadIdx.x == kFdOneBlock - 1) {
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

// grid (tiles of 1024 points, groups of 64 hypotheses of the chunk [h_first, h_end))
__global__ __launch_bounds__(kBlock) void fd_score_kernel(const float4* __restrict__ pts, const int n, const FdHyp* __restrict__ hyps,
                                                          const int* __restrict__ meta, const int max_hyp, const int h_first, const int h_end,
                                                          const int order, const double thr, int* __restrict__ counts) {
  __shared__ int s_cnt[kFdHypSub];
  const int H = min(min(meta[0], max_hyp), h_end);
  const int h0 = h_first + blockIdx.y * kFdHypSub;
  if (h0 >= H) return;   // uniform per workgroup
  const int h1 = min(h0 + kFdHypSub, H);
  if (threadIdx.x < kFdHypSub) s_cnt[threadIdx.x] = 0;
  float4 p[kFdTilePoints];
  bool ok[kFdTilePoints];
#pragma unroll
  for (int k = 0; k < kFdTilePoints; k++) {
    const long long i = (long long)blockIdx.x * kFdTile + k * kBlock + threadIdx.x;
    ok[k] = i < n;
    p[k] = ok[k] ? pts[i] : make_float4(0.f, 0.f, 0.f, 0.f);
  }
  __syncthreads();
  const int lane = threadIdx.x & (kWave - 1);
  for (int hh = h0; hh < h1; hh++) {
    const FdHyp* hy = hyps + hh;   // the same address in every lane
    const float a = hy->c[0], b = hy->c[1], c = hy->c[2], d = hy->c[3];
    int cnt = 0;
#pragma unroll
    for (int k = 0; k < kFdTilePoints; k++) cnt += __popcll(__ballot(ok[k] && fd_is_inlier(p[k], a, b, c, d, order, thr)));
    if (lane == 0 && cnt) atomicAdd(&s_cnt[hh - h0], cnt);
  }
  __syncthreads();
  if ((int)threadIdx.x < h1 - h0 && s_cnt[threadIdx.x]) atomicAdd(&counts[h0 + threadIdx.x], s_cnt[threadIdx.x]);   // h0 + threadIdx.x < h1 <= max_hyp
}

// ================================================================================================ host side
namespace {

inline unsigned fd_blocks(int64_t n) { return (unsigned)((n + kBlock - 1) / kBlock); }

// the sample stream: SampleConsensusModel::drawIndexSample on an identity permutation `s` of at least n entries that carries over
// between draws, D times; `s` is the identity again on return
void fd_draws(std::vector<int>& s, const uint32_t* raw, int64_t n, int64_t D, int* out) {
  std::vector<int> touched;
  touched.reserve((size_t)D * 3);
  for (int64_t d = 0; d < D; d++) {
    for (int i = 0; i < 3; i++) {
      const int j = i + (int)(raw[3 * d + i] % (uint32_t)(n - i));
      std::swap(s[(size_t)i], s[(size_t)j]);
      touched.push_back(j);
    }
    out[3 * d] = s[0];
    out[3 * d + 1] = s[1];
    out[3 * d + 2] = s[2];
  }
  s[0] = 0; s[1] = 1; s[2] = 2;
  for (int t : touched) s[(size_t)t] = t;
}

void fd_grow_perm(std::vector<int>& s, int64_t n) {
  if ((int64_t)s.size() >= n) return;
  const size_t old = s.size();
  s.resize((size_t)n);
  for (size_t i = old; i < (size_t)n; i++) s[i] = (int)i;
}

void fd_grow_mt(std::vector<uint32_t>& v, int64_t count) {   // boost::mt19937(12345)() >> 1 from the seed on
  if ((int64_t)v.size() >= count) return;
  std::mt19937 gen(12345u);
  v.resize((size_t)count);
  for (uint32_t& x : v) x = (uint32_t)gen() >> 1;
}

// RandomSampleConsensus::computeModel's walk: k = 1, best = -INT_MAX, while it < k; a strictly greater count takes over and resets k;
// after ++it the loop stops once it > max_iterations.  step() consumes one hypothesis.
struct FdWalk {
  int it = 0, best = -INT_MAX, win = -1;
  double k = 1.0;
  bool open() const { return (double)it < k; }
  // -> false when the loop broke at it > max_iterations
  bool step(int count, int64_t n, int max_iterations, double log_one_minus_p) {
    if (count > best) {
      best = count;
      win = it;
      const double w = (double)count / (double)n;
      double p_no_outliers = 1.0 - std::pow(w, 3.0);
      p_no_outliers = std::max(DBL_EPSILON, p_no_outliers);
      p_no_outliers = std::min(1.0 - DBL_EPSILON, p_no_outliers);
      k = log_one_minus_p / std::log(p_no_outliers);
    }
    ++it;
    return !(it > max_iterations);
  }
};

// count + scan + scatter of fd.flags over n points of `in` into `out`; *m = kept points (read back: the host waits here)
int fd_compact(dgs_handle* h, const float4* in, int64_t n, DevBuf<float4>& out, int64_t* m) {
  FdScratch& fd = h->fd;
  *m = 0;
  if (n == 0) return DGS_OK;
  const unsigned nb = fd_blocks(n);
  DGS_HIP_TRY(h, out.reserve((size_t)n));
  DGS_HIP_TRY(h, fd.blk.reserve(nb));
  DGS_HIP_TRY(h, fd.cnt.reserve(4));
  hipLaunchKernelGGL(pf_count_kernel, dim3(nb), dim3(kBlock), 0, h->stream, fd.flags.ptr, (int)n, fd.blk.ptr);
  hipLaunchKernelGGL(pf_scan_kernel, dim3(1), dim3(kFdOneBlock), 0, h->stream, fd.blk.ptr, (int)nb, fd.cnt.ptr);
  hipLaunchKernelGGL(pf_scatter_kernel, dim3(nb), dim3(kBlock), 0, h->stream, in, fd.flags.ptr, (int)n, fd.blk.ptr, out.ptr, 0);
  DGS_HIP_TRY(h, hipGetLastError());
  if (ensure_pinned(h, 4096) != DGS_OK) return DGS_ERR_HIP;
  int* hc = reinterpret_cast<int*>(h->pinned);
  DGS_HIP_TRY(h, hipMemcpyAsync(hc, fd.cnt.ptr, sizeof(int), hipMemcpyDeviceToHost, h->stream));
  DGS_HIP_TRY(h, hipStreamSynchronize(h->stream));
  *m = hc[0];
  return DGS_OK;
}

FdMat fd_mat(const float* col16) {
  FdMat M;
  for (int r = 0; r < 4; r++)
    for (int c = 0; c < 4; c++) M.m[4 * r + c] = col16[4 * c + r];
  return M;
}

// steps 1-4: -> the filtered cloud in fd.filtered, its size in *nf
int fd_filter(dgs_handle* h, const dgs_floor_detection_params& p, const float* tilt16, const float* tilt_inv16, const float4* in, int64_t n, int64_t* nf) {
  FdScratch& fd = h->fd;
  *nf = 0;
  fd.n_clipped = fd.n_filtered = 0;
  fd.have_normals = false;
  if (n == 0) return DGS_OK;
  DGS_HIP_TRY(h, fd.flags.reserve((size_t)n));
  DGS_HIP_TRY(h, fd.tilted.reserve((size_t)n));
  const float hi = (float)(p.sensor_height + p.height_clip_range), lo = (float)(p.sensor_height - p.height_clip_range);
  hipLaunchKernelGGL(fd_tilt_clip_kernel, dim3(fd_blocks(n)), dim3(kBlock), 0, h->stream, in, (int)n, fd_mat(tilt16), p.transform_order, hi, lo,
                     fd.tilted.ptr, fd.flags.ptr);
  int64_t nc = 0;
  if (int rc = fd_compact(h, fd.tilted.ptr, n, fd.clipped, &nc)) return rc;
  fd.n_clipped = nc;
  const float4* kept = fd.clipped.ptr;
  int64_t nk = nc;
  if (p.use_normal_filtering && nc > 0) {
    CloudState& c = fd.cloud;
    DGS_HIP_TRY(h, c.pts.reserve((size_t)nc));
    DGS_HIP_TRY(h, hipMemcpyAsync(c.pts.ptr, fd.clipped.ptr, (size_t)nc * sizeof(float4), hipMemcpyDeviceToDevice, h->stream));
    c.n = nc;
    c.invalidate();
    DGS_HIP_TRY(h, fd.normals.reserve((size_t)nc));
    DGS_HIP_TRY(h, fd.cov9.reserve((size_t)nc * 9));
    DGS_HIP_TRY(h, fd.nflags.reserve((size_t)nc));
    const int k = (int)std::min<int64_t>(kFdNormalK, nc);   // FLANN returns min(k, n) neighbours
    if (int rc = knn_lists(h, c, k, &fd.nbr)) return rc;
    // ne.setViewPoint(0.0f, 0.0f, sensor_height) (:220)
    hipLaunchKernelGGL(pf_normal_kernel, dim3(fd_blocks(nc)), dim3(kBlock), 0, h->stream, make_bvh_view(c.bvh), c.pts.ptr, (int)nc, k, fd.nbr.ptr, 0.0f,
                       0.0f, (float)p.sensor_height, fd.nflags.ptr, fd.normals.ptr, fd.cov9.ptr);
    hipLaunchKernelGGL(fd_normal_flag_kernel, dim3(fd_blocks(nc)), dim3(kBlock), 0, h->stream, fd.normals.ptr, (int)nc,
                       std::cos(p.normal_filter_thresh * M_PI / 180.0), fd.flags.ptr);
    fd.have_normals = true;
    if (int rc = fd_compact(h, fd.clipped.ptr, nc, fd.kept, &nk)) return rc;
    kept = fd.kept.ptr;
  }
  if (nk > 0) {
    DGS_HIP_TRY(h, fd.filtered.reserve((size_t)nk));
    hipLaunchKernelGGL(fd_transform_kernel, dim3(fd_blocks(nk)), dim3(kBlock), 0, h->stream, kept, (int)nk, fd_mat(tilt_inv16), p.transform_order,
                       fd.filtered.ptr);
    DGS_HIP_TRY(h, hipGetLastError());
  }
  fd.n_filtered = nk;
  *nf = nk;
  return DGS_OK;
}

enum { FD_WALK_DONE = 0, FD_WALK_NEED_DRAWS = 1 };

// steps 5-8 over fd.filtered (n >= 3 points) with a draw list of D draws: the walk's end state in fd.trace, the winner's coefficients in
// coeffs, the filtered cloud in fd.host_filtered.  *outcome = FD_WALK_NEED_DRAWS when the walk ran past the list.
int fd_ransac(dgs_handle* h, const dgs_floor_detection_params& p, int64_t n, const uint32_t* raw, int64_t D, int* outcome, float* coeffs) {
  FdScratch& fd = h->fd;
  dgs_floor_detection_trace& tr = fd.trace;
  const int max_hyp = p.max_iterations + 1;
  // pinned block: meta | hypotheses | counts | filtered cloud | draw list
  const size_t off_hyp = 64, off_cnt = off_hyp + (size_t)max_hyp * sizeof(FdHyp), off_cloud = (off_cnt + (size_t)max_hyp * sizeof(int) + 63) / 64 * 64;
  const size_t off_draws = off_cloud + (size_t)n * sizeof(float4);
  if (ensure_pinned(h, off_draws + (size_t)D * 3 * sizeof(int)) != DGS_OK) return DGS_ERR_HIP;
  char* pin = static_cast<char*>(h->pinned);
  int* h_meta = reinterpret_cast<int*>(pin);
  FdHyp* h_hyp = reinterpret_cast<FdHyp*>(pin + off_hyp);
  int* h_cnt = reinterpret_cast<int*>(pin + off_cnt);
  int* h_draws = reinterpret_cast<int*>(pin + off_draws);
  DGS_HIP_TRY(h, fd.draws.reserve((size_t)D * 3));
  DGS_HIP_TRY(h, fd.hyps.reserve((size_t)max_hyp));
  DGS_HIP_TRY(h, fd.counts.reserve((size_t)max_hyp));
  DGS_HIP_TRY(h, fd.meta.reserve(4));
  fd_grow_perm(fd.perm, n);
  fd_draws(fd.perm, raw, n, D, h_draws);
  DGS_HIP_TRY(h, hipMemcpyAsync(fd.draws.ptr, h_draws, (size_t)D * 3 * sizeof(int), hipMemcpyHostToDevice, h->stream));
  hipLaunchKernelGGL(fd_prepare_kernel, dim3(1), dim3(kFdOneBlock), 0, h->stream, fd.filtered.ptr, (int)n, fd.draws.ptr, (int)D, p.max_sample_checks,
                     p.plane_dot_order, max_hyp, fd.hyps.ptr, fd.counts.ptr, fd.meta.ptr);
  DGS_HIP_TRY(h, hipMemcpyAsync(pin + off_cloud, fd.filtered.ptr, (size_t)n * sizeof(float4), hipMemcpyDeviceToHost, h->stream));

  FdWalk wk;
  const double log_one_minus_p = std::log(1.0 - p.probability);
  int scored = 0, chunks = 0, H = 0, fail_at = INT_MAX, draws = 0;
  bool failed = false, need = false;
  while (wk.open()) {
    if (wk.it >= scored) {
      if (chunks > 0 && scored >= H) {   // no further good draw in the list: a run of bad ones completed, or the list is too short
        if (fail_at < D) { failed = true; draws = fail_at + 1; } else { need = true; draws = (int)D; }
        break;
      }
      const int h_end = (int)std::min<int64_t>(max_hyp, (int64_t)scored + (chunks == 0 ? p.hyp_chunk_first : p.hyp_chunk));
      hipLaunchKernelGGL(fd_score_kernel, dim3((unsigned)((n + kFdTile - 1) / kFdTile), (unsigned)((h_end - scored + kFdHypSub - 1) / kFdHypSub)), dim3(kBlock),
                         0, h->stream, fd.filtered.ptr, (int)n, fd.hyps.ptr, fd.meta.ptr, max_hyp, scored, h_end, p.plane_dot_order, p.distance_threshold,
                         fd.counts.ptr);
      DGS_HIP_TRY(h, hipGetLastError());
      DGS_HIP_TRY(h, hipMemcpyAsync(h_meta, fd.meta.ptr, 2 * sizeof(int), hipMemcpyDeviceToHost, h->stream));
      DGS_HIP_TRY(h, hipMemcpyAsync(h_hyp + scored, fd.hyps.ptr + scored, (size_t)(h_end - scored) * sizeof(FdHyp), hipMemcpyDeviceToHost, h->stream));
      DGS_HIP_TRY(h, hipMemcpyAsync(h_cnt + scored, fd.counts.ptr + scored, (size_t)(h_end - scored) * sizeof(int), hipMemcpyDeviceToHost, h->stream));
      DGS_HIP_TRY(h, hipStreamSynchronize(h->stream));
      chunks++;
      H = std::min(h_meta[0], max_hyp);
      fail_at = h_meta[1];
      scored = std::min(h_end, H);
      continue;
    }
    if (h_hyp[wk.it].draw > fail_at) {   // getSamples returned an empty selection before this hypothesis' draw: the loop breaks
      failed = true;
      draws = fail_at + 1;
      break;
    }
    draws = h_hyp[wk.it].draw + 1;
    if (!wk.step(h_cnt[wk.it], n, p.max_iterations, log_one_minus_p)) break;
  }
  tr.draws = draws;
  tr.hypotheses_scored = scored;
  tr.iterations = wk.it;
  tr.chunks_launched = chunks;
  tr.ransac_failed = failed ? 1 : 0;
  *outcome = need ? FD_WALK_NEED_DRAWS : FD_WALK_DONE;
  if (need) return DGS_OK;
  fd.host_filtered.resize((size_t)n);
  std::memcpy(fd.host_filtered.data(), pin + off_cloud, (size_t)n * sizeof(float4));
  if (wk.win >= 0) {
    const FdHyp& w = h_hyp[wk.win];
    tr.winner_rank = wk.win;
    tr.sample[0] = w.i0; tr.sample[1] = w.i1; tr.sample[2] = w.i2;
    tr.count = wk.best;
    for (int a = 0; a < 4; a++) coeffs[a] = w.c[a];
  }
  return DGS_OK;
}

const char* fd_bad_params(const dgs_floor_detection_params* p) {
  if (!p) return "floor detection: params is NULL";
  if (p->struct_size != sizeof(dgs_floor_detection_params)) return "floor detection: wrong struct_size";
  if (p->floor_pts_thresh < 0) return "floor detection: floor_pts_thresh must not be negative (upstream compares it as size_t)";
  if (p->max_iterations < 0 || p->max_iterations > (1 << 20)) return "floor detection: max_iterations must lie in 0..1048576";
  if (p->max_sample_checks < 1) return "floor detection: max_sample_checks must be positive";
  if (p->transform_order < 0 || p->transform_order > 1) return "floor detection: unknown transform_order";
  if (p->plane_dot_order < 0 || p->plane_dot_order > 2) return "floor detection: unknown plane_dot_order";
  if (p->hyp_chunk_first < 1 || p->hyp_chunk < 1) return "floor detection: hyp_chunk_first and hyp_chunk must be positive";
  if (!(p->probability > 0.0 && p->probability < 1.0)) return "floor detection: probability must lie in (0, 1)";
  return nullptr;
}

int fd_detect(dgs_handle* h, const dgs_floor_detection_params& p, const float* tilt16, const float* tilt_inv16, const float* in_xyz16, int64_t n,
              int32_t in_on_device, const uint32_t* rng_raw, int64_t rng_len, float* coeffs4_out, int32_t* status_out) {
  FdScratch& fd = h->fd;
  dgs_floor_detection_trace& tr = fd.trace;
  std::memset(&tr, 0, sizeof(tr));
  tr.winner_rank = -1;
  tr.sample[0] = tr.sample[1] = tr.sample[2] = -1;
  fd.inliers.clear();
  fd.host_filtered.clear();
  fd.n_clipped = fd.n_filtered = 0;
  fd.have_normals = false;
  *status_out = DGS_FD_TOO_FEW_POINTS;
  if (n == 0) return DGS_OK;   // cloud_callback returns on an empty cloud (:76-78)
  const float4* in = reinterpret_cast<const float4*>(in_xyz16);
  if (!in_on_device) {
    DGS_HIP_TRY(h, fd.in.reserve((size_t)n));
    DGS_HIP_TRY(h, hipMemcpyAsync(fd.in.ptr, in_xyz16, (size_t)n * sizeof(float4), hipMemcpyHostToDevice, h->stream));
    in = fd.in.ptr;
  }
  int64_t nf = 0;
  if (int rc = fd_filter(h, p, tilt16, tilt_inv16, in, n, &nf)) return rc;
  tr.n_clipped = (int32_t)fd.n_clipped;
  tr.n_filtered = (int32_t)nf;
  if (nf < (int64_t)p.floor_pts_thresh) return DGS_OK;   // too few points for RANSAC (:133)

  float coeffs[4] = {0.f, 0.f, 0.f, 0.f};
  if (nf < 3) {   // getSamples: fewer points than the sample size, the selection is empty and the loop breaks at once
    tr.ransac_failed = 1;
    fd.host_filtered.resize((size_t)nf);
    if (nf > 0) {
      DGS_HIP_TRY(h, hipMemcpyAsync(fd.host_filtered.data(), fd.filtered.ptr, (size_t)nf * sizeof(float4), hipMemcpyDeviceToHost, h->stream));
      DGS_HIP_TRY(h, hipStreamSynchronize(h->stream));
    }
  } else {
    const int max_hyp = p.max_iterations + 1;
    const int64_t avail = rng_raw ? rng_len / 3 : INT32_MAX / 4;
    int64_t D = std::min<int64_t>(avail, (int64_t)max_hyp + kFdDrawSlack);
    for (;;) {
      if (D < 1) { *status_out = DGS_FD_RNG_EXHAUSTED; return DGS_OK; }
      const uint32_t* raw = rng_raw;
      if (!rng_raw) {
        fd_grow_mt(fd.mt_raw, 3 * D);
        raw = fd.mt_raw.data();
      }
      int outcome = FD_WALK_DONE;
      if (int rc = fd_ransac(h, p, nf, raw, D, &outcome, coeffs)) return rc;
      if (outcome == FD_WALK_DONE) break;
      if (D >= avail) { *status_out = DGS_FD_RNG_EXHAUSTED; return DGS_OK; }
      D = std::min<int64_t>(avail, std::min<int64_t>(D * 4, (int64_t)max_hyp * p.max_sample_checks + p.max_sample_checks));
    }
  }
  // selectWithinDistance of the winner, in index order; no model: empty inliers
  if (tr.winner_rank >= 0) {
    for (int64_t i = 0; i < nf; i++)
      if (fd_is_inlier(fd.host_filtered[(size_t)i], coeffs[0], coeffs[1], coeffs[2], coeffs[3], p.plane_dot_order, p.distance_threshold))
        fd.inliers.push_back((int32_t)i);
  }
  for (int a = 0; a < 4; a++) tr.raw_coeffs[a] = coeffs[a];
  if ((int64_t)fd.inliers.size() < (int64_t)p.floor_pts_thresh) { *status_out = DGS_FD_TOO_FEW_INLIERS; return DGS_OK; }   // :147
  {
#pragma clang fp contract(off)
    // reference = tilt_matrix.inverse() * UnitZ: the third column (:152); the dot product in float, compared in double (:157-158)
    const float rx = tilt_inv16[8], ry = tilt_inv16[9], rz = tilt_inv16[10];
    const float dot = (coeffs[0] * rx + coeffs[1] * ry) + coeffs[2] * rz;
    tr.dot = dot;
    if (std::abs((double)dot) < std::cos(p.floor_normal_thresh * M_PI / 180.0)) { *status_out = DGS_FD_NOT_VERTICAL; return DGS_OK; }
    // make the normal upward (:164-166)
    const float up = (0.0f * coeffs[0] + 0.0f * coeffs[1]) + 1.0f * coeffs[2];
    if (up < 0.0f)
      for (int a = 0; a < 4; a++) coeffs[a] = coeffs[a] * -1.0f;
  }
  for (int a = 0; a < 4; a++) coeffs4_out[a] = coeffs[a];
  *status_out = DGS_FD_DETECTED;
  return DGS_OK;
}

}  // namespace

void floor_detection_release(dgs_handle* h) {
  FdScratch& fd = h->fd;
  for (DevBuf<float4>* b : {&fd.in, &fd.tilted, &fd.clipped, &fd.kept, &fd.filtered, &fd.normals}) b->release();
  fd.flags.release(); fd.nflags.release(); fd.blk.release(); fd.cnt.release(); fd.nbr.release(); fd.cov9.release(); fd.draws.release();
  fd.hyps.release(); fd.counts.release(); fd.meta.release();
  fd.cloud.release();
  fd.host_filtered.clear(); fd.inliers.clear();
  fd.n_clipped = fd.n_filtered = 0;
}

}  // namespace dgs

using namespace dgs;

extern "C" {

int dgs_floor_detection_params_init(dgs_floor_detection_params* p) {
  if (!p) return DGS_ERR_INVALID_ARGUMENT;
  std::memset(p, 0, sizeof(*p));
  p->struct_size = sizeof(*p);
  p->tilt_deg = 0.0;
  p->sensor_height = 2.0;
  p->height_clip_range = 1.0;
  p->floor_pts_thresh = 512;
  p->floor_normal_thresh = 10.0;
  p->use_normal_filtering = 1;
  p->normal_filter_thresh = 20.0;
  p->distance_threshold = 0.1;
  p->max_iterations = 1000;
  p->probability = 0.99;
  p->max_sample_checks = 1000;
  p->transform_order = 0;
  p->plane_dot_order = 0;
  p->hyp_chunk_first = 64;
  p->hyp_chunk = 512;
  return DGS_OK;
}

int dgs_floor_detection(dgs_handle* h, const dgs_floor_detection_params* params, const float* tilt16, const float* tilt_inv16, const float* in_xyz16,
                        int64_t n, int32_t in_on_device, const uint32_t* rng_raw, int64_t rng_len, float* coeffs4_out, int32_t* status_out) {
  if (const char* why = fd_bad_params(params)) {   // before anything touches a device
    if (h) h->err = why;
    return DGS_ERR_INVALID_ARGUMENT;
  }
  if (!h || !tilt16 || !tilt_inv16 || !coeffs4_out || !status_out || n < 0 || n > INT32_MAX || (n > 0 && !in_xyz16) || rng_len < 0 ||
      (rng_len > 0 && !rng_raw))
    return DGS_ERR_INVALID_ARGUMENT;
  for (int a = 0; a < 4; a++) coeffs4_out[a] = 0.f;
  h->err.clear();
  DGS_HIP_TRY(h, hipSetDevice(h->device));
  const int rc = fd_detect(h, *params, tilt16, tilt_inv16, in_xyz16, n, in_on_device, rng_len > 0 ? rng_raw : nullptr, rng_len, coeffs4_out, status_out);
  if (rc != DGS_OK) {
    (void)hipStreamSynchronize(h->stream);
    return rc;
  }
  DGS_HIP_TRY(h, hipStreamSynchronize(h->stream));   // a staged host input may go away after the call
  return DGS_OK;
}

int dgs_floor_detection_get_filtered(dgs_handle* h, float* out_xyz16, int64_t capacity, int32_t out_on_device, int64_t* n) {
  if (!h || !n || capacity < 0) return DGS_ERR_INVALID_ARGUMENT;
  const int64_t m = h->fd.n_filtered;
  *n = m;
  if (m == 0 || !out_xyz16 || capacity < m) return DGS_OK;
  DGS_HIP_TRY(h, hipSetDevice(h->device));
  DGS_HIP_TRY(h, hipMemcpyAsync(out_xyz16, h->fd.filtered.ptr, (size_t)m * sizeof(float4), out_on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost,
                                h->stream));
  DGS_HIP_TRY(h, hipStreamSynchronize(h->stream));
  return DGS_OK;
}

int dgs_floor_detection_get_inliers(dgs_handle* h, int32_t* indices, float* points_xyz16, int64_t capacity, int64_t* n) {
  if (!h || !n || capacity < 0) return DGS_ERR_INVALID_ARGUMENT;
  const FdScratch& fd = h->fd;
  const int64_t m = (int64_t)fd.inliers.size();
  *n = m;
  if (m == 0 || capacity < m) return DGS_OK;
  if (indices) std::memcpy(indices, fd.inliers.data(), (size_t)m * sizeof(int32_t));
  if (points_xyz16)
    for (int64_t j = 0; j < m; j++) std::memcpy(points_xyz16 + 4 * j, &fd.host_filtered[(size_t)fd.inliers[(size_t)j]], sizeof(float4));
  return DGS_OK;
}

int dgs_floor_detection_get_trace(dgs_handle* h, dgs_floor_detection_trace* trace) {
  if (!h || !trace) return DGS_ERR_INVALID_ARGUMENT;
  *trace = h->fd.trace;
  return DGS_OK;
}

int dgs_floor_detection_get_clipped(dgs_handle* h, float* clipped_xyz16, float* normals4, int64_t capacity, int64_t* n) {
  if (!h || !n || capacity < 0) return DGS_ERR_INVALID_ARGUMENT;
  const FdScratch& fd = h->fd;
  const int64_t m = fd.n_clipped;
  *n = m;
  if (m == 0 || capacity < m) return DGS_OK;
  DGS_HIP_TRY(h, hipSetDevice(h->device));
  if (clipped_xyz16) DGS_HIP_TRY(h, hipMemcpyAsync(clipped_xyz16, fd.clipped.ptr, (size_t)m * sizeof(float4), hipMemcpyDeviceToHost, h->stream));
  if (normals4 && fd.have_normals)
    DGS_HIP_TRY(h, hipMemcpyAsync(normals4, fd.normals.ptr, (size_t)m * sizeof(float4), hipMemcpyDeviceToHost, h->stream));
  DGS_HIP_TRY(h, hipStreamSynchronize(h->stream));
  return DGS_OK;
}

int dgs_floor_detection_draws(int64_t n, const uint32_t* rng_raw, int64_t n_draws, int32_t* triples_out) {
  if (n < 3 || n > INT32_MAX || n_draws < 0 || n_draws > (1 << 24) || (n_draws > 0 && !triples_out)) return DGS_ERR_INVALID_ARGUMENT;
  std::vector<int> perm;
  fd_grow_perm(perm, n);
  std::vector<uint32_t> mt;
  if (!rng_raw) {
    fd_grow_mt(mt, 3 * n_draws);
    rng_raw = mt.data();
  }
  fd_draws(perm, rng_raw, n, n_draws, triples_out);
  return DGS_OK;
}

int dgs_floor_detection_walk(int64_t n, int32_t max_iterations, double probability, const int32_t* counts, int64_t n_counts, int32_t* winner_out,
                             int32_t* iterations_out, int32_t* open_out) {
  if (n < 1 || max_iterations < 0 || !(probability > 0.0 && probability < 1.0) || n_counts < 0 || (n_counts > 0 && !counts) || !winner_out ||
      !iterations_out || !open_out)
    return DGS_ERR_INVALID_ARGUMENT;
  FdWalk wk;
  const double log_one_minus_p = std::log(1.0 - probability);
  bool broke = false;
  while (wk.open() && wk.it < n_counts) {
    if (!wk.step(counts[wk.it], n, max_iterations, log_one_minus_p)) { broke = true; break; }
  }
  *winner_out = wk.win;
  *iterations_out = wk.it;
  *open_out = (!broke && wk.open()) ? 1 : 0;
  return DGS_OK;
}

}  // extern "C"
