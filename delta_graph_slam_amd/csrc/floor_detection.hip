// FloorDetectionNodelet::detect (upstream apps/floor_detection_nodelet.cpp:110-238) on the device: the tilt transform, the two plane
// clips, the k = 10 normal filter, the back-transform, a RANSAC plane fit (pcl::RandomSampleConsensus over
// pcl::SampleConsensusModelPlane, driven directly: PCL's defaults, no refit) and the nodelet's three checks.
//
// MI355X design
//   * fd_tilt_clip_kernel transforms a point and takes both clip decisions in one pass; the kept points are compacted in order by the
//     shared stable compaction (compact.h: pf_count_kernel, pf_scan_kernel, pf_scatter_kernel).
//   * The normal pass is the prefilter's: an index of the detector's own over the clipped cloud, knn_lists.hip's exact k-NN lists and
//     pf_normal_kernel, unchanged.  fd_normal_flag_kernel applies the floor rule to the normals it wrote.
//   * The RANSAC is sac.h's, shared with the line extraction, over FdModel (the plane's sample test, four coefficients and inlier test).
//     The draw stream does not depend on any count, so the host builds the draw list from n alone and uploads it;
//     sac_prepare_kernel<FdModel> turns it into hypotheses and sac_score_kernel<FdModel, 64> scores a chunk of them against every point.
//   * RandomSampleConsensus::computeModel's walk (SacWalk) runs on the host over the counts that come back (upstream's own libm for pow
//     and log).  With a floor in view it ends after a handful of hypotheses, so the first launch scores hyp_chunk_first of them and
//     further chunks of hyp_chunk are launched only while the walk is open: one host wait per chunk, one in the common case.
//   * The filtered cloud comes back with the first chunk; the winner's inlier list and the checks are host work.
// Semantics and the PCL 1.10 details recalled from upstream: DESIGN.md §6j.
#include <algorithm>
#include <cfloat>
#include <climits>
#include <cmath>
#include <cstring>
#include "compact.h"
#include "floor_detection_body.h"
#include "floor_detection_plan.h"
#include "handle.h"
#include "nn_group.h"
#include "sac.h"

namespace dgs {

// the prefilter's normal pass (prefilter.hip)
__global__ void pf_normal_kernel(const BvhView b, const float4* __restrict__ pts, const int n, const int k, const int* __restrict__ nbr, const float vx,
                                 const float vy, const float vz, unsigned char* __restrict__ flags, float4* __restrict__ normals, float* __restrict__ cov9);

// ================================================================================================ filter stage
// the bodies, the transform and the plane model: floor_detection_body.h, shared with floor_detection_batch.hip
__global__ __launch_bounds__(kBlock) void fd_tilt_clip_kernel(const float4* __restrict__ in, const int n, const FdMat M, const int order, const float hi,
                                                              const float lo, float4* __restrict__ out, unsigned char* __restrict__ flags) {
  fd_tilt_clip_body(in, n, M, order, hi, lo, out, flags, (int)blockIdx.x);
}

__global__ __launch_bounds__(kBlock) void fd_normal_flag_kernel(const float4* __restrict__ normals, const int n, const double cos_thr,
                                                                unsigned char* __restrict__ flags) {
  fd_normal_flag_body(normals, n, cos_thr, flags, (int)blockIdx.x);
}

__global__ __launch_bounds__(kBlock) void fd_transform_kernel(const float4* __restrict__ in, const int n, const FdMat M, const int order,
                                                              float4* __restrict__ out) {
  fd_transform_body(in, n, M, order, out, (int)blockIdx.x);
}


// ================================================================================================ host side
namespace {

// steps 1-4: -> the filtered cloud in fd.filtered, its size in *nf
int fd_filter(dgs_handle* h, const dgs_floor_detection_params& p, const float* tilt16, const float* tilt_inv16, const float4* in, int64_t n, int64_t* nf) {
  FdScratch& fd = h->fd;
  *nf = 0;
  fd.scan.n_clipped = fd.scan.n_filtered = 0;
  fd.scan.have_normals = false;
  if (n == 0) return DGS_OK;
  DGS_HIP_TRY(h, fd.flags.reserve((size_t)n));
  DGS_HIP_TRY(h, fd.tilted.reserve((size_t)n));
  const float hi = (float)(p.sensor_height + p.height_clip_range), lo = (float)(p.sensor_height - p.height_clip_range);
  hipLaunchKernelGGL(fd_tilt_clip_kernel, dim3(compact_blocks(n)), dim3(kBlock), 0, h->stream, in, (int)n, fd_mat(tilt16), p.transform_order, hi, lo,
                     fd.tilted.ptr, fd.flags.ptr);
  int64_t nc = 0;
  if (int rc = compact_points(h, fd.tilted.ptr, fd.flags.ptr, n, fd.blk, fd.cnt, fd.clipped, false, &nc)) return rc;
  fd.scan.n_clipped = nc;
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
    hipLaunchKernelGGL(pf_normal_kernel, dim3(compact_blocks(nc)), dim3(kBlock), 0, h->stream, make_bvh_view(c.bvh), c.pts.ptr, (int)nc, k, fd.nbr.ptr, 0.0f,
                       0.0f, (float)p.sensor_height, fd.nflags.ptr, fd.normals.ptr, fd.cov9.ptr);
    hipLaunchKernelGGL(fd_normal_flag_kernel, dim3(compact_blocks(nc)), dim3(kBlock), 0, h->stream, fd.normals.ptr, (int)nc,
                       std::cos(p.normal_filter_thresh * M_PI / 180.0), fd.flags.ptr);
    fd.scan.have_normals = true;
    if (int rc = compact_points(h, fd.clipped.ptr, fd.flags.ptr, nc, fd.blk, fd.cnt, fd.kept, false, &nk)) return rc;
    kept = fd.kept.ptr;
  }
  if (nk > 0) {
    DGS_HIP_TRY(h, fd.filtered.reserve((size_t)nk));
    hipLaunchKernelGGL(fd_transform_kernel, dim3(compact_blocks(nk)), dim3(kBlock), 0, h->stream, kept, (int)nk, fd_mat(tilt_inv16), p.transform_order,
                       fd.filtered.ptr);
    DGS_HIP_TRY(h, hipGetLastError());
  }
  fd.scan.n_filtered = nk;
  *nf = nk;
  return DGS_OK;
}

}  // namespace

bool fd_walk_to_trace(const fdplan::ScanWalk& w, const FdHyp* hyps, dgs_floor_detection_trace& tr, float* coeffs) {
  const SacWalk& wk = w.wk;
  tr.draws = wk.draws;
  tr.hypotheses_scored = w.scored;
  tr.iterations = wk.it;
  tr.chunks_launched = w.chunks;
  tr.ransac_failed = wk.status == SAC_FAILED ? 1 : 0;
  if (wk.status == SAC_NEED_DRAWS) return false;
  if (wk.win >= 0) {
    const FdHyp& win = hyps[wk.win];
    tr.winner_rank = wk.win;
    tr.sample[0] = win.i0; tr.sample[1] = win.i1; tr.sample[2] = win.i2;
    tr.count = wk.best;
    for (int a = 0; a < 4; a++) coeffs[a] = win.c[a];
  }
  return true;
}

namespace {

// steps 5-8 over `pts` (n >= 3 points) with a draw list of D draws: one score launch and one host wait per chunk of hypotheses the walk
// asks for.  -> the walk's end state in tr, the winner's coefficients in coeffs, the filtered cloud in *host_cloud; *need_draws when
// the walk ran past the list.
int fd_ransac(dgs_handle* h, const dgs_floor_detection_params& p, const float4* pts, int64_t n, const uint32_t* raw, int64_t D, SacScratch& sac,
              DevBuf<FdHyp>& hyps, dgs_floor_detection_trace& tr, std::vector<float4>* host_cloud, bool* need_draws, float* coeffs) {
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
  DGS_HIP_TRY(h, sac.draws.reserve((size_t)D * 3));
  DGS_HIP_TRY(h, hyps.reserve((size_t)max_hyp));
  DGS_HIP_TRY(h, sac.counts.reserve((size_t)max_hyp));
  DGS_HIP_TRY(h, sac.meta.reserve(4));
  sac_grow_perm(sac.perm, n);
  sac_draws<3>(sac.perm, raw, n, D, h_draws);
  DGS_HIP_TRY(h, hipMemcpyAsync(sac.draws.ptr, h_draws, (size_t)D * 3 * sizeof(int), hipMemcpyHostToDevice, h->stream));
  const FdModel::Params prm{p.plane_dot_order, p.max_sample_checks, p.distance_threshold};
  hipLaunchKernelGGL(sac_prepare_kernel<FdModel>, dim3(1), dim3(kSacPrepareBlock), 0, h->stream, pts, (int)n, sac.draws.ptr, (int)D, prm,
                     max_hyp, hyps.ptr, sac.counts.ptr, sac.meta.ptr);
  DGS_HIP_TRY(h, hipMemcpyAsync(pin + off_cloud, pts, (size_t)n * sizeof(float4), hipMemcpyDeviceToHost, h->stream));

  fdplan::ScanWalk w;
  w.n = n;
  w.D = D;
  const double log_one_minus_p = std::log(1.0 - p.probability);
  while (w.advance(h_hyp, h_cnt, p.max_iterations, p.hyp_chunk_first, p.hyp_chunk, log_one_minus_p, FdModel::ratio_power)) {
    const int h0 = w.h_first, hc = w.h_end - w.h_first;   // h0 = the hypotheses scored so far: only the new chunk comes down
    hipLaunchKernelGGL((sac_score_kernel<FdModel, kFdHypSub>), dim3((unsigned)((n + kSacTile - 1) / kSacTile), (unsigned)((hc + kFdHypSub - 1) / kFdHypSub)),
                       dim3(kBlock), 0, h->stream, pts, (int)n, hyps.ptr, sac.meta.ptr, max_hyp, h0, w.h_end, prm, sac.counts.ptr);
    DGS_HIP_TRY(h, hipGetLastError());
    DGS_HIP_TRY(h, hipMemcpyAsync(h_meta, sac.meta.ptr, 2 * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    DGS_HIP_TRY(h, hipMemcpyAsync(h_hyp + h0, hyps.ptr + h0, (size_t)hc * sizeof(FdHyp), hipMemcpyDeviceToHost, h->stream));
    DGS_HIP_TRY(h, hipMemcpyAsync(h_cnt + h0, sac.counts.ptr + h0, (size_t)hc * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    DGS_HIP_TRY(h, hipStreamSynchronize(h->stream));
    w.scored_round(h_meta[0], h_meta[1], max_hyp);
  }
  *need_draws = !fd_walk_to_trace(w, h_hyp, tr, coeffs);
  if (*need_draws) return DGS_OK;
  host_cloud->resize((size_t)n);
  std::memcpy(host_cloud->data(), pin + off_cloud, (size_t)n * sizeof(float4));
  return DGS_OK;
}

}  // namespace

int fd_ransac_lists(dgs_handle* h, const dgs_floor_detection_params& p, const float4* pts, int64_t n, const uint32_t* rng_raw, SacDrawPlan& plan,
                    SacScratch& sac, DevBuf<FdHyp>& hyps, FdScan& sc, float* coeffs, bool* exhausted, StageCounts* did) {
  for (*exhausted = false;;) {
    const uint32_t* raw = rng_raw;
    if (!raw) {
      sac_grow_mt(sac.mt_raw, 3 * plan.D);
      raw = sac.mt_raw.data();
    }
    bool need_draws = false;
    if (int rc = fd_ransac(h, p, pts, n, raw, plan.D, sac, hyps, sc.trace, &sc.host_filtered, &need_draws, coeffs)) return rc;
    did->launches += 1 + sc.trace.chunks_launched;   // the prepare launch and one score launch per chunk
    did->waits += sc.trace.chunks_launched;
    if (!need_draws) return DGS_OK;
    if (!plan.grow()) {
      *exhausted = true;
      return DGS_OK;
    }
  }
}

void fd_select_inliers(FdScan& sc, const dgs_floor_detection_params& p, const float* c) {
  // read once: the compiler cannot tell that push_back leaves them alone, and the single call runs this loop inside its timed path
  const float4* pts = sc.host_filtered.data();
  const int64_t n = (int64_t)sc.host_filtered.size();
  const float a = c[0], b = c[1], cz = c[2], d = c[3];
  const int order = p.plane_dot_order;
  const double thr = p.distance_threshold;
  for (int64_t i = 0; i < n; i++)
    if (fd_is_inlier(pts[i], a, b, cz, d, order, thr)) sc.inliers.push_back((int32_t)i);
}

void fd_verdict(FdScan& sc, const dgs_floor_detection_params& p, const float* tilt_inv16, const float* coeffs, int64_t inliers) {
  dgs_floor_detection_trace& tr = sc.trace;
  sc.status = fdplan::verdict(tr.winner_rank >= 0 ? coeffs : nullptr, inliers, tilt_inv16, p.floor_pts_thresh, p.floor_normal_thresh, tr.raw_coeffs, &tr.dot,
                              sc.coeffs);
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

namespace {

// -> fd.scan: its status, coefficients, trace, host cloud and inliers
int fd_detect(dgs_handle* h, const dgs_floor_detection_params& p, const float* tilt16, const float* tilt_inv16, const float* in_xyz16, int64_t n,
              int32_t in_on_device, const uint32_t* rng_raw, int64_t rng_len) {
  FdScratch& fd = h->fd;
  FdScan& sc = fd.scan;
  dgs_floor_detection_trace& tr = sc.trace;
  sc.reset();   // DGS_FD_TOO_FEW_POINTS
  sc.n = n;
  if (n == 0) return DGS_OK;   // cloud_callback returns on an empty cloud (:76-78)
  const float4* in = reinterpret_cast<const float4*>(in_xyz16);
  if (!in_on_device) {
    DGS_HIP_TRY(h, fd.in.reserve((size_t)n));
    DGS_HIP_TRY(h, hipMemcpyAsync(fd.in.ptr, in_xyz16, (size_t)n * sizeof(float4), hipMemcpyHostToDevice, h->stream));
    in = fd.in.ptr;
  }
  int64_t nf = 0;
  if (int rc = fd_filter(h, p, tilt16, tilt_inv16, in, n, &nf)) return rc;
  tr.n_clipped = (int32_t)sc.n_clipped;
  tr.n_filtered = (int32_t)nf;
  if (!fdplan::reaches_ransac(n, nf, p.floor_pts_thresh)) return DGS_OK;   // too few points for RANSAC (:133)

  float coeffs[4] = {0.f, 0.f, 0.f, 0.f};
  if (nf < 3) {   // getSamples: fewer points than the sample size, the selection is empty and the loop breaks at once
    tr.ransac_failed = 1;
    sc.host_filtered.resize((size_t)nf);
    if (nf > 0) {
      DGS_HIP_TRY(h, hipMemcpyAsync(sc.host_filtered.data(), fd.filtered.ptr, (size_t)nf * sizeof(float4), hipMemcpyDeviceToHost, h->stream));
      DGS_HIP_TRY(h, hipStreamSynchronize(h->stream));
    }
  } else {
    SacDrawPlan plan(rng_raw ? rng_len / 3 : INT32_MAX / 4, p.max_iterations + 1, p.max_sample_checks);
    bool exhausted = plan.empty();
    StageCounts did;   // the single call reports no counts
    if (!exhausted)
      if (int rc = fd_ransac_lists(h, p, fd.filtered.ptr, nf, rng_raw, plan, fd.sac, fd.hyps, sc, coeffs, &exhausted, &did)) return rc;
    if (exhausted) {
      sc.status = DGS_FD_RNG_EXHAUSTED;
      return DGS_OK;
    }
  }
  // selectWithinDistance of the winner, in index order; no model: empty inliers
  if (tr.winner_rank >= 0) fd_select_inliers(sc, p, coeffs);
  fd_verdict(sc, p, tilt_inv16, coeffs, (int64_t)sc.inliers.size());
  return DGS_OK;
}

}  // namespace

void floor_detection_release(dgs_handle* h) {
  FdScratch& fd = h->fd;
  for (DevBuf<float4>* b : {&fd.in, &fd.tilted, &fd.clipped, &fd.kept, &fd.filtered, &fd.normals}) b->release();
  fd.flags.release(); fd.nflags.release(); fd.blk.release(); fd.cnt.release(); fd.nbr.release(); fd.cov9.release(); fd.hyps.release();
  fd.sac.release();
  fd.cloud.release();
  fd.scan.host_filtered.clear(); fd.scan.inliers.clear();
  fd.scan.n_clipped = fd.scan.n_filtered = 0;
}

// ---- the getters of the single call and the batch: sc = the scan's record, or nullptr when there is no such scan
int fd_get_filtered(dgs_handle* h, const FdScan* sc, const float4* d_filtered, float* out_xyz16, int64_t capacity, int32_t out_on_device, int64_t* n) {
  if (!sc || !n || capacity < 0) return DGS_ERR_INVALID_ARGUMENT;
  const int64_t m = sc->n_filtered;
  *n = m;
  if (m == 0 || !out_xyz16 || capacity < m) return DGS_OK;
  DGS_HIP_TRY(h, hipSetDevice(h->device));
  DGS_HIP_TRY(h, hipMemcpyAsync(out_xyz16, d_filtered, (size_t)m * sizeof(float4), out_on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, h->stream));
  DGS_HIP_TRY(h, hipStreamSynchronize(h->stream));
  return DGS_OK;
}

int fd_get_inliers(const FdScan* sc, int32_t* indices, float* points_xyz16, int64_t capacity, int64_t* n) {
  if (!sc || !n || capacity < 0) return DGS_ERR_INVALID_ARGUMENT;
  const int64_t m = (int64_t)sc->inliers.size();
  *n = m;
  if (m == 0 || capacity < m) return DGS_OK;
  if (indices) std::memcpy(indices, sc->inliers.data(), (size_t)m * sizeof(int32_t));
  if (points_xyz16)
    for (int64_t j = 0; j < m; j++) std::memcpy(points_xyz16 + 4 * j, &sc->host_filtered[(size_t)sc->inliers[(size_t)j]], sizeof(float4));
  return DGS_OK;
}

int fd_get_trace(const FdScan* sc, dgs_floor_detection_trace* trace) {
  if (!sc || !trace) return DGS_ERR_INVALID_ARGUMENT;
  *trace = sc->trace;
  return DGS_OK;
}

int fd_get_clipped(dgs_handle* h, const FdScan* sc, const float4* d_clipped, const float4* d_normals, float* clipped_xyz16, float* normals4, int64_t capacity,
                   int64_t* n) {
  if (!sc || !n || capacity < 0) return DGS_ERR_INVALID_ARGUMENT;
  const int64_t m = sc->n_clipped;
  *n = m;
  if (m == 0 || capacity < m) return DGS_OK;
  DGS_HIP_TRY(h, hipSetDevice(h->device));
  if (clipped_xyz16) DGS_HIP_TRY(h, hipMemcpyAsync(clipped_xyz16, d_clipped, (size_t)m * sizeof(float4), hipMemcpyDeviceToHost, h->stream));
  if (normals4 && sc->have_normals) DGS_HIP_TRY(h, hipMemcpyAsync(normals4, d_normals, (size_t)m * sizeof(float4), hipMemcpyDeviceToHost, h->stream));
  DGS_HIP_TRY(h, hipStreamSynchronize(h->stream));
  return DGS_OK;
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
  *status_out = DGS_FD_TOO_FEW_POINTS;
  const int rc = fd_detect(h, *params, tilt16, tilt_inv16, in_xyz16, n, in_on_device, rng_len > 0 ? rng_raw : nullptr, rng_len);
  if (rc != DGS_OK) {
    (void)hipStreamSynchronize(h->stream);
    return rc;
  }
  DGS_HIP_TRY(h, hipStreamSynchronize(h->stream));   // a staged host input may go away after the call
  *status_out = h->fd.scan.status;
  for (int a = 0; a < 4; a++) coeffs4_out[a] = h->fd.scan.coeffs[a];
  return DGS_OK;
}

int dgs_floor_detection_get_filtered(dgs_handle* h, float* out_xyz16, int64_t capacity, int32_t out_on_device, int64_t* n) {
  if (!h) return DGS_ERR_INVALID_ARGUMENT;
  return fd_get_filtered(h, &h->fd.scan, h->fd.filtered.ptr, out_xyz16, capacity, out_on_device, n);
}
int dgs_floor_detection_get_inliers(dgs_handle* h, int32_t* indices, float* points_xyz16, int64_t capacity, int64_t* n) {
  if (!h) return DGS_ERR_INVALID_ARGUMENT;
  return fd_get_inliers(&h->fd.scan, indices, points_xyz16, capacity, n);
}
int dgs_floor_detection_get_trace(dgs_handle* h, dgs_floor_detection_trace* trace) {
  if (!h) return DGS_ERR_INVALID_ARGUMENT;
  return fd_get_trace(&h->fd.scan, trace);
}
int dgs_floor_detection_get_clipped(dgs_handle* h, float* clipped_xyz16, float* normals4, int64_t capacity, int64_t* n) {
  if (!h) return DGS_ERR_INVALID_ARGUMENT;
  return fd_get_clipped(h, &h->fd.scan, h->fd.clipped.ptr, h->fd.normals.ptr, clipped_xyz16, normals4, capacity, n);
}

int dgs_floor_detection_draws(int64_t n, const uint32_t* rng_raw, int64_t n_draws, int32_t* triples_out) {
  if (n < 3 || n > INT32_MAX || n_draws < 0 || n_draws > (1 << 24) || (n_draws > 0 && !triples_out)) return DGS_ERR_INVALID_ARGUMENT;
  std::vector<int> perm;
  sac_grow_perm(perm, n);
  std::vector<uint32_t> mt;
  if (!rng_raw) {
    sac_grow_mt(mt, 3 * n_draws);
    rng_raw = mt.data();
  }
  sac_draws<3>(perm, rng_raw, n, n_draws, triples_out);
  return DGS_OK;
}

int dgs_floor_detection_walk(int64_t n, int32_t max_iterations, double probability, const int32_t* counts, int64_t n_counts, int32_t* winner_out,
                             int32_t* iterations_out, int32_t* open_out) {
  if (n < 1 || max_iterations < 0 || !(probability > 0.0 && probability < 1.0) || n_counts < 0 || (n_counts > 0 && !counts) || !winner_out ||
      !iterations_out || !open_out)
    return DGS_ERR_INVALID_ARGUMENT;
  SacWalk wk;
  const double log_one_minus_p = std::log(1.0 - probability);
  bool broke = false;
  while (wk.open() && wk.it < n_counts) {
    if (!wk.step(counts[wk.it], n, max_iterations, log_one_minus_p, FdModel::ratio_power)) { broke = true; break; }
  }
  *winner_out = wk.win;
  *iterations_out = wk.it;
  *open_out = (!broke && wk.open()) ? 1 : 0;
  return DGS_OK;
}

}  // extern "C"
