// FloorDetectionNodelet::detect over MANY scans in one call (dgs_floor_detection_batch): the frames of several streams, one chain of
// launches and three host waits whatever their number.  Scan i receives, bit for bit, what dgs_floor_detection (floor_detection.hip)
// gives it alone; DESIGN.md §6v.
//
// Filter stages.  Every stage uploads one FdbSeg per scan that is still live; every scan owns whole workgroups, and a workgroup finds
// its scan by bisecting the launch's first workgroups with its blockIdx.x (seg_find, seg_device.h): scalar loads, the entry in SGPRs.
// From there on it is a workgroup of the single launch: the bodies of floor_detection_body.h with the scan's own arguments and the
// workgroup's number inside the scan.  Tilt and clip: one flag launch, one segmented compaction (compact.h, as prefilter_batch.hip
// runs it), host wait 1.  Normal filter: prefilter_batch_normal_stage over the clipped clouds in place (batched index build, batched
// k-NN search, pf_normal_body), then the floor rule's flag launch and a compaction, host wait 2.  One launch does the back-transform.
//
// RANSAC.  The host builds every scan's draw list from its n_filtered alone; all lists go up in one copy.  fdb_prepare_kernel: one
// 1024-lane workgroup per scan, sac_prepare_body over its list.  fdb_score_kernel, once per round: x = the 1,024-point tiles of all
// scans whose walk is open, y = the hypothesis groups of the round's longest chunk; the entry carries the scan's own [h_first, h_end)
// and a workgroup beyond it leaves at once.  Counts are integer atomics: every count is the single launch's.  After a round one host
// wait brings back meta, hypotheses and counts of all scans (three copies, the last two strided), and the host advances every walk as
// the single call does (fdplan::ScanWalk).  A walk that runs past its draw list is finished by fd_ransac_lists on the scan's own cloud.
//
// Decisions.  §6j's checks need the winner's inlier count, not the list: the walk's best count is that number (the score body and the
// host loop run fd_is_inlier, the same IEEE operations under the same flags, over the same points), so nothing is downloaded.  A
// scan's filtered cloud comes to the host and its inlier list is made when a getter asks.
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <vector>

#include "compact.h"
#include "floor_detection_plan.h"
#include "floor_detection_body.h"
#include "handle.h"
#include "seg_device.h"
#include "seg_table.h"

namespace dgs {

static_assert(fdplan::kTile == kSacTile && fdplan::kHypGroup == kFdHypSub, "floor_detection_plan.h restates the score launch's tile and group");
static_assert(pfbplan::kPlanBlock == kBlock, "prefilter_batch_plan.h restates the workgroup of the per-point passes");
static_assert(fdplan::kDetected == DGS_FD_DETECTED && fdplan::kTooFewPoints == DGS_FD_TOO_FEW_POINTS && fdplan::kTooFewInliers == DGS_FD_TOO_FEW_INLIERS &&
                  fdplan::kNotVertical == DGS_FD_NOT_VERTICAL && fdplan::kRngExhausted == DGS_FD_RNG_EXHAUSTED,
              "floor_detection_plan.h restates the statuses");

struct FdbSeg {
  const float4* in;        // tilt: the raw scan; floor rule: the normals; back-transform: the kept points
  float4* src;             // what the compaction reads: the tilted points (the tilt pass writes them) / the clipped cloud
  float4* out;             // the compaction's or the back-transform's output: room for n points
  unsigned char* flags;    // the scan's flags: the shared array + blk0 * 256
  int n, blk0;             // points; first workgroup in the stage's launches
  int pad[2];
};
static_assert(sizeof(FdbSeg) == 48, "one entry is three 16-byte scalar loads");

struct FdbSac {
  const float4* pts;       // the scan's filtered cloud
  const int* draws;        // its draw list
  FdHyp* hyps;             // its max_hyp records
  int* counts;             // its max_hyp counts
  int* meta;               // its 4 ints
  int n, D;
  int h_first, h_end;      // the chunk this round scores
  int tile0, pad;          // first workgroup (x) in the round's score launch
};
static_assert(sizeof(FdbSac) == 64, "one entry is four 16-byte scalar loads");

// ---- filter stages -------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void fdb_tilt_clip_kernel(const FdbSeg* __restrict__ tab, const int* __restrict__ first, const int m, const FdMat M,
                                                               const int order, const float hi, const float lo) {
  const FdbSeg& e = tab[seg_find(first, m, (int)blockIdx.x)];
  fd_tilt_clip_body(e.in, e.n, M, order, hi, lo, e.src, e.flags, (int)blockIdx.x - e.blk0);
}
__global__ __launch_bounds__(kBlock) void fdb_normal_flag_kernel(const FdbSeg* __restrict__ tab, const int* __restrict__ first, const int m, const double cos_thr) {
  const FdbSeg& e = tab[seg_find(first, m, (int)blockIdx.x)];
  fd_normal_flag_body(e.in, e.n, cos_thr, e.flags, (int)blockIdx.x - e.blk0);
}
__global__ __launch_bounds__(kBlock) void fdb_transform_kernel(const FdbSeg* __restrict__ tab, const int* __restrict__ first, const int m, const FdMat M,
                                                               const int order) {
  const FdbSeg& e = tab[seg_find(first, m, (int)blockIdx.x)];
  fd_transform_body(e.in, e.n, M, order, e.out, (int)blockIdx.x - e.blk0);
}
// the scatter of the segmented stable compaction (compact.h; its count launch is compact_count_seg_kernel<FdbSeg>)
__global__ __launch_bounds__(kBlock) void fdb_scatter_kernel(const FdbSeg* __restrict__ tab, const int* __restrict__ first, const int m, const int* __restrict__ blk,
                                                             int* __restrict__ totals) {
  const int c = seg_find(first, m, (int)blockIdx.x);
  const FdbSeg& e = tab[c];
  compact_scatter_seg<int>(e, c, first, blk, totals, [&](const int i, const int off) { e.out[off] = e.src[i]; });   // `out` holds n points
}

// ---- RANSAC ----------------------------------------------------------------------------------------------------------------------
// one workgroup per scan: sac_prepare_kernel<FdModel> over the scan's own list
__global__ __launch_bounds__(kSacPrepareBlock) void fdb_prepare_kernel(const FdbSac* __restrict__ tab, const FdModel::Params prm, const int max_hyp) {
  const FdbSac& e = tab[blockIdx.x];
  sac_prepare_body<FdModel>(e.pts, e.n, e.draws, e.D, prm, max_hyp, e.hyps, e.counts, e.meta);
}
// grid (tiles of all open scans, hypothesis groups of the longest chunk): sac_score_kernel<FdModel, 64> over the scan's own chunk
__global__ __launch_bounds__(kBlock) void fdb_score_kernel(const FdbSac* __restrict__ tab, const int* __restrict__ first, const int m, const FdModel::Params prm,
                                                           const int max_hyp) {
  const FdbSac& e = tab[seg_find(first, m, (int)blockIdx.x)];
  sac_score_body<FdModel, kFdHypSub>(e.pts, e.n, e.hyps, e.meta, max_hyp, e.h_first, e.h_end, prm, e.counts, (int)blockIdx.x - e.tile0, (int)blockIdx.y);
}

// ---- host --------------------------------------------------------------------------------------------------------------------
namespace {

// a filter stage's table: every entry's flags, size and first workgroup, then entries | first workgroups in one copy
int fdb_upload(dgs_handle* h, const fdplan::Stage& St, std::vector<FdbSeg>& segs, SegDev<FdbSeg>* dev) {
  if (int rc = seg_flags(h, h->fdb.seg, St, segs)) return rc;
  return seg_upload(h, h->fdb.seg, St, segs, nullptr, 0, dev);
}
// count, scan, scatter over all scans of the stage; kept[j] = kept points of item j (read back: the host waits here)
int fdb_compact(dgs_handle* h, const fdplan::Stage& St, const SegDev<FdbSeg>& dev, std::vector<int64_t>& kept) {
  return seg_compact(h, h->fdb.seg, St, dev, h->fdb.counts8, kept, [&](const dim3 grid, const int* blk, int* totals) {
    hipLaunchKernelGGL(fdb_scatter_kernel, grid, dim3(kBlock), 0, h->stream, dev.tab, dev.first, (int)St.items.size(), blk, totals);
  });
}

// a scan of the RANSAC stage
struct FdbLive {
  int scan;                  // number inside the call
  fdplan::ScanWalk w;
  SacDrawPlan plan;
  const uint32_t* raw;       // the caller's stream, or nullptr: mt19937(12345)
  int64_t draw0;             // first int of its draw list in the shared array
  bool open;
};

// steps 5-9 over the filtered clouds of the scans in `live`; *dirty: launches are queued behind the last host wait
int fdb_ransac(dgs_handle* h, const dgs_floor_detection_params& p, const float* tilt_inv16, std::vector<FdbLive>& live, bool* dirty) {
  FdbScratch& S = h->fdb;
  hipStream_t st = h->stream;
  const int m = (int)live.size();
  if (m == 0) return DGS_OK;
  const int max_hyp = p.max_iterations + 1;
  const FdModel::Params prm{p.plane_dot_order, p.max_sample_checks, p.distance_threshold};
  const double log_one_minus_p = std::log(1.0 - p.probability);

  // the draw lists, from n_filtered alone
  int64_t ints = 0, max_n = 0, max_D = 0;
  bool need_mt = false;
  for (FdbLive& L : live) {
    L.draw0 = ints;
    ints += L.plan.D * 3;
    max_n = std::max(max_n, L.w.n);
    max_D = std::max(max_D, L.plan.D);
    need_mt = need_mt || !L.raw;
  }
  const segtab::StageTable T = segtab::stage_table((size_t)m, sizeof(FdbSac), 0);
  segtab::Layout lay;
  lay.end = T.up;
  const size_t off_draws = lay.take((size_t)ints * sizeof(int), 64), off_meta = lay.take((size_t)m * 4 * sizeof(int), 64);
  const size_t off_cnt = lay.take((size_t)m * max_hyp * sizeof(int), 64), off_hyp = lay.take((size_t)m * max_hyp * sizeof(FdHyp), 64);
  DGS_HIP_TRY(h, S.sac_stage.reserve(lay.end));
  DGS_HIP_TRY(h, S.sac_tables.reserve(T.up));
  DGS_HIP_TRY(h, S.draws.reserve((size_t)ints));
  DGS_HIP_TRY(h, S.hyps.reserve((size_t)m * max_hyp));
  DGS_HIP_TRY(h, S.counts.reserve((size_t)m * max_hyp));
  DGS_HIP_TRY(h, S.meta.reserve((size_t)m * 4));
  char* pin = S.sac_stage.at(0);
  int* h_draws = reinterpret_cast<int*>(pin + off_draws);
  int* h_meta = reinterpret_cast<int*>(pin + off_meta);
  int* h_cnt = reinterpret_cast<int*>(pin + off_cnt);
  FdHyp* h_hyp = reinterpret_cast<FdHyp*>(pin + off_hyp);
  sac_grow_perm(S.sac.perm, max_n);
  if (need_mt) sac_grow_mt(S.sac.mt_raw, 3 * max_D);
  for (FdbLive& L : live) sac_draws<3>(S.sac.perm, L.raw ? L.raw : S.sac.mt_raw.data(), L.w.n, L.plan.D, h_draws + L.draw0);
  DGS_HIP_TRY(h, hipMemcpyAsync(S.draws.ptr, h_draws, (size_t)ints * sizeof(int), hipMemcpyHostToDevice, st));

  // a round's table: the scans of R in order
  std::vector<FdbSac> segs;
  const FdbSac* d_tab = reinterpret_cast<const FdbSac*>(S.sac_tables.ptr + T.entries);
  const int* d_first = reinterpret_cast<const int*>(S.sac_tables.ptr + T.first);
  auto upload_round = [&](const fdplan::Round& R) -> int {
    const size_t r = R.items.size();
    segs.assign(r, FdbSac{});
    for (size_t a = 0; a < r; a++) {
      const fdplan::RoundItem& it = R.items[a];
      const FdbLive& L = live[(size_t)it.scan];
      FdbSac& e = segs[a];
      e.pts = S.filtered[(size_t)L.scan].ptr;
      e.draws = S.draws.ptr + L.draw0;
      e.hyps = S.hyps.ptr + (size_t)it.scan * max_hyp;
      e.counts = S.counts.ptr + (size_t)it.scan * max_hyp;
      e.meta = S.meta.ptr + (size_t)it.scan * 4;
      e.n = (int)L.w.n;
      e.D = (int)L.plan.D;
      e.h_first = it.h_first;
      e.h_end = it.h_end;
      e.tile0 = it.tile0;
    }
    segtab::place(pin, T, segs.data(), r * sizeof(FdbSac), R.first());
    DGS_HIP_TRY(h, hipMemcpyAsync(S.sac_tables.ptr, pin, T.up, hipMemcpyHostToDevice, st));
    return DGS_OK;
  };

  for (int round = 0;; round++) {
    fdplan::Round R;
    for (int j = 0; j < m; j++) {
      FdbLive& L = live[(size_t)j];
      if (!L.open) continue;
      L.open = L.w.advance(h_hyp + (size_t)j * max_hyp, h_cnt + (size_t)j * max_hyp, p.max_iterations, p.hyp_chunk_first, p.hyp_chunk, log_one_minus_p,
                           FdModel::ratio_power);
      if (L.open) fdplan::round_add(R, j, L.w.n, L.w.h_first, L.w.h_end);
    }
    if (R.items.empty()) break;
    if (int rc = upload_round(R)) return rc;
    const int r = (int)R.items.size();
    if (round == 0) {   // every scan is open in the first round: its table serves the prepare launch as well
      hipLaunchKernelGGL(fdb_prepare_kernel, dim3((unsigned)r), dim3(kSacPrepareBlock), 0, st, d_tab, prm, max_hyp);
      S.counts8[0]++;
    }
    hipLaunchKernelGGL(fdb_score_kernel, dim3((unsigned)R.tiles, (unsigned)R.groups), dim3(kBlock), 0, st, d_tab, d_first, r, prm, max_hyp);
    DGS_HIP_TRY(h, hipGetLastError());
    // meta, and the round's window of hypotheses and counts, of all scans: row j of the strided copies is scan j
    const size_t w = (size_t)(R.h_hi - R.h_lo);
    DGS_HIP_TRY(h, hipMemcpyAsync(h_meta, S.meta.ptr, (size_t)m * 4 * sizeof(int), hipMemcpyDeviceToHost, st));
    DGS_HIP_TRY(h, hipMemcpy2DAsync(h_hyp + R.h_lo, (size_t)max_hyp * sizeof(FdHyp), S.hyps.ptr + R.h_lo, (size_t)max_hyp * sizeof(FdHyp), w * sizeof(FdHyp),
                                    (size_t)m, hipMemcpyDeviceToHost, st));
    DGS_HIP_TRY(h, hipMemcpy2DAsync(h_cnt + R.h_lo, (size_t)max_hyp * sizeof(int), S.counts.ptr + R.h_lo, (size_t)max_hyp * sizeof(int), w * sizeof(int),
                                    (size_t)m, hipMemcpyDeviceToHost, st));
    DGS_HIP_TRY(h, hipStreamSynchronize(st));
    *dirty = false;
    S.counts8[0]++;
    S.counts8[1]++;
    S.counts8[7]++;
    for (const fdplan::RoundItem& it : R.items) live[(size_t)it.scan].w.scored_round(h_meta[(size_t)it.scan * 4], h_meta[(size_t)it.scan * 4 + 1], max_hyp);
  }

  // the walks' end states; a walk that ran past its list is finished alone, over longer ones
  for (int j = 0; j < m; j++) {
    FdbLive& L = live[(size_t)j];
    FdScan& sc = S.scans[(size_t)L.scan];
    float coeffs[4] = {0.f, 0.f, 0.f, 0.f};
    if (!fd_walk_to_trace(L.w, h_hyp + (size_t)j * max_hyp, sc.trace, coeffs)) {
      S.counts8[4]++;
      bool exhausted = !L.plan.grow();
      StageCounts did;
      if (!exhausted)
        if (int rc = fd_ransac_lists(h, p, S.filtered[(size_t)L.scan].ptr, L.w.n, L.raw, L.plan, S.sac, S.hyps_single, sc, coeffs, &exhausted, &did)) return rc;
      S.counts8[0] += did.launches;
      S.counts8[1] += did.waits;
      if (exhausted) {
        sc.status = DGS_FD_RNG_EXHAUSTED;
        continue;
      }
      sc.have_host = true;
    }
    fd_verdict(sc, p, tilt_inv16, coeffs, sc.trace.count);
  }
  return DGS_OK;
}

// the chain over the scans [f, f + n) of the call.  d_in: device pointers.
int fdb_chain(dgs_handle* h, const dgs_floor_detection_params& p, const float* tilt16, const float* tilt_inv16, int f, int n, const float4* const* d_in,
              const int64_t* sizes, const uint32_t* const* rng_raw, const int64_t* rng_len) {
  FdbScratch& S = h->fdb;
  hipStream_t st = h->stream;
  std::vector<int64_t> cur((size_t)n, 0), kept;
  std::vector<FdbSeg> segs;
  SegDev<FdbSeg> dev{};
  bool dirty = false;   // launches are queued behind the last host wait: the pinned blocks may still be read

  // 1. tilt and the two clips -> the clipped clouds
  {
    const fdplan::Stage St = fdplan::make_stage(n, sizes);
    const int m = (int)St.items.size();
    if (m > 0) {
      DGS_HIP_TRY(h, S.tilted.reserve((size_t)St.points));
      segs.assign((size_t)m, FdbSeg{});
      for (int j = 0; j < m; j++) {
        const int s = St.items[j].scan;
        CloudState& c = S.clip[(size_t)(f + s)];
        DGS_HIP_TRY(h, c.pts.reserve((size_t)sizes[s]));
        segs[j].in = d_in[s];
        segs[j].src = S.tilted.ptr + St.items[j].point0;
        segs[j].out = c.pts.ptr;
      }
      if (int rc = fdb_upload(h, St, segs, &dev)) return rc;
      const float hi = (float)(p.sensor_height + p.height_clip_range), lo = (float)(p.sensor_height - p.height_clip_range);
      hipLaunchKernelGGL(fdb_tilt_clip_kernel, dim3((unsigned)St.blocks), dim3(kBlock), 0, st, dev.tab, dev.first, m, fd_mat(tilt16), p.transform_order, hi, lo);
      S.counts8[0]++;
      if (int rc = fdb_compact(h, St, dev, kept)) return rc;
      for (int j = 0; j < m; j++) {
        const int s = St.items[j].scan;
        cur[s] = kept[j];
        S.clip[(size_t)(f + s)].n = kept[j];
        S.scans[(size_t)(f + s)].n_clipped = kept[j];
      }
    }
  }

  // 2. the normal filter over the clipped clouds in place
  std::vector<const float4*> kept_ptr((size_t)n, nullptr);
  for (int s = 0; s < n; s++) kept_ptr[s] = S.clip[(size_t)(f + s)].pts.ptr;
  if (p.use_normal_filtering) {
    const fdplan::Stage St = fdplan::make_stage(n, cur.data());
    const int m = (int)St.items.size();
    if (m > 0) {
      std::vector<float4*> normals((size_t)n, nullptr);
      for (int j = 0; j < m; j++) {
        const int s = St.items[j].scan;
        DGS_HIP_TRY(h, S.normals[(size_t)(f + s)].reserve((size_t)St.items[j].n));
        normals[s] = S.normals[(size_t)(f + s)].ptr;
        S.scans[(size_t)(f + s)].have_normals = true;
      }
      bool fell_back = false;
      std::fill(S.nrm.counts8, S.nrm.counts8 + 8, 0);
      // ne.setViewPoint(0.0f, 0.0f, sensor_height) (:220)
      const int rc = prefilter_batch_normal_stage(h, S.nrm, n, S.clip.data() + f, cur.data(), 0.0f, 0.0f, (float)p.sensor_height, normals.data(), &fell_back);
      S.counts8[0] += S.nrm.counts8[0];
      S.counts8[1] += S.nrm.counts8[1];
      S.counts8[6] += S.nrm.counts8[6];
      if (rc) return rc;
      if (fell_back) S.counts8[4] += n;
      DGS_HIP_TRY(h, S.kept.reserve((size_t)St.points));
      segs.assign((size_t)m, FdbSeg{});
      for (int j = 0; j < m; j++) {
        const int s = St.items[j].scan;
        segs[j].in = normals[s];
        segs[j].src = S.clip[(size_t)(f + s)].pts.ptr;
        segs[j].out = S.kept.ptr + St.items[j].point0;
        kept_ptr[s] = segs[j].out;
      }
      if (int rc2 = fdb_upload(h, St, segs, &dev)) return rc2;
      hipLaunchKernelGGL(fdb_normal_flag_kernel, dim3((unsigned)St.blocks), dim3(kBlock), 0, st, dev.tab, dev.first, m,
                         std::cos(p.normal_filter_thresh * M_PI / 180.0));
      S.counts8[0]++;
      if (int rc2 = fdb_compact(h, St, dev, kept)) return rc2;
      for (int j = 0; j < m; j++) cur[St.items[j].scan] = kept[j];
    }
  }

  // 3. the back-transform -> the filtered clouds
  {
    const fdplan::Stage St = fdplan::make_stage(n, cur.data());
    const int m = (int)St.items.size();
    if (m > 0) {
      segs.assign((size_t)m, FdbSeg{});
      for (int j = 0; j < m; j++) {
        const int s = St.items[j].scan;
        DGS_HIP_TRY(h, S.filtered[(size_t)(f + s)].reserve((size_t)St.items[j].n));
        segs[j].in = kept_ptr[s];
        segs[j].out = S.filtered[(size_t)(f + s)].ptr;
      }
      if (int rc = fdb_upload(h, St, segs, &dev)) return rc;
      hipLaunchKernelGGL(fdb_transform_kernel, dim3((unsigned)St.blocks), dim3(kBlock), 0, st, dev.tab, dev.first, m, fd_mat(tilt_inv16), p.transform_order);
      DGS_HIP_TRY(h, hipGetLastError());
      S.counts8[0]++;
      dirty = true;
    }
  }

  // 4. who reaches the RANSAC
  std::vector<FdbLive> live;
  for (int s = 0; s < n; s++) {
    FdScan& sc = S.scans[(size_t)(f + s)];
    sc.n_filtered = cur[s];
    sc.trace.n_clipped = (int32_t)sc.n_clipped;
    sc.trace.n_filtered = (int32_t)cur[s];
    if (!fdplan::reaches_ransac(sizes[s], cur[s], p.floor_pts_thresh)) continue;   // DGS_FD_TOO_FEW_POINTS
    if (cur[s] < 3) {   // getSamples: fewer points than the sample size, the selection is empty and the loop breaks at once
      sc.trace.ransac_failed = 1;
      fd_verdict(sc, p, tilt_inv16, nullptr, 0);
      continue;
    }
    const uint32_t* raw = (rng_raw && rng_len && rng_len[s] > 0) ? rng_raw[s] : nullptr;
    FdbLive L{f + s, fdplan::ScanWalk{}, SacDrawPlan(raw ? rng_len[s] / 3 : INT32_MAX / 4, p.max_iterations + 1, p.max_sample_checks), raw, 0, true};
    if (L.plan.empty()) {
      sc.status = DGS_FD_RNG_EXHAUSTED;
      continue;
    }
    L.w.n = cur[s];
    L.w.D = L.plan.D;
    live.push_back(L);
    S.counts8[3]++;
  }
  if (int rc = fdb_ransac(h, p, tilt_inv16, live, &dirty)) return rc;
  if (dirty) {   // nothing reached the RANSAC: the back-transform's table is still on its way
    DGS_HIP_TRY(h, hipStreamSynchronize(st));
    S.counts8[1]++;
  }
  return DGS_OK;
}

FdScan* fdb_scan(dgs_handle* h, int32_t scan) {
  if (!h || scan < 0 || (size_t)scan >= h->fdb.scans.size()) return nullptr;
  return &h->fdb.scans[(size_t)scan];
}

}  // namespace

void floor_detection_batch_release(dgs_handle* h) {
  FdbScratch& S = h->fdb;
  for (CloudState& c : S.clip) c.release();
  for (DevBuf<float4>& b : S.normals) b.release();
  for (DevBuf<float4>& b : S.filtered) b.release();
  S.clip.clear(); S.normals.clear(); S.filtered.clear(); S.scans.clear();
  prefilter_batch_release(S.nrm);
  S.in.release(); S.tilted.release(); S.kept.release(); S.seg.release();
  S.sac_tables.release(); S.sac_stage.release(); S.draws.release(); S.counts.release(); S.meta.release(); S.hyps.release();
  S.sac.release(); S.hyps_single.release();
}

}  // namespace dgs

using namespace dgs;

extern "C" {

int dgs_floor_detection_batch(dgs_handle* h, const dgs_floor_detection_params* params, const float* tilt16, const float* tilt_inv16, int32_t n_scans,
                              const float* const* in_xyz16, const int64_t* sizes, int32_t in_on_device, const uint32_t* const* rng_raw, const int64_t* rng_len,
                              float* coeffs4_out, int32_t* status_out) {
  if (const char* why = fd_bad_params(params)) {   // before anything touches a device
    if (h) h->err = why;
    return DGS_ERR_INVALID_ARGUMENT;
  }
  if (!h || !tilt16 || !tilt_inv16 || n_scans < 0) return DGS_ERR_INVALID_ARGUMENT;
  FdbScratch& S = h->fdb;
  if (n_scans == 0) {   // nothing listed, nothing launched
    std::fill(S.counts8, S.counts8 + 8, 0);
    S.scans.clear();
    return DGS_OK;
  }
  if (!in_xyz16 || !sizes || !coeffs4_out || !status_out || (rng_raw && !rng_len)) return DGS_ERR_INVALID_ARGUMENT;
  int64_t total = 0;
  for (int s = 0; s < n_scans; s++) {
    if (sizes[s] < 0 || sizes[s] > INT32_MAX || (sizes[s] > 0 && !in_xyz16[s])) return DGS_ERR_INVALID_ARGUMENT;
    if (rng_len && (rng_len[s] < 0 || (rng_len[s] > 0 && (!rng_raw || !rng_raw[s])))) return DGS_ERR_INVALID_ARGUMENT;
    total += sizes[s];
  }
  if (total > INT32_MAX) {
    h->err = "dgs_floor_detection_batch: more than 2^31 points in one call";
    return DGS_ERR_INVALID_ARGUMENT;
  }
  // from here on things are written
  h->err.clear();
  DGS_HIP_TRY(h, hipSetDevice(h->device));
  std::fill(S.counts8, S.counts8 + 8, 0);
  S.counts8[2] = n_scans;
  S.params = *params;
  if ((int)S.clip.size() < n_scans) {   // CloudState and DevBuf own nothing by destructor: growing moves the buffers' addresses along
    S.clip.resize((size_t)n_scans);
    S.normals.resize((size_t)n_scans);
    S.filtered.resize((size_t)n_scans);
  }
  S.scans.assign((size_t)n_scans, FdScan{});
  for (int s = 0; s < n_scans; s++) {
    for (int a = 0; a < 4; a++) coeffs4_out[4 * s + a] = 0.f;
    status_out[s] = DGS_FD_TOO_FEW_POINTS;
    S.scans[(size_t)s].reset();
    S.scans[(size_t)s].n = sizes[s];
    S.clip[(size_t)s].n = 0;
    S.clip[(size_t)s].invalidate();
  }
  const int64_t budget = S.points_budget > 0 ? S.points_budget : fdplan::kBatchPoints;
  const std::vector<fdplan::Chunk> chunks = fdplan::make_chunks(n_scans, sizes, budget);
  std::vector<const float4*> d_in((size_t)n_scans);
  for (const fdplan::Chunk& ch : chunks) {
    const int f = ch.first;
    int rc = DGS_OK;
    if (in_on_device) {
      for (int s = f; s < f + ch.count; s++) d_in[s] = reinterpret_cast<const float4*>(in_xyz16[s]);
    } else {
      rc = stage_host_inputs(h, S.in, ch.count, in_xyz16 + f, sizes + f, d_in.data() + f);
    }
    if (rc == DGS_OK)
      rc = fdb_chain(h, *params, tilt16, tilt_inv16, f, ch.count, d_in.data() + f, sizes + f, rng_raw ? rng_raw + f : nullptr, rng_len ? rng_len + f : nullptr);
    if (rc != DGS_OK) {
      (void)hipStreamSynchronize(h->stream);
      S.scans.clear();
      return rc;
    }
    S.counts8[5]++;
  }
  for (int s = 0; s < n_scans; s++) {
    const FdScan& sc = S.scans[(size_t)s];
    status_out[s] = sc.status;
    for (int a = 0; a < 4; a++) coeffs4_out[4 * s + a] = sc.coeffs[a];
  }
  return DGS_OK;
}

int dgs_floor_detection_batch_get_filtered(dgs_handle* h, int32_t scan, float* out_xyz16, int64_t capacity, int32_t out_on_device, int64_t* n) {
  const FdScan* sc = fdb_scan(h, scan);
  return fd_get_filtered(h, sc, sc ? h->fdb.filtered[(size_t)scan].ptr : nullptr, out_xyz16, capacity, out_on_device, n);
}

int dgs_floor_detection_batch_get_inliers(dgs_handle* h, int32_t scan, int32_t* indices, float* points_xyz16, int64_t capacity, int64_t* n) {
  FdScan* sc = fdb_scan(h, scan);
  if (sc && n && capacity >= 0 && !sc->have_inliers) {   // the list is made when somebody asks; no model: empty inliers
    if (sc->trace.winner_rank >= 0 && sc->status != DGS_FD_RNG_EXHAUSTED) {
      if (!sc->have_host) {
        const int64_t nf = sc->n_filtered;
        DGS_HIP_TRY(h, hipSetDevice(h->device));
        sc->host_filtered.resize((size_t)nf);
        DGS_HIP_TRY(h, hipMemcpyAsync(sc->host_filtered.data(), h->fdb.filtered[(size_t)scan].ptr, (size_t)nf * sizeof(float4), hipMemcpyDeviceToHost, h->stream));
        DGS_HIP_TRY(h, hipStreamSynchronize(h->stream));
        sc->have_host = true;
      }
      fd_select_inliers(*sc, h->fdb.params, sc->trace.raw_coeffs);
    }
    sc->have_inliers = true;
  }
  return fd_get_inliers(sc, indices, points_xyz16, capacity, n);
}

int dgs_floor_detection_batch_get_trace(dgs_handle* h, int32_t scan, dgs_floor_detection_trace* trace) { return fd_get_trace(fdb_scan(h, scan), trace); }

int dgs_floor_detection_batch_get_clipped(dgs_handle* h, int32_t scan, float* clipped_xyz16, float* normals4, int64_t capacity, int64_t* n) {
  const FdScan* sc = fdb_scan(h, scan);
  return fd_get_clipped(h, sc, sc ? h->fdb.clip[(size_t)scan].pts.ptr : nullptr, sc ? h->fdb.normals[(size_t)scan].ptr : nullptr, clipped_xyz16, normals4,
                        capacity, n);
}

int dgs_floor_detection_batch_get_counts(dgs_handle* h, int64_t* counts8) {
  if (!h || !counts8) return DGS_ERR_INVALID_ARGUMENT;
  std::copy(h->fdb.counts8, h->fdb.counts8 + 8, counts8);
  return DGS_OK;
}

}  // extern "C"
