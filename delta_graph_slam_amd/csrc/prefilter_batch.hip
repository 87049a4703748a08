// PrefilteringNodelet::cloud_callback over MANY scans in one call (dgs_prefilter_scan_batch): the frames of several streams, one chain of
// launches whatever their number.  Scan i receives, bit for bit and in the same order, what dgs_prefilter_scan (prefilter.hip) gives it
// alone; DESIGN.md §6t.
//
// The table.  Every stage uploads one PfbSeg per scan that is still live: where its points, flags, neighbour lists and outputs are, its
// size and index, and its first workgroup in the stage's launches.  Every scan owns whole workgroups.  A workgroup finds its scan by
// bisecting the launch's array of first workgroups with its blockIdx.x (seg_find, seg_device.h); the address is workgroup-uniform, so the
// bisection and the entry are scalar loads and the entry lives in SGPRs.  From there on the workgroup is a workgroup of the single
// launch: the bodies of prefilter_body.h with the scan's own arguments and the workgroup's number inside the scan.
//
// Compaction.  The flags of all scans stand in one array, each scan at its first workgroup * 256.  One count launch over all workgroups,
// ONE pf_scan_kernel over all counts (compact.h: a scan's total and a workgroup's first slot inside its scan are differences of the
// scanned values), one scatter launch that writes element j of scan s to out_s + slot and, from the scan's first workgroup, its total;
// one download of the totals, one host wait.
//
// k-NN stages (radius, statistical, normal).  The stage's input clouds are CloudStates of the handle's pool; their indices come from
// the batched build (fitness_batch.hip, the non-k-d Hilbert build that pf_knn's bvh_build runs for the single call, restated over
// segments), their lists from gicp_knn_leaf_body with the `parts` each scan would get alone (cov_batch_plan.h): the index and the search
// of the single call, so the same sets with the same ties.
//
// Down-sampling.  VOXELGRID: voxelgrid_batch (voxel_batch.hip), two host waits.  APPROX_VOXELGRID: the single routine per scan.
// DGS_KNN_LEAF=0: the per-query walk per scan (knn_lists) into the scan's slice of the neighbour table.  Both counted in counts8[4].
#include <algorithm>
#include <climits>
#include <cstring>
#include <vector>

#include "compact.h"
#include "handle.h"
#include "knn_leaf.h"
#include "nn_group.h"
#include "prefilter_batch_plan.h"
#include "prefilter_body.h"
#include "seg_device.h"
#include "seg_table.h"

namespace dgs {

static_assert(pfbplan::kPlanBlock == kBlock, "prefilter_batch_plan.h restates the workgroup of the per-point passes");
static_assert(pfbplan::kOk == DGS_OK && pfbplan::kInvalidArgument == DGS_ERR_INVALID_ARGUMENT, "prefilter_batch_plan.h restates the status codes");

struct PfbSeg {
  BvhView b;               // index over `in` (k-NN stages)
  const float4* in;        // the stage's input: the raw scan (head / distance) or a pool cloud
  float4* out;             // the compaction's output: room for n points
  unsigned char* flags;    // the scan's flags: the shared array + blk0 * 256
  int* nbr;                // its slice of the stage's neighbour table: [position in index order * 32 + slot]
  float* mean_d;           // statistical pass: its slice of the mean distances
  double* stats;           // statistical pass: its 4 doubles
  float4* normals;         // normal pass: its slices
  float* cov9;
  double lz;               // height filter: lidar_position.z
  float vx, vy, vz;        // normal filter: the view point
  int n, k, parts;         // points; neighbours asked for; waves per leaf of the search
  int blk0, knn_blk0;      // first workgroup in the per-point launches / in the search launch
};
static_assert(sizeof(PfbSeg) == 144, "one entry is nine 16-byte scalar loads");

// ---- flags -------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void pfb_distance_kernel(const PfbSeg* __restrict__ tab, const int* __restrict__ first, const int m, const double near_t,
                                                              const double far_t) {
  const PfbSeg& e = tab[seg_find(first, m, (int)blockIdx.x)];
  pf_distance_body(e.in, e.n, near_t, far_t, e.flags, (int)blockIdx.x - e.blk0);
}
__global__ __launch_bounds__(kBlock) void pfb_head_flag_kernel(const PfbSeg* __restrict__ tab, const PfHead* __restrict__ heads, const int* __restrict__ first,
                                                               const int m, const double near_t, const double far_t) {
  const int c = seg_find(first, m, (int)blockIdx.x);
  const PfbSeg& e = tab[c];
  pf_head_flag_body(e.in, (long long)e.n, heads[c], near_t, far_t, e.flags, (int)blockIdx.x - e.blk0);
}
__global__ __launch_bounds__(kBlock) void pfb_height_kernel(const PfbSeg* __restrict__ tab, const int* __restrict__ first, const int m) {
  const PfbSeg& e = tab[seg_find(first, m, (int)blockIdx.x)];
  pf_height_body(e.in, e.n, e.lz, e.flags, (int)blockIdx.x - e.blk0);
}

// ---- the scatters of the segmented stable compaction (compact.h; the count launch is compact_count_seg_kernel<PfbSeg>) ------------------
__global__ __launch_bounds__(kBlock) void pfb_scatter_kernel(const PfbSeg* __restrict__ tab, const int* __restrict__ first, const int m, const int* __restrict__ blk,
                                                             int* __restrict__ totals, const int flatten) {
  const int c = seg_find(first, m, (int)blockIdx.x);
  const PfbSeg& e = tab[c];
  compact_scatter_seg<int>(e, c, first, blk, totals, [&](const int i, const int off) {
    float4 p = e.in[i];
    if (flatten) p.z = 0.f;   // flatten (:181): point.z = 0
    e.out[off] = p;           // `out` holds n points
  });
}
__global__ __launch_bounds__(kBlock) void pfb_head_scatter_kernel(const PfbSeg* __restrict__ tab, const PfHead* __restrict__ heads, const int* __restrict__ first,
                                                                  const int m, const int* __restrict__ blk, int* __restrict__ totals) {
  const int c = seg_find(first, m, (int)blockIdx.x);
  const PfbSeg& e = tab[c];
  compact_scatter_seg<long long>(e, c, first, blk, totals,
                                 [&](const long long i, const int off) { pf_head_scatter_body(e.in, (long long)e.n, heads[c], i, off, e.out); });
}

// ---- k-NN stages ---------------------------------------------------------------------------------------------------------------
// gicp_knn_leaf_kernel (knn_lists.hip) over the stage's scans, its launch bounds
__global__ __launch_bounds__(kBlock, DGS_KNN_WAVES) void pfb_knn_kernel(const PfbSeg* __restrict__ tab, const int* __restrict__ knn_first, const int m,
                                                                        int* __restrict__ stats) {
  const PfbSeg& e = tab[seg_find(knn_first, m, (int)blockIdx.x)];
  gicp_knn_leaf_body<kKnnSlots>(e.b, e.n, e.k, e.parts, e.nbr, stats, (int)blockIdx.x - e.knn_blk0);
}
__global__ __launch_bounds__(kBlock) void pfb_radius_kernel(const PfbSeg* __restrict__ tab, const int* __restrict__ first, const int m, const double r2,
                                                            const int inclusive) {
  const PfbSeg& e = tab[seg_find(first, m, (int)blockIdx.x)];
  pf_radius_body(e.b, e.in, e.n, e.k, e.nbr, r2, inclusive, e.flags, (int)blockIdx.x - e.blk0);
}
__global__ __launch_bounds__(kBlock) void pfb_sor_distance_kernel(const PfbSeg* __restrict__ tab, const int* __restrict__ first, const int m, const int sqrt_float) {
  const PfbSeg& e = tab[seg_find(first, m, (int)blockIdx.x)];
  pf_sor_distance_body(e.b, e.in, e.n, e.k, e.nbr, sqrt_float, e.mean_d, (int)blockIdx.x - e.blk0);
}
// one workgroup per scan: pf_sor_stats_kernel's fixed reduction order
__global__ __launch_bounds__(kPfStatsBlock) void pfb_sor_stats_kernel(const PfbSeg* __restrict__ tab, const double mul) {
  const PfbSeg& e = tab[blockIdx.x];
  pf_sor_stats_body(e.mean_d, e.n, mul, e.stats);
}
__global__ __launch_bounds__(kBlock) void pfb_sor_flag_kernel(const PfbSeg* __restrict__ tab, const int* __restrict__ first, const int m) {
  const PfbSeg& e = tab[seg_find(first, m, (int)blockIdx.x)];
  pf_sor_flag_body(e.mean_d, e.n, e.stats, e.flags, (int)blockIdx.x - e.blk0);
}
__global__ __launch_bounds__(kBlock) void pfb_normal_kernel(const PfbSeg* __restrict__ tab, const int* __restrict__ first, const int m) {
  const PfbSeg& e = tab[seg_find(first, m, (int)blockIdx.x)];
  pf_normal_body(e.b, e.in, e.n, e.k, e.nbr, e.vx, e.vy, e.vz, e.flags, e.normals, e.cov9, (int)blockIdx.x - e.blk0);
}

// ---- host --------------------------------------------------------------------------------------------------------------------
namespace {

using PfbDev = SegDev<PfbSeg>;

// the flag array of a stage and every entry's place in it and in the search launch
int pfb_flags(dgs_handle* h, PfbScratch& S, const pfbplan::Stage& St, std::vector<PfbSeg>& segs) {
  if (int rc = seg_flags(h, S.seg, St, segs)) return rc;
  for (size_t j = 0; j < segs.size(); j++) {
    segs[j].knn_blk0 = St.items[j].knn_blk0;
    segs[j].parts = St.items[j].parts;
  }
  return DGS_OK;
}
// entries | heads | first workgroups | first search workgroups -> S.seg.tables in one copy.  The stream is idle here: every stage ended
// with a host wait.
int pfb_upload(dgs_handle* h, PfbScratch& S, const pfbplan::Stage& St, const std::vector<PfbSeg>& segs, const PfHead* heads, PfbDev* dev) {
  return seg_upload(h, S.seg, St, segs, heads, sizeof(PfHead), dev);
}

// count, scan, scatter over all scans of the stage; kept[j] = kept points of item j (read back: the host waits here)
int pfb_compact(dgs_handle* h, PfbScratch& S, const pfbplan::Stage& St, const PfbDev& dev, bool head, bool flatten, std::vector<int64_t>& kept) {
  const int m = (int)St.items.size();
  return seg_compact(h, S.seg, St, dev, S.counts8, kept, [&](const dim3 grid, const int* blk, int* totals) {
    if (head)
      hipLaunchKernelGGL(pfb_head_scatter_kernel, grid, dim3(kBlock), 0, h->stream, dev.tab, static_cast<const PfHead*>(dev.heads), dev.first, m, blk, totals);
    else
      hipLaunchKernelGGL(pfb_scatter_kernel, grid, dim3(kBlock), 0, h->stream, dev.tab, dev.first, m, blk, totals, flatten ? 1 : 0);
  });
}

// indices of the stage's input clouds by the batched build, their k-NN lists into S.nbr; the entries get views and slices
int pfb_knn(dgs_handle* h, PfbScratch& S, const pfbplan::Stage& St, CloudState* pool, std::vector<PfbSeg>& segs) {
  const int m = (int)St.items.size();
  std::vector<CloudState*> cs((size_t)m);
  for (int j = 0; j < m; j++) cs[j] = &pool[St.items[j].scan];
  StageCounts build;
  const int rc = fitness_batch_build_state_indices(h, m, cs.data(), &build);
  S.counts8[0] += build.launches;
  S.counts8[1] += build.waits;
  S.counts8[6] += build.built;
  if (rc) return rc;
  DGS_HIP_TRY(h, S.nbr.reserve((size_t)St.points * kKnnMax));
  DGS_HIP_TRY(h, h->knn_stats.reserve(8));
  for (int j = 0; j < m; j++) {
    segs[j].b = make_bvh_view(cs[j]->bvh);
    segs[j].in = cs[j]->pts.ptr;
    segs[j].nbr = S.nbr.ptr + (size_t)St.items[j].point0 * kKnnMax;
  }
  return DGS_OK;
}
// the search launch over the uploaded table, or (DGS_KNN_LEAF=0) the per-query walk scan by scan into the same slices
int pfb_knn_search(dgs_handle* h, PfbScratch& S, const pfbplan::Stage& St, CloudState* pool, const std::vector<PfbSeg>& segs, const PfbDev& dev, bool leaf) {
  const int m = (int)St.items.size();
  if (leaf) {
    hipLaunchKernelGGL(pfb_knn_kernel, dim3((unsigned)St.knn_blocks), dim3(kBlock), 0, h->stream, dev.tab, dev.knn_first, m, h->knn_stats.ptr);
    S.counts8[0]++;
    return DGS_OK;
  }
  for (int j = 0; j < m; j++) {
    DevBuf<int> slice;   // a view of the scan's slice: knn_lists finds it large enough and writes at stride 32 from its start
    slice.ptr = segs[j].nbr;
    slice.cap = (size_t)St.items[j].n * kKnnMax;
    if (int rc = knn_lists(h, pool[St.items[j].scan], segs[j].k, &slice)) return rc;
    S.counts8[0]++;
  }
  return DGS_OK;
}

// the chain over the scans [0, n) of one chunk.  d_in: device pointers.  heads: one per scan, or nullptr (no head).
int pfb_chain(dgs_handle* h, const dgs_prefilter_params* p, int n, const PfHead* heads, const double* lidar3, const float4* const* d_in, const int64_t* sizes,
              float* const* out3d, const int64_t* cap3d, float* const* out2d, const int64_t* cap2d, int32_t out_on_device, int64_t* n3d_out, int64_t* n2d_out,
              int32_t* status, double* stats4) {
  PfbScratch& S = h->pfb;
  hipStream_t st = h->stream;
  for (std::vector<CloudState>* pool : {&S.a, &S.b, &S.c, &S.d, &S.e})
    if ((int)pool->size() < n) pool->resize((size_t)n);   // CloudState owns nothing by destructor: growing the pool moves the buffers' addresses along
  std::vector<int64_t> cur((size_t)n), kept;
  std::vector<CloudState*> src((size_t)n);   // the cloud every scan's current points stand in
  std::vector<PfbSeg> segs;
  PfbDev dev{};
  const bool fallback_knn = !knn_uses_leaf_search(h, kKnnMax);
  bool fell_back = false;

  // 1. distance filter, behind the raw-scan head when there is one
  {
    const pfbplan::Stage St = pfbplan::make_stage(n, sizes, false, h->knn_parts);
    const int m = (int)St.items.size();
    for (int s = 0; s < n; s++) { cur[s] = 0; src[s] = &S.a[s]; S.a[s].n = 0; S.a[s].invalidate(); }
    if (m > 0) {
      segs.assign((size_t)m, PfbSeg{});
      if (int rc = pfb_flags(h, S, St, segs)) return rc;
      for (int j = 0; j < m; j++) {
        const int s = St.items[j].scan;
        DGS_HIP_TRY(h, S.a[s].pts.reserve((size_t)sizes[s]));
        segs[j].in = d_in[s];
        segs[j].out = S.a[s].pts.ptr;
      }
      if (int rc = pfb_upload(h, S, St, segs, heads, &dev)) return rc;
      if (heads)
        hipLaunchKernelGGL(pfb_head_flag_kernel, dim3((unsigned)St.blocks), dim3(kBlock), 0, st, dev.tab, static_cast<const PfHead*>(dev.heads), dev.first, m, p->distance_near_thresh, p->distance_far_thresh);
      else
        hipLaunchKernelGGL(pfb_distance_kernel, dim3((unsigned)St.blocks), dim3(kBlock), 0, st, dev.tab, dev.first, m, p->distance_near_thresh, p->distance_far_thresh);
      S.counts8[0]++;
      if (int rc = pfb_compact(h, S, St, dev, heads != nullptr, false, kept)) return rc;
      for (int j = 0; j < m; j++) { cur[St.items[j].scan] = kept[j]; S.a[St.items[j].scan].n = kept[j]; }
    }
  }

  // 2. down-sampling
  if (p->downsample_method != DGS_PF_DOWNSAMPLE_NONE) {
    const float leaf = (float)p->downsample_resolution;   // setLeafSize(float, float, float)
    for (int s = 0; s < n; s++) { S.b[s].n = 0; S.b[s].invalidate(); }
    if (p->downsample_method == DGS_PF_DOWNSAMPLE_VOXELGRID) {
      std::vector<const float4*> vin;
      std::vector<int64_t> vn, vout;
      std::vector<CloudState*> vst;
      std::vector<int> who;
      for (int s = 0; s < n; s++)
        if (cur[s] > 0) { vin.push_back(S.a[s].pts.ptr); vn.push_back(cur[s]); vst.push_back(&S.b[s]); who.push_back(s); }
      if (!who.empty()) {
        vout.assign(who.size(), 0);
        StageCounts down;   // dgs_cloud_assign_get_counts keeps reporting the last assign call
        const int rc = voxelgrid_batch(h, (int)who.size(), vin.data(), vn.data(), leaf, vst.data(), nullptr, vout.data(), &down);
        S.counts8[0] += down.launches;
        S.counts8[1] += down.waits;
        if (rc) return rc;
        for (size_t j = 0; j < who.size(); j++) cur[who[j]] = vout[j];
      }
    } else {
      fell_back = true;
      for (int s = 0; s < n; s++) {
        if (cur[s] == 0) continue;
        DGS_HIP_TRY(h, S.b[s].pts.reserve((size_t)cur[s]));
        int64_t m2 = 0;
        if (int rc = approx_voxel_grid_filter(h, S.a[s].pts.ptr, cur[s], leaf, S.b[s].pts.ptr, cur[s], &m2)) return rc;
        S.counts8[0] += 8;   // as dgs_cloud_assign_batch counts the single routine
        S.counts8[1]++;
        cur[s] = m2;
        S.b[s].n = m2;
      }
    }
    for (int s = 0; s < n; s++) src[s] = &S.b[s];
  }

  // 3. outlier removal -> /filtered_points
  if (p->outlier_removal_method != DGS_PF_OUTLIER_NONE) {
    const bool stat = p->outlier_removal_method == DGS_PF_OUTLIER_STATISTICAL;
    const int k = stat ? p->statistical_mean_k + 1 : p->radius_min_neighbors + 1;
    std::vector<int64_t> live((size_t)n);
    for (int s = 0; s < n; s++) {
      live[s] = cur[s];
      if (stat && pfbplan::statistical_status(cur[s], p->statistical_mean_k) != pfbplan::kOk) {
        status[s] = DGS_ERR_INVALID_ARGUMENT;   // the single call's answer for this scan; the others run
        live[s] = 0;
      }
      if (!stat && pfbplan::radius_removes_all(cur[s], k)) live[s] = 0;
      cur[s] = 0;
      S.c[s].n = 0;
      S.c[s].invalidate();
    }
    const pfbplan::Stage St = pfbplan::make_stage(n, live.data(), true, h->knn_parts);
    const int m = (int)St.items.size();
    if (m > 0) {
      segs.assign((size_t)m, PfbSeg{});
      if (int rc = pfb_flags(h, S, St, segs)) return rc;
      // the stage's input clouds are a or b, whichever every scan's points stand in
      std::vector<CloudState>& pool = p->downsample_method != DGS_PF_DOWNSAMPLE_NONE ? S.b : S.a;
      if (int rc = pfb_knn(h, S, St, pool.data(), segs)) return rc;
      if (stat) {
        DGS_HIP_TRY(h, S.mean_d.reserve((size_t)St.points));
        DGS_HIP_TRY(h, S.stats.reserve((size_t)n * 4));
      }
      for (int j = 0; j < m; j++) {
        const int s = St.items[j].scan;
        DGS_HIP_TRY(h, S.c[s].pts.reserve((size_t)St.items[j].n));
        segs[j].out = S.c[s].pts.ptr;
        segs[j].k = k;
        if (stat) {
          segs[j].mean_d = S.mean_d.ptr + St.items[j].point0;
          segs[j].stats = S.stats.ptr + (size_t)j * 4;
        }
      }
      if (int rc = pfb_upload(h, S, St, segs, nullptr, &dev)) return rc;
      if (int rc = pfb_knn_search(h, S, St, pool.data(), segs, dev, !fallback_knn)) return rc;
      fell_back = fell_back || fallback_knn;
      if (stat) {
        hipLaunchKernelGGL(pfb_sor_distance_kernel, dim3((unsigned)St.blocks), dim3(kBlock), 0, st, dev.tab, dev.first, m, p->statistical_sqrt_float);
        hipLaunchKernelGGL(pfb_sor_stats_kernel, dim3((unsigned)m), dim3(kPfStatsBlock), 0, st, dev.tab, p->statistical_stddev);
        hipLaunchKernelGGL(pfb_sor_flag_kernel, dim3((unsigned)St.blocks), dim3(kBlock), 0, st, dev.tab, dev.first, m);
        S.counts8[0] += 3;
        // the scans' statistics ride on the compaction's host wait
        DGS_HIP_TRY(h, hipMemcpyAsync(dev.stats_h, S.stats.ptr, (size_t)m * 4 * sizeof(double), hipMemcpyDeviceToHost, st));
      } else {
        hipLaunchKernelGGL(pfb_radius_kernel, dim3((unsigned)St.blocks), dim3(kBlock), 0, st, dev.tab, dev.first, m, p->radius_radius * p->radius_radius, p->radius_inclusive);
        S.counts8[0]++;
      }
      if (int rc = pfb_compact(h, S, St, dev, false, false, kept)) return rc;
      for (int j = 0; j < m; j++) {
        const int s = St.items[j].scan;
        cur[s] = kept[j];
        S.c[s].n = kept[j];
        if (stat) {
          for (int a = 0; a < 3; a++) stats4[(size_t)s * 4 + a] = dev.stats_h[(size_t)j * 4 + a];
          stats4[(size_t)s * 4 + 3] = (double)St.items[j].n;
        }
      }
    }
    for (int s = 0; s < n; s++) src[s] = &S.c[s];
  }
  const std::vector<int64_t> n3 = cur;
  const std::vector<CloudState*> s3 = src;

  // 4. height filter
  {
    for (int s = 0; s < n; s++) { S.d[s].n = 0; S.d[s].invalidate(); }
    const pfbplan::Stage St = pfbplan::make_stage(n, cur.data(), false, h->knn_parts);
    const int m = (int)St.items.size();
    for (int s = 0; s < n; s++) cur[s] = 0;
    if (m > 0) {
      segs.assign((size_t)m, PfbSeg{});
      if (int rc = pfb_flags(h, S, St, segs)) return rc;
      for (int j = 0; j < m; j++) {
        const int s = St.items[j].scan;
        DGS_HIP_TRY(h, S.d[s].pts.reserve((size_t)St.items[j].n));
        segs[j].in = s3[s]->pts.ptr;
        segs[j].out = S.d[s].pts.ptr;
        segs[j].lz = lidar3[(size_t)s * 3 + 2];
      }
      if (int rc = pfb_upload(h, S, St, segs, nullptr, &dev)) return rc;
      hipLaunchKernelGGL(pfb_height_kernel, dim3((unsigned)St.blocks), dim3(kBlock), 0, st, dev.tab, dev.first, m);
      S.counts8[0]++;
      if (int rc = pfb_compact(h, S, St, dev, false, false, kept)) return rc;
      for (int j = 0; j < m; j++) { cur[St.items[j].scan] = kept[j]; S.d[St.items[j].scan].n = kept[j]; }
    }
  }

  // 5. normal filter + 6. flatten (the scatter of the normal pass writes z = 0)
  {
    const pfbplan::Stage St = pfbplan::make_stage(n, cur.data(), true, h->knn_parts);
    const int m = (int)St.items.size();
    for (int s = 0; s < n; s++) cur[s] = 0;
    if (m > 0) {
      segs.assign((size_t)m, PfbSeg{});
      if (int rc = pfb_flags(h, S, St, segs)) return rc;
      if (int rc = pfb_knn(h, S, St, S.d.data(), segs)) return rc;
      DGS_HIP_TRY(h, S.normals.reserve((size_t)St.points));
      DGS_HIP_TRY(h, S.cov9.reserve((size_t)St.points * 9));
      for (int j = 0; j < m; j++) {
        const int s = St.items[j].scan;
        DGS_HIP_TRY(h, S.e[s].pts.reserve((size_t)St.items[j].n));
        segs[j].out = S.e[s].pts.ptr;
        segs[j].k = (int)std::min<int64_t>(kPfNormalK, St.items[j].n);   // FLANN returns min(k, n) neighbours
        segs[j].normals = S.normals.ptr + St.items[j].point0;
        segs[j].cov9 = S.cov9.ptr + (size_t)St.items[j].point0 * 9;
        segs[j].vx = (float)lidar3[(size_t)s * 3];   // ne.setViewPoint(float, float, float)
        segs[j].vy = (float)lidar3[(size_t)s * 3 + 1];
        segs[j].vz = (float)lidar3[(size_t)s * 3 + 2];
      }
      if (int rc = pfb_upload(h, S, St, segs, nullptr, &dev)) return rc;
      if (int rc = pfb_knn_search(h, S, St, S.d.data(), segs, dev, !fallback_knn)) return rc;
      fell_back = fell_back || fallback_knn;
      hipLaunchKernelGGL(pfb_normal_kernel, dim3((unsigned)St.blocks), dim3(kBlock), 0, st, dev.tab, dev.first, m);
      S.counts8[0]++;
      if (int rc = pfb_compact(h, S, St, dev, false, true, kept)) return rc;
      for (int j = 0; j < m; j++) { cur[St.items[j].scan] = kept[j]; S.e[St.items[j].scan].n = kept[j]; S.counts8[3]++; }
    }
  }

  // the outputs: what the single call reports and copies for every scan that ended the chain
  const hipMemcpyKind kind = out_on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
  for (int s = 0; s < n; s++) {
    if (status[s] != DGS_OK) continue;   // counts stay 0
    n3d_out[s] = n3[s];
    n2d_out[s] = cur[s];
    const pfbplan::Outputs o = pfbplan::output_status(n3[s], cap3d[s], cur[s], cap2d[s]);
    status[s] = o.status;
    if (o.copy3d) DGS_HIP_TRY(h, hipMemcpyAsync(out3d[s], s3[s]->pts.ptr, (size_t)n3[s] * sizeof(float4), kind, st));
    if (o.copy2d) DGS_HIP_TRY(h, hipMemcpyAsync(out2d[s], S.e[s].pts.ptr, (size_t)cur[s] * sizeof(float4), kind, st));
  }
  DGS_HIP_TRY(h, hipStreamSynchronize(st));
  DGS_HIP_TRY(h, hipGetLastError());
  S.counts8[1]++;
  if (fell_back) S.counts8[4] += n;
  return DGS_OK;
}

}  // namespace

// stage 5 of pfb_chain without its compaction, for a caller with a rule of its own over the normals
int prefilter_batch_normal_stage(dgs_handle* h, PfbScratch& S, int n, CloudState* pool, const int64_t* sizes, float vx, float vy, float vz,
                                 float4* const* normals, bool* fell_back) {
  const pfbplan::Stage St = pfbplan::make_stage(n, sizes, true, h->knn_parts);
  const int m = (int)St.items.size();
  *fell_back = false;
  if (m == 0) return DGS_OK;
  const bool fallback_knn = !knn_uses_leaf_search(h, kKnnMax);
  std::vector<PfbSeg> segs((size_t)m, PfbSeg{});
  PfbDev dev{};
  if (int rc = pfb_flags(h, S, St, segs)) return rc;   // the prefilter rule's flags: written by the body, read by nobody
  if (int rc = pfb_knn(h, S, St, pool, segs)) return rc;
  DGS_HIP_TRY(h, S.cov9.reserve((size_t)St.points * 9));
  for (int j = 0; j < m; j++) {
    segs[j].k = (int)std::min<int64_t>(kPfNormalK, St.items[j].n);   // FLANN returns min(k, n) neighbours
    segs[j].normals = normals[St.items[j].scan];
    segs[j].cov9 = S.cov9.ptr + (size_t)St.items[j].point0 * 9;
    segs[j].vx = vx;
    segs[j].vy = vy;
    segs[j].vz = vz;
  }
  if (int rc = pfb_upload(h, S, St, segs, nullptr, &dev)) return rc;
  if (int rc = pfb_knn_search(h, S, St, pool, segs, dev, !fallback_knn)) return rc;
  hipLaunchKernelGGL(pfb_normal_kernel, dim3((unsigned)St.blocks), dim3(kBlock), 0, h->stream, dev.tab, dev.first, m);
  S.counts8[0]++;
  DGS_HIP_TRY(h, hipGetLastError());
  *fell_back = fallback_knn;
  return DGS_OK;
}

void prefilter_batch_release(dgs_handle* h) { prefilter_batch_release(h->pfb); }
void prefilter_batch_release(PfbScratch& S) {
  for (std::vector<CloudState>* pool : {&S.a, &S.b, &S.c, &S.d, &S.e}) {
    for (CloudState& c : *pool) c.release();
    pool->clear();
  }
  S.in.release(); S.seg.release(); S.nbr.release(); S.mean_d.release(); S.stats.release(); S.normals.release(); S.cov9.release();
  S.stats_host.clear();
}

}  // namespace dgs

using namespace dgs;

extern "C" {

int dgs_prefilter_scan_batch(dgs_handle* h, const dgs_prefilter_params* p, int32_t n_scans, const dgs_prefilter_scan_params* scan_params,
                             const float* const* in_xyz16, const int64_t* sizes, int32_t in_on_device, float* const* out3d_xyz16, const int64_t* cap3d,
                             float* const* out2d_xyz16, const int64_t* cap2d, int32_t out_on_device, int64_t* n3d_out, int64_t* n2d_out, double* lidar_xyz_out,
                             int32_t* status_out) {
  if (!h || !p || p->struct_size != sizeof(dgs_prefilter_params) || n_scans < 0) return DGS_ERR_INVALID_ARGUMENT;
  if (p->downsample_method < DGS_PF_DOWNSAMPLE_NONE || p->downsample_method > DGS_PF_DOWNSAMPLE_APPROX_VOXELGRID ||
      p->outlier_removal_method < DGS_PF_OUTLIER_NONE || p->outlier_removal_method > DGS_PF_OUTLIER_RADIUS ||
      (p->downsample_method != DGS_PF_DOWNSAMPLE_NONE && !(p->downsample_resolution > 0)))
    return DGS_ERR_INVALID_ARGUMENT;
  if (p->outlier_removal_method == DGS_PF_OUTLIER_STATISTICAL && (p->statistical_mean_k < 1 || p->statistical_mean_k + 1 > kKnnMax)) {
    h->err = "StatisticalOutlierRemoval: mean_k + 1 must lie in 2..32 (the k-NN of the HIP index)";
    return DGS_ERR_INVALID_ARGUMENT;
  }
  if (p->outlier_removal_method == DGS_PF_OUTLIER_RADIUS && (p->radius_min_neighbors < 0 || p->radius_min_neighbors + 1 > kKnnMax)) {
    h->err = "RadiusOutlierRemoval: min_neighbors + 1 must lie in 1..32 (the k-NN of the HIP index)";
    return DGS_ERR_INVALID_ARGUMENT;
  }
  PfbScratch& S = h->pfb;
  if (n_scans == 0) {   // nothing listed, nothing launched
    std::fill(S.counts8, S.counts8 + 8, 0);
    S.stats_host.clear();
    return DGS_OK;
  }
  if (!in_xyz16 || !sizes || !out3d_xyz16 || !cap3d || !out2d_xyz16 || !cap2d || !n3d_out || !n2d_out || !status_out) return DGS_ERR_INVALID_ARGUMENT;
  int64_t total = 0;
  for (int s = 0; s < n_scans; s++) {
    if (sizes[s] < 0 || sizes[s] > INT32_MAX || (sizes[s] > 0 && !in_xyz16[s]) || cap3d[s] < 0 || (cap3d[s] > 0 && !out3d_xyz16[s]) || cap2d[s] < 0 ||
        (cap2d[s] > 0 && !out2d_xyz16[s]))
      return DGS_ERR_INVALID_ARGUMENT;
    total += sizes[s];
  }
  if (total > INT32_MAX) {
    h->err = "dgs_prefilter_scan_batch: more than 2^31 points in one call";
    return DGS_ERR_INVALID_ARGUMENT;
  }
  std::vector<PfHead> heads;
  std::vector<double> lidar((size_t)n_scans * 3, 0.0);   // Eigen::Vector3d::Zero() without a head
  if (scan_params) {
    heads.resize((size_t)n_scans);
    for (int s = 0; s < n_scans; s++)
      if (!pf_make_head(&scan_params[s], &heads[s], &lidar[(size_t)s * 3])) return DGS_ERR_INVALID_ARGUMENT;
  }
  // from here on things are written
  h->err.clear();
  DGS_HIP_TRY(h, hipSetDevice(h->device));
  std::fill(S.counts8, S.counts8 + 8, 0);
  S.counts8[2] = n_scans;
  S.stats_host.assign((size_t)n_scans * 4, 0.0);
  h->pf.stat_n = h->pf.normal_n = 0;   // the single call's hooks have nothing of this call to report
  for (int s = 0; s < n_scans; s++) {
    n3d_out[s] = n2d_out[s] = 0;
    status_out[s] = DGS_OK;
  }
  if (lidar_xyz_out) std::memcpy(lidar_xyz_out, lidar.data(), lidar.size() * sizeof(double));
  const int64_t budget = S.points_budget > 0 ? S.points_budget : pfbplan::kBatchPoints;
  const std::vector<pfbplan::Chunk> chunks = pfbplan::make_chunks(n_scans, sizes, budget);
  std::vector<const float4*> d_in((size_t)n_scans);
  for (const pfbplan::Chunk& ch : chunks) {
    const int f = ch.first;
    if (in_on_device) {
      for (int s = f; s < f + ch.count; s++) d_in[s] = reinterpret_cast<const float4*>(in_xyz16[s]);
    } else if (int rc = stage_host_inputs(h, S.in, ch.count, in_xyz16 + f, sizes + f, d_in.data() + f)) {
      return rc;
    }
    const int rc = pfb_chain(h, p, ch.count, heads.empty() ? nullptr : heads.data() + f, lidar.data() + (size_t)f * 3, d_in.data() + f, sizes + f, out3d_xyz16 + f,
                             cap3d + f, out2d_xyz16 + f, cap2d + f, out_on_device, n3d_out + f, n2d_out + f, status_out + f, S.stats_host.data() + (size_t)f * 4);
    if (rc != DGS_OK) {
      (void)hipStreamSynchronize(h->stream);
      return rc;
    }
    S.counts8[5]++;
  }
  return DGS_OK;
}

int dgs_prefilter_batch_get_counts(dgs_handle* h, int64_t* counts8) {
  if (!h || !counts8) return DGS_ERR_INVALID_ARGUMENT;
  std::copy(h->pfb.counts8, h->pfb.counts8 + 8, counts8);
  return DGS_OK;
}

int dgs_prefilter_batch_get_statistics(dgs_handle* h, double* stats4_per_scan, int64_t capacity_scans, int64_t* n_scans) {
  if (!h || !n_scans || capacity_scans < 0) return DGS_ERR_INVALID_ARGUMENT;
  const int64_t m = (int64_t)(h->pfb.stats_host.size() / 4);
  *n_scans = m;
  if (stats4_per_scan && capacity_scans >= m && m > 0) std::memcpy(stats4_per_scan, h->pfb.stats_host.data(), (size_t)m * 4 * sizeof(double));
  return DGS_OK;
}

}  // extern "C"
