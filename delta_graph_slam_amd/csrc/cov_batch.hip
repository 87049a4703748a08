// The k-NN covariances of MANY resident clouds in one pass: per chunk of clouds one table upload, one search launch and one covariance
// launch, whatever the number of clouds.  ensure_covariance (gicp_cov.hip) and ensure_pcov (pcl_gicp.hip) make the same covariances one
// cloud at a time, a pair of launches each; this file makes them for FAST_GICP / FAST_VGICP (6 doubles per point) and for GICP_HIP /
// GICP_OMP_HIP (9 doubles per point) with the bodies those kernels run (knn_leaf.h, gicp_cov_body.h, pg_cov.h) -- the same bits.
//
// The table.  One CovBatchEntry per cloud of the chunk: the cloud's index, points, slice of the chunk's neighbour table, output, size, the
// `parts` knn_lists would give it alone (cov_batch_plan.h: the slot order of a neighbour list depends on it, and the 6-double sums follow
// slot order) and its first workgroup in either launch.  Every cloud owns whole workgroups.  A workgroup finds its cloud by bisecting the
// launch's array of first workgroups with its blockIdx.x (seg_find, seg_device.h); the address is workgroup-uniform, so the bisection and the entry are scalar
// loads and the entry lives in SGPRs, like PgTarget (pcl_gicp.hip).  From there on the workgroup is a workgroup of the single-cloud
// launch: same body, same local index, same arguments.
//
// Chunks.  A chunk's neighbour table is h->knn_nbr (points * 32 or * 64 ints), reused by the next chunk in stream order; the plan
// (cov_batch_plan.h) fills chunks up to a point budget.  Nothing in here waits for the device: the tables, laid out by seg_table.h, travel
// from a PinnedBlock of their own, and only a call that finds the previous pass's upload still in flight waits for it (counted).
//
// Served one cloud at a time inside the call, results unchanged, and counted as such: gicp_cov_jacobi_svd = 2 (upstream order,
// gicp_cov_ordered.hip) and the per-query walk (DGS_KNN_LEAF=0, DGS_KNN_LEAF_WIDE=0 for wide k).
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

#include "cov_batch_plan.h"
#include "gicp_cov_body.h"
#include "handle.h"
#include "knn_leaf.h"
#include "nn_group.h"
#include "pg_cov.h"
#include "seg_device.h"
#include "seg_table.h"

namespace dgs {

static_assert(covplan::kPlanLeaf == kLeaf && covplan::kPlanWavesPerBlock == kBlock / kWave, "cov_batch_plan.h restates the search's geometry");

struct CovBatchEntry {
  BvhView b;
  const float4* pts;
  int* nbr;              // the cloud's slice of the chunk's neighbour table: [position in index order * stride + slot]
  double* out;           // CloudState::cov (6 per point) or CloudState::pcov (9 per point)
  int n, parts;
  int knn_blk0, cov_blk0;   // first workgroup of the cloud in the search launch and in the covariance launch
  int pad[4];
};
static_assert(sizeof(CovBatchEntry) == 96, "one entry is six 16-byte scalar loads");

// (seg_find, the bisection of the array of first workgroups: seg_device.h)
// ---- the search: gicp_knn_leaf_kernel / gicp_knn_leaf_wide_kernel over the chunk, their launch bounds
__global__ __launch_bounds__(kBlock, DGS_KNN_WAVES) void cov_knn_batch_kernel(const CovBatchEntry* __restrict__ tab, const int* __restrict__ first, const int m, const int k,
                                                                              int* __restrict__ stats) {
  const CovBatchEntry e = tab[seg_find(first, m, (int)blockIdx.x)];
  gicp_knn_leaf_body<kKnnSlots>(e.b, e.n, k, e.parts, e.nbr, stats, (int)blockIdx.x - e.knn_blk0);
}
__global__ __launch_bounds__(kBlock, DGS_KNN_WAVES) void cov_knn_batch_wide_kernel(const CovBatchEntry* __restrict__ tab, const int* __restrict__ first, const int m,
                                                                                   const int k, int* __restrict__ stats) {
  const CovBatchEntry e = tab[seg_find(first, m, (int)blockIdx.x)];
  gicp_knn_leaf_body<kKnnSlotsWide>(e.b, e.n, k, e.parts, e.nbr, stats, (int)blockIdx.x - e.knn_blk0);
}

// ---- FAST_GICP / FAST_VGICP: gicp_cov_from_knn_kernel / gicp_cov_from_knn_wide_kernel over the chunk
__global__ __launch_bounds__(kBlock) void cov_fast_batch_kernel(const CovBatchEntry* __restrict__ tab, const int* __restrict__ first, const int m, const int k, const int method) {
  const CovBatchEntry e = tab[seg_find(first, m, (int)blockIdx.x)];
  gicp_cov_from_knn_body<kKnnSlots>(e.b, e.pts, e.n, k, method, e.nbr, e.out, (int)blockIdx.x - e.cov_blk0);
}
__global__ __launch_bounds__(kBlock) void cov_fast_batch_wide_kernel(const CovBatchEntry* __restrict__ tab, const int* __restrict__ first, const int m, const int k,
                                                                     const int method) {
  const CovBatchEntry e = tab[seg_find(first, m, (int)blockIdx.x)];
  gicp_cov_from_knn_body<kKnnSlotsWide>(e.b, e.pts, e.n, k, method, e.nbr, e.out, (int)blockIdx.x - e.cov_blk0);
}

// ---- GICP_HIP: pg_cov_kernel / pg_cov_wide_kernel over the chunk
__global__ __launch_bounds__(kBlock) void cov_pcl_batch_kernel(const CovBatchEntry* __restrict__ tab, const int* __restrict__ first, const int m, const int k, const double eps) {
  const CovBatchEntry e = tab[seg_find(first, m, (int)blockIdx.x)];
  pg_cov_body(e.b, e.pts, e.n, k, eps, e.nbr, e.out, (int)blockIdx.x - e.cov_blk0);
}
__global__ __launch_bounds__(kPgWideBlock) void cov_pcl_batch_wide_kernel(const CovBatchEntry* __restrict__ tab, const int* __restrict__ first, const int m, const int k,
                                                                          const double eps) {
  const CovBatchEntry e = tab[seg_find(first, m, (int)blockIdx.x)];
  pg_cov_wide_body(e.b, e.pts, e.n, k, eps, e.nbr, e.out, (int)blockIdx.x - e.cov_blk0);
}

// ---- host --------------------------------------------------------------------------------------------------------------------
// counts8 of the last pass: [0] kernel launches of the pass, [1] host waits, [2] clouds listed, [3] clouds covered, [4] clouds whose cache
// was valid, [5] chunks, [6] clouds served by a per-cloud fallback, [7] indices built (by the caller that builds them: cloud_build_covariances,
// the align_pairs paths).
int ensure_covariances(dgs_handle* h, int n, CloudState* const* clouds, int kind) {
  CbScratch& S = h->cb;
  std::fill(S.counts8, S.counts8 + 8, 0);
  S.counts8[2] = n;
  const int k = h->prm.gicp_correspondence_randomness;
  if (k > kKnnMaxWide) {
    h->err = kKnnTooWide;
    return DGS_ERR_UNSUPPORTED;
  }
  const bool pcl = kind == covplan::kPcl;
  const covplan::Key key{kind, k, h->prm.gicp_regularization, h->pg_opt.gicp_epsilon};
  std::vector<covplan::CloudInfo> infos((size_t)n);
  for (int i = 0; i < n; i++) {
    const CloudState& c = *clouds[i];
    infos[i] = pcl ? covplan::CloudInfo{&c, c.n, c.pcov_valid, c.pcov_k, 0, c.pcov_eps} : covplan::CloudInfo{&c, c.n, c.cov_valid, c.cov_k, c.cov_reg, 0.0};
  }
  const bool wide = k > kKnnMax;
  const int width = wide ? kKnnMaxWide : kKnnMax;
  const int cov_points_per_block = pcl ? (wide ? kPgWideBlock : kBlock) : kCovPerBlock;
  const int64_t budget = S.points_budget > 0 ? S.points_budget : covplan::kCovBatchPoints;
  const covplan::Plan P = covplan::make_plan(key, n, infos.data(), budget, h->knn_parts, cov_points_per_block);
  S.counts8[4] = P.cached;
  const int M = (int)P.items.size();
  if (M == 0) return DGS_OK;
  // a listed cloud without an index gets the one the single pass would build for it
  for (const covplan::Item& it : P.items) {
    CloudState& c = *clouds[it.input];
    if (c.bvh.valid) continue;
    const int rc = bvh_build(h, c.bvh, c.pts.ptr, c.n, nullptr, h->batch_kd && &c == h->tgt);
    if (rc) return rc;
  }
  if ((!pcl && h->prm.gicp_cov_jacobi_svd == DGS_GICP_COV_UPSTREAM_ORDER) || !knn_uses_leaf_search(h, k)) {
    for (const covplan::Item& it : P.items) {
      const int rc = pcl ? ensure_pcov(h, *clouds[it.input]) : ensure_covariance(h, *clouds[it.input]);
      if (rc) return rc;
      S.counts8[0] += 2;
      S.counts8[3]++;
      S.counts8[6]++;
    }
    return DGS_OK;
  }
  hipStream_t st = h->stream;
  // every allocation before the first launch
  for (const covplan::Item& it : P.items) {
    CloudState& c = *clouds[it.input];
    if (pcl) DGS_HIP_TRY(h, c.pcov.reserve((size_t)c.n * 9));
    else DGS_HIP_TRY(h, c.cov.reserve((size_t)c.n * 6));
  }
  DGS_HIP_TRY(h, h->knn_nbr.reserve((size_t)P.max_chunk_points * width));
  DGS_HIP_TRY(h, h->knn_stats.reserve(8));
  // the tables of all chunks, back to back: entries | first search workgroups (count + 1) | first covariance workgroups (count + 1)
  std::vector<segtab::ChunkTable> sec(P.chunks.size());
  segtab::Layout L;
  for (size_t c = 0; c < P.chunks.size(); c++) sec[c] = segtab::chunk_table(L, (size_t)P.chunks[c].count, sizeof(CovBatchEntry));
  const size_t bytes = L.end;
  DGS_HIP_TRY(h, S.tables.reserve(bytes));
  bool waited = false;
  DGS_HIP_TRY(h, S.stage.wait_if_in_flight(&waited));
  if (waited) S.counts8[1]++;
  DGS_HIP_TRY(h, S.stage.reserve(bytes));
  char* stage = S.stage.at(0);
  for (size_t c = 0; c < P.chunks.size(); c++) {
    const covplan::Chunk& ch = P.chunks[c];
    const covplan::Item* items = P.items.data() + ch.first;
    CovBatchEntry* tab = reinterpret_cast<CovBatchEntry*>(stage + sec[c].entries);
    const std::vector<int> knn_first = segtab::first_array(items, (size_t)ch.count, &covplan::Item::knn_blk0, ch.knn_blocks);
    const std::vector<int> cov_first = segtab::first_array(items, (size_t)ch.count, &covplan::Item::cov_blk0, ch.cov_blocks);
    std::memcpy(stage + sec[c].knn_first, knn_first.data(), knn_first.size() * sizeof(int));
    std::memcpy(stage + sec[c].cov_first, cov_first.data(), cov_first.size() * sizeof(int));
    for (int j = 0; j < ch.count; j++) {
      const covplan::Item& it = P.items[(size_t)ch.first + j];
      CloudState& cs = *clouds[it.input];
      std::memset(&tab[j], 0, sizeof(CovBatchEntry));
      tab[j].b = make_bvh_view(cs.bvh);
      tab[j].pts = cs.pts.ptr;
      tab[j].nbr = h->knn_nbr.ptr + (size_t)it.nbr_point0 * width;
      tab[j].out = pcl ? cs.pcov.ptr : cs.cov.ptr;
      tab[j].n = (int)cs.n;
      tab[j].parts = it.parts;
      tab[j].knn_blk0 = it.knn_blk0;
      tab[j].cov_blk0 = it.cov_blk0;
    }
  }
  const int cov_method = h->prm.gicp_regularization | (h->prm.gicp_cov_jacobi_svd ? 0x100 : 0);
  const double eps = h->pg_opt.gicp_epsilon;
  const int slot = prof_begin(h, DGS_K_GICP_COVARIANCE);
  for (size_t c = 0; c < P.chunks.size(); c++) {
    const covplan::Chunk& ch = P.chunks[c];
    unsigned char* dev = S.tables.ptr + sec[c].entries;
    DGS_HIP_TRY(h, hipMemcpyAsync(dev, stage + sec[c].entries, sec[c].end - sec[c].entries, hipMemcpyHostToDevice, st));
    if (c + 1 == P.chunks.size()) DGS_HIP_TRY(h, S.stage.mark(st));
    const CovBatchEntry* tab = reinterpret_cast<const CovBatchEntry*>(dev);
    const int* knn_first = reinterpret_cast<const int*>(S.tables.ptr + sec[c].knn_first);
    const int* cov_first = reinterpret_cast<const int*>(S.tables.ptr + sec[c].cov_first);
#ifdef DGS_KNN_STATS
    (void)hipMemsetAsync(h->knn_stats.ptr, 0, 8 * sizeof(int), st);
#endif
    if (wide)
      hipLaunchKernelGGL(cov_knn_batch_wide_kernel, dim3((unsigned)ch.knn_blocks), dim3(kBlock), 0, st, tab, knn_first, ch.count, k, h->knn_stats.ptr);
    else
      hipLaunchKernelGGL(cov_knn_batch_kernel, dim3((unsigned)ch.knn_blocks), dim3(kBlock), 0, st, tab, knn_first, ch.count, k, h->knn_stats.ptr);
    if (pcl) {
      if (wide)
        hipLaunchKernelGGL(cov_pcl_batch_wide_kernel, dim3((unsigned)ch.cov_blocks), dim3(kPgWideBlock), 0, st, tab, cov_first, ch.count, k, eps);
      else
        hipLaunchKernelGGL(cov_pcl_batch_kernel, dim3((unsigned)ch.cov_blocks), dim3(kBlock), 0, st, tab, cov_first, ch.count, k, eps);
    } else {
      if (wide)
        hipLaunchKernelGGL(cov_fast_batch_wide_kernel, dim3((unsigned)ch.cov_blocks), dim3(kBlock), 0, st, tab, cov_first, ch.count, k, cov_method);
      else
        hipLaunchKernelGGL(cov_fast_batch_kernel, dim3((unsigned)ch.cov_blocks), dim3(kBlock), 0, st, tab, cov_first, ch.count, k, cov_method);
    }
    S.counts8[0] += 2;
    S.counts8[5]++;
  }
  prof_end_counted(h, DGS_K_GICP_COVARIANCE, slot, M);   // "covariance passes, one per cloud": the bracket stands for M of them
  DGS_HIP_TRY(h, hipGetLastError());
  for (const covplan::Item& it : P.items) {
    CloudState& c = *clouds[it.input];
    if (pcl) { c.pcov_valid = true; c.pcov_k = k; c.pcov_eps = eps; }
    else { c.cov_valid = true; c.cov_k = k; c.cov_reg = h->prm.gicp_regularization; }
  }
  S.counts8[3] = M;
  return DGS_OK;
}

// dgs_cloud_build_covariances: the missing indices in one batched build (fitness_batch.hip), then the covariances the handle's method
// and parameters would make of every listed cloud on first use.
int cloud_build_covariances(dgs_handle* h, int n, dgs_cloud* const* clouds) {
  CbScratch& S = h->cb;
  std::fill(S.counts8, S.counts8 + 8, 0);
  if (h->prm.gicp_correspondence_randomness > kKnnMaxWide) {
    h->err = kKnnTooWide;
    return DGS_ERR_UNSUPPORTED;
  }
  if (n == 0) return DGS_OK;
  StageCounts build;
  int rc = fitness_batch_build_indices(h, n, clouds, &build);
  if (rc) return rc;
  std::vector<CloudState*> cs((size_t)n);
  for (int i = 0; i < n; i++) cs[i] = &clouds[i]->st;
  rc = ensure_covariances(h, n, cs.data(), h->prm.method == DGS_METHOD_PCL_GICP ? covplan::kPcl : covplan::kFast);
  S.counts8[7] = build.built;
  return rc;
}

void cov_batch_release(dgs_handle* h) {
  h->cb.tables.release();
  h->cb.stage.release();
}

}  // namespace dgs
