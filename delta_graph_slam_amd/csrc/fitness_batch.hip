// InformationMatrixCalculator::calc_fitness_score over all edges of an optimisation tick, between clouds that are resident in HBM
// (dgs_calc_fitness_score_batch_clouds), and the batched build of the exact-NN indices those edges need (dgs_cloud_build_indices).
//
// The reference weighs every new odometry edge (apps/delta_graph_slam_nodelet.cpp:572, up to max_keyframes_per_update = 10 per tick)
// and every accepted loop edge (:820) by the mean squared NN distance of cloud2, moved by the edge's relative pose, in cloud1
// (src/hdl_graph_slam/information_matrix_calculator.cpp:77-108), building a kd-tree over cloud1 each time.  dgs_calc_fitness_score
// is that call for one pair of raw arrays: two uploads, one index build, one walk, one wait -- per edge.  Here the clouds are
// dgs_cloud objects, the index over cloud1 is the one the cloud keeps (CloudState::bvh: the loop detector's target index and the ICP
// walks' a moment later), and a tick costs one batched index build for the clouds that have none, ONE walk launch over all edges, one
// closing launch, one download and one host wait.
//
// Walk.  A workgroup is one slice of one edge: it finds its edge in a prefix table of rows (seg_find: wave-uniform, scalar loads), reads the
// edge's BvhView, source, size and transform from the edge table and then does exactly what nn_fitness_kernel does -- the same
// nn_query_group<false> / nn_warm_bound_round calls (nn_group.h), so a distance is the very float the single call produces.  Index
// depths differ between edges, never inside a workgroup.  FIXED SLICES: the rows of an edge and the stretch each wave walks are a
// function of the edge's own cloud2 size (fb_rows_of), the rows are summed per edge in a fixed order by the closing launch, so an
// edge's (sum, used) is bit-identical whatever else the batch holds, wherever the edge stands in it, and alone.
//
// Build.  bvh_build (nn_bvh.hip) restated over segments: per-cloud boxes (min / max: exact in any order), hilbert30 keys with the
// cloud's number above bit 30, one stable radix sort of the 64-bit keys of all clouds (values = original indices, so each segment's
// order is what the 30-bit sort gives that cloud alone), a gather into each cloud's own Bvh::sorted, and the node boxes level by
// level over all clouds at once: the number of launches follows the deepest cloud, not the number of clouds.  No host wait.
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstring>
#include <vector>

#include "handle.h"
#include "nn_group.h"
#include "seg_device.h"
#include "seg_table.h"

namespace dgs {

constexpr int kFbRowQueries = 128;   // cloud2 points per partial row: 4 waves x 4 rounds of 8 adjacent queries (warm bounds from round 2 on)
constexpr int kFbMaxRows = 512;      // ... up to this many rows; beyond 65,536 points the stretches grow instead

inline int fb_rows_of(const int n) { return n <= 0 ? 0 : std::max(1, std::min(kFbMaxRows, (n + kFbRowQueries - 1) / kFbRowQueries)); }

struct FbEdge {
  BvhView b;          // index over cloud1
  const float4* src;  // cloud2
  int n, rows, row0, pad;
  float T[16];        // column-major
};
static_assert(sizeof(FbEdge) == 128, "FbEdge is 128 bytes");

struct FbSeg {
  const float4* pts;
  float4* sorted;
  float4* box_lo;
  float4* box_hi;
  int n, n_pad, off, depth;
};

// ---- walk --------------------------------------------------------------------------------------------------------------------
// INLIER false: the sum and the number of the squared NN distances <= bound (PCL compares the SQUARED distance with max_range), rows
// {sum, used}.  INLIER true: the points of cloud2 whose squared NN distance is strictly below `bound` (the nearestKSearch loop of
// publish_scan_matching_status; nn_fitness_kernel's `best < inlier_sq`), rows {inliers, 0}: counts are integers, so any order of the
// sums gives the same total.
template <bool INLIER>
__device__ __forceinline__ void fb_walk_body(const int* __restrict__ row0s, const FbEdge* __restrict__ edges, const int n_edges, const float bound,
                                             double* __restrict__ rows) {
  // the edge of this workgroup: row0s[e] <= blockIdx.x < row0s[e + 1] (edges without rows have no workgroup: seg_find passes them by)
  const FbEdge* __restrict__ E = edges + __builtin_amdgcn_readfirstlane(seg_find(row0s, n_edges, (int)blockIdx.x));
  const BvhView b = E->b;
  const float4* __restrict__ src = E->src;
  const int n = E->n, n_rows = E->rows, slice = (int)blockIdx.x - E->row0;
  const float t00 = E->T[0], t10 = E->T[1], t20 = E->T[2], t01 = E->T[4], t11 = E->T[5], t21 = E->T[6], t02 = E->T[8], t12 = E->T[9], t22 = E->T[10],
              t03 = E->T[12], t13 = E->T[13], t23 = E->T[14];
  double s = 0.0, c = 0.0;
  constexpr int QPB = kBlock / 8;  // queries per workgroup per round
  const int sub = threadIdx.x & 7;
  // every wave walks a contiguous stretch of cloud2, 8 adjacent points per round (nn_fitness_kernel); stretch and rows follow n alone
  const int run = (n + n_rows * QPB - 1) / (n_rows * QPB);
  const int first = (slice * (kBlock / kWave) + (threadIdx.x >> 6)) * (8 * run) + ((threadIdx.x & 63) >> 3);
  float px = 0.f, py = 0.f, pz = 0.f, prev_best = INFINITY;
  bool prev_found = false;
  for (int r = 0; r < run; r++) {
    const int i = first + r * 8;
    const bool alive = i < n;
    const float4 p = alive ? src[i] : make_float4(0.f, 0.f, 0.f, 0.f);
    // pcl::transformPointCloud: ((m0 x + m1 y) + m2 z) + m3 in float, every step rounded
    const float x = affine_row_rn(t00, t01, t02, t03, p.x, p.y, p.z);
    const float y = affine_row_rn(t10, t11, t12, t13, p.x, p.y, p.z);
    const float z = affine_row_rn(t20, t21, t22, t23, p.x, p.y, p.z);
    float best;
    int bi;
    nn_query_group<false>(b, x, y, z, alive, nn_warm_bound_round(prev_best, prev_found, x, y, z, px, py, pz), best, bi);
    prev_found = alive && bi != 0x7FFFFFFF;
    prev_best = best;
    px = x; py = y; pz = z;
    if (alive && sub == 0) {
      if (bi == 0x7FFFFFFF) best = INFINITY;  // nothing found (non-finite query): as the unbounded search reports it
      if constexpr (INLIER) {
        if (best < bound) s += 1.0;
      } else if (best <= bound) {
        s += (double)best;
        c += 1.0;
      }
    }
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if constexpr (INLIER) {
    __shared__ double sm[kBlock / kWave];
    s = wave_sum(s);
    if (lane == 0) sm[wave] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
      rows[(size_t)blockIdx.x * 2] = ((sm[0] + sm[1]) + sm[2]) + sm[3];
      rows[(size_t)blockIdx.x * 2 + 1] = 0.0;
    }
  } else {
    __shared__ double sm[kBlock / kWave][2];
    s = wave_sum(s); c = wave_sum(c);
    if (lane == 0) { sm[wave][0] = s; sm[wave][1] = c; }
    __syncthreads();
    if (threadIdx.x < 2) rows[(size_t)blockIdx.x * 2 + threadIdx.x] = ((sm[0][threadIdx.x] + sm[1][threadIdx.x]) + sm[2][threadIdx.x]) + sm[3][threadIdx.x];
  }
}
__global__ __launch_bounds__(kBlock) void fb_walk_kernel(const int* __restrict__ row0s, const FbEdge* __restrict__ edges, const int n_edges,
                                                         const float max_range, double* __restrict__ rows) {
  fb_walk_body<false>(row0s, edges, n_edges, max_range, rows);
}
__global__ __launch_bounds__(kBlock) void fb_inlier_kernel(const int* __restrict__ row0s, const FbEdge* __restrict__ edges, const int n_edges,
                                                           const float inlier_sq, double* __restrict__ rows) {
  fb_walk_body<true>(row0s, edges, n_edges, inlier_sq, rows);
}

// one wave per edge: lane l sums the edge's rows l, l + 64, ... in order, then the lanes are summed in a fixed order
__global__ __launch_bounds__(kWave) void fb_close_kernel(const int* __restrict__ row0s, const double* __restrict__ rows, const int n_edges,
                                                         double* __restrict__ out) {
  const int e = blockIdx.x;
  if (e >= n_edges) return;
  const int r0 = row0s[e], nr = row0s[e + 1] - r0;
  double s = 0.0, c = 0.0;
  for (int k = threadIdx.x; k < nr; k += kWave) {
    s += rows[(size_t)(r0 + k) * 2];
    c += rows[(size_t)(r0 + k) * 2 + 1];
  }
  s = wave_sum(s); c = wave_sum(c);
  if (threadIdx.x == 0) {
    out[e * 2] = s;
    out[e * 2 + 1] = c;
  }
}

// ---- batched Hilbert index build ---------------------------------------------------------------------------------------------
// blockIdx.y = cloud.  Boxes of the finite points: the per-segment bodies of seg_device.h over this file's records.
__global__ __launch_bounds__(kBlock) void fb_minmax_kernel(const FbSeg* __restrict__ segs, float* __restrict__ partial) {
  const FbSeg& S = segs[blockIdx.y];
  seg_box_partial_body(S.pts, S.n, partial);
}
__global__ __launch_bounds__(kWave) void fb_minmax_final_kernel(const float* __restrict__ partial, float* __restrict__ boxes) { seg_box_final_body(partial, boxes); }

// hilbert_key_kernel (nn_bvh.hip) per segment, the cloud's number above the 30 key bits
__global__ __launch_bounds__(kBlock) void fb_key_kernel(const FbSeg* __restrict__ segs, const float* __restrict__ boxes, unsigned long long* __restrict__ keys,
                                                        uint32_t* __restrict__ vals) {
  const FbSeg& S = segs[blockIdx.y];
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= S.n) return;
  const float* mm6 = boxes + (size_t)blockIdx.y * 6;
  const float4 p = S.pts[i];
  float org[3] = {mm6[0], mm6[1], mm6[2]};
  float ext = fmaxf(fmaxf(mm6[3] - mm6[0], mm6[4] - mm6[1]), fmaxf(mm6[5] - mm6[2], 1e-6f));
  if (!(mm6[0] <= mm6[3])) { org[0] = org[1] = org[2] = 0.f; ext = 1.f; }
  const float scale = 1023.0f / ext;
  const uint32_t k = (isfinite(p.x) && isfinite(p.y) && isfinite(p.z)) ? hilbert30(p.x, p.y, p.z, org, scale) : 0x3FFFFFFFu;
  keys[(size_t)S.off + i] = ((unsigned long long)blockIdx.y << 30) | k;
  vals[(size_t)S.off + i] = (uint32_t)i;
}

// gather_index_kernel (nn_bvh.hip) per segment, into the cloud's own Bvh::sorted
__global__ __launch_bounds__(kBlock) void fb_gather_kernel(const FbSeg* __restrict__ segs, const uint32_t* __restrict__ order) {
  const FbSeg& S = segs[blockIdx.y];
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= S.n_pad) return;
  if (i < S.n) {
    const uint32_t o = order[(size_t)S.off + i];
    float4 p = S.pts[o];
    p.w = __uint_as_float(o);
    S.sorted[i] = p;
  } else {
    S.sorted[i] = make_float4(NAN, NAN, NAN, __uint_as_float(0xFFFFFFFFu));  // padding: distance is NaN, never selected
  }
}

// bvh_boxes_kernel (nn_bvh.hip) for step `step` of every cloud: step 0 its leaf slots, step k its level depth - k (none when that is the root)
__global__ __launch_bounds__(kBlock) void fb_boxes_kernel(const FbSeg* __restrict__ segs, const int step) {
  const FbSeg& S = segs[blockIdx.y];
  const int level = S.depth - step;
  if (level < 1) return;
  const int count = 1 << (3 * level), first = (count - 1) / (kFan - 1);
  const int t = blockIdx.x * kBlock + threadIdx.x;
  if (t >= count) return;
  const int node = first + t;
  float mn[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, mx[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
  if (step == 0) {
#pragma unroll
    for (int k = 0; k < kLeaf; k++) {
      const int i = t * kLeaf + k;
      if (i < S.n) {
        const float4 p = S.sorted[i];
        if (isfinite(p.x) && isfinite(p.y) && isfinite(p.z)) {
          mn[0] = fminf(mn[0], p.x); mn[1] = fminf(mn[1], p.y); mn[2] = fminf(mn[2], p.z);
          mx[0] = fmaxf(mx[0], p.x); mx[1] = fmaxf(mx[1], p.y); mx[2] = fmaxf(mx[2], p.z);
        }
      }
    }
  } else {
#pragma unroll
    for (int k = 0; k < kFan; k++) {
      const float4 l = S.box_lo[node * kFan + k], h = S.box_hi[node * kFan + k];
      mn[0] = fminf(mn[0], l.x); mn[1] = fminf(mn[1], l.y); mn[2] = fminf(mn[2], l.z);
      mx[0] = fmaxf(mx[0], h.x); mx[1] = fmaxf(mx[1], h.y); mx[2] = fmaxf(mx[2], h.z);
    }
  }
  // into the parent's child-box arrays: parent * kFan + slot = node - 1
  S.box_lo[node - 1] = make_float4(mn[0], mn[1], mn[2], 0.f);
  S.box_hi[node - 1] = make_float4(mx[0], mx[1], mx[2], 0.f);
}

// ---- host --------------------------------------------------------------------------------------------------------------------
// the build of dgs_cloud objects' indices inside a call that reports in FbScratch::counts8 (zeroed by the caller)
static int fb_build_counted(dgs_handle* h, int n, dgs_cloud* const* clouds, StageCounts* did) {
  std::vector<CloudState*> states((size_t)n);
  for (int i = 0; i < n; i++) states[i] = &clouds[i]->st;
  StageCounts sc;
  const int rc = fitness_batch_build_state_indices(h, n, states.data(), &sc);
  h->fb.counts8[0] += sc.launches;
  h->fb.counts8[1] += sc.waits;
  h->fb.counts8[3] += sc.built;
  if (did) *did = sc;
  return rc;
}

int fitness_batch_build_indices(dgs_handle* h, int n, dgs_cloud* const* clouds, StageCounts* did) {
  std::fill(h->fb.counts8, h->fb.counts8 + 8, 0);
  return fb_build_counted(h, n, clouds, did);
}

// The build over cloud states, whoever owns them: dgs_cloud objects (above) or a handle's own stage clouds (prefilter_batch.hip).
int fitness_batch_build_state_indices(dgs_handle* h, int n, CloudState* const* clouds, StageCounts* sink) {
  FbScratch& F = h->fb;
  if (side_join(h) != DGS_OK) return DGS_ERR_HIP;   // an index being built on the side stream
  std::vector<CloudState*> todo;
  for (int i = 0; i < n; i++) {
    CloudState* c = clouds[i];
    if (c->n > 0 && !c->bvh.valid && std::find(todo.begin(), todo.end(), c) == todo.end()) todo.push_back(c);
  }
  const int M = (int)todo.size();
  if (M == 0) return DGS_OK;
  hipStream_t st = h->stream;
  // shapes first, for every cloud: a cloud that cannot be indexed fails the call before any Bvh has been touched
  struct Shape { int n_pad, depth, first_leaf; int64_t slots; };
  std::vector<Shape> shapes((size_t)M);
  int64_t total = 0;
  int max_n = 0, max_pad = 0, max_depth = 0;
  for (int s = 0; s < M; s++) {
    const int cn = (int)todo[s]->n, n_leaves = (cn + kLeaf - 1) / kLeaf;
    int depth = 1;
    int64_t slots = kFan;
    while (slots < n_leaves) { slots *= kFan; depth++; }
    if (depth > 8) { h->err = "cloud too large for the nearest-neighbour index (more than 8 levels)"; return DGS_ERR_UNSUPPORTED; }
    shapes[s] = Shape{n_leaves * kLeaf, depth, (int)((slots - 1) / (kFan - 1)), slots};
    total += cn;
    max_n = std::max(max_n, cn);
    max_pad = std::max(max_pad, shapes[s].n_pad);
    max_depth = std::max(max_depth, depth);
  }
  if (total > INT32_MAX) { h->err = "dgs_cloud_build_indices: more than 2^31 points in one build"; return DGS_ERR_UNSUPPORTED; }
  std::vector<FbSeg> segs((size_t)M);
  int off = 0;
  for (int s = 0; s < M; s++) {
    CloudState& C = *todo[s];
    Bvh& B = C.bvh;
    const Shape& S = shapes[s];
    B.valid = false;
    B.n = C.n;
    B.leaves = (int)S.slots;
    B.levels = S.depth;
    DGS_HIP_TRY(h, B.sorted.reserve((size_t)S.n_pad));
    DGS_HIP_TRY(h, B.node_lo.reserve((size_t)S.first_leaf * kFan));
    DGS_HIP_TRY(h, B.node_hi.reserve((size_t)S.first_leaf * kFan));
    segs[s] = FbSeg{C.pts.ptr, B.sorted.ptr, B.node_lo.ptr, B.node_hi.ptr, (int)C.n, S.n_pad, off, S.depth};
    off += (int)C.n;
  }
  DGS_HIP_TRY(h, F.segs.reserve((size_t)M));
  DGS_HIP_TRY(h, F.mm.reserve((size_t)M * (kSegBoxBlocks + 1) * 6));
  DGS_HIP_TRY(h, F.keys.reserve((size_t)total));
  DGS_HIP_TRY(h, F.keys_alt.reserve((size_t)total));
  DGS_HIP_TRY(h, F.vals.reserve((size_t)total));
  DGS_HIP_TRY(h, F.vals_alt.reserve((size_t)total));
  int seg_bits = 0;
  while ((1 << seg_bits) < M) seg_bits++;
  size_t tb = 0;
  (void)hipcub::DeviceRadixSort::SortPairs(nullptr, tb, F.keys.ptr, F.keys_alt.ptr, F.vals.ptr, F.vals_alt.ptr, (int)total, 0, 30 + seg_bits, st);
  DGS_HIP_TRY(h, h->cub_temp.reserve(tb + 256));
  // the table travels from a pinned block of its own, which the previous build's copy may still be reading
  bool waited = false;
  DGS_HIP_TRY(h, F.bstage.wait_if_in_flight(&waited));
  if (waited) sink->waits++;
  DGS_HIP_TRY(h, F.bstage.reserve(sizeof(FbSeg) * (size_t)M));
  std::memcpy(F.bstage.ptr, segs.data(), sizeof(FbSeg) * (size_t)M);
  DGS_HIP_TRY(h, hipMemcpyAsync(F.segs.ptr, F.bstage.ptr, sizeof(FbSeg) * (size_t)M, hipMemcpyHostToDevice, st));
  DGS_HIP_TRY(h, F.bstage.mark(st));
  float* boxes = F.mm.ptr + (size_t)M * kSegBoxBlocks * 6;
  hipLaunchKernelGGL(fb_minmax_kernel, dim3(kSegBoxBlocks, M), dim3(kBlock), 0, st, F.segs.ptr, F.mm.ptr);
  hipLaunchKernelGGL(fb_minmax_final_kernel, dim3(M), dim3(kWave), 0, st, F.mm.ptr, boxes);
  hipLaunchKernelGGL(fb_key_kernel, dim3((max_n + kBlock - 1) / kBlock, M), dim3(kBlock), 0, st, F.segs.ptr, boxes, F.keys.ptr, F.vals.ptr);
  tb = h->cub_temp.cap;
  DGS_HIP_TRY(h, hipcub::DeviceRadixSort::SortPairs(h->cub_temp.ptr, tb, F.keys.ptr, F.keys_alt.ptr, F.vals.ptr, F.vals_alt.ptr, (int)total, 0, 30 + seg_bits, st));
  hipLaunchKernelGGL(fb_gather_kernel, dim3((max_pad + kBlock - 1) / kBlock, M), dim3(kBlock), 0, st, F.segs.ptr, F.vals_alt.ptr);
  sink->launches += 5;
  // leaf slots first, then every internal level bottom-up (the root's own box is never needed)
  for (int step = 0; step < max_depth; step++) {
    const int64_t count = (int64_t)1 << (3 * (max_depth - step));
    hipLaunchKernelGGL(fb_boxes_kernel, dim3((unsigned)((count + kBlock - 1) / kBlock), M), dim3(kBlock), 0, st, F.segs.ptr, step);
    sink->launches++;
  }
  DGS_HIP_TRY(h, hipGetLastError());
  for (CloudState* c : todo) {
    c->bvh.kd = false;
    c->bvh.valid = true;
  }
  sink->built += M;
  return DGS_OK;
}

int fitness_batch_clouds(dgs_handle* h, int n_edges, dgs_cloud* const* cloud1s, dgs_cloud* const* cloud2s, const float* relposes16, double max_range,
                         double* scores, int64_t* used) {
  std::fill(h->fb.counts8, h->fb.counts8 + 8, 0);
  if (n_edges == 0) return DGS_OK;
  int rc = fb_build_counted(h, n_edges, cloud1s, nullptr);
  if (rc != DGS_OK) return rc;
  std::vector<FbEdgeIn> in((size_t)n_edges);
  for (int e = 0; e < n_edges; e++)
    in[e] = FbEdgeIn{&cloud1s[e]->st.bvh, cloud2s[e]->st.pts.ptr, cloud1s[e]->st.n, cloud2s[e]->st.n, relposes16 ? relposes16 + (size_t)e * 16 : kIdentity16};
  return fitness_batch_edges(h, n_edges, in.data(), max_range, scores, used);
}

// The walk and the closing launch over edges given as (index over cloud1, cloud2's points, pose): what fitness_batch_clouds runs once its
// clouds' indices stand, and what a batch-independent handle scores its own target's candidates with (fitness_target_edges).
// inlier false: fb_walk_kernel under max_range = `bound`, totals {sum, used}; true: fb_inlier_kernel under the strict threshold `bound`,
// totals {inliers, 0}.  *totals: 2 doubles per edge in the pinned block (zeros for an edge without rows), valid until the next call.
static int fb_run_edges(dgs_handle* h, int n_edges, const FbEdgeIn* in, bool inlier, double bound, const double** totals) {
  FbScratch& F = h->fb;
  F.counts8[2] = n_edges;
  // one pinned block: [row prefix | edge table] up, [sum, used per edge] down
  segtab::Layout L;
  L.take(((size_t)n_edges + 1) * sizeof(int), 128);
  const size_t pre_bytes = L.take((size_t)n_edges * sizeof(FbEdge), 128), up_bytes = L.end, down_bytes = (size_t)n_edges * 2 * sizeof(double);
  L.take(down_bytes, alignof(double));   // at up_bytes: a multiple of 128
  DGS_HIP_TRY(h, F.stage.reserve(L.end));
  int* row0s = reinterpret_cast<int*>(F.stage.ptr);
  FbEdge* edges = reinterpret_cast<FbEdge*>(F.stage.at(pre_bytes));
  double* down = reinterpret_cast<double*>(F.stage.at(up_bytes));
  int64_t total_rows = 0;
  for (int e = 0; e < n_edges; e++) {
    FbEdge& E = edges[e];
    std::memset(&E, 0, sizeof(E));
    const bool empty = in[e].n1 == 0 || in[e].n2 == 0;   // no neighbour / no query: the "nr == 0" branch of the reference
    if (!empty) {
      E.b = make_bvh_view(*in[e].index);
      E.src = in[e].src;
      E.n = (int)in[e].n2;
      E.rows = fb_rows_of(E.n);
    }
    E.row0 = (int)total_rows;
    std::memcpy(E.T, in[e].T16, sizeof(float) * 16);
    row0s[e] = (int)total_rows;
    total_rows += E.rows;
  }
  row0s[n_edges] = (int)total_rows;
  F.counts8[4] = total_rows;
  if (total_rows > 0) {
    hipStream_t st = h->stream;
    DGS_HIP_TRY(h, F.tab.reserve(up_bytes));
    DGS_HIP_TRY(h, F.rows.reserve((size_t)total_rows * 2 + (size_t)n_edges * 2));
    double* d_out = F.rows.ptr + (size_t)total_rows * 2;
    DGS_HIP_TRY(h, hipMemcpyAsync(F.tab.ptr, F.stage.ptr, up_bytes, hipMemcpyHostToDevice, st));
    const int* d_row0s = reinterpret_cast<const int*>(F.tab.ptr);
    const FbEdge* d_edges = reinterpret_cast<const FbEdge*>(F.tab.ptr + pre_bytes);
    // PCL's comparison is float(sq_dist) <= double(max_range); clamp so DBL_MAX keeps every finite distance (nn_fitness_enqueue clamps the
    // inlier threshold the same way)
    const float mr = (bound >= (double)FLT_MAX) ? FLT_MAX : (float)bound;
    hipLaunchKernelGGL(inlier ? fb_inlier_kernel : fb_walk_kernel, dim3((unsigned)total_rows), dim3(kBlock), 0, st, d_row0s, d_edges, n_edges, mr, F.rows.ptr);
    hipLaunchKernelGGL(fb_close_kernel, dim3(n_edges), dim3(kWave), 0, st, d_row0s, F.rows.ptr, n_edges, d_out);
    F.counts8[0] += 2;
    DGS_HIP_TRY(h, hipMemcpyAsync(down, d_out, down_bytes, hipMemcpyDeviceToHost, st));
    DGS_HIP_TRY(h, hipStreamSynchronize(st));
    F.counts8[1]++;
    F.bstage.settled();   // the build's upload went first on the same stream
    DGS_HIP_TRY(h, hipGetLastError());
  }
  for (int e = 0; e < n_edges; e++)
    if (!edges[e].rows) down[e * 2] = down[e * 2 + 1] = 0.0;
  *totals = down;
  return DGS_OK;
}

int fitness_batch_edges(dgs_handle* h, int n_edges, const FbEdgeIn* in, double max_range, double* scores, int64_t* used) {
  if (n_edges == 0) return DGS_OK;
  const double* down = nullptr;
  const int rc = fb_run_edges(h, n_edges, in, false, max_range, &down);
  if (rc != DGS_OK) return rc;
  for (int e = 0; e < n_edges; e++) {
    const double sum = down[e * 2], cnt = down[e * 2 + 1];
    scores[e] = cnt > 0.0 ? sum / cnt : DBL_MAX;
    if (used) used[e] = (int64_t)cnt;
  }
  return DGS_OK;
}

// dgs_calc_inlier_fraction_batch_clouds: missing indices by the batched build, one walk launch over all edges, one closing launch, one wait
int inlier_batch_clouds(dgs_handle* h, int n_edges, dgs_cloud* const* cloud1s, dgs_cloud* const* cloud2s, const float* relposes16, double max_sq_dist,
                        double* fractions, int64_t* inliers) {
  std::fill(h->fb.counts8, h->fb.counts8 + 8, 0);
  if (n_edges == 0) return DGS_OK;
  int rc = fb_build_counted(h, n_edges, cloud1s, nullptr);
  if (rc != DGS_OK) return rc;
  std::vector<FbEdgeIn> in((size_t)n_edges);
  for (int e = 0; e < n_edges; e++)
    in[e] = FbEdgeIn{&cloud1s[e]->st.bvh, cloud2s[e]->st.pts.ptr, cloud1s[e]->st.n, cloud2s[e]->st.n, relposes16 ? relposes16 + (size_t)e * 16 : kIdentity16};
  const double* down = nullptr;
  rc = fb_run_edges(h, n_edges, in.data(), true, max_sq_dist, &down);
  if (rc != DGS_OK) return rc;
  for (int e = 0; e < n_edges; e++) {
    const bool empty = in[e].n1 == 0 || in[e].n2 == 0;
    if (inliers) inliers[e] = empty ? 0 : (int64_t)down[e * 2];
    if (fractions) fractions[e] = empty ? (double)NAN : down[e * 2] / (double)in[e].n2;   // dgs_get_inlier_fraction's division
  }
  return DGS_OK;
}

int fitness_target_edges(dgs_handle* h, int n, const float4* const* srcs, const int64_t* sizes, const float* T16s, size_t T_stride_floats, double max_range, double* scores) {
  if (side_join(h) != DGS_OK) return DGS_ERR_HIP;   // an index being built on the side stream
  h->use_grid = false;                               // the edge scorer walks the tree
  int rc = ensure_target_index(h);
  if (rc != DGS_OK) return rc;
  std::fill(h->fb.counts8, h->fb.counts8 + 8, 0);
  std::vector<FbEdgeIn> in((size_t)n);
  for (int i = 0; i < n; i++) in[i] = FbEdgeIn{&h->tgt->bvh, srcs[i], h->nt, sizes[i], T16s + (size_t)i * T_stride_floats};
  return fitness_batch_edges(h, n, in.data(), max_range, scores, nullptr);
}

void fitness_batch_release(dgs_handle* h) {
  FbScratch& F = h->fb;
  F.tab.release(); F.rows.release(); F.segs.release(); F.mm.release(); F.keys.release(); F.keys_alt.release(); F.vals.release(); F.vals_alt.release();
  F.stage.release(); F.bstage.release();
}

}  // namespace dgs
