// LineBasedScanmatcher::edge_extraction (upstream src/hdl_graph_slam/line_based_scanmatcher.cpp:459-471, get_edges :501-682) on the
// device, for a batch of independent segments of lines: the edges of every segment in edge_extraction's order (pairs i < j ascending in
// (i, j), a pair's edges in the order of get_edges' four cases), bit for bit the host's.  The pair function is la::edge_pair
// (line_align.h), the one the host's get_edges calls: + - * /, sqrt, comparisons, fmin / fmax; the file is built without contraction and
// the device's f64 divide and square root are correctly rounded.
//
// MI355X design
//   * A pair is one lane.  A segment of n lines owns n * n consecutive pair slots p = pair_off + i * n + j; j <= i counts 0.  No integer
//     square root and no per-segment launch: the grid is the batch's slots in workgroups of 256, a lane finds its segment by bisection of
//     the segment table (at most 13 steps, L2 hits).
//   * le_count_kernel stores 0..4 per slot and the workgroup's sum; le_scan_kernel (one workgroup) turns the sums into offsets;
//     le_offsets_kernel reads every segment's first edge off them.  The host waits once for those n_seg + 1 integers: they size the edge
//     buffer, and the aligners need them for their hypothesis tables.  le_emit_kernel scans the stored counts inside the workgroup and
//     recomputes only the pairs that emit, each writing its edges at its offset.
//   * The lines are read from global memory, not staged in LDS: a workgroup of 256 consecutive slots reads line i (one address for all
//     lanes of a row) and up to 256 consecutive lines j, every one once, so an LDS copy would be written and read exactly once.  A
//     segment's lines (at most 24 KiB) stay in L2 across its workgroups.  The kernels use no LDS beyond a few words and are bound by the
//     FP64 divide and square-root sequences of la::edge_pair (up to 12 square roots and 20 divides per pair), not by memory.
// Semantics, limits and measurements: DESIGN.md 6l.
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstring>
#include <vector>

#include "handle.h"
#include "line_align.h"
#include "seg_table.h"

namespace dgs {

constexpr int kLeWaves = kBlock / kWave;
constexpr int kLeScanBlock = 1024;

__device__ __forceinline__ la::Line le_line(const double* __restrict__ lines, const int k) {
  la::Line l;
  l.a = la::load3(lines + 6 * (long long)k);
  l.b = la::load3(lines + 6 * (long long)k + 3);
  return l;
}
// the segment that owns slot p: the last one whose first slot is <= p (segments without slots share their successor's offset).
// p < all slots, so that segment's range holds p.
__device__ __forceinline__ int le_find(const LeSeg* __restrict__ segs, const int n, const long long p) {
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (segs[mid].pair_off <= p) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}
// the lines of slot p, or false for a slot with j <= i
__device__ __forceinline__ bool le_pair(const LeSeg* __restrict__ segs, const int n_seg, const double* __restrict__ lines, const long long p,
                                        la::Line* l1, la::Line* l2, LeSeg* sg) {
  *sg = segs[le_find(segs, n_seg, p)];
  const int local = (int)(p - sg->pair_off);          // < n * n <= 512 * 512, and n >= 1 because the segment has a slot
  const int i = local / sg->n, j = local % sg->n;
  if (j <= i) return false;
  *l1 = le_line(lines, sg->line_off + i);             // i < j < n: inside the segment's lines
  *l2 = le_line(lines, sg->line_off + j);
  return true;
}

__global__ __launch_bounds__(kBlock) void le_count_kernel(const LeSeg* __restrict__ segs, const int n_seg, const double* __restrict__ lines,
                                                          const long long P, unsigned char* __restrict__ cnt, int* __restrict__ blk) {
  __shared__ int s_w[kLeWaves];
  const long long p = (long long)blockIdx.x * kBlock + threadIdx.x;
  int c = 0;
  if (p < P) {
    la::Line l1, l2;
    LeSeg sg;
    if (le_pair(segs, n_seg, lines, p, &l1, &l2, &sg)) c = la::edge_pair<false>(l1, l2, sg.only_angular != 0, sg.max_dist, nullptr, 0);
    cnt[p] = (unsigned char)c;
  }
  int sum = c;
#pragma unroll
  for (int o = kWave / 2; o > 0; o >>= 1) sum += __shfl_xor(sum, o, kWave);
  if ((threadIdx.x & (kWave - 1)) == 0) s_w[threadIdx.x / kWave] = sum;
  __syncthreads();
  if (threadIdx.x == 0) {
    int t = 0;
    for (int w = 0; w < kLeWaves; w++) t += s_w[w];
    blk[blockIdx.x] = t;
  }
}

// blk[0 .. nb) -> their exclusive prefix sums in place, blk[nb] = the total.  One workgroup walks the array in chunks of its size.
__global__ __launch_bounds__(kLeScanBlock) void le_scan_kernel(int* __restrict__ blk, const int nb) {
  __shared__ int s_w[kLeScanBlock / kWave];
  __shared__ int s_carry;
  const int lane = threadIdx.x & (kWave - 1), wv = threadIdx.x / kWave;
  if (threadIdx.x == 0) s_carry = 0;
  __syncthreads();
  for (int base = 0; base < nb; base += kLeScanBlock) {   // uniform
    const int i = base + threadIdx.x;
    const int v = i < nb ? blk[i] : 0;
    int x = v;
#pragma unroll
    for (int o = 1; o < kWave; o <<= 1) {
      const int y = __shfl_up(x, o, kWave);
      if (lane >= o) x += y;
    }
    if (lane == kWave - 1) s_w[wv] = x;
    __syncthreads();
    int before = s_carry, all = 0;
    for (int w = 0; w < kLeScanBlock / kWave; w++) {
      if (w < wv) before += s_w[w];
      all += s_w[w];
    }
    if (i < nb) blk[i] = before + x - v;
    __syncthreads();
    if (threadIdx.x == 0) s_carry += all;
    __syncthreads();
  }
  if (threadIdx.x == 0) blk[nb] = s_carry;
}

// eoff[s]: the edges in front of segment s's first slot; eoff[n_seg]: all edges
__global__ __launch_bounds__(kBlock) void le_offsets_kernel(const LeSeg* __restrict__ segs, const int n_seg, const long long P,
                                                            const unsigned char* __restrict__ cnt, const int* __restrict__ blk, int* __restrict__ eoff) {
  const int s = blockIdx.x * kBlock + threadIdx.x;
  if (s > n_seg) return;
  const long long p = s < n_seg ? segs[s].pair_off : P;   // <= P
  const long long b = p / kBlock;                         // <= nb, and blk has nb + 1 entries
  int off = blk[b];
  for (long long q = b * kBlock; q < p; q++) off += cnt[q];   // q < p <= P
  eoff[s] = off;
}

__global__ __launch_bounds__(kBlock) void le_emit_kernel(const LeSeg* __restrict__ segs, const int n_seg, const double* __restrict__ lines,
                                                         const long long P, const unsigned char* __restrict__ cnt, const int* __restrict__ blk,
                                                         double* __restrict__ edges) {
  __shared__ int s_w[kLeWaves];
  const int lane = threadIdx.x & (kWave - 1), wv = threadIdx.x / kWave;
  const long long p = (long long)blockIdx.x * kBlock + threadIdx.x;
  const int c = p < P ? cnt[p] : 0;
  int x = c;
#pragma unroll
  for (int o = 1; o < kWave; o <<= 1) {
    const int y = __shfl_up(x, o, kWave);
    if (lane >= o) x += y;
  }
  if (lane == kWave - 1) s_w[wv] = x;
  __syncthreads();
  if (c == 0) return;
  int off = blk[blockIdx.x] + x - c;
  for (int w = 0; w < wv; w++) off += s_w[w];
  la::Line l1, l2;
  LeSeg sg;
  if (!le_pair(segs, n_seg, lines, p, &l1, &l2, &sg)) return;   // not taken: c > 0 only where j > i
  // off + c <= all edges (the scan of these very counts), which is what `edges` holds; the pair emits c edges again (same inputs, same
  // operations), and at most c are written whatever it computes
  la::edge_pair<true>(l1, l2, sg.only_angular != 0, sg.max_dist, reinterpret_cast<la::Edge*>(edges) + off, c);
}
static_assert(sizeof(la::Edge) == 9 * sizeof(double) && sizeof(dgs_edge_feature) == sizeof(la::Edge), "an edge is nine doubles on both sides");

// ================================================================================================ host side
namespace {

// the pinned block: the segment table | the edge offsets' download (n_seg + 1 ints), both from a multiple of 8 on; L.end is one as well
struct LeTable {
  segtab::Layout L;
  size_t down;
};
inline LeTable le_table(size_t n_seg) {
  LeTable T;
  T.L.take(n_seg * sizeof(LeSeg), 8);
  T.down = T.L.take((n_seg + 1) * sizeof(int), 8);
  T.L.take(0, 8);
  return T;
}

}  // namespace

int line_edges_run(dgs_handle* h, const double* d_lines, const std::vector<LeSeg>& segs, const bool emit) {
  LeScratch& s = h->le;
  const size_t n_seg = segs.size();
  const long long P = la::pair_slots(segs);
  long long tri = 0;
  for (const LeSeg& g : segs) tri += (long long)g.n * (g.n - 1) / 2;
  s.eoff_host.assign(n_seg + 1, 0);
  s.counts4[0] = s.counts4[1] = s.counts4[3] = 0;
  s.counts4[2] = tri;
  if (P == 0) return DGS_OK;
  const int nb = (int)((P + kBlock - 1) / kBlock);
  DGS_HIP_TRY(h, s.segs.reserve(n_seg));
  DGS_HIP_TRY(h, s.cnt.reserve((size_t)P));
  DGS_HIP_TRY(h, s.blk.reserve((size_t)nb + 1));
  DGS_HIP_TRY(h, s.eoff.reserve(n_seg + 1));
  const LeTable T = le_table(n_seg);
  DGS_HIP_TRY(h, s.stage.reserve(T.L.end));
  char* up = s.stage.at(0);
  int* down = reinterpret_cast<int*>(s.stage.at(T.down));
  std::memcpy(up, segs.data(), n_seg * sizeof(LeSeg));
  DGS_HIP_TRY(h, hipMemcpyAsync(s.segs.ptr, up, n_seg * sizeof(LeSeg), hipMemcpyHostToDevice, h->stream));
  hipLaunchKernelGGL(le_count_kernel, dim3((unsigned)nb), dim3(kBlock), 0, h->stream, s.segs.ptr, (int)n_seg, d_lines, P, s.cnt.ptr, s.blk.ptr);
  hipLaunchKernelGGL(le_scan_kernel, dim3(1), dim3(kLeScanBlock), 0, h->stream, s.blk.ptr, nb);
  hipLaunchKernelGGL(le_offsets_kernel, dim3((unsigned)((n_seg + 1 + kBlock - 1) / kBlock)), dim3(kBlock), 0, h->stream, s.segs.ptr, (int)n_seg, P,
                     s.cnt.ptr, s.blk.ptr, s.eoff.ptr);
  s.counts4[0] += 3;
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipMemcpyAsync(down, s.eoff.ptr, (n_seg + 1) * sizeof(int), hipMemcpyDeviceToHost, h->stream);
  const hipError_t e2 = hipStreamSynchronize(h->stream);   // the wait for the edge offsets, also on the error path
  s.counts4[1] += 1;
  DGS_HIP_TRY(h, e);
  DGS_HIP_TRY(h, e2);
  std::memcpy(s.eoff_host.data(), down, (n_seg + 1) * sizeof(int));
  const int total = s.eoff_host[n_seg];
  s.counts4[3] = total;
  if (!emit || total == 0) return DGS_OK;
  DGS_HIP_TRY(h, s.edges.reserve((size_t)total * 9));
  hipLaunchKernelGGL(le_emit_kernel, dim3((unsigned)nb), dim3(kBlock), 0, h->stream, s.segs.ptr, (int)n_seg, d_lines, P, s.cnt.ptr, s.blk.ptr, s.edges.ptr);
  s.counts4[0] += 1;
  DGS_HIP_TRY(h, hipGetLastError());
  return DGS_OK;
}

void line_edges_release(dgs_handle* h) {
  LeScratch& s = h->le;
  s.lines.release(); s.segs.release(); s.cnt.release(); s.blk.release(); s.eoff.release(); s.edges.release(); s.stage.release();
  s.eoff_host.clear();
}

}  // namespace dgs

using namespace dgs;

extern "C" {

int dgs_line_edge_extraction_batch(dgs_handle* h, const dgs_line_feature* lines, const int64_t* offsets, int64_t n_items, const int32_t* only_angular,
                                   const double* max_dist, dgs_edge_feature* edges, int64_t capacity, int64_t* edge_offsets, int64_t* n_edges) {
  // the arguments first, the handle last: what is wrong with a call does not depend on where it would run
  const char* why = nullptr;
  if (n_items < 0 || !n_edges || capacity < 0 || (capacity > 0 && !edges) || (n_items > 0 && (!offsets || !only_angular || !max_dist)))
    why = "line edges: a required argument is NULL or negative";
  else if (n_items > DGS_LA_MAX_ITEMS) why = "line edges: more than DGS_LA_MAX_ITEMS segments";
  else if (n_items > 0 && offsets[0] != 0) why = "line edges: the first offset is not 0";
  long long slots = 0;
  for (int64_t b = 0; b < n_items && !why; b++) {
    const int64_t n = offsets[b + 1] - offsets[b];
    if (n < 0) why = "line edges: offsets are not ascending";
    else if (n > DGS_LA_MAX_LINES_TARGET) why = "line edges: more than DGS_LA_MAX_LINES_TARGET lines in a segment";
    else if (std::isnan(max_dist[b])) why = "line edges: a max_dist is NaN";
    else if ((slots += n * n) > DGS_LA_MAX_EDGE_PAIRS) why = "line edges: more than DGS_LA_MAX_EDGE_PAIRS pairs (the squares of the segments' line counts, summed)";
  }
  const int64_t n_lines = why || n_items == 0 ? 0 : offsets[n_items];
  if (!why && n_lines > 0 && !lines) why = "line edges: the line array is NULL";
  if (!why && !la::all_finite(lines, n_lines)) why = "line edges: a line coordinate is not finite";
  if (!why && !h) why = "line edges: the handle is NULL";
  if (why) {
    if (h) h->err = why;
    else set_handleless_error(why);
    return DGS_ERR_INVALID_ARGUMENT;
  }
  h->err.clear();
  *n_edges = 0;
  std::vector<LeSeg> segs;
  for (int64_t b = 0; b < n_items; b++) la::add_segment(&segs, (int)offsets[b], (int)(offsets[b + 1] - offsets[b]), only_angular[b] != 0, max_dist[b]);
  LeScratch& s = h->le;
  DGS_HIP_TRY(h, hipSetDevice(h->device));
  // one pinned block: the segment table and the offsets' download (line_edges_run), behind them the packed lines
  segtab::Layout L = le_table(segs.size()).L;
  const size_t b_lines = (size_t)n_lines * 6 * sizeof(double), b_tab = L.take(b_lines, alignof(double));
  DGS_HIP_TRY(h, s.stage.reserve(L.end));
  DGS_HIP_TRY(h, s.lines.reserve(std::max<size_t>((size_t)n_lines * 6, 1)));
  if (n_lines) {
    double* up = reinterpret_cast<double*>(s.stage.at(b_tab));
    la::pack_lines(la::lines_of(lines, n_lines), up);
    DGS_HIP_TRY(h, hipMemcpyAsync(s.lines.ptr, up, b_lines, hipMemcpyHostToDevice, h->stream));
  }
  // without room for the edges only their number is wanted: the first run stops after the counts
  int rc = line_edges_run(h, s.lines.ptr, segs, capacity > 0);
  if (rc != DGS_OK) {
    (void)hipStreamSynchronize(h->stream);
    return rc;
  }
  const int64_t total = s.eoff_host[segs.size()];
  *n_edges = total;
  if (edge_offsets)
    for (size_t b = 0; b <= segs.size(); b++) edge_offsets[b] = s.eoff_host[b];
  if (total > capacity) {
    (void)hipStreamSynchronize(h->stream);   // the emit pass, if it ran, is not left pending
    h->err = "line edges: more edges than capacity";
    return DGS_ERR_INVALID_ARGUMENT;
  }
  if (total > 0) {
    DGS_HIP_TRY(h, hipMemcpyAsync(edges, s.edges.ptr, (size_t)total * sizeof(dgs_edge_feature), hipMemcpyDeviceToHost, h->stream));
    DGS_HIP_TRY(h, hipStreamSynchronize(h->stream));
    s.counts4[1] += 1;
  }
  return DGS_OK;
}

int dgs_line_edge_extraction(dgs_handle* h, const dgs_line_feature* lines, int64_t n, int32_t only_angular_edges, double max_dist_angular_edge,
                             dgs_edge_feature* edges, int64_t capacity, int64_t* n_edges) {
  const int64_t off[2] = {0, n};
  return dgs_line_edge_extraction_batch(h, lines, off, 1, &only_angular_edges, &max_dist_angular_edge, edges, capacity, nullptr, n_edges);
}

int dgs_line_edges_get_counts(dgs_handle* h, int64_t* counts4) {
  if (!h || !counts4) return DGS_ERR_INVALID_ARGUMENT;
  for (int k = 0; k < 4; k++) counts4[k] = h->le.counts4[k];
  return DGS_OK;
}

}  // extern "C"
