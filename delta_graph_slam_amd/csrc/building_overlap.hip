// are_buildings_overlapped over every pair of buildings (upstream include/hdl_graph_slam/check_overlapping.hpp with getOverlappedBuildings,
// apps/delta_graph_slam_nodelet.cpp:767-787) and LineBasedScanmatcher::align_overlapped_buildings (src/hdl_graph_slam/
// line_based_scanmatcher.cpp:29-107) for a batch of overlapped pairs, on the device.  The scalar functions are building_overlap.h's and
// line_align.h's, shared with the host restatements the tests compare against.
//
// MI355X design
//   * Pair search, five launches whatever the number of buildings B, one upload, one download, one host wait:
//       bo_shrink_kernel   a lane per line: the line shrunk toward its own building's centre, once, into a packed x1 y1 x2 y2 table;
//       bo_flag_kernel     a workgroup owns kBoTileRows rows i with their shrunken lines in LDS (32 KiB); its four waves stride over
//                          the 64-wide chunks of j > i, lanes stride over the La x Lb line pairs of one building pair, __any gives the
//                          pair's flag and the wave keeps the chunk's 64 flags as one word per row: bits[i][j / 64];
//       bo_count_kernel    a wave per row: the popcount of its words;
//       bo_scan_kernel     one workgroup: the exclusive scan of the row counts and the total;
//       bo_emit_kernel     a wave per row: lane l owns bit l of a word, its position is the row's offset plus the popcount of the bits
//                          below it, so the list is (i ascending, j ascending) with no atomics and does not depend on the launch shape.
//     The predicate accepts rounded points outside a segment's box, so there is no bounding-box culling: exact brute force.
//   * Alignment, three launches whatever the number of items: bo_hypothesis_kernel (a lane per hypothesis of the batch: the transform,
//     its norm, the angle gate), bo_overlap_kernel (a wave per angle-passing hypothesis against the item's shrunken target table in LDS,
//     lanes over the Ls x Lt line pairs, __any gives the overlap flag), bo_argmin_kernel (a workgroup per item: the arg-min in h order,
//     the record, the aligned lines).  Nothing is accumulated across waves or with atomics: an item's bits do not depend on the batch.
// Semantics, limits and memory: DESIGN.md 6h.
#include <algorithm>
#include <cfloat>
#include <climits>
#include <cmath>
#include <cstddef>
#include <cstring>
#include <vector>

#include "handle.h"
#include "building_overlap.h"

namespace dgs {

constexpr int kBoTileRows = 2;          // rows i per workgroup of bo_flag_kernel: 2 x 512 lines x 32 bytes of LDS
constexpr int kBoWaves = kBlock / kWave;
constexpr int kBoUnits = 16;            // hypotheses per workgroup of bo_overlap_kernel: four per wave
constexpr int kBoSegDoubles = 4;

struct BoHyp {
  la::Tf t;
  double tn;            // translation.norm()
  int gate, pad;
};
static_assert(sizeof(BoHyp) == 72, "DESIGN.md 6h and dgs_reg.h state 72 bytes per hypothesis");

struct BoItem {
  int Ls, Lt, Es, Et;
  int src_off, trg_off, es_off, et_off;   // first source line, target line, source edge and target edge of the item in the batch's arrays
  long long h_off;                        // first hypothesis of the item
  double cs[2], ct[2];                    // x and y of center_source and center_target
};

struct BoRecord {
  la::Tf t;
  double tn;
  long long winner, n_angle_passed, n_not_overlapped;
};

// the last entry of the ascending table `off` (n entries) that is <= v: the building of a line, the item of a hypothesis (empty ones share
// their successor's offset).  v < the total, so the result's range holds v.
template <typename T>
__device__ __forceinline__ int bo_find(const T* __restrict__ off, const int n, const T v) {
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (off[mid] <= v) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

// ================================================================================================ pair search
__global__ __launch_bounds__(kBlock) void bo_shrink_kernel(const int* __restrict__ off, const double* __restrict__ ctr, const double* __restrict__ pts,
                                                           const int B, const int n_lines, double* __restrict__ shr) {
  const int l = blockIdx.x * kBlock + threadIdx.x;
  if (l >= n_lines) return;
  const int b = bo_find<int>(off, B, l);
  const double* p = pts + (long long)kBoSegDoubles * l;
  bo::store_seg(shr + (long long)kBoSegDoubles * l, bo::shrink_line(la::v3(p[0], p[1], 0.0), la::v3(p[2], p[3], 0.0), ctr[2 * b], ctr[2 * b + 1]));
}

// does any (line of the row in LDS, line of building j) pair intersect?  Uniform over the wave.
__device__ __forceinline__ bool bo_pair_wave(const double* s_a, const int La, const double* __restrict__ b_lines, const int Lb, const int lane) {
  const int n = La * Lb;                                              // <= 512 * 512
  for (int p0 = 0; p0 < n; p0 += kWave) {
    const int p = p0 + lane;
    bool x = false;
    if (p < n) {
      const int a = p / Lb, b = p - a * Lb;
      x = bo::lines_intersected(bo::load_seg(s_a + kBoSegDoubles * a), bo::load_seg(b_lines + kBoSegDoubles * b));
    }
    if (__any(x ? 1 : 0)) return true;                                // upstream's early return: the value is the same
  }
  return false;
}

__global__ __launch_bounds__(kBlock) void bo_flag_kernel(const int* __restrict__ off, const double* __restrict__ shr, const int B, const int W,
                                                         unsigned long long* __restrict__ bits) {
  __shared__ double s_row[kBoTileRows][DGS_LA_MAX_LINES_TARGET * kBoSegDoubles];
  const int i0 = blockIdx.x * kBoTileRows;
  if (i0 >= B) return;                                                // uniform
  int cnt[kBoTileRows];
#pragma unroll
  for (int r = 0; r < kBoTileRows; r++) {
    cnt[r] = 0;
    if (i0 + r < B) {
      const int first = off[i0 + r];
      cnt[r] = off[i0 + r + 1] - first;                               // <= DGS_LA_MAX_LINES_TARGET (checked on the host)
      for (int k = threadIdx.x; k < cnt[r] * kBoSegDoubles; k += kBlock) s_row[r][k] = shr[(long long)kBoSegDoubles * first + k];
    }
  }
  __syncthreads();
  const int lane = threadIdx.x & (kWave - 1), wv = threadIdx.x / kWave;
  for (int c = (i0 + 1) / kWave + wv; c < W; c += kBoWaves) {         // from the first chunk that holds a j > i0; uniform per wave
    unsigned long long m[kBoTileRows];
#pragma unroll
    for (int r = 0; r < kBoTileRows; r++) m[r] = 0ull;
    const int j_end = min(kWave * c + kWave, B);
    for (int j = max(kWave * c, i0 + 1); j < j_end; j++) {
      const int fb = off[j], Lb = off[j + 1] - fb;
      const double* bl = shr + (long long)kBoSegDoubles * fb;
#pragma unroll
      for (int r = 0; r < kBoTileRows; r++)
        if (j > i0 + r && i0 + r < B && bo_pair_wave(s_row[r], cnt[r], bl, Lb, lane)) m[r] |= 1ull << (j & (kWave - 1));
    }
    if (lane == 0) {
#pragma unroll
      for (int r = 0; r < kBoTileRows; r++)
        if (i0 + r < B) bits[(long long)(i0 + r) * W + c] = m[r];     // row < B, c < W: inside B * W words
    }
  }
}
static_assert(kWave == 64, "a chunk of j is one 64-bit word");

// Row i reads its words from chunk (i + 1) / 64 on: the chunks before it hold no j > i and are never written.
__global__ __launch_bounds__(kBlock) void bo_count_kernel(const unsigned long long* __restrict__ bits, const int B, const int W, int* __restrict__ row) {
  const int lane = threadIdx.x & (kWave - 1), i = blockIdx.x * kBoWaves + threadIdx.x / kWave;
  if (i >= B) return;                                                 // uniform per wave
  int n = 0;
  for (int c = (i + 1) / kWave + lane; c < W; c += kWave) n += __popcll(bits[(long long)i * W + c]);
#pragma unroll
  for (int o = kWave / 2; o > 0; o >>= 1) n += __shfl_xor(n, o, kWave);
  if (lane == 0) row[i] = n;
}

// One workgroup: row[0 .. B) becomes its exclusive scan, row[B] the total (< 2^27: B <= DGS_BO_MAX_BUILDINGS).
__global__ __launch_bounds__(kBlock) void bo_scan_kernel(int* __restrict__ row, const int B) {
  __shared__ int s_part[kBlock];
  const int per = (B + kBlock - 1) / kBlock;
  const int b0 = min((int)threadIdx.x * per, B), b1 = min(b0 + per, B);
  int sum = 0;
  for (int k = b0; k < b1; k++) sum += row[k];
  s_part[threadIdx.x] = sum;
  __syncthreads();
  if (threadIdx.x == 0) {
    int run = 0;
    for (int t = 0; t < kBlock; t++) {
      const int v = s_part[t];
      s_part[t] = run;
      run += v;
    }
    row[B] = run;
  }
  __syncthreads();
  int run = s_part[threadIdx.x];
  for (int k = b0; k < b1; k++) {
    const int v = row[k];
    row[k] = run;
    run += v;
  }
}

__global__ __launch_bounds__(kBlock) void bo_emit_kernel(const unsigned long long* __restrict__ bits, const int* __restrict__ row, const int B, const int W,
                                                         int2* __restrict__ pairs, const long long capacity, long long* __restrict__ total) {
  const int lane = threadIdx.x & (kWave - 1), i = blockIdx.x * kBoWaves + threadIdx.x / kWave;
  if (blockIdx.x == 0 && threadIdx.x == 0) *total = row[B];
  if (i >= B) return;                                                 // uniform per wave
  long long base = row[i];
  for (int c0 = (i + 1) / kWave; c0 < W; c0 += kWave) {                // 64 words per step, one per lane
    const int c = c0 + lane;
    const unsigned long long w = c < W ? bits[(long long)i * W + c] : 0ull;
    unsigned long long nz = __ballot(w != 0ull);
    while (nz) {                                                      // uniform: the words that hold a pair, ascending
      const int k = __ffsll((long long)nz) - 1;
      nz &= nz - 1;
      const unsigned long long ww = (unsigned long long)__shfl((long long)w, k, kWave);
      if ((ww >> lane) & 1ull) {
        const long long pos = base + __popcll(ww & ((1ull << lane) - 1ull));
        if (pos < capacity) pairs[pos] = make_int2(i, kWave * (c0 + k) + lane);   // the download holds min(capacity, total) pairs
      }
      base += __popcll(ww);
    }
  }
}

// ================================================================================================ alignment
__global__ __launch_bounds__(kBlock) void bo_hypothesis_kernel(const BoItem* __restrict__ items, const int n_items, const long long H,
                                                               const double* __restrict__ src, const double* __restrict__ trg,
                                                               const double* __restrict__ es, const double* __restrict__ et, const double cos_max_angle,
                                                               const int float_chain, BoHyp* __restrict__ hyps) {
  const long long g = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (g >= H) return;
  // the item that owns g: the last one whose first hypothesis is <= g
  int lo = 0, hi = n_items - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (items[mid].h_off <= g) lo = mid;
    else hi = mid - 1;
  }
  const BoItem it = items[lo];
  const long long h = g - it.h_off, n_edge = (long long)it.Es * it.Et;   // 0 <= h < Es * Et + Ls * Lt of this item
  BoHyp hy;
  if (h < n_edge) {
    const int is = it.es_off + (int)(h / it.Et), ie = it.et_off + (int)(h % it.Et);
    hy.t = la::align_edges(la::load_edge(es + 9 * (long long)is), la::load_edge(et + 9 * (long long)ie), nullptr);
  } else {
    const long long k = h - n_edge;
    const double* s = src + 6 * ((long long)it.src_off + k / it.Lt);
    const double* t = trg + 6 * ((long long)it.trg_off + k % it.Lt);
    la::Line ls, lt;
    ls.a = la::load3(s); ls.b = la::load3(s + 3);
    lt.a = la::load3(t); lt.b = la::load3(t + 3);
    hy.t = la::align_lines(ls, lt);
  }
  hy.gate = bo::gate_angle_only(hy.t, cos_max_angle, float_chain, &hy.tn);
  hy.pad = 0;
  hyps[g] = hy;
}

__global__ __launch_bounds__(kBlock) void bo_overlap_kernel(const BoItem* __restrict__ items, const int2* __restrict__ wg, const int n_wg,
                                                            const double* __restrict__ src, const double* __restrict__ trg, BoHyp* __restrict__ hyps) {
  __shared__ double s_t[DGS_LA_MAX_LINES_TARGET * kBoSegDoubles];
  if ((int)blockIdx.x >= n_wg) return;                                // uniform: the grid is at least one workgroup
  const int2 w = wg[blockIdx.x];
  const BoItem it = items[w.x];
  for (int j = threadIdx.x; j < it.Lt; j += kBlock) {                 // Lt <= DGS_LA_MAX_LINES_TARGET (checked on the host)
    const double* t = trg + 6 * ((long long)it.trg_off + j);
    bo::store_seg(s_t + kBoSegDoubles * j, bo::shrink_line(la::load3(t), la::load3(t + 3), it.ct[0], it.ct[1]));
  }
  __syncthreads();
  const int lane = threadIdx.x & (kWave - 1), wv = threadIdx.x / kWave;
  const long long H = (long long)it.Es * it.Et + (long long)it.Ls * it.Lt;
  const long long end = min((long long)w.y + kBoUnits, H);
  const int n = it.Ls * it.Lt;                                        // <= 256 * 512
  for (long long u = (long long)w.y + wv; u < end; u += kBoWaves) {   // uniform per wave
    const long long idx = it.h_off + u;
    const BoHyp hy = hyps[idx];
    if (hy.gate != la::GATE_PASS) continue;
    bool hit = false;
    for (int p0 = 0; p0 < n && !hit; p0 += kWave) {
      const int p = p0 + lane;
      bool x = false;
      if (p < n) {
        const int a = p / it.Lt, b = p - a * it.Lt;
        const double* s = src + 6 * ((long long)it.src_off + a);
        // transform_lines, then shrink_polygon toward the unmoved source centre
        const bo::Seg moved = bo::shrink_line(la::apply(hy.t, la::load3(s)), la::apply(hy.t, la::load3(s + 3)), it.cs[0], it.cs[1]);
        x = bo::lines_intersected(moved, bo::load_seg(s_t + kBoSegDoubles * b));
      }
      hit = __any(x ? 1 : 0) != 0;
    }
    if (hit && lane == 0) hyps[idx].gate = bo::GATE_OVERLAP;
  }
}

// One workgroup per item: the lowest h among the smallest norms that passed both gates, the record and the aligned lines.
__global__ __launch_bounds__(kBlock) void bo_argmin_kernel(const BoItem* __restrict__ items, const int n_items, const double* __restrict__ src,
                                                           const BoHyp* __restrict__ hyps, BoRecord* __restrict__ rec, double* __restrict__ aligned) {
  __shared__ double s_s[kBoWaves];
  __shared__ int s_h[kBoWaves], s_a[kBoWaves], s_f[kBoWaves];
  __shared__ int s_win;
  if ((int)blockIdx.x >= n_items) return;
  const BoItem it = items[blockIdx.x];
  const int H = (int)((long long)it.Es * it.Et + (long long)it.Ls * it.Lt);   // <= DGS_LA_MAX_HYPOTHESES
  double best = DBL_MAX;
  int bh = -1, n_angle = 0, n_free = 0;
  for (int h = threadIdx.x; h < H; h += kBlock) {                     // h ascends per lane: the first of equal norms stays
    const BoHyp hy = hyps[it.h_off + h];
    if (hy.gate != la::GATE_ANGLE) n_angle++;
    if (hy.gate != la::GATE_PASS) continue;
    n_free++;
    if (hy.tn < best) { best = hy.tn; bh = h; }                       // a NaN norm, or one not below DBL_MAX, never takes over
  }
  bo::argmin_wave(best, bh);
#pragma unroll
  for (int o = kWave / 2; o > 0; o >>= 1) {
    n_angle += __shfl_xor(n_angle, o, kWave);
    n_free += __shfl_xor(n_free, o, kWave);
  }
  const int lane = threadIdx.x & (kWave - 1), wv = threadIdx.x / kWave;
  if (lane == 0) { s_s[wv] = best; s_h[wv] = bh; s_a[wv] = n_angle; s_f[wv] = n_free; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < kBoWaves; w++) {
      if (bo::takes_under(s_s[w], s_h[w], best, bh)) { best = s_s[w]; bh = s_h[w]; }
      n_angle += s_a[w];
      n_free += s_f[w];
    }
    BoRecord r;
    r.t = bh >= 0 ? hyps[it.h_off + bh].t : la::tf_identity();
    r.tn = best;
    r.winner = bh;
    r.n_angle_passed = n_angle;
    r.n_not_overlapped = n_free;
    rec[blockIdx.x] = r;
    s_win = bh;
  }
  __syncthreads();
  const int win = s_win;
  la::Tf t = la::tf_identity();
  if (win >= 0) t = hyps[it.h_off + win].t;
  for (int k = threadIdx.x; k < 2 * it.Ls; k += kBlock) {              // transform_lines(linesSource, transform), or the source lines as they are
    const long long p = 3 * (2 * (long long)it.src_off + k);
    la::V3 v = la::load3(src + p);
    if (win >= 0) v = la::apply(t, v);
    la::store3(aligned + p, v);
  }
}

// ================================================================================================ host side
namespace {

inline size_t bo_align8(size_t b) { return (b + 7) & ~(size_t)7; }
inline dim3 bo_blocks(long long n, int per) { return dim3((unsigned)std::max<long long>((n + per - 1) / per, 1)); }
inline bool bo_finite3(const double* c, int64_t n) {
  for (int64_t i = 0; i < 3 * n; i++)
    if (!std::isfinite(c[i])) return false;
  return true;
}

}  // namespace

void building_overlap_release(dgs_handle* h) {
  BoScratch& s = h->bo;
  s.in.release(); s.shr.release(); s.bits.release(); s.row.release(); s.out.release();
  s.ain.release(); s.hyps.release(); s.aout.release();
  s.off.clear();
}

}  // namespace dgs

using namespace dgs;

extern "C" {

int dgs_building_overlap_pairs(dgs_handle* h, const dgs_line_feature* lines, const int64_t* line_offsets, const double* centers, int64_t n_buildings,
                               int32_t* pairs, int64_t capacity, int64_t* n_pairs) {
  if (!h || !n_pairs || n_buildings < 0 || capacity < 0 || (capacity > 0 && !pairs) || (n_buildings > 0 && (!line_offsets || !centers)))
    return DGS_ERR_INVALID_ARGUMENT;
  h->err.clear();
  BoScratch& s = h->bo;
  for (int k = 0; k < 4; k++) s.counts8[k] = 0;
  *n_pairs = 0;
  if (n_buildings == 0) return DGS_OK;
  const char* why = nullptr;
  if (n_buildings > DGS_BO_MAX_BUILDINGS) why = "building overlap: more than DGS_BO_MAX_BUILDINGS buildings";
  else if (line_offsets[0] != 0) why = "building overlap: the first offset is not 0";
  for (int64_t b = 0; b < n_buildings && !why; b++) {
    const int64_t l = line_offsets[b + 1] - line_offsets[b];
    if (l < 0) why = "building overlap: offsets are not ascending";
    else if (l > DGS_LA_MAX_LINES_TARGET) why = "building overlap: more than DGS_LA_MAX_LINES_TARGET lines in a building";
  }
  const int64_t n_lines = why ? 0 : line_offsets[n_buildings];
  if (!why && n_lines > 0 && !lines) why = "building overlap: the line array is NULL";
  if (!why && (!la::all_finite(lines, n_lines) || !bo_finite3(centers, n_buildings))) why = "building overlap: a coordinate is not finite";
  if (why) {
    h->err = why;
    return DGS_ERR_INVALID_ARGUMENT;
  }
  s.counts8[2] = n_buildings;
  if (n_buildings == 1) return DGS_OK;                                 // no pair: nothing to launch
  const int B = (int)n_buildings, W = (B + kWave - 1) / kWave, N = (int)n_lines;   // N <= 2^14 * 512
  const long long max_pairs = (long long)B * (B - 1) / 2, cap = std::min<long long>(capacity, max_pairs);

  // ---- one upload: offsets, centres (x, y), line end points (x, y)
  const size_t b_off = bo_align8((size_t)(B + 1) * sizeof(int)), b_in = b_off + ((size_t)2 * B + (size_t)kBoSegDoubles * N) * sizeof(double);
  const size_t b_out = sizeof(long long) + (size_t)cap * sizeof(int2);
  DGS_HIP_TRY(h, hipSetDevice(h->device));
  DGS_HIP_TRY(h, s.in.reserve(b_in));
  DGS_HIP_TRY(h, s.shr.reserve(std::max<size_t>((size_t)kBoSegDoubles * N, 1)));
  DGS_HIP_TRY(h, s.bits.reserve((size_t)B * W));
  DGS_HIP_TRY(h, s.row.reserve((size_t)B + 1));
  DGS_HIP_TRY(h, s.out.reserve(b_out));
  if (ensure_pinned(h, b_in + b_out) != DGS_OK) return DGS_ERR_HIP;
  char* up = static_cast<char*>(h->pinned);
  char* down = up + b_in;                                              // b_in is a multiple of 8
  int* u_off = reinterpret_cast<int*>(up);
  for (int b = 0; b <= B; b++) u_off[b] = (int)line_offsets[b];
  double* o = reinterpret_cast<double*>(up + b_off);
  for (int b = 0; b < B; b++) { *o++ = centers[3 * b]; *o++ = centers[3 * b + 1]; }
  for (int l = 0; l < N; l++) { *o++ = lines[l].point_a[0]; *o++ = lines[l].point_a[1]; *o++ = lines[l].point_b[0]; *o++ = lines[l].point_b[1]; }
  DGS_HIP_TRY(h, hipMemcpyAsync(s.in.ptr, up, b_in, hipMemcpyHostToDevice, h->stream));
  const int* d_off = reinterpret_cast<const int*>(s.in.ptr);
  const double* d_ctr = reinterpret_cast<const double*>(s.in.ptr + b_off);
  const double* d_pts = d_ctr + 2 * (size_t)B;
  long long* d_total = reinterpret_cast<long long*>(s.out.ptr);
  int2* d_pairs = reinterpret_cast<int2*>(s.out.ptr + sizeof(long long));

  // ---- five launches whatever B, counted where they are issued
#define BO_LAUNCH(...)                  \
  do {                                  \
    hipLaunchKernelGGL(__VA_ARGS__);    \
    s.counts8[0]++;                     \
  } while (0)
  const dim3 blk(kBlock);
  BO_LAUNCH(bo_shrink_kernel, bo_blocks(N, kBlock), blk, 0, h->stream, d_off, d_ctr, d_pts, B, N, s.shr.ptr);
  BO_LAUNCH(bo_flag_kernel, bo_blocks(B, kBoTileRows), blk, 0, h->stream, d_off, s.shr.ptr, B, W, s.bits.ptr);
  BO_LAUNCH(bo_count_kernel, bo_blocks(B, kBoWaves), blk, 0, h->stream, s.bits.ptr, B, W, s.row.ptr);
  BO_LAUNCH(bo_scan_kernel, dim3(1), blk, 0, h->stream, s.row.ptr, B);
  BO_LAUNCH(bo_emit_kernel, bo_blocks(B, kBoWaves), blk, 0, h->stream, s.bits.ptr, s.row.ptr, B, W, d_pairs, cap, d_total);
#undef BO_LAUNCH
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipMemcpyAsync(down, s.out.ptr, b_out, hipMemcpyDeviceToHost, h->stream);
  const hipError_t e2 = hipStreamSynchronize(h->stream);               // the one host wait, also on the error path
  s.counts8[1] = 1;
  DGS_HIP_TRY(h, e);
  DGS_HIP_TRY(h, e2);
  long long total = 0;
  std::memcpy(&total, down, sizeof(total));
  *n_pairs = total;
  s.counts8[3] = total;
  const long long n_out = std::min<long long>(total, cap);
  if (n_out > 0) std::memcpy(pairs, down + sizeof(long long), (size_t)n_out * sizeof(int2));
  if (total > capacity) {
    h->err = "building overlap: more overlapped pairs than capacity; the first `capacity` are written, *n_pairs is the full count";
    return DGS_ERR_CAPACITY;
  }
  return DGS_OK;
}

int dgs_line_align_overlapped_batch(dgs_handle* h, const dgs_line_align_params* params, int64_t n_items, const dgs_line_feature* src_lines,
                                    const int64_t* src_offsets, const dgs_line_feature* trg_lines, const int64_t* trg_offsets,
                                    const double* centers_source, const double* centers_target, dgs_line_feature* aligned_lines,
                                    dgs_line_overlap_alignment* alignments) {
  if (const char* why = la::params_guard(params)) {                    // before anything touches a device
    if (h) h->err = why;
    return DGS_ERR_INVALID_ARGUMENT;
  }
  if (!h || n_items < 0 || (n_items > 0 && (!alignments || !src_offsets || !trg_offsets || !centers_source || !centers_target)))
    return DGS_ERR_INVALID_ARGUMENT;
  h->err.clear();
  BoScratch& s = h->bo;
  for (int k = 4; k < 8; k++) s.counts8[k] = 0;
  s.off.assign(1, 0);
  if (n_items == 0) return DGS_OK;
  const char* why = nullptr;
  if (n_items > DGS_LA_MAX_ITEMS) why = "line align: more than DGS_LA_MAX_ITEMS items";
  else if (src_offsets[0] != 0 || trg_offsets[0] != 0) why = "line align: the first offset is not 0";
  for (int64_t b = 0; b < n_items && !why; b++) {
    const int64_t ls = src_offsets[b + 1] - src_offsets[b], lt = trg_offsets[b + 1] - trg_offsets[b];
    if (ls < 0 || lt < 0) why = "line align: offsets are not ascending";
    else if (ls > DGS_LA_MAX_LINES_SOURCE) why = "line align: more than DGS_LA_MAX_LINES_SOURCE source lines in an item";
    else if (lt > DGS_LA_MAX_LINES_TARGET) why = "line align: more than DGS_LA_MAX_LINES_TARGET target lines in an item";
  }
  const int64_t n_src = why ? 0 : src_offsets[n_items], n_trg = why ? 0 : trg_offsets[n_items];
  if (!why && ((n_src > 0 && !src_lines) || (n_trg > 0 && !trg_lines))) why = "line align: a line array is NULL";
  if (!why && (!la::all_finite(src_lines, n_src) || !la::all_finite(trg_lines, n_trg) || !bo_finite3(centers_source, n_items) ||
               !bo_finite3(centers_target, n_items)))
    why = "line align: a coordinate is not finite";
  if (why) {
    h->err = why;
    return DGS_ERR_INVALID_ARGUMENT;
  }

  // ---- the host's share: edges, offsets, the workgroup table
  const std::vector<la::Line> src = la::lines_of(src_lines, n_src), trg = la::lines_of(trg_lines, n_trg);
  const auto part = [](const std::vector<la::Line>& v, int first, int n) { return std::vector<la::Line>(v.begin() + first, v.begin() + first + n); };
  std::vector<BoItem> items((size_t)n_items);
  std::vector<la::Edge> es, et;
  std::vector<int2> wg;
  long long H = 0;
  s.off.clear();
  for (int64_t b = 0; b < n_items; b++) {
    BoItem& it = items[(size_t)b];
    it.Ls = (int)(src_offsets[b + 1] - src_offsets[b]);
    it.Lt = (int)(trg_offsets[b + 1] - trg_offsets[b]);
    it.src_off = (int)src_offsets[b];
    it.trg_off = (int)trg_offsets[b];
    it.es_off = (int)es.size();
    it.et_off = (int)et.size();
    la::edge_extraction(part(src, it.src_off, it.Ls), es);
    la::edge_extraction(part(trg, it.trg_off, it.Lt), et);
    it.Es = (int)es.size() - it.es_off;
    it.Et = (int)et.size() - it.et_off;
    it.h_off = H;
    for (int a = 0; a < 2; a++) { it.cs[a] = centers_source[3 * b + a]; it.ct[a] = centers_target[3 * b + a]; }
    const long long hi = (long long)it.Es * it.Et + (long long)it.Ls * it.Lt;
    s.off.push_back(H);
    for (long long u = 0; u < hi; u += kBoUnits) wg.push_back(make_int2((int)b, (int)u));
    H += hi;
    if (H > DGS_LA_MAX_HYPOTHESES) {
      s.off.assign(1, 0);
      h->err = "line align: more than DGS_LA_MAX_HYPOTHESES hypotheses in the batch (edge pairs and line pairs, all items)";
      return DGS_ERR_INVALID_ARGUMENT;
    }
  }
  s.off.push_back(H);

  // ---- one upload
  const size_t b_items = bo_align8(items.size() * sizeof(BoItem)), b_wg = bo_align8(wg.size() * sizeof(int2));
  const size_t n_srcd = (size_t)n_src * 6, n_trgd = (size_t)n_trg * 6, n_es = es.size() * 9, n_et = et.size() * 9;
  const size_t b_in = b_items + b_wg + (n_srcd + n_trgd + n_es + n_et) * sizeof(double);
  const size_t b_rec = (size_t)n_items * sizeof(BoRecord), b_out = b_rec + n_srcd * sizeof(double);
  DGS_HIP_TRY(h, hipSetDevice(h->device));
  DGS_HIP_TRY(h, s.ain.reserve(b_in));
  DGS_HIP_TRY(h, s.hyps.reserve((size_t)std::max<long long>(H, 1)));
  DGS_HIP_TRY(h, s.aout.reserve(b_out));
  if (ensure_pinned(h, b_in + b_out) != DGS_OK) return DGS_ERR_HIP;
  char* up = static_cast<char*>(h->pinned);
  char* down = up + b_in;                                              // b_in is a multiple of 8
  std::memcpy(up, items.data(), items.size() * sizeof(BoItem));
  if (!wg.empty()) std::memcpy(up + b_items, wg.data(), wg.size() * sizeof(int2));
  double* o = reinterpret_cast<double*>(up + b_items + b_wg);
  o = la::pack_lines(src, o);
  o = la::pack_lines(trg, o);
  o = la::pack_edges(es, o);
  la::pack_edges(et, o);
  DGS_HIP_TRY(h, hipMemcpyAsync(s.ain.ptr, up, b_in, hipMemcpyHostToDevice, h->stream));
  const BoItem* d_items = reinterpret_cast<const BoItem*>(s.ain.ptr);
  const int2* d_wg = reinterpret_cast<const int2*>(s.ain.ptr + b_items);
  const double* d_src = reinterpret_cast<const double*>(s.ain.ptr + b_items + b_wg);
  const double* d_trg = d_src + n_srcd;
  const double* d_es = d_trg + n_trgd;
  const double* d_et = d_es + n_es;
  BoRecord* d_rec = reinterpret_cast<BoRecord*>(s.aout.ptr);
  double* d_aligned = reinterpret_cast<double*>(s.aout.ptr + b_rec);

  // ---- three launches whatever the batch holds (a grid is at least one workgroup; the kernels check their counts)
#define BO_LAUNCH(...)                  \
  do {                                  \
    hipLaunchKernelGGL(__VA_ARGS__);    \
    s.counts8[4]++;                     \
  } while (0)
  const dim3 blk(kBlock);
  BO_LAUNCH(bo_hypothesis_kernel, bo_blocks(H, kBlock), blk, 0, h->stream, d_items, (int)n_items, H, d_src, d_trg, d_es, d_et, std::cos(bo::kMaxAngle),
            params->angle_gate_float_chain ? 1 : 0, s.hyps.ptr);
  BO_LAUNCH(bo_overlap_kernel, dim3((unsigned)std::max<size_t>(wg.size(), 1)), blk, 0, h->stream, d_items, d_wg, (int)wg.size(), d_src, d_trg, s.hyps.ptr);
  BO_LAUNCH(bo_argmin_kernel, dim3((unsigned)n_items), blk, 0, h->stream, d_items, (int)n_items, d_src, s.hyps.ptr, d_rec, d_aligned);
#undef BO_LAUNCH
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipMemcpyAsync(down, s.aout.ptr, b_out, hipMemcpyDeviceToHost, h->stream);
  const hipError_t e2 = hipStreamSynchronize(h->stream);               // the one host wait, also on the error path
  s.counts8[5] = 1;
  DGS_HIP_TRY(h, e);
  DGS_HIP_TRY(h, e2);

  const BoRecord* rec = reinterpret_cast<const BoRecord*>(down);
  const double* al = reinterpret_cast<const double*>(down + b_rec);
  for (int64_t b = 0; b < n_items; b++) {
    const BoItem& it = items[(size_t)b];
    const BoRecord& r = rec[b];
    dgs_line_overlap_alignment& out = alignments[b];
    std::memset(&out, 0, sizeof(out));
    la::matrix(r.t, out.transformation);
    out.translation_norm = r.tn;
    out.winner = r.winner;
    out.n_hypotheses_edge = (int64_t)it.Es * it.Et;
    out.n_hypotheses_line = (int64_t)it.Ls * it.Lt;
    out.n_angle_passed = r.n_angle_passed;
    out.n_not_overlapped = r.n_not_overlapped;
    out.n_edges_source = it.Es;
    out.n_edges_target = it.Et;
    out.is_identity = la::is_identity(r.t) ? 1 : 0;
    out.status = r.winner >= 0 ? DGS_LA_ALIGNED
                 : out.n_hypotheses_edge + out.n_hypotheses_line == 0 ? DGS_LA_NO_HYPOTHESES
                 : r.n_not_overlapped == 0 ? DGS_LA_ALL_GATED
                                           : DGS_LA_NONE_BETTER;
  }
  if (aligned_lines)
    for (int64_t i = 0; i < n_src; i++) {
      aligned_lines[i] = src_lines[i];   // transform_lines copies the line and replaces its two points
      std::memcpy(aligned_lines[i].point_a, al + 6 * i, 24);
      std::memcpy(aligned_lines[i].point_b, al + 6 * i + 3, 24);
    }
  s.counts8[6] = n_items;
  s.counts8[7] = H;
  return DGS_OK;
}

int dgs_line_align_overlapped(dgs_handle* h, const dgs_line_align_params* params, const dgs_line_feature* src_lines, int64_t n_src,
                              const dgs_line_feature* trg_lines, int64_t n_trg, const double* center_source, const double* center_target,
                              dgs_line_feature* aligned_lines, dgs_line_overlap_alignment* alignment) {
  const int64_t so[2] = {0, n_src}, to[2] = {0, n_trg};
  return dgs_line_align_overlapped_batch(h, params, 1, src_lines, so, trg_lines, to, center_source, center_target, aligned_lines, alignment);
}

int dgs_line_align_overlapped_get_hypotheses(dgs_handle* h, int64_t item, int64_t first, int64_t count, dgs_line_align_overlapped_hypothesis* records) {
  if (!h || first < 0 || count < 0) return DGS_ERR_INVALID_ARGUMENT;
  BoScratch& s = h->bo;
  if (!records || count == 0) return DGS_OK;
  if (item < 0 || item + 1 >= (int64_t)s.off.size() || first + count > s.off[(size_t)item + 1] - s.off[(size_t)item]) {
    h->err = "line align: the range lies beyond the last call's hypotheses";
    return DGS_ERR_INVALID_ARGUMENT;
  }
  const size_t n = (size_t)count;
  std::vector<BoHyp> hy(n);
  DGS_HIP_TRY(h, hipSetDevice(h->device));
  DGS_HIP_TRY(h, hipMemcpyAsync(hy.data(), s.hyps.ptr + (s.off[(size_t)item] + first), n * sizeof(BoHyp), hipMemcpyDeviceToHost, h->stream));
  DGS_HIP_TRY(h, hipStreamSynchronize(h->stream));
  for (size_t i = 0; i < n; i++) {
    dgs_line_align_overlapped_hypothesis& r = records[i];
    r.gate = hy[i].gate;
    r.reserved = 0;
    r.rotation[0] = hy[i].t.r00; r.rotation[1] = hy[i].t.r01; r.rotation[2] = hy[i].t.r10; r.rotation[3] = hy[i].t.r11;
    r.translation[0] = hy[i].t.tx; r.translation[1] = hy[i].t.ty; r.translation[2] = hy[i].t.tz;
    r.translation_norm = hy[i].tn;
  }
  return DGS_OK;
}

int dgs_building_overlap_get_counts(dgs_handle* h, int64_t* counts8) {
  if (!h || !counts8) return DGS_ERR_INVALID_ARGUMENT;
  for (int k = 0; k < 8; k++) counts8[k] = h->bo.counts8[k];
  return DGS_OK;
}

}  // extern "C"
