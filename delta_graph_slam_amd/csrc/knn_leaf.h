// The wave-per-leaf exact k-NN search as a device body, written once: gicp_knn_leaf_kernel / gicp_knn_leaf_wide_kernel (knn_lists.hip) run
// it over one cloud, cov_knn_batch_kernel / cov_knn_batch_wide_kernel (cov_batch.hip) over every cloud of a chunk.  A workgroup hands the
// body its index among the workgroups of ITS cloud; everything else the body reads is the cloud's own.
#pragma once
#include <cmath>
#include <cstdint>

#include "handle.h"
#include "nn_group.h"

namespace dgs {

// a group's list -> the table: slot s * 8 + sub of the 8-lane group -> nbr[pos * (SLOTS * 8) + slot], -1 = nothing found
template <int SLOTS>
__device__ __forceinline__ void knn_write_list(const KnnListT<SLOTS>& L, const int pos, const int sub, const int k, int* __restrict__ nbr) {
#pragma unroll
  for (int s = 0; s < SLOTS; s++) {
    const int slot = s * 8 + sub;
    if (slot < k) nbr[(size_t)pos * (SLOTS * 8) + slot] = (L.dist(s) < INFINITY) ? L.index(s) : -1;
  }
}

// ---- k-NN sets, one WAVE per leaf of the index (8 Hilbert-adjacent query points), in three cooperative steps:
//  (a) a window of 8 leaves around the query leaf (64 points, one per lane) gives every query an upper bound T_j on its k-th
//      squared distance: the k-th smallest of its distances to the window (bit-descent over ballot counts);
//  (b) ONE walk of the tree for the 8 queries together: a frontier of nodes in LDS, 8 nodes x 8 child boxes per pass, a child
//      qualifies when it is within T_j of ANY query j (the very test of the per-query walk, so no neighbour can be missed), the
//      qualifying leaves end up in an LDS list (<= kLeafCap; typical 15-20);
//  (c) per query: distances to all candidate points (lane = point), the k smallest (distance, index) keys selected by the same
//      bit-descent, ties at the k-th distance broken towards the lower index, and written to nbr.
// The sets are the same as those of the per-query walk (knn_query_group): same float distance, same order relation.  Per wave this
// is ~10 k instructions instead of ~50 k (there, every one of ~40 insertions per query costs ~65 instructions of cross-lane
// minimum / replace-the-largest).
// Sparse corners of a cloud (0.7 % of the leaves of a 64-beam scan) have window bounds so loose that the lists overflow.  Those
// waves retry with the bounds scaled down (s T_j): whatever s, a query whose candidates hold >= k points within s T_j has its
// exact answer among them (every point within s T_j sits in a gathered leaf); s is bisected between "overflows" and "too few
// points" until every query of the leaf is answered.  Only what still fails after kKnnRetries -- or is irregular: fewer than 8
// leaves, a non-finite point in the window, fewer than k finite window points -- takes the per-query walk.
#ifndef DGS_KNN_LEAF_CAP
#define DGS_KNN_LEAF_CAP 64
#endif
constexpr int kLeafCap = DGS_KNN_LEAF_CAP, kFrontCap = 64, kLeafChunks = kLeafCap / 8, kKnnRetries = 12;
constexpr unsigned kInfBits = 0x7F800000u;

__device__ __forceinline__ float readlane_f32(float v, int l) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l)); }
__device__ __forceinline__ int lanes_below(unsigned long long m) { return (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u)); }

// k-th smallest (1-based) of the wave's values d[0 .. chunks) (bit patterns of non-negative floats, kInfBits = none), built from
// the top bit down: V keeps the largest prefix with fewer than k values below it.  If some prefix has EXACTLY k values below it
// the descent stops there and returns it with lt_only = true: then { d < V } is the answer set and ties cannot matter.
// `upper`: bit pattern of a value known to be >= the k-th smallest (0 = nothing known).  The descent is scalar work -- a compare,
// a population count and a branch per chunk and bit, ~18 rounds per call on scan data, two thirds of this kernel's instructions -- and
// its first eight rounds only find the binade of the answer: with a bound, the binades at and just below the bound's are tried
// directly (one round each) and the descent starts at the mantissa.
template <int NC>
__device__ __forceinline__ int count_below(const unsigned (&d)[NC], const int chunks, const unsigned trial) {
  int cnt = 0;
#pragma unroll
  for (int c = 0; c < NC; c++)
    if (c < chunks) cnt += __popcll(__ballot(d[c] < trial));
  return cnt;
}
template <int NC>
__device__ __forceinline__ unsigned kth_smallest_bits(const unsigned (&d)[NC], const int chunks, const int k, bool& lt_only, const unsigned upper = 0u) {
  unsigned V = 0;
  int bit = 30;
  lt_only = false;
  if (upper >= (4u << 23) && upper < 0x7F800000u) {
    const unsigned e = upper >> 23;   // the k-th smallest is below (e + 1) << 23
#pragma unroll 1
    for (unsigned t = 0; t < 3u; t++) {
      const unsigned base = (e - t) << 23;
      const int cnt = count_below<NC>(d, chunks, base);
      if (cnt == k) { lt_only = true; return base; }
      if (cnt < k) { V = base; bit = 22; break; }   // fewer than k below this binade, at least k below the next: the answer has this exponent
    }
  }
#pragma unroll 1
  for (; bit >= 0; bit--) {
    const unsigned trial = V | (1u << bit);
    const int cnt = count_below<NC>(d, chunks, trial);
    if (cnt == k) { lt_only = true; return trial; }
    if (cnt < k) V = trial;
  }
  return V;
}

// An UPPER BOUND of the k-th smallest of the wave's values: the descent above cut after the top `rounds` bits, the undecided low bits
// set (so that at least k values are <= the result).  For the window bound of step (a), which only prunes.
__device__ __forceinline__ unsigned kth_smallest_upper_bound(const unsigned d, const int k, const int rounds) {
  unsigned V = 0;
  int bit = 30;
#pragma unroll 1
  for (; bit > 30 - rounds; bit--) {
    const unsigned trial = V | (1u << bit);
    const int cnt = __popcll(__ballot(d < trial));
    if (cnt == k) return trial;        // exactly k values below trial: the k-th smallest is below it
    if (cnt < k) V = trial;
  }
  return V | ((2u << bit) - 1u);        // the k-th smallest has prefix V: it is at most V with every lower bit set
}

// Step (a) for NQ queries j0 .. j0 + NQ - 1 of the leaf at once: per query an UPPER BOUND of the k-th smallest distance to the 64 window
// points (the top 14 bits of the bit descent, the undecided low bits set: within 1.6 %, and it only prunes), written to lane j of Tl.
// Returns false when a query has fewer than k finite window points (the caller takes the careful path).
// FULL: k may be the whole window (the wide kernel at k = 64).  Then "exactly k values below trial" holds at the first bit tried and says
// nothing -- no (k + 1)-th value stands above it -- so the descent goes on to the bits of the largest window distance itself.
template <int NQ, bool FULL>
__device__ __forceinline__ bool knn_window_bounds(const float4 wp, const bool wfinite, const int w0, const int j0, const int k, float& Tl) {
  const int lane = threadIdx.x & 63;
  unsigned d[NQ], V[NQ];
  bool done[NQ];
  bool ok = true;
#pragma unroll
  for (int t = 0; t < NQ; t++) {
    const float qx = readlane_f32(wp.x, w0 + j0 + t), qy = readlane_f32(wp.y, w0 + j0 + t), qz = readlane_f32(wp.z, w0 + j0 + t);
    const float dp = sqdist_rn(qx, qy, qz, wp.x, wp.y, wp.z);
    d[t] = (wfinite && dp < INFINITY) ? __float_as_uint(dp) : kInfBits;
    ok = ok && (__popcll(__ballot(d[t] < kInfBits)) >= k);
    V[t] = 0;
    done[t] = false;
  }
  if (!ok) return false;
  constexpr int kRounds = 14;
#pragma unroll 1
  for (int bit = 30; bit > 30 - kRounds; bit--) {
#pragma unroll
    for (int t = 0; t < NQ; t++) {
      const unsigned trial = V[t] | (1u << bit);
      const int cnt = __popcll(__ballot(d[t] < trial));
      if (!done[t]) {
        if (cnt == k && (!FULL || k < kWave)) { V[t] = trial; done[t] = true; }   // exactly k values below trial: the k-th smallest is below it
        else if (cnt < k) V[t] = trial;
      }
    }
  }
#pragma unroll
  for (int t = 0; t < NQ; t++) {
    const unsigned bound = done[t] ? V[t] : (V[t] | ((2u << (30 - kRounds)) - 1u));   // prefix V: at most V with every lower bit set
    if (lane == j0 + t) Tl = __uint_as_float(bound);
  }
  return true;
}

// step (b): the leaves within Tl[j] * scale of any query j of `open`; returns their number, or -1 when a list overflowed.
// Lane layout: 8 frontier nodes x 8 children per pass, the queries in a loop inside.  Measured and dropped (round 3, `profiles/r03`):
// (query x child) lanes with one node per pass (no query loop, but 4-8x the passes: 0.174-0.190 against 0.168-0.173 ms per 65,536-point
// cloud), and one test per node against the box of the open queries above the leaves (an eighth of the tests, but the sparse rings of a
// 16-beam scan then overflow the frontier and walk again: 0.081 -> 0.160 ms per 26,668-point cloud).
__device__ __forceinline__ int knn_gather_leaves(const BvhView& b, const float4 wp, const int w0, const int n_q, const unsigned open, const float Tl,
                                                 const float scale, int (*front)[kFrontCap], int* leaves) {
  const int lane = threadIdx.x & 63;
  int cur = 0, count = 1, level0 = 0;
  if (b.depth >= 3) {
    // The 64 nodes two levels below the root (heap ids 9..72, their boxes at 8..71) in ONE pass, a node per lane: it replaces the
    // three dependent passes root -> 8 -> 64 every wave would otherwise repeat.  Empty nodes carry inverted boxes and never hit.
    const float4 lo = load16_at(b.box_lo, 8u + lane), hi = load16_at(b.box_hi, 8u + lane);
    bool hit = false;
    // over the set bits of `open` (with 2 or 4 waves per leaf a wave has 4 or 2 of the 8 queries: a loop over all 8 spent most of its
    // scalar instructions skipping the others)
#pragma unroll 1
    for (unsigned rest = open; rest != 0u; rest &= rest - 1u) {
      const int j = __builtin_ctz(rest);
      const float qx = readlane_f32(wp.x, w0 + j), qy = readlane_f32(wp.y, w0 + j), qz = readlane_f32(wp.z, w0 + j);
      hit = hit || (aabb_sqdist_rn(lo, hi, qx, qy, qz) <= readlane_f32(Tl, j) * scale);
    }
    const unsigned long long m = __ballot(hit);
    if (hit) front[0][lanes_below(m)] = 9 + lane;
    count = __popcll(m);
    level0 = 2;
  } else if (lane == 0) {
    front[0][0] = 0;
  }
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_s_waitcnt(0xc07f);
  for (int level = level0; level < b.depth; level++) {
    const bool last = level == b.depth - 1;
    int next = 0;
    for (int base = 0; base < count; base += 8) {
      const int slot = base + (lane >> 3);
      const bool valid = slot < count;
      const int node = valid ? front[cur][slot] : 0;
      const unsigned ofs = (unsigned)node * kFan + (lane & 7);
      const float4 lo = load16_at(b.box_lo, ofs), hi = load16_at(b.box_hi, ofs);
      bool hit = false;
#pragma unroll 1
      for (unsigned rest = open; rest != 0u; rest &= rest - 1u) {
        const int j = __builtin_ctz(rest);
        const float qx = readlane_f32(wp.x, w0 + j), qy = readlane_f32(wp.y, w0 + j), qz = readlane_f32(wp.z, w0 + j);
        hit = hit || (aabb_sqdist_rn(lo, hi, qx, qy, qz) <= readlane_f32(Tl, j) * scale);
      }
      hit = hit && valid;
      const unsigned long long m = __ballot(hit);
      const int pos = next + lanes_below(m);
      const int child = node * kFan + 1 + (lane & 7);
      if (hit) {
        if (last) { if (pos < kLeafCap) leaves[pos] = child - b.first_leaf; }
        else if (pos < kFrontCap) front[cur ^ 1][pos] = child;
      }
      next += __popcll(m);
    }
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_s_waitcnt(0xc07f);
    if (next > (last ? kLeafCap : kFrontCap)) return -1;
    cur ^= 1;
    count = next;
  }
  return count;
}


// step (c) for a candidate list of exactly NCH chunks (NCH * 8 leaves, the last chunk possibly partial): per open query the k-th smallest
// candidate distance, the selection (ties at the k-th distance to the lower index) and its neighbour list; answered queries leave `open`
template <int NCH, int STRIDE>
__device__ __forceinline__ void knn_select(const BvhView& b, const float4 wp, const int w0, const int n_q, const int n_cand, const int k, const float Tl,
                                           const float scale, const int* leaves, int* __restrict__ nbr, const int l, unsigned& open) {
  const int lane = threadIdx.x & 63;
  float4 cp[NCH];
#pragma unroll
  for (int c = 0; c < NCH; c++) {
    cp[c] = make_float4(NAN, NAN, NAN, __uint_as_float(0xFFFFFFFFu));
    {
      const int li = c * 8 + (lane >> 3);
      if (li < n_cand) cp[c] = load16_at(b.sorted, (unsigned)(leaves[li] * kLeaf + (lane & 7)));
    }
  }
#pragma unroll 1
  for (unsigned rest = open; rest != 0u; rest &= rest - 1u) {
    const int j = __builtin_ctz(rest);
    const float qx = readlane_f32(wp.x, w0 + j), qy = readlane_f32(wp.y, w0 + j), qz = readlane_f32(wp.z, w0 + j);
    const unsigned Ttry = __float_as_uint(readlane_f32(Tl, j) * scale);
    unsigned d[NCH];
    int within = 0;
#pragma unroll
    for (int c = 0; c < NCH; c++) {
      d[c] = kInfBits;
      {
        const float dp = sqdist_rn(qx, qy, qz, cp[c].x, cp[c].y, cp[c].z);   // NaN for padding / empty lanes
        if (dp < INFINITY && (int)__float_as_uint(cp[c].w) >= 0) d[c] = __float_as_uint(dp);
        within += __popcll(__ballot(d[c] <= Ttry));
      }
    }
    if (within < k) continue;   // the scaled bound was too small for this query: nothing can be concluded
    bool lt = true;
    // exactly k candidates within the bound (it sits at most 1.6 % above the k-th distance of the window): they are the answer, no descent
    const unsigned V = (within == k) ? Ttry + 1u : kth_smallest_bits<NCH>(d, NCH, k, lt, Ttry);   // at least k are within Ttry: the answer is <= Ttry
    // selection: everything below V; if V IS the k-th smallest, the k - (count below) lowest indices among the values equal to V
    bool sel[NCH];
    int below = 0, equal = 0;
#pragma unroll
    for (int c = 0; c < NCH; c++) {
      sel[c] = d[c] < V;
      { below += __popcll(__ballot(d[c] < V)); equal += __popcll(__ballot(d[c] == V)); }
    }
    if (!lt) {
      const int need = k - below;
      if (equal == need) {
#pragma unroll
        for (int c = 0; c < NCH; c++) sel[c] = d[c] <= V;
      } else {
        // more values at the k-th distance than places left: lowest index first (rare: duplicate or symmetric points)
        for (int t = 0; t < need; t++) {
          int mine = 0x7FFFFFFF;
#pragma unroll
          for (int c = 0; c < NCH; c++)
            if (d[c] == V && !sel[c]) mine = min(mine, (int)__float_as_uint(cp[c].w));
          int best = mine;
#pragma unroll
          for (int o = 32; o > 0; o >>= 1) best = min(best, __shfl_xor(best, o));
#pragma unroll
          for (int c = 0; c < NCH; c++)
            if (d[c] == V && (int)__float_as_uint(cp[c].w) == best) sel[c] = true;
        }
      }
    }
    int* __restrict__ out = nbr + (size_t)(l * kLeaf + j) * STRIDE;
    int written = 0;
#pragma unroll
    for (int c = 0; c < NCH; c++) {
      {
        const unsigned long long m = __ballot(sel[c]);
        if (sel[c]) out[written + lanes_below(m)] = (int)__float_as_uint(cp[c].w);
        written += __popcll(m);
      }
    }
    open &= ~(1u << j);
  }
}

template <int N, int STRIDE>
__device__ __forceinline__ void knn_select_dispatch(const int chunks, const BvhView& b, const float4 wp, const int w0, const int n_q, const int n_cand, const int k,
                                                    const float Tl, const float scale, const int* leaves, int* __restrict__ nbr, const int l, unsigned& open) {
  if (chunks <= N || N == kLeafChunks) knn_select<N, STRIDE>(b, wp, w0, n_q, n_cand, k, Tl, scale, leaves, nbr, l, open);
  else if constexpr (N < kLeafChunks) knn_select_dispatch<N + 1, STRIDE>(chunks, b, wp, w0, n_q, n_cand, k, Tl, scale, leaves, nbr, l, open);
}

// `parts` (1, 2, 4 or 8) waves share a leaf, each answering 8 / parts of its queries: a small cloud has too few leaves to fill the
// chip, and a wave's 8 selections are one dependent chain -- shorter chains on more waves, at the price of one walk per part.
// -DDGS_KNN_WAVES: waves per SIMD the compiler must leave room for.  4 = what the kernel's 109 registers give anyway; 5 / 6 / 7 / 8 (with
// -DDGS_KNN_LEAF_CAP = 64 / 48 / 40 / 32) were measured and are no faster, spills or not: the kernel is bound by the scalar unit.
#ifndef DGS_KNN_WAVES
#define DGS_KNN_WAVES 4
#endif
// blk: the workgroup's index among the workgroups of this cloud (blockIdx.x for a launch over one cloud).
template <int SLOTS>
__device__ __forceinline__ void gicp_knn_leaf_body(const BvhView& b, const int n, const int k, const int parts, int* __restrict__ nbr, int* __restrict__ stats,
                                                   const int blk) {
  __shared__ int s_front[kBlock / kWave][2][kFrontCap];
  __shared__ int s_leaves[kBlock / kWave][kLeafCap];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int n_leaves = (n + kLeaf - 1) / kLeaf;
  const int wid = blk * (kBlock / kWave) + wv;
  const int l = wid / parts, part = wid % parts;      // this wave's query leaf and its share of the queries (wave-uniform)
  if (l >= n_leaves) return;
  bool fast = n_leaves >= 8;
  // ---- (a) window of 8 leaves, one point per lane; the queries are lanes w0 + j
  const int start = fast ? min(max(l - 3, 0), n_leaves - 8) : 0;
  const int w0 = fast ? (l - start) * 8 : 0;
  float4 wp = make_float4(NAN, NAN, NAN, __uint_as_float(0xFFFFFFFFu));
  if (fast) wp = load16_at(b.sorted, (unsigned)(start * 8 + lane));
  const bool wreal = fast && (start * 8 + lane) < n;
  const bool wfinite = wreal && (wp.x - wp.x == 0.f) && (wp.y - wp.y == 0.f) && (wp.z - wp.z == 0.f);
  if (__ballot(wreal && !wfinite) != 0ull) fast = false;   // a non-finite point nearby: the careful path
  const int n_q = min(kLeaf, n - l * kLeaf);                // queries of this leaf (the last leaf may be partial)
  const int per = kLeaf / parts, j_lo = part * per, j_hi = min(n_q, j_lo + per);
  if (j_lo >= j_hi) return;
#ifdef DGS_KNN_STATS
  const unsigned long long ts0 = wall_clock64();
  unsigned long long acc_b = 0, acc_c = 0;
#endif
  float Tl = 0.f;   // lane j holds T_j
  if (fast) {
    // the bounds of this wave's queries, their descents interleaved (one descent is a chain of dependent ballot -> count -> branch
    // rounds; 2 / 4 / 8 of them side by side hide each other's latency)
    switch (j_hi - j_lo) {
      case 8: fast = knn_window_bounds<8, (SLOTS > kKnnSlots)>(wp, wfinite, w0, j_lo, k, Tl); break;
      case 4: fast = knn_window_bounds<4, (SLOTS > kKnnSlots)>(wp, wfinite, w0, j_lo, k, Tl); break;
      case 2: fast = knn_window_bounds<2, (SLOTS > kKnnSlots)>(wp, wfinite, w0, j_lo, k, Tl); break;
      default:
        for (int j = j_lo; j < j_hi && fast; j++) fast = knn_window_bounds<1, (SLOTS > kKnnSlots)>(wp, wfinite, w0, j, k, Tl);
        break;
    }
  }
#ifdef DGS_KNN_STATS
  const unsigned long long ts1 = wall_clock64();
#endif
  unsigned open = ((1u << j_hi) - 1u) & ~((1u << j_lo) - 1u);
  int iters = 0;
  if (fast) {
    float scale = 1.f, s_small = 0.f, s_over = 0.f;   // s_small: answered nobody new; s_over: overflowed (0 = not seen yet)
    for (; open != 0u && iters < kKnnRetries; iters++) {
#ifdef DGS_KNN_STATS
      const unsigned long long tb0 = wall_clock64();
#endif
      const int n_cand = knn_gather_leaves(b, wp, w0, n_q, open, Tl, scale, s_front[wv], s_leaves[wv]);
#ifdef DGS_KNN_STATS
      const unsigned long long tb1 = wall_clock64();
      acc_b += tb1 - tb0;
#endif
      if (n_cand < 0) {
        s_over = scale;
        scale = (s_small > 0.f) ? sqrtf(s_small * s_over) : scale * 0.0625f;
        continue;
      }
      // ---- (c) candidates: chunk c = leaves c * 8 .. c * 8 + 7 of the list, lane -> (leaf lane / 8, point lane % 8).  The chunk count
      // is a template argument: with it as a run-time bound every one of the dozen per-chunk loops below carried a scalar compare and a
      // branch per possible chunk and round -- the kernel was bound by the CU's one scalar unit (2,600 scalar against 1,360 vector
      // instructions per wave, `profiles/r03/knn_*`), not by anything it computes.
      const int chunks = (n_cand + 7) >> 3;
      const unsigned was_open = open;
      knn_select_dispatch<1, SLOTS * 8>(chunks, b, wp, w0, n_q, n_cand, k, Tl, scale, s_leaves[wv], nbr, l, open);
#ifdef DGS_KNN_STATS
      acc_c += wall_clock64() - tb1;
#endif
      if (open != 0u) {
        if (open != was_open) s_over = 0.f;   // fewer queries now: what overflowed before may fit
        s_small = scale;
        scale = (s_over > 0.f) ? sqrtf(s_small * s_over) : fminf(1.f, scale * 4.f);
      }
    }
  }
#ifdef DGS_KNN_STATS
  if (lane == 0) {
    atomicAdd(&stats[0], 1); atomicAdd(&stats[1], (fast && open == 0u) ? 1 : 0); atomicAdd(&stats[2], iters); atomicAdd(&stats[3], iters > 1 ? 1 : 0);
    atomicAdd(&stats[4], (int)(ts1 - ts0)); atomicAdd(&stats[5], (int)acc_b); atomicAdd(&stats[6], (int)acc_c); atomicAdd(&stats[7], (int)(wall_clock64() - ts0));
  }
#endif
  if (fast && open == 0u) return;
  // ---- the careful path: the per-query walk, 8 lanes per query
  {
    const int sub = lane & 7, jq = lane >> 3, pos = l * kLeaf + jq;
    const bool mine = jq >= j_lo && jq < j_hi;
    const float4 q = (mine && pos < n) ? b.sorted[pos] : make_float4(0.f, 0.f, 0.f, 0.f);
    const int i = (mine && pos < n) ? (int)__float_as_uint(q.w) : -1;
    const bool alive = mine && pos < n && i >= 0 && i < n;
    KnnListT<SLOTS> L;
    knn_query_group(b, q.x, q.y, q.z, alive, k, L);
    if (alive) knn_write_list(L, pos, sub, k, nbr);
  }
}

}  // namespace dgs
