// MapCloudGenerator::generate (src/hdl_graph_slam/map_cloud_generator.cpp:13-50): every keyframe cloud transformed by
// its pose, concatenated, put through a pcl::octree::OctreePointCloud of `resolution`, and replaced by the centres of the occupied
// voxels in the octree's depth-first order.
//
// MI355X design
//   * The keyframe clouds are read in place through a table of pointers, sizes and float poses (McFrame); work is dealt in chunks of
//     kMcChunk points of one keyframe (McChunk).  With resolution > 0 the concatenation is never built.
//   * The octree's origin depends on the order of the points (adoptBoundingBoxToPoint grows the box towards each point that leaves it).
//     A bounds pass gives one transformed box per chunk; the host replays the growth over the chunk boxes in order and launches a
//     find-first kernel (wave ballot + vector atomicMin) only on a chunk whose box leaves the current octree box: a few tens of
//     short waits per map, at most one growth per depth level.
//   * The replay leaves a table of at most 23 epochs (runs of points inserted under one box).  A point's key is made with the box of
//     its own epoch and moved by the growths that follow, as its leaf is in the tree; with that table the key is a pure function of
//     the point and its index.  The key pass interleaves the three axis keys into one 64-bit word (depth <= 21) and inserts it into
//     an open-addressing table in HBM (64-bit vector atomicCAS; a plain load first, so a voxel that is already there costs no
//     atomic).  The occupied slots are compacted and only the unique keys are radix-sorted: ascending interleaved key = the
//     depth-first order over child indices 0..7.  When the table overflows, or on request, every key is sorted and the unique ones
//     are taken instead.
//   * The centre pass maps each key back to (key + 0.5) * resolution + min in double.
// Semantics and the PCL 1.10 details recalled from upstream: DESIGN.md §6d.
#include <cfloat>
#include <climits>
#include <cmath>
#include <cstring>

#include <hipcub/hipcub.hpp>

#include "handle.h"

namespace dgs {

constexpr int kMcChunk = 4096;                      // points of one keyframe per chunk: 16 per lane of a workgroup
constexpr int kMcMaxDepth = 21;                     // 3 x 21 key bits in a 64-bit word
constexpr int kMcMaxGridBlocks = 4096;
constexpr long long kMcMaxSlots = 1ll << 26;        // 512 MiB of keys
constexpr int kMcProbeLimit = 4096;
constexpr unsigned long long kMcEmpty = ~0ull;      // never a key: keys have at most 63 bits

struct McFrame {
  const float4* pts;
  int n, pad;
  float m[12];   // row-major 3 x 4: pose.matrix().cast<float>()
};
static_assert(sizeof(McFrame) == 64, "McFrame must be 64 bytes");

struct McChunk {
  long long start;   // index of the chunk's first point in the concatenation
  int frame, begin, count, pad;
};

struct McBox {
  double mn[3], mx[3];
  int defined;
};

// A run of points inserted under one octree box.  A leaf sits where genOctreeKeyforPoint put it AT INSERTION (the first point of a map
// lies exactly on a voxel boundary, so the box of another epoch may round it to the other side); every later growth puts the old
// root under a child of the new one, which adds 2^depth to the key on each axis whose min moved.
struct McEpoch {
  long long start;   // index in the concatenation of the epoch's first point
  double mn[3];      // the box's min during the epoch
  unsigned off[3];   // what the later growths add to a key made in this epoch
  int pad;
};

struct McGrid {
  double mn[3], res;   // the final min: the origin of the centres
  const McEpoch* epochs;
  int n_epochs, x_msb;
};

// dst = pose * (x, y, z, 1): per row ((m0 x + m1 y) + m2 z) + m3, every step rounded; the input's pad lane is not read
__device__ __forceinline__ float4 mc_transform(const float* __restrict__ m, const float4 p) {
  return make_float4(affine_row_rn(m[0], m[1], m[2], m[3], p.x, p.y, p.z), affine_row_rn(m[4], m[5], m[6], m[7], p.x, p.y, p.z),
                     affine_row_rn(m[8], m[9], m[10], m[11], p.x, p.y, p.z), 1.f);
}

__device__ __forceinline__ bool mc_finite(const float4 q) { return isfinite(q.x) && isfinite(q.y) && isfinite(q.z); }

// bits of a 21-bit axis key to every third bit
__device__ __forceinline__ unsigned long long mc_spread(unsigned v) {
  unsigned long long x = v & 0x1fffffu;
  x = (x | x << 32) & 0x1f00000000ffffull;
  x = (x | x << 16) & 0x1f0000ff0000ffull;
  x = (x | x << 8) & 0x100f00f00f00f00full;
  x = (x | x << 4) & 0x10c30c30c30c30c3ull;
  x = (x | x << 2) & 0x1249249249249249ull;
  return x;
}
__device__ __forceinline__ unsigned mc_compact(unsigned long long x) {
  x &= 0x1249249249249249ull;
  x = (x | x >> 2) & 0x10c30c30c30c30c3ull;
  x = (x | x >> 4) & 0x100f00f00f00f00full;
  x = (x | x >> 8) & 0x1f0000ff0000ffull;
  x = (x | x >> 16) & 0x1f00000000ffffull;
  x = (x | x >> 32) & 0x1fffffull;
  return (unsigned)x;
}

// genOctreeKeyforPoint under the box of the point's epoch: (unsigned)(((double)x - min) / resolution) per axis, moved by the later
// growths, interleaved with the first axis of the child index on top
__device__ __forceinline__ unsigned long long mc_key(const McGrid& g, const McEpoch& e, const float4 q) {
  const unsigned kx = (unsigned)(((double)q.x - e.mn[0]) / g.res) + e.off[0];
  const unsigned ky = (unsigned)(((double)q.y - e.mn[1]) / g.res) + e.off[1];
  const unsigned kz = (unsigned)(((double)q.z - e.mn[2]) / g.res) + e.off[2];
  return g.x_msb ? (mc_spread(kx) << 2) | (mc_spread(ky) << 1) | mc_spread(kz) : (mc_spread(kz) << 2) | (mc_spread(ky) << 1) | mc_spread(kx);
}

// ================================================================================================ bounds pass
// per chunk: min3, max3 of the transformed finite points, their number (bit-cast int), pad
__global__ __launch_bounds__(kBlock) void mc_bounds_kernel(const McFrame* __restrict__ frames, const McChunk* __restrict__ chunks, const int n_chunks,
                                                           float* __restrict__ boxes) {
  __shared__ float s_v[kBlock / kWave][8];
  const int lane = threadIdx.x & (kWave - 1), wv = threadIdx.x / kWave;
  for (int c = blockIdx.x; c < n_chunks; c += gridDim.x) {
    const McChunk ch = chunks[c];
    const McFrame* f = frames + ch.frame;
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    int cnt = 0;
    for (int i = threadIdx.x; i < ch.count; i += kBlock) {   // ch.begin + i < f->n <= INT32_MAX
      const float4 q = mc_transform(f->m, f->pts[ch.begin + i]);
      if (mc_finite(q)) {
        lo[0] = fminf(lo[0], q.x); lo[1] = fminf(lo[1], q.y); lo[2] = fminf(lo[2], q.z);
        hi[0] = fmaxf(hi[0], q.x); hi[1] = fmaxf(hi[1], q.y); hi[2] = fmaxf(hi[2], q.z);
        cnt++;
      }
    }
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) {
#pragma unroll
      for (int a = 0; a < 3; a++) {
        lo[a] = fminf(lo[a], __shfl_xor(lo[a], o, kWave));
        hi[a] = fmaxf(hi[a], __shfl_xor(hi[a], o, kWave));
      }
      cnt += __shfl_xor(cnt, o, kWave);
    }
    if (lane == 0) {
#pragma unroll
      for (int a = 0; a < 3; a++) { s_v[wv][a] = lo[a]; s_v[wv][3 + a] = hi[a]; }
      s_v[wv][6] = __int_as_float(cnt);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      float* b = boxes + (size_t)c * 8;
      int total = 0;
#pragma unroll
      for (int w = 0; w < kBlock / kWave; w++) {
#pragma unroll
        for (int a = 0; a < 3; a++) { lo[a] = fminf(lo[a], s_v[w][a]); hi[a] = fmaxf(hi[a], s_v[w][3 + a]); }
        total += __float_as_int(s_v[w][6]);
      }
#pragma unroll
      for (int a = 0; a < 3; a++) { b[a] = lo[a]; b[3 + a] = hi[a]; }
      b[6] = __int_as_float(total);
      b[7] = 0.f;
    }
    __syncthreads();
  }
}

// ================================================================================================ growth replay: find-first
// Lowest index (within the keyframe) of a finite point of pts[begin .. begin + count) that violates `box` (x < min or x >= max on some
// axis, the float promoted to double), or of any finite point while the box is undefined: wave ballot, one vector atomicMin per wave.
__global__ __launch_bounds__(kBlock) void mc_find_first_kernel(const McFrame* __restrict__ frames, const int frame, const int begin, const int count,
                                                               const McBox box, int* __restrict__ found) {
  const McFrame* f = frames + frame;
  const int i = blockIdx.x * kBlock + threadIdx.x;
  bool v = false;
  if (i < count) {
    const float4 q = mc_transform(f->m, f->pts[begin + i]);
    if (mc_finite(q)) {
      const double x = (double)q.x, y = (double)q.y, z = (double)q.z;
      v = !box.defined || x < box.mn[0] || y < box.mn[1] || z < box.mn[2] || x >= box.mx[0] || y >= box.mx[1] || z >= box.mx[2];
    }
  }
  const unsigned long long m = __ballot(v);
  if (m != 0ull && (threadIdx.x & (kWave - 1)) == 0) atomicMin(found, begin + i + (__ffsll((long long)m) - 1));
}

// found[4..7] = {index, x, y, z of the transformed point}; found[0] is armed for the next find-first pass
__global__ void mc_fetch_kernel(const McFrame* __restrict__ frames, const int frame, int* __restrict__ found) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const int idx = found[0];
  found[4] = idx;
  if (idx != INT_MAX) {
    const McFrame* f = frames + frame;
    const float4 q = mc_transform(f->m, f->pts[idx]);
    found[5] = __float_as_int(q.x);
    found[6] = __float_as_int(q.y);
    found[7] = __float_as_int(q.z);
  }
  found[0] = INT_MAX;
}

// ================================================================================================ key pass
// Linear probing from the top bits of a multiplicative hash.  A slot only ever changes from empty to a key, so a plain load that
// shows the key is final and one that shows a stale "empty" is settled by the CAS.  cnt[1] != 0: the table overflowed.
__device__ __forceinline__ void mc_insert(unsigned long long* __restrict__ table, const unsigned long long mask, const int shift, const int probe_limit,
                                          const unsigned long long key, long long* __restrict__ cnt) {
  unsigned long long slot = (key * 0x9E3779B97F4A7C15ull) >> shift;
  for (int probes = 0; probes < probe_limit; probes++) {
    unsigned long long cur = table[slot];
    if (cur == key) return;
    if (cur == kMcEmpty) {
      cur = atomicCAS(&table[slot], kMcEmpty, key);
      if (cur == kMcEmpty || cur == key) return;
    }
    slot = (slot + 1) & mask;
  }
  cnt[1] = 1;
}

// HASH: every finite point's key into the table.  Otherwise all_keys[index in the concatenation] = key, or `sentinel` (above every
// key) for a non-finite point.
template <bool HASH>
__global__ __launch_bounds__(kBlock) void mc_key_kernel(const McFrame* __restrict__ frames, const McChunk* __restrict__ chunks, const int n_chunks,
                                                        const McGrid g, unsigned long long* __restrict__ table, const unsigned long long mask,
                                                        const int shift, const int probe_limit, long long* __restrict__ cnt,
                                                        const unsigned long long sentinel) {
  const int lane = threadIdx.x & (kWave - 1);
  for (int c = blockIdx.x; c < n_chunks; c += gridDim.x) {
    const McChunk ch = chunks[c];
    const McFrame* f = frames + ch.frame;
    int e_lo = 0, e_hi = 0;   // epochs of the chunk's first and last point: almost always the same one
    for (int k = 1; k < g.n_epochs; k++) {
      if (g.epochs[k].start <= ch.start) e_lo = k;
      if (g.epochs[k].start < ch.start + ch.count) e_hi = k;
    }
    for (int base = 0; base < ch.count; base += kBlock) {   // uniform trip count: the shuffle below runs in whole waves
      const int i = base + threadIdx.x;
      bool ok = false;
      unsigned long long key = sentinel;
      if (i < ch.count) {
        const float4 q = mc_transform(f->m, f->pts[ch.begin + i]);
        ok = mc_finite(q);
        if (ok) {
          int e = e_lo;
          for (int k = e_lo + 1; k <= e_hi; k++)
            if (g.epochs[k].start <= ch.start + i) e = k;
          key = mc_key(g, g.epochs[e], q);
        }
      }
      if (HASH) {
        // neighbours along a scan line mostly share a voxel: the lane after an equal key leaves the insert to it
        const unsigned long long prev = __shfl_up(key, 1, kWave);
        if (ok && (lane == 0 || prev != key)) mc_insert(table, mask, shift, probe_limit, key, cnt);
      } else if (i < ch.count) {
        table[ch.start + i] = key;
      }
    }
  }
}

struct McOccupied {
  __host__ __device__ bool operator()(const unsigned long long& k) const { return k != kMcEmpty; }
};

// ================================================================================================ centre pass / concatenation
// genLeafNodeCenterFromOctreeKey: (float)((key + 0.5) * resolution + min) per axis in double, product and sum rounded apart
__global__ __launch_bounds__(kBlock) void mc_centre_kernel(const unsigned long long* __restrict__ keys, const long long n, const McGrid g,
                                                           float4* __restrict__ out) {
#pragma clang fp contract(off)
  const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const unsigned long long k = keys[i];
  const unsigned a2 = mc_compact(k >> 2), a1 = mc_compact(k >> 1), a0 = mc_compact(k);
  const unsigned kx = g.x_msb ? a2 : a0, kz = g.x_msb ? a0 : a2;
  const double x = ((double)kx + 0.5) * g.res;
  const double y = ((double)a1 + 0.5) * g.res;
  const double z = ((double)kz + 0.5) * g.res;
  out[i] = make_float4((float)(x + g.mn[0]), (float)(y + g.mn[1]), (float)(z + g.mn[2]), 1.f);
}

__global__ __launch_bounds__(kBlock) void mc_concat_kernel(const McFrame* __restrict__ frames, const McChunk* __restrict__ chunks, const int n_chunks,
                                                           float4* __restrict__ out) {
  for (int c = blockIdx.x; c < n_chunks; c += gridDim.x) {
    const McChunk ch = chunks[c];
    const McFrame* f = frames + ch.frame;
    for (int i = threadIdx.x; i < ch.count; i += kBlock) out[ch.start + i] = mc_transform(f->m, f->pts[ch.begin + i]);
  }
}

// ================================================================================================ host side
namespace {

// adoptBoundingBoxToPoint / getKeyBitSize over one point; all box arithmetic in double
struct McOctree {
  double res = 0.0;
  double mn[3] = {0, 0, 0}, mx[3] = {0, 0, 0};
  int depth = 0, growths = 0;
  bool defined = false;
  const dgs_map_cloud_params* p = nullptr;
  std::vector<McEpoch> epochs;

  bool inside(const float* b) const {   // chunk box min3, max3
    for (int a = 0; a < 3; a++)
      if ((double)b[a] < mn[a] || (double)b[3 + a] >= mx[a]) return false;
    return true;
  }
  void open_epoch(long long start) {
    McEpoch e;
    e.start = start;
    for (int a = 0; a < 3; a++) { e.mn[a] = mn[a]; e.off[a] = 0; }
    e.pad = 0;
    epochs.push_back(e);
  }
  // `index`: the point's place in the concatenation
  int adopt(const float q[3], long long index) {
    const double eps = (double)FLT_EPSILON;
    if (!defined) {
      for (int a = 0; a < 3; a++) {
        mn[a] = (double)q[a] - res / 2;
        mx[a] = (double)q[a] + res / 2;
      }
      // getKeyBitSize with no leaves: max_voxels = max(ceil((max - min - eps) / res), 2), depth = ceil(log2(max_voxels) - eps)
      unsigned max_voxels = 2;
      for (int a = 0; a < 3; a++) max_voxels = std::max(max_voxels, (unsigned)std::ceil((mx[a] - mn[a] - eps) / res));
      depth = (int)std::min(32.0, std::ceil(std::log2((double)max_voxels) - eps));
      if (depth > kMcMaxDepth) return DGS_ERR_GRID_TOO_LARGE;
      const double side = (double)(1 << depth) * res;
      for (int a = 0; a < 3; a++) {
        if (p->first_box_oversize) {
          const double over = (side - (mx[a] - mn[a])) / 2.0;
          if (over > eps) { mn[a] -= over; mx[a] += over; }
        } else {
          mx[a] = mn[a] + side;
        }
      }
      defined = true;
      open_epoch(index);
      return DGS_OK;
    }
    bool grown = false;
    while (true) {
      bool lower[3], upper[3], any = false;
      for (int a = 0; a < 3; a++) {
        lower[a] = (double)q[a] < mn[a];
        upper[a] = (double)q[a] >= mx[a];
        any = any || lower[a] || upper[a];
      }
      if (!any) {
        if (grown) open_epoch(index);
        return DGS_OK;
      }
      if (depth + 1 > kMcMaxDepth) return DGS_ERR_GRID_TOO_LARGE;
      double side = (double)(1 << depth) * res;
      for (int a = 0; a < 3; a++)
        if (p->grow_shift_without_upper ? !upper[a] : lower[a]) {
          mn[a] -= side;
          for (McEpoch& e : epochs) e.off[a] += 1u << depth;   // the old root goes under the child of the new root with this bit set
        }
      grown = true;
      depth++;
      side = (double)(1 << depth) * res;
      if (p->max_minus_epsilon) side -= eps;
      for (int a = 0; a < 3; a++) mx[a] = mn[a] + side;
      growths++;
    }
  }
};

int mc_begin(dgs_handle* h) {
  h->err.clear();
  DGS_HIP_TRY(h, hipSetDevice(h->device));
  return DGS_OK;
}

int mc_finish(dgs_handle* h, int rc) {
  if (rc != DGS_OK) {
    (void)hipStreamSynchronize(h->stream);
    h->mc.n_out = 0;
    return rc;
  }
  DGS_HIP_TRY(h, hipStreamSynchronize(h->stream));
  DGS_HIP_TRY(h, hipGetLastError());
  return DGS_OK;
}

inline unsigned mc_grid(int64_t items, int per_block) {
  return (unsigned)std::max<int64_t>(1, std::min<int64_t>((items + per_block - 1) / per_block, kMcMaxGridBlocks));
}

int mc_temp(dgs_handle* h, size_t bytes) {
  DGS_HIP_TRY(h, h->mc.temp.reserve(std::max<size_t>(bytes, 16)));
  return DGS_OK;
}

// the growth replay: walks the chunk boxes in order, asks the device for the first violating point of a chunk that leaves the box
int mc_replay(dgs_handle* h, const std::vector<McChunk>& chunks, const std::vector<float>& boxes, McOctree& oc) {
  McScratch& mc = h->mc;
  if (ensure_pinned(h, 4096) != DGS_OK) return DGS_ERR_HIP;
  int* res = reinterpret_cast<int*>(h->pinned);
  for (size_t c = 0; c < chunks.size(); c++) {
    const float* b = &boxes[c * 8];
    int finite;
    std::memcpy(&finite, &b[6], sizeof(int));
    if (finite == 0 || (oc.defined && oc.inside(b))) continue;
    const McChunk& ch = chunks[c];
    int from = 0;
    while (from < ch.count) {
      McBox box;
      for (int a = 0; a < 3; a++) { box.mn[a] = oc.mn[a]; box.mx[a] = oc.mx[a]; }
      box.defined = oc.defined ? 1 : 0;
      const int cnt = ch.count - from;
      hipLaunchKernelGGL(mc_find_first_kernel, dim3((cnt + kBlock - 1) / kBlock), dim3(kBlock), 0, h->stream, mc.frames.ptr, ch.frame, ch.begin + from, cnt,
                         box, mc.found.ptr);
      hipLaunchKernelGGL(mc_fetch_kernel, dim3(1), dim3(kWave), 0, h->stream, mc.frames.ptr, ch.frame, mc.found.ptr);
      DGS_HIP_TRY(h, hipGetLastError());
      DGS_HIP_TRY(h, hipMemcpyAsync(res, mc.found.ptr + 4, 4 * sizeof(int), hipMemcpyDeviceToHost, h->stream));
      DGS_HIP_TRY(h, hipStreamSynchronize(h->stream));
      mc.find_launches++;
      if (res[0] == INT_MAX) break;   // the box was left by points in front of `from` only (max shrinks by FLT_EPSILON at the first growth)
      float q[3];
      std::memcpy(q, &res[1], sizeof(q));
      if (int rc = oc.adopt(q, ch.start + (res[0] - ch.begin))) {
        h->err = "map cloud: the octree would be deeper than 21 levels (the points span more than 2^21 voxels)";
        return rc;
      }
      from = res[0] - ch.begin + 1;
      if (oc.inside(b)) break;
    }
  }
  return DGS_OK;
}

struct McInput {
  const float4* pts;   // device
  int64_t n;
};

int mc_generate(dgs_handle* h, const dgs_map_cloud_params* p, const std::vector<McInput>& in, const double* poses16, double resolution, int64_t* n_out) {
  McScratch& mc = h->mc;
  mc.n_out = 0;
  mc.depth = mc.growths = mc.find_launches = mc.used_sort = 0;
  for (int a = 0; a < 3; a++) mc.bb_min[a] = mc.bb_max[a] = 0.0;
  // ---- tables
  std::vector<McFrame> frames(in.size());
  std::vector<McChunk> chunks;
  int64_t total = 0;
  for (size_t k = 0; k < in.size(); k++) {
    McFrame& f = frames[k];
    f.pts = in[k].pts;
    f.n = (int)in[k].n;
    f.pad = 0;
    for (int r = 0; r < 3; r++)
      for (int c = 0; c < 4; c++) f.m[r * 4 + c] = (float)poses16[k * 16 + c * 4 + r];   // pose.matrix().cast<float>()
    for (int64_t b = 0; b < in[k].n; b += kMcChunk) {
      McChunk ch;
      ch.start = total + b;
      ch.frame = (int)k;
      ch.begin = (int)b;
      ch.count = (int)std::min<int64_t>(kMcChunk, in[k].n - b);
      ch.pad = 0;
      chunks.push_back(ch);
    }
    total += in[k].n;
  }
  if (total == 0) return DGS_OK;
  if (chunks.size() > (size_t)INT32_MAX) {
    h->err = "map cloud: too many points";
    return DGS_ERR_INVALID_ARGUMENT;
  }
  const int n_chunks = (int)chunks.size();
  DGS_HIP_TRY(h, mc.frames.reserve(frames.size()));
  DGS_HIP_TRY(h, mc.chunks.reserve(chunks.size()));
  DGS_HIP_TRY(h, hipMemcpyAsync(mc.frames.ptr, frames.data(), frames.size() * sizeof(McFrame), hipMemcpyHostToDevice, h->stream));
  DGS_HIP_TRY(h, hipMemcpyAsync(mc.chunks.ptr, chunks.data(), chunks.size() * sizeof(McChunk), hipMemcpyHostToDevice, h->stream));
  const unsigned chunk_grid = (unsigned)std::min(n_chunks, kMcMaxGridBlocks);

  // ---- resolution <= 0: the concatenation is the result (:35-36)
  if (!(resolution > 0.0)) {
    DGS_HIP_TRY(h, mc.out.reserve((size_t)total));
    hipLaunchKernelGGL(mc_concat_kernel, dim3(chunk_grid), dim3(kBlock), 0, h->stream, mc.frames.ptr, mc.chunks.ptr, n_chunks, mc.out.ptr);
    DGS_HIP_TRY(h, hipGetLastError());
    DGS_HIP_TRY(h, hipStreamSynchronize(h->stream));   // `frames` / `chunks` are read by the copies above
    mc.n_out = total;
    *n_out = total;
    return DGS_OK;
  }

  // ---- bounds pass
  std::vector<float> boxes((size_t)n_chunks * 8);
  DGS_HIP_TRY(h, mc.boxes.reserve(boxes.size()));
  if (mc.found.cap == 0) {
    DGS_HIP_TRY(h, mc.found.reserve(8));
    static const int kArm[8] = {INT_MAX, 0, 0, 0, INT_MAX, 0, 0, 0};
    DGS_HIP_TRY(h, hipMemcpyAsync(mc.found.ptr, kArm, sizeof(kArm), hipMemcpyHostToDevice, h->stream));
  }
  hipLaunchKernelGGL(mc_bounds_kernel, dim3(chunk_grid), dim3(kBlock), 0, h->stream, mc.frames.ptr, mc.chunks.ptr, n_chunks, mc.boxes.ptr);
  DGS_HIP_TRY(h, hipGetLastError());
  DGS_HIP_TRY(h, hipMemcpyAsync(boxes.data(), mc.boxes.ptr, boxes.size() * sizeof(float), hipMemcpyDeviceToHost, h->stream));
  DGS_HIP_TRY(h, hipStreamSynchronize(h->stream));
  int64_t finite_total = 0;
  for (int c = 0; c < n_chunks; c++) {
    int f;
    std::memcpy(&f, &boxes[(size_t)c * 8 + 6], sizeof(int));
    finite_total += f;
  }
  if (finite_total == 0) return DGS_OK;   // no point reaches the octree: no voxel

  // ---- growth replay
  McOctree oc;
  oc.res = resolution;
  oc.p = p;
  if (int rc = mc_replay(h, chunks, boxes, oc)) return rc;
  if (!p->key_at_insertion) {   // every key under the final min: one epoch
    oc.epochs.clear();
    oc.open_epoch(0);
  }
  DGS_HIP_TRY(h, mc.epochs.reserve(oc.epochs.size()));
  DGS_HIP_TRY(h, hipMemcpyAsync(mc.epochs.ptr, oc.epochs.data(), oc.epochs.size() * sizeof(McEpoch), hipMemcpyHostToDevice, h->stream));
  McGrid g;
  for (int a = 0; a < 3; a++) g.mn[a] = oc.mn[a];
  g.res = resolution;
  g.epochs = mc.epochs.ptr;
  g.n_epochs = (int)oc.epochs.size();
  g.x_msb = p->child_index_x_msb ? 1 : 0;
  const int key_bits = 3 * oc.depth;

  // ---- keys -> unique -> sorted
  DGS_HIP_TRY(h, mc.cnt.reserve(2));
  int64_t m = 0;
  // AUTO: a table of twice the points keeps the load under 1/2; beyond 2^26 slots that no longer holds and the sort is taken at once
  bool sorted_all = p->dedup_method == DGS_MAP_DEDUP_SORT ||
                    (p->dedup_method == DGS_MAP_DEDUP_AUTO && p->hash_slots == 0 && 2 * total > kMcMaxSlots && total <= INT32_MAX);
  if (!sorted_all) {
    // twice the points (an upper bound of the voxels) keeps the load under 1/2; a power of two, at most 2^26 slots
    const long long want = p->hash_slots > 0 ? (long long)p->hash_slots : std::max<long long>(2 * total, 1024);
    long long slots = 2;
    int log2_slots = 1;
    while (slots < want && slots < kMcMaxSlots) { slots <<= 1; log2_slots++; }
    DGS_HIP_TRY(h, mc.table.reserve((size_t)slots));
    DGS_HIP_TRY(h, mc.keys.reserve((size_t)std::min<long long>(slots, finite_total)));
    DGS_HIP_TRY(h, hipMemsetAsync(mc.table.ptr, 0xff, (size_t)slots * sizeof(unsigned long long), h->stream));
    DGS_HIP_TRY(h, hipMemsetAsync(mc.cnt.ptr, 0, 2 * sizeof(long long), h->stream));
    hipLaunchKernelGGL(mc_key_kernel<true>, dim3(chunk_grid), dim3(kBlock), 0, h->stream, mc.frames.ptr, mc.chunks.ptr, n_chunks, g, mc.table.ptr,
                       (unsigned long long)(slots - 1), 64 - log2_slots, (int)std::min<long long>(slots, kMcProbeLimit), mc.cnt.ptr, kMcEmpty);
    DGS_HIP_TRY(h, hipGetLastError());
    if (ensure_pinned(h, 4096) != DGS_OK) return DGS_ERR_HIP;
    long long* hc = reinterpret_cast<long long*>(h->pinned);
    // the overflow flag first: an overflowed table may hold more keys than mc.keys was sized for
    DGS_HIP_TRY(h, hipMemcpyAsync(hc, mc.cnt.ptr, 2 * sizeof(long long), hipMemcpyDeviceToHost, h->stream));
    DGS_HIP_TRY(h, hipStreamSynchronize(h->stream));
    if (hc[1] != 0) {
      if (p->dedup_method == DGS_MAP_DEDUP_HASH) {
        h->err = "map cloud: the key table overflowed (dedup_method = HASH)";
        return DGS_ERR_INVALID_ARGUMENT;
      }
      sorted_all = true;
    } else {
      size_t tb = 0;
      (void)hipcub::DeviceSelect::If(nullptr, tb, mc.table.ptr, mc.keys.ptr, mc.cnt.ptr, (int64_t)slots, McOccupied(), h->stream);
      if (int rc = mc_temp(h, tb)) return rc;
      DGS_HIP_TRY(h, hipcub::DeviceSelect::If(mc.temp.ptr, tb, mc.table.ptr, mc.keys.ptr, mc.cnt.ptr, (int64_t)slots, McOccupied(), h->stream));
      DGS_HIP_TRY(h, hipMemcpyAsync(hc, mc.cnt.ptr, sizeof(long long), hipMemcpyDeviceToHost, h->stream));
      DGS_HIP_TRY(h, hipStreamSynchronize(h->stream));
      m = hc[0];
      DGS_HIP_TRY(h, mc.keys_alt.reserve((size_t)m));
      (void)hipcub::DeviceRadixSort::SortKeys(nullptr, tb, mc.keys.ptr, mc.keys_alt.ptr, m, 0, key_bits, h->stream);
      if (int rc = mc_temp(h, tb)) return rc;
      DGS_HIP_TRY(h, hipcub::DeviceRadixSort::SortKeys(mc.temp.ptr, tb, mc.keys.ptr, mc.keys_alt.ptr, m, 0, key_bits, h->stream));
    }
  }
  if (sorted_all) {
    if (total > INT32_MAX) {
      h->err = "map cloud: more than INT32_MAX points on the sort path";
      return DGS_ERR_UNSUPPORTED;
    }
    mc.used_sort = 1;
    const unsigned long long sentinel = 1ull << key_bits;   // key_bits <= 63
    DGS_HIP_TRY(h, mc.table.reserve((size_t)total));
    DGS_HIP_TRY(h, mc.keys.reserve((size_t)total));
    DGS_HIP_TRY(h, mc.keys_alt.reserve((size_t)total));
    hipLaunchKernelGGL(mc_key_kernel<false>, dim3(chunk_grid), dim3(kBlock), 0, h->stream, mc.frames.ptr, mc.chunks.ptr, n_chunks, g, mc.table.ptr, 0ull, 0,
                       0, mc.cnt.ptr, sentinel);
    DGS_HIP_TRY(h, hipGetLastError());
    size_t tb = 0, tb2 = 0;
    (void)hipcub::DeviceRadixSort::SortKeys(nullptr, tb, mc.table.ptr, mc.keys.ptr, total, 0, key_bits + 1, h->stream);
    (void)hipcub::DeviceSelect::Unique(nullptr, tb2, mc.keys.ptr, mc.keys_alt.ptr, mc.cnt.ptr, total, h->stream);
    tb = std::max(tb, tb2);
    if (int rc = mc_temp(h, tb)) return rc;
    DGS_HIP_TRY(h, hipcub::DeviceRadixSort::SortKeys(mc.temp.ptr, tb, mc.table.ptr, mc.keys.ptr, total, 0, key_bits + 1, h->stream));
    DGS_HIP_TRY(h, hipcub::DeviceSelect::Unique(mc.temp.ptr, tb, mc.keys.ptr, mc.keys_alt.ptr, mc.cnt.ptr, total, h->stream));
    if (ensure_pinned(h, 4096) != DGS_OK) return DGS_ERR_HIP;
    long long* hc = reinterpret_cast<long long*>(h->pinned);
    DGS_HIP_TRY(h, hipMemcpyAsync(hc, mc.cnt.ptr, sizeof(long long), hipMemcpyDeviceToHost, h->stream));
    DGS_HIP_TRY(h, hipStreamSynchronize(h->stream));
    m = hc[0] - (finite_total < total ? 1 : 0);   // the sentinel of the non-finite points sorts last
  }

  // ---- centres
  const unsigned long long* sorted = mc.keys_alt.ptr;   // read here: both paths may have moved the buffer
  DGS_HIP_TRY(h, mc.out.reserve((size_t)std::max<int64_t>(m, 1)));
  if (m > 0) hipLaunchKernelGGL(mc_centre_kernel, dim3((unsigned)((m + kBlock - 1) / kBlock)), dim3(kBlock), 0, h->stream, sorted, (long long)m, g, mc.out.ptr);
  DGS_HIP_TRY(h, hipGetLastError());
  DGS_HIP_TRY(h, hipStreamSynchronize(h->stream));
  for (int a = 0; a < 3; a++) { mc.bb_min[a] = oc.mn[a]; mc.bb_max[a] = oc.mx[a]; }
  mc.depth = oc.depth;
  mc.growths = oc.growths;
  mc.n_out = m;
  *n_out = m;
  return DGS_OK;
}

bool mc_bad_params(const dgs_map_cloud_params* p) {
  return !p || p->struct_size != sizeof(dgs_map_cloud_params) || p->dedup_method < DGS_MAP_DEDUP_AUTO || p->dedup_method > DGS_MAP_DEDUP_SORT ||
         p->hash_slots < 0;
}

}  // namespace

void map_cloud_release(dgs_handle* h) {
  McScratch& mc = h->mc;
  mc.in.release(); mc.frames.release(); mc.chunks.release(); mc.epochs.release(); mc.boxes.release(); mc.found.release(); mc.table.release(); mc.keys.release();
  mc.keys_alt.release(); mc.cnt.release(); mc.temp.release(); mc.out.release();
  mc.n_out = 0;
}

}  // namespace dgs

using namespace dgs;

extern "C" {

int dgs_map_cloud_params_init(dgs_map_cloud_params* p) {
  if (!p) return DGS_ERR_INVALID_ARGUMENT;
  std::memset(p, 0, sizeof(*p));
  p->struct_size = sizeof(*p);
  p->first_box_oversize = 1;
  p->grow_shift_without_upper = 1;
  p->max_minus_epsilon = 1;
  p->child_index_x_msb = 1;
  p->key_at_insertion = 1;
  p->dedup_method = DGS_MAP_DEDUP_AUTO;
  p->hash_slots = 0;
  return DGS_OK;
}

int dgs_map_cloud_generate(dgs_handle* h, const dgs_map_cloud_params* p, int32_t n_keyframes, const float* const* clouds, const int64_t* sizes,
                           int32_t in_on_device, const double* poses16, double resolution, int64_t* n_out) {
  if (!h || mc_bad_params(p) || !n_out || n_keyframes < 0 || (n_keyframes > 0 && (!clouds || !sizes || !poses16)) || resolution != resolution)
    return DGS_ERR_INVALID_ARGUMENT;
  int64_t total = 0;
  for (int32_t k = 0; k < n_keyframes; k++) {
    if (sizes[k] < 0 || sizes[k] > INT32_MAX || (sizes[k] > 0 && !clouds[k])) return DGS_ERR_INVALID_ARGUMENT;
    total += sizes[k];
  }
  *n_out = 0;
  if (int rc = mc_begin(h)) return rc;
  h->mc.n_out = 0;
  std::vector<McInput> in((size_t)n_keyframes);
  int64_t off = 0;
  if (!in_on_device && total > 0) DGS_HIP_TRY(h, h->mc.in.reserve((size_t)total));
  for (int32_t k = 0; k < n_keyframes; k++) {
    in[k].n = sizes[k];
    in[k].pts = reinterpret_cast<const float4*>(clouds[k]);
    if (!in_on_device && sizes[k] > 0) {
      DGS_HIP_TRY(h, hipMemcpyAsync(h->mc.in.ptr + off, clouds[k], (size_t)sizes[k] * sizeof(float4), hipMemcpyHostToDevice, h->stream));
      in[k].pts = h->mc.in.ptr + off;
      off += sizes[k];
    }
  }
  return mc_finish(h, mc_generate(h, p, in, poses16, resolution, n_out));
}

int dgs_map_cloud_generate_clouds(dgs_handle* h, const dgs_map_cloud_params* p, int32_t n_keyframes, dgs_cloud* const* clouds, const double* poses16,
                                  double resolution, int64_t* n_out) {
  if (!h || mc_bad_params(p) || !n_out || n_keyframes < 0 || (n_keyframes > 0 && (!clouds || !poses16)) || resolution != resolution)
    return DGS_ERR_INVALID_ARGUMENT;
  for (int32_t k = 0; k < n_keyframes; k++)
    if (!clouds[k] || clouds[k]->device != h->device || clouds[k]->st.n < 0 || clouds[k]->st.n > INT32_MAX) return DGS_ERR_INVALID_ARGUMENT;
  *n_out = 0;
  if (int rc = mc_begin(h)) return rc;
  h->mc.n_out = 0;
  std::vector<McInput> in((size_t)n_keyframes);
  for (int32_t k = 0; k < n_keyframes; k++) {
    in[k].n = clouds[k]->st.n;
    in[k].pts = clouds[k]->st.pts.ptr;
  }
  return mc_finish(h, mc_generate(h, p, in, poses16, resolution, n_out));
}

int dgs_map_cloud_get(dgs_handle* h, float* out_xyz16, int64_t capacity, int32_t out_on_device, int64_t* n) {
  if (!h || !n || capacity < 0 || (capacity > 0 && !out_xyz16)) return DGS_ERR_INVALID_ARGUMENT;
  const int64_t m = h->mc.n_out;
  *n = m;
  if (capacity == 0 && !out_xyz16) return DGS_OK;
  if (m > capacity) {
    h->err = "output buffer too small for the map cloud";
    return DGS_ERR_INVALID_ARGUMENT;
  }
  if (m == 0) return DGS_OK;
  if (int rc = mc_begin(h)) return rc;
  DGS_HIP_TRY(h, hipMemcpyAsync(out_xyz16, h->mc.out.ptr, (size_t)m * sizeof(float4), out_on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, h->stream));
  DGS_HIP_TRY(h, hipStreamSynchronize(h->stream));
  return DGS_OK;
}

int dgs_map_cloud_get_grid(dgs_handle* h, double* min3, double* max3, int32_t* depth, int32_t* growths) {
  if (!h) return DGS_ERR_INVALID_ARGUMENT;
  const McScratch& mc = h->mc;
  for (int a = 0; a < 3; a++) {
    if (min3) min3[a] = mc.bb_min[a];
    if (max3) max3[a] = mc.bb_max[a];
  }
  if (depth) *depth = mc.depth;
  if (growths) *growths = mc.growths;
  return DGS_OK;
}

}  // extern "C"
