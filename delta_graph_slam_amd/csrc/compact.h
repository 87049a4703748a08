// The stable compaction every pass-through stage shares: a keep flag per element, a count pass (wave ballot + popcount per workgroup),
// one workgroup scanning the counts, and a scatter pass (ballot prefix inside the wave, the wave totals of the workgroup, the scanned
// workgroup offset).  The three kernels live in prefilter.hip; the prefilter, the floor detection, the line extraction and align_global
// launch them through the helpers below, and every scatter kernel takes its output slot from compact_slot.
#pragma once

#include <cstring>

#include "handle.h"
#include "prefilter_batch_plan.h"
#include "seg_device.h"
#include "seg_table.h"

namespace dgs {

constexpr int kCompactScanBlock = 1024;   // pf_scan_kernel's workgroup and chunk: its __launch_bounds__ and its only launch (compact_offsets)

__global__ __launch_bounds__(kBlock) void pf_count_kernel(const unsigned char* __restrict__ flags, const int n, int* __restrict__ blk);
__global__ __launch_bounds__(kCompactScanBlock) void pf_scan_kernel(int* __restrict__ blk, const int nb, int* __restrict__ total);
__global__ __launch_bounds__(kBlock) void pf_scatter_kernel(const float4* __restrict__ in, const unsigned char* __restrict__ flags, const int n,
                                                            const int* __restrict__ blk, float4* __restrict__ out, const int flatten);

// One lane per element, workgroups of kBlock over blk's scanned counts: -> whether element i is flagged; if so *off is its place in the
// compacted output (< number of flagged elements <= n).  Holds a barrier: every lane of the workgroup calls it.
template <class Index>
__device__ __forceinline__ bool compact_slot(const unsigned char* __restrict__ flags, const Index i, const Index n, const int* __restrict__ blk,
                                             int* off) {
  __shared__ int s_w[kBlock / kWave];
  const int lane = threadIdx.x & (kWave - 1), wv = threadIdx.x / kWave;
  const bool f = i < n && flags[i] != 0;
  const unsigned long long m = __ballot(f);
  if (lane == 0) s_w[wv] = __popcll(m);
  __syncthreads();
  if (!f) return false;
  int o = blk[blockIdx.x];
  for (int w = 0; w < wv; w++) o += s_w[w];
  *off = o + __popcll(m & ((1ull << lane) - 1ull));
  return true;
}

// ---- the same compaction over many segments in one chain (prefilter_batch.hip, floor_detection_batch.hip).  Every segment owns whole
// workgroups of the count and scatter launches, and its flags stand at its first workgroup * kBlock of the shared flag array.  The count
// pass writes every workgroup's count to blk[global workgroup] and workgroup 0 a 0 behind the last one: blk has gridDim.x + 1 entries
// and pf_scan_kernel scans all of them, so blk[first workgroup of segment s + 1] - blk[first workgroup of segment s] is the segment's
// total and blk[w] - blk[first workgroup of w's segment] is workgroup w's first slot inside its segment's output: what compact_offsets
// gives the segment alone (integer sums).  A segment entry `Seg` has flags (the segment's own), n (its size) and blk0 (its first
// workgroup); the launch bisects `first` (seg_find, seg_device.h).
template <class Seg>
__global__ __launch_bounds__(kBlock) void compact_count_seg_kernel(const Seg* __restrict__ tab, const int* __restrict__ first, const int m,
                                                                   int* __restrict__ blk) {
  __shared__ int s_w[kBlock / kWave];
  const Seg& e = tab[seg_find(first, m, (int)blockIdx.x)];
  const int i = ((int)blockIdx.x - e.blk0) * kBlock + threadIdx.x;
  const unsigned long long f = __ballot(i < e.n && e.flags[i] != 0);
  if ((threadIdx.x & (kWave - 1)) == 0) s_w[threadIdx.x / kWave] = __popcll(f);
  __syncthreads();
  if (threadIdx.x == 0) {
    int t = 0;
#pragma unroll
    for (int w = 0; w < kBlock / kWave; w++) t += s_w[w];
    blk[blockIdx.x] = t;
    if (blockIdx.x == 0) blk[gridDim.x] = 0;
  }
}
// The scatter launch's body for a workgroup of segment c = entry e: the segment's first workgroup writes its total, and every flagged
// element i (local, of the caller's Index type) goes to store(i, off), off < the segment's total <= n its place in the segment's output.
template <class Index, class Seg, class Store>
__device__ __forceinline__ void compact_scatter_seg(const Seg& e, const int c, const int* __restrict__ first, const int* __restrict__ blk,
                                                    int* __restrict__ totals, Store store) {
  __shared__ int s_w[kBlock / kWave];
  const int lb = (int)blockIdx.x - e.blk0, seg0 = blk[e.blk0];
  if (lb == 0 && threadIdx.x == 0) totals[c] = blk[first[c + 1]] - seg0;
  const Index i = (Index)lb * kBlock + threadIdx.x;
  const int lane = threadIdx.x & (kWave - 1), wv = threadIdx.x / kWave;
  const bool f = i < (Index)e.n && e.flags[i] != 0;
  const unsigned long long m = __ballot(f);
  if (lane == 0) s_w[wv] = __popcll(m);
  __syncthreads();
  if (!f) return;
  int o = blk[blockIdx.x] - seg0;
  for (int w = 0; w < wv; w++) o += s_w[w];
  store(i, o + __popcll(m & ((1ull << lane) - 1ull)));
}

inline unsigned compact_blocks(int64_t n) { return (unsigned)((n + kBlock - 1) / kBlock); }

// count + scan of `flags` over n elements: blk (compact_blocks(n) ints) becomes every workgroup's first output slot, *total the number
// of flagged elements
inline void compact_offsets(hipStream_t stream, const unsigned char* flags, int64_t n, int* blk, int* total) {
  const unsigned nb = compact_blocks(n);
  hipLaunchKernelGGL(pf_count_kernel, dim3(nb), dim3(kBlock), 0, stream, flags, (int)n, blk);
  hipLaunchKernelGGL(pf_scan_kernel, dim3(1), dim3(kCompactScanBlock), 0, stream, blk, (int)nb, total);
}

// compact n elements by `flags` into `out` (reserved here for n): count, scan, the caller's scatter launch scatter(workgroups), and
// *m = kept elements, read back through the pinned block: the host waits here
template <class T, class Scatter>
int compact_scatter(dgs_handle* h, const unsigned char* flags, int64_t n, DevBuf<int>& blk, DevBuf<int>& cnt, DevBuf<T>& out, int64_t* m,
                    Scatter scatter) {
  *m = 0;
  if (n == 0) return DGS_OK;
  DGS_HIP_TRY(h, out.reserve((size_t)n));
  DGS_HIP_TRY(h, blk.reserve(compact_blocks(n)));
  DGS_HIP_TRY(h, cnt.reserve(4));
  compact_offsets(h->stream, flags, n, blk.ptr, cnt.ptr);
  scatter(compact_blocks(n));
  DGS_HIP_TRY(h, hipGetLastError());
  if (ensure_pinned(h, 4096) != DGS_OK) return DGS_ERR_HIP;
  int* hc = reinterpret_cast<int*>(h->pinned);
  DGS_HIP_TRY(h, hipMemcpyAsync(hc, cnt.ptr, sizeof(int), hipMemcpyDeviceToHost, h->stream));
  DGS_HIP_TRY(h, hipStreamSynchronize(h->stream));
  *m = hc[0];
  return DGS_OK;
}

// the points of `in` whose flag is set, in order, whole 16-byte points; `flatten` zeroes z on the way
inline int compact_points(dgs_handle* h, const float4* in, const unsigned char* flags, int64_t n, DevBuf<int>& blk, DevBuf<int>& cnt,
                          DevBuf<float4>& out, bool flatten, int64_t* m) {
  return compact_scatter(h, flags, n, blk, cnt, out, m, [&](unsigned nb) {
    hipLaunchKernelGGL(pf_scatter_kernel, dim3(nb), dim3(kBlock), 0, h->stream, in, flags, (int)n, blk.ptr, out.ptr, flatten ? 1 : 0);
  });
}

// ---- the host side of the segmented compaction, over a stage of pfbplan (one item per live scan) and the buffers of a SegCompact
// the device addresses of an uploaded stage table and the pinned places its results come down into
template <class Seg>
struct SegDev {
  const Seg* tab;
  const void* heads;   // one record per item, for a stage that has them
  const int* first;
  const int* knn_first;
  int* totals_h;       // where the compaction's totals arrive (one per item)
  double* stats_h;     // room for 4 doubles per item
};

// the flag array of a stage and every entry's place in it
template <class Seg>
int seg_flags(dgs_handle* h, SegCompact& C, const pfbplan::Stage& St, std::vector<Seg>& segs) {
  DGS_HIP_TRY(h, C.flags.reserve((size_t)St.blocks * kBlock));
  for (size_t j = 0; j < segs.size(); j++) {
    segs[j].flags = C.flags.ptr + (size_t)St.items[j].blk0 * kBlock;
    segs[j].n = (int)St.items[j].n;
    segs[j].blk0 = St.items[j].blk0;
  }
  return DGS_OK;
}

// entries | heads | first workgroups | first search workgroups (zeros in a stage without a search) -> C.tables in one copy from the
// pinned block.  `heads`: head_bytes per scan of the chunk, or nullptr.  Nothing in flight reads the block: every stage ends with a
// host wait, or its caller waits before the next one (floor_detection_batch.hip fdb_chain), so it may be rewritten and regrown.
template <class Seg>
int seg_upload(dgs_handle* h, SegCompact& C, const pfbplan::Stage& St, const std::vector<Seg>& segs, const void* heads, const size_t head_bytes,
               SegDev<Seg>* dev) {
  const size_t m = St.items.size();
  const segtab::StageTable T = segtab::stage_table(m, sizeof(Seg), heads ? head_bytes : 0);
  DGS_HIP_TRY(h, C.stage.reserve(T.all));
  DGS_HIP_TRY(h, C.tables.reserve(T.up));
  DGS_HIP_TRY(h, C.totals.reserve(m));
  char* st = C.stage.at(0);
  segtab::place(st, T, segs.data(), m * sizeof(Seg), St.first());
  if (heads)
    for (size_t j = 0; j < m; j++) std::memcpy(st + T.heads + j * head_bytes, static_cast<const char*>(heads) + (size_t)St.items[j].scan * head_bytes, head_bytes);
  const std::vector<int> knn_first = St.knn_first();
  std::memcpy(st + T.knn_first, knn_first.data(), (m + 1) * sizeof(int));
  DGS_HIP_TRY(h, hipMemcpyAsync(C.tables.ptr, st, T.up, hipMemcpyHostToDevice, h->stream));
  dev->tab = reinterpret_cast<const Seg*>(C.tables.ptr + T.entries);
  dev->heads = C.tables.ptr + T.heads;
  dev->first = reinterpret_cast<const int*>(C.tables.ptr + T.first);
  dev->knn_first = reinterpret_cast<const int*>(C.tables.ptr + T.knn_first);
  dev->totals_h = reinterpret_cast<int*>(st + T.totals);
  dev->stats_h = reinterpret_cast<double*>(st + T.stats);
  return DGS_OK;
}

// count, scan, the caller's scatter launch scatter(workgroups, blk, totals) over all scans of the stage; kept[j] = kept points of item
// j, read back: the host waits here.  Three launches and one wait are added to counts8[0] and [1].
template <class Seg, class Scatter>
int seg_compact(dgs_handle* h, SegCompact& C, const pfbplan::Stage& St, const SegDev<Seg>& dev, int64_t* counts8, std::vector<int64_t>& kept,
                Scatter scatter) {
  const int m = (int)St.items.size();
  DGS_HIP_TRY(h, C.blk.reserve((size_t)St.blocks + 1));
  DGS_HIP_TRY(h, C.cnt.reserve(4));
  hipLaunchKernelGGL(compact_count_seg_kernel<Seg>, dim3((unsigned)St.blocks), dim3(kBlock), 0, h->stream, dev.tab, dev.first, m, C.blk.ptr);
  hipLaunchKernelGGL(pf_scan_kernel, dim3(1), dim3(kCompactScanBlock), 0, h->stream, C.blk.ptr, St.blocks + 1, C.cnt.ptr);
  scatter(dim3((unsigned)St.blocks), C.blk.ptr, C.totals.ptr);
  DGS_HIP_TRY(h, hipGetLastError());
  DGS_HIP_TRY(h, hipMemcpyAsync(dev.totals_h, C.totals.ptr, (size_t)m * sizeof(int), hipMemcpyDeviceToHost, h->stream));
  DGS_HIP_TRY(h, hipStreamSynchronize(h->stream));
  counts8[0] += 3;
  counts8[1]++;
  kept.assign((size_t)m, 0);
  for (int j = 0; j < m; j++) kept[j] = dev.totals_h[j];
  return DGS_OK;
}

}  // namespace dgs
