// The stable compaction every pass-through stage shares: a keep flag per element, a count pass (wave ballot + popcount per workgroup),
// one workgroup scanning the counts, and a scatter pass (ballot prefix inside the wave, the wave totals of the workgroup, the scanned
// workgroup offset).  The three kernels live in prefilter.hip; the prefilter, the floor detection, the line extraction and align_global
// launch them through the helpers below, and every scatter kernel takes its output slot from compact_slot.
#pragma once

#include "handle.h"

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

// ---- the same compaction over many segments in one chain (prefilter_batch.hip).  Every segment owns whole workgroups of the count and
// scatter launches, and its flags stand at its first workgroup * kBlock of the shared flag array.  The count pass writes every
// workgroup's count to blk[global workgroup] (and a 0 behind the last one), pf_scan_kernel scans all of them plus that one, so
// blk[first workgroup of segment s + 1] - blk[first workgroup of segment s] is the segment's total and blk[w] - blk[first workgroup of
// w's segment] is workgroup w's first slot inside its segment's output: what compact_offsets gives the segment alone (integer sums).
// `flags`: the segment's own flags, i its local element, n its size.  -> the workgroup's count in lane 0 of wave 0 (every lane calls it).
template <class Index>
__device__ __forceinline__ int compact_count_seg(const unsigned char* __restrict__ flags, const Index i, const Index n) {
  __shared__ int s_w[kBlock / kWave];
  const bool f = i < n && flags[i] != 0;
  const unsigned long long m = __ballot(f);
  if ((threadIdx.x & (kWave - 1)) == 0) s_w[threadIdx.x / kWave] = __popcll(m);
  __syncthreads();
  int t = 0;
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 0; w < kBlock / kWave; w++) t += s_w[w];
  }
  return t;
}
// compact_slot for a workgroup whose first slot inside its segment's output is `base`
template <class Index>
__device__ __forceinline__ bool compact_slot_seg(const unsigned char* __restrict__ flags, const Index i, const Index n, const int base, int* off) {
  __shared__ int s_w[kBlock / kWave];
  const int lane = threadIdx.x & (kWave - 1), wv = threadIdx.x / kWave;
  const bool f = i < n && flags[i] != 0;
  const unsigned long long m = __ballot(f);
  if (lane == 0) s_w[wv] = __popcll(m);
  __syncthreads();
  if (!f) return false;
  int o = base;
  for (int w = 0; w < wv; w++) o += s_w[w];
  *off = o + __popcll(m & ((1ull << lane) - 1ull));
  return true;
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

}  // namespace dgs
