// Device-side tail of a fixed-slices round launch (icp_iterate_kernel, pg_round_kernel; host side: batch_rounds.h): every workgroup
// is one slice of one pair, publishes one row of double sums, and the pair's last workgroup gets the totals.
#pragma once
#include "common.h"

namespace dgs {

// Wave DPP sums -> LDS -> this slice's row (write-through) -> the pair's ticket (common.h "in-launch hand-off"); in the workgroup that
// took the pair's last ticket the rows are then summed into tot and the function returns true, behind a barrier, for all its lanes.
// Called by all kBlock lanes.  ncols: live columns of acc (workgroup-uniform); the other columns of the row are written as 0.
// Every sum has a fixed order: the four waves as ((w0 + w1) + w2) + w3, the rows as kBlock / PAD strided partial sums per column in
// slice order, those partial sums in group order -- a pair's totals are a function of its own slices alone.
template <int ACCUM, int PAD>
__device__ __forceinline__ bool slice_rows_close(const double (&acc)[ACCUM], const int ncols, double* __restrict__ rows, const int slice0, const int n_slices,
                                                 int* ticket, double (&tot)[PAD]) {
  static_assert(kBlock / kWave == 4 && ACCUM <= PAD && kBlock % PAD == 0, "row shape");
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __shared__ double sm[kBlock / kWave][ACCUM];
#pragma unroll
  for (int k = 0; k < ACCUM; k++) {
    if (k < ncols) {
      const double v = wave_sum_to_lane63(acc[k]);
      if (lane == 63) sm[wave][k] = v;
    }
  }
  __syncthreads();
  double* row = rows + (size_t)blockIdx.x * PAD;
  if (threadIdx.x < PAD) {
    double v = 0.0;
    if ((int)threadIdx.x < ncols) v = ((sm[0][threadIdx.x] + sm[1][threadIdx.x]) + sm[2][threadIdx.x]) + sm[3][threadIdx.x];
    handoff_store_row(row + threadIdx.x, v);
    handoff_drain_stores();
  }
  __shared__ int s_last;
  __syncthreads();
  if (threadIdx.x == 0) s_last = handoff_take_ticket(ticket, n_slices) ? 1 : 0;
  __syncthreads();
  if (!s_last) return false;
  constexpr int G = kBlock / PAD;
  __shared__ double part[G][PAD];
  const int col = threadIdx.x % PAD, grp = threadIdx.x / PAD;
  double v = 0.0;
  const double* base = rows + (size_t)slice0 * PAD + col;
  for (int b = grp; b < n_slices; b += G) v += handoff_load_row(base + (size_t)b * PAD);
  part[grp][col] = v;
  __syncthreads();
  if (threadIdx.x < PAD) {
    double t = 0.0;
#pragma unroll
    for (int k = 0; k < G; k++) t += part[k][threadIdx.x];
    tot[threadIdx.x] = t;
  }
  __syncthreads();
  return true;
}

}  // namespace dgs
