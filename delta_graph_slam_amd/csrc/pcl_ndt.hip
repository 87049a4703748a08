// PCL_NDT_HIP (DGS_METHOD_PCL_NDT): pcl::NormalDistributionsTransform::computeDerivatives / computeHessian on the device -- score, gradient
// and Hessian in DOUBLE, which is what separates pcl::NDT from ndt_omp (whose updateDerivatives is float).  Serves the reference
// factory's default branch (src/hdl_graph_slam/registrations.cpp:94-100).  DESIGN.md section 6i.
//
// This file holds the evaluation kernel alone.  The align loop is the NDT driver's (ndt_align.hip: launch plan, chunks, flags, export),
// the optimiser the upstream order's (ndt_optimiser.h, ndt_strict.h ndt_close_strict: More-Thuente, JacobiSVD Newton step, the trial
// cache): those headers are included a second time here, in a namespace of their own, with DGS_NDT_PCL_DOUBLE -- write_evaluation then
// leaves the double angle vectors with EVERY evaluation, and the stand-alone solve kernels stay with ndt_align.hip.
//
// Kernel: one launch per evaluation for the whole batch.  A lane takes a point: float transform, the 27-cell walk with the float
// distance test (pn::neighbourhood) kept as a BIT MASK -- the voxel of a slot is looked up again from the cell and the slot's offset
// where the item runs, so no 27-entry private array exists --, the point's 23 double products with the angle vectors, then its valid
// voxels one after the other (a wave runs as many rounds as its fullest lane has voxels), pn::item adding to the lane's 43 double sums.
// A pair's points are cut into FIXED slices (ndt_strict.h strict_slices_of: a function of the pair's own size); a slice's sums make
// one row (strict_block_row: lanes, then waves, in fixed order), the pair's closing workgroup adds the rows in slice order
// (ndt_close_strict) and advances the optimiser.  So a pair's doubles do not depend on the batch it runs in, and an evaluation
// differs from a CPU run of upstream in the association of the double additions only.
// The three evaluation kinds are three instantiations of the point loop behind a workgroup-uniform branch: a More-Thuente trial
// carries no Hessian code.  One wave per SIMD (__launch_bounds__(kBlock, 1)): 86 registers of sums, 46 of point tables and the item's
// 3 x 3 / 6 x 3 double temporaries do not fit 256 registers, and the FP64 work of an item (~600 operations) is issue bound, not
// latency bound.  No scratch memory (tests/test_pcl_ndt_cpu.py reads the code object's metadata).
#include <cmath>
#include <cstring>
#include <vector>

#include "handle.h"
#include "pcl_ndt.h"
#include "solve6.h"

#define DGS_NDT_PCL_DOUBLE 1

namespace dgs {
namespace pcl_ndt {

#include "ndt_fast.h"   // Offsets, the declarations ndt_optimiser.h completes (no kernel of it is instantiated here)
#pragma clang fp contract(off)
#include "ndt_exp_tables.h"
#include "ndt_optimiser.h"
#include "ndt_strict.h"

static_assert(pn::kAccum == kStrictAccum && pn::kPointsPerWorkgroup == kBlock && pn::kSlots == Offsets<DGS_NDT_KDTREE>::N, "pcl_ndt.h and the NDT driver agree");

__device__ __forceinline__ pn::Grid grid_view(const VoxelGrid& g, const int leaf_pow2) {
  pn::Grid v;
#pragma unroll
  for (int k = 0; k < 3; k++) { v.min_b[k] = g.min_b[k]; v.max_b[k] = g.max_b[k]; }
  v.mul1 = g.mul1;
  v.mul2 = g.mul2;
  v.leaf = g.leaf;
  v.inv_leaf = g.inv_leaf;
  v.leaf_pow2 = leaf_pow2;
  v.cell2vox = g.cell2vox;
  v.centroid = reinterpret_cast<const float*>(g.centroid);
  return v;
}

// the points of slice q of a pair: i = q * kBlock + lane, + n_slices * kBlock, ...
template <int KIND>
__device__ __forceinline__ void slice_points(const float4* __restrict__ src, const int n, const int q, const int n_slices, const float (&T)[12], const pn::Grid& g,
                                             const double (*J)[3], const double (*H)[3], const double* __restrict__ vtab, const double gauss_d1, const double gauss_d2,
                                             const unsigned long long* __restrict__ exptab, double (&acc)[pn::kAccum]) {
  auto expd = [exptab](const double a) { return exptab ? glibc_exp_dev(a, exptab) : det_exp(a); };
#pragma unroll 1
  for (int i = q * kBlock + (int)threadIdx.x; i < n; i += n_slices * kBlock) {
    const float4 x = src[i];
    float xt[3];
    pn::transform_point(T, x.x, x.y, x.z, xt);
    int c[3];
    unsigned mask = pn::neighbourhood(g, xt, c);
    if (!mask) continue;
    const double xd[3] = {(double)x.x, (double)x.y, (double)x.z};
    double xj[8], xh[15];
    pn::point_tables<KIND != 0>(xd, J, H, xj, xh);
#pragma unroll 1
    while (mask) {
      const int k = __ffs(mask) - 1;
      mask &= mask - 1u;
      const int vid = pn::slot_voxel(g, c, k);   // >= 0: the slot passed the neighbourhood's tests
      pn::item<KIND>(xt, xj, xh, vtab + (size_t)vid * 12, gauss_d1, gauss_d2, acc, expd);
    }
  }
}

// FUSED: round `launch` of the align; the workgroup that takes the pair's last ticket closes the evaluation.  Otherwise rows only (the
// test hooks: ndt_solve_kernel adds them).
template <bool FUSED>
__global__ __launch_bounds__(kBlock, 1) void pcl_ndt_kernel(const float4* const* __restrict__ src_ptrs, const int* __restrict__ src_sizes, NdtPair* __restrict__ pairs,
                                                           const VoxelGrid g, const double* __restrict__ vtab, const double gauss_d1, const double gauss_d2,
                                                           const int leaf_pow2, double* __restrict__ partials, const int n_pairs, const int cap_blocks,
                                                           int* __restrict__ pair_blocks, const NdtConsts consts, int* __restrict__ done_flags, const int launch) {
  int pair, slice, blocks_per_pair;
  if (!deal_workgroup(n_pairs, cap_blocks, [&](int pi) { return FUSED ? (launch <= pairs[pi].serve[0]) : (pairs[pi].active != 0); }, pair, slice, blocks_per_pair)) return;
  const NdtPair& st = pairs[pair];
  const float4* __restrict__ src = src_ptrs[pair];
  const int n = src_sizes[pair];
  const int n_slices = strict_slices_of(n, cap_blocks);
  if (slice == 0 && threadIdx.x == 0) pair_blocks[pair] = n_slices;
  const int kind = st.need_hessian;   // 0: score + gradient, 1: + Hessian, 2: Hessian alone (computeHessian)
  float T[12];
#pragma unroll
  for (int k = 0; k < 12; k++) T[k] = st.T[k];
  // the double angle vectors of this evaluation: read per point, the same address in every lane
  __shared__ double s_ang[23][3];
  if (threadIdx.x < 69) {
    const int r = threadIdx.x / 3, c = threadIdx.x % 3;
    s_ang[r][c] = (r < 8) ? st.jang_d[r][c] : st.hang_d[r - 8][c];
  }
  __syncthreads();
  const double (*J)[3] = s_ang;
  const double (*H)[3] = s_ang + 8;
  const pn::Grid gv = grid_view(g, leaf_pow2);
  const unsigned long long* __restrict__ exptab = consts.exp_libm ? kGlibcExpTab : nullptr;
  double* rows_of_pair = partials + (size_t)pair * cap_blocks * kStrictPad;
#pragma unroll 1
  for (int q = slice; q < n_slices; q += blocks_per_pair) {
    double acc[pn::kAccum];
#pragma unroll
    for (int k = 0; k < pn::kAccum; k++) acc[k] = 0.0;
    if (kind == 1) slice_points<1>(src, n, q, n_slices, T, gv, J, H, vtab, gauss_d1, gauss_d2, exptab, acc);
    else if (kind == 2) slice_points<2>(src, n, q, n_slices, T, gv, J, H, vtab, gauss_d1, gauss_d2, exptab, acc);
    else slice_points<0>(src, n, q, n_slices, T, gv, J, H, vtab, gauss_d1, gauss_d2, exptab, acc);
    strict_block_row<FUSED>(acc, kind ? kStrictAccum : 7, rows_of_pair + (size_t)q * kStrictPad);
    __syncthreads();   // the next slice's reduction reuses the LDS of this one
  }
  if (!FUSED) return;
  __shared__ int s_last;
  if (threadIdx.x < kStrictPad) handoff_drain_stores();
  __syncthreads();
  if (threadIdx.x == 0) s_last = handoff_take_ticket(&pairs[pair].ticket, blocks_per_pair) ? 1 : 0;
  __syncthreads();
  if (!s_last) return;
  ndt_close_strict<false, true>(pairs + pair, rows_of_pair, n_slices, consts, done_flags + pair, launch);
}

// The evaluation the init kernel has set up (ndt_align.hip: the guess, or a test hook's pose) gets its double angle vectors.
__global__ void pcl_ndt_tables_kernel(NdtPair* __restrict__ pairs, const int n_pairs, const NdtConsts c) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_pairs) return;
  NdtPair* st = pairs + i;
  double x[6];
  for (int k = 0; k < 6; k++) x[k] = st->s.x_t[k];
  write_evaluation<false>(st, st, st->s, c, x, st->need_hessian, false, true);
}

// dgs_pcl_ndt_neighbours: the neighbourhood of every query as the kernel finds it; ids ascending, -1 padded
__global__ __launch_bounds__(kBlock) void pcl_ndt_neighbours_kernel(const float4* __restrict__ queries, const int64_t m, const VoxelGrid g, const int leaf_pow2,
                                                                   int* __restrict__ counts, int* __restrict__ ids) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= m) return;
  const pn::Grid gv = grid_view(g, leaf_pow2);
  const float4 x = queries[i];
  const float xt[3] = {x.x, x.y, x.z};
  int c[3];
  unsigned mask = pn::neighbourhood(gv, xt, c);
  int* row = ids + i * pn::kSlots;
  int cnt = 0;
  while (mask) {
    const int k = __ffs(mask) - 1;
    mask &= mask - 1u;
    const int vid = pn::slot_voxel(gv, c, k);
    int j = cnt++;
    for (; j > 0 && row[j - 1] > vid; j--) row[j] = row[j - 1];   // insertion into the row itself: at most 27 entries
    row[j] = vid;
  }
  for (int j = cnt; j < pn::kSlots; j++) row[j] = -1;
  counts[i] = cnt;
}

}  // namespace pcl_ndt

static int leaf_is_pow2(const dgs_handle* h) {
  int fe = 0;
  return (std::frexp(h->grid.leaf, &fe) == 0.5f) ? 1 : 0;
}

void pcl_ndt_launch(dgs_handle* h, int n_pairs, int cap_blocks, int total_blocks, int launch, hipStream_t st) {
  const int leaf_pow2 = leaf_is_pow2(h);
  if (launch >= 0)
    hipLaunchKernelGGL((pcl_ndt::pcl_ndt_kernel<true>), dim3(total_blocks), dim3(kBlock), 0, st, h->src_ptrs.ptr, h->src_sizes.ptr, h->pairs.ptr, h->grid, h->vox_dbg.ptr,
                       h->consts.gauss_d1, h->consts.gauss_d2, leaf_pow2, h->partials.ptr, n_pairs, cap_blocks, h->pair_blocks.ptr, h->consts, h->done_flags, launch);
  else
    hipLaunchKernelGGL((pcl_ndt::pcl_ndt_kernel<false>), dim3(total_blocks), dim3(kBlock), 0, st, h->src_ptrs.ptr, h->src_sizes.ptr, h->pairs.ptr, h->grid, h->vox_dbg.ptr,
                       h->consts.gauss_d1, h->consts.gauss_d2, leaf_pow2, h->partials.ptr, n_pairs, cap_blocks, h->pair_blocks.ptr, h->consts, h->done_counter.ptr, launch);
}

void pcl_ndt_init_tables(dgs_handle* h, int n_pairs, hipStream_t st) {
  hipLaunchKernelGGL(pcl_ndt::pcl_ndt_tables_kernel, dim3((n_pairs + 63) / 64), dim3(64), 0, st, h->pairs.ptr, n_pairs, h->consts);
}

int pcl_ndt_neighbours(dgs_handle* h, const float* queries_xyz16, int64_t m, int on_device, int32_t* counts, int32_t* voxel_ids) {
  if (m == 0) return DGS_OK;
  hipStream_t st = h->stream;
  const float4* dq = reinterpret_cast<const float4*>(queries_xyz16);
  if (!on_device) {
    DGS_HIP_TRY(h, h->scratch_cloud.reserve((size_t)m));
    DGS_HIP_TRY(h, hipMemcpyAsync(h->scratch_cloud.ptr, queries_xyz16, (size_t)m * sizeof(float4), hipMemcpyHostToDevice, st));
    dq = h->scratch_cloud.ptr;
  }
  DevBuf<int> out;   // a test hook: its buffer lives for the call
  hipError_t e = out.reserve((size_t)m * (pn::kSlots + 1));
  if (e != hipSuccess) { h->err = std::string("hipMalloc: ") + hipGetErrorString(e); return DGS_ERR_HIP; }
  int* d_counts = out.ptr;
  int* d_ids = out.ptr + m;
  hipLaunchKernelGGL(pcl_ndt::pcl_ndt_neighbours_kernel, dim3((unsigned)((m + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, dq, m, h->grid, leaf_is_pow2(h), d_counts, d_ids);
  int rc = DGS_OK;
  if ((e = hipMemcpyAsync(counts, d_counts, (size_t)m * sizeof(int), hipMemcpyDeviceToHost, st)) != hipSuccess ||
      (e = hipMemcpyAsync(voxel_ids, d_ids, (size_t)m * pn::kSlots * sizeof(int), hipMemcpyDeviceToHost, st)) != hipSuccess ||
      (e = hipStreamSynchronize(st)) != hipSuccess || (e = hipGetLastError()) != hipSuccess) {
    h->err = std::string("dgs_pcl_ndt_neighbours: ") + hipGetErrorString(e);
    rc = DGS_ERR_HIP;
    (void)hipStreamSynchronize(st);
  }
  out.release();
  return rc;
}

}  // namespace dgs
