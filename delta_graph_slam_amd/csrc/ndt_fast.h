// The default (fast) evaluation order of NDT's computeDerivatives: the per-point fold shared with the queue kernel, the block
// reduction of the 28 totals and ndt_derivatives_kernel.  Included by ndt_align.hip FIRST, inside namespace dgs and above its
// `#pragma clang fp contract(off)`: this is the only NDT device code the compiler may contract into multiply-adds.  Needs handle.h
// (common.h: NdtPair, VoxelGrid, the hand-off helpers); ndt_close_evaluation is declared here and defined in ndt_optimiser.h.

// ================================================================================================ derivatives
template <int SEARCH>
struct Offsets;
template <>
struct Offsets<DGS_NDT_DIRECT1> {
  static constexpr int N = 1;
};
template <>
struct Offsets<DGS_NDT_DIRECT7> {
  static constexpr int N = 7;
};
template <>
struct Offsets<DGS_NDT_DIRECT26> {
  static constexpr int N = 27;
};
template <>
struct Offsets<DGS_NDT_KDTREE> {
  static constexpr int N = 27;
};

template <int SEARCH>
__device__ __forceinline__ void neighbour_offset(int k, int& dx, int& dy, int& dz) {
  if (SEARCH == DGS_NDT_DIRECT1) {
    dx = dy = dz = 0;
  } else if (SEARCH == DGS_NDT_DIRECT7) {
    // (0,0,0) (+x) (-x) (+y) (-y) (+z) (-z): pclomp getNeighborhoodAtPoint7 order
    dx = (k == 1) - (k == 2);
    dy = (k == 3) - (k == 4);
    dz = (k == 5) - (k == 6);
  } else {
    dx = k / 9 - 1;
    dy = (k / 3) % 3 - 1;
    dz = k % 3 - 1;
  }
}

template <bool QUEUE = false, bool DONE_FLAG = false>
__device__ __forceinline__ bool ndt_close_evaluation(NdtPair* st, const double* partials_of_pair, int blocks_per_pair, const NdtConsts& c, int* done_counter, int launch,
                                                     NdtPair* hdr_next = nullptr, int need_h_in = -1);

// FUSED = false: derivatives only; ndt_solve_kernel (one workgroup per pair) follows as a second launch.
// FUSED = true: the workgroup of a pair that finishes LAST (a per-pair ticket) also sums the pair's partial rows in their fixed
// order and advances the optimiser, so an evaluation is ONE launch: no second kernel boundary, no second launch latency, and the
// optimiser steps of pairs that finish early overlap the derivative work of the others.  The hand-off is the write-through form
// of the agent-scope recipe: every byte of a row is stored sc1 (8-byte agent-scope stores), the storing wave drains, a
// workgroup barrier, ONE lane takes the ticket with an agent-scope atomic add; the workgroup whose add came last reads the rows
// with sc1 loads behind a barrier that lane joins.  Results do not depend on placement or timing; the rows are still added in
// slice order.  `launch` numbers the launches of one align: a pair takes part while launch <= its last_launch word,
// which its closing workgroup may write during a launch without changing what the other workgroups of that launch see.
// __launch_bounds__(kBlock, 4) holds the kernel at the derivative loop's 4 waves per SIMD; the optimiser tail (one workgroup per
// pair and launch) spills what does not fit.
// ---- the per-point work of computeDerivatives (fast order), shared by the launch-per-evaluation kernel and the queue kernel ----------
// The angle tables of the evaluation come through an accessor: the pair's record in HBM read with scalar loads (valid across a
// kernel boundary), or a copy in scalar registers made from coherent loads (inside the persistent queue kernel).
struct NdtHdrGlobal {
  const NdtPair& st;
  __device__ __forceinline__ float J(int k, int c) const { return st.jang[k][c]; }
  __device__ __forceinline__ float H(int k, int c) const { return st.hang[k][c]; }
};
struct NdtHdrRegs {
  float j[24], h[45];
  __device__ __forceinline__ float J(int k, int c) const { return j[k * 3 + c]; }
  __device__ __forceinline__ float H(int k, int c) const { return h[k * 3 + c]; }
};

template <int SEARCH, class HDR>
__device__ __forceinline__ void ndt_point_loop(const float (&T)[12], const HDR& hdr, const bool need_h, const float4* __restrict__ src, const int n,
                                               const int first, const int stride, const VoxelGrid& g, const double gd1, const float gd2,
                                               const int leaf_pow2, double (&acc)[kAccum]) {
  const float r2 = g.leaf * g.leaf;
  for (int i = first; i < n; i += stride) {
    const float4 x = src[i];
    // pcl::transformPointCloud in float, ((m0 x + m1 y) + m2 z) + m3 with every step rounded (no FMA contraction):
    // q = x' - mean is a cancellation, so one ulp of x' is ~1e-5 of a point's contribution -- keep x' exact.
    const float xt0 = affine_row_rn(T[0], T[1], T[2], T[3], x.x, x.y, x.z);
    const float xt1 = affine_row_rn(T[4], T[5], T[6], T[7], x.x, x.y, x.z);
    const float xt2 = affine_row_rn(T[8], T[9], T[10], T[11], x.x, x.y, x.z);
    // getNeighborhoodAtPoint: floor(x / leaf_size); x * (1 / leaf) is the same number when leaf is a power of two
    const int c0 = (int)floorf(leaf_pow2 ? xt0 * g.inv_leaf : xt0 / g.leaf);
    const int c1 = (int)floorf(leaf_pow2 ? xt1 * g.inv_leaf : xt1 / g.leaf);
    const int c2 = (int)floorf(leaf_pow2 ? xt2 * g.inv_leaf : xt2 / g.leaf);

    // ---- gather: voxel ids of the neighbourhood (independent loads, issued together)
    constexpr int NB = Offsets<SEARCH>::N;
    int vid[NB];
    // interior cells (every neighbour inside the grid) need no per-neighbour bounds test: base pointer + fixed offsets
    const bool interior = c0 > g.min_b[0] && c0 < g.max_b[0] && c1 > g.min_b[1] && c1 < g.max_b[1] && c2 > g.min_b[2] && c2 < g.max_b[2];
    if (interior) {
      const int* __restrict__ base = g.cell2vox + ((c0 - g.min_b[0]) + (c1 - g.min_b[1]) * g.mul1 + (c2 - g.min_b[2]) * g.mul2);
#pragma unroll
      for (int k = 0; k < NB; k++) {
        int dx, dy, dz;
        neighbour_offset<SEARCH>(k, dx, dy, dz);
        vid[k] = base[dx + dy * g.mul1 + dz * g.mul2];
      }
    } else {
#pragma unroll
      for (int k = 0; k < NB; k++) {
        int dx, dy, dz;
        neighbour_offset<SEARCH>(k, dx, dy, dz);
        const int a0 = c0 + dx, a1 = c1 + dy, a2 = c2 + dz;
        const bool inb = a0 >= g.min_b[0] && a0 <= g.max_b[0] && a1 >= g.min_b[1] && a1 <= g.max_b[1] && a2 >= g.min_b[2] && a2 <= g.max_b[2];
        vid[k] = inb ? g.cell2vox[(a0 - g.min_b[0]) + (a1 - g.min_b[1]) * g.mul1 + (a2 - g.min_b[2]) * g.mul2] : -1;
      }
    }

    // ---- fold the neighbourhood:  A = sum w C,  b = sum w C q,  M = sum w d2 (Cq)(Cq)^T,  score
    float N[6] = {0, 0, 0, 0, 0, 0}, b[3] = {0, 0, 0}, sc = 0.f;   // N = A - M, accumulated directly
    bool any = false;
#pragma unroll
    for (int k = 0; k < NB; k++) {
      if (vid[k] < 0) continue;
      if (SEARCH == DGS_NDT_KDTREE) {
        const float4 ce = g.centroid[vid[k]];
        const float ex = ce.x - xt0, ey = ce.y - xt1, ez = ce.z - xt2;
        if (!(ex * ex + ey * ey + ez * ez < r2)) continue;
      }
      const VoxelRec* __restrict__ rec = g.vox + vid[k];
      const float4* __restrict__ r4 = reinterpret_cast<const float4*>(rec);  // three aligned 16-B loads
      const double2 m01 = *reinterpret_cast<const double2*>(rec);
      const float4 rb = r4[1], rc = r4[2];
      const double mx = m01.x, my = m01.y;
      const double mz = __hiloint2double(__float_as_int(rb.y), __float_as_int(rb.x));
      const float q0 = (float)((double)xt0 - mx), q1 = (float)((double)xt1 - my), q2 = (float)((double)xt2 - mz);
      const float Cxx = rb.z, Cxy = rb.w, Cxz = rc.x, Cyy = rc.y, Cyz = rc.z, Czz = rc.w;
      const float u0 = q0 * Cxx + q1 * Cxy + q2 * Cxz;
      const float u1 = q0 * Cxy + q1 * Cyy + q2 * Cyz;
      const float u2 = q0 * Cxz + q1 * Cyz + q2 * Czz;
      // The library expf (<= 1 ulp).  Round 3 had put a 6-instruction hardware form here (v_exp_f32 of x * log2 e with the product's rounding error
      // folded back in, <= 2 ulp; 2 % of the step): on the bench shard it moved pair 20 of seed 40 to another optimum, 0.945 m from the reference's and
      // outside the reference's own 34-twin band (0.872 m) -- isolated in round 4 with A/B builds (profiles/r04/fast_order_variants.jsonl: the pair is
      // back inside the gate with expf or det_expf, whichever way N is accumulated) and reverted.  The A/B builds are removed; see history.
      float e = expf(-gd2 * (q0 * u0 + q1 * u1 + q2 * u2) * 0.5f);
      // gauss_d1 is a double upstream: float(double(e) * d1), not e * float(d1) -- the float constant alone would scale score,
      // gradient and Hessian by (1 + 2.8e-8) at 1 m resolution, which was the whole per-evaluation difference to a CPU run
      const float score_inc = (float)(-gd1 * (double)e);
      e = gd2 * e;
      if (e > 1.f || e < 0.f || e != e) continue;  // upstream "error checking for invalid values"
      const float w = (float)((double)e * gd1);
      sc += score_inc;
      any = true;
      b[0] += w * u0; b[1] += w * u1; b[2] += w * u2;
      if (need_h) {   // a score + gradient evaluation (a More-Thuente trial) needs neither A nor M: wave-uniform, a scalar branch
        const float wd = w * gd2, t0 = wd * u0, t1 = wd * u1, t2 = wd * u2;
        N[0] += w * Cxx; N[1] += w * Cxy; N[2] += w * Cxz; N[3] += w * Cyy; N[4] += w * Cyz; N[5] += w * Czz;
        N[0] -= t0 * u0; N[1] -= t0 * u1; N[2] -= t0 * u2; N[3] -= t1 * u1; N[4] -= t1 * u2; N[5] -= t2 * u2;
      }
    }
    if (!any) continue;

    // ---- project through the point Jacobian (eq. 6.18/6.19): J = [I | J3 J4 J5]
    // Rows 5..7 of the table have no z entry (computeAngleDerivatives writes exact zeros there), and the xy parts of rows 0 / 1 are kept:
    // the second-derivative rows f3 / f2 are exactly those (below).
    float xj[8];
    const float jxy0 = hdr.J(0, 0) * x.x + hdr.J(0, 1) * x.y, jxy1 = hdr.J(1, 0) * x.x + hdr.J(1, 1) * x.y;
    xj[0] = jxy0 + hdr.J(0, 2) * x.z;
    xj[1] = jxy1 + hdr.J(1, 2) * x.z;
#pragma unroll
    for (int k = 2; k < 5; k++) xj[k] = hdr.J(k, 0) * x.x + hdr.J(k, 1) * x.y + hdr.J(k, 2) * x.z;
#pragma unroll
    for (int k = 5; k < 8; k++) xj[k] = hdr.J(k, 0) * x.x + hdr.J(k, 1) * x.y;
    const float J3[3] = {0.f, xj[0], xj[1]}, J4[3] = {xj[2], xj[3], xj[4]}, J5[3] = {xj[5], xj[6], xj[7]};
    acc[0] += (double)sc;
    acc[1] += (double)b[0];
    acc[2] += (double)b[1];
    acc[3] += (double)b[2];
    acc[4] += (double)(b[1] * J3[1] + b[2] * J3[2]);
    acc[5] += (double)(b[0] * J4[0] + b[1] * J4[1] + b[2] * J4[2]);
    acc[6] += (double)(b[0] * J5[0] + b[1] * J5[1] + b[2] * J5[2]);
    if (need_h) {
      const float N0 = N[0], N1 = N[1], N2 = N[2], N3 = N[3], N4 = N[4], N5 = N[5];
      // N * J_k
      const float n3[3] = {N1 * J3[1] + N2 * J3[2], N3 * J3[1] + N4 * J3[2], N4 * J3[1] + N5 * J3[2]};
      const float n4[3] = {N0 * J4[0] + N1 * J4[1] + N2 * J4[2], N1 * J4[0] + N3 * J4[1] + N4 * J4[2], N2 * J4[0] + N4 * J4[1] + N5 * J4[2]};
      const float n5[3] = {N0 * J5[0] + N1 * J5[1] + N2 * J5[2], N1 * J5[0] + N3 * J5[1] + N4 * J5[2], N2 * J5[0] + N4 * J5[1] + N5 * J5[2]};
      // Of the fifteen second-derivative rows (eq. 6.21) nine are first-derivative rows (eq. 6.19) again, as computeAngleDerivatives
      // writes them -- the same double expressions or their exact negations, so the float entries are the same bits:
      //   a2 = -j1, a3 = j0, b2 = -j4, b3 = j3, c2 = -j7, c3 = j6;  f1 = xy part of d1, f2 = xy part of a2, f3 = xy part of a3;
      // e1..e3 (and c2, c3, f1..f3) have no z entry.  Same values as the full 15 x 3 products, 30 instructions fewer per point.
      float xh[15];
      xh[0] = -xj[1]; xh[1] = xj[0]; xh[2] = -xj[4]; xh[3] = xj[3]; xh[4] = -xj[7]; xh[5] = xj[6];
      const float hxy6 = hdr.H(6, 0) * x.x + hdr.H(6, 1) * x.y;
      xh[6] = hxy6 + hdr.H(6, 2) * x.z;
#pragma unroll
      for (int k = 7; k < 9; k++) xh[k] = hdr.H(k, 0) * x.x + hdr.H(k, 1) * x.y + hdr.H(k, 2) * x.z;
#pragma unroll
      for (int k = 9; k < 12; k++) xh[k] = hdr.H(k, 0) * x.x + hdr.H(k, 1) * x.y;
      xh[12] = hxy6; xh[13] = -jxy1; xh[14] = jxy0;
      // b . second derivatives: a=(0,xh0,xh1) b=(0,xh2,xh3) c=(0,xh4,xh5) d=(xh6..8) e=(xh9..11) f=(xh12..14)
      const float ba = b[1] * xh[0] + b[2] * xh[1];
      const float bb = b[1] * xh[2] + b[2] * xh[3];
      const float bc = b[1] * xh[4] + b[2] * xh[5];
      const float bd = b[0] * xh[6] + b[1] * xh[7] + b[2] * xh[8];
      const float be = b[0] * xh[9] + b[1] * xh[10] + b[2] * xh[11];
      const float bf = b[0] * xh[12] + b[1] * xh[13] + b[2] * xh[14];
      // upper triangle, row-major: (0,0..5) (1,1..5) (2,2..5) (3,3..5) (4,4..5) (5,5)
      acc[7] += (double)N0;  acc[8] += (double)N1;  acc[9] += (double)N2;  acc[10] += (double)n3[0]; acc[11] += (double)n4[0]; acc[12] += (double)n5[0];
      acc[13] += (double)N3; acc[14] += (double)N4; acc[15] += (double)n3[1]; acc[16] += (double)n4[1]; acc[17] += (double)n5[1];
      acc[18] += (double)N5; acc[19] += (double)n3[2]; acc[20] += (double)n4[2]; acc[21] += (double)n5[2];
      acc[22] += (double)(J3[1] * n3[1] + J3[2] * n3[2] + ba);
      acc[23] += (double)(J3[1] * n4[1] + J3[2] * n4[2] + bb);
      acc[24] += (double)(J3[1] * n5[1] + J3[2] * n5[2] + bc);
      acc[25] += (double)(J4[0] * n4[0] + J4[1] * n4[1] + J4[2] * n4[2] + bd);
      acc[26] += (double)(J4[0] * n5[0] + J4[1] * n5[1] + J4[2] * n5[2] + be);
      acc[27] += (double)(J5[0] * n5[0] + J5[1] * n5[1] + J5[2] * n5[2] + bf);
    }
  }
}

// Block reduction of the 28 per-thread totals into one row.  A DPP butterfly over 28 doubles costs ~900 wave-instructions; instead
// every wave transposes through LDS, 14 values at a time: lane l stores value k at row k (stride 65 doubles: conflict-free both
// ways), then lane k adds the 64 entries of row k in lane order (fixed order -> reproducible).  ~290 wave-instructions.
// COHERENT: the row is handed over inside the launch (common.h, "in-launch hand-off"): write-through stores.
template <bool COHERENT>
__device__ __forceinline__ void ndt_block_row(const double (&acc)[kAccum], double* __restrict__ row_of_slice) {
  constexpr int HALF = kAccum / 2, RS = 65;
  __shared__ double tr[kBlock / kWave][HALF * RS];
  __shared__ double sm[kBlock / kWave][kAccumPad];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  double* my = tr[wave];
#pragma unroll
  for (int h = 0; h < 2; h++) {
#pragma unroll
    for (int k = 0; k < HALF; k++) my[k * RS + lane] = acc[h * HALF + k];
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0): this wave's LDS writes have landed
    if (lane < HALF) {
      double v = 0.0;
#pragma unroll 8
      for (int j = 0; j < 64; j++) v += my[lane * RS + j];
      sm[wave][h * HALF + lane] = v;
    }
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_s_waitcnt(0xc07f);
  }
  __syncthreads();
  if (threadIdx.x < kAccumPad) {
    double v = 0.0;
    if (threadIdx.x < kAccum) v = ((sm[0][threadIdx.x] + sm[1][threadIdx.x]) + sm[2][threadIdx.x]) + sm[3][threadIdx.x];
    double* row = row_of_slice + threadIdx.x;
    if (COHERENT) handoff_store_row(row, v);   // write-through (sc1): no release fence needed
    else *row = v;
  }
}

typedef float v2f __attribute__((ext_vector_type(2)));
__device__ __forceinline__ v2f affine_row_rn2(float m0, float m1, float m2, float m3, v2f x, v2f y, v2f z) {
#pragma clang fp contract(off)
  return ((m0 * x + m1 * y) + m2 * z) + m3;   // v_pk_mul_f32 / v_pk_add_f32: every element individually rounded, as affine_row_rn
}

// PACK2 (instantiated in the EXPERIMENTS build only: measured 29-46 % slower): two source points per lane and step, the float fold and projection written on 2-vectors so that they compile to
// v_pk_fma_f32 / v_pk_mul_f32 / v_pk_add_f32 (two points per instruction); look-ups, the double q = x' - mean, exp and the
// double accumulation stay per point.  The per-thread order of accumulation is unchanged (i, i + stride, i + 2 stride, ...).
template <int SEARCH, bool FUSED, bool PACK2>
__global__ __launch_bounds__(kBlock, PACK2 ? 2 : 4) void ndt_derivatives_kernel(const float4* const* __restrict__ src_ptrs, const int* __restrict__ src_sizes,
                                                                    NdtPair* __restrict__ pairs, const VoxelGrid g, const double gd1,
                                                                    const float gd2, const int leaf_pow2, double* __restrict__ partials,
                                                                    const int n_pairs, const int cap_blocks, int* __restrict__ pair_blocks,
                                                                    const NdtConsts consts, int* __restrict__ done_counter, const int launch) {
  // ---- map this workgroup to (still-active pair, slice).  The launch always has gridDim.x workgroups; they are dealt
  // evenly to the pairs that are still iterating, so a batch whose pairs converge at different iterations keeps the chip
  // busy on the stragglers instead of spinning up empty blocks.  Every wave derives the same mapping from the pairs'
  // `active` words (written by the previous solve launch): one strided load + ballot per 64 pairs, no inter-block traffic.
  const int lane_id = threadIdx.x & 63;
  int n_active = 0;
  for (int c0 = 0; c0 < n_pairs; c0 += 64) {
    const int pi = c0 + lane_id;
    const int a = (pi < n_pairs) ? (FUSED ? (int)(launch <= pairs[pi].last_launch) : pairs[pi].active) : 0;
    n_active += __popcll(__ballot(a != 0));
  }
  if (n_active == 0) return;
  const int blocks_per_pair = min((int)gridDim.x / n_active, cap_blocks);
  const int rank = blockIdx.x / blocks_per_pair, slice = blockIdx.x % blocks_per_pair;
  if (rank >= n_active) return;
  int pair = -1;
  {
    int seen = 0;
    for (int c0 = 0; c0 < n_pairs && pair < 0; c0 += 64) {
      const int pi = c0 + lane_id;
      const int a = (pi < n_pairs) ? (FUSED ? (int)(launch <= pairs[pi].last_launch) : pairs[pi].active) : 0;
      unsigned long long m = __ballot(a != 0);
      const int cnt = __popcll(m);
      if (rank < seen + cnt) {
        for (int k = rank - seen; k > 0; k--) m &= m - 1ull;  // drop the (rank - seen) lowest set bits
        pair = c0 + __ffsll((long long)m) - 1;
      }
      seen += cnt;
    }
  }
  pair = __builtin_amdgcn_readfirstlane(pair);
  if (slice == 0 && threadIdx.x == 0) pair_blocks[pair] = blocks_per_pair;
  const NdtPair& st = pairs[pair];
  const float4* __restrict__ src = src_ptrs[pair];
  const int n = src_sizes[pair];
  const bool need_h = st.need_hessian != 0;

  float T[12];
#pragma unroll
  for (int k = 0; k < 12; k++) T[k] = st.T[k];

  double acc[kAccum];
#pragma unroll
  for (int k = 0; k < kAccum; k++) acc[k] = 0.0;

  if constexpr (PACK2 && SEARCH == DGS_NDT_DIRECT7) {
    constexpr int NB = 7;
    const int stride = blocks_per_pair * kBlock;
    for (int i = slice * kBlock + threadIdx.x; i < n; i += 2 * stride) {
      const int ib = i + stride;
      const bool hb = ib < n;
      const float4 xa = src[i], xb = src[hb ? ib : i];
      v2f X = {xa.x, xb.x}, Y = {xa.y, xb.y}, Z = {xa.z, xb.z};
      const v2f xt0 = affine_row_rn2(T[0], T[1], T[2], T[3], X, Y, Z);
      const v2f xt1 = affine_row_rn2(T[4], T[5], T[6], T[7], X, Y, Z);
      const v2f xt2 = affine_row_rn2(T[8], T[9], T[10], T[11], X, Y, Z);
      int vid[2][NB];
#pragma unroll
      for (int p = 0; p < 2; p++) {
        const float a0 = p ? xt0.y : xt0.x, a1 = p ? xt1.y : xt1.x, a2 = p ? xt2.y : xt2.x;
        const int c0 = (int)floorf(leaf_pow2 ? a0 * g.inv_leaf : a0 / g.leaf);
        const int c1 = (int)floorf(leaf_pow2 ? a1 * g.inv_leaf : a1 / g.leaf);
        const int c2 = (int)floorf(leaf_pow2 ? a2 * g.inv_leaf : a2 / g.leaf);
        const bool interior = c0 > g.min_b[0] && c0 < g.max_b[0] && c1 > g.min_b[1] && c1 < g.max_b[1] && c2 > g.min_b[2] && c2 < g.max_b[2];
        if (interior && (p == 0 || hb)) {
          const int* __restrict__ base = g.cell2vox + ((c0 - g.min_b[0]) + (c1 - g.min_b[1]) * g.mul1 + (c2 - g.min_b[2]) * g.mul2);
#pragma unroll
          for (int k = 0; k < NB; k++) {
            int dx, dy, dz;
            neighbour_offset<SEARCH>(k, dx, dy, dz);
            vid[p][k] = base[dx + dy * g.mul1 + dz * g.mul2];
          }
        } else {
#pragma unroll
          for (int k = 0; k < NB; k++) {
            int dx, dy, dz;
            neighbour_offset<SEARCH>(k, dx, dy, dz);
            const int b0 = c0 + dx, b1 = c1 + dy, b2 = c2 + dz;
            const bool inb = (p == 0 || hb) && b0 >= g.min_b[0] && b0 <= g.max_b[0] && b1 >= g.min_b[1] && b1 <= g.max_b[1] && b2 >= g.min_b[2] && b2 <= g.max_b[2];
            vid[p][k] = inb ? g.cell2vox[(b0 - g.min_b[0]) + (b1 - g.min_b[1]) * g.mul1 + (b2 - g.min_b[2]) * g.mul2] : -1;
          }
        }
      }
      v2f A[6], M[6], b[3], sc = {0.f, 0.f};
#pragma unroll
      for (int k = 0; k < 6; k++) { A[k] = (v2f){0.f, 0.f}; M[k] = (v2f){0.f, 0.f}; }
#pragma unroll
      for (int k = 0; k < 3; k++) b[k] = (v2f){0.f, 0.f};
      bool any_a = false, any_b = false;
#pragma unroll
      for (int k = 0; k < NB; k++) {
        const int va = vid[0][k], vb = vid[1][k];
        if (va < 0 && vb < 0) continue;
        const float4* __restrict__ ra4 = reinterpret_cast<const float4*>(g.vox + max(va, 0));
        const float4* __restrict__ rb4 = reinterpret_cast<const float4*>(g.vox + max(vb, 0));
        const float4 a0 = ra4[0], a1 = ra4[1], a2 = ra4[2], b0 = rb4[0], b1 = rb4[1], b2 = rb4[2];
        const double mxa = __hiloint2double(__float_as_int(a0.y), __float_as_int(a0.x)), mya = __hiloint2double(__float_as_int(a0.w), __float_as_int(a0.z)),
                     mza = __hiloint2double(__float_as_int(a1.y), __float_as_int(a1.x));
        const double mxb = __hiloint2double(__float_as_int(b0.y), __float_as_int(b0.x)), myb = __hiloint2double(__float_as_int(b0.w), __float_as_int(b0.z)),
                     mzb = __hiloint2double(__float_as_int(b1.y), __float_as_int(b1.x));
        // a voxel slot that is missing for one of the two points contributes exact zeros for it (q = 0 -> u = 0, w = 0)
        const v2f q0 = {va >= 0 ? (float)((double)xt0.x - mxa) : 0.f, vb >= 0 ? (float)((double)xt0.y - mxb) : 0.f};
        const v2f q1 = {va >= 0 ? (float)((double)xt1.x - mya) : 0.f, vb >= 0 ? (float)((double)xt1.y - myb) : 0.f};
        const v2f q2 = {va >= 0 ? (float)((double)xt2.x - mza) : 0.f, vb >= 0 ? (float)((double)xt2.y - mzb) : 0.f};
        const v2f Cxx = {a1.z, b1.z}, Cxy = {a1.w, b1.w}, Cxz = {a2.x, b2.x}, Cyy = {a2.y, b2.y}, Cyz = {a2.z, b2.z}, Czz = {a2.w, b2.w};
        const v2f u0 = q0 * Cxx + q1 * Cxy + q2 * Cxz;
        const v2f u1 = q0 * Cxy + q1 * Cyy + q2 * Cyz;
        const v2f u2 = q0 * Cxz + q1 * Cyz + q2 * Czz;
        const v2f arg = -gd2 * (q0 * u0 + q1 * u1 + q2 * u2) * 0.5f;
        v2f e = {expf(arg.x), expf(arg.y)};   // the library expf, as the default kernel (round 4)
        const float sia = (float)(-gd1 * (double)e.x), sib = (float)(-gd1 * (double)e.y);
        e = gd2 * e;
        const bool oka = va >= 0 && !(e.x > 1.f || e.x < 0.f || e.x != e.x), okb = vb >= 0 && !(e.y > 1.f || e.y < 0.f || e.y != e.y);
        const v2f w = {oka ? (float)((double)e.x * gd1) : 0.f, okb ? (float)((double)e.y * gd1) : 0.f};
        const v2f wd = w * gd2;
        sc += (v2f){oka ? sia : 0.f, okb ? sib : 0.f};
        any_a |= oka;
        any_b |= okb;
        b[0] += w * u0; b[1] += w * u1; b[2] += w * u2;
        A[0] += w * Cxx; A[1] += w * Cxy; A[2] += w * Cxz; A[3] += w * Cyy; A[4] += w * Cyz; A[5] += w * Czz;
        M[0] += wd * u0 * u0; M[1] += wd * u0 * u1; M[2] += wd * u0 * u2; M[3] += wd * u1 * u1; M[4] += wd * u1 * u2; M[5] += wd * u2 * u2;
      }
      if (!any_a && !any_b) continue;
      // a point without any contributing voxel projects exact zeros (also when its coordinates are not finite)
      if (!any_a) { X.x = 0.f; Y.x = 0.f; Z.x = 0.f; }
      if (!any_b) { X.y = 0.f; Y.y = 0.f; Z.y = 0.f; }
      v2f xj[8];
#pragma unroll
      for (int k = 0; k < 8; k++) xj[k] = st.jang[k][0] * X + st.jang[k][1] * Y + st.jang[k][2] * Z;
      const v2f g3 = b[1] * xj[0] + b[2] * xj[1];
      const v2f g4 = b[0] * xj[2] + b[1] * xj[3] + b[2] * xj[4];
      const v2f g5 = b[0] * xj[5] + b[1] * xj[6] + b[2] * xj[7];
#define DGS_ACC2(K, V) { const v2f v_ = (V); acc[K] += (double)v_.x; acc[K] += (double)v_.y; }
      DGS_ACC2(0, sc) DGS_ACC2(1, b[0]) DGS_ACC2(2, b[1]) DGS_ACC2(3, b[2]) DGS_ACC2(4, g3) DGS_ACC2(5, g4) DGS_ACC2(6, g5)
      if (need_h) {
        const v2f N0 = A[0] - M[0], N1 = A[1] - M[1], N2 = A[2] - M[2], N3 = A[3] - M[3], N4 = A[4] - M[4], N5 = A[5] - M[5];
        const v2f n30 = N1 * xj[0] + N2 * xj[1], n31 = N3 * xj[0] + N4 * xj[1], n32 = N4 * xj[0] + N5 * xj[1];
        const v2f n40 = N0 * xj[2] + N1 * xj[3] + N2 * xj[4], n41 = N1 * xj[2] + N3 * xj[3] + N4 * xj[4], n42 = N2 * xj[2] + N4 * xj[3] + N5 * xj[4];
        const v2f n50 = N0 * xj[5] + N1 * xj[6] + N2 * xj[7], n51 = N1 * xj[5] + N3 * xj[6] + N4 * xj[7], n52 = N2 * xj[5] + N4 * xj[6] + N5 * xj[7];
        v2f xh[15];
#pragma unroll
        for (int k = 0; k < 15; k++) xh[k] = st.hang[k][0] * X + st.hang[k][1] * Y + st.hang[k][2] * Z;
        const v2f ba = b[1] * xh[0] + b[2] * xh[1], bb = b[1] * xh[2] + b[2] * xh[3], bc = b[1] * xh[4] + b[2] * xh[5];
        const v2f bd = b[0] * xh[6] + b[1] * xh[7] + b[2] * xh[8], be = b[0] * xh[9] + b[1] * xh[10] + b[2] * xh[11];
        const v2f bf = b[0] * xh[12] + b[1] * xh[13] + b[2] * xh[14];
        DGS_ACC2(7, N0) DGS_ACC2(8, N1) DGS_ACC2(9, N2) DGS_ACC2(10, n30) DGS_ACC2(11, n40) DGS_ACC2(12, n50)
        DGS_ACC2(13, N3) DGS_ACC2(14, N4) DGS_ACC2(15, n31) DGS_ACC2(16, n41) DGS_ACC2(17, n51)
        DGS_ACC2(18, N5) DGS_ACC2(19, n32) DGS_ACC2(20, n42) DGS_ACC2(21, n52)
        DGS_ACC2(22, xj[0] * n31 + xj[1] * n32 + ba)
        DGS_ACC2(23, xj[0] * n41 + xj[1] * n42 + bb)
        DGS_ACC2(24, xj[0] * n51 + xj[1] * n52 + bc)
        DGS_ACC2(25, xj[2] * n40 + xj[3] * n41 + xj[4] * n42 + bd)
        DGS_ACC2(26, xj[2] * n50 + xj[3] * n51 + xj[4] * n52 + be)
        DGS_ACC2(27, xj[5] * n50 + xj[6] * n51 + xj[7] * n52 + bf)
      }
#undef DGS_ACC2
    }
  } else
  {
    ndt_point_loop<SEARCH>(T, NdtHdrGlobal{st}, need_h, src, n, slice * kBlock + (int)threadIdx.x, blocks_per_pair * kBlock, g, gd1, gd2, leaf_pow2, acc);
  }

  ndt_block_row<FUSED>(acc, partials + ((size_t)pair * cap_blocks + slice) * kAccumPad);
  if (!FUSED) return;
  // ---- publish this slice's row, take a ticket; the workgroup that takes the pair's last ticket closes the evaluation
  __shared__ int s_last;
  if (threadIdx.x < kAccumPad) handoff_drain_stores();   // the storing wave drains its stores
  __syncthreads();
  if (threadIdx.x == 0) s_last = handoff_take_ticket(&pairs[pair].ticket, blocks_per_pair) ? 1 : 0;
  __syncthreads();
  if (!s_last) return;
#ifdef DGS_CLOSE_STAMPS
  if (threadIdx.x == 0 && pairs[pair].s.nr_iterations == 1) pairs[pair].traj[kTrajCap - 1][5] = (double)wall_clock64();
#endif
  ndt_close_evaluation<false, true>(pairs + pair, partials + (size_t)pair * cap_blocks * kAccumPad, blocks_per_pair, consts, done_counter + pair, launch);
}
