// ndt_strict_order 2 (UPSTREAM_SEQUENTIAL): round 2's lane-per-point validation kernel writing per-point totals to HBM, and the
// index-order sum over them.  Included by ndt_align.hip inside namespace dgs, below ndt_strict.h (strict_point_hd, strict_gather)
// and ndt_exp_tables.h, with floating-point contraction off.

// ================================================================================================ validation modes
// dgs_params.ndt_strict_order >= 1: computeDerivatives / updateDerivatives in upstream's own operation order (SURVEY.md App. A
// "Per point"; the CPU checker states the same sequence).  Per point: float point gradient (3x6) and second-derivative
// vectors, then per neighbour voxel q = float(double(x') - mean), C = float(icov) (all 9 entries: after the eigenvalue clamp
// the covariance is rebuilt as V diag V^-1 and is not exactly symmetric), q^T C, exp, the float 3x6 product C * J, the float
// gradient / Hessian increments, each converted and added to the point's DOUBLE totals.  One point -> 43 doubles.
// LITERAL = false (default): the same values with upstream's structural zeros and ones not multiplied out -- the point gradient
// is [I | J3 J4 J5] with a zero in J3's first row, the point Hessian is zero outside its 3x3 rotational block: 1 * a, a + 0 and
// 0 * a are exact whenever a is finite, so C * J, x^T C H and J^T C J shrink from ~800 to ~450 float operations per voxel and the
// register copy of the 6x6x3 point Hessian to its 6 distinct vectors.  Every operation that remains is upstream's, in upstream's
// order.  Bit-identical to LITERAL = true (DGS_NDT_STRICT_LITERAL=1; test_strict_gpu.py::test_structural_zero_shortcuts_are_bit_identical)
// as long as the float products stay finite; where one overflows upstream turns 0 * inf into NaN and this path keeps inf -- both
// end in a non-finite Hessian and a failed registration.
template <int SEARCH, bool LITERAL>
__device__ __forceinline__ void ndt_point_strict(const float4 x, const float* T, const NdtPair& st, const VoxelGrid& g, const double* __restrict__ vtab,
                                                 const double gauss_d1, const float gd2, const int leaf_pow2, const bool need_h, double* out, const bool exp_libm) {
#pragma unroll
  for (int k = 0; k < kStrictAccum; k++) out[k] = 0.0;
  float xt[3];
  xt[0] = affine_row_rn(T[0], T[1], T[2], T[3], x.x, x.y, x.z);
  xt[1] = affine_row_rn(T[4], T[5], T[6], T[7], x.x, x.y, x.z);
  xt[2] = affine_row_rn(T[8], T[9], T[10], T[11], x.x, x.y, x.z);
  const int c0 = (int)floorf(leaf_pow2 ? xt[0] * g.inv_leaf : xt[0] / g.leaf);
  const int c1 = (int)floorf(leaf_pow2 ? xt[1] * g.inv_leaf : xt[1] / g.leaf);
  const int c2 = (int)floorf(leaf_pow2 ? xt[2] * g.inv_leaf : xt[2] / g.leaf);
  constexpr int NB = Offsets<SEARCH>::N;
  const float r2 = g.leaf * g.leaf;
  // computePointDerivatives
  const float xp[3] = {x.x, x.y, x.z};
  float pg[3][6] = {{1, 0, 0, 0, 0, 0}, {0, 1, 0, 0, 0, 0}, {0, 0, 1, 0, 0, 0}};
  float xj[8];
#pragma unroll
  for (int i = 0; i < 8; i++) xj[i] = st.jang[i][0] * xp[0] + st.jang[i][1] * xp[1] + st.jang[i][2] * xp[2];
  pg[1][3] = xj[0]; pg[2][3] = xj[1];
  pg[0][4] = xj[2]; pg[1][4] = xj[3]; pg[2][4] = xj[4];
  pg[0][5] = xj[5]; pg[1][5] = xj[6]; pg[2][5] = xj[7];
  // the 6 distinct vectors of the point Hessian's rotational block: (3,3) (3,4) (3,5) (4,4) (4,5) (5,5); zero without a Hessian
  float hv[6][3];
#pragma unroll
  for (int i = 0; i < 6; i++) hv[i][0] = hv[i][1] = hv[i][2] = 0.f;
  if (need_h) {
    float xh[15];
#pragma unroll
    for (int i = 0; i < 15; i++) xh[i] = st.hang[i][0] * xp[0] + st.hang[i][1] * xp[1] + st.hang[i][2] * xp[2];
    hv[0][1] = xh[0]; hv[0][2] = xh[1];     // a = (0, xh0, xh1)
    hv[1][1] = xh[2]; hv[1][2] = xh[3];     // b
    hv[2][1] = xh[4]; hv[2][2] = xh[5];     // c
    hv[3][0] = xh[6]; hv[3][1] = xh[7]; hv[3][2] = xh[8];       // d
    hv[4][0] = xh[9]; hv[4][1] = xh[10]; hv[4][2] = xh[11];     // e
    hv[5][0] = xh[12]; hv[5][1] = xh[13]; hv[5][2] = xh[14];    // f
  }
  // (i, j) of the rotational block -> its vector
  auto hvec = [&](int i, int j) -> const float* {
    const int lo = (i < j ? i : j) - 3, hi = (i < j ? j : i) - 3;
    return hv[lo == 0 ? hi : (lo == 1 ? 2 + hi : 5)];
  };
  double score_pt = 0.0, g_pt[6] = {0, 0, 0, 0, 0, 0}, h_pt[36];
#pragma unroll
  for (int k = 0; k < 36; k++) h_pt[k] = 0.0;
  // the neighbourhood's voxel ids first (independent loads, issued together): at 2 waves per SIMD (172 VGPRs are the double totals of
  // the point and of the thread) little else hides the table's latency.  (Loading the next voxel's record one iteration ahead was
  // tried: 24 more live registers, 1 wave per SIMD, 15 -> 19.7 ms per step.)
  int vids[NB];
#pragma unroll
  for (int k = 0; k < NB; k++) {
    int dx, dy, dz;
    neighbour_offset<SEARCH>(k, dx, dy, dz);
    const int a0 = c0 + dx, a1 = c1 + dy, a2 = c2 + dz;
    const bool inb = a0 >= g.min_b[0] && a0 <= g.max_b[0] && a1 >= g.min_b[1] && a1 <= g.max_b[1] && a2 >= g.min_b[2] && a2 <= g.max_b[2];
    vids[k] = inb ? g.cell2vox[(a0 - g.min_b[0]) + (a1 - g.min_b[1]) * g.mul1 + (a2 - g.min_b[2]) * g.mul2] : -1;
  }
  if (SEARCH == DGS_NDT_KDTREE) {
#pragma unroll
    for (int k = 0; k < NB; k++) {
      if (vids[k] < 0) continue;
      const float4 ce = g.centroid[vids[k]];
      const float ex = ce.x - xt[0], ey = ce.y - xt[1], ez = ce.z - xt[2];
      if (!(ex * ex + ey * ey + ez * ez < r2)) vids[k] = -1;
    }
  }
#pragma unroll 1
  for (int k = 0; k < NB; k++) {
    int vid = vids[0];   // vids stays in registers: a dynamic subscript is a chain of selects, not scratch memory
#pragma unroll
    for (int j = 1; j < NB; j++) vid = (k == j) ? vids[j] : vid;
    if (vid < 0) continue;
    const double* __restrict__ rec = vtab + (size_t)vid * 12;  // mean[3], icov[9] (row-major), double
    float q[3], C[3][3];
#pragma unroll
    for (int r = 0; r < 3; r++) q[r] = (float)((double)xt[r] - rec[r]);
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
      for (int c = 0; c < 3; c++) C[r][c] = (float)rec[3 + r * 3 + c];
    float qC[3];
#pragma unroll
    for (int c = 0; c < 3; c++) qC[c] = q[0] * C[0][c] + q[1] * C[1][c] + q[2] * C[2][c];
    const float e_arg = -gd2 * (q[0] * qC[0] + q[1] * qC[1] + q[2] * qC[2]) * 0.5f;
    float e_x_cov_x = exp_libm ? glibc_expf_dev(e_arg, kGlibcExp2fTab) : det_expf(e_arg);
    const float score_inc = (float)(-gauss_d1 * (double)e_x_cov_x);
    e_x_cov_x = gd2 * e_x_cov_x;
    if (e_x_cov_x > 1 || e_x_cov_x < 0 || e_x_cov_x != e_x_cov_x) continue;
    e_x_cov_x = (float)((double)e_x_cov_x * gauss_d1);
    float cPG[3][6];
    float g6[6];
    constexpr bool literal = LITERAL;
    if (!LITERAL) {
#pragma unroll
      for (int r = 0; r < 3; r++) {
        cPG[r][0] = C[r][0]; cPG[r][1] = C[r][1]; cPG[r][2] = C[r][2];            // C * (unit column): exact
        cPG[r][3] = C[r][1] * pg[1][3] + C[r][2] * pg[2][3];                      // (C0 * 0 + m1) + m2
#pragma unroll
        for (int c = 4; c < 6; c++) cPG[r][c] = C[r][0] * pg[0][c] + C[r][1] * pg[1][c] + C[r][2] * pg[2][c];
      }
    } else {
#pragma unroll
      for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = 0; c < 6; c++) cPG[r][c] = C[r][0] * pg[0][c] + C[r][1] * pg[1][c] + C[r][2] * pg[2][c];
    }
#pragma unroll
    for (int c = 0; c < 6; c++) g6[c] = q[0] * cPG[0][c] + q[1] * cPG[1][c] + q[2] * cPG[2][c];
#pragma unroll
    for (int c = 0; c < 6; c++) g_pt[c] += (double)(e_x_cov_x * g6[c]);
    if (need_h) {
      if (literal) {
#pragma unroll
        for (int i = 0; i < 6; i++)
#pragma unroll
          for (int j = 0; j < 6; j++) {
            float xCH = qC[0] * 0.f + qC[1] * 0.f + qC[2] * 0.f;
            if (i >= 3 && j >= 3) {
              const float* v = hvec(i, j);
              xCH = qC[0] * v[0] + qC[1] * v[1] + qC[2] * v[2];
            }
            const float pcp = pg[0][j] * cPG[0][i] + pg[1][j] * cPG[1][i] + pg[2][j] * cPG[2][i];
            h_pt[i * 6 + j] += (double)(e_x_cov_x * (-gd2 * g6[i] * g6[j] + xCH + pcp));
          }
      } else {
        float xch[6];   // x^T C H for the 6 distinct vectors
#pragma unroll
        for (int v = 0; v < 6; v++) xch[v] = qC[0] * hv[v][0] + qC[1] * hv[v][1] + qC[2] * hv[v][2];
#pragma unroll
        for (int i = 0; i < 6; i++)
#pragma unroll
          for (int j = 0; j < 6; j++) {
            float t = -gd2 * g6[i] * g6[j];
            if (i >= 3 && j >= 3) {
              const int lo = (i < j ? i : j) - 3, hi = (i < j ? j : i) - 3;
              t = t + xch[lo == 0 ? hi : (lo == 1 ? 2 + hi : 5)];
            }
            // J^T C J: column j of J is a unit vector for j < 3, has a zero first entry for j == 3
            const float pcp = (j < 3) ? cPG[j][i] : (j == 3) ? (pg[1][3] * cPG[1][i] + pg[2][3] * cPG[2][i]) : (pg[0][j] * cPG[0][i] + pg[1][j] * cPG[1][i] + pg[2][j] * cPG[2][i]);
            h_pt[i * 6 + j] += (double)(e_x_cov_x * (t + pcp));
          }
      }
    }
    score_pt += (double)score_inc;
  }
  out[0] = score_pt;
#pragma unroll
  for (int k = 0; k < 6; k++) out[1 + k] = g_pt[k];
#pragma unroll
  for (int k = 0; k < 36; k++) out[7 + k] = h_pt[k];
}

// Round 2's validation kernel, kept for ndt_strict_order 2 (ROWS = true; order 1 runs ndt_strict_kernel, ndt_strict.h).  ROWS = false:
// per-thread double totals over a strided set of points, block sums in a fixed order, one 48-double row per workgroup.  ROWS = true: the 43 per-point totals go to HBM, column-major per pair
// ([43][max_n]), for the sequential index-order sum of ndt_strict_seqsum_kernel.
template <int SEARCH, bool ROWS, bool LITERAL>
__global__ __launch_bounds__(kBlock, 2) void ndt_derivatives_strict_kernel(const float4* const* __restrict__ src_ptrs, const int* __restrict__ src_sizes,
                                                                        const NdtPair* __restrict__ pairs, const VoxelGrid g,
                                                                        const double* __restrict__ vtab, const double gauss_d1, const float gd2,
                                                                        const int leaf_pow2, double* __restrict__ partials, double* __restrict__ rows,
                                                                        const int max_n, const int n_pairs, const int cap_blocks,
                                                                        int* __restrict__ pair_blocks, const double gauss_d2, const size_t rows_pair_stride, const int exp_libm) {
  int pair, slice, blocks_per_pair;
  if (!deal_workgroup(n_pairs, cap_blocks, [&](int pi) { return pairs[pi].active != 0; }, pair, slice, blocks_per_pair)) return;
  if (slice == 0 && threadIdx.x == 0) pair_blocks[pair] = blocks_per_pair;
  const NdtPair& st = pairs[pair];
  const float4* __restrict__ src = src_ptrs[pair];
  const int n = src_sizes[pair];
  const bool need_h = st.need_hessian != 0;
  float T[12];
#pragma unroll
  for (int k = 0; k < 12; k++) T[k] = st.T[k];
  double acc[kStrictAccum];
#pragma unroll
  for (int k = 0; k < kStrictAccum; k++) acc[k] = 0.0;
  const int ncol = need_h ? kStrictAccum : 7;
  if (ROWS && st.need_hessian == 2) {
    // computeHessian in PCL's double form (evaluation kind 2): every (point, voxel) term to HBM, entry-major [36][n * NB], for the
    // sequential sum in upstream's order (ndt_strict_seqsum_kernel)
    constexpr int NB = Offsets<SEARCH>::N;
    const size_t row_stride = (size_t)max_n * NB;
    for (int i = slice * kBlock + threadIdx.x; i < n; i += blocks_per_pair * kBlock) {
      const float4 x = src[i];
      float xt[3];
      xt[0] = affine_row_rn(T[0], T[1], T[2], T[3], x.x, x.y, x.z);
      xt[1] = affine_row_rn(T[4], T[5], T[6], T[7], x.x, x.y, x.z);
      xt[2] = affine_row_rn(T[8], T[9], T[10], T[11], x.x, x.y, x.z);
      int vids[NB];
      const unsigned mask = strict_neighbourhood<SEARCH>(xt, g, leaf_pow2, vids);
      strict_point_hd<SEARCH, true>(x, xt, vids, mask, st, vtab, gauss_d1, gauss_d2, acc, rows + (size_t)pair * rows_pair_stride + (size_t)i * NB, row_stride, exp_libm ? kGlibcExpTab : nullptr);
    }
    return;
  }
  for (int i = slice * kBlock + threadIdx.x; i < n; i += blocks_per_pair * kBlock) {
    double o[kStrictAccum];
    ndt_point_strict<SEARCH, LITERAL>(src[i], T, st, g, vtab, gauss_d1, gd2, leaf_pow2, need_h, o, exp_libm != 0);
    if (ROWS) {
      double* __restrict__ col = rows + (size_t)pair * rows_pair_stride + i;
      for (int k = 0; k < ncol; k++) col[(size_t)k * max_n] = o[k];
    } else {
#pragma unroll
      for (int k = 0; k < kStrictAccum; k++) acc[k] += o[k];
    }
  }
  if (ROWS) return;
  __shared__ double sm[kBlock / kWave][kStrictPad];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < kStrictAccum; k++) {
    const double v = wave_sum(acc[k]);
    if (lane == 0) sm[wave][k] = v;
  }
  __syncthreads();
  if (threadIdx.x < kStrictPad) {
    double v = 0.0;
    if (threadIdx.x < kStrictAccum) v = ((sm[0][threadIdx.x] + sm[1][threadIdx.x]) + sm[2][threadIdx.x]) + sm[3][threadIdx.x];
    partials[((size_t)pair * cap_blocks + slice) * kStrictPad + threadIdx.x] = v;
  }
}

// ndt_strict_order 2: upstream's final loop -- score / gradient / Hessian entries summed over the points in index order, one
// lane per entry (a dependent chain of n double additions: this mode exists to prove bit-parity, not to be fast)
__global__ __launch_bounds__(kWave) void ndt_strict_seqsum_kernel(const NdtPair* __restrict__ pairs, const int* __restrict__ src_sizes,
                                                                  const double* __restrict__ rows, const int max_n, double* __restrict__ totals,
                                                                  const size_t rows_pair_stride, const int nb_slots) {
  const int pair = blockIdx.x;
  const NdtPair& st = pairs[pair];
  if (!st.active) return;
  const int c = threadIdx.x;
  if (c >= kStrictPad) return;
  if (st.need_hessian == 2) {
    // computeHessian (kind 2): the Hessian entries alone, every (point, voxel slot) term in upstream's order
    double v = 0.0;
    if (c >= 7 && c < kStrictAccum) {
      const size_t n = (size_t)src_sizes[pair] * nb_slots;
      const double* __restrict__ col = rows + (size_t)pair * rows_pair_stride + (size_t)(c - 7) * ((size_t)max_n * nb_slots);
      size_t i = 0;
      for (; i + 8 <= n; i += 8) {
        double t[8];
#pragma unroll
        for (int u = 0; u < 8; u++) t[u] = col[i + u];
#pragma unroll
        for (int u = 0; u < 8; u++) v += t[u];
      }
      for (; i < n; i++) v += col[i];
    }
    totals[(size_t)pair * kStrictPad + c] = v;
    return;
  }
  const int ncol = st.need_hessian ? kStrictAccum : 7;
  double v = 0.0;
  if (c < ncol) {
    const int n = src_sizes[pair];
    const double* __restrict__ col = rows + (size_t)pair * rows_pair_stride + (size_t)c * max_n;
    int i = 0;
    for (; i + 8 <= n; i += 8) {
      double t[8];
#pragma unroll
      for (int u = 0; u < 8; u++) t[u] = col[i + u];
#pragma unroll
      for (int u = 0; u < 8; u++) v += t[u];
    }
    for (; i < n; i++) v += col[i];
  }
  totals[(size_t)pair * kStrictPad + c] = v;
}
