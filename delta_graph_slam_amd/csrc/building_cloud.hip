// interpolate (upstream src/hdl_graph_slam/ros_utils.cpp:146-165) over many lines at once, with Building::getCloud's
// pcl::transformPointCloud (building.cpp:17-19) folded in: BuildingTools::buildPointCloud's clouds, the aligned / not-aligned line
// clouds of a frame and the buildings' clouds of an optimisation tick, each as one call.
//
// MI355X design
//   * Point k of every line sits at the same i_k (the k-fold float sum of sample_step), so one table of i_k on the handle
//     (building_cloud.h StepTable, made on the host and uploaded where it grew) turns a line's point count into an upper bound search
//     and makes every point independent of the others.
//   * bc_count_kernel, one lane per line: the float conversions, normalized() and norm() as Eigen 3.3 forms them, the search in the
//     table, and the lowest line that cannot be served (atomicMin; the only atomic of the stage).
//   * compact.h's pf_scan_kernel scans the counts in place into line offsets and leaves the total beside the error word: one 8-byte
//     read-back, the stage's one host wait, sizes the output.
//   * bc_fill_kernel: a workgroup owns DGS_BC_TILE consecutive output points.  One search in the line offsets finds the line that owns
//     its first point; from there it walks forward in chunks of kBlock lines staged in LDS (offset, a, dn, the item's matrix).  A lane
//     finds its point's line in the LDS offsets, reads i_k from the table and writes one whole 16-byte point; lanes of a wave write
//     consecutive addresses.  No atomics, no per-point search in global memory.  The same launch gathers the items' point offsets.
// Semantics and the Eigen / PCL details recalled from upstream: DESIGN.md §6m.
#include <climits>
#include <cmath>
#include <cstring>

#include "building_cloud.h"
#include "compact.h"
#include "handle.h"

namespace dgs {

constexpr int kBcTile = DGS_BC_TILE;
static_assert(kBcTile % kBlock == 0, "a tile is whole rounds of the workgroup");

struct BcHeader {
  int err_line;   // lowest line whose norm is +inf or past the table's end; INT_MAX: none
  int total;      // points of all lines (pf_scan_kernel)
};

struct BcMat {
  float m[12];   // row-major 3 x 4
};

struct BcConsts {
  int sqnorm_order, guard;
  int table_n;   // entries of the table this call may use
};

// pcl::transformPointCloud(Matrix4f) as floor_detection.hip's fd_transform restates it, on (x, y, 0): the z terms stay in the sums
// (0 * m is NaN for a non-finite m, and -0 + 0 is +0); the fourth float becomes 1
__device__ __forceinline__ float4 bc_transform(const float x, const float y, const float4 r0, const float4 r1, const float4 r2, const int order) {
#pragma clang fp contract(off)
  const float z = 0.0f;
  float4 q;
  if (order == 0) {
    q.x = x * r0.x + (y * r0.y + (z * r0.z + r0.w));
    q.y = x * r1.x + (y * r1.y + (z * r1.z + r1.w));
    q.z = x * r2.x + (y * r2.y + (z * r2.z + r2.w));
  } else {
    q.x = ((r0.x * x + r0.y * y) + r0.z * z) + r0.w;
    q.y = ((r1.x * x + r1.y * y) + r1.z * z) + r1.w;
    q.z = ((r2.x * x + r2.y * y) + r2.z * z) + r2.w;
  }
  q.w = 1.0f;
  return q;
}

// ================================================================================================ count pass
// ends: 6 doubles per line (pointA, pointB).  rec[l] = {a.x, a.y, dn.x, dn.y}, cnt[l] = points of line l.
__global__ __launch_bounds__(kBlock) void bc_count_kernel(const double* __restrict__ ends, const int n_lines, const float* __restrict__ table,
                                                          const BcConsts c, float4* __restrict__ rec, int* __restrict__ cnt,
                                                          BcHeader* __restrict__ hdr) {
#pragma clang fp contract(off)
  const int l = blockIdx.x * kBlock + threadIdx.x;
  if (l >= n_lines) return;
  const double* e = ends + (size_t)l * 6;
  const float ax = (float)e[0], ay = (float)e[1], az = (float)e[2];   // cast<float>(): round to nearest
  const float bx = (float)e[3], by = (float)e[4], bz = (float)e[5];
  const float dx = bx - ax, dy = by - ay, dz = bz - az;
  const float xx = dx * dx, yy = dy * dy, zz = dz * dz;
  // squaredNorm() with a zero w term [UPSTREAM-RECALL]: sqnorm_order
  const float n2 = c.sqnorm_order == DGS_PF_NORM_PAIRS_XY_ZW ? (xx + yy) + (zz + 0.0f)
                   : c.sqnorm_order == DGS_PF_NORM_PAIRS_XZ_YW ? (xx + zz) + (yy + 0.0f) : ((xx + yy) + zz) + 0.0f;
  const float norm = sqrtf(n2);   // correctly rounded: hipcc's default for sqrtf and `/` (HIP's __fsqrt_rn is the hardware's approximate v_sqrt_f32)
  float nx = dx, ny = dy;
  // normalized() [UPSTREAM-RECALL]: Eigen 3.3 divides by sqrt(n2) only when n2 > 0; the older form always: normalized_guard
  if (!c.guard || n2 > 0.0f) {
    nx = dx / norm;
    ny = dy / norm;
  }
  rec[l] = make_float4(ax, ay, nx, ny);
  int k = 0;
  if (norm == norm) {   // a NaN norm fails `i <= norm` at once
    if (norm > table[c.table_n - 1]) {   // +inf, or a line upstream would sample past the table's end
      atomicMin(&hdr->err_line, l);
    } else {   // entries <= norm: the table ascends strictly
      int lo = 0, hi = c.table_n;
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (table[mid] <= norm) lo = mid + 1;
        else hi = mid;
      }
      k = lo;
    }
  }
  cnt[l] = k;
}

// ================================================================================================ fill pass
// off: the scanned counts (first point per line), n_lines entries; `total` stands in for entry n_lines.  item_off[i] = off[item_lines[i]].
__global__ __launch_bounds__(kBlock) void bc_fill_kernel(const int* __restrict__ off, const float4* __restrict__ rec, const int* __restrict__ tix,
                                                         const BcMat* __restrict__ mats, const float* __restrict__ table, const int n_lines,
                                                         const int total, const int transform_order, const int* __restrict__ item_lines,
                                                         const int n_items, int* __restrict__ item_off, float4* __restrict__ out) {
#pragma clang fp contract(off)
  __shared__ int s_off[kBlock + 1];
  __shared__ int s_tix[kBlock];
  __shared__ float4 s_rec[kBlock], s_m0[kBlock], s_m1[kBlock], s_m2[kBlock];
  for (int i = blockIdx.x * kBlock + threadIdx.x; i <= n_items; i += gridDim.x * kBlock) {
    const int l = item_lines[i];
    item_off[i] = l < n_lines ? off[l] : total;
  }
  const int p0 = blockIdx.x * kBcTile;
  if (p0 >= total) return;   // the whole workgroup
  const int p1 = min(p0 + kBcTile, total);
  // the line that owns p0: the last line whose first point is <= p0 (it is not empty: an empty line shares its offset with the next)
  int lo = 0, hi = n_lines;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (off[mid] <= p0) lo = mid + 1;
    else hi = mid;
  }
  int line = lo - 1;
  int done = p0;
  while (done < p1) {   // uniform over the workgroup
    const int nl = min(kBlock, n_lines - line);
    __syncthreads();
    if ((int)threadIdx.x < nl) {
      const int l = line + threadIdx.x;
      s_off[threadIdx.x] = off[l];
      s_rec[threadIdx.x] = rec[l];
      const int t = tix[l];
      s_tix[threadIdx.x] = t;
      if (t >= 0) {
        const float4* m = reinterpret_cast<const float4*>(mats + t);
        s_m0[threadIdx.x] = m[0];
        s_m1[threadIdx.x] = m[1];
        s_m2[threadIdx.x] = m[2];
      }
    }
    if (threadIdx.x == 0) s_off[nl] = line + nl < n_lines ? off[line + nl] : total;
    __syncthreads();
    const int chunk_end = min(p1, s_off[nl]);
    for (int p = done + threadIdx.x; p < chunk_end; p += kBlock) {
      int a = 0, b = nl;   // the last j < nl with s_off[j] <= p; s_off[0] <= p < s_off[nl]
      while (b - a > 1) {
        const int mid = (a + b) >> 1;
        if (s_off[mid] <= p) a = mid;
        else b = mid;
      }
      const float4 r = s_rec[a];
      const float ik = table[p - s_off[a]];
      const float x = r.x + ik * r.z, y = r.y + ik * r.w;
      out[p] = s_tix[a] >= 0 ? bc_transform(x, y, s_m0[a], s_m1[a], s_m2[a], transform_order) : make_float4(x, y, 0.0f, 1.0f);
    }
    done = chunk_end;
    line += nl;
  }
}

// ================================================================================================ host side
namespace {

const char* bc_bad_params(const dgs_building_cloud_params* p) {
  if (!p) return "building cloud: no parameters";
  if (p->struct_size != sizeof(dgs_building_cloud_params)) return "building cloud: wrong struct_size";
  if (p->sqnorm_order < DGS_PF_NORM_PAIRS_XY_ZW || p->sqnorm_order > DGS_PF_NORM_SEQUENTIAL) return "building cloud: unknown sqnorm_order";
  if (p->transform_order < 0 || p->transform_order > 1) return "building cloud: unknown transform_order";
  if (!(p->sample_step > 0.0f) || !std::isfinite(p->sample_step)) return "building cloud: sample_step must be positive and finite";
  if (p->max_points_per_line < 1) return "building cloud: max_points_per_line must be at least 1";
  return nullptr;
}

inline size_t bc_align(size_t b) { return (b + 15) & ~(size_t)15; }

}  // namespace

void building_cloud_release(dgs_handle* h) {
  BcScratch& s = h->bcl;
  s.in.release(); s.table.release(); s.rec.release(); s.cnt.release(); s.item_off.release(); s.out.release();
  s.n_out = 0;
  s.n_items = -1;
}

}  // namespace dgs

using namespace dgs;

extern "C" {

int dgs_building_cloud_params_init(dgs_building_cloud_params* p) {
  if (!p) return DGS_ERR_INVALID_ARGUMENT;
  std::memset(p, 0, sizeof(*p));
  p->struct_size = sizeof(*p);
  p->sample_step = 0.02f;   // const float sample_step = 0.02 (:148)
  p->sqnorm_order = DGS_PF_NORM_PAIRS_XY_ZW;
  p->normalized_guard = 1;
  p->transform_order = 0;
  p->max_points_per_line = 1 << 20;
  return DGS_OK;
}

int dgs_building_cloud_generate(dgs_handle* h, const dgs_building_cloud_params* p, const dgs_line_feature* lines, const int64_t* line_offsets,
                                int64_t n_items, const float* transforms16, const int32_t* transform_index, int64_t* n_points) {
  // ---- arguments: refused before the handle or a device is looked at
  const char* why = bc_bad_params(p);
  if (!why && (!h || !n_points)) why = "building cloud: no handle or no n_points";
  if (!why && (n_items < 0 || n_items >= INT32_MAX || !line_offsets)) why = "building cloud: bad item count or no line offsets";
  if (!why && bc::first_bad_offset(line_offsets, n_items) >= 0) why = "building cloud: line offsets must ascend from 0";
  if (!why && (line_offsets[n_items] >= INT32_MAX || (line_offsets[n_items] > 0 && !lines))) why = "building cloud: too many lines, or no lines array";
  if (why) {
    if (h) h->err = why;
    else set_handleless_error(why);
    return DGS_ERR_INVALID_ARGUMENT;
  }
  const int n_lines = (int)line_offsets[n_items];
  int n_mats = 0;
  if (transforms16) {
    n_mats = 1;
    if (transform_index)
      for (int64_t i = 0; i < n_items; i++) {
        if (transform_index[i] < -1) {
          h->err = "building cloud: transform_index of item " + std::to_string(i) + " is below -1";
          return DGS_ERR_INVALID_ARGUMENT;
        }
        n_mats = std::max(n_mats, transform_index[i] + 1);
      }
  }
  BcScratch& s = h->bcl;
  h->err.clear();
  *n_points = 0;
  s.n_out = 0;
  s.n_items = -1;   // nothing to read until this call has succeeded
  for (int k = 0; k < 8; k++) s.counts8[k] = 0;
  s.counts8[6] = kBcTile;
  DGS_HIP_TRY(h, hipSetDevice(h->device));

  // ---- the table: long enough for the longest line, as far as max_points_per_line and the sequence allow
  if (s.steps.v.empty() || std::memcmp(&s.steps.step, &p->sample_step, sizeof(float)) != 0) {
    s.steps.reset(p->sample_step);
    s.table_on_device = 0;
  }
  double need = 0.0;
  int64_t bound_total = 0;
  for (int l = 0; l < n_lines; l++) need = std::max(need, bc::norm_bound(lines[l].point_a, lines[l].point_b));
  const int64_t added = s.steps.extend(need, p->max_points_per_line);
  const int64_t table_n = s.steps.usable(p->max_points_per_line);
  for (int l = 0; l < n_lines; l++)
    bound_total += bc::count_points(s.steps.v.data(), table_n, (float)std::min(bc::norm_bound(lines[l].point_a, lines[l].point_b), 3.0e38));
  if (bound_total > INT32_MAX - 2 * kBcTile) {   // the fill kernel counts points in int, a tile past the last one included
    h->err = "building cloud: more than INT32_MAX points";
    return DGS_ERR_INVALID_ARGUMENT;
  }
  const size_t table_size = s.steps.v.size();
  if (s.table.cap < table_size) s.table_on_device = 0;   // reserve drops what the buffer held
  DGS_HIP_TRY(h, s.table.reserve(table_size));
  const size_t table_new = table_size - (size_t)s.table_on_device;

  // ---- one staged upload: header, first line per item, matrix per line, matrices, end points; behind it the table's new entries
  const size_t o_items = bc_align(sizeof(BcHeader));
  const size_t o_tix = o_items + bc_align(((size_t)n_items + 1) * sizeof(int));
  const size_t o_mats = o_tix + bc_align((size_t)n_lines * sizeof(int));
  const size_t o_ends = o_mats + bc_align((size_t)n_mats * sizeof(BcMat));
  const size_t b_in = o_ends + (size_t)n_lines * 6 * sizeof(double);
  const size_t b_all = bc_align(b_in) + table_new * sizeof(float) + 64;
  if (ensure_pinned(h, b_all) != DGS_OK) return DGS_ERR_HIP;
  char* up = static_cast<char*>(h->pinned);
  BcHeader* hh = reinterpret_cast<BcHeader*>(up);
  hh->err_line = INT_MAX;
  hh->total = 0;
  int* u_items = reinterpret_cast<int*>(up + o_items);
  int* u_tix = reinterpret_cast<int*>(up + o_tix);
  BcMat* u_mats = reinterpret_cast<BcMat*>(up + o_mats);
  double* u_ends = reinterpret_cast<double*>(up + o_ends);
  for (int64_t i = 0; i <= n_items; i++) u_items[i] = (int)line_offsets[i];
  for (int64_t i = 0; i < n_items; i++) {
    const int t = !transforms16 ? -1 : (transform_index ? transform_index[i] : 0);
    for (int64_t l = line_offsets[i]; l < line_offsets[i + 1]; l++) u_tix[l] = t;
  }
  for (int m = 0; m < n_mats; m++)
    for (int r = 0; r < 3; r++)
      for (int c = 0; c < 4; c++) u_mats[m].m[r * 4 + c] = transforms16[(size_t)m * 16 + c * 4 + r];
  for (int l = 0; l < n_lines; l++) {
    std::memcpy(u_ends + (size_t)l * 6, lines[l].point_a, 3 * sizeof(double));
    std::memcpy(u_ends + (size_t)l * 6 + 3, lines[l].point_b, 3 * sizeof(double));
  }
  float* u_table = reinterpret_cast<float*>(up + bc_align(b_in));
  if (table_new) std::memcpy(u_table, s.steps.v.data() + s.table_on_device, table_new * sizeof(float));
  DGS_HIP_TRY(h, s.in.reserve(b_in));
  DGS_HIP_TRY(h, s.rec.reserve((size_t)std::max(n_lines, 1)));
  DGS_HIP_TRY(h, s.cnt.reserve((size_t)n_lines + 1));
  DGS_HIP_TRY(h, s.item_off.reserve((size_t)n_items + 1));
  DGS_HIP_TRY(h, hipMemcpyAsync(s.in.ptr, up, b_in, hipMemcpyHostToDevice, h->stream));
  if (table_new) DGS_HIP_TRY(h, hipMemcpyAsync(s.table.ptr + s.table_on_device, u_table, table_new * sizeof(float), hipMemcpyHostToDevice, h->stream));
  BcHeader* d_hdr = reinterpret_cast<BcHeader*>(s.in.ptr);
  const int* d_items = reinterpret_cast<const int*>(s.in.ptr + o_items);
  const int* d_tix = reinterpret_cast<const int*>(s.in.ptr + o_tix);
  const BcMat* d_mats = reinterpret_cast<const BcMat*>(s.in.ptr + o_mats);
  const double* d_ends = reinterpret_cast<const double*>(s.in.ptr + o_ends);

  // ---- counts, their scan, the total
  BcConsts c;
  c.sqnorm_order = p->sqnorm_order;
  c.guard = p->normalized_guard ? 1 : 0;
  c.table_n = (int)table_n;
  hipLaunchKernelGGL(bc_count_kernel, dim3(std::max(1u, compact_blocks(n_lines))), dim3(kBlock), 0, h->stream, d_ends, n_lines, s.table.ptr, c, s.rec.ptr,
                     s.cnt.ptr, d_hdr);
  hipLaunchKernelGGL(pf_scan_kernel, dim3(1), dim3(kCompactScanBlock), 0, h->stream, s.cnt.ptr, n_lines, &d_hdr->total);
  DGS_HIP_TRY(h, hipGetLastError());
  DGS_HIP_TRY(h, hipMemcpyAsync(hh, d_hdr, sizeof(BcHeader), hipMemcpyDeviceToHost, h->stream));
  DGS_HIP_TRY(h, hipStreamSynchronize(h->stream));   // the stage's one wait: every upload above has been read behind it
  s.table_on_device = (int64_t)table_size;
  s.counts8[0] = 2;
  s.counts8[1] = 1;
  s.counts8[2] = n_lines;
  s.counts8[4] = (int64_t)table_size;
  s.counts8[5] = added;
  s.counts8[7] = n_items;
  if (hh->err_line != INT_MAX) {
    const int l = hh->err_line;
    const int64_t item = bc::item_of_line(line_offsets, n_items, l);
    h->err = "building cloud: line " + std::to_string(l - line_offsets[item]) + " of item " + std::to_string(item) + " (line " + std::to_string(l) +
             " of the call) is infinitely long or longer than the table of sample positions reaches (" + std::to_string(table_n) +
             " points, max_points_per_line " + std::to_string(p->max_points_per_line) + ")";
    return DGS_ERR_INVALID_ARGUMENT;
  }
  const int total = hh->total;

  // ---- the points
  DGS_HIP_TRY(h, s.out.reserve((size_t)std::max(total, 1)));
  const unsigned tiles = (unsigned)std::max(1, (total + kBcTile - 1) / kBcTile);
  hipLaunchKernelGGL(bc_fill_kernel, dim3(tiles), dim3(kBlock), 0, h->stream, s.cnt.ptr, s.rec.ptr, d_tix, d_mats, s.table.ptr, n_lines, total,
                     p->transform_order, d_items, (int)n_items, s.item_off.ptr, s.out.ptr);
  DGS_HIP_TRY(h, hipGetLastError());
  s.counts8[0] = 3;
  s.counts8[3] = total;
  s.n_out = total;
  s.n_items = n_items;
  *n_points = total;
  return DGS_OK;
}

int dgs_building_cloud_get(dgs_handle* h, float* out_xyz16, int64_t capacity, int32_t out_on_device, int64_t* point_offsets, int64_t* n,
                           const float** device_ptr_out) {
  if (!h || !n || capacity < 0 || (capacity > 0 && !out_xyz16)) return DGS_ERR_INVALID_ARGUMENT;
  BcScratch& s = h->bcl;
  if (s.n_items < 0) {
    h->err = "building cloud: no result to read (no call yet, or the last one failed)";
    return DGS_ERR_INVALID_ARGUMENT;
  }
  const int64_t m = s.n_out;
  *n = m;
  if (device_ptr_out) *device_ptr_out = reinterpret_cast<const float*>(s.out.ptr);
  const bool want_points = out_xyz16 != nullptr;
  if (want_points && m > capacity) {
    h->err = "output buffer too small for the building cloud";
    return DGS_ERR_INVALID_ARGUMENT;
  }
  if (!want_points && !point_offsets && !device_ptr_out) return DGS_OK;
  DGS_HIP_TRY(h, hipSetDevice(h->device));
  int* ho = nullptr;
  if (point_offsets) {
    if (ensure_pinned(h, ((size_t)s.n_items + 1) * sizeof(int)) != DGS_OK) return DGS_ERR_HIP;
    ho = reinterpret_cast<int*>(h->pinned);
    DGS_HIP_TRY(h, hipMemcpyAsync(ho, s.item_off.ptr, ((size_t)s.n_items + 1) * sizeof(int), hipMemcpyDeviceToHost, h->stream));
  }
  if (want_points && m > 0)
    DGS_HIP_TRY(h, hipMemcpyAsync(out_xyz16, s.out.ptr, (size_t)m * sizeof(float4), out_on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, h->stream));
  DGS_HIP_TRY(h, hipStreamSynchronize(h->stream));   // also behind the fill launch: its device pointer may be read from any stream now
  DGS_HIP_TRY(h, hipGetLastError());
  if (point_offsets)
    for (int64_t i = 0; i <= s.n_items; i++) point_offsets[i] = ho[i];
  return DGS_OK;
}

int dgs_building_cloud_get_counts(dgs_handle* h, int64_t* counts8) {
  if (!h || !counts8) return DGS_ERR_INVALID_ARGUMENT;
  for (int k = 0; k < 8; k++) counts8[k] = h->bcl.counts8[k];
  return DGS_OK;
}

}  // extern "C"
