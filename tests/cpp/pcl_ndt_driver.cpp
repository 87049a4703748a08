// CPU replay of delta_graph_slam_amd/csrc/pcl_ndt.h, the header the PCL_NDT_HIP kernel runs: the same text compiled for the host.
//   pcl_ndt_driver host <scene file> <result file>
// Scene file (little endian), written by tests/test_pcl_ndt_cpu.py:
//   int32[14]  min_b[3] max_b[3] mul1 mul2 leaf_pow2 n_voxels n_cells n_points kind fix_d1
//   float[2]   leaf inv_leaf          double[8]  gauss_d1 gauss_d2 pose[6]          float[12]  T, row-major 3 x 4
//   int32[n_cells] cell -> voxel      float[4 n_voxels] centroids      double[12 n_voxels] mean | icov      float[4 n_points] source
// Result file: int32 n_items; int32[n_points] neighbours per point; int32[n_items] voxel of every item, a point's in slot order;
//   double[43 n_items] the item's increments (score, gradient, Hessian row-major).
// Build: g++ -std=c++17 -O1 -ffp-contract=off (-fsanitize=address,undefined for the sanitizer run of DESIGN.md 6i).
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../delta_graph_slam_amd/csrc/pcl_ndt.h"

namespace pn = dgs::pn;

template <class T>
static bool read_vec(FILE* f, std::vector<T>& v, size_t n) {
  v.resize(n);
  return n == 0 || std::fread(v.data(), sizeof(T), n, f) == n;
}

template <int KIND>
static void one_item(const float (&xt)[3], const double (&x)[3], const pn::Tables& tab, const double* rec, double d1, double d2, double* out43) {
  double xj[8], xh[15];
  pn::point_tables<KIND != 0>(x, tab.j, tab.h, xj, xh);
  double acc[pn::kAccum];
  for (int k = 0; k < pn::kAccum; k++) acc[k] = 0.0;
  pn::item<KIND>(xt, xj, xh, rec, d1, d2, acc, [](double a) { return std::exp(a); });
  std::memcpy(out43, acc, sizeof(acc));
}

int main(int argc, char** argv) {
  if (argc != 4 || std::strcmp(argv[1], "host") != 0) {
    std::fprintf(stderr, "usage: %s host <scene> <result>\n", argv[0]);
    return 2;
  }
  FILE* f = std::fopen(argv[2], "rb");
  if (!f) return 3;
  int32_t hdr[14];
  float lf[2], T[12];
  double dd[8];
  if (std::fread(hdr, 4, 14, f) != 14 || std::fread(lf, 4, 2, f) != 2 || std::fread(dd, 8, 8, f) != 8 || std::fread(T, 4, 12, f) != 12) return 4;
  const int nv = hdr[9], n_cells = hdr[10], ns = hdr[11], kind = hdr[12], fix_d1 = hdr[13];
  if (nv < 0 || n_cells < 0 || ns < 0 || kind < 0 || kind > 2) return 4;
  std::vector<int32_t> cell2vox;
  std::vector<float> cent, src;
  std::vector<double> vtab;
  if (!read_vec(f, cell2vox, (size_t)n_cells) || !read_vec(f, cent, (size_t)nv * 4) || !read_vec(f, vtab, (size_t)nv * 12) || !read_vec(f, src, (size_t)ns * 4)) return 4;
  std::fclose(f);
  for (int32_t v : cell2vox)
    if (v < -1 || v >= nv) return 5;
  pn::Grid g;
  for (int k = 0; k < 3; k++) { g.min_b[k] = hdr[k]; g.max_b[k] = hdr[3 + k]; }
  g.mul1 = hdr[6];
  g.mul2 = hdr[7];
  g.leaf_pow2 = hdr[8];
  g.leaf = lf[0];
  g.inv_leaf = lf[1];
  g.cell2vox = cell2vox.data();
  g.centroid = cent.data();
  if ((int64_t)(g.max_b[0] - g.min_b[0] + 1) * (g.max_b[1] - g.min_b[1] + 1) * (g.max_b[2] - g.min_b[2] + 1) != n_cells) return 5;
  pn::Tables tab;
  pn::angle_tables(dd[5], dd[6], dd[7], fix_d1, tab);

  std::vector<int32_t> counts((size_t)ns, 0), vids;
  std::vector<double> inc;
  for (int i = 0; i < ns; i++) {
    const float* s = src.data() + (size_t)i * 4;
    float xt[3];
    pn::transform_point(T, s[0], s[1], s[2], xt);
    int c[3];
    unsigned mask = pn::neighbourhood(g, xt, c);
    const double x[3] = {(double)s[0], (double)s[1], (double)s[2]};
    for (int k = 0; k < pn::kSlots; k++) {
      if (!((mask >> k) & 1u)) continue;
      const int vid = pn::slot_voxel(g, c, k);
      counts[i]++;
      vids.push_back(vid);
      inc.resize(inc.size() + pn::kAccum);
      double* out = inc.data() + inc.size() - pn::kAccum;
      const double* rec = vtab.data() + (size_t)vid * 12;
      if (kind == 1) one_item<1>(xt, x, tab, rec, dd[0], dd[1], out);
      else if (kind == 2) one_item<2>(xt, x, tab, rec, dd[0], dd[1], out);
      else one_item<0>(xt, x, tab, rec, dd[0], dd[1], out);
    }
  }
  FILE* o = std::fopen(argv[3], "wb");
  if (!o) return 6;
  const int32_t n_items = (int32_t)vids.size();
  std::fwrite(&n_items, 4, 1, o);
  if (!counts.empty()) std::fwrite(counts.data(), 4, counts.size(), o);
  if (!vids.empty()) std::fwrite(vids.data(), 4, vids.size(), o);   // (an empty vector's data() may be null)
  if (!inc.empty()) std::fwrite(inc.data(), 8, inc.size(), o);
  std::fclose(o);
  return 0;
}
