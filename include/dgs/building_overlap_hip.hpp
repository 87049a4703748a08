// dgs::HipBuildingOverlap -- getOverlappedBuildings (apps/delta_graph_slam_nodelet.cpp:767-787) with are_buildings_overlapped
// (include/hdl_graph_slam/check_overlapping.hpp) over libdgs_reg.so (include/dgs_reg.h, dgs_building_overlap_pairs).
// INTEGRATION.md 4g shows the rewritten loop of the optimisation tick.  Header-only and free of Eigen and PCL: LineFeatureT is any struct
// with pointA and pointB indexable by 0..2.  The handle is created at the first call.  A failure never throws: overlappedPairs() returns
// false (last_error() says why) and the caller falls back to the scalar double loop.
#pragma once

#include <algorithm>
#include <array>
#include <cstdint>
#include <memory>
#include <utility>
#include <vector>

#include "../dgs_reg.h"

namespace dgs {

template <typename LineFeatureT>
class HipBuildingOverlap {
 public:
  using LinePtr = std::shared_ptr<LineFeatureT>;

  explicit HipBuildingOverlap(int device = 0) : device_(device) {}
  ~HipBuildingOverlap() {
    if (h_) dgs_destroy(h_);
  }
  HipBuildingOverlap(const HipBuildingOverlap&) = delete;
  HipBuildingOverlap& operator=(const HipBuildingOverlap&) = delete;

  const char* last_error() const { return dgs_last_error(h_); }

  // buildings[b]: Building::getLines(); centers[b]: the translation of Building::estimate() (z is not read).  pairs: every overlapped
  // (i, j), i < j, in upstream's order (i ascending, then j ascending).  false: *pairs is untouched.
  bool overlappedPairs(const std::vector<std::vector<LinePtr>>& buildings, const std::vector<std::array<double, 3>>& centers,
                       std::vector<std::pair<int, int>>* pairs) {
    if (!pairs || centers.size() != buildings.size() || !ensure_handle()) return false;
    lines_.clear();
    off_.assign(1, 0);
    ctr_.clear();
    for (size_t b = 0; b < buildings.size(); b++) {
      for (const LinePtr& l : buildings[b]) {
        dgs_line_feature f{};
        for (int a = 0; a < 3; a++) {
          f.point_a[a] = l->pointA[a];
          f.point_b[a] = l->pointB[a];
        }
        lines_.push_back(f);
      }
      off_.push_back((int64_t)lines_.size());
      ctr_.insert(ctr_.end(), centers[b].begin(), centers[b].end());
    }
    if (lines_.empty()) lines_.resize(1);
    if (ctr_.empty()) ctr_.resize(3);
    int64_t n = 0;
    out_.resize(std::max<size_t>(4 * buildings.size(), 64) * 2);   // overlaps are few; a fuller list takes a second call
    int rc = dgs_building_overlap_pairs(h_, lines_.data(), off_.data(), ctr_.data(), (int64_t)buildings.size(), out_.data(), (int64_t)out_.size() / 2, &n);
    if (rc == DGS_ERR_CAPACITY) {
      out_.resize((size_t)n * 2);
      rc = dgs_building_overlap_pairs(h_, lines_.data(), off_.data(), ctr_.data(), (int64_t)buildings.size(), out_.data(), n, &n);
    }
    if (rc != DGS_OK) return false;
    pairs->clear();
    for (int64_t k = 0; k < n; k++) pairs->emplace_back(out_[(size_t)(2 * k)], out_[(size_t)(2 * k + 1)]);
    return true;
  }

 private:
  bool ensure_handle() {
    if (h_) return true;
    dgs_params prm;
    if (dgs_params_init(&prm, DGS_METHOD_NDT) != DGS_OK) return false;
    prm.device = device_;
    return dgs_create(&prm, &h_) == DGS_OK;
  }

  dgs_handle* h_ = nullptr;
  int device_ = 0;
  std::vector<dgs_line_feature> lines_;
  std::vector<int64_t> off_;
  std::vector<double> ctr_;
  std::vector<int32_t> out_;
};

}  // namespace dgs
