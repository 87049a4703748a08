// dgs::HipLineAligner -- LineBasedScanmatcher::align_global (src/hdl_graph_slam/line_based_scanmatcher.cpp:112-203, from the extracted
// source lines on) over libdgs_reg.so (include/dgs_reg.h, dgs_line_align_global).  INTEGRATION.md 4e shows the patch to align_global.
// Header-only and free of Eigen and PCL: LineFeatureT is any struct with upstream's six fields (pointA, pointB: indexable by 0..2 and
// assignable from double; mean_error, std_sigma, max_error, min_error), BestFitAlignmentT any struct with not_aligned_lines,
// aligned_lines (vectors of std::shared_ptr<LineFeatureT>), transformation (callable as transformation(row, col)) and fitness_score
// (real_avg_distance, avg_distance, coverage, coverage_percentage).  Built from the nodelet's private parameters
// (apps/delta_graph_slam_nodelet.cpp:98-102, same names and defaults).  The handle is created at the first call.  A failure of any kind
// never throws: alignGlobal() returns false (last_error() says why) and the caller falls back to the scalar loop.
#pragma once

#include <cstdint>
#include <memory>
#include <vector>

#include "../dgs_reg.h"

namespace dgs {

template <typename LineFeatureT, typename BestFitAlignmentT>
class HipLineAligner {
 public:
  using LinePtr = std::shared_ptr<LineFeatureT>;

  // NodeHandle: anything with param<T>(name, default), e.g. ros::NodeHandle (private_nh)
  template <typename NodeHandle>
  explicit HipLineAligner(NodeHandle& private_nh, int device = 0) : device_(device) {
    dgs_line_align_params_init(&p_);
    p_.g_avg_distance_weight = private_nh.template param<double>("delta_global_avg_distance_weight", 1.5);
    p_.g_coverage_weight = private_nh.template param<double>("delta_global_coverage_weight", 0.5);
    p_.g_transform_weight = private_nh.template param<double>("delta_global_transform_weight", 0.5);
    p_.g_max_score_distance = private_nh.template param<double>("delta_global_max_score_distance", 3.5);
    p_.g_max_score_translation = private_nh.template param<double>("delta_global_max_score_translation", 3.5);
  }
  ~HipLineAligner() {
    if (h_) dgs_destroy(h_);
  }
  HipLineAligner(const HipLineAligner&) = delete;
  HipLineAligner& operator=(const HipLineAligner&) = delete;

  dgs_line_align_params& params() { return p_; }
  const char* last_error() const { return dgs_last_error(h_); }
  const dgs_line_alignment& last() const { return al_; }   // winner, counts, refinement steps and status of the last call

  // linesSource: line_extraction's output; linesTarget: the buildings' lines before merge_lines.  false: *result is untouched.
  bool alignGlobal(const std::vector<LinePtr>& linesSource, const std::vector<LinePtr>& linesTarget, bool constrain_angle, double max_range,
                   BestFitAlignmentT* result) {
    if (!result || !ensure_handle()) return false;
    pack(linesSource, &src_);
    pack(linesTarget, &trg_);
    out_.resize(src_.size() ? src_.size() : 1);
    if (dgs_line_align_global(h_, &p_, src_.data(), (int64_t)linesSource.size(), trg_.data(), (int64_t)linesTarget.size(), constrain_angle ? 1 : 0,
                              max_range, out_.data(), &al_) != DGS_OK)
      return false;
    result->not_aligned_lines = linesSource;
    result->aligned_lines.clear();
    for (size_t i = 0; i < linesSource.size(); i++) {
      auto line = std::make_shared<LineFeatureT>(*linesSource[i]);   // transform_lines copies the line and replaces its two points
      for (int a = 0; a < 3; a++) {
        line->pointA[a] = out_[i].point_a[a];
        line->pointB[a] = out_[i].point_b[a];
      }
      result->aligned_lines.push_back(line);
    }
    for (int r = 0; r < 4; r++)
      for (int c = 0; c < 4; c++) result->transformation(r, c) = al_.transformation[4 * r + c];
    result->fitness_score.real_avg_distance = al_.fitness_score[0];
    result->fitness_score.avg_distance = al_.fitness_score[1];
    result->fitness_score.coverage = al_.fitness_score[2];
    result->fitness_score.coverage_percentage = al_.fitness_score[3];
    return true;
  }

 private:
  static void pack(const std::vector<LinePtr>& lines, std::vector<dgs_line_feature>* out) {
    out->resize(lines.size() ? lines.size() : 1);
    for (size_t i = 0; i < lines.size(); i++) {
      dgs_line_feature& f = (*out)[i];
      for (int a = 0; a < 3; a++) {
        f.point_a[a] = lines[i]->pointA[a];
        f.point_b[a] = lines[i]->pointB[a];
      }
      f.mean_error = lines[i]->mean_error;
      f.std_sigma = lines[i]->std_sigma;
      f.max_error = lines[i]->max_error;
      f.min_error = lines[i]->min_error;
    }
  }
  bool ensure_handle() {
    if (h_) return true;
    dgs_params prm;
    if (dgs_params_init(&prm, DGS_METHOD_NDT) != DGS_OK) return false;
    prm.device = device_;
    return dgs_create(&prm, &h_) == DGS_OK;
  }

  dgs_line_align_params p_{};
  dgs_line_alignment al_{};
  dgs_handle* h_ = nullptr;
  int device_ = 0;
  std::vector<dgs_line_feature> src_, trg_, out_;
};

}  // namespace dgs
