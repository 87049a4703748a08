// dgs::HipLineAligner -- LineBasedScanmatcher::align_global (src/hdl_graph_slam/line_based_scanmatcher.cpp:112-203, from the extracted
// source lines on) over libdgs_reg.so (include/dgs_reg.h, dgs_line_align_global).  INTEGRATION.md 4e shows the patch to align_global.
// Header-only and free of Eigen and PCL: LineFeatureT is any struct with upstream's six fields (pointA, pointB: indexable by 0..2 and
// assignable from double; mean_error, std_sigma, max_error, min_error), BestFitAlignmentT any struct with not_aligned_lines,
// aligned_lines (vectors of std::shared_ptr<LineFeatureT>), transformation (callable as transformation(row, col)) and fitness_score
// (real_avg_distance, avg_distance, coverage, coverage_percentage).  Built from the nodelet's private parameters
// (apps/delta_graph_slam_nodelet.cpp:98-102, same names and defaults).  The handle is created at the first call.  A failure of any kind
// never throws: alignGlobal() returns false (last_error() says why) and the caller falls back to the scalar loop.
// alignLocal() / alignLocalBatch() are LineBasedScanmatcher::align_local (:205-297; dgs_line_align_local_batch): one call for
// all near buildings of a keyframe.  They also set BestFitAlignmentT::isEdgeAligned.  The l_* weights come from the
// nodelet's delta_local_* parameters (apps/delta_graph_slam_nodelet.cpp:105-108); delta_local_avg_distance_weight is not read, because
// upstream's setter of that name writes the global member, so l_avg_distance_weight keeps the constructor's 0.6.
// alignOverlappedBatch() is LineBasedScanmatcher::align_overlapped_buildings (:29-107; dgs_line_align_overlapped_batch) from
// the building-frame lines on, one call for all overlapped pairs of a round; the caller keeps the frame transforms.
// edgeExtraction() / edgeExtractionBatch() are LineBasedScanmatcher::edge_extraction (:459-471) on the device
// (dgs_line_edge_extraction_batch): EdgeFeatureT is any struct with upstream's edgePoint, pointA and pointB (indexable by
// 0..2 and assignable from double).  params().edges_on_device = 1 makes alignGlobal() and alignLocalBatch() take their edges from the same
// kernels instead of the host's loop over line pairs: identical results, one more host wait per call; the default is 0.
#pragma once

#include <cstddef>
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
    p_.l_coverage_weight = private_nh.template param<double>("delta_local_coverage_weight", 1.5);
    p_.l_transform_weight = private_nh.template param<double>("delta_local_transform_weight", 0.1);
    p_.l_max_score_distance = private_nh.template param<double>("delta_local_max_score_distance", 1.0);
    p_.l_max_score_translation = private_nh.template param<double>("delta_local_max_score_translation", 3.5);
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

  struct LocalItem {   // one near building: align_local(linesSource, linesTarget, max_range)
    const std::vector<LinePtr>* linesSource;
    const std::vector<LinePtr>* linesTarget;
  };
  const std::vector<dgs_line_local_alignment>& lastLocal() const { return lal_; }   // winners, counts and statuses of the last batch

  // One device call for all items.  false: *results is untouched.
  bool alignLocalBatch(const std::vector<LocalItem>& items, double max_range, std::vector<BestFitAlignmentT>* results) {
    if (!results || !ensure_handle()) return false;
    src_.clear();
    trg_.clear();
    so_.assign(1, 0);
    to_.assign(1, 0);
    for (const LocalItem& it : items) {
      append(*it.linesSource, &src_);
      append(*it.linesTarget, &trg_);
      so_.push_back((int64_t)src_.size());
      to_.push_back((int64_t)trg_.size());
    }
    out_.resize(src_.size() ? src_.size() : 1);
    lal_.assign(items.size() ? items.size() : 1, dgs_line_local_alignment{});
    if (dgs_line_align_local_batch(h_, &p_, (int64_t)items.size(), src_.data(), so_.data(), trg_.data(), to_.data(), max_range, out_.data(),
                                   lal_.data()) != DGS_OK)
      return false;
    lal_.resize(items.size());
    results->assign(items.size(), BestFitAlignmentT());
    for (size_t b = 0; b < items.size(); b++) {
      BestFitAlignmentT& r = (*results)[b];
      const std::vector<LinePtr>& ls = *items[b].linesSource;
      r.not_aligned_lines = ls;
      for (size_t i = 0; i < ls.size(); i++) {
        auto line = std::make_shared<LineFeatureT>(*ls[i]);
        for (int a = 0; a < 3; a++) {
          line->pointA[a] = out_[(size_t)so_[b] + i].point_a[a];
          line->pointB[a] = out_[(size_t)so_[b] + i].point_b[a];
        }
        r.aligned_lines.push_back(line);
      }
      for (int rr = 0; rr < 4; rr++)
        for (int c = 0; c < 4; c++) r.transformation(rr, c) = lal_[b].transformation[4 * rr + c];
      r.fitness_score.real_avg_distance = lal_[b].fitness_score[0];
      r.fitness_score.avg_distance = lal_[b].fitness_score[1];
      r.fitness_score.coverage = lal_[b].fitness_score[2];
      r.fitness_score.coverage_percentage = lal_[b].fitness_score[3];
      r.isEdgeAligned = lal_[b].is_edge_aligned != 0;
    }
    return true;
  }
  struct OverlapItem {   // one overlapped pair (A, B) in A's frame: A's and B's lines, A's centre (upstream: zero) and B's
    const std::vector<LinePtr>* linesSource;
    const std::vector<LinePtr>* linesTarget;
    double center_source[3];
    double center_target[3];
  };
  const std::vector<dgs_line_overlap_alignment>& lastOverlapped() const { return lov_; }   // winners, counts, is_identity of the last batch

  // One device call for all items.  Sets not_aligned_lines, aligned_lines and transformation; false: *results is untouched.
  bool alignOverlappedBatch(const std::vector<OverlapItem>& items, std::vector<BestFitAlignmentT>* results) {
    if (!results || !ensure_handle()) return false;
    src_.clear();
    trg_.clear();
    so_.assign(1, 0);
    to_.assign(1, 0);
    cs_.clear();
    ct_.clear();
    for (const OverlapItem& it : items) {
      append(*it.linesSource, &src_);
      append(*it.linesTarget, &trg_);
      so_.push_back((int64_t)src_.size());
      to_.push_back((int64_t)trg_.size());
      cs_.insert(cs_.end(), it.center_source, it.center_source + 3);
      ct_.insert(ct_.end(), it.center_target, it.center_target + 3);
    }
    out_.resize(src_.size() ? src_.size() : 1);
    lov_.assign(items.size() ? items.size() : 1, dgs_line_overlap_alignment{});
    if (dgs_line_align_overlapped_batch(h_, &p_, (int64_t)items.size(), src_.data(), so_.data(), trg_.data(), to_.data(), cs_.data(), ct_.data(),
                                        out_.data(), lov_.data()) != DGS_OK)
      return false;
    lov_.resize(items.size());
    results->assign(items.size(), BestFitAlignmentT());
    for (size_t b = 0; b < items.size(); b++) {
      BestFitAlignmentT& r = (*results)[b];
      const std::vector<LinePtr>& ls = *items[b].linesSource;
      r.not_aligned_lines = ls;
      for (size_t i = 0; i < ls.size(); i++) {
        auto line = std::make_shared<LineFeatureT>(*ls[i]);
        for (int a = 0; a < 3; a++) {
          line->pointA[a] = out_[(size_t)so_[b] + i].point_a[a];
          line->pointB[a] = out_[(size_t)so_[b] + i].point_b[a];
        }
        r.aligned_lines.push_back(line);
      }
      for (int rr = 0; rr < 4; rr++)
        for (int c = 0; c < 4; c++) r.transformation(rr, c) = lov_[b].transformation[4 * rr + c];
    }
    return true;
  }
  dgs_handle* handle() { return ensure_handle() ? h_ : nullptr; }   // for the test hooks

  struct EdgeItem {   // one edge_extraction(lines, only_angular_edges, max_dist_angular_edge) call
    const std::vector<LinePtr>* lines;
    bool only_angular_edges;
    double max_dist_angular_edge;
  };
  // One device call for all items; (*edges)[b] is what edge_extraction returns for item b.  false: *edges is untouched.
  template <typename EdgeFeatureT>
  bool edgeExtractionBatch(const std::vector<EdgeItem>& items, std::vector<std::vector<std::shared_ptr<EdgeFeatureT>>>* edges) {
    if (!edges || !ensure_handle()) return false;
    src_.clear();
    so_.assign(1, 0);
    std::vector<int32_t> only;
    std::vector<double> dist;
    for (const EdgeItem& it : items) {
      append(*it.lines, &src_);
      so_.push_back((int64_t)src_.size());
      only.push_back(it.only_angular_edges ? 1 : 0);
      dist.push_back(it.max_dist_angular_edge);
    }
    if (items.empty()) {   // the arrays of an empty batch may not be NULL-checked by every caller: give them one element
      only.push_back(0);
      dist.push_back(0.0);
    }
    to_.assign(items.size() + 1, 0);
    int64_t n = 0;
    const int rc = dgs_line_edge_extraction_batch(h_, src_.data(), so_.data(), (int64_t)items.size(), only.data(), dist.data(), nullptr, 0, to_.data(), &n);
    if (rc != DGS_OK && n == 0) return false;   // with edges to fetch the count-only call reports the missing room
    std::vector<dgs_edge_feature> e((size_t)(n ? n : 1));
    if (n && dgs_line_edge_extraction_batch(h_, src_.data(), so_.data(), (int64_t)items.size(), only.data(), dist.data(), e.data(), n, to_.data(), &n) != DGS_OK)
      return false;
    edges->assign(items.size(), std::vector<std::shared_ptr<EdgeFeatureT>>());
    for (size_t b = 0; b < items.size(); b++)
      for (int64_t k = to_[b]; k < to_[b + 1]; k++) {
        auto f = std::make_shared<EdgeFeatureT>();
        for (int a = 0; a < 3; a++) {
          f->edgePoint[a] = e[(size_t)k].edge_point[a];
          f->pointA[a] = e[(size_t)k].point_a[a];
          f->pointB[a] = e[(size_t)k].point_b[a];
        }
        (*edges)[b].push_back(f);
      }
    return true;
  }
  template <typename EdgeFeatureT>
  bool edgeExtraction(const std::vector<LinePtr>& lines, bool only_angular_edges, double max_dist_angular_edge,
                      std::vector<std::shared_ptr<EdgeFeatureT>>* edges) {
    std::vector<std::vector<std::shared_ptr<EdgeFeatureT>>> r;
    if (!edges || !edgeExtractionBatch<EdgeFeatureT>({EdgeItem{&lines, only_angular_edges, max_dist_angular_edge}}, &r)) return false;
    *edges = r[0];
    return true;
  }

  bool alignLocal(const std::vector<LinePtr>& linesSource, const std::vector<LinePtr>& linesTarget, double max_range, BestFitAlignmentT* result) {
    std::vector<BestFitAlignmentT> r;
    if (!result || !alignLocalBatch({LocalItem{&linesSource, &linesTarget}}, max_range, &r)) return false;
    *result = r[0];
    return true;
  }

 private:
  static void append(const std::vector<LinePtr>& lines, std::vector<dgs_line_feature>* out) {
    std::vector<dgs_line_feature> one;
    pack(lines, &one);
    out->insert(out->end(), one.begin(), one.begin() + (std::ptrdiff_t)lines.size());
  }
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
  std::vector<int64_t> so_, to_;
  std::vector<dgs_line_local_alignment> lal_;
  std::vector<dgs_line_overlap_alignment> lov_;
  std::vector<double> cs_, ct_;
};

}  // namespace dgs
