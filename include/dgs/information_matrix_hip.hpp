// dgs::HipInformationMatrixCalculator -- hdl_graph_slam::InformationMatrixCalculator (src/hdl_graph_slam/information_matrix_calculator.cpp,
// include/hdl_graph_slam/information_matrix_calculator.hpp) over libdgs_reg.so (include/dgs_reg.h, dgs_calc_fitness_score_batch_clouds;
// DESIGN.md 6k).  INTEGRATION.md shows the two call sites of the optimisation tick (apps/delta_graph_slam_nodelet.cpp:572,820).
// Header-only and free of Eigen and ROS (pcl::PointCloud is the only outside type): PointT is a 16-byte x, y, z, pad point (pcl::PointXYZ), PoseT anything whose
// operator()(row, col) reads a 4 x 4 transform (Eigen::Isometry3d), MatT anything whose operator()(row, col) writes a 3 x 3 matrix
// (Eigen::MatrixXd, Eigen::Matrix3d).  Parameters load from any Params with param<T>(name, default) (ros::NodeHandle); the defaults are
// the reference CONSTRUCTOR's (fitness_score_thresh 0.5; the reference's `load` template says 2.5 and is not what the nodelet calls).
// Clouds are uploaded once per pcl::PointCloud object and kept with their NN index; an entry holds its cloud's shared pointer, so the address
// it is keyed by cannot pass to another cloud, and forget(ptr) releases both when a keyframe goes.  The handle is
// created at the first call.  A failure never throws: the calc_* calls that need the device return false (last_error() says why) and the
// caller keeps its CPU path.
#pragma once

#include <cmath>
#include <cstdint>
#include <memory>
#include <type_traits>
#include <unordered_map>
#include <vector>

#include <pcl/point_cloud.h>

#include "../dgs_reg.h"

namespace dgs {

template <typename PointT, typename PoseT, typename MatT>
class HipInformationMatrixCalculator {
  static_assert(sizeof(PointT) == 16, "clouds must be 16-byte x, y, z, pad points (pcl::PointXYZ)");

 public:
  using CloudConstPtr = typename pcl::PointCloud<PointT>::ConstPtr;   // boost::shared_ptr before PCL 1.11, std::shared_ptr from it on
  struct Edge {
    CloudConstPtr cloud1, cloud2;
    PoseT relpose;
  };

  explicit HipInformationMatrixCalculator(int device = 0) : device_(device) {}
  template <class Params>
  explicit HipInformationMatrixCalculator(Params& nh, int device = 0) : device_(device) {
    load(nh);
  }
  ~HipInformationMatrixCalculator() {
    for (auto& kv : clouds_) dgs_cloud_destroy(kv.second.cloud);
    if (h_) dgs_destroy(h_);
  }
  HipInformationMatrixCalculator(const HipInformationMatrixCalculator&) = delete;
  HipInformationMatrixCalculator& operator=(const HipInformationMatrixCalculator&) = delete;

  // information_matrix_calculator.cpp:28-48
  template <class Params>
  void load(Params& nh) {
    use_const_inf_matrix = nh.template param<bool>("use_const_inf_matrix", false);
    const_stddev_x = nh.template param<double>("const_stddev_x", 0.5);
    const_stddev_q = nh.template param<double>("const_stddev_q", 0.1);
    var_gain_a = nh.template param<double>("var_gain_a", 20.0);
    min_stddev_x = nh.template param<double>("min_stddev_x", 0.1);
    max_stddev_x = nh.template param<double>("max_stddev_x", 5.0);
    min_stddev_q = nh.template param<double>("min_stddev_q", 0.05);
    max_stddev_q = nh.template param<double>("max_stddev_q", 0.2);
    fitness_score_thresh = nh.template param<double>("fitness_score_thresh", 0.5);
    b_var_gain_a = nh.template param<double>("delta_var_gain_a", 20.0);
    b_min_stddev_x = nh.template param<double>("delta_min_stddev_x", 0.1);
    b_max_stddev_x = nh.template param<double>("delta_max_stddev_x", 5.0);
    b_min_stddev_q = nh.template param<double>("delta_min_stddev_q", 0.05);
    b_max_stddev_q = nh.template param<double>("delta_max_stddev_q", 0.2);
    b_avg_fitness_score = nh.template param<double>("delta_avg_fitness_score", 0.5);
    b_importance_ratio_global = nh.template param<double>("delta_importance_ratio_global", 1.0);
    b_importance_ratio_local = nh.template param<double>("delta_importance_ratio_local", 1.0);
  }

  const char* last_error() const { return dgs_last_error(h_); }
  dgs_handle* handle() { return h_; }

  // the device copy (and index) of a cloud that is going away, or whose points changed in place
  void forget(const void* cloud) {
    auto it = clouds_.find(cloud);
    if (it == clouds_.end()) return;
    dgs_cloud_destroy(it->second.cloud);
    clouds_.erase(it);
  }

  // calc_fitness_score of every edge in one device call; scores[e] = DBL_MAX where no point qualifies.  false: *scores is untouched.
  bool calc_fitness_scores(const std::vector<Edge>& edges, std::vector<double>* scores, double max_range = 1.7976931348623157e308) {
    if (!scores || !ensure_handle()) return false;
    const size_t n = edges.size();
    c1_.assign(n, nullptr);
    c2_.assign(n, nullptr);
    rel_.assign(n * 16, 0.f);
    for (size_t e = 0; e < n; e++) {
      if (!edges[e].cloud1 || !edges[e].cloud2) return false;
      c1_[e] = resident(edges[e].cloud1);
      c2_[e] = resident(edges[e].cloud2);
      if (!c1_[e] || !c2_[e]) return false;
      for (int c = 0; c < 4; c++)
        for (int r = 0; r < 4; r++) rel_[e * 16 + (size_t)(c * 4 + r)] = (float)edges[e].relpose(r, c);   // relpose.cast<float>(), column-major
    }
    out_.assign(n, 0.0);
    if (dgs_calc_fitness_score_batch_clouds(h_, (int32_t)n, c1_.data(), c2_.data(), rel_.data(), max_range, out_.data(), nullptr) != DGS_OK) return false;
    *scores = out_;
    return true;
  }

  // calc_information_matrix for all edges of a tick (.cpp:53-75 per edge).  false: *infs is untouched.
  bool calc_information_matrices(const std::vector<Edge>& edges, std::vector<MatT>* infs) {
    if (!infs) return false;
    std::vector<MatT> res;
    if (use_const_inf_matrix) {
      for (size_t e = 0; e < edges.size(); e++) res.push_back(constant());
    } else {
      std::vector<double> fit;
      if (!calc_fitness_scores(edges, &fit)) return false;
      for (const double f : fit) res.push_back(from_fitness(f));
    }
    infs->swap(res);
    return true;
  }

  bool calc_information_matrix(const CloudConstPtr& cloud1, const CloudConstPtr& cloud2, const PoseT& relpose, MatT* inf) {
    if (!inf) return false;
    std::vector<MatT> res;
    if (!calc_information_matrices(std::vector<Edge>{Edge{cloud1, cloud2, relpose}}, &res)) return false;
    *inf = res[0];
    return true;
  }

  // .cpp:110-132; host arithmetic only.  The constant matrix is returned undivided, as upstream does.
  MatT calc_information_matrix_buildings_global(double fitness_score) const {
    if (use_const_inf_matrix) return constant();
    MatT inf = from_fitness(fitness_score);
    for (int r = 0; r < 3; r++)
      for (int c = 0; c < 3; c++) inf(r, c) = inf(r, c) / b_importance_ratio_global;
    return inf;
  }

  // .cpp:134-157; host arithmetic only.  AlignmentT: BestFitAlignment (fitness_score.avg_distance, .coverage_percentage, isEdgeAligned).
  template <class AlignmentT>
  MatT calc_information_matrix_buildings_local(const AlignmentT& result) const {
    const float w_x = (float)b_weight(b_var_gain_a, b_avg_fitness_score, std::pow(b_min_stddev_x, 2), std::pow(b_max_stddev_x, 2), result.fitness_score.avg_distance);
    const float w_q = (float)b_weight(b_var_gain_a, b_avg_fitness_score, std::pow(b_min_stddev_q, 2), std::pow(b_max_stddev_q, 2), result.fitness_score.avg_distance);
    MatT inf = diagonal(1.0 / w_x, 1.0 / w_q);
    for (int r = 0; r < 3; r++)
      for (int c = 0; c < 3; c++) {
        if (result.isEdgeAligned) inf(r, c) = inf(r, c) * b_importance_ratio_local;
        inf(r, c) = inf(r, c) * (result.fitness_score.coverage_percentage / 100.);
      }
    return inf;
  }

  bool use_const_inf_matrix = false;
  double const_stddev_x = 0.5, const_stddev_q = 0.1;
  double var_gain_a = 20.0, min_stddev_x = 0.1, max_stddev_x = 5.0, min_stddev_q = 0.05, max_stddev_q = 0.2, fitness_score_thresh = 0.5;
  double b_var_gain_a = 20.0, b_min_stddev_x = 0.1, b_max_stddev_x = 5.0, b_min_stddev_q = 0.05, b_max_stddev_q = 0.2, b_avg_fitness_score = 0.5;
  double b_importance_ratio_global = 1.0, b_importance_ratio_local = 1.0;

 private:
  static double weight(double a, double max_x, double min_y, double max_y, double x) {
    const double y = (1.0 - std::exp(-a * x)) / (1.0 - std::exp(-a * max_x));
    return min_y + (max_y - min_y) * y;
  }
  static double b_weight(double a, double avg_x, double min_y, double max_y, double x) {
    const double y = std::exp(a * (x - avg_x)) / (std::exp(a * (x - avg_x)) + 1.0);
    return min_y + (max_y - min_y) * y;
  }
  static MatT diagonal(double xy, double q) {
    MatT inf = make();
    for (int r = 0; r < 3; r++)
      for (int c = 0; c < 3; c++) inf(r, c) = (r != c) ? 0.0 : (r < 2 ? xy : q);
    return inf;
  }
  static MatT make() {
    if constexpr (std::is_constructible<MatT, int, int>::value) return MatT(3, 3);
    else return MatT();
  }
  MatT constant() const { return diagonal(1.0 / const_stddev_x, 1.0 / const_stddev_q); }
  MatT from_fitness(double fitness_score) const {   // the two weights pass through `float` (.cpp:68-69)
    const float w_x = (float)weight(var_gain_a, fitness_score_thresh, std::pow(min_stddev_x, 2), std::pow(max_stddev_x, 2), fitness_score);
    const float w_q = (float)weight(var_gain_a, fitness_score_thresh, std::pow(min_stddev_q, 2), std::pow(max_stddev_q, 2), fitness_score);
    return diagonal(1.0 / w_x, 1.0 / w_q);
  }

  bool ensure_handle() {
    if (h_) return true;
    dgs_params prm;
    if (dgs_params_init(&prm, DGS_METHOD_NDT) != DGS_OK) return false;
    prm.device = device_;
    return dgs_create(&prm, &h_) == DGS_OK;
  }

  dgs_cloud* resident(const CloudConstPtr& cloud) {
    auto it = clouds_.find(cloud.get());
    if (it != clouds_.end() && it->second.n == cloud->points.size()) return it->second.cloud;
    if (it != clouds_.end()) forget(cloud.get());
    dgs_cloud* c = nullptr;
    if (dgs_cloud_create(h_, reinterpret_cast<const float*>(cloud->points.data()), (int64_t)cloud->points.size(), 0, &c) != DGS_OK) return nullptr;
    clouds_[cloud.get()] = Resident{c, cloud->points.size(), cloud};
    return c;
  }

  struct Resident {
    dgs_cloud* cloud;
    size_t n;
    CloudConstPtr owner;   // keeps the host cloud alive: its address cannot pass to another cloud while the entry exists
  };
  dgs_handle* h_ = nullptr;
  int device_ = 0;
  std::unordered_map<const void*, Resident> clouds_;
  std::vector<dgs_cloud*> c1_, c2_;
  std::vector<float> rel_;
  std::vector<double> out_;
};

}  // namespace dgs
