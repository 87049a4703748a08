// dgs::HipRegistration -- pcl::Registration<PointSource, PointTarget> over libdgs_reg.so (include/dgs_reg.h).
//
// This is the object a patched hdl_graph_slam::select_registration_method returns for registration_method
// "NDT_HIP" / "FAST_GICP_HIP" (reference factory: src/hdl_graph_slam/registrations.cpp:22-124).  It is
// consumed unchanged through the base-class pointer by
//   apps/scan_matching_odometry_nodelet.cpp:180,185,218,222,228,318,327   and
//   include/hdl_graph_slam/loop_detector.hpp:124,138,145,148,149,155.
// Header-only; needs PCL (pcl/registration/registration.h) and Eigen at the USER's build, nothing else.
//
// Contract kept from the reference's registration objects:
//   * setInputTarget / setInputSource take the caller's shared cloud; the points are copied to HBM at the call
//     (pcl::PointXYZ is already the 16-byte x, y, z, pad record the ABI wants), the pointer is also kept in the base class;
//   * align(out, guess) -> pcl::Registration::align -> computeTransformation(out, guess) below; `out` receives
//     final_transformation * source; failure of any kind (no device, HIP error) never throws: converged_ = false and
//     final_transformation_ = guess, which the callers already treat as "skip" (scan_matching_odometry_nodelet.cpp:222-226,
//     loop_detector.hpp:149);
//   * getFitnessScore(max_range) shadows pcl::Registration's (non-virtual there) and is answered on the device; call it
//     through the derived type (INTEGRATION.md section 3/4 patch the two call sites with a downcast) or use
//     dgs_get_fitness_score -- through a base-class pointer PCL's own single-threaded CPU loop runs on the same
//     final_transformation_ and the base kd-tree.  After setKeepPclTree(false) that tree is no longer rebuilt; it is then
//     pointed at a one-point sentinel cloud at 1e30, so a base-pointer getFitnessScore() returns DBL_MAX ("no score")
//     instead of a value computed against a stale target, and nearestKSearch reports an infinite distance.
#pragma once

#include <cfloat>
#include <cstring>
#include <memory>
#include <string>
#include <unordered_map>
#include <vector>

#include <pcl/registration/registration.h>

#include "../dgs_reg.h"

namespace dgs {

template <typename PointSource, typename PointTarget>
class HipRegistration : public pcl::Registration<PointSource, PointTarget, float> {
 public:
  using Base = pcl::Registration<PointSource, PointTarget, float>;
  using PointCloudSource = typename Base::PointCloudSource;
  using PointCloudSourceConstPtr = typename Base::PointCloudSourceConstPtr;
  using PointCloudTargetConstPtr = typename Base::PointCloudTargetConstPtr;
  using Matrix4 = typename Base::Matrix4;

  static_assert(sizeof(PointSource) == 16 && sizeof(PointTarget) == 16, "clouds must be 16-byte x, y, z, pad points (pcl::PointXYZ)");

  explicit HipRegistration(dgs_method method) {
    dgs_params_init(&params_, method);
    dgs_icp_options_init(&icp_options_);
    dgs_pcl_gicp_options_init(&pg_options_);
    this->reg_name_ = (method == DGS_METHOD_GICP) ? "dgs::HipRegistration<FAST_GICP>" : (method == DGS_METHOD_VGICP) ? "dgs::HipRegistration<FAST_VGICP>"
                      : (method == DGS_METHOD_ICP)       ? "dgs::HipRegistration<ICP>"
                      : (method == DGS_METHOD_PCL_GICP)  ? "dgs::HipRegistration<PCL_GICP>"
                      : (method == DGS_METHOD_PCL_NDT)   ? "dgs::HipRegistration<PCL_NDT>"
                                                         : "dgs::HipRegistration<NDT>";
    // the reference's setters below write into params_; PCL's own setters (epsilon, iterations, distance) are read at align()
    this->transformation_epsilon_ = params_.transformation_epsilon;
    this->max_iterations_ = params_.maximum_iterations;
    this->corr_dist_threshold_ = params_.gicp_max_correspondence_distance;
  }
  ~HipRegistration() override {
    forgetPairClouds();
    if (handle_) dgs_destroy(handle_);
  }
  HipRegistration(const HipRegistration&) = delete;
  HipRegistration& operator=(const HipRegistration&) = delete;

  // ---- the setters registrations.cpp calls on ndt_omp / fast_gicp objects (:30-34, :106-118) ----
  void setNumThreads(int n) { params_.num_threads = n; dirty_ = true; }
  void setResolution(float r) { params_.ndt_resolution = r; params_.vgicp_resolution = r; dirty_ = true; }  // NDT leaf / VGICP voxel size
  void setNeighborSearchMethod(int method) { params_.vgicp_search_method = method; dirty_ = true; }        // FastVGICP (dgs_vgicp_search)
  void setNeighborhoodSearchMethod(int method) { params_.ndt_search_method = method; dirty_ = true; }  // dgs_ndt_search == pclomp order
  void setCorrespondenceRandomness(int k) { params_.gicp_correspondence_randomness = k; dirty_ = true; }
  void setStepSize(double s) { params_.ndt_step_size = s; dirty_ = true; }
  // dgs_ndt_strict_order: 0 fast (re-associated, opt-in), 1 upstream operation order (default), 2 + index-order sums (validation, dgs_reg.h)
  void setNdtStrictOrder(int order) { params_.ndt_strict_order = order; dirty_ = true; }
  // the pieces of the upstream order, one by one (all on by default; dgs_reg.h): Eigen's two-sided JacobiSVD sequence for the Newton
  // step, PCL's double computeHessian after a line search, the guess's rotation as Affine3f::rotation() takes it, std::exp(float) as glibc computes it
  void setNdtUpstreamFidelity(bool jacobi_svd, bool hessian_double, bool guess_polar, bool exp_glibc = true, bool cov_eigen_qr = true) {
    params_.ndt_newton_solver = jacobi_svd;
    params_.ndt_hessian_recompute_double = hessian_double;
    params_.ndt_guess_rotation_polar = guess_polar;
    params_.ndt_exp_glibc = exp_glibc;
    params_.ndt_cov_eigensolver = cov_eigen_qr;
    dirty_ = true;
  }
  void setOulierRatio(double r) { params_.ndt_outlier_ratio = r; dirty_ = true; }  // (sic) upstream spelling
  void setRotationEpsilon(double e) {   // FAST_GICP's dgs_params field; GICP_HIP's rotation_epsilon_ (applied to a live handle)
    if (params_.method == DGS_METHOD_PCL_GICP) { pg_options_.rotation_epsilon = e; apply_pg_options(); }
    else { params_.gicp_rotation_epsilon = e; dirty_ = true; }
  }
  void setRegularizationMethod(int m) { params_.gicp_regularization = m; dirty_ = true; }
  // dgs_gicp_cov_mode (dgs_reg.h): 0 tree sums + symmetric eigen-decomposition (default), 1 tree sums + JacobiSVD, 2 upstream order (ordered neighbours,
  // sequential sums, JacobiSVD: the covariances of calculate_covariances bit for bit).  FAST_GICP / FAST_VGICP; takes effect at the next handle.
  void setCovarianceMode(int mode) { params_.gicp_cov_jacobi_svd = mode; dirty_ = true; }
  void setDevice(int ordinal) { params_.device = ordinal; dirty_ = true; }
  // pcl::IterativeClosestPoint (DGS_METHOD_ICP): registrations.cpp:63, and the criteria settings dgs_params has no field for
  // (applied to a live handle in place: its target stays uploaded and indexed)
  void setUseReciprocalCorrespondences(bool on) {   // ICP: reciprocal mode; GICP_HIP: accepted and without effect, as upstream
    icp_options_.use_reciprocal_correspondences = on ? 1 : 0;
    pg_options_.use_reciprocal_correspondences = on ? 1 : 0;
    apply_icp_options();
    apply_pg_options();
  }
  // dgs_set_batch_independent (dgs_reg.h): every field of a pair's result, and every fitness, a function of (parameters, target,
  // source, guess) alone -- align(), alignPairs() and any batch give the same bits for the same pair.  Applied to a live handle in place, and
  // to every handle made later; a method that refuses the switch (NDT_HIP in the fast order) says so in lastError() at the next align().
  void setBatchIndependent(bool on) {
    batch_independent_ = on;
    if (handle_ && dgs_set_batch_independent(handle_, on ? 1 : 0) != DGS_OK) dirty_ = true;   // else: at the next dgs_create
  }
  bool getBatchIndependent() const { return batch_independent_; }
  void setIcpOptions(const dgs_icp_options& o) { icp_options_ = o; icp_options_.struct_size = sizeof(dgs_icp_options); apply_icp_options(); }
  const dgs_icp_options& icpOptions() const { return icp_options_; }
  // pcl::GeneralizedIterativeClosestPoint (DGS_METHOD_PCL_GICP): registrations.cpp:74 and the settings dgs_params has no field for
  void setMaximumOptimizerIterations(int n) { pg_options_.max_optimizer_iterations = n; apply_pg_options(); }
  void setPclGicpOptions(const dgs_pcl_gicp_options& o) { pg_options_ = o; pg_options_.struct_size = sizeof(dgs_pcl_gicp_options); apply_pg_options(); }
  const dgs_pcl_gicp_options& pclGicpOptions() const { return pg_options_; }
  dgs_params params() const {   // the dgs_params the next dgs_create gets (PCL's own setters are read at align())
    dgs_params p = params_;
    p.transformation_epsilon = this->transformation_epsilon_;
    p.maximum_iterations = this->max_iterations_;
    p.gicp_max_correspondence_distance = this->corr_dist_threshold_;
    return p;
  }
  const std::string& registrationName() const { return this->reg_name_; }   // pcl::Registration::getClassName()
  // false: skip PCL's CPU kd-tree rebuild in initCompute() on every new target (then use getInlierFraction() instead of
  // getSearchMethodTarget()->nearestKSearch())
  void setKeepPclTree(bool keep) {
    keep_pcl_tree_ = keep;
    this->force_no_recompute_ = !keep;
    if (!keep) park_pcl_tree();
    else this->target_cloud_updated_ = true;   // PCL rebuilds its tree at the next align()
  }

  void setInputTarget(const PointCloudTargetConstPtr& cloud) override {
    Base::setInputTarget(cloud);
    target_dirty_ = true;
    if (!keep_pcl_tree_) park_pcl_tree();
  }
  void setInputSource(const PointCloudSourceConstPtr& cloud) override {
    Base::setInputSource(cloud);
    source_dirty_ = true;
  }

  // registration->getFitnessScore(max_range) on the device (see the header comment about base-class pointers)
  double getFitnessScore(double max_range = DBL_MAX) {
    double s = DBL_MAX;
    if (!handle_ || dgs_get_fitness_score(handle_, max_range, &s) != DGS_OK) return DBL_MAX;
    return s;
  }
  // the inlier loop of publish_scan_matching_status (scan_matching_odometry_nodelet.cpp:321-332) in one call
  double getInlierFraction(double max_sq_dist) {
    double f = 0.0;
    if (!handle_ || dgs_get_inlier_fraction(handle_, max_sq_dist, &f) != DGS_OK) return 0.0;
    return f;
  }
  // n registrations that each name their own target in ONE device call (dgs_align_pairs_clouds; no method gate here: the
  // library serves FAST_GICP and GICP_HIP / GICP_OMP_HIP and names any other method in lastError()): pair i is
  // (targets[i], sources[i], guesses[i]) -- a tick of loop_detector.hpp:59-80, where every new keyframe is a target with a short candidate
  // list of its own.  (*results)[i] is what setInputTarget(targets[i]) + setInputSource(sources[i]) + align(guesses[i]) would leave, with
  // fitness = getFitnessScore(max_range) when compute_fitness.  The clouds are uploaded once per pcl::PointCloud object and kept with their
  // index and covariances (an entry holds its cloud's shared pointer; forgetPairCloud(ptr) releases one, a new handle releases all).
  // REQUIREMENT: a cloud passed here is immutable while it is resident, as KeyFrame::cloud is (keyframe.hpp:51).  The entry is keyed by
  // the cloud object's address and its point count, so points edited in place at the same size are NOT seen: call forgetPairCloud(ptr)
  // before using such a cloud again.  Entries (host cloud kept alive + device copy) live until forgetPairCloud / forgetPairClouds, a new
  // handle or the destructor: call forgetPairCloud when a keyframe leaves the graph, or memory grows with every cloud ever passed.
  // This object's own target, source and last result are untouched.  false: nothing was registered (lastError() says why) and *results
  // is untouched; statuses of single pairs (empty source or target; GICP_HIP: a cloud of fewer than k points) are in the records.
  bool alignPairs(const std::vector<PointCloudTargetConstPtr>& targets, const std::vector<PointCloudSourceConstPtr>& sources,
                  const std::vector<Matrix4>& guesses, bool compute_fitness, double max_range, std::vector<dgs_result>* results) {
    const size_t n = targets.size();
    if (!results || sources.size() != n || (!guesses.empty() && guesses.size() != n) || !ensure_handle()) return false;
    std::vector<dgs_cloud*> t(n, nullptr), s(n, nullptr);
    std::vector<float> g(guesses.empty() ? 0 : n * 16);
    for (size_t i = 0; i < n; i++) {
      if (!targets[i] || !sources[i]) return false;
      t[i] = resident(targets[i]);
      s[i] = resident(sources[i]);
      if (!t[i] || !s[i]) return false;
      if (!guesses.empty()) std::memcpy(&g[i * 16], guesses[i].data(), sizeof(float) * 16);   // Eigen's column-major, as the ABI wants
    }
    std::vector<dgs_result> out(n);
    if (dgs_align_pairs_clouds(handle_, (int32_t)n, t.data(), s.data(), guesses.empty() ? nullptr : g.data(), compute_fitness ? 1 : 0, max_range,
                               out.data()) != DGS_OK)
      return false;
    results->swap(out);
    return true;
  }
  // What alignPairs would do to these clouds before its first round, ahead of time and for all of them together
  // (dgs_cloud_build_covariances): upload (once per pcl::PointCloud object, alignPairs' residency and its REQUIREMENT), the exact-NN
  // indices in one batched build, the k-NN covariances in one search and one covariance launch per chunk of clouds.  FAST_GICP,
  // FAST_VGICP, GICP_HIP / GICP_OMP_HIP; any other method is named in lastError().  false: nothing was built.
  template <class CloudPtr>
  bool buildCovariances(const std::vector<CloudPtr>& clouds) {
    if (!ensure_handle()) return false;
    std::vector<dgs_cloud*> c(clouds.size(), nullptr);
    for (size_t i = 0; i < clouds.size(); i++) {
      if (!clouds[i]) return false;
      c[i] = resident(clouds[i]);
      if (!c[i]) return false;
    }
    return dgs_cloud_build_covariances(handle_, (int32_t)c.size(), c.data()) == DGS_OK;
  }
  void forgetPairCloud(const void* cloud) {
    auto it = pair_clouds_.find(cloud);
    if (it == pair_clouds_.end()) return;
    dgs_cloud_destroy(it->second.cloud);
    pair_clouds_.erase(it);
  }
  void forgetPairClouds() {
    for (auto& kv : pair_clouds_) dgs_cloud_destroy(kv.second.cloud);
    pair_clouds_.clear();
  }

  const dgs_result& lastResult() const { return last_; }
  std::string lastError() const { return handle_ ? dgs_last_error(handle_) : dgs_last_error(nullptr); }
  dgs_handle* handle() { return handle_; }

 protected:
  void apply_icp_options() {
    if (handle_ && params_.method == DGS_METHOD_ICP && dgs_set_icp_options(handle_, &icp_options_) != DGS_OK) dirty_ = true;   // else: at the next dgs_create
  }
  void apply_pg_options() {
    if (handle_ && params_.method == DGS_METHOD_PCL_GICP && dgs_set_pcl_gicp_options(handle_, &pg_options_) != DGS_OK) dirty_ = true;
  }
  bool ensure_handle() {
    params_.transformation_epsilon = this->transformation_epsilon_;
    params_.maximum_iterations = this->max_iterations_;
    params_.gicp_max_correspondence_distance = this->corr_dist_threshold_;
    if (handle_ && !dirty_ && params_.transformation_epsilon == applied_.transformation_epsilon &&
        params_.maximum_iterations == applied_.maximum_iterations &&
        params_.gicp_max_correspondence_distance == applied_.gicp_max_correspondence_distance)
      return true;
    forgetPairClouds();   // their covariances were made under the old parameters
    if (handle_) dgs_destroy(handle_);
    handle_ = nullptr;
    if (dgs_create(&params_, &handle_) != DGS_OK) return false;
    if (params_.method == DGS_METHOD_ICP && dgs_set_icp_options(handle_, &icp_options_) != DGS_OK) return false;
    if (params_.method == DGS_METHOD_PCL_GICP && dgs_set_pcl_gicp_options(handle_, &pg_options_) != DGS_OK) return false;
    if (batch_independent_ && dgs_set_batch_independent(handle_, 1) != DGS_OK) return false;
    applied_ = params_;
    dirty_ = false;
    target_dirty_ = source_dirty_ = true;
    return true;
  }

  void computeTransformation(PointCloudSource& output, const Matrix4& guess) override {
    this->converged_ = false;
    this->nr_iterations_ = 0;
    this->final_transformation_ = guess;
    if (!ensure_handle()) return;
    if (target_dirty_ && this->target_) {
      if (dgs_set_input_target(handle_, reinterpret_cast<const float*>(this->target_->points.data()), (int64_t)this->target_->points.size(), 0) != DGS_OK) return;
      target_dirty_ = false;
    }
    if (source_dirty_ && this->input_) {
      if (dgs_set_input_source(handle_, reinterpret_cast<const float*>(this->input_->points.data()), (int64_t)this->input_->points.size(), 0) != DGS_OK) return;
      source_dirty_ = false;
    }
    output.points.resize(this->input_->points.size());
    if (dgs_align(handle_, guess.data(), &last_, reinterpret_cast<float*>(output.points.data()), 0) != DGS_OK) return;
    std::memcpy(this->final_transformation_.data(), last_.final_transformation, sizeof(float) * 16);
    this->transformation_ = this->final_transformation_;
    this->converged_ = last_.converged != 0;
    this->nr_iterations_ = last_.iterations;
  }

  // the base kd-tree is not maintained (setKeepPclTree(false)): make that visible instead of leaving the previous target in it
  void park_pcl_tree() {
    if (!sentinel_) {
      typename pcl::PointCloud<PointTarget>::Ptr c(new pcl::PointCloud<PointTarget>());
      c->points.resize(1);
      c->points[0].x = c->points[0].y = c->points[0].z = 1e30f;
      c->width = 1;
      sentinel_ = c;
    }
    if (this->tree_) this->tree_->setInputCloud(sentinel_);
  }

  // alignPairs: the device copy of a host cloud, keyed by the cloud object's address; `owner` keeps that address from passing to another cloud
  struct PairCloud {
    dgs_cloud* cloud;
    size_t n;
    std::shared_ptr<void> owner;   // a copy of the caller's smart pointer, whatever its kind (boost:: before PCL 1.11, std:: from it on)
  };
  template <class CloudPtr>
  dgs_cloud* resident(const CloudPtr& cloud) {
    const void* key = cloud.get();
    const size_t n = cloud->points.size();
    auto it = pair_clouds_.find(key);
    if (it != pair_clouds_.end() && it->second.n == n) return it->second.cloud;
    if (it != pair_clouds_.end()) forgetPairCloud(key);
    dgs_cloud* c = nullptr;
    if (dgs_cloud_create(handle_, reinterpret_cast<const float*>(cloud->points.data()), (int64_t)n, 0, &c) != DGS_OK) return nullptr;
    pair_clouds_[key] = PairCloud{c, n, std::make_shared<CloudPtr>(cloud)};
    return c;
  }
  std::unordered_map<const void*, PairCloud> pair_clouds_;

  typename pcl::PointCloud<PointTarget>::ConstPtr sentinel_;
  dgs_params params_{};
  dgs_params applied_{};
  dgs_icp_options icp_options_{};
  dgs_pcl_gicp_options pg_options_{};
  dgs_handle* handle_ = nullptr;
  dgs_result last_{};
  bool dirty_ = true, target_dirty_ = true, source_dirty_ = true, keep_pcl_tree_ = true;
  bool batch_independent_ = false;   // setBatchIndependent: applied to every handle this object makes
};

}  // namespace dgs
