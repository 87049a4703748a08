// Factory branches for hdl_graph_slam::select_registration_method (src/hdl_graph_slam/registrations.cpp:22-124).
// Usage inside the reference factory (see INTEGRATION.md for the full patch):
//
//   #include <dgs/registrations_hip.hpp>
//   ...
//   if (auto reg = dgs::select_hip_registration<PointT>(registration_method, pnh)) return reg;
//
// `Params` is anything with `template <class T> T param(const std::string&, const T&)` -- ros::NodeHandle in the nodelets.
#pragma once

#include <iostream>
#include <string>
#include <utility>

#include "hip_registration.hpp"

namespace dgs {

// pnh.param<bool>(name, def) where the handle has a typed getParam (ros::NodeHandle); otherwise the value read as an int (parameter
// sources that only know numbers and strings)
template <typename Params>
auto param_bool(Params& pnh, const std::string& name, bool def, int) -> decltype(pnh.getParam(name, std::declval<bool&>()), bool()) {
  bool v = def;
  return pnh.getParam(name, v) ? v : def;
}
template <typename Params>
bool param_bool(Params& pnh, const std::string& name, bool def, long) {
  return pnh.template param<int>(name, def ? 1 : 0) != 0;
}

template <typename PointT, typename Params>
typename pcl::Registration<PointT, PointT>::Ptr select_hip_registration_method(const std::string& registration_method, Params& pnh);

// not a parameter of the reference: dgs_batch_independent (default false) turns on HipRegistration::setBatchIndependent for whichever HIP
// back-end the method names -- a pair's result then does not depend on the batch, the launch shape or the entry point that registered it
template <typename PointT, typename Params>
typename pcl::Registration<PointT, PointT>::Ptr select_hip_registration(const std::string& registration_method, Params& pnh) {
  typename pcl::Registration<PointT, PointT>::Ptr base = select_hip_registration_method<PointT>(registration_method, pnh);
  if (base && param_bool(pnh, "dgs_batch_independent", false, 0)) static_cast<HipRegistration<PointT, PointT>*>(base.get())->setBatchIndependent(true);
  return base;
}

template <typename PointT, typename Params>
typename pcl::Registration<PointT, PointT>::Ptr select_hip_registration_method(const std::string& registration_method, Params& pnh) {
  using Reg = HipRegistration<PointT, PointT>;
  if (registration_method == "FAST_GICP_HIP") {
    std::cout << "registration: FAST_GICP_HIP" << std::endl;
    typename pcl::Registration<PointT, PointT>::Ptr base(new Reg(DGS_METHOD_GICP));
    Reg* gicp = static_cast<Reg*>(base.get());
    gicp->setNumThreads(pnh.template param<int>("reg_num_threads", 0));                                   // registrations.cpp:30
    gicp->setTransformationEpsilon(pnh.template param<double>("reg_transformation_epsilon", 0.01));       // :31
    gicp->setMaximumIterations(pnh.template param<int>("reg_maximum_iterations", 64));                    // :32
    gicp->setMaxCorrespondenceDistance(pnh.template param<double>("reg_max_correspondence_distance", 2.5));  // :33
    gicp->setCorrespondenceRandomness(pnh.template param<int>("reg_correspondence_randomness", 20));      // :34
    // not a parameter of the reference: covariances in upstream's operation order (dgs_reg.h, DGS_GICP_COV_UPSTREAM_ORDER); off by default
    if (param_bool(pnh, "reg_covariance_upstream_order", false, 0)) gicp->setCovarianceMode(DGS_GICP_COV_UPSTREAM_ORDER);
    return base;
  }
  if (registration_method == "FAST_VGICP_HIP") {
    std::cout << "registration: FAST_VGICP_HIP" << std::endl;
    typename pcl::Registration<PointT, PointT>::Ptr base(new Reg(DGS_METHOD_VGICP));
    Reg* vgicp = static_cast<Reg*>(base.get());
    vgicp->setNumThreads(pnh.template param<int>("reg_num_threads", 0));                                  // registrations.cpp:51
    vgicp->setResolution(static_cast<float>(pnh.template param<double>("reg_resolution", 1.0)));          // :52
    vgicp->setTransformationEpsilon(pnh.template param<double>("reg_transformation_epsilon", 0.01));      // :53
    vgicp->setMaximumIterations(pnh.template param<int>("reg_maximum_iterations", 64));                   // :54
    vgicp->setCorrespondenceRandomness(pnh.template param<int>("reg_correspondence_randomness", 20));     // :55
    if (param_bool(pnh, "reg_covariance_upstream_order", false, 0)) vgicp->setCovarianceMode(DGS_GICP_COV_UPSTREAM_ORDER);   // as FAST_GICP_HIP
    return base;
  }
  if (registration_method == "ICP_HIP") {   // registrations.cpp:59-64 on the GPU (the reference's own "ICP" string keeps its branch)
    std::cout << "registration: ICP_HIP" << std::endl;
    typename pcl::Registration<PointT, PointT>::Ptr base(new Reg(DGS_METHOD_ICP));
    Reg* icp = static_cast<Reg*>(base.get());
    icp->setTransformationEpsilon(pnh.template param<double>("reg_transformation_epsilon", 0.01));          // :60
    icp->setMaximumIterations(pnh.template param<int>("reg_maximum_iterations", 64));                       // :61
    icp->setMaxCorrespondenceDistance(pnh.template param<double>("reg_max_correspondence_distance", 2.5));  // :62
    icp->setUseReciprocalCorrespondences(param_bool(pnh, "reg_use_reciprocal_correspondences", false, 0));  // :63
    return base;
  }
  if (registration_method == "GICP_HIP" || registration_method == "GICP_OMP_HIP") {   // registrations.cpp:65-87 on the GPU (pcl:: and
    // pclomp::GeneralizedIterativeClosestPoint are one algorithm; the reference's own "GICP" / "GICP_OMP" strings keep their branches)
    std::cout << "registration: " << registration_method << std::endl;
    typename pcl::Registration<PointT, PointT>::Ptr base(new Reg(DGS_METHOD_PCL_GICP));
    Reg* gicp = static_cast<Reg*>(base.get());
    gicp->setTransformationEpsilon(pnh.template param<double>("reg_transformation_epsilon", 0.01));                // :69 / :79
    gicp->setMaximumIterations(pnh.template param<int>("reg_maximum_iterations", 64));                             // :70 / :80
    gicp->setUseReciprocalCorrespondences(param_bool(pnh, "reg_use_reciprocal_correspondences", false, 0));        // :71 / :81
    gicp->setMaxCorrespondenceDistance(pnh.template param<double>("reg_max_correspondence_distance", 2.5));        // :72 / :82
    gicp->setCorrespondenceRandomness(pnh.template param<int>("reg_correspondence_randomness", 20));               // :73 / :83
    gicp->setMaximumOptimizerIterations(pnh.template param<int>("reg_max_optimizer_iterations", 20));              // :74 / :84
    return base;
  }
  if (registration_method == "PCL_NDT_HIP") {   // registrations.cpp:94-100 on the GPU: pcl::NormalDistributionsTransform (the reference's own
    // "NDT" string and every unknown name keep that branch); setStepSize / setOulierRatio keep PCL's defaults (0.1, 0.55)
    const double ndt_resolution = pnh.template param<double>("reg_resolution", 0.5);                      // :93
    std::cout << "registration: PCL_NDT_HIP " << ndt_resolution << std::endl;
    typename pcl::Registration<PointT, PointT>::Ptr base(new Reg(DGS_METHOD_PCL_NDT));
    Reg* ndt = static_cast<Reg*>(base.get());
    ndt->setTransformationEpsilon(pnh.template param<double>("reg_transformation_epsilon", 0.01));        // :97
    ndt->setMaximumIterations(pnh.template param<int>("reg_maximum_iterations", 64));                     // :98
    ndt->setResolution(static_cast<float>(ndt_resolution));                                                // :99
    return base;
  }
  if (registration_method == "NDT_HIP") {
    const double ndt_resolution = pnh.template param<double>("reg_resolution", 0.5);                      // :93
    const std::string nn_search_method = pnh.template param<std::string>("reg_nn_search_method", "DIRECT7");  // :103
    std::cout << "registration: NDT_HIP " << nn_search_method << " " << ndt_resolution << std::endl;
    typename pcl::Registration<PointT, PointT>::Ptr base(new Reg(DGS_METHOD_NDT));
    Reg* ndt = static_cast<Reg*>(base.get());
    ndt->setNumThreads(pnh.template param<int>("reg_num_threads", 0));                                    // :102
    ndt->setTransformationEpsilon(pnh.template param<double>("reg_transformation_epsilon", 0.01));        // :110
    ndt->setMaximumIterations(pnh.template param<int>("reg_maximum_iterations", 64));                     // :111
    ndt->setResolution(static_cast<float>(ndt_resolution));                                                // :112
    ndt->setNeighborhoodSearchMethod(nn_search_method == "KDTREE" ? DGS_NDT_KDTREE : nn_search_method == "DIRECT1" ? DGS_NDT_DIRECT1 : DGS_NDT_DIRECT7);  // :113-119
    return base;
  }
  return typename pcl::Registration<PointT, PointT>::Ptr();
}

}  // namespace dgs
