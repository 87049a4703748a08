/* dgs_reg.h -- C ABI of libdgs_reg.so: MI355X (gfx950) scan registration for delta_graph_slam.
 *
 * This is the drop-in boundary for ONE hot path of KennyRotella/delta_graph_slam: the
 * pcl::Registration<pcl::PointXYZ,pcl::PointXYZ> object that
 *   /root/reference/src/hdl_graph_slam/registrations.cpp:22-124  (select_registration_method) builds, and that
 *   /root/reference/apps/scan_matching_odometry_nodelet.cpp:173-270,309-346 and
 *   /root/reference/include/hdl_graph_slam/loop_detector.hpp:119-173 drive.
 * Each entry point names the reference interface it replaces.  The C++ adapter that re-exposes this ABI as a
 * pcl::Registration subclass is include/dgs/hip_registration.hpp; INTEGRATION.md shows the factory patch.
 *
 * Conventions
 *   - extern "C", opaque handle, POD structs, plain pointers + counts, int status (0 = DGS_OK), never throws.
 *   - Clouds are pcl::PointXYZ arrays: float[n][4] = x, y, z, pad (16-byte stride; the pad value is ignored).
 *   - Transforms are Eigen::Matrix4f memory: 16 floats, COLUMN-major.
 *   - `on_device` != 0 means the pointer is a device (HBM) pointer valid on the handle's device; the call then
 *     works on the handle's stream and does not touch host memory.  Ordering contract for device pointers: the DATA must be
 *     complete when the call is made (the handle's stream is not ordered against the stream that produced it: synchronise that
 *     stream, or make the handle share it with dgs_set_stream), and the library has finished READING the buffer when the call
 *     returns (set_input_* copy it, align_batch / fitness calls read it in place), so it may be freed or reused at once.
 *     With host pointers the library copies at the call and never retains the pointer.
 *   - A handle is used by one thread at a time; different handles are independent (two live handles per
 *     process is the reference's normal case: odometry + loop detector).
 *   - There is NO CPU fallback: every call fails with DGS_ERR_HIP when no gfx950 device is usable.
 */
#ifndef DGS_REG_H
#define DGS_REG_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DGS_ABI_VERSION 5

typedef struct dgs_handle dgs_handle;
typedef struct dgs_cloud dgs_cloud; /* a cloud resident in HBM together with its NN index / covariances (see below) */

enum dgs_status {
  DGS_OK = 0,
  DGS_ERR_INVALID_ARGUMENT = 1,
  DGS_ERR_HIP = 2,            /* a HIP runtime call failed; dgs_last_error() has the text */
  DGS_ERR_NO_TARGET = 3,      /* align()/fitness before setInputTarget (PCL: "no input target dataset") */
  DGS_ERR_NO_SOURCE = 4,
  DGS_ERR_GRID_TOO_LARGE = 5, /* voxel index would overflow (pcl::VoxelGridCovariance: "Leaf size is too small") */
  DGS_ERR_UNSUPPORTED = 6,
  DGS_ERR_CAPACITY = 7        /* dgs_building_overlap_pairs: more results than `capacity`; the first `capacity` are written, the count is full */
};

/* registration_method strings of registrations.cpp:26-124 that this library serves */
enum dgs_method {
  DGS_METHOD_NDT = 0,  /* "NDT_OMP": pclomp::NormalDistributionsTransform, registrations.cpp:101-120 */
  DGS_METHOD_GICP = 1, /* "FAST_GICP": fast_gicp::FastGICP, registrations.cpp:27-36 */
  DGS_METHOD_VGICP = 2, /* "FAST_VGICP": fast_gicp::FastVGICP, registrations.cpp:48-56 */
  DGS_METHOD_ICP = 3,   /* "ICP_HIP": pcl::IterativeClosestPoint, registrations.cpp:59-64 (point-to-point, DESIGN.md "ICP_HIP").  Reads
                           transformation_epsilon, maximum_iterations and gicp_max_correspondence_distance (= setMaxCorrespondenceDistance);
                           the rest of its settings are dgs_icp_options.  The reference's own "ICP" string is not this method. */
  DGS_METHOD_PCL_GICP = 4, /* "GICP_HIP" / "GICP_OMP_HIP": pcl::GeneralizedIterativeClosestPoint, registrations.cpp:65-87 (DESIGN.md
                             "GICP_HIP").  Reads transformation_epsilon, maximum_iterations, gicp_max_correspondence_distance and
                             gicp_correspondence_randomness (k_correspondences_); the rest is dgs_pcl_gicp_options.  The reference's own
                             "GICP" / "GICP_OMP" strings are not this method. */
  DGS_METHOD_PCL_NDT = 5   /* "PCL_NDT_HIP": pcl::NormalDistributionsTransform, the factory's default branch (registrations.cpp:94-100;
                             DESIGN.md 6i): score, gradient and Hessian in double, the neighbourhood always the radius search (centroids
                             within ndt_resolution).  Reads transformation_epsilon, maximum_iterations, ndt_resolution, ndt_step_size,
                             ndt_outlier_ratio, ndt_min_points_per_voxel, ndt_min_covar_eigvalue_mult, ndt_line_search,
                             ndt_mt_max_step_iterations, ndt_fix_hessian_d1, ndt_newton_solver, ndt_guess_rotation_polar, ndt_exp_glibc and
                             ndt_cov_eigensolver; num_threads, ndt_search_method, ndt_strict_order and ndt_hessian_recompute_double are
                             accepted and without effect (the closing computeHessian is always PCL's double pass).  The reference's own
                             strings for this branch ("NDT" and every unknown name) are not this method. */
};

/* fast_gicp::NeighborSearchMethod of FastVGICP (voxel offsets searched around the voxel of T * p) */
enum dgs_vgicp_search { DGS_VGICP_DIRECT1 = 0, DGS_VGICP_DIRECT7 = 1, DGS_VGICP_DIRECT27 = 2 };

/* pclomp::NeighborSearchMethod (registrations.cpp:113-119), same enumerator order as upstream */
enum dgs_ndt_search { DGS_NDT_KDTREE = 0, DGS_NDT_DIRECT26 = 1, DGS_NDT_DIRECT7 = 2, DGS_NDT_DIRECT1 = 3 };

/* NDT step-length control (computeStepLengthMT).
 * MORE_THUENTE (default): the More-Thuente line search as SURVEY.md App. A states it and PCL >= 1.8.1 executes it
 *   (interval check `(step_max - step_min) < 0`).
 * FIXED_STEP: the pre-1.8.1 PCL initialisation `(step_max - step_min) > 0`, which marks the interval converged at
 *   once, so the trial loop never runs and every iteration is one derivative evaluation at the clamped Newton step.
 *   Kept because un-pinned ndt_omp forks differ here; it oscillates on planar scenes (DESIGN.md "NDT sensitivity"). */
enum dgs_ndt_line_search { DGS_NDT_LS_FIXED_STEP = 0, DGS_NDT_LS_MORE_THUENTE = 1 };

/* Order of the per-point arithmetic of NDT computeDerivatives / updateDerivatives (DESIGN.md "Parity").
 * FAST: the <= 7 voxels of a point are folded in float and projected once through the point Jacobian (1/3 of the
 *   flops, FMA contraction allowed, the library expf, Gauss-Jordan Newton solve): the same algebra as upstream, re-associated.
 *   Opt-in: 2.4 x the throughput of UPSTREAM, a few ill-conditioned pairs per 32 land outside 1e-4 m of a CPU run.
 * UPSTREAM (default since ABI 5): every float operation of upstream's per-voxel update in upstream's order, individually rounded (no FMA), a
 *   platform-independent exp, each voxel's increments added to the point's double totals, the full (not exactly symmetric)
 *   6x6 Hessian, Jacobi-SVD Newton solve; the points' totals are summed in the GPU's own fixed order, so only the order of
 *   the double summation differs from a CPU run of upstream.  That order follows the launch: a pair's bits are reproducible only for
 *   an identical batch composition, unless dgs_set_batch_independent.
 * UPSTREAM_SEQUENTIAL: as UPSTREAM, and the per-point totals are written out and summed in point-index order like
 *   upstream's final loop: every evaluation is bit-identical to the CPU restatement (slow: one lane per sum). */
enum dgs_ndt_strict_order { DGS_NDT_ORDER_FAST = 0, DGS_NDT_ORDER_UPSTREAM = 1, DGS_NDT_ORDER_UPSTREAM_SEQUENTIAL = 2 };

/* fast_gicp::RegularizationMethod, same enumerator order as upstream */
enum dgs_gicp_regularization {
  DGS_GICP_REG_NONE = 0, DGS_GICP_REG_MIN_EIG = 1, DGS_GICP_REG_NORMALIZED_MIN_EIG = 2,
  DGS_GICP_REG_PLANE = 3, DGS_GICP_REG_FROBENIUS = 4
};
enum dgs_gicp_optimizer { DGS_GICP_OPT_GAUSS_NEWTON = 0, DGS_GICP_OPT_LEVENBERG_MARQUARDT = 1 };
/* dgs_params.gicp_cov_jacobi_svd: how FAST_GICP / FAST_VGICP form and regularise the k-NN covariances */
enum dgs_gicp_cov_mode {
  DGS_GICP_COV_SYM_EIG = 0,        /* tree sums over the neighbours, symmetric eigen-decomposition (default) */
  DGS_GICP_COV_JACOBI_SVD = 1,     /* tree sums, Eigen::JacobiSVD<Matrix3d> restated */
  DGS_GICP_COV_UPSTREAM_ORDER = 2  /* neighbours in ascending (distance, index) order, summed one after another, JacobiSVD: upstream's operation order */
};

typedef struct dgs_params {
  uint32_t struct_size; /* sizeof(dgs_params), set by dgs_params_init */
  int32_t method;       /* dgs_method */
  int32_t device;       /* HIP device ordinal; -1 = the calling thread's current device */
  int32_t num_threads;  /* reg_num_threads (registrations.cpp:30,102): accepted, ignored on the GPU */

  /* setTransformationEpsilon / setMaximumIterations (registrations.cpp:31-32,110-111) */
  double transformation_epsilon; /* default 0.01 */
  int32_t maximum_iterations;    /* default 64 */

  /* ---- NDT (pclomp::NormalDistributionsTransform) ---- */
  int32_t ndt_search_method;        /* setNeighborhoodSearchMethod; default DGS_NDT_DIRECT7 (registrations.cpp:103) */
  double ndt_resolution;            /* setResolution; factory default 0.5 (registrations.cpp:93) */
  double ndt_step_size;             /* upstream default 0.1 */
  double ndt_outlier_ratio;         /* upstream default 0.55 */
  double ndt_min_covar_eigvalue_mult; /* VoxelGridCovariance default 0.01 */
  int32_t ndt_min_points_per_voxel; /* VoxelGridCovariance default 6 */
  int32_t ndt_line_search;          /* dgs_ndt_line_search, default DGS_NDT_LS_MORE_THUENTE */
  int32_t ndt_mt_max_step_iterations; /* default 10 */
  int32_t ndt_fix_hessian_d1;       /* 0 = upstream h_ang_d1 table (z-term +sy); 1 = exact (-sy) */
  int32_t ndt_strict_order;         /* dgs_ndt_strict_order, default DGS_NDT_ORDER_UPSTREAM */

  /* ---- GICP (fast_gicp::FastGICP) ---- */
  double gicp_max_correspondence_distance; /* setMaxCorrespondenceDistance; factory default 2.5 (registrations.cpp:33); also ICP's
                                              setMaxCorrespondenceDistance (DGS_METHOD_ICP, registrations.cpp:62) */
  double gicp_rotation_epsilon;            /* upstream default 2e-3 */
  double gicp_lm_init_lambda_factor;       /* upstream default 1e-9 */
  int32_t gicp_correspondence_randomness;  /* setCorrespondenceRandomness (k), default 20 (registrations.cpp:34).  Range 1..64 for FAST_GICP,
                                            * FAST_VGICP and GICP_HIP / GICP_OMP_HIP: k <= 32 runs the kernels of every earlier release, 33..64
                                            * their wide forms; k > 64 is DGS_ERR_UNSUPPORTED at the first covariance pass */
  int32_t gicp_regularization;             /* default DGS_GICP_REG_PLANE */
  int32_t gicp_optimizer;                  /* default DGS_GICP_OPT_LEVENBERG_MARQUARDT */
  int32_t gicp_lm_max_iterations;          /* default 10 */
  /* FAST_VGICP (uses the gicp_* fields above except gicp_max_correspondence_distance: VGICP has no distance gate) */
  int32_t vgicp_search_method;             /* default DGS_VGICP_DIRECT1 (FastVGICP constructor) */
  double vgicp_resolution;                 /* setResolution(reg_resolution), factory default 1.0 (registrations.cpp:52) */
  /* ---- six details of un-vendored upstream code behind named switches (ABI 5; [UPSTREAM-RECALL]).  Each
   * defaults to what the published upstream source does as far as it can be recalled; 0 restores the stand-in of ABI <= 4. ---- */
  int32_t ndt_newton_solver;            /* upstream evaluation orders (ndt_strict_order >= 1): 1 = Eigen::JacobiSVD's own two-sided Jacobi sequence
                                           (what computeTransformation's `sv.solve(-score_gradient)` runs); 0 = one-sided Hestenes Jacobi.  The FAST
                                           order keeps its Gauss-Jordan step either way. */
  int32_t ndt_hessian_recompute_double; /* computeStepLengthMT ends with computeHessian when the line search took extra trials: 1 = PCL's double-precision
                                           computeHessian / updateHessian, as ndt_omp kept it; 0 = the float computeDerivatives pass again.  Upstream
                                           orders only (the FAST order re-runs its own float pass). */
  int32_t ndt_guess_rotation_polar;     /* initial pose vector: Euler angles of Affine3f::rotation(), i.e. of the polar factor of the guess's 3x3
                                           (a float JacobiSVD) = 1, of the raw 3x3 = 0.  All orders. */
  int32_t ndt_exp_glibc;                /* upstream evaluation orders: updateDerivatives' `std::exp(float)`: 1 = glibc's expf (>= 2.27, the x86-64 FMA build)
                                           restated operation for operation -- the restatement is compared with the build image's libm on every
                                           float in [-104, 0] (tests/test_oracle_round4.py); 0 = the platform-independent polynomial of ABI <= 4
                                           (correctly rounded but for ~1e-9 of the arguments: NOT what a libm returns).  The FAST order uses the
                                           device library's expf either way.  (Was reserved0: same struct size.) */
  int32_t ndt_cov_eigensolver;          /* voxel covariances (VoxelGridCovariance: `eigensolver.compute(leaf.cov_)`, all orders): 1 = Eigen 3.3's
                                           SelfAdjointEigenSolver<Matrix3d>::compute restated -- scaling, the 3x3 Householder tridiagonalisation,
                                           implicit QR steps with Wilkinson's shift, selection sort; 0 = cyclic Jacobi (ABI <= 4).  The eigenvectors
                                           matter where a flat voxel's covariance is rebuilt from them (eigenvalue clamp). */
  int32_t gicp_cov_jacobi_svd;          /* FAST_GICP / FAST_VGICP covariance regularisation (calculate_covariances): 1 = Eigen::JacobiSVD<Matrix3d> restated (two-sided
                                           Jacobi; the routine fast_gicp calls), 0 (default) = the symmetric eigen-decomposition of ABI <= 4 -- the same factors up to
                                           rounding on regular neighbourhoods.  Not the default because JacobiSVD skips rotations below 2 eps maxDiag: on a rank-deficient
                                           neighbourhood (duplicated points, points on a line) the basis of the null space -- and with it U diag(1, 1, 1e-3) V^T -- then
                                           jumps with the last bit of the input covariance, which the device (8-lane tree sums) and a CPU sum in different orders.
                                           2 (DGS_GICP_COV_UPSTREAM_ORDER) = JacobiSVD fed upstream's bits: each point's neighbours put in ascending (float squared
                                           distance, index) order, mean and covariance summed over them one after another in double, every operation individually
                                           rounded -- the six stored entries are the CPU restatement's (oracle, cov_svd = 1) bit for bit, rank-deficient
                                           neighbourhoods included; slower (one lane per point).  dgs_gicp_cov_mode; fixed at dgs_create.  (Was reserved1.) */
} dgs_params;

/* What the callers read back after align(): hasConverged(), getFinalTransformation(), and the
 * getFitnessScore() the loop detector takes per candidate (loop_detector.hpp:145-155). */
typedef struct dgs_result {
  float final_transformation[16]; /* getFinalTransformation(), column-major */
  int32_t converged;              /* hasConverged() */
  int32_t iterations;             /* nr_iterations_ */
  int32_t evaluations;            /* derivative / linearisation passes as upstream counts them (NDT, upstream orders: repeated More-Thuente trial poses answered from the line search's cache included) */
  int32_t status;                 /* dgs_status of this registration (batch entries fail independently) */
  double score;                   /* NDT: score (trans_probability * Ns); GICP: final sum of Mahalanobis errors */
  double fitness;                 /* getFitnessScore(max_range) when requested, else NaN */
} dgs_result;

/* Defaults = the reference factory's defaults for `method` (registrations.cpp:27-36 / 93-120). */
int dgs_params_init(dgs_params* params, int32_t method);

/* pcl::IterativeClosestPoint settings that dgs_params has no field for (DGS_METHOD_ICP only; dgs_params keeps its size).
 * use_reciprocal_correspondences: setUseReciprocalCorrespondences (registrations.cpp:63), default 0.
 * euclidean_fitness_epsilon: setEuclideanFitnessEpsilon, the relative MSE threshold of DefaultConvergenceCriteria; default -DBL_MAX (never fires).
 * rotation_epsilon: setTransformationRotationEpsilon; 0 (default) = the rotation threshold is 1 - transformation_epsilon. */
typedef struct dgs_icp_options {
  uint32_t struct_size; /* sizeof(dgs_icp_options), set by dgs_icp_options_init */
  int32_t use_reciprocal_correspondences;
  double euclidean_fitness_epsilon;
  double rotation_epsilon;
} dgs_icp_options;
int dgs_icp_options_init(dgs_icp_options* options);

/* pcl::GeneralizedIterativeClosestPoint settings that dgs_params has no field for (DGS_METHOD_PCL_GICP only; dgs_params keeps its size).
 * max_optimizer_iterations: setMaximumOptimizerIterations (registrations.cpp:74), default 20.
 * rotation_epsilon: setRotationEpsilon, default 2e-3 (the GICP constructor's value).
 * gicp_epsilon: the smallest singular value of every regularised covariance, default 1e-3.
 * use_reciprocal_correspondences: setUseReciprocalCorrespondences (registrations.cpp:72), default 0; accepted and without effect, as
 *   upstream (GICP's computeTransformation never reads it). */
typedef struct dgs_pcl_gicp_options {
  uint32_t struct_size; /* sizeof(dgs_pcl_gicp_options), set by dgs_pcl_gicp_options_init */
  int32_t max_optimizer_iterations;
  double rotation_epsilon;
  double gicp_epsilon;
  int32_t use_reciprocal_correspondences;
} dgs_pcl_gicp_options;
int dgs_pcl_gicp_options_init(dgs_pcl_gicp_options* options);

/* new pclomp::NormalDistributionsTransform / fast_gicp::FastGICP + setters (registrations.cpp:29-35,105-119) */
int dgs_create(const dgs_params* params, dgs_handle** out);
void dgs_destroy(dgs_handle* h);
const char* dgs_last_error(const dgs_handle* h); /* never NULL; "" when the last call succeeded */
int dgs_abi_version(void);

/* Settings of an ICP handle, taking effect at the next align; DGS_ERR_UNSUPPORTED on a handle of another method. */
int dgs_set_icp_options(dgs_handle* h, const dgs_icp_options* options);
/* Settings of a GICP_HIP handle, taking effect at the next align; DGS_ERR_UNSUPPORTED on a handle of another method. */
int dgs_set_pcl_gicp_options(dgs_handle* h, const dgs_pcl_gicp_options* options);
/* setCorrespondenceRandomness on a live GICP_HIP handle (dgs_params.gicp_correspondence_randomness): the covariances of the target and
 * of every source are recomputed for the new k at the next align.  DGS_ERR_UNSUPPORTED on a handle of another method, and for k > 64
 * (the handle keeps its k). */
int dgs_pcl_gicp_set_correspondence_randomness(dgs_handle* h, int32_t k);

/* Batch-independent results on request.  Off by default; while it is on, every dgs_result field of a pair, and every
 * fitness, is a function of (method parameters, target, source, guess) alone: batch size, the pair's neighbours in the batch, the launch
 * shape and the entry point (dgs_align, dgs_align_batch*, dgs_align_pairs_clouds, a dgs_group member) do not enter.  May be changed
 * between calls at any time; nothing that is cached on clouds is invalidated.
 *   behaviour changes: FAST_GICP and FAST_VGICP sum a pair over slices that follow its own size -- the layout of a lone default dgs_align,
 *     so a pair of any batch carries the bits of its own single align with the switch OFF; NDT with ndt_strict_order 1 takes the
 *     item-compacted kernel's fixed slices (what DGS_NDT_FIXED_SLICES=1 at dgs_create selects, which keeps giving the initial value).
 *   fitness routing only: NDT order 2, ICP_HIP, GICP_HIP, PCL_NDT_HIP -- their sums are batch-independent already.  For every method,
 *     dgs_get_fitness_score and the fitness of dgs_align_batch* (and of dgs_group_align_batch*) then go through the edge scorer of
 *     dgs_calc_fitness_score_batch_clouds, whose rows follow the edge alone; the value stays within a relative 1e-9 of the default one.
 *   refused: NDT with ndt_strict_order 0 (the re-associated fast order), and order 1 under DGS_NDT_STRICT_KERNEL=2: DGS_ERR_UNSUPPORTED,
 *     the reason in dgs_last_error.  NULL handle or NULL `on`: DGS_ERR_INVALID_ARGUMENT.  No device work in any of the three calls.
 * A target whose index an earlier switch-off batch of ten or more candidates built k-d ordered keeps the covariances made from that index.
 * Additions only: DGS_ABI_VERSION is unchanged. */
int dgs_set_batch_independent(dgs_handle* h, int32_t on);
int dgs_get_batch_independent(const dgs_handle* h, int32_t* on);

/* Run all of this handle's work on a caller-owned hipStream_t (NULL = a stream the handle owns). */
int dgs_set_stream(dgs_handle* h, void* hip_stream);
/* Block until everything this handle enqueued has finished. */
int dgs_synchronize(dgs_handle* h);

/* registration->setInputTarget(cloud): scan_matching_odometry_nodelet.cpp:180,254; loop_detector.hpp:124.
 * NDT: builds the voxel-Gaussian model (VoxelGridCovariance).  GICP: exact-NN index; covariances lazily. */
int dgs_set_input_target(dgs_handle* h, const float* xyz16, int64_t n, int32_t on_device);
/* registration->setInputSource(cloud): scan_matching_odometry_nodelet.cpp:185; loop_detector.hpp:138 */
int dgs_set_input_source(dgs_handle* h, const float* xyz16, int64_t n, int32_t on_device);

/* registration->align(*aligned, guess): scan_matching_odometry_nodelet.cpp:218; loop_detector.hpp:145.
 * `guess16` NULL = identity.  `aligned_xyz16` (nullable) receives final_transformation * source,
 * n_source points (host or device per `aligned_on_device`).  A registration that fails internally reports
 * converged = 0 and final_transformation = guess (the reference treats that as "skip this frame",
 * scan_matching_odometry_nodelet.cpp:222-226). */
int dgs_align(dgs_handle* h, const float* guess16, dgs_result* out, float* aligned_xyz16, int32_t aligned_on_device);

/* registration->getFitnessScore(max_range): loop_detector.hpp:148, scan_matching_odometry_nodelet.cpp:318.
 * Mean squared exact-1-NN distance of final_transformation * source to the target over points with
 * d^2 <= max_range (PCL compares the SQUARED distance with max_range; the reference's in-tree twin does the
 * same, information_matrix_calculator.cpp:97); DBL_MAX when no point qualifies. */
int dgs_get_fitness_score(dgs_handle* h, double max_range, double* score);

/* The inlier loop of publish_scan_matching_status (scan_matching_odometry_nodelet.cpp:321-332):
 * fraction of final_transformation * source points whose exact 1-NN squared distance to the target is
 * < max_sq_dist (the reference passes 0.5 * 0.5). */
int dgs_get_inlier_fraction(dgs_handle* h, double max_sq_dist, double* fraction);

/* registration->getSearchMethodTarget()->nearestKSearch(pt, 1, idx, sqdist) for m query points
 * (scan_matching_odometry_nodelet.cpp:327).  Exact; ties resolve to the lowest target index. */
int dgs_nearest_search_target(dgs_handle* h, const float* queries_xyz16, int64_t m, int32_t on_device,
                              int32_t* indices, float* sq_dists);

/* The candidate loop of LoopDetector::matching (loop_detector.hpp:137-156) as ONE batched call against the
 * current target: for c in [0, n): setInputSource(sources[c]); align(guess[c]); getFitnessScore(max_range).
 * `sources[c]` / `sizes[c]` may be ragged; `guesses16` is n*16 floats (NULL = identity); fitness is computed
 * when `compute_fitness` != 0.  results[c].status reports per-candidate failures.  The arg-min over
 * (converged, fitness) stays with the caller (loop_detector.hpp:149-155). */
int dgs_align_batch(dgs_handle* h, int32_t n, const float* const* sources, const int64_t* sizes, int32_t on_device,
                    const float* guesses16, int32_t compute_fitness, double fitness_max_range, dgs_result* results);

/* ---- device-resident clouds: KeyFrame::cloud kept in HBM -------------------------------------------------
 * The loop detector registers the same keyframe clouds again and again (every graph_update_interval tick,
 * /root/reference/apps/delta_graph_slam_nodelet.cpp:147-148,816; clouds live in KeyFrame::cloud, keyframe.hpp:51).  A dgs_cloud
 * is uploaded once; the exact-NN index and the GICP covariances derived from it are built on first use and kept, which is
 * what fast_gicp does per object when setInputSource sees the same pointer again.  A cloud belongs to the device of the
 * handle that created it, may be used by any handle on that device (one at a time) and must outlive the calls using it. */
int dgs_cloud_create(dgs_handle* h, const float* xyz16, int64_t n, int32_t on_device, dgs_cloud** out);
void dgs_cloud_destroy(dgs_cloud* cloud);
int64_t dgs_cloud_size(const dgs_cloud* cloud);
/* setInputTarget / setInputSource without a copy */
int dgs_set_input_target_cloud(dgs_handle* h, dgs_cloud* cloud);
int dgs_set_input_source_cloud(dgs_handle* h, dgs_cloud* cloud);
/* dgs_align_batch over resident clouds (loop_detector.hpp:137-156 with cached candidates) */
int dgs_align_batch_clouds(dgs_handle* h, int32_t n, dgs_cloud* const* sources, const float* guesses16, int32_t compute_fitness,
                           double fitness_max_range, dgs_result* results);
/* n registrations that each name their own target: pair i = (targets[i], sources[i], guess i), all pairs advancing together in the same
 * round launches (a tick of the loop detector: every new keyframe is a target with a short candidate list of its own).
 * results[i] is what dgs_set_input_target_cloud(targets[i]) followed by dgs_align_batch_clouds over sources[i] alone would report (the
 * sums of a pair are formed by as many workgroups as the batch leaves it, so poses agree to rounding, as between any two batches);
 * fitness is getFitnessScore(fitness_max_range) of source i under its final transform against target i, from one
 * dgs_calc_fitness_score_batch_clouds-style launch over all n edges (bit-identical in any batch).  FAST_GICP and GICP_HIP handles: any
 * other method is DGS_ERR_UNSUPPORTED with the method named in dgs_last_error (their target models live on the handle, not on the cloud).
 * GICP_HIP sums over fixed slices, so its transforms, flags, counts and scores are the bits of dgs_align on the pair alone.
 * One deliberate difference from dgs_set_input_target_cloud + dgs_align there: a target of fewer than k = gicp_correspondence_randomness
 * points fails only the pairs that name it (status DGS_ERR_INVALID_ARGUMENT, transform = guess, as for a source of fewer than k points),
 * the other pairs run and the call returns DGS_OK; k > 32 fails the call with DGS_ERR_UNSUPPORTED.  dgs_pcl_gicp_get_trajectory(pair)
 * afterwards answers for the pairs of this call.
 * n == 0: DGS_OK without a launch.  A NULL cloud or a cloud of another device: DGS_ERR_INVALID_ARGUMENT.  An empty source: status
 * DGS_ERR_NO_SOURCE for that pair, transform = guess; an empty target: DGS_ERR_NO_TARGET for that pair; the other pairs run.  A cloud may be
 * the target of any number of pairs, the source of others, and both sides of one pair.  Missing indices of all clouds are built in one
 * batched build and kept, covariances are made once per cloud and kept (dgs_params.gicp_cov_jacobi_svd is honoured).  The handle's own
 * registration target / source / last result and what dgs_get_counts reports are untouched.  Additions only: DGS_ABI_VERSION is unchanged. */
int dgs_align_pairs_clouds(dgs_handle* h, int32_t n, dgs_cloud* const* targets, dgs_cloud* const* sources, const float* guesses16,
                           int32_t compute_fitness, double fitness_max_range, dgs_result* results);

/* LoopDetector::find_candidates (/root/reference/include/hdl_graph_slam/loop_detector.hpp:83-111) over n keyframes on the device
 * (second half): keyframe i is a candidate iff
 *   new_accum_distance - accum_distance[i] >= accum_distance_thresh            (:93-96: "traveled distance ... too small" skips)
 *   and sqrt(dx * dx + dy * dy) <= distance_thresh, (dx, dy) = xy[i] - new_xy  (:98-105: Eigen's norm() of the 2-D difference, double)
 * `xy` holds n pairs (x, y) = node->estimate().translation().head<2>().  `indices` receives the candidates' positions in KEYFRAME ORDER
 * (the order matters: loop_detector.hpp:149 breaks score ties in favour of the later candidate); *n_out is always the full count,
 * DGS_ERR_INVALID_ARGUMENT when it exceeds `capacity`.  The "too close to the last loop edge" test (:85-87) stays with the caller.
 * Poses change at every graph optimisation, so the arrays travel with the call (host pointers, or device pointers with on_device). */
int dgs_find_loop_candidates(dgs_handle* h, const double* accum_distance, const double* xy, int64_t n, int32_t on_device, double new_accum_distance,
                             const double* new_xy, double accum_distance_thresh, double distance_thresh, int32_t* indices, int64_t capacity, int64_t* n_out);

/* InformationMatrixCalculator::calc_fitness_score(cloud1, cloud2, relpose, max_range)
 * (/root/reference/src/hdl_graph_slam/information_matrix_calculator.cpp:77-108; called per odometry edge and per loop
 * edge, apps/delta_graph_slam_nodelet.cpp:572,820): exact-NN index over cloud1, cloud2 transformed by the float cast of
 * relpose (column-major 16 floats, NULL = identity), mean squared NN distance over points with d^2 <= max_range, DBL_MAX
 * when none qualifies.  Uses buffers of its own: the handle's registration target / source / result are untouched. */
int dgs_calc_fitness_score(dgs_handle* h, const float* cloud1_xyz16, int64_t n1, const float* cloud2_xyz16, int64_t n2,
                           int32_t on_device, const float* relpose16, double max_range, double* score);

/* The same over a batch of edges between device-resident clouds: what one optimisation tick asks for (up to max_keyframes_per_update
 * odometry edges, apps/delta_graph_slam_nodelet.cpp:572, and one per accepted loop, :820).  Edge e is calc_fitness_score(cloud1s[e],
 * cloud2s[e], relpose e, max_range) with exactly dgs_calc_fitness_score's semantics; relposes16 holds n_edges x 16 column-major
 * floats (NULL = identity everywhere); used[e] (nullable) receives the reference's nr, scores[e] DBL_MAX when nr == 0 or a cloud is
 * empty.  A cloud may stand in any number of edges, on either side, on both sides of one edge.  The index over cloud1 is the one the
 * dgs_cloud keeps: built here when it has none (all missing ones in one batched Hilbert-order build), kept for every later user
 * (registration target, loop detection, ICP walks), used as it is when it exists (Hilbert or k-d order).  One walk launch over all
 * edges, one closing launch, one download, one host wait.  An edge's partial rows are a function of its own cloud2 size and are summed
 * in a fixed order, so its (score, used) is bit-identical in any batch, at any position, and alone.  DGS_NN_GRID has no effect here.
 * The handle's registration target / source / result are untouched.  n_edges == 0: DGS_OK without a launch.  A NULL cloud or a cloud
 * of another device: DGS_ERR_INVALID_ARGUMENT. */
int dgs_calc_fitness_score_batch_clouds(dgs_handle* h, int32_t n_edges, dgs_cloud* const* cloud1s, dgs_cloud* const* cloud2s,
                                        const float* relposes16, double max_range, double* scores, int64_t* used);
/* Builds the Hilbert-ordered exact-NN index of every listed cloud that has none, all of them together: a number of launches that
 * follows the deepest cloud, not n; no host wait (the work is enqueued on the handle's stream).  The indices equal, bit for bit,
 * what each cloud would get as a registration target. */
int dgs_cloud_build_indices(dgs_handle* h, int32_t n, dgs_cloud* const* clouds);
/* counts8: of the last dgs_calc_fitness_score_batch_clouds (or dgs_cloud_build_indices) call kernel launches (the radix sort
 * counts as one), host waits, edges, indices built, partial rows; then, not of that call but since dgs_create, the single-cloud index
 * builds this handle made by any other path (registration targets, the prefilter, dgs_calc_fitness_score ...); the rest 0. */
int dgs_fitness_batch_get_counts(dgs_handle* h, int64_t* counts8);
/* The second half of what a resident cloud needs before it can be registered: the k-NN covariances this handle's method and parameters
 * would make of each listed cloud on first use -- FAST_GICP / FAST_VGICP: 6 doubles per point under (reg_correspondence_randomness,
 * regularisation); GICP_HIP / GICP_OMP_HIP: 9 doubles per point under (k, epsilon) -- for all listed clouds together: the missing
 * indices in dgs_cloud_build_indices' batched build, then per chunk of clouds (4 Mi points; DGS_COV_BATCH_POINTS in the environment of
 * dgs_create) one table upload, one search launch and one covariance launch, whatever n.  Enqueued on the handle's stream, no host
 * wait.  The covariances are kept on the cloud for every later user and are, bit for bit, what a lone dgs_set_input_source_cloud +
 * dgs_align would have made.  Dropped from the work: a cloud listed before, an empty cloud, a cloud whose covariances already answer
 * the handle's key, and (GICP_HIP) a cloud of fewer than k points, which stays without covariances.  gicp_cov_jacobi_svd = 2 and the
 * per-query k-NN walk (DGS_KNN_LEAF=0, DGS_KNN_LEAF_WIDE=0) are served one cloud at a time inside the call, results unchanged.
 * Any other method: DGS_ERR_UNSUPPORTED with the method named; reg_correspondence_randomness > 64: DGS_ERR_UNSUPPORTED; a NULL cloud or
 * a cloud of another device: DGS_ERR_INVALID_ARGUMENT, nothing modified; n == 0: DGS_OK without a launch. */
int dgs_cloud_build_covariances(dgs_handle* h, int32_t n, dgs_cloud* const* clouds);
/* counts8: of the last batched covariance pass, explicit (dgs_cloud_build_covariances) or internal (dgs_align_pairs_clouds, a
 * dgs_align_batch* of two or more sources): kernel launches of the pass (index builds are dgs_fitness_batch_get_counts'), host waits
 * (0, unless the previous pass's table upload was still in flight), clouds listed, clouds covered, clouds that had a valid cache,
 * chunks, clouds served by a per-cloud fallback, indices built. */
int dgs_cloud_covariances_get_counts(dgs_handle* h, int64_t* counts8);

/* The inlier count of publish_scan_matching_status (apps/scan_matching_odometry_nodelet.cpp:321-332) over a batch of edges between
 * device-resident clouds, with dgs_calc_fitness_score_batch_clouds' arguments: cloud1 carries the index, cloud2 is moved by the edge's
 * relative pose.  inliers[e] (nullable) = the points of relpose e * cloud2s[e] whose exact 1-NN squared distance in cloud1s[e] is
 * < max_sq_dist (strict, compared in float as dgs_get_inlier_fraction compares it); fractions[e] (nullable) = inliers[e] / size of
 * cloud2s[e].  The count equals dgs_get_inlier_fraction's for the same pair exactly.  An edge with an empty cloud1 or cloud2: fraction
 * NaN, count 0, the other edges run.  Missing indices by the batched build, one walk launch over all edges, one closing launch, one
 * download, one host wait; dgs_fitness_batch_get_counts answers for this call too.  n_edges == 0: DGS_OK without a launch.  A NULL cloud,
 * a cloud of another device or a NaN threshold: DGS_ERR_INVALID_ARGUMENT.  Additions only: DGS_ABI_VERSION is unchanged. */
int dgs_calc_inlier_fraction_batch_clouds(dgs_handle* h, int32_t n_edges, dgs_cloud* const* cloud1s, dgs_cloud* const* cloud2s,
                                          const float* relposes16, double max_sq_dist, double* fractions, int64_t* inliers);

/* Refills n resident clouds in one call: clouds[i] (it exists, possibly empty) afterwards holds input i (sizes[i] points; host arrays, or
 * device arrays with on_device) passed through `filter`: 0 NONE (a copy), 1 VOXELGRID, 2 APPROX_VOXELGRID, both with leaf_size;
 * out_sizes[i] receives its new size.  The cloud's index, walk index and both covariance caches are invalidated; its buffer is kept when
 * it holds sizes[i] points (it is grown to the INPUT size, so a stream of similar scans stops allocating after its first frames); handles
 * that use the cloud as target or source are detached first, as dgs_cloud_destroy detaches them.  An input may not be a listed cloud's
 * own buffer.
 * VOXELGRID: cloud i receives, bit for bit and in the same order, what dgs_voxel_grid_filter(input i, leaf_size) returns -- a grid from
 * the cloud's own bounding box, float sums in point-index order inside a cell, cells in ascending index, non-finite points dropped --
 * from ONE chain of launches over all clouds (boxes, keys, one sort of (cloud, cell) keys, run lengths, centroids) and two host waits
 * whatever n is: the boxes come back to size the grids, then the n sizes.  PCL's overflow test is kept per cloud: if any cloud fails it
 * the call returns DGS_ERR_GRID_TOO_LARGE, dgs_last_error names the cloud's position in the batch, and no cloud has been modified.
 * APPROX_VOXELGRID runs dgs_approx_voxel_grid_filter's routine once per cloud inside the call: identical results, n host waits.
 * The same cloud listed twice, a NULL cloud, a cloud of another device, a negative size, a NULL input of positive size, an unknown filter
 * or a leaf_size that is not positive: DGS_ERR_INVALID_ARGUMENT, nothing modified.  n == 0: DGS_OK without a launch.  Any handle of the
 * clouds' device may make the call; its registration state is untouched.  Additions only: DGS_ABI_VERSION is unchanged. */
int dgs_cloud_assign_batch(dgs_handle* h, int32_t n, const float* const* inputs_xyz16, const int64_t* sizes, int32_t on_device,
                           int32_t filter /* 0 NONE, 1 VOXELGRID, 2 APPROX_VOXELGRID */, float leaf_size, dgs_cloud* const* clouds, int64_t* out_sizes);
/* counts8: of the last dgs_cloud_assign_batch call kernel launches (a sort, a run-length pass and a scan count as one each), host waits,
 * clouds; the rest 0. */
int dgs_cloud_assign_get_counts(dgs_handle* h, int64_t* counts8);
/* The points of a resident cloud, in its order: *n_out is always its size, DGS_ERR_INVALID_ARGUMENT when it exceeds `capacity`. */
int dgs_cloud_read(dgs_handle* h, const dgs_cloud* cloud, float* out_xyz16, int64_t capacity, int32_t out_on_device, int64_t* n_out);

/* pcl::VoxelGrid<PointXYZ> centroid down-sampling, the step right before the path
 * (/root/reference/apps/scan_matching_odometry_nodelet.cpp:83-89,155-165; apps/prefiltering_nodelet.cpp:59-63):
 * cell = floor(p / leaf) as PCL indexes it, output = centroid of every occupied cell in cell-index order, pad lane = 1.
 * Sums are formed in float in point-index order (PCL's std::sort leaves the order inside a cell unspecified).
 * `*n_out` receives the number of cells; fails with DGS_ERR_INVALID_ARGUMENT when out_capacity is smaller. */
int dgs_voxel_grid_filter(dgs_handle* h, const float* in_xyz16, int64_t n, int32_t in_on_device, float leaf_size, float* out_xyz16,
                          int64_t out_capacity, int32_t out_on_device, int64_t* n_out);

/* pcl::ApproximateVoxelGrid<PointXYZ>, the reference's other down-sampling choice
 * (/root/reference/apps/scan_matching_odometry_nodelet.cpp:90-96; apps/prefiltering_nodelet.cpp:64-69): upstream's single pass
 * through a 512-entry history table hashed by the cell, reproduced exactly -- same output points (float sums in point order,
 * divided by the float count) in the same order: a cell is emitted when another cell evicts it from its slot, the rest in slot
 * order at the end.  Same argument conventions as dgs_voxel_grid_filter; the input must be finite (upstream does not check). */
int dgs_approx_voxel_grid_filter(dgs_handle* h, const float* in_xyz16, int64_t n, int32_t in_on_device, float leaf_size, float* out_xyz16,
                                 int64_t out_capacity, int32_t out_on_device, int64_t* n_out);

/* ---- several GPUs of one process: the candidate loop of LoopDetector::matching sharded across devices -------------------------
 * The reference runs loop detection inside the nodelet manager process under main_thread_mutex
 * (/root/reference/apps/delta_graph_slam_nodelet.cpp:797,816; candidate loop loop_detector.hpp:137-156), so the multi-GPU form a
 * nodelet can link is ONE process driving G devices.  A dgs_group owns one dgs_handle, one host thread and one stream per listed
 * device.  dgs_group_set_input_target = loop_detector.hpp:124 on every member (G parallel host->device copies).
 * dgs_group_align_batch deals candidate c to member c mod G, every member runs its share as one dgs_align_batch, the fixed-size
 * result records are exchanged with ncclAllGather (RCCL over xGMI; communicators from ncclCommInitAll, library loaded with
 * dlopen) and returned in ORIGINAL candidate order; best_index / best_score (nullable) receive the arg-min of
 * loop_detector.hpp:126-156 over (converged, fitness) with its tie rule (on an equal score the later candidate wins), -1 /
 * DBL_MAX when no candidate converged.  The fitness_score_thresh test (:162) stays with the caller.  A group whose device list
 * names one device twice (a one-GPU rehearsal), or that cannot load RCCL, gathers on the host instead: same results.
 * Every member writes the records of its share ON THE DEVICE (optimiser state + fitness sums -> record), so the all-gather sends what
 * the kernels left in HBM; the group's functions leave the caller's current HIP device unchanged.
 * Sources and the target are host arrays (KeyFrame::cloud) or, below, clouds resident on the group's devices; a group is used by
 * one thread at a time. */
typedef struct dgs_group dgs_group;
int dgs_group_create(const dgs_params* params, const int32_t* devices, int32_t n_devices, dgs_group** out); /* params->device is ignored */
void dgs_group_destroy(dgs_group* g);
const char* dgs_group_last_error(const dgs_group* g);
int32_t dgs_group_size(const dgs_group* g);
int32_t dgs_group_uses_rccl(const dgs_group* g);               /* 1: the group holds RCCL communicators */
int32_t dgs_group_rccl_ranks(const dgs_group* g);              /* ncclCommCount of the group's communicator (0: no RCCL) */
int32_t dgs_group_last_gather_used_rccl(const dgs_group* g);   /* 1: the last dgs_group_align_batch exchanged its records with ncclAllGather */
dgs_handle* dgs_group_member(dgs_group* g, int32_t k);         /* member k's handle (e.g. for dgs_profile_*); owned by the group */
int dgs_group_set_input_target(dgs_group* g, const float* xyz16, int64_t n);
int dgs_group_set_icp_options(dgs_group* g, const dgs_icp_options* options);   /* dgs_set_icp_options on every member */
int dgs_group_set_pcl_gicp_options(dgs_group* g, const dgs_pcl_gicp_options* options);   /* dgs_set_pcl_gicp_options on every member */
int dgs_group_set_batch_independent(dgs_group* g, int32_t on);   /* dgs_set_batch_independent on every member: a candidate's record is the same whichever member registers it */
int dgs_group_align_batch(dgs_group* g, int32_t n, const float* const* sources, const int64_t* sizes, const float* guesses16,
                          int32_t compute_fitness, double fitness_max_range, dgs_result* results, int32_t* best_index, double* best_score);

/* Keyframe clouds resident on the group's devices.  KeyFrame::cloud is set once and never written again
 * (/root/reference/include/hdl_graph_slam/keyframe.hpp:51) and the same keyframes are candidates tick after tick
 * (apps/delta_graph_slam_nodelet.cpp:816 -> loop_detector.hpp:59-70), so a nodelet uploads each keyframe ONCE:
 *   owner >= 0: one copy, on member owner mod G (a candidate keyframe: owner = its id keeps the shares even);
 *   owner = -1: a copy on every member (the new keyframe, which is every member's target).
 * dgs_group_set_input_target_cloud = loop_detector.hpp:124 on every member; members without a copy take one from a holder, device
 * to device over xGMI, and keep it (a keyframe is a target first and a candidate on later ticks).
 * dgs_group_align_batch_clouds = dgs_group_align_batch without any upload: candidate c runs on member c mod G when that member
 * holds its cloud, else on the cloud's owner; results, arg-min and tie rule as above.  A dgs_group_cloud belongs to the group it
 * was created with (may be destroyed before or after it). */
typedef struct dgs_group_cloud dgs_group_cloud;
int dgs_group_cloud_create(dgs_group* g, const float* xyz16, int64_t n, int32_t owner, dgs_group_cloud** out);
void dgs_group_cloud_destroy(dgs_group_cloud* cloud);
int64_t dgs_group_cloud_size(const dgs_group_cloud* cloud);
int32_t dgs_group_cloud_copies(const dgs_group_cloud* cloud);   /* members that hold a copy */
/* Drops every copy but ONE: the one on member `owner mod G` when that member holds one, else the first holder's (owner < 0: the first
 * holder's).  A new keyframe is every member's target for one tick (dgs_group_set_input_target_cloud leaves a copy on every member); as
 * a candidate of later ticks it needs the one copy on its owner only -- the caller trims it when the tick is over.  A copy still bound to
 * its member as target or source is detached like in dgs_cloud_destroy. */
int dgs_group_cloud_trim(dgs_group* g, dgs_group_cloud* cloud, int32_t owner);
int dgs_group_set_input_target_cloud(dgs_group* g, dgs_group_cloud* cloud);
int dgs_group_align_batch_clouds(dgs_group* g, int32_t n, dgs_group_cloud* const* sources, const float* guesses16, int32_t compute_fitness,
                                 double fitness_max_range, dgs_result* results, int32_t* best_index, double* best_score);

/* ---- measurement hooks (bench.py roofline leg; not part of the reference surface) ---------------------- */
enum dgs_kernel_id {
  DGS_K_NDT_DERIVATIVES = 0, DGS_K_NDT_SOLVE = 1, DGS_K_NDT_VOXEL_BUILD = 2, DGS_K_NN_SEARCH = 3,
  DGS_K_GICP_LINEARIZE = 4, DGS_K_GICP_COVARIANCE = 5, DGS_K_TRANSFORM = 6, DGS_K_COUNT = 7
};
/* When enabled, every launch of a tracked kernel is bracketed by hipEvents on the launch stream. */
int dgs_profile_enable(dgs_handle* h, int32_t enable);
/* Sum of event-measured durations and number of launches since the last dgs_profile_reset (synchronises).
 * DGS_K_GICP_COVARIANCE counts covariance passes, one per cloud: a batched pass (dgs_cloud_build_covariances and the paths that use it)
 * advances the count by the number of clouds it covers and the time by the pass's own; its launches: dgs_cloud_covariances_get_counts. */
int dgs_profile_get(dgs_handle* h, int32_t kernel_id, double* total_ms, int64_t* launches);
int dgs_profile_reset(dgs_handle* h);
/* Counts describing the current problem, for algorithmic-byte accounting:
 * out[0] = target points, out[1] = source points, out[2] = valid voxels V, out[3] = occupied voxels,
 * out[4] = voxel grid cells, out[5] = derivative evaluations of the last align / batch that ran on the device (sum over pairs; ICP: correspondence
 * passes; NDT, upstream orders: the sum of dgs_result.evaluations minus out[6] unless DGS_NDT_REUSE_TRIALS=0), out[6] = NDT, upstream orders:
 * More-Thuente trial poses of the last align / batch that their line search had evaluated before (answered from its cache). */
int dgs_get_counts(dgs_handle* h, int64_t out[8]);

/* Test hooks: single evaluations on the device, so tests can compare kernels with the oracle directly. */
/* NDT computeDerivatives at pose p (6 doubles).  T16 NULL = build the float transform from p. */
int dgs_ndt_derivatives(dgs_handle* h, const double* p6, const float* T16, double* score, double* grad6, double* hess36);
/* NDT computeHessian in PCL's double-precision form at pose p (the pass computeStepLengthMT ends with when a line search took extra
 * trials; dgs_params.ndt_hessian_recompute_double).  Upstream evaluation orders only (DGS_ERR_UNSUPPORTED otherwise). */
int dgs_ndt_hessian_double(dgs_handle* h, const double* p6, double* hess36);
/* The score + gradient evaluation of a More-Thuente trial at pose p, through the kernels of the upstream evaluation orders (which skip the
 * Hessian code for it).  Upstream evaluation orders only (DGS_ERR_UNSUPPORTED otherwise). */
int dgs_ndt_score_gradient(dgs_handle* h, const double* p6, double* score, double* grad6);
/* How a launch of `grid` workgroups is dealt to the pairs of a batch whose active[pair] != 0 (n_pairs host ints; grid >= n_pairs), at most
 * cap_blocks workgroups per pair: out receives 4 ints per wave, 4 waves per workgroup (16 * grid host ints): pair, slice, workgroups per
 * pair -- all -1 for a workgroup without work -- and the number of active pairs, as every wave derives them on the device. */
int dgs_deal_probe(dgs_handle* h, const int32_t* active, int32_t n_pairs, int32_t cap_blocks, int32_t grid, int32_t* out);
/* The same for the cost-ordered dealing of the item-compacted NDT kernel: kinds[pair] in 0..2 is the evaluation kind the pair waits for.  The
 * active pairs are ranked by (cost class, heaviest first; pair index) and workgroup b serves slice b % per of the pair of rank b / per.
 * order3 (may be NULL) receives the kinds from the heaviest class to the lightest, as the library was built. */
int dgs_deal_probe_cost(dgs_handle* h, const int32_t* active, const int32_t* kinds, int32_t n_pairs, int32_t cap_blocks, int32_t grid, int32_t* out, int32_t* order3);
/* The block reduction behind an evaluation of the upstream evaluation order: one workgroup of 256 threads reduces totals[256][43] (host doubles,
 * a thread's 43 sums per row) to one row of `ncol` column sums (1..43), twice: rows2[0..47] through the passes of the item-compacted kernel
 * (as wide as a wave's table region allows), rows2[48..95] through the stand-alone form's passes of 11 columns.  Entries at and behind ncol
 * are 0.  A column is the sum of its 64 entries per wave in thread order, the four waves' sums added in wave order, in both. */
int dgs_strict_row_probe(dgs_handle* h, const double* totals, int32_t ncol, double* rows2);
/* DGS_METHOD_PCL_NDT handles are served by dgs_ndt_derivatives (its evaluation with the Hessian; hess36 == NULL asks for the score +
 * gradient evaluation of a More-Thuente trial), dgs_ndt_hessian_double, dgs_ndt_get_trajectory and dgs_ndt_get_voxels as well.
 * Test hook of such a handle: the neighbourhood of `m` query points (x y z pad, taken as they are: no transform) in the current
 * target's voxel model as the evaluation kernel finds it -- counts[i] valid voxels whose float centroid lies within ndt_resolution of
 * query i, their numbers (rows of dgs_ndt_get_voxels) in voxel_ids[27 i ..] in ascending order, the rest of the row -1.  counts and
 * voxel_ids are host arrays.  DGS_ERR_UNSUPPORTED on a handle of another method. */
int dgs_pcl_ndt_neighbours(dgs_handle* h, const float* queries_xyz16, int64_t m, int32_t on_device, int32_t* counts, int32_t* voxel_ids);
/* NDT pose (x, y, z, rx, ry, rz) after every outer iteration of pair `pair` of the last align / align_batch;
 * poses6 holds up to 72 x 6 doubles, *len receives the number written (entry 0 is the initial guess). */
int dgs_ndt_get_trajectory(dgs_handle* h, int32_t pair, double* poses6, int32_t* len);
/* ICP: for every iteration of pair `pair` of the last align / align_batch, the incremental transform T_k (16 floats, column-major),
 * that iteration's MSE and its number of kept correspondences.  Up to `capacity` entries are written; *len receives the iteration count. */
int dgs_icp_get_trajectory(dgs_handle* h, int32_t pair, float* T16s, double* mse, int32_t* n_corr, int32_t capacity, int32_t* len);
/* GICP_HIP: the next dgs_pcl_gicp_evaluate runs its correspondence pass at transformation_ = T16 and guess = guess16 (column-major; NULL =
 * identity).  Both stay set until changed. */
int dgs_pcl_gicp_set_probe(dgs_handle* h, const float* T16, const float* guess16);
/* GICP_HIP: one correspondence pass over the handle's source and target at the probe's transformation_ / guess, then f and its gradient
 * at state x6 = (tx, ty, tz, roll, pitch, yaw) over that pass's *m kept pairs (OptimizationFunctorWithIndices, on the device). */
int dgs_pcl_gicp_evaluate(dgs_handle* h, const double* x6, int32_t* m, double* f, double* g6);
/* GICP_HIP: for every outer iteration of pair `pair` of the last align / align_batch: transformation_ (16 floats, column-major), the kept
 * pairs, BFGS inner iterations, evaluation passes and the last f.  Up to `capacity` entries; *len receives the outer iteration count. */
int dgs_pcl_gicp_get_trajectory(dgs_handle* h, int32_t pair, float* T16s, int32_t* n_corr, int32_t* inner, int32_t* passes, double* f,
                                int32_t capacity, int32_t* len);
/* NDT voxel table dump.  First call with NULL arrays returns the number of occupied voxels in *n. */
int dgs_ndt_get_voxels(dgs_handle* h, int64_t* n, int64_t* keys, int32_t* counts, int32_t* valid, double* mean3,
                       double* icov9);

/* Test hook: squared exact 1-NN distances of m query points to the target through the index the fitness pass uses (the
 * one-lane-per-query grid of nn_grid.hip with its tree fallback); must equal dgs_nearest_search_target's sq_dists bit for bit. */
int dgs_nn_fitness_distances(dgs_handle* h, const float* queries_xyz16, int64_t m, int32_t on_device, float* sq_dists);

/* GICP regularised k-NN covariances (FastGICP::calculate_covariances): which = 0 source, 1 target;
 * cov9 receives 9 doubles (row-major 3x3) per point.  On a GICP_HIP handle: pcl::GeneralizedIterativeClosestPoint's covariances. */
int dgs_gicp_get_covariances(dgs_handle* h, int32_t which, double* cov9);
/* GICP FastGICP::linearize (error_only = 0: new correspondences at the pose; returns sum of errors, H 6x6, b 6) or
 * FastGICP::compute_error (error_only = 1: correspondences / Mahalanobis matrices of the last linearisation).
 * The pose is a row-major double 4x4 (Eigen::Isometry3d).  With DGS_METHOD_VGICP the same calls are FastVGICP's. */
int dgs_gicp_linearize(dgs_handle* h, const double* T16_rowmajor, int32_t error_only, double* error, double* hess36, double* b6);
/* Test hook (FAST_VGICP): the target's Gaussian voxel map in ascending (z, y, x) voxel-coordinate order: coord3 int32[3], counts,
 * mean double[3], cov double[9] per voxel; *n_voxels is always set, arrays are filled when capacity suffices. */
int dgs_vgicp_get_voxels(dgs_handle* h, int64_t capacity, int32_t* coord3, int32_t* counts, double* mean3, double* cov9, int64_t* n_voxels);

/* ---- PrefilteringNodelet::cloud_callback on the device (/root/reference/apps/prefiltering_nodelet.cpp:111-164) ---------------
 * The chain from the distance filter to flatten: distance filter (:275-291) -> down-sampling (:249-260) -> outlier removal
 * (:262-273) = /filtered_points; then height filter (:192-212) -> normal filter (:217-245) -> flatten (:166-188) =
 * /flat_filtered_points.  Deskewing and the base_link transform stay with the caller, which passes lidar_position
 * (Eigen::Vector3d, 3 doubles; NULL = origin).  Every pass-through filter keeps the input order and copies the whole 16-byte point.
 * The prefilter works in buffers and an NN index of its own: the handle's registration target / source / NDT model / results are
 * untouched (as dgs_calc_fitness_score).  Semantics, including the PCL 1.10 details recalled from upstream: DESIGN.md §6c. */
enum dgs_prefilter_downsample { DGS_PF_DOWNSAMPLE_NONE = 0, DGS_PF_DOWNSAMPLE_VOXELGRID = 1, DGS_PF_DOWNSAMPLE_APPROX_VOXELGRID = 2 };
enum dgs_prefilter_outlier { DGS_PF_OUTLIER_NONE = 0, DGS_PF_OUTLIER_STATISTICAL = 1, DGS_PF_OUTLIER_RADIUS = 2 };
/* Defaults (dgs_prefilter_params_init) = initialize_params (:55-109): VOXELGRID 0.1, STATISTICAL 20 / 1.0, RADIUS 0.8 / 2,
 * distance 1.0 .. 100.0.  use_distance_filter is read upstream (:100) but the filter runs unconditionally (:153): accepted, ignored.
 * radius_inclusive: RadiusOutlierRemoval keeps a point iff its k-th neighbour distance d^2 <= r^2 (1, PCL 1.10) or < r^2 (0).
 * statistical_sqrt_float: StatisticalOutlierRemoval sums sqrt of the float d^2 in float (1, PCL 1.10's sqrt(float)) or in double (0). */
typedef struct dgs_prefilter_params {
  uint32_t struct_size;             /* sizeof(dgs_prefilter_params), set by dgs_prefilter_params_init */
  int32_t downsample_method;        /* dgs_prefilter_downsample */
  double downsample_resolution;
  int32_t outlier_removal_method;   /* dgs_prefilter_outlier */
  int32_t statistical_mean_k;
  double statistical_stddev;
  double radius_radius;
  int32_t radius_min_neighbors;
  int32_t use_distance_filter;
  double distance_near_thresh;
  double distance_far_thresh;
  int32_t radius_inclusive;
  int32_t statistical_sqrt_float;
} dgs_prefilter_params;
int dgs_prefilter_params_init(dgs_prefilter_params* params);
/* The whole chain.  out3d receives /filtered_points, out2d /flat_filtered_points (host arrays, or device pointers with
 * out_on_device); *n3d_out / *n2d_out are always the full counts, DGS_ERR_INVALID_ARGUMENT when one exceeds its capacity.
 * DGS_ERR_INVALID_ARGUMENT also for STATISTICAL with 0 < points <= statistical_mean_k, and for k-NN sizes above 32
 * (statistical_mean_k + 1, radius_min_neighbors + 1). */
int dgs_prefilter(dgs_handle* h, const dgs_prefilter_params* params, const float* in_xyz16, int64_t n, int32_t in_on_device, const double* lidar_xyz,
                  float* out3d_xyz16, int64_t cap3d, float* out2d_xyz16, int64_t cap2d, int32_t out_on_device, int64_t* n3d_out, int64_t* n2d_out);
/* Single stages (same argument conventions; the inputs of the k-NN stages must be finite, as the chain guarantees). */
int dgs_prefilter_distance(dgs_handle* h, const float* in_xyz16, int64_t n, int32_t in_on_device, double near_thresh, double far_thresh, float* out_xyz16,
                           int64_t out_capacity, int32_t out_on_device, int64_t* n_out);
int dgs_prefilter_radius(dgs_handle* h, const float* in_xyz16, int64_t n, int32_t in_on_device, double radius, int32_t min_neighbors, int32_t inclusive,
                         float* out_xyz16, int64_t out_capacity, int32_t out_on_device, int64_t* n_out);
int dgs_prefilter_statistical(dgs_handle* h, const float* in_xyz16, int64_t n, int32_t in_on_device, int32_t mean_k, double stddev_mul, int32_t sqrt_float,
                              float* out_xyz16, int64_t out_capacity, int32_t out_on_device, int64_t* n_out);
/* normal_filtering (:217-245) alone: NormalEstimation with k = 10 over the given cloud, viewpoint lidar_xyz, keep |n.z| < 0.2f. */
int dgs_prefilter_normal(dgs_handle* h, const float* in_xyz16, int64_t n, int32_t in_on_device, const double* lidar_xyz, float* out_xyz16,
                         int64_t out_capacity, int32_t out_on_device, int64_t* n_out);
/* Test hooks over the last statistical pass: per-point mean neighbour distances (input order) and stats4 = {mean, stddev, threshold,
 * points}; and over the last normal pass: per-point normals4 (the normalised, flipped normal; NaN where upstream's is NaN) and the
 * 9 floats of computeMeanAndCovarianceMatrix (row-major).  *n is always set; arrays (nullable) are filled when capacity suffices. */
int dgs_prefilter_get_statistics(dgs_handle* h, float* mean_distances, int64_t capacity, double* stats4, int64_t* n);
int dgs_prefilter_get_normals(dgs_handle* h, float* normals4, float* cov9, int64_t capacity, int64_t* n);

/* ---- The raw scan: deskewing (apps/prefiltering_nodelet.cpp:293-354) and the base_link_frame transform (:122-150) in front of the
 * chain, fused into the distance filter's pass over the raw cloud.  Semantics: DESIGN.md §6c.
 * deskew_norm_order replaces the squaredNorm inside delta_q.inverse() (:347): its association over the quaternion coefficients
 *   stored (x, y, z, w) [UPSTREAM-RECALL, Eigen 3.3 with SSE3]. */
enum dgs_prefilter_norm_order {
  DGS_PF_NORM_PAIRS_XY_ZW = 0, /* (x² + y²) + (z² + w²): hadd(hadd), the default */
  DGS_PF_NORM_PAIRS_XZ_YW = 1, /* (x² + z²) + (y² + w²) */
  DGS_PF_NORM_SEQUENTIAL = 2   /* ((x² + y²) + z²) + w² */
};
/* Replaces the per-scan state of deskewing (:330-331 ang_v, :340 scan_period) and of the transform (:137-146 transform_isometry).
 * has_angular_velocity = 0 is the nodelet's empty IMU queue (:295-297): the input bits pass untouched, which a zero angular velocity
 * does not promise (-0.0f comes out +0.0f).  transform is the row-major 4 x 4 double matrix handed to pcl::transformPointCloud
 * (:146), taken as given: the caller zeroes m(0,3) and m(1,3) (:141-142).  transform_sets_w: the transformed point's fourth float is
 * 1.0f (1, PCL 1.10 [UPSTREAM-RECALL]) or the input's (0); a non-finite point is copied whole either way.
 * Defaults (dgs_prefilter_scan_params_init): neither step, scan_period 0.1, identity, norm order 0, sets_w 1. */
typedef struct dgs_prefilter_scan_params {
  uint32_t struct_size;          /* sizeof(dgs_prefilter_scan_params), set by dgs_prefilter_scan_params_init */
  int32_t has_angular_velocity;
  double angular_velocity[3];    /* imu_msg->angular_velocity x, y, z as received (the sign flip of :331 is applied inside) */
  double scan_period;
  int32_t has_transform;
  double transform[16];
  int32_t deskew_norm_order;     /* dgs_prefilter_norm_order */
  int32_t transform_sets_w;
} dgs_prefilter_scan_params;
/* Replaces the defaults deskewing reads: scan_period 0.1 (:340), no IMU message (:295), an empty base_link_frame (:104, :123). */
int dgs_prefilter_scan_params_init(dgs_prefilter_scan_params* params);
/* Replaces cloud_callback from :120 to :160: deskewing, the base_link transform, then dgs_prefilter's chain with
 * lidar_position = transform.translation() (:143; zero without a transform, :113), which lidar_xyz_out (3 doubles, nullable)
 * receives.  Argument and error conventions are dgs_prefilter's; a wrong struct_size of either struct or a deskew_norm_order
 * outside 0..2 is DGS_ERR_INVALID_ARGUMENT.  The raw cloud is read by the head's two kernels only and no deskewed or transformed
 * cloud is stored; with neither step enabled the result is dgs_prefilter's with a zero lidar_xyz. */
int dgs_prefilter_scan(dgs_handle* h, const dgs_prefilter_params* chain_params, const dgs_prefilter_scan_params* scan_params, const float* in_xyz16,
                       int64_t n, int32_t in_on_device, float* out3d_xyz16, int64_t cap3d, float* out2d_xyz16, int64_t cap2d, int32_t out_on_device,
                       int64_t* n3d_out, int64_t* n2d_out, double* lidar_xyz_out);
/* Replaces deskewing (:340-351) and pcl::transformPointCloud (:146) alone: every point at its own place, non-finite ones included,
 * *n_out == n.  For tests, and for callers that publish the deskewed cloud. */
int dgs_prefilter_deskew(dgs_handle* h, const dgs_prefilter_scan_params* scan_params, const float* in_xyz16, int64_t n, int32_t in_on_device,
                         float* out_xyz16, int64_t out_capacity, int32_t out_on_device, int64_t* n_out);

/* ---- dgs_prefilter_scan over many scans in one device call: the frames of several streams ------------------------
 * Scan i receives, bit for bit and in the same order, what dgs_prefilter_scan(h, chain_params, &scan_params[i], in_xyz16[i], sizes[i],
 * ...) writes: out3d_xyz16[i] / out2d_xyz16[i] (capacities cap3d[i] / cap2d[i]), n3d_out[i] / n2d_out[i] and lidar_xyz_out[3 i ..]
 * (nullable); with scan_params == NULL, what dgs_prefilter with a zero lidar_xyz writes.  One chain parameter set serves all scans,
 * the head is per scan.  A scan's result depends on neither its place in the batch nor the other scans.  The launches and host waits
 * of a call follow the parameter set, the deepest index among the scans and the number of chunks, not n_scans.
 * status_out[i] (one per scan) is what the single call would have returned for scan i; a per-scan condition does not fail the call
 * and the other scans run: STATISTICAL with 0 < points <= statistical_mean_k (DGS_ERR_INVALID_ARGUMENT, counts 0) and an output
 * capacity too small (DGS_ERR_INVALID_ARGUMENT, the full counts are reported).  An empty scan, and a scan that a stage empties, end
 * with counts 0 and DGS_OK.
 * DGS_ERR_INVALID_ARGUMENT with nothing written: a wrong struct_size of the chain parameters or of any head, a deskew_norm_order out
 * of range, k-NN sizes above 32, a NULL array, a negative size, a NULL input of positive size, more than 2^31 points in total.
 * n_scans == 0 is DGS_OK without a launch.  A grid too large for VOXELGRID in any scan fails the call (DGS_ERR_GRID_TOO_LARGE).
 * Own buffers on the handle: registration state and the single call's scratch are untouched; afterwards dgs_prefilter_get_statistics
 * and dgs_prefilter_get_normals report n = 0.  Additions only: DGS_ABI_VERSION is unchanged. */
int dgs_prefilter_scan_batch(dgs_handle* h, const dgs_prefilter_params* chain_params, int32_t n_scans,
                             const dgs_prefilter_scan_params* scan_params /* n_scans entries; NULL: no head, lidar position zero */,
                             const float* const* in_xyz16, const int64_t* sizes, int32_t in_on_device, float* const* out3d_xyz16, const int64_t* cap3d,
                             float* const* out2d_xyz16, const int64_t* cap2d, int32_t out_on_device, int64_t* n3d_out, int64_t* n2d_out,
                             double* lidar_xyz_out /* 3 per scan, nullable */, int32_t* status_out /* one per scan */);
/* counts8 of the last batch call: [0] kernel launches (a library sort, run-length pass or scan counts as one each), [1] host waits,
 * [2] scans listed, [3] scans that ran the whole chain (reached the normal filter), [4] scans served by a per-scan fallback
 * (APPROX_VOXELGRID, DGS_KNN_LEAF=0: every scan of the chunk), [5] chunks (DGS_PREFILTER_BATCH_POINTS raw points each, default
 * 4 Mi), [6] indices built, [7] reserved. */
int dgs_prefilter_batch_get_counts(dgs_handle* h, int64_t* counts8);
/* {mean, stddev, threshold, points} of every scan's statistical pass in the last batch call, zeros where that pass did not run.
 * *n_scans is always set; the array (nullable) is filled when capacity_scans suffices. */
int dgs_prefilter_batch_get_statistics(dgs_handle* h, double* stats4_per_scan, int64_t capacity_scans, int64_t* n_scans);

/* ---- MapCloudGenerator::generate on the device (src/hdl_graph_slam/map_cloud_generator.cpp:13-50) ------------
 * Every keyframe cloud transformed by its pose (pose.matrix().cast<float>(), w = 1, no FMA), concatenated in keyframe and point
 * order, inserted into a pcl::octree::OctreePointCloud of `resolution` and replaced by the centres of the occupied voxels in the
 * octree's depth-first order; with resolution <= 0 the concatenation itself is the result.  The keyframe clouds are read in place
 * (the concatenation is never built when resolution > 0); only the poses travel.  The map works in buffers of its own: the
 * handle's registration target / source / NDT model / results and the prefilter's scratch are untouched.
 * Semantics, including the PCL 1.10 details recalled from upstream ([UPSTREAM-RECALL]): DESIGN.md §6d.  Each recalled detail whose
 * error would change the output is a field here (1 = as recalled, the default):
 *   first_box_oversize:       the first finite point p defines [p - res/2, p + res/2]; getKeyBitSize, with no leaves yet, widens it
 *                             by the oversize res/2 on both sides to [p - res, p + res] (1), or sets max = min + 2 res (0).
 *   grow_shift_without_upper: a growth moves min by the side length on every axis WITHOUT an upper violation (1), or only on the
 *                             axes with a lower violation (0).
 *   max_minus_epsilon:        after a growth max = min + (side - FLT_EPSILON) (1), or min + side (0).
 *   child_index_x_msb:        child index (x_bit << 2) | (y_bit << 1) | z_bit (1), or (z_bit << 2) | (y_bit << 1) | x_bit (0).
 *   key_at_insertion:         a leaf stays where genOctreeKeyforPoint put it under the box of the moment it was inserted, and later
 *                             growths move it by whole voxels (1); or every key is made with the final min (0).
 * dedup_method: DGS_MAP_DEDUP_AUTO = the hash table when twice the points fit 2^26 slots, else the sort of all keys; a table that
 * overflows (a probe sequence longer than 4,096) is also redone by the sort.  HASH: the table, clamped to 2^26 slots; SORT: the sort.
 * hash_slots (test hook): slots of the table, rounded up to a power of two; 0 = sized from the point count. */
enum dgs_map_dedup { DGS_MAP_DEDUP_AUTO = 0, DGS_MAP_DEDUP_HASH = 1, DGS_MAP_DEDUP_SORT = 2 };
typedef struct dgs_map_cloud_params {
  uint32_t struct_size; /* sizeof(dgs_map_cloud_params), set by dgs_map_cloud_params_init */
  int32_t first_box_oversize;
  int32_t grow_shift_without_upper;
  int32_t max_minus_epsilon;
  int32_t child_index_x_msb;
  int32_t key_at_insertion;
  int32_t dedup_method; /* dgs_map_dedup */
  int64_t hash_slots;
} dgs_map_cloud_params;
int dgs_map_cloud_params_init(dgs_map_cloud_params* params);
/* clouds[k]: xyz16 points of keyframe k (sizes[k] <= INT32_MAX of them; host arrays, or device pointers with in_on_device; NULL
 * allowed where sizes[k] == 0); poses16: 16 doubles per keyframe, COLUMN-major (Eigen::Isometry3d::matrix()), cast to float here.
 * *n_out = points of the map, which stays on the handle until the next map call: read it with dgs_map_cloud_get.
 * n_keyframes == 0 is not an error and gives 0 (the callers' layers return null, as upstream :14-17).  A span that needs an octree
 * deeper than 21 levels is DGS_ERR_GRID_TOO_LARGE: nothing is produced, the handle stays usable. */
int dgs_map_cloud_generate(dgs_handle* h, const dgs_map_cloud_params* params, int32_t n_keyframes, const float* const* clouds, const int64_t* sizes,
                           int32_t in_on_device, const double* poses16, double resolution, int64_t* n_out);
/* The same over resident clouds (on the handle's device); they are not modified, their indices and covariances stay valid. */
int dgs_map_cloud_generate_clouds(dgs_handle* h, const dgs_map_cloud_params* params, int32_t n_keyframes, dgs_cloud* const* clouds,
                                  const double* poses16, double resolution, int64_t* n_out);
/* Copies the last map out (host array, or device pointer with out_on_device).  *n is always the full count;
 * DGS_ERR_INVALID_ARGUMENT when it exceeds `capacity` (capacity 0 with a NULL array asks for the count alone). */
int dgs_map_cloud_get(dgs_handle* h, float* out_xyz16, int64_t capacity, int32_t out_on_device, int64_t* n);
/* Test hook over the last map with resolution > 0: the octree's final bounding box (3 + 3 doubles), depth and the number of
 * growths (new roots); all zero after a concatenation or an empty map.  Every pointer is nullable. */
int dgs_map_cloud_get_grid(dgs_handle* h, double* min3, double* max3, int32_t* depth, int32_t* growths);

/* ---- LineBasedScanmatcher::line_extraction on the device (src/hdl_graph_slam/line_based_scanmatcher.cpp:299-457) --------------
 * Repeats, while at least min_cluster_size points remain: a RANSAC line fit (pcl::SACSegmentation, SACMODEL_LINE, optimised
 * coefficients), a Euclidean clustering of its inliers, the distance statistics of the biggest cluster and its removal.  Semantics,
 * the PCL 1.10 details recalled from upstream and the two places where this differs on purpose (stalls): DESIGN.md 6e.
 * The extractor works in buffers of its own: the handle's registration target / source / results, the prefilter's scratch and the
 * map are untouched.  Additions only: DGS_ABI_VERSION is unchanged. */
enum dgs_line_extraction_status {
  DGS_LE_DONE = 0,          /* fewer than min_cluster_size points remain: upstream's loop condition */
  DGS_LE_RANSAC_FAILED = 1, /* a round drew 1000 bad samples in a row (upstream reads an empty coefficient vector there) */
  DGS_LE_STALL = 2,         /* every cluster of a round was larger than max_cluster_size (upstream loops forever there) */
  DGS_LE_MAX_ROUNDS = 3,    /* the max_rounds safety cap */
  DGS_LE_RNG_EXHAUSTED = 4  /* the caller's rng_raw stream ran out */
};
/* Defaults (dgs_line_extraction_params_init) = LineBasedScanmatcher's constructor (line_based_scanmatcher.hpp:80-89): 25, 25000,
 * 1.0f, 0.1f, 500, 150, 1.0, SAC_RANSAC; any-axis sample test, norm order 0, inclusive clustering, 4096 rounds. */
typedef struct dgs_line_extraction_params {
  uint32_t struct_size;          /* sizeof(dgs_line_extraction_params), set by dgs_line_extraction_params_init */
  int32_t min_cluster_size;
  int32_t max_cluster_size;
  float cluster_tolerance;
  float sac_distance_threshold;
  int32_t max_iterations;
  float merror_threshold;        /* a line is emitted iff mean_error < merror_threshold ... */
  float line_length_threshold;   /* ... and |A - B| > line_length_threshold (upstream spells it line_lenght_threshold) */
  int32_t sac_method_type;       /* only 0 (pcl::SAC_RANSAC) is served: anything else is DGS_ERR_INVALID_ARGUMENT */
  int32_t sample_good_any_axis;  /* 1: a sample is good when its points differ in x OR y OR z (later PCL); 0: x AND y AND z (recalled
                                    for PCL 1.10), which never accepts a sample of a flattened cloud */
  int32_t sqnorm_order;          /* dgs_prefilter_norm_order of the squared norm in the inlier test (its w term is 0).  For a flattened
                                    cloud (z = 0 everywhere) two of the three terms are +-0 and every association gives the same bits */
  int32_t cluster_inclusive;     /* 1: two points are linked iff d2 <= tolerance^2, 0: d2 < tolerance^2 (dgs_prefilter_radius' convention) */
  int32_t max_rounds;            /* safety cap on the rounds of one extraction */
  int32_t record_lists;          /* test hook: keep every round's inlier and cluster index lists (one more host wait per round) */
} dgs_line_extraction_params;
int dgs_line_extraction_params_init(dgs_line_extraction_params* params);
/* upstream's LineFeature: pointA, pointB, mean_error, std_sigma, max_error, min_error */
typedef struct dgs_line_feature {
  double point_a[3];
  double point_b[3];
  double mean_error;
  double std_sigma;
  double max_error;
  double min_error;
} dgs_line_feature;
/* in_xyz16: n xyz16 points (host array, or device pointer with in_on_device), e.g. dgs_prefilter's 2-D output; it is not modified.
 * rng_raw (nullable): rng_len values that stand in for boost::mt19937(12345)() >> 1, restarted every round like the generator;
 * running past its end ends the extraction with DGS_LE_RNG_EXHAUSTED.  lines: room for `capacity` features; more lines than that is
 * DGS_ERR_INVALID_ARGUMENT.  *status_out (nullable): dgs_line_extraction_status.  Whatever the status, the lines found so far are
 * returned with DGS_OK. */
int dgs_line_extraction(dgs_handle* h, const dgs_line_extraction_params* params, const float* in_xyz16, int64_t n, int32_t in_on_device,
                        const uint32_t* rng_raw, int64_t rng_len, dgs_line_feature* lines, int64_t capacity, int64_t* n_lines,
                        int32_t* status_out);
/* Test hook: one record per round of the last extraction. */
typedef struct dgs_line_extraction_round {
  int32_t n_before;    /* points the round started with */
  int32_t draws;       /* samples drawn (two raw values each) */
  int32_t iterations;  /* hypotheses walked */
  int32_t sample0;     /* the winner's two point indices (-1 when the round failed) */
  int32_t sample1;
  int32_t inliers;
  int32_t cluster;     /* size of the cluster taken (0: none) */
  int32_t emitted;
} dgs_line_extraction_round;
/* rounds: room for `capacity` records (nullable); *n_rounds is always the full count.  With record_lists, the inlier and cluster
 * index lists (positions in the round's cloud, ascending) of round `list_round` are copied to inlier_idx / cluster_idx when those
 * are non-NULL (room for the round's `inliers` / `cluster` entries).  counts4 (nullable): kernel launches, host waits, rounds
 * launched (re-launches with a longer draw list included) and library sort calls of the last extraction. */
int dgs_line_extraction_get_rounds(dgs_handle* h, dgs_line_extraction_round* rounds, int64_t capacity, int64_t* n_rounds, int32_t list_round,
                                   int32_t* inlier_idx, int32_t* cluster_idx, int64_t* counts4);

/* ---- LineBasedScanmatcher::align_global on the device (src/hdl_graph_slam/line_based_scanmatcher.cpp:109-203) ------------------
 * The target lines are merged (host, order-dependent), the edges of both sides are extracted (on the host, or with
 * params->edges_on_device on the device: one more host wait, which reads the two edge counts back), every (source edge, target edge)
 * hypothesis h = es * Et + et is aligned, gated and scored on the device, the strict arg-max over h is taken there, and the
 * refinement pass over the aligned lines runs on the host.  Semantics, the Eigen details recalled from upstream and the limits:
 * DESIGN.md 6f.  The aligner works in buffers of its own: registration, prefilter, map and line-extraction state are untouched.
 * Additions only: DGS_ABI_VERSION is unchanged. */
enum dgs_line_align_status {
  DGS_LA_ALIGNED = 0,       /* an edge-pair hypothesis beat the identity's score */
  DGS_LA_NO_HYPOTHESES = 1, /* one side has no edges */
  DGS_LA_ALL_GATED = 2,     /* every hypothesis failed a gate */
  DGS_LA_NONE_BETTER = 3,   /* no surviving hypothesis scored strictly above the identity */
  DGS_LA_LINE_ALIGNED = 4   /* align_local: no edge pair took over, a line pair of the second phase did */
};
enum dgs_line_align_gate {
  DGS_LA_GATE_PASS = 0,
  DGS_LA_GATE_DISTANCE = 1, /* translation.norm() > max_distance */
  DGS_LA_GATE_IDENTITY = 2, /* transform == Identity */
  DGS_LA_GATE_ANGLE = 3,    /* constrain_angle (align_local: always) and cos(angle) < cos(max_angle) */
  DGS_LA_GATE_LINE_DIRECTION = 4, /* align_local's line pairs: |cos| between the two directions < cos(max_angle) */
  DGS_LA_GATE_LINE_DISTANCE = 5,  /* align_local's line pairs: align_lines' translation.norm() > max_distance */
  DGS_LA_GATE_RANK = 6,     /* align_local's line pairs with refine_three_nearest: a neighbour of rank >= 3, not visited */
  DGS_LA_GATE_OVERLAP = 7   /* align_overlapped: the angle gate passed, the moved source still overlaps the target */
};
#define DGS_LA_MAX_LINES_SOURCE 256       /* what limits Ls, Lt and the hypothesis count */
#define DGS_LA_MAX_LINES_TARGET 512       /* after merging */
#define DGS_LA_MAX_HYPOTHESES (1 << 21)
/* Defaults (dgs_line_align_params_init) = LineBasedScanmatcher's constructor (line_based_scanmatcher.hpp:91-95): 0.6, 1.0, 0.2, 5.0,
 * 5.0; align_global's constants 2.0 and pi / 9 (:115-116); the float angle chain; ties to the lowest target index. */
typedef struct dgs_line_align_params {
  uint32_t struct_size;            /* sizeof(dgs_line_align_params), set by dgs_line_align_params_init */
  int32_t angle_gate_float_chain;  /* 1: the angle gate's angle through transform3Dto2D on the float cast, as upstream (recalled Eigen
                                      3.3); 0: atan2(r10, r00) in double */
  double g_avg_distance_weight;    /* the three weights: >= 0; +infinity is accepted and makes a hypothesis whose term is 0 score NaN, */
  double g_coverage_weight;        /* which never wins; a negative or NaN weight is DGS_ERR_INVALID_ARGUMENT */
  double g_transform_weight;
  double g_max_score_distance;     /* > 0 */
  double g_max_score_translation;
  double max_distance;
  double max_angle;
  int32_t nn_tie_highest_index;    /* 0: equal real_distances go to the lowest target index (recalled: std::sort's insertion sort
                                      below 16 elements keeps the order); 1: to the highest */
  int32_t reserved;
  /* ---- appended for align_local.  A caller whose struct_size ends at `reserved` gets the defaults below. */
  double l_avg_distance_weight;    /* weight_local's members (line_based_scanmatcher.hpp:96-100): 0.6, 1.0, 0.2, 5.0, 5.0; same rules as g_* */
  double l_coverage_weight;
  double l_transform_weight;
  double l_max_score_distance;
  double l_max_score_translation;
  double l_max_distance;           /* align_local's constants (:208-209): 2.5 and pi / 9 */
  double l_max_angle;
  int32_t refine_three_nearest;    /* 0: the line-pair phase visits every neighbour rank (what upstream's `i<3 || i<size` does for three or
                                      more); 1: ranks 0..2 only, what its comment intends */
  int32_t edges_on_device;         /* the member that was `reserved2` (dgs_line_align_params_init has always zeroed it, and the struct keeps
                                      its size): 0: align_global and align_local extract their edges on the host, as before; 1: on the
                                      device (dgs_line_edge_extraction_batch's kernels): the same edges bit for bit, one
                                      more host wait per call.  A caller whose struct_size ends at `reserved` gets 0. */
} dgs_line_align_params;
int dgs_line_align_params_init(dgs_line_align_params* params);
/* upstream's BestFitAlignment without the two line vectors, and what the search saw */
typedef struct dgs_line_alignment {
  double transformation[16];   /* row-major 4 x 4 */
  double fitness_score[4];     /* FitnessScore: real_avg_distance, avg_distance, coverage, coverage_percentage */
  double score;                /* weight_global of the result */
  int64_t winner;              /* the winning h = es * Et + et; -1 when none beat the identity */
  int64_t n_hypotheses;        /* Es * Et */
  int64_t n_survivors;         /* hypotheses that passed the gates */
  int32_t n_edges_source;
  int32_t n_edges_target;
  int32_t n_lines_target;      /* after merge_lines */
  int32_t refine_steps;        /* iterations of the refinement pass (:160-200) that took over */
  int32_t status;              /* dgs_line_align_status */
  int32_t reserved;
} dgs_line_alignment;
/* align_global (:109-203) from the extracted source lines on (line_extraction stays with dgs_line_extraction).  aligned_lines:
 * room for n_src features (nullable); not_aligned_lines are src_lines themselves.  More than DGS_LA_MAX_LINES_SOURCE source lines,
 * DGS_LA_MAX_LINES_TARGET merged target lines or DGS_LA_MAX_HYPOTHESES hypotheses, or a coordinate that is not finite, is
 * DGS_ERR_INVALID_ARGUMENT with a message: nothing is truncated. */
int dgs_line_align_global(dgs_handle* h, const dgs_line_align_params* params, const dgs_line_feature* src_lines, int64_t n_src,
                          const dgs_line_feature* trg_lines, int64_t n_trg, int32_t constrain_angle, double max_range,
                          dgs_line_feature* aligned_lines, dgs_line_alignment* alignment);
/* merge_lines (:1086-1103) with are_lines_aligned (:1012-1084) on the host, no handle and no device.  out: room for n features; a
 * merged line has zero statistics (upstream leaves them unset). */
int dgs_line_merge(const dgs_line_feature* lines, int64_t n, dgs_line_feature* out, int64_t* n_out);
/* upstream's EdgeFeature */
typedef struct dgs_edge_feature {
  double edge_point[3];
  double point_a[3];
  double point_b[3];
} dgs_edge_feature;
/* edge_extraction (:459-471) with get_edges (:501-682) and lines_intersection (:473-499) on the host, no handle and no device;
 * only_angular_edges = false.  Fewer than two lines give no edges.  *n_edges is always the full count, DGS_ERR_INVALID_ARGUMENT
 * when it exceeds `capacity` (capacity 0 with a NULL array asks for the count alone). */
int dgs_line_edges(const dgs_line_feature* lines, int64_t n, dgs_edge_feature* edges, int64_t capacity, int64_t* n_edges);
/* Test hook: what the device computed per hypothesis in the last dgs_line_align_global call. */
typedef struct dgs_line_align_hypothesis {
  int32_t gate;           /* dgs_line_align_gate */
  int32_t slot;           /* position among the survivors, in h order; -1 when gated */
  double rotation[4];     /* r00 r01 r10 r11 of align_edges' transform (:693-740) */
  double translation[3];
  double fitness_score[4];/* calc_fitness_score (:905-955) of the transformed source lines; zeros when gated */
  double score;           /* weight_global; 0 when gated */
} dgs_line_align_hypothesis;
/* records: room for `count` records of h = first .. first + count - 1 (nullable).  counts4 (nullable): kernel launches, host waits,
 * hypotheses and survivors of the last call's device phase. */
int dgs_line_align_get_hypotheses(dgs_handle* h, int64_t first, int64_t count, dgs_line_align_hypothesis* records, int64_t* counts4);

/* ---- LineBasedScanmatcher::align_local on the device, batched (src/hdl_graph_slam/line_based_scanmatcher.cpp:205-297) -----------
 * One call takes n_items independent (source lines, target lines) pairs -- a keyframe's near buildings.  Per item: the baseline
 * (calc_fitness_score with is_local, weight_local), the edge pairs h = es * Et + et of edge_extraction(src, true, 0.01) x
 * edge_extraction(trg, true) gated by distance then angle, the strict arg-max, then the line pairs k = i * Lt + r over the snapshot
 * of the first phase's result (i: line of the snapshot, r: rank of a target line by (real_distance, index)), and the second
 * arg-max.  Edges are extracted on the host, or with params->edges_on_device on the device in one batched extraction over all items'
 * sources and targets (one more host wait, which reads the edge offsets back; the summed squares of the line counts are then limited by
 * DGS_LA_MAX_EDGE_PAIRS); everything else runs on the device with one upload, one download, one host wait and a number of kernel
 * launches that does not depend on n_items.  Nothing is merged: the target lines are used as given.  Semantics,
 * the deliberate differences from upstream and the limits: DESIGN.md 6g.  Additions only: DGS_ABI_VERSION is unchanged. */
#define DGS_LA_MAX_ITEMS 4096             /* items per batch call; the summed hypotheses of both phases: DGS_LA_MAX_HYPOTHESES */
typedef struct dgs_line_local_alignment {
  double transformation[16];       /* row-major 4 x 4: best_trans * transform, or best_trans when no line pair took over */
  double fitness_score[4];         /* FitnessScore of the result */
  double score;                    /* weight_local of the result */
  double edge_transformation[16];  /* best_trans: the first phase's result (the identity when no edge pair took over) */
  double edge_fitness_score[4];
  double edge_score;
  double baseline_fitness_score[4];
  double baseline_score;
  int64_t winner_edge;             /* the winning h = es * Et + et, -1: none */
  int64_t winner_line;             /* the winning k = i * Lt + r, -1: none */
  int64_t n_hypotheses_edge;       /* Es * Et */
  int64_t n_survivors_edge;
  int64_t n_hypotheses_line;       /* Ls * Lt */
  int64_t n_survivors_line;
  int32_t n_edges_source;
  int32_t n_edges_target;
  int32_t is_edge_aligned;         /* upstream's isEdgeAligned */
  int32_t status;                  /* dgs_line_align_status: ALIGNED (an edge pair took over), LINE_ALIGNED, NO_HYPOTHESES (neither phase
                                      has one), ALL_GATED, NONE_BETTER */
} dgs_line_local_alignment;
/* src_lines / trg_lines: the lines of all items back to back; src_offsets / trg_offsets: n_items + 1 ascending offsets into them
 * (item b owns [offsets[b], offsets[b + 1])).  aligned_lines (nullable): room for src_offsets[n_items] features, laid out like
 * src_lines; the statistics of a source line are carried through.  alignments: n_items records.  More than DGS_LA_MAX_ITEMS items,
 * DGS_LA_MAX_LINES_SOURCE / DGS_LA_MAX_LINES_TARGET lines in an item, DGS_LA_MAX_HYPOTHESES hypotheses summed over items and both
 * phases, a NaN max_range or a coordinate that is not finite is DGS_ERR_INVALID_ARGUMENT with a message: nothing is truncated. */
int dgs_line_align_local_batch(dgs_handle* h, const dgs_line_align_params* params, int64_t n_items, const dgs_line_feature* src_lines,
                               const int64_t* src_offsets, const dgs_line_feature* trg_lines, const int64_t* trg_offsets, double max_range,
                               dgs_line_feature* aligned_lines, dgs_line_local_alignment* alignments);
/* a batch of one */
int dgs_line_align_local(dgs_handle* h, const dgs_line_align_params* params, const dgs_line_feature* src_lines, int64_t n_src,
                         const dgs_line_feature* trg_lines, int64_t n_trg, double max_range, dgs_line_feature* aligned_lines,
                         dgs_line_local_alignment* alignment);
/* edge_extraction with its two upstream arguments (dgs_line_edges is only_angular_edges = 0, max_dist_angular_edge = 7.0) */
int dgs_line_edges_angular(const dgs_line_feature* lines, int64_t n, int32_t only_angular_edges, double max_dist_angular_edge,
                           dgs_edge_feature* edges, int64_t capacity, int64_t* n_edges);
/* Test hook: what the device computed per hypothesis in the last dgs_line_align_local_batch call. */
typedef struct dgs_line_align_local_hypothesis {
  int32_t gate;           /* dgs_line_align_gate */
  int32_t target;         /* phase 1: the target line of rank r; phase 0: -1 */
  double rotation[4];     /* r00 r01 r10 r11 of this hypothesis's own transform (align_edges / align_lines) */
  double translation[3];
  double fitness_score[4];/* zeros when gated */
  double score;           /* weight_local; 0 when gated */
} dgs_line_align_local_hypothesis;
/* records: room for `count` records of hypotheses first .. first + count - 1 of `item` in `phase` (0: edge pairs, 1: line pairs)
 * (nullable).  counts8 (nullable): kernel launches, host waits, items, summed hypotheses of phase 0 and of phase 1, summed survivors of
 * phase 0 and of phase 1, and workgroups of the two scoring launches together, all of the last call. */
int dgs_line_align_local_get_hypotheses(dgs_handle* h, int64_t item, int32_t phase, int64_t first, int64_t count,
                                        dgs_line_align_local_hypothesis* records, int64_t* counts8);

/* ---- edge_extraction on the device, batched (src/hdl_graph_slam/line_based_scanmatcher.cpp:459-471, get_edges :501-682) -----------
 * The lines of n_items segments back to back with n_items + 1 ascending offsets; per segment only_angular[b] and max_dist[b]
 * (align_local: 1 and 0.01 for the source, 1 and 7.0 for the target; align_global: 0 and 7.0).  The edges of all segments come back to
 * back, a segment's in edge_extraction's order (pairs i < j ascending in (i, j), a pair's edges in case order), bit for bit what
 * dgs_line_edges_angular gives for that segment; edge_offsets (nullable): n_items + 1 offsets into them.  A segment of fewer than two
 * lines gives no edges.  *n_edges is always the full count, DGS_ERR_INVALID_ARGUMENT when it exceeds `capacity` (capacity 0 with a NULL
 * array asks for the count and the offsets alone; nothing is emitted then).  More than DGS_LA_MAX_ITEMS segments, more than
 * DGS_LA_MAX_LINES_TARGET lines in a segment, more than DGS_LA_MAX_EDGE_PAIRS pairs (the squares of the segments' line counts summed: the
 * kernels index a segment's pairs as i * n + j), offsets that do not ascend from 0, a NaN max_dist or a coordinate that is not finite is
 * DGS_ERR_INVALID_ARGUMENT with a message, checked before anything is launched and before the handle is looked at (with a NULL handle
 * the message is dgs_last_error(NULL)'s): nothing is truncated.  Three launches for the counts, one host wait, one launch for the edges,
 * a second wait for their download.  Own buffers on the handle.  Semantics and kernels: DESIGN.md 6l.  Additions only: DGS_ABI_VERSION
 * is unchanged. */
#define DGS_LA_MAX_EDGE_PAIRS (1 << 24)
int dgs_line_edge_extraction_batch(dgs_handle* h, const dgs_line_feature* lines, const int64_t* offsets, int64_t n_items,
                                   const int32_t* only_angular, const double* max_dist, dgs_edge_feature* edges, int64_t capacity,
                                   int64_t* edge_offsets, int64_t* n_edges);
/* a batch of one segment */
int dgs_line_edge_extraction(dgs_handle* h, const dgs_line_feature* lines, int64_t n, int32_t only_angular_edges, double max_dist_angular_edge,
                             dgs_edge_feature* edges, int64_t capacity, int64_t* n_edges);
/* Test hook.  counts4: kernel launches, host waits, pairs i < j and edges of the last device edge extraction on this handle (a
 * dgs_line_edge_extraction* call, or an aligner call with edges_on_device). */
int dgs_line_edges_get_counts(dgs_handle* h, int64_t* counts4);

/* ---- are_buildings_overlapped and LineBasedScanmatcher::align_overlapped_buildings on the device ---------------------------------
 * (include/hdl_graph_slam/check_overlapping.hpp; src/hdl_graph_slam/line_based_scanmatcher.cpp:29-107; the loop of
 * apps/delta_graph_slam_nodelet.cpp:846-900).  Semantics, the deliberate non-differences from the geometric predicate, the limits
 * and the memory formula: DESIGN.md 6h.  Own buffers on the handle: registration, prefilter, map, line-extraction and the two
 * aligners' state are untouched.  Additions only: DGS_ABI_VERSION is unchanged. */
#define DGS_BO_MAX_BUILDINGS (1 << 14)    /* the pair flags take B * B / 8 bytes: 32 MiB here */
#define DGS_LA_OVERLAP_MAX_ANGLE 1.0471975511965976 /* M_PI / 3.0 (:47) */
/* getOverlappedBuildings (nodelet :767-787): every pair i < j of the n_buildings buildings whose shrunken polygons intersect
 * (are_buildings_overlapped), i ascending, then j ascending.  lines: the lines of all buildings back to back; line_offsets:
 * n_buildings + 1 ascending offsets; centers: double[n_buildings][3], x and y are read.  pairs: int32[capacity][2] (nullable with
 * capacity 0).  *n_pairs is always the full count; with more pairs than `capacity` the first `capacity` are written and the call
 * returns DGS_ERR_CAPACITY.  More than DGS_BO_MAX_BUILDINGS buildings, more than DGS_LA_MAX_LINES_TARGET lines in one building or a
 * coordinate that is not finite is DGS_ERR_INVALID_ARGUMENT with a message.  One upload, one download, one host wait, five launches. */
int dgs_building_overlap_pairs(dgs_handle* h, const dgs_line_feature* lines, const int64_t* line_offsets, const double* centers,
                               int64_t n_buildings, int32_t* pairs, int64_t capacity, int64_t* n_pairs);
typedef struct dgs_line_overlap_alignment {
  double transformation[16];       /* row-major 4 x 4: the winner's transform, or the identity */
  double translation_norm;         /* the winner's translation.norm(); DBL_MAX (upstream's start value) without a winner */
  int64_t winner;                  /* h = es * Et + et for an edge pair, Es * Et + i * Lt + j for a line pair; -1: none */
  int64_t n_hypotheses_edge;       /* Es * Et */
  int64_t n_hypotheses_line;       /* Ls * Lt */
  int64_t n_angle_passed;          /* hypotheses past the angle gate */
  int64_t n_not_overlapped;        /* and past the overlap gate */
  int32_t n_edges_source;
  int32_t n_edges_target;
  int32_t is_identity;             /* the transformation is bit-equal to the identity: the nodelet adds no edge then (:875) */
  int32_t status;                  /* dgs_line_align_status: ALIGNED, NO_HYPOTHESES, ALL_GATED (no hypothesis passed both gates),
                                      NONE_BETTER (one passed, but its norm is NaN or not below DBL_MAX) */
} dgs_line_overlap_alignment;
/* align_overlapped_buildings from the building-frame lines on, for n_items independent (source, target) pairs: the caller keeps the
 * frame transforms around it.  Layout of lines, offsets and aligned_lines as in dgs_line_align_local_batch;
 * centers_source / centers_target: double[n_items][3] (upstream: zero, and B's centre in A's frame).  Of `params` only
 * angle_gate_float_chain is read (edges_on_device is not: the items are pairs of single buildings with a handful of lines); the angle
 * is DGS_LA_OVERLAP_MAX_ANGLE.  Edges come from edge_extraction with its defaults on the host; one upload, one download, one host wait, three launches.  DGS_LA_MAX_ITEMS, DGS_LA_MAX_LINES_SOURCE / _TARGET per item and
 * DGS_LA_MAX_HYPOTHESES summed over the batch as for align_local; 72 bytes of device memory per hypothesis. */
int dgs_line_align_overlapped_batch(dgs_handle* h, const dgs_line_align_params* params, int64_t n_items, const dgs_line_feature* src_lines,
                                    const int64_t* src_offsets, const dgs_line_feature* trg_lines, const int64_t* trg_offsets,
                                    const double* centers_source, const double* centers_target, dgs_line_feature* aligned_lines,
                                    dgs_line_overlap_alignment* alignments);
/* a batch of one */
int dgs_line_align_overlapped(dgs_handle* h, const dgs_line_align_params* params, const dgs_line_feature* src_lines, int64_t n_src,
                              const dgs_line_feature* trg_lines, int64_t n_trg, const double* center_source, const double* center_target,
                              dgs_line_feature* aligned_lines, dgs_line_overlap_alignment* alignment);
/* Test hook: what the device computed per hypothesis in the last dgs_line_align_overlapped_batch call. */
typedef struct dgs_line_align_overlapped_hypothesis {
  int32_t gate;           /* DGS_LA_GATE_PASS, DGS_LA_GATE_ANGLE or DGS_LA_GATE_OVERLAP */
  int32_t reserved;
  double rotation[4];     /* r00 r01 r10 r11 of align_edges' / align_lines' transform */
  double translation[3];
  double translation_norm;
} dgs_line_align_overlapped_hypothesis;
/* records: room for `count` records of hypotheses first .. first + count - 1 of `item` (nullable) */
int dgs_line_align_overlapped_get_hypotheses(dgs_handle* h, int64_t item, int64_t first, int64_t count,
                                             dgs_line_align_overlapped_hypothesis* records);
/* counts8: of the last dgs_building_overlap_pairs call kernel launches, host waits, buildings, pairs; of the last
 * dgs_line_align_overlapped_batch call kernel launches, host waits, items, hypotheses. */
int dgs_building_overlap_get_counts(dgs_handle* h, int64_t* counts8);

/* ---- FloorDetectionNodelet::detect on the device (apps/floor_detection_nodelet.cpp:110-238) -----------------------------------
 * Tilt transform, the two plane clips, the k = 10 normal filter, the back-transform, a RANSAC plane fit
 * (pcl::RandomSampleConsensus over pcl::SampleConsensusModelPlane, driven directly: no refit) and the nodelet's three checks.
 * Semantics and the PCL 1.10 details recalled from upstream: DESIGN.md 6j.  The detector works in buffers of its own:
 * registration, prefilter, map and line state are untouched.  Additions only: DGS_ABI_VERSION is unchanged. */
enum dgs_floor_detection_status {
  DGS_FD_DETECTED = 0,        /* coeffs4_out holds the plane, its normal upward */
  DGS_FD_TOO_FEW_POINTS = 1,  /* the filtered cloud has fewer than floor_pts_thresh points (:133) */
  DGS_FD_TOO_FEW_INLIERS = 2, /* the winner has fewer than floor_pts_thresh inliers (:147) */
  DGS_FD_NOT_VERTICAL = 3,    /* the winner's normal is farther than floor_normal_thresh from the tilted z axis (:158) */
  DGS_FD_RNG_EXHAUSTED = 4    /* the caller's rng_raw stream ran out */
};
/* Defaults (dgs_floor_detection_params_init) = the nodelet's (:57-63) and PCL's: 0, 2, 1, 512, 10, true, 20; 0.1, 1000, 0.99, 1000;
 * orders 0; chunks of 64 then 512 hypotheses. */
typedef struct dgs_floor_detection_params {
  uint32_t struct_size;          /* sizeof(dgs_floor_detection_params), set by dgs_floor_detection_params_init */
  int32_t floor_pts_thresh;      /* negative: DGS_ERR_INVALID_ARGUMENT (upstream compares it as size_t) */
  double tilt_deg;               /* read by the adapters, which build tilt16 / tilt_inv16 from it; the library takes the matrices */
  double sensor_height;
  double height_clip_range;
  double floor_normal_thresh;    /* degrees */
  double normal_filter_thresh;   /* degrees */
  double distance_threshold;     /* ransac.setDistanceThreshold(0.1) (:140) */
  double probability;            /* SampleConsensus::probability_ */
  int32_t use_normal_filtering;
  int32_t max_iterations;        /* SampleConsensus::max_iterations_ */
  int32_t max_sample_checks;     /* SampleConsensusModel::max_sample_checks_ */
  int32_t transform_order;       /* 0: x*m0 + (y*m1 + (z*m2 + m3)) per coordinate, 1: ((m0*x + m1*y) + m2*z) + m3 */
  int32_t plane_dot_order;       /* four-term dot products of the plane model: 0 (a+b)+(c+d), 1 (a+c)+(b+d), 2 left to right */
  int32_t hyp_chunk_first;       /* hypotheses scored before the host first walks the counts */
  int32_t hyp_chunk;             /* hypotheses per further launch while the walk is open; the result depends on neither */
  int32_t reserved;
} dgs_floor_detection_params;
int dgs_floor_detection_params_init(dgs_floor_detection_params* params);
/* tilt16 / tilt_inv16: the two 4 x 4 float matrices of detect(), column-major (Eigen's data()).  in_xyz16: n xyz16 points (host
 * array, or device pointer with in_on_device), e.g. dgs_prefilter_scan's 3-D output; it is not modified.  rng_raw (nullable):
 * rng_len values that stand in for boost::mt19937(12345)() >> 1, three per draw; running past its end is DGS_FD_RNG_EXHAUSTED.
 * coeffs4_out: the four plane coefficients, written (zeros unless detected) whatever the status.  *status_out:
 * dgs_floor_detection_status.  An empty cloud is DGS_FD_TOO_FEW_POINTS with DGS_OK. */
int dgs_floor_detection(dgs_handle* h, const dgs_floor_detection_params* params, const float* tilt16, const float* tilt_inv16,
                        const float* in_xyz16, int64_t n, int32_t in_on_device, const uint32_t* rng_raw, int64_t rng_len,
                        float* coeffs4_out, int32_t* status_out);
/* The filtered cloud of the last detect (/floor_detection/floor_filtered_points).  out_xyz16 (nullable): room for `capacity`
 * points, written when capacity >= *n; *n is always the full count. */
int dgs_floor_detection_get_filtered(dgs_handle* h, float* out_xyz16, int64_t capacity, int32_t out_on_device, int64_t* n);
/* The winner's inliers of the last detect: indices into the filtered cloud, ascending, and (nullable) the points themselves
 * (/floor_detection/floor_points), both host arrays with room for `capacity` entries, written when capacity >= *n. */
int dgs_floor_detection_get_inliers(dgs_handle* h, int32_t* indices, float* points_xyz16, int64_t capacity, int64_t* n);
typedef struct dgs_floor_detection_trace {
  int32_t n_clipped;          /* points after the two plane clips */
  int32_t n_filtered;         /* points of the filtered cloud */
  int32_t draws;              /* samples drawn (three raw values each) */
  int32_t hypotheses_scored;  /* hypotheses the device scored against the cloud */
  int32_t iterations;         /* hypotheses the walk consumed */
  int32_t chunks_launched;    /* score launches = host waits of the RANSAC */
  int32_t winner_rank;        /* rank of the winner among the good samples (-1: no model) */
  int32_t sample[3];          /* the winner's three point indices (-1: no model) */
  int32_t count;              /* the winner's inlier count */
  int32_t ransac_failed;      /* max_sample_checks bad draws in a row (or fewer than three points) ended the walk */
  float raw_coeffs[4];        /* the winner's coefficients before the upward flip (zeros: no model) */
  float dot;                  /* the verticality check's dot product */
  int32_t reserved;
} dgs_floor_detection_trace;
int dgs_floor_detection_get_trace(dgs_handle* h, dgs_floor_detection_trace* trace);
/* Test hook: the clipped cloud of the last detect and, with use_normal_filtering, its normals (xyz0 per point; else untouched).
 * Host arrays (nullable) with room for `capacity` points, written when capacity >= *n. */
int dgs_floor_detection_get_clipped(dgs_handle* h, float* clipped_xyz16, float* normals4, int64_t capacity, int64_t* n);
/* The two host pieces of the RANSAC, callable without a device.  Draws: the first n_draws index triples of the sample stream over n
 * points (n >= 3), from rng_raw (3 * n_draws values) or, when NULL, from mt19937(12345)() >> 1.  Walk: RandomSampleConsensus::
 * computeModel over inlier counts -> winner (-1: none), iterations consumed, and whether it ran past n_counts still open. */
int dgs_floor_detection_draws(int64_t n, const uint32_t* rng_raw, int64_t n_draws, int32_t* triples_out);
int dgs_floor_detection_walk(int64_t n, int32_t max_iterations, double probability, const int32_t* counts, int64_t n_counts,
                             int32_t* winner_out, int32_t* iterations_out, int32_t* open_out);
/* detect() over n_scans scans in one call, e.g. the frames of several streams: one chain of launches and three host waits whatever
 * their number.  One parameter set and one tilt / tilt_inv pair for all scans.  in_xyz16[i]: sizes[i] xyz16 points
 * (all host arrays, or all device pointers with in_on_device), not modified.  rng_raw (nullable array) and rng_len (nullable when
 * rng_raw is): per scan what dgs_floor_detection takes; rng_raw[i] NULL or rng_len[i] 0: mt19937(12345).  Scan i receives in
 * coeffs4_out[4 * i ..] and status_out[i], bit for bit, what dgs_floor_detection gives it alone, wherever it stands in the batch.
 * Per-scan conditions (TOO_FEW_POINTS, an empty scan included, TOO_FEW_INLIERS, NOT_VERTICAL, RNG_EXHAUSTED) are statuses with
 * zero coefficients; the other scans run.  Refused with DGS_ERR_INVALID_ARGUMENT before anything is written: what
 * dgs_floor_detection refuses in the parameters, a NULL array, a negative size or rng_len, a NULL input of positive size, a size
 * above INT32_MAX, more than 2^31 points in total.  n_scans == 0 is DGS_OK without a launch.  The batch works in buffers of its
 * own: the getters of the single call keep reporting the last dgs_floor_detection. */
int dgs_floor_detection_batch(dgs_handle* h, const dgs_floor_detection_params* params, const float* tilt16, const float* tilt_inv16,
                              int32_t n_scans, const float* const* in_xyz16, const int64_t* sizes, int32_t in_on_device,
                              const uint32_t* const* rng_raw, const int64_t* rng_len, float* coeffs4_out, int32_t* status_out);
/* The getters of the single call by scan number of the last batch (0 <= scan < n_scans, else DGS_ERR_INVALID_ARGUMENT).  The
 * filtered cloud and the inlier list of a scan are fetched and computed when asked for.  In the trace, hypotheses_scored and
 * chunks_launched say how far that scan's own scoring went inside the batch's rounds: a scan's first chunk may be scored in a round
 * in which other scans score a later one, so they are not the single call's launch counts. */
int dgs_floor_detection_batch_get_filtered(dgs_handle* h, int32_t scan, float* out_xyz16, int64_t capacity, int32_t out_on_device, int64_t* n);
int dgs_floor_detection_batch_get_inliers(dgs_handle* h, int32_t scan, int32_t* indices, float* points_xyz16, int64_t capacity, int64_t* n);
int dgs_floor_detection_batch_get_trace(dgs_handle* h, int32_t scan, dgs_floor_detection_trace* trace);
int dgs_floor_detection_batch_get_clipped(dgs_handle* h, int32_t scan, float* clipped_xyz16, float* normals4, int64_t capacity, int64_t* n);
/* Of the last batch: [0] kernel launches, [1] host waits, [2] scans listed, [3] scans that reached the RANSAC, [4] scans served by a
 * per-scan fallback (a draw list that had to grow; every scan of a chunk under DGS_KNN_LEAF=0), [5] chunks of scans
 * (DGS_FLOOR_BATCH_POINTS raw points each, default 4 Mi), [6] indices built, [7] RANSAC rounds (score launches) of the call. */
int dgs_floor_detection_batch_get_counts(dgs_handle* h, int64_t* counts8);

/* ---- interpolate, BuildingTools::buildPointCloud and Building::getCloud on the device --------------------------------------------
 * (src/hdl_graph_slam/ros_utils.cpp:146-165, building_tools.cpp:166-196, building.cpp:7-22; the call sites of
 * apps/delta_graph_slam_nodelet.cpp:266-288, :327-336, :689-711, :751-757, :1184-1198).  Every line of every item is sampled into
 * points a + i_k * normalized(b - a) with i_0 = 0, i_{k+1} = fl(i_k + sample_step), one point per i_k <= norm(b - a), z = 0, the fourth
 * float 1; an item's points may then go through pcl::transformPointCloud(Matrix4f).  All float32, no FMA; semantics, kernels and the
 * Eigen / PCL details recalled from upstream ([UPSTREAM-RECALL]): DESIGN.md 6m.  Each recalled detail is a field:
 *   sqnorm_order:     dgs_prefilter_norm_order of squaredNorm's terms x², y², z² (the w term is 0, so orders 0 and 2 give the same bits).
 *   normalized_guard: 1 = Eigen 3.3's normalized(): d / sqrt(n2) when n2 > 0, else d.  0 = the older form, which divides
 *                     unconditionally: a zero-length line then gives one NaN point instead of one point at a.
 *   transform_order:  dgs_floor_detection_params::transform_order, the same restatement of pcl::transformPointCloud.
 * sample_step is upstream's 0.02f.  max_points_per_line ends the table of i_k (it also ends where i_{k+1} <= i_k); a line whose norm is
 * +inf or exceeds the table's last entry is DGS_ERR_INVALID_ARGUMENT (upstream would not terminate, or would exhaust memory).
 * Own buffers on the handle: registration, prefilter, map, line, overlap and floor state are untouched.  Additions only:
 * DGS_ABI_VERSION is unchanged. */
#define DGS_BC_TILE 1024                  /* output points per workgroup of the fill kernel */
typedef struct dgs_building_cloud_params {
  uint32_t struct_size;          /* sizeof(dgs_building_cloud_params), set by dgs_building_cloud_params_init */
  float sample_step;             /* > 0 and finite */
  int32_t sqnorm_order;          /* dgs_prefilter_norm_order */
  int32_t normalized_guard;
  int32_t transform_order;       /* 0 or 1 */
  int32_t max_points_per_line;   /* >= 1 */
  int32_t reserved;
} dgs_building_cloud_params;
/* Defaults: 0.02f, DGS_PF_NORM_PAIRS_XY_ZW, 1, 0, 1 << 20. */
int dgs_building_cloud_params_init(dgs_building_cloud_params* params);
/* lines: the lines of all n_items items back to back (point_a and point_b are read); line_offsets: n_items + 1 ascending offsets from
 * 0.  transforms16 (nullable): 4 x 4 float matrices, COLUMN-major (Eigen's data()), 16 floats each; transform_index (nullable): per
 * item the matrix its points go through, -1 for none.  With transforms16 and no transform_index every item takes matrix 0; without
 * transforms16 no item is transformed and transform_index is not read.  The points come in item order, line order within an item and
 * k ascending; *n_points is their number.  They stay on the handle until the next call: read them with dgs_building_cloud_get.
 * n_items == 0 and items without lines are not errors.  A NaN norm gives no point.  On DGS_ERR_INVALID_ARGUMENT the message names
 * the item and the line, nothing is produced and the handle stays usable.  Three launches whatever the sizes, one host wait. */
int dgs_building_cloud_generate(dgs_handle* h, const dgs_building_cloud_params* params, const dgs_line_feature* lines,
                                const int64_t* line_offsets, int64_t n_items, const float* transforms16, const int32_t* transform_index,
                                int64_t* n_points);
/* Copies the last result out: the points (host array, or device pointer with out_on_device; nullable with capacity 0) and the
 * n_items + 1 point offsets of the items (a host array, nullable).  *n is always the full count; DGS_ERR_INVALID_ARGUMENT when it
 * exceeds `capacity`.  device_ptr_out (nullable): the stage's own buffer on the device, valid until the next generate call. */
int dgs_building_cloud_get(dgs_handle* h, float* out_xyz16, int64_t capacity, int32_t out_on_device, int64_t* point_offsets, int64_t* n,
                           const float** device_ptr_out);
/* Test hook.  counts8 of the last generate call: kernel launches, host waits, lines, points, entries of the step table, entries the
 * call added to it, DGS_BC_TILE, items. */
int dgs_building_cloud_get_counts(dgs_handle* h, int64_t* counts8);

#ifdef __cplusplus
}
#endif
#endif /* DGS_REG_H */
