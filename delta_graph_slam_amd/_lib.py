"""ctypes binding of libdgs_reg.so (include/dgs_reg.h).  Fails loudly when the HIP library is missing --
there is no CPU fallback anywhere in this package."""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("DGS_REG_LIB") or os.path.join(_HERE, "libdgs_reg.so")   # DGS_REG_LIB: an alternative build (A/B runs)

DGS_OK = 0
STATUS = {0: "DGS_OK", 1: "DGS_ERR_INVALID_ARGUMENT", 2: "DGS_ERR_HIP", 3: "DGS_ERR_NO_TARGET", 4: "DGS_ERR_NO_SOURCE",
          5: "DGS_ERR_GRID_TOO_LARGE", 6: "DGS_ERR_UNSUPPORTED", 7: "DGS_ERR_CAPACITY"}
DGS_ERR_CAPACITY = 7
METHOD_NDT, METHOD_GICP, METHOD_VGICP, METHOD_ICP, METHOD_PCL_GICP, METHOD_PCL_NDT = 0, 1, 2, 3, 4, 5
VGICP_SEARCH = {"DIRECT1": 0, "DIRECT7": 1, "DIRECT27": 2}
NDT_SEARCH = {"KDTREE": 0, "DIRECT26": 1, "DIRECT7": 2, "DIRECT1": 3}
NDT_ORDER = {"FAST": 0, "UPSTREAM": 1, "UPSTREAM_SEQUENTIAL": 2}
GICP_REG = {"NONE": 0, "MIN_EIG": 1, "NORMALIZED_MIN_EIG": 2, "PLANE": 3, "FROBENIUS": 4}
GICP_COV = {"SYM_EIG": 0, "JACOBI_SVD": 1, "UPSTREAM_ORDER": 2}   # dgs_gicp_cov_mode: dgs_params.gicp_cov_jacobi_svd
K_NDT_DERIVATIVES, K_NDT_SOLVE, K_NDT_VOXEL_BUILD, K_NN_SEARCH, K_GICP_LINEARIZE, K_GICP_COVARIANCE, K_TRANSFORM = range(7)


class DgsError(RuntimeError):
    def __init__(self, status: int, msg: str = ""):
        self.status = status
        super().__init__(f"{STATUS.get(status, status)}: {msg}")


class Params(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32), ("method", C.c_int32), ("device", C.c_int32), ("num_threads", C.c_int32),
        ("transformation_epsilon", C.c_double), ("maximum_iterations", C.c_int32), ("ndt_search_method", C.c_int32),
        ("ndt_resolution", C.c_double), ("ndt_step_size", C.c_double), ("ndt_outlier_ratio", C.c_double),
        ("ndt_min_covar_eigvalue_mult", C.c_double), ("ndt_min_points_per_voxel", C.c_int32),
        ("ndt_line_search", C.c_int32), ("ndt_mt_max_step_iterations", C.c_int32), ("ndt_fix_hessian_d1", C.c_int32),
        ("ndt_strict_order", C.c_int32),
        ("gicp_max_correspondence_distance", C.c_double), ("gicp_rotation_epsilon", C.c_double),
        ("gicp_lm_init_lambda_factor", C.c_double), ("gicp_correspondence_randomness", C.c_int32),
        ("gicp_regularization", C.c_int32), ("gicp_optimizer", C.c_int32), ("gicp_lm_max_iterations", C.c_int32),
        ("vgicp_search_method", C.c_int32), ("vgicp_resolution", C.c_double),
        ("ndt_newton_solver", C.c_int32), ("ndt_hessian_recompute_double", C.c_int32), ("ndt_guess_rotation_polar", C.c_int32),
        ("ndt_exp_glibc", C.c_int32),
        ("ndt_cov_eigensolver", C.c_int32), ("gicp_cov_jacobi_svd", C.c_int32),
    ]


class IcpOptions(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("use_reciprocal_correspondences", C.c_int32), ("euclidean_fitness_epsilon", C.c_double),
                ("rotation_epsilon", C.c_double)]


class PclGicpOptions(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("max_optimizer_iterations", C.c_int32), ("rotation_epsilon", C.c_double),
                ("gicp_epsilon", C.c_double), ("use_reciprocal_correspondences", C.c_int32)]


class PrefilterParams(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("downsample_method", C.c_int32), ("downsample_resolution", C.c_double),
                ("outlier_removal_method", C.c_int32), ("statistical_mean_k", C.c_int32), ("statistical_stddev", C.c_double),
                ("radius_radius", C.c_double), ("radius_min_neighbors", C.c_int32), ("use_distance_filter", C.c_int32),
                ("distance_near_thresh", C.c_double), ("distance_far_thresh", C.c_double), ("radius_inclusive", C.c_int32),
                ("statistical_sqrt_float", C.c_int32)]


class PrefilterScanParams(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("has_angular_velocity", C.c_int32), ("angular_velocity", C.c_double * 3),
                ("scan_period", C.c_double), ("has_transform", C.c_int32), ("transform", C.c_double * 16), ("deskew_norm_order", C.c_int32),
                ("transform_sets_w", C.c_int32)]


class MapCloudParams(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("first_box_oversize", C.c_int32), ("grow_shift_without_upper", C.c_int32),
                ("max_minus_epsilon", C.c_int32), ("child_index_x_msb", C.c_int32), ("key_at_insertion", C.c_int32), ("dedup_method", C.c_int32), ("hash_slots", C.c_int64)]


class LineExtractionParams(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("min_cluster_size", C.c_int32), ("max_cluster_size", C.c_int32), ("cluster_tolerance", C.c_float),
                ("sac_distance_threshold", C.c_float), ("max_iterations", C.c_int32), ("merror_threshold", C.c_float),
                ("line_length_threshold", C.c_float), ("sac_method_type", C.c_int32), ("sample_good_any_axis", C.c_int32),
                ("sqnorm_order", C.c_int32), ("cluster_inclusive", C.c_int32), ("max_rounds", C.c_int32), ("record_lists", C.c_int32)]


class LineFeatureC(C.Structure):
    _fields_ = [("point_a", C.c_double * 3), ("point_b", C.c_double * 3), ("mean_error", C.c_double), ("std_sigma", C.c_double),
                ("max_error", C.c_double), ("min_error", C.c_double)]


class LineExtractionRound(C.Structure):
    _fields_ = [("n_before", C.c_int32), ("draws", C.c_int32), ("iterations", C.c_int32), ("sample0", C.c_int32), ("sample1", C.c_int32),
                ("inliers", C.c_int32), ("cluster", C.c_int32), ("emitted", C.c_int32)]


class FloorDetectionParams(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("floor_pts_thresh", C.c_int32), ("tilt_deg", C.c_double), ("sensor_height", C.c_double),
                ("height_clip_range", C.c_double), ("floor_normal_thresh", C.c_double), ("normal_filter_thresh", C.c_double),
                ("distance_threshold", C.c_double), ("probability", C.c_double), ("use_normal_filtering", C.c_int32),
                ("max_iterations", C.c_int32), ("max_sample_checks", C.c_int32), ("transform_order", C.c_int32),
                ("plane_dot_order", C.c_int32), ("hyp_chunk_first", C.c_int32), ("hyp_chunk", C.c_int32), ("reserved", C.c_int32)]


class BuildingCloudParams(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("sample_step", C.c_float), ("sqnorm_order", C.c_int32), ("normalized_guard", C.c_int32),
                ("transform_order", C.c_int32), ("max_points_per_line", C.c_int32), ("reserved", C.c_int32)]


class FloorDetectionTrace(C.Structure):
    _fields_ = [("n_clipped", C.c_int32), ("n_filtered", C.c_int32), ("draws", C.c_int32), ("hypotheses_scored", C.c_int32),
                ("iterations", C.c_int32), ("chunks_launched", C.c_int32), ("winner_rank", C.c_int32), ("sample", C.c_int32 * 3),
                ("count", C.c_int32), ("ransac_failed", C.c_int32), ("raw_coeffs", C.c_float * 4), ("dot", C.c_float),
                ("reserved", C.c_int32)]


class LineAlignParams(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("angle_gate_float_chain", C.c_int32), ("g_avg_distance_weight", C.c_double),
                ("g_coverage_weight", C.c_double), ("g_transform_weight", C.c_double), ("g_max_score_distance", C.c_double),
                ("g_max_score_translation", C.c_double), ("max_distance", C.c_double), ("max_angle", C.c_double),
                ("nn_tie_highest_index", C.c_int32), ("reserved", C.c_int32),
                # appended for align_local
                ("l_avg_distance_weight", C.c_double), ("l_coverage_weight", C.c_double), ("l_transform_weight", C.c_double),
                ("l_max_score_distance", C.c_double), ("l_max_score_translation", C.c_double), ("l_max_distance", C.c_double),
                ("l_max_angle", C.c_double), ("refine_three_nearest", C.c_int32), ("edges_on_device", C.c_int32)]   # the former reserved2


class LineAlignment(C.Structure):
    _fields_ = [("transformation", C.c_double * 16), ("fitness_score", C.c_double * 4), ("score", C.c_double), ("winner", C.c_int64),
                ("n_hypotheses", C.c_int64), ("n_survivors", C.c_int64), ("n_edges_source", C.c_int32), ("n_edges_target", C.c_int32),
                ("n_lines_target", C.c_int32), ("refine_steps", C.c_int32), ("status", C.c_int32), ("reserved", C.c_int32)]


class LineLocalAlignment(C.Structure):
    _fields_ = [("transformation", C.c_double * 16), ("fitness_score", C.c_double * 4), ("score", C.c_double),
                ("edge_transformation", C.c_double * 16), ("edge_fitness_score", C.c_double * 4), ("edge_score", C.c_double),
                ("baseline_fitness_score", C.c_double * 4), ("baseline_score", C.c_double), ("winner_edge", C.c_int64),
                ("winner_line", C.c_int64), ("n_hypotheses_edge", C.c_int64), ("n_survivors_edge", C.c_int64),
                ("n_hypotheses_line", C.c_int64), ("n_survivors_line", C.c_int64), ("n_edges_source", C.c_int32),
                ("n_edges_target", C.c_int32), ("is_edge_aligned", C.c_int32), ("status", C.c_int32)]


class LineAlignLocalHypothesis(C.Structure):
    _fields_ = [("gate", C.c_int32), ("target", C.c_int32), ("rotation", C.c_double * 4), ("translation", C.c_double * 3),
                ("fitness_score", C.c_double * 4), ("score", C.c_double)]


class LineOverlapAlignment(C.Structure):
    _fields_ = [("transformation", C.c_double * 16), ("translation_norm", C.c_double), ("winner", C.c_int64),
                ("n_hypotheses_edge", C.c_int64), ("n_hypotheses_line", C.c_int64), ("n_angle_passed", C.c_int64),
                ("n_not_overlapped", C.c_int64), ("n_edges_source", C.c_int32), ("n_edges_target", C.c_int32),
                ("is_identity", C.c_int32), ("status", C.c_int32)]


class LineAlignOverlappedHypothesis(C.Structure):
    _fields_ = [("gate", C.c_int32), ("reserved", C.c_int32), ("rotation", C.c_double * 4), ("translation", C.c_double * 3),
                ("translation_norm", C.c_double)]


class EdgeFeatureC(C.Structure):
    _fields_ = [("edge_point", C.c_double * 3), ("point_a", C.c_double * 3), ("point_b", C.c_double * 3)]


class LineAlignHypothesis(C.Structure):
    _fields_ = [("gate", C.c_int32), ("slot", C.c_int32), ("rotation", C.c_double * 4), ("translation", C.c_double * 3),
                ("fitness_score", C.c_double * 4), ("score", C.c_double)]


LA_STATUS = {0: "ALIGNED", 1: "NO_HYPOTHESES", 2: "ALL_GATED", 3: "NONE_BETTER", 4: "LINE_ALIGNED"}
LA_GATE = {0: "PASS", 1: "DISTANCE", 2: "IDENTITY", 3: "ANGLE", 4: "LINE_DIRECTION", 5: "LINE_DISTANCE", 6: "RANK", 7: "OVERLAP"}
BO_MAX_BUILDINGS = 1 << 14
LA_MAX_ITEMS, LA_MAX_LINES_TARGET, LA_MAX_EDGE_PAIRS = 4096, 512, 1 << 24
LE_STATUS = {0: "DONE", 1: "RANSAC_FAILED", 2: "STALL", 3: "MAX_ROUNDS", 4: "RNG_EXHAUSTED"}
FD_STATUS = {0: "DETECTED", 1: "TOO_FEW_POINTS", 2: "TOO_FEW_INLIERS", 3: "NOT_VERTICAL", 4: "RNG_EXHAUSTED"}
SAC_METHODS = ["SAC_RANSAC", "SAC_LMEDS", "SAC_MSAC", "SAC_RRANSAC", "SAC_RMSAC", "SAC_MLESAC", "SAC_PROSAC"]
MAP_DEDUP = {"AUTO": 0, "HASH": 1, "SORT": 2}
PF_DOWNSAMPLE = {"NONE": 0, "VOXELGRID": 1, "APPROX_VOXELGRID": 2}
PF_OUTLIER = {"NONE": 0, "STATISTICAL": 1, "RADIUS": 2}
PF_NORM_ORDER = {"PAIRS_XY_ZW": 0, "PAIRS_XZ_YW": 1, "SEQUENTIAL": 2}


class Result(C.Structure):
    _fields_ = [("final_transformation", C.c_float * 16), ("converged", C.c_int32), ("iterations", C.c_int32),
                ("evaluations", C.c_int32), ("status", C.c_int32), ("score", C.c_double), ("fitness", C.c_double)]


# every symbol include/dgs_reg.h declares (checked by tests/test_abi.py against the header text)
SYMBOLS = [
    "dgs_params_init", "dgs_create", "dgs_destroy", "dgs_last_error", "dgs_abi_version", "dgs_set_stream",
    "dgs_synchronize", "dgs_set_input_target", "dgs_set_input_source", "dgs_align", "dgs_get_fitness_score",
    "dgs_get_inlier_fraction", "dgs_nearest_search_target", "dgs_nn_fitness_distances", "dgs_align_batch", "dgs_find_loop_candidates", "dgs_calc_fitness_score", "dgs_voxel_grid_filter", "dgs_approx_voxel_grid_filter", "dgs_cloud_create", "dgs_cloud_destroy", "dgs_cloud_size",
    "dgs_set_input_target_cloud", "dgs_set_input_source_cloud", "dgs_align_batch_clouds", "dgs_align_pairs_clouds", "dgs_profile_enable",
    "dgs_profile_get", "dgs_profile_reset", "dgs_get_counts", "dgs_ndt_derivatives", "dgs_ndt_hessian_double", "dgs_ndt_score_gradient", "dgs_deal_probe", "dgs_deal_probe_cost", "dgs_strict_row_probe", "dgs_pcl_ndt_neighbours", "dgs_ndt_get_voxels",
    "dgs_ndt_get_trajectory", "dgs_gicp_get_covariances", "dgs_gicp_linearize", "dgs_vgicp_get_voxels",
    "dgs_group_create", "dgs_group_destroy", "dgs_group_last_error", "dgs_group_size", "dgs_group_uses_rccl", "dgs_group_rccl_ranks", "dgs_group_last_gather_used_rccl",
    "dgs_group_member", "dgs_group_set_input_target", "dgs_group_align_batch",
    "dgs_group_cloud_create", "dgs_group_cloud_destroy", "dgs_group_cloud_size", "dgs_group_cloud_copies", "dgs_group_cloud_trim", "dgs_group_set_input_target_cloud",
    "dgs_group_align_batch_clouds",
    "dgs_icp_options_init", "dgs_set_icp_options", "dgs_group_set_icp_options", "dgs_icp_get_trajectory",
    "dgs_pcl_gicp_options_init", "dgs_set_pcl_gicp_options", "dgs_group_set_pcl_gicp_options", "dgs_pcl_gicp_get_trajectory",
    "dgs_pcl_gicp_set_probe", "dgs_pcl_gicp_evaluate", "dgs_pcl_gicp_set_correspondence_randomness",
    "dgs_set_batch_independent", "dgs_get_batch_independent", "dgs_group_set_batch_independent",
    "dgs_prefilter_params_init", "dgs_prefilter", "dgs_prefilter_distance", "dgs_prefilter_radius", "dgs_prefilter_statistical",
    "dgs_prefilter_normal", "dgs_prefilter_get_statistics", "dgs_prefilter_get_normals",
    "dgs_prefilter_scan_params_init", "dgs_prefilter_scan", "dgs_prefilter_deskew",
    "dgs_map_cloud_params_init", "dgs_map_cloud_generate", "dgs_map_cloud_generate_clouds", "dgs_map_cloud_get", "dgs_map_cloud_get_grid",
    "dgs_line_extraction_params_init", "dgs_line_extraction", "dgs_line_extraction_get_rounds",
    "dgs_line_align_params_init", "dgs_line_align_global", "dgs_line_merge", "dgs_line_edges", "dgs_line_align_get_hypotheses",
    "dgs_line_align_local_batch", "dgs_line_align_local", "dgs_line_edges_angular", "dgs_line_align_local_get_hypotheses",
    "dgs_building_overlap_pairs", "dgs_line_align_overlapped_batch", "dgs_line_align_overlapped", "dgs_line_align_overlapped_get_hypotheses",
    "dgs_building_overlap_get_counts",
    "dgs_line_edge_extraction_batch", "dgs_line_edge_extraction", "dgs_line_edges_get_counts",
    "dgs_floor_detection_params_init", "dgs_floor_detection", "dgs_floor_detection_get_filtered", "dgs_floor_detection_get_inliers",
    "dgs_floor_detection_get_trace", "dgs_floor_detection_get_clipped", "dgs_floor_detection_draws", "dgs_floor_detection_walk",
    "dgs_calc_fitness_score_batch_clouds", "dgs_cloud_build_indices", "dgs_fitness_batch_get_counts",
    "dgs_building_cloud_params_init", "dgs_building_cloud_generate", "dgs_building_cloud_get", "dgs_building_cloud_get_counts",
    "dgs_cloud_assign_batch", "dgs_cloud_assign_get_counts", "dgs_cloud_read", "dgs_calc_inlier_fraction_batch_clouds",
    "dgs_cloud_build_covariances", "dgs_cloud_covariances_get_counts",
    "dgs_prefilter_scan_batch", "dgs_prefilter_batch_get_counts", "dgs_prefilter_batch_get_statistics",
    "dgs_floor_detection_batch", "dgs_floor_detection_batch_get_filtered", "dgs_floor_detection_batch_get_inliers",
    "dgs_floor_detection_batch_get_trace", "dgs_floor_detection_batch_get_clipped", "dgs_floor_detection_batch_get_counts",
]

_libs = {}
EXPERIMENTS_LIB_PATH = os.path.join(_HERE, "libdgs_reg_exp.so")   # `make experiments`: + nn_grid.hip and the packed-FP32 kernel (measured losers)


def load(path=None):
    """Load libdgs_reg.so (or another build of it, e.g. EXPERIMENTS_LIB_PATH).  Raises ImportError (never falls back) when it has
    not been built."""
    path = path or LIB_PATH
    if path in _libs:
        return _libs[path]
    if not os.path.exists(path):
        raise ImportError(
            f"{path} is missing: build the HIP extension first (python -c 'import __graft_entry__ as g; g.build()' "
            "or make -C delta_graph_slam_amd/csrc).  delta_graph_slam_amd has no CPU fallback.")
    lib = C.CDLL(path)
    P = C.POINTER
    lib.dgs_last_error.restype = C.c_char_p
    lib.dgs_last_error.argtypes = [C.c_void_p]
    lib.dgs_params_init.argtypes = [P(Params), C.c_int32]
    lib.dgs_create.argtypes = [P(Params), P(C.c_void_p)]
    lib.dgs_destroy.argtypes = [C.c_void_p]
    lib.dgs_destroy.restype = None
    lib.dgs_set_stream.argtypes = [C.c_void_p, C.c_void_p]
    lib.dgs_synchronize.argtypes = [C.c_void_p]
    lib.dgs_set_input_target.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32]
    lib.dgs_set_input_source.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32]
    lib.dgs_align.argtypes = [C.c_void_p, C.c_void_p, P(Result), C.c_void_p, C.c_int32]
    lib.dgs_get_fitness_score.argtypes = [C.c_void_p, C.c_double, P(C.c_double)]
    lib.dgs_get_inlier_fraction.argtypes = [C.c_void_p, C.c_double, P(C.c_double)]
    lib.dgs_nearest_search_target.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p]
    lib.dgs_nn_fitness_distances.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p]
    lib.dgs_align_batch.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32,
                                    C.c_double, P(Result)]
    lib.dgs_find_loop_candidates.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_double, C.c_void_p, C.c_double, C.c_double, C.c_void_p,
                                             C.c_int64, P(C.c_int64)]
    lib.dgs_calc_fitness_score.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_double, P(C.c_double)]
    lib.dgs_calc_fitness_score_batch_clouds.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_void_p, C.c_void_p]
    lib.dgs_calc_inlier_fraction_batch_clouds.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_void_p, C.c_void_p]
    lib.dgs_cloud_assign_batch.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_float, C.c_void_p, C.c_void_p]
    lib.dgs_cloud_assign_get_counts.argtypes = [C.c_void_p, C.c_void_p]
    lib.dgs_cloud_read.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, P(C.c_int64)]
    lib.dgs_cloud_build_indices.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
    lib.dgs_fitness_batch_get_counts.argtypes = [C.c_void_p, C.c_void_p]
    lib.dgs_cloud_build_covariances.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
    lib.dgs_cloud_covariances_get_counts.argtypes = [C.c_void_p, C.c_void_p]
    lib.dgs_voxel_grid_filter.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_float, C.c_void_p, C.c_int64, C.c_int32, P(C.c_int64)]
    lib.dgs_approx_voxel_grid_filter.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_float, C.c_void_p, C.c_int64, C.c_int32, P(C.c_int64)]
    lib.dgs_cloud_create.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, P(C.c_void_p)]
    lib.dgs_cloud_destroy.argtypes = [C.c_void_p]
    lib.dgs_cloud_destroy.restype = None
    lib.dgs_cloud_size.argtypes = [C.c_void_p]
    lib.dgs_cloud_size.restype = C.c_int64
    lib.dgs_set_input_target_cloud.argtypes = [C.c_void_p, C.c_void_p]
    lib.dgs_set_input_source_cloud.argtypes = [C.c_void_p, C.c_void_p]
    lib.dgs_align_batch_clouds.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_double, P(Result)]
    lib.dgs_align_pairs_clouds.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_double, P(Result)]
    lib.dgs_profile_enable.argtypes = [C.c_void_p, C.c_int32]
    lib.dgs_profile_get.argtypes = [C.c_void_p, C.c_int32, P(C.c_double), P(C.c_int64)]
    lib.dgs_profile_reset.argtypes = [C.c_void_p]
    lib.dgs_get_counts.argtypes = [C.c_void_p, P(C.c_int64)]
    lib.dgs_ndt_derivatives.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, P(C.c_double), C.c_void_p, C.c_void_p]
    lib.dgs_ndt_hessian_double.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    lib.dgs_ndt_score_gradient.argtypes = [C.c_void_p, C.c_void_p, P(C.c_double), C.c_void_p]
    lib.dgs_deal_probe.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]
    lib.dgs_deal_probe_cost.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
    lib.dgs_strict_row_probe.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
    lib.dgs_pcl_ndt_neighbours.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p]
    lib.dgs_ndt_get_voxels.argtypes = [C.c_void_p, P(C.c_int64), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.dgs_ndt_get_trajectory.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, P(C.c_int32)]
    lib.dgs_gicp_get_covariances.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
    lib.dgs_gicp_linearize.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, P(C.c_double), C.c_void_p, C.c_void_p]
    lib.dgs_vgicp_get_voxels.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, P(C.c_int64)]
    lib.dgs_group_create.argtypes = [P(Params), C.c_void_p, C.c_int32, P(C.c_void_p)]
    lib.dgs_group_destroy.argtypes = [C.c_void_p]
    lib.dgs_group_destroy.restype = None
    lib.dgs_group_last_error.argtypes = [C.c_void_p]
    lib.dgs_group_last_error.restype = C.c_char_p
    lib.dgs_group_size.argtypes = [C.c_void_p]
    lib.dgs_group_uses_rccl.argtypes = [C.c_void_p]
    lib.dgs_group_rccl_ranks.argtypes = [C.c_void_p]
    lib.dgs_group_last_gather_used_rccl.argtypes = [C.c_void_p]
    lib.dgs_group_member.argtypes = [C.c_void_p, C.c_int32]
    lib.dgs_group_member.restype = C.c_void_p
    lib.dgs_group_set_input_target.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
    lib.dgs_group_align_batch.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_double, P(Result), P(C.c_int32),
                                          P(C.c_double)]
    lib.dgs_group_cloud_create.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, P(C.c_void_p)]
    lib.dgs_group_cloud_destroy.argtypes = [C.c_void_p]
    lib.dgs_group_cloud_destroy.restype = None
    lib.dgs_group_cloud_size.argtypes = [C.c_void_p]
    lib.dgs_group_cloud_size.restype = C.c_int64
    lib.dgs_group_cloud_copies.argtypes = [C.c_void_p]
    lib.dgs_group_cloud_trim.argtypes = [C.c_void_p, C.c_void_p, C.c_int32]
    lib.dgs_group_set_input_target_cloud.argtypes = [C.c_void_p, C.c_void_p]
    lib.dgs_group_align_batch_clouds.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_double, P(Result), P(C.c_int32),
                                                 P(C.c_double)]
    lib.dgs_icp_options_init.argtypes = [P(IcpOptions)]
    lib.dgs_set_icp_options.argtypes = [C.c_void_p, P(IcpOptions)]
    lib.dgs_group_set_icp_options.argtypes = [C.c_void_p, P(IcpOptions)]
    lib.dgs_icp_get_trajectory.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, P(C.c_int32)]
    lib.dgs_pcl_gicp_options_init.argtypes = [P(PclGicpOptions)]
    lib.dgs_set_pcl_gicp_options.argtypes = [C.c_void_p, P(PclGicpOptions)]
    lib.dgs_group_set_pcl_gicp_options.argtypes = [C.c_void_p, P(PclGicpOptions)]
    lib.dgs_pcl_gicp_get_trajectory.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32,
                                                P(C.c_int32)]
    lib.dgs_pcl_gicp_set_correspondence_randomness.argtypes = [C.c_void_p, C.c_int32]
    lib.dgs_set_batch_independent.argtypes = [C.c_void_p, C.c_int32]
    lib.dgs_get_batch_independent.argtypes = [C.c_void_p, P(C.c_int32)]
    lib.dgs_group_set_batch_independent.argtypes = [C.c_void_p, C.c_int32]
    lib.dgs_pcl_gicp_set_probe.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    lib.dgs_pcl_gicp_evaluate.argtypes = [C.c_void_p, C.c_void_p, P(C.c_int32), P(C.c_double), C.c_void_p]
    lib.dgs_prefilter_params_init.argtypes = [P(PrefilterParams)]
    lib.dgs_prefilter.argtypes = [C.c_void_p, P(PrefilterParams), C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p,
                                  C.c_int64, C.c_int32, P(C.c_int64), P(C.c_int64)]
    lib.dgs_prefilter_distance.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_double, C.c_double, C.c_void_p, C.c_int64, C.c_int32,
                                           P(C.c_int64)]
    lib.dgs_prefilter_radius.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_double, C.c_int32, C.c_int32, C.c_void_p, C.c_int64,
                                         C.c_int32, P(C.c_int64)]
    lib.dgs_prefilter_statistical.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_double, C.c_int32, C.c_void_p,
                                              C.c_int64, C.c_int32, P(C.c_int64)]
    lib.dgs_prefilter_normal.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, P(C.c_int64)]
    lib.dgs_prefilter_get_statistics.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, P(C.c_int64)]
    lib.dgs_prefilter_get_normals.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, P(C.c_int64)]
    lib.dgs_prefilter_scan_params_init.argtypes = [P(PrefilterScanParams)]
    lib.dgs_prefilter_scan.argtypes = [C.c_void_p, P(PrefilterParams), P(PrefilterScanParams), C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_int64,
                                       C.c_void_p, C.c_int64, C.c_int32, P(C.c_int64), P(C.c_int64), C.c_void_p]
    lib.dgs_prefilter_scan_batch.argtypes = [C.c_void_p, P(PrefilterParams), C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p,
                                             C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.dgs_prefilter_batch_get_counts.argtypes = [C.c_void_p, C.c_void_p]
    lib.dgs_prefilter_batch_get_statistics.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, P(C.c_int64)]
    lib.dgs_prefilter_deskew.argtypes = [C.c_void_p, P(PrefilterScanParams), C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_int64, C.c_int32,
                                         P(C.c_int64)]
    lib.dgs_map_cloud_params_init.argtypes = [P(MapCloudParams)]
    lib.dgs_map_cloud_generate.argtypes = [C.c_void_p, P(MapCloudParams), C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_double,
                                           P(C.c_int64)]
    lib.dgs_map_cloud_generate_clouds.argtypes = [C.c_void_p, P(MapCloudParams), C.c_int32, C.c_void_p, C.c_void_p, C.c_double, P(C.c_int64)]
    lib.dgs_map_cloud_get.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, P(C.c_int64)]
    lib.dgs_map_cloud_get_grid.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, P(C.c_int32), P(C.c_int32)]
    lib.dgs_line_extraction_params_init.argtypes = [P(LineExtractionParams)]
    lib.dgs_line_extraction.argtypes = [C.c_void_p, P(LineExtractionParams), C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p,
                                        C.c_int64, P(C.c_int64), P(C.c_int32)]
    lib.dgs_line_extraction_get_rounds.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, P(C.c_int64), C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.dgs_line_align_params_init.argtypes = [P(LineAlignParams)]
    lib.dgs_line_align_global.argtypes = [C.c_void_p, P(LineAlignParams), C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int32, C.c_double,
                                          C.c_void_p, P(LineAlignment)]
    lib.dgs_line_merge.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, P(C.c_int64)]
    lib.dgs_line_edges.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, P(C.c_int64)]
    lib.dgs_line_align_get_hypotheses.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p]
    lib.dgs_line_align_local_batch.argtypes = [C.c_void_p, P(LineAlignParams), C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                               C.c_double, C.c_void_p, C.c_void_p]
    lib.dgs_line_align_local.argtypes = [C.c_void_p, P(LineAlignParams), C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_double, C.c_void_p,
                                         P(LineLocalAlignment)]
    lib.dgs_line_edges_angular.argtypes = [C.c_void_p, C.c_int64, C.c_int32, C.c_double, C.c_void_p, C.c_int64, P(C.c_int64)]
    lib.dgs_line_align_local_get_hypotheses.argtypes = [C.c_void_p, C.c_int64, C.c_int32, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p]
    lib.dgs_building_overlap_pairs.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, P(C.c_int64)]
    lib.dgs_line_align_overlapped_batch.argtypes = [C.c_void_p, P(LineAlignParams), C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                    C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.dgs_line_align_overlapped.argtypes = [C.c_void_p, P(LineAlignParams), C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                              C.c_void_p, P(LineOverlapAlignment)]
    lib.dgs_line_edge_extraction_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                                                   C.c_void_p, P(C.c_int64)]
    lib.dgs_line_edge_extraction.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_double, C.c_void_p, C.c_int64, P(C.c_int64)]
    lib.dgs_line_edges_get_counts.argtypes = [C.c_void_p, C.c_void_p]
    lib.dgs_line_align_overlapped_get_hypotheses.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_void_p]
    lib.dgs_building_overlap_get_counts.argtypes = [C.c_void_p, C.c_void_p]
    lib.dgs_floor_detection_params_init.argtypes = [P(FloorDetectionParams)]
    lib.dgs_floor_detection.argtypes = [C.c_void_p, P(FloorDetectionParams), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p,
                                        C.c_int64, C.c_void_p, P(C.c_int32)]
    lib.dgs_floor_detection_get_filtered.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, P(C.c_int64)]
    lib.dgs_floor_detection_get_inliers.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, P(C.c_int64)]
    lib.dgs_floor_detection_get_trace.argtypes = [C.c_void_p, P(FloorDetectionTrace)]
    lib.dgs_floor_detection_get_clipped.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, P(C.c_int64)]
    lib.dgs_floor_detection_draws.argtypes = [C.c_int64, C.c_void_p, C.c_int64, C.c_void_p]
    lib.dgs_floor_detection_walk.argtypes = [C.c_int64, C.c_int32, C.c_double, C.c_void_p, C.c_int64, P(C.c_int32), P(C.c_int32), P(C.c_int32)]
    lib.dgs_floor_detection_batch.argtypes = [C.c_void_p, P(FloorDetectionParams), C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32,
                                              C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.dgs_floor_detection_batch_get_filtered.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_int32, P(C.c_int64)]
    lib.dgs_floor_detection_batch_get_inliers.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, P(C.c_int64)]
    lib.dgs_floor_detection_batch_get_trace.argtypes = [C.c_void_p, C.c_int32, P(FloorDetectionTrace)]
    lib.dgs_floor_detection_batch_get_clipped.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, P(C.c_int64)]
    lib.dgs_floor_detection_batch_get_counts.argtypes = [C.c_void_p, C.c_void_p]
    lib.dgs_building_cloud_params_init.argtypes = [P(BuildingCloudParams)]
    lib.dgs_building_cloud_generate.argtypes = [C.c_void_p, P(BuildingCloudParams), C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                                P(C.c_int64)]
    lib.dgs_building_cloud_get.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, P(C.c_int64), P(C.c_void_p)]
    lib.dgs_building_cloud_get_counts.argtypes = [C.c_void_p, C.c_void_p]
    _libs[path] = lib
    return lib
