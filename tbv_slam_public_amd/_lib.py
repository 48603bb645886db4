"""ctypes binding of libcfear_hip.so (include/cfear_hip.h).

The library is built in-tree by tbv_slam_public_amd/csrc/Makefile (hipcc, gfx950).  There is no
CPU fallback: loading fails loudly if the .so is missing, and cfear_ctx_create fails with
CFEAR_ERR_NO_DEVICE when no MI355X is visible.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
SO_PATH = os.path.join(_HERE, "libcfear_hip.so")

OK = 0
ERR_INVALID_ARGUMENT, ERR_HIP, ERR_CAPACITY = -1, -2, -3
ERR_TOO_FEW_RESIDUALS, ERR_SOLVER, ERR_EMPTY_CLOUD, ERR_NO_DEVICE = -4, -5, -6, -7
ERR_IO, ERR_FORMAT = -8, -9

P2P, P2L, P2D = 0, 1, 2
LOSS = {"None": 0, "Huber": 1, "Cauchy": 2, "SoftLOne": 3, "Combined": 4, "Tukey": 5}
COST = {"P2P": 0, "P2L": 1, "P2D": 2}

# CFEAR_SURF_PATH_*: the route word of the surface-point kernels (cfear_scan_surface_path)
SURF_PATH_KIND_MASK, SURF_PATH_FAST, SURF_PATH_SINGLE, SURF_PATH_GLOBAL = 3, 1, 2, 3
SURF_PATH_ROWS, SURF_PATH_K64, SURF_PATH_WFLOAT, SURF_PATH_SLABS, SURF_PATH_READ2 = 0x4, 0x8, 0x10, 0x20, 0x40
SURF_PATH_TIER16, SURF_PATH_TIER4, SURF_PATH_TIER1, SURF_PATH_TOP_BUCKET, SURF_PATH_CEN_SCRATCH = 0x80, 0x100, 0x200, 0x400, 0x800
SURF_PATH_PREPARED, SURF_PATH_REASON_SHIFT, SURF_PATH_REASON_MASK = 0x1000, 13, 0xE000
SURF_REASON_REACH, SURF_REASON_ROTATION, SURF_REASON_POINTS, SURF_REASON_CELLS, SURF_REASON_ORDER, SURF_REASON_ROWS3 = 1, 2, 3, 4, 5, 6
SURF_PATH_SLAB_COUNT_SHIFT, SURF_PATH_SLAB_COUNT_MASK = 16, 0xFF0000


class CfearError(RuntimeError):
    def __init__(self, status, msg=""):
        super().__init__("cfear status %d: %s" % (status, msg))
        self.status = status


class PolarDesc(C.Structure):
    _fields_ = [("rows", C.c_int32), ("cols", C.c_int32), ("stride", C.c_int32), ("batch", C.c_int32),
                ("batch_stride", C.c_int64)]


class KStrongParams(C.Structure):
    _fields_ = [("k_strongest", C.c_int32), ("z_min", C.c_float), ("range_res", C.c_float),
                ("min_distance", C.c_float), ("want_peaks", C.c_int32)]


class KStrongOut(C.Structure):
    _fields_ = [("sel_range", C.c_void_p), ("sel_intensity", C.c_void_p), ("sel_count", C.c_void_p),
                ("is_peak", C.c_void_p), ("xyzi", C.c_void_p), ("n_points", C.c_void_p),
                ("xyzi_peaks", C.c_void_p), ("n_peaks", C.c_void_p)]


class CacfarParams(C.Structure):
    _fields_ = [("window_size", C.c_int32), ("nb_guard_cells", C.c_int32), ("false_alarm_rate", C.c_float),
                ("range_res", C.c_float), ("z_min", C.c_float), ("min_distance", C.c_float),
                ("max_distance", C.c_double)]


class CacfarPlan(C.Structure):     # struct cfear_cacfar_plan
    _fields_ = [(n, C.c_int32) for n in ("D", "DL", "nch", "wide", "pre_on", "lut_ok", "need_cols", "colsp", "bin_lo", "bin_hi",
                                         "pad_lo", "pad_hi", "keys", "cols_route", "cols_supported", "table_index")] + \
               [(n, C.c_int64) for n in ("lds_bytes", "piece_rows", "total_rows")]


ROWKEYS_BINS_MAJOR, CACFAR_PLAN_KEYS = 1, 0x100      # CFEAR_ROWKEYS_BINS_MAJOR, CFEAR_CACFAR_PLAN_KEYS


class KStrongPlan(C.Structure):    # struct cfear_kstrong_plan
    _fields_ = [(n, C.c_int32) for n in ("nchunk", "vec", "mask", "table_index", "u_zmin", "thi", "min_range_bin", "kpad",
                                         "refused", "pad")] + [("lds_bytes", C.c_int64)]


# CFEAR_KSTRONG_REFUSED_*
KSTRONG_REFUSED = {0: None, 1: "bad polar descriptor", 2: "cols > 8192", 3: "k_strongest outside [1, 1024]", 4: "range_res <= 0"}


class Cen2018Params(C.Structure):
    _fields_ = [("zq", C.c_float), ("sigma_gauss", C.c_int32), ("min_range_bins", C.c_int32), ("pad", C.c_int32),
                ("range_res", C.c_double)]


class Cen2019Params(C.Structure):
    _fields_ = [("max_points", C.c_int32), ("min_range_bins", C.c_int32), ("range_res", C.c_double)]


class Cell(C.Structure):
    _fields_ = [("mean", C.c_double * 2), ("normal", C.c_double * 2), ("cov", C.c_double * 4),
                ("scale", C.c_double), ("avg_intensity", C.c_double), ("lambda_min", C.c_double),
                ("lambda_max", C.c_double), ("nsamples", C.c_int32), ("pad", C.c_int32)]


CELL_DTYPE = np.dtype([("mean", "<f8", (2,)), ("normal", "<f8", (2,)), ("cov", "<f8", (4,)),
                       ("scale", "<f8"), ("avg_intensity", "<f8"), ("lambda_min", "<f8"),
                       ("lambda_max", "<f8"), ("nsamples", "<i4"), ("pad", "<i4")])
assert CELL_DTYPE.itemsize == C.sizeof(Cell) == 104


class FeatureParams(C.Structure):
    _fields_ = [("radius", C.c_float), ("downsample_factor", C.c_double), ("origin", C.c_double * 2),
                ("weight_intensity", C.c_int32), ("compensate", C.c_int32), ("mot", C.c_double * 3),
                ("ccw", C.c_int32), ("pad", C.c_int32)]


class RegParams(C.Structure):
    _fields_ = [("cost", C.c_int32), ("loss", C.c_int32), ("loss_limit", C.c_double),
                ("weight_opt", C.c_int32), ("max_itr_association", C.c_int32),
                ("max_itr_solver", C.c_int32), ("min_itr", C.c_int32), ("radius", C.c_double),
                ("cov_scale", C.c_double), ("regularization", C.c_double),
                ("score_tolerance", C.c_double), ("itr", C.c_int32), ("pad", C.c_int32)]


class RegResult(C.Structure):
    _fields_ = [("pose", C.c_double * 3), ("score", C.c_double), ("final_cost", C.c_double),
                ("num_residuals", C.c_int32), ("outer_iters", C.c_int32), ("lm_iters", C.c_int32),
                ("status", C.c_int32), ("last_relative_decrease", C.c_double), ("reserved", C.c_double)]


RESULT_DTYPE = np.dtype([("pose", "<f8", (3,)), ("score", "<f8"), ("final_cost", "<f8"),
                         ("num_residuals", "<i4"), ("outer_iters", "<i4"), ("lm_iters", "<i4"),
                         ("status", "<i4"), ("last_relative_decrease", "<f8"), ("reserved", "<f8")])
assert RESULT_DTYPE.itemsize == C.sizeof(RegResult) == 72


class RegJob(C.Structure):
    _fields_ = [("scans", C.POINTER(C.c_void_p)), ("n_scans", C.c_int32), ("pad", C.c_int32),
                ("poses_xyt", C.POINTER(C.c_double))]


class TieRecord(C.Structure):      # cfear_tie_record
    _fields_ = [(n, C.c_int32) for n in ("n_queries", "n_in_radius", "n_associated", "n_tied", "n_tied_effective", "max_group",
                                         "status", "pad")]


TIE_RECORD_DTYPE = np.dtype([(n, "<i4") for n in ("n_queries", "n_in_radius", "n_associated", "n_tied", "n_tied_effective",
                                                  "max_group", "status", "pad")])
assert TIE_RECORD_DTYPE.itemsize == C.sizeof(TieRecord) == 32
TIE_TILE = 1024                     # CFEAR_TIE_TILE


class VoxelAuditParams(C.Structure):      # cfear_voxel_audit_params
    _fields_ = [("radius", C.c_float), ("pad", C.c_float), ("downsample_factor", C.c_double)]


VOXEL_AUDIT_RECORD_DTYPE = np.dtype([(n, "<i4") for n in ("status", "n_points", "n_voxels", "n_centroids_reversed_differ", "n_pairs_exposed",
                                                          "n_voxels_exposed", "n_voxels_exposed_at_threshold", "n_voxels_changed_reversed",
                                                          "max_voxel_points", "pad")] + [("max_halfwidth", "<f8")])
VOXEL_AUDIT_VOXEL_DTYPE = np.dtype([("key", "<u4"), ("n_points", "<i4"), ("c_fwd", "<f4", (2,)), ("c_rev", "<f4", (2,)), ("e", "<f8", (2,)),
                                    ("n_sure_in", "<i4"), ("n_exposed", "<i4"), ("changed_reversed", "<i4"), ("pad", "<i4")])
assert C.sizeof(VoxelAuditParams) == 16 and VOXEL_AUDIT_RECORD_DTYPE.itemsize == 48 and VOXEL_AUDIT_VOXEL_DTYPE.itemsize == 56
CEN2019_ORDER_RECORD_DTYPE = np.dtype([(n, "<i4") for n in (                 # cfear_cen2019_order_record
    "n_candidates", "n_fresh", "n_sure_fresh", "n_possibly_fresh", "n_band", "n_rows_straddle_tied", "n_marks_in", "n_marks",
    "n_marks_out", "n_targets", "n_targets_certain", "n_targets_reversed", "n_targets_changed_reversed",
    "n_marks_changed_reversed")] + [("h_hi", "<f4"), ("h_lo", "<f4")])
assert CEN2019_ORDER_RECORD_DTYPE.itemsize == 64
VOXEL_AUDIT_TILE, VOXEL_AUDIT_MAX_POINTS = 1024, 40960      # CFEAR_VOXEL_AUDIT_TILE, CFEAR_VOXEL_AUDIT_MAX_POINTS

CANDIDATE_DTYPE = np.dtype([("target", "<i4"), ("source", "<i4"), ("target_xyt", "<f8", (3,)), ("source_xyt", "<f8", (3,))])
assert CANDIDATE_DTYPE.itemsize == 56


class CovSamplingParams(C.Structure):
    _fields_ = [("xy_range", C.c_double), ("yaw_range", C.c_double), ("samples_per_axis", C.c_int32),
                ("pad", C.c_int32), ("covariance_scaler", C.c_double)]


class CoralParams(C.Structure):
    _fields_ = [("radius", C.c_double), ("weight_res_intensity", C.c_int32), ("pad", C.c_int32)]


class CoralJob(C.Structure):
    _fields_ = [("ref_xyzi", C.c_void_p), ("src_xyzi", C.c_void_p), ("n_ref", C.c_int32), ("n_src", C.c_int32),
                ("ref_pose", C.c_double * 3), ("src_pose", C.c_double * 3), ("offset", C.c_double * 3)]


class CoralResult(C.Structure):
    _fields_ = [("joint", C.c_double), ("sep", C.c_double), ("overlap", C.c_double), ("valid", C.c_int32),
                ("count_valid", C.c_int32), ("status", C.c_int32), ("pad", C.c_int32)]


CORAL_RESULT_DTYPE = np.dtype([("joint", "<f8"), ("sep", "<f8"), ("overlap", "<f8"), ("valid", "<i4"),
                               ("count_valid", "<i4"), ("status", "<i4"), ("pad", "<i4")])


class P2pJob(C.Structure):        # cfear_p2p_job
    _fields_ = [("ref_xyzi", C.c_void_p), ("src_xyzi", C.c_void_p), ("n_ref", C.c_int32), ("n_src", C.c_int32),
                ("T", C.c_double * 6)]


P2P_RESULT_DTYPE = np.dtype([("mean", "<f8"), ("sum", "<f8"), ("matched", "<i4"), ("n_src", "<i4"), ("status", "<i4"),
                             ("pad", "<i4")])
assert C.sizeof(P2pJob) == 72 and P2P_RESULT_DTYPE.itemsize == 32
P2P_MAX_REF_POINTS, P2P_MAX_SRC_POINTS = 16384, 1048576


class CartParams(C.Structure):    # cfear_cart_params
    _fields_ = [("radar_resolution", C.c_float), ("cart_resolution", C.c_float), ("cart_pixel_width", C.c_int32), ("pad", C.c_int32)]


class CartJob(C.Structure):       # cfear_cart_job
    _fields_ = [("src", C.c_void_p), ("ref", C.c_void_p), ("x", C.c_double), ("y", C.c_double), ("yaw", C.c_double)]


CART_RESULT_DTYPE = np.dtype([("abs_diff", "<f8"), ("status", "<i4"), ("pad", "<i4")])
assert C.sizeof(CartParams) == 16 and C.sizeof(CartJob) == 40 and CART_RESULT_DTYPE.itemsize == 16
CART_MAX_WIDTH = 4096


class ScParams(C.Structure):
    _fields_ = [("num_ring", C.c_int32), ("num_sector", C.c_int32), ("max_radius", C.c_double),
                ("search_ratio", C.c_double), ("desc_function", C.c_int32), ("pad", C.c_int32),
                ("desc_divider", C.c_double), ("no_point", C.c_double)]


class ScCloud(C.Structure):
    _fields_ = [("xyzi", C.c_void_p), ("n", C.c_int32), ("pad", C.c_int32)]


SC_INTER_AREA = 3                   # CFEAR_SC_INTER_AREA (cv::INTER_AREA)


class ScRawParams(C.Structure):
    _fields_ = [("radar_threshold", C.c_double), ("transpose", C.c_int32), ("normalize", C.c_int32),
                ("interpolation", C.c_int32), ("pad", C.c_int32)]


class ScManagerParams(C.Structure):
    _fields_ = [("sc", ScParams), ("num_candidates_from_tree", C.c_int32), ("n_candidates", C.c_int32),
                ("odom_sigma_error", C.c_double), ("odometry_coupled_closure", C.c_int32), ("augment_sc", C.c_int32),
                ("distance_exclude_recent", C.c_double), ("pad", C.c_int64)]


class ScNode(C.Structure):         # cfear_sc_node
    _fields_ = [("cloud", ScCloud), ("T", C.c_double * 8), ("Tinv", C.c_double * 8), ("id", C.c_int32), ("pad", C.c_int32)]


SC_NODES_CLOUD, SC_NODES_RAW = 0, 1   # CFEAR_SC_NODES_*


class ScBatch(C.Structure):        # cfear_sc_batch
    _fields_ = [("n_graphs", C.c_int32), ("mode", C.c_int32), ("node_off", C.c_void_p), ("n_detect", C.c_void_p),
                ("ids", C.c_void_p), ("T", C.c_void_p), ("Tinv", C.c_void_p), ("xyzi", C.c_void_p), ("point_off", C.c_void_p),
                ("n_aggregate", C.c_int32), ("pad", C.c_int32), ("imgs", C.c_void_p), ("desc", C.POINTER(PolarDesc)),
                ("raw", C.POINTER(ScRawParams))]


SC_CANDIDATE_DTYPE = np.dtype([("min_dist", "<f8"), ("min_dist_sc", "<f8"), ("min_dist_odom", "<f8"),
                               ("yaw_diff_rad", "<f4"), ("nn_idx", "<i4"), ("argmin_shift", "<i4"), ("pad", "<i4"),
                               ("Taug", "<f8", (3,))])
assert SC_CANDIDATE_DTYPE.itemsize == 64


class VerifyParams(C.Structure):
    _fields_ = [("align_intercept", C.c_double), ("align_coef", C.c_double * 6), ("loop_intercept", C.c_double),
                ("loop_coef", C.c_double * 3), ("model_threshold", C.c_double), ("all_candidates", C.c_int32),
                ("verification_disabled", C.c_int32), ("use_covariance_sampling", C.c_int32), ("pad", C.c_int32),
                ("coral", CoralParams), ("sampling", CovSamplingParams)]


class VerifyJob(C.Structure):
    _fields_ = [("from_scan", C.c_void_p), ("to_scan", C.c_void_p), ("from_peaks", C.c_void_p),
                ("to_peaks", C.c_void_p), ("n_from", C.c_int32), ("n_to", C.c_int32), ("from_pose", C.c_double * 3),
                ("t_be_guess", C.c_double * 3), ("sc_sim", C.c_double), ("odom_bounds", C.c_double),
                ("group", C.c_int32), ("pad", C.c_int32)]


class VerifyResult(C.Structure):
    _fields_ = [("t_be", C.c_double * 3), ("cov", C.c_double * 36), ("coral", C.c_double * 3),
                ("cfear", C.c_double * 3), ("alignment_quality", C.c_double), ("odom_bounds", C.c_double),
                ("sc_sim", C.c_double), ("probability", C.c_double), ("reg_ok", C.c_int32),
                ("cov_sampled", C.c_int32), ("accepted", C.c_int32), ("rank", C.c_int32), ("reg", RegResult)]


VERIFY_RESULT_DTYPE = np.dtype([("t_be", "<f8", (3,)), ("cov", "<f8", (6, 6)), ("coral", "<f8", (3,)),
                                ("cfear", "<f8", (3,)), ("alignment_quality", "<f8"), ("odom_bounds", "<f8"),
                                ("sc_sim", "<f8"), ("probability", "<f8"), ("reg_ok", "<i4"), ("cov_sampled", "<i4"),
                                ("accepted", "<i4"), ("rank", "<i4"), ("reg", RESULT_DTYPE)])
assert VERIFY_RESULT_DTYPE.itemsize == C.sizeof(VerifyResult) == 480


class OdometryParams(C.Structure):
    _fields_ = [("filter_type", C.c_int32), ("kstrong", KStrongParams), ("cacfar", CacfarParams),
                ("reg", RegParams), ("res", C.c_float), ("submap_scan_size", C.c_int32),
                ("weight_intensity", C.c_int32), ("use_guess", C.c_int32), ("compensate", C.c_int32),
                ("radar_ccw", C.c_int32), ("use_keyframe", C.c_int32), ("rotate_ccw", C.c_int32),
                ("min_keyframe_dist", C.c_double), ("min_keyframe_rot_deg", C.c_double),
                ("downsample_factor", C.c_double), ("estimate_cov_by_sampling", C.c_int32), ("keep_nodes", C.c_int32),
                ("cov_sampling", CovSamplingParams)]


class FrameInfo(C.Structure):
    _fields_ = [("pose", C.c_double * 3), ("n_points", C.c_int32), ("n_cells", C.c_int32),
                ("keyframe_added", C.c_int32), ("reg_status", C.c_int32), ("outer_iters", C.c_int32),
                ("lm_iters", C.c_int32), ("score", C.c_double)]


FRAMEINFO_DTYPE = np.dtype([("pose", "<f8", (3,)), ("n_points", "<i4"), ("n_cells", "<i4"),
                            ("keyframe_added", "<i4"), ("reg_status", "<i4"), ("outer_iters", "<i4"),
                            ("lm_iters", "<i4"), ("score", "<f8")])
assert FRAMEINFO_DTYPE.itemsize == C.sizeof(FrameInfo) == 56

# every symbol include/cfear_hip.h declares
EXPORTS = [
    "cfear_abi_version", "cfear_status_string", "cfear_ctx_create", "cfear_ctx_destroy",
    "cfear_ctx_synchronize", "cfear_last_error", "cfear_ctx_profile_enable", "cfear_ctx_profile_read",
    "cfear_filter_kstrongest", "cfear_filter_cacfar", "cfear_compensate", "cfear_scan_create",
    "cfear_scan_from_cells", "cfear_scan_size", "cfear_scan_get_cells", "cfear_scan_destroy",
    "cfear_reg_params_default", "cfear_register", "cfear_register_batch", "cfear_get_cost",
    "cfear_get_cost_batch", "cfear_cov_sampling_params_default", "cfear_covariance_by_sampling",
    "cfear_covariance_by_sampling_batch", "cfear_coral_params_default", "cfear_coral_quality",
    "cfear_coral_quality_batch", "cfear_sc_params_default", "cfear_sc_descriptors", "cfear_sc_distance_batch",
    "cfear_polar_rotate_ccw", "cfear_scan_closest_idx", "cfear_scan_surface_path",
    "cfear_sc_manager_params_default", "cfear_sc_manager_create", "cfear_sc_manager_add", "cfear_sc_manager_detect",
    "cfear_sc_manager_size", "cfear_sc_manager_destroy", "cfear_sc_raw_params_default", "cfear_sc_raw_descriptors",
    "cfear_sc_manager_add_raw", "cfear_sc_local_map_descriptors", "cfear_sc_detect_sequence",
    "cfear_verify_params_default", "cfear_verify_loop_candidates", "cfear_verify_by_odometry", "cfear_verify_apply_constraints",
    "cfear_cost_prepare", "cfear_cost_num_blocks", "cfear_cost_num_residuals", "cfear_cost_get_blocks",
    "cfear_cost_evaluate", "cfear_cost_normal_eq", "cfear_cost_destroy",
    "cfear_odometry_params_default", "cfear_odometry_params_preset", "cfear_odometry_create", "cfear_odometry_process",
    "cfear_odometry_process_prefetch", "cfear_odometry_get_covariance", "cfear_odometry_destroy",
    "cfear_odometry_get_scan", "cfear_odometry_get_cloud", "cfear_odometry_get_peaks", "cfear_odometry_process_clouds",
    "cfear_odometry_process_offsets", "cfear_odometry_discard_prefetch",
    "cfear_keyframe_based_fuse", "cfear_acc_vel_sanity_check", "cfear_filter_kstrongest_legacy", "cfear_filter_kstrongest_rowkeys",
    "cfear_graph_save", "cfear_graph_load", "cfear_graph_size", "cfear_graph_node_at", "cfear_graph_destroy",
    "cfear_pose3d_from_xyt", "cfear_pose3d_to_xyt", "cfear_odometry_get_constraint",
    "cfear_shard_range", "cfear_gather_records", "cfear_register_batch_sharded", "cfear_verify_loop_candidates_sharded",
    "cfear_rccl_allgather", "cfear_rccl_allgather_device", "cfear_pgo_params_default", "cfear_pgo_solve", "cfear_pgo_solve_batch",
    "cfear_scan_table_create", "cfear_scan_table_size", "cfear_scan_table_destroy", "cfear_register_candidates",
    "cfear_ctx_get_stream", "cfear_ctx_set_option", "cfear_ctx_get_option",
    "cfear_rccl_unique_id", "cfear_rccl_comm_init", "cfear_rccl_comm_destroy",
    "cfear_candidate_pipe_create", "cfear_candidate_pipe_submit", "cfear_candidate_pipe_collect", "cfear_candidate_pipe_destroy", "cfear_candidate_pipe_stats",
    "cfear_eval_params_default", "cfear_eval_trajectories", "cfear_eval_check", "cfear_kitti_read", "cfear_kitti_write",
    "cfear_kitti_from_xyt", "cfear_cen2018_params_default", "cfear_filter_cen2018",
    "cfear_cen2019_params_default", "cfear_filter_cen2019",
    "cfear_logreg_params_default", "cfear_logreg_fit_batch", "cfear_p2p_quality", "cfear_p2p_quality_batch",
    "cfear_cart_params_default", "cfear_polar_to_cartesian", "cfear_cart_quality_batch",
    "cfear_cacfar_plan", "cfear_filter_cacfar_rowkeys", "cfear_kstrong_plan",
    "cfear_closure_params_default", "cfear_closure_candidates_batch",
    "cfear_loop_stats_params_default", "cfear_loop_stats_batch", "cfear_loop_curves_params_default", "cfear_loop_curves_batch",
    "cfear_sync_trajectories", "cfear_tum_write", "cfear_cov_write",
    "cfear_graph_align_batch", "cfear_graph_map_batch", "cfear_graph_string_write", "cfear_graph_output_write",
    "cfear_association_ties_batch", "cfear_scan_closest_ties",
    "cfear_voxel_audit_params_default", "cfear_voxel_order_audit_batch",
    "cfear_cen2019_order_audit",
    "cfear_scan_create_batch", "cfear_scan_batch_size", "cfear_scan_batch_get", "cfear_scan_batch_destroy",
    "cfear_odometry_replay_clouds", "cfear_odometry_replay",
    "cfear_sc_detect_batch",
    "cfear_kstrong_rowkeys_derive",
    "cfear_odometry_grid_plan", "cfear_odometry_grid_create", "cfear_odometry_grid_process", "cfear_odometry_grid_destroy",
    "cfear_loop_verify_params_default", "cfear_verify_graph_candidates", "cfear_verify_sc_rows",
    "cfear_cov_fit_records", "cfear_covariance_by_sampling_candidates", "cfear_verify_sample_covariances",
]


class RowkeysClass(C.Structure):    # cfear_rowkeys_class
    _fields_ = [("image", C.c_int32), ("k_strongest", C.c_int32), ("z_min", C.c_float), ("range_res", C.c_float),
                ("min_distance", C.c_float)]


# cfear_grid_stream: one record per stream of cfear_odometry_grid_plan
GRID_STREAM_DTYPE = np.dtype([(n, "<i4") for n in ("sequence", "config", "sweep", "filter_class", "surface_group", "matcher_group",
                                                   "surface_slot", "matcher_slot")])


class GridTotals(C.Structure):      # cfear_grid_totals
    _fields_ = [(n, C.c_int32) for n in ("n_streams", "n_sequences", "n_sweeps", "n_classes", "n_derived_classes",
                                         "max_classes_per_sequence", "n_surface_groups", "n_matcher_groups")]
REPLAY_AUDIT = 1                    # #define CFEAR_REPLAY_AUDIT

# cfear_replay_frame: one record per frame of a replay (cfear_odometry_replay_clouds)
REPLAY_FRAME_DTYPE = np.dtype([("pose", "<f8", 3), ("guess", "<f8", 3), ("dev", "<f8", 3), ("score", "<f8"), ("final_cost", "<f8"),
                               ("last_relative_decrease", "<f8")] +
                              [(n, "<i4") for n in ("n_points", "n_cells", "is_keyframe", "n_targets", "reg_status", "outer_iters", "lm_iters",
                                                    "num_residuals", "sanity_ok", "n_tied_start", "n_tied_effective_start", "n_tied_end",
                                                    "n_tied_effective_end", "n_voxels_exposed", "n_voxels_changed_reversed", "exposed")])
assert REPLAY_FRAME_DTYPE.itemsize == 160

PIPE_GRAPH, PIPE_TIMING = 1, 2      # enum { CFEAR_PIPE_GRAPH, CFEAR_PIPE_TIMING }


class RcclComm(C.Structure):        # cfear_rccl_comm
    _fields_ = [("ctx", C.c_void_p), ("nccl_comm", C.c_void_p), ("world", C.c_int32), ("pad", C.c_int32)]


# enum cfear_option (include/cfear_hip.h): test / measurement hooks of a context
OPT_FUSED_DECODE, OPT_MATCHER_LDS_KB, OPT_MATCHER_WAVES, OPT_HOST_TIMELINE, OPT_SC_QUERY_CHUNK, OPT_COUNT = 0, 1, 2, 3, 4, 5
# OPT_COUNT counts the options above, which all take 0 as "the library's choice"; it is NOT the header's CFEAR_OPT_COUNT (6).
# CFEAR_OPT_PGO_GRAPH_CHUNK follows them with a different value range: n >= 1 graphs per chunk of cfear_pgo_solve_batch, 0 refused.
OPT_PGO_GRAPH_CHUNK = 5
OPT_REPLAY_CHUNK = 100              # #define CFEAR_OPT_REPLAY_CHUNK: frames per chunk of a replay, 0 = by free memory (numbered apart from the enum)
OPT_KSTRONG_ROW_PAIRS = 101         # #define CFEAR_OPT_KSTRONG_ROW_PAIRS: 1 (default) two rows per wavefront in the k-strongest sweep, 0 = the single-row table


class PgoParams(C.Structure):
    _fields_ = [("loop_vxx", C.c_double), ("loop_vyy", C.c_double), ("loop_vtt", C.c_double), ("odom_vxx", C.c_double),
                ("odom_vyy", C.c_double), ("odom_vtt", C.c_double), ("loop_scaling", C.c_double),
                ("replace_cov_by_identity", C.c_int32), ("max_num_iterations", C.c_int32), ("loop_loss_limit", C.c_double)]


class PgoSummary(C.Structure):
    _fields_ = [("initial_cost", C.c_double), ("final_cost", C.c_double), ("iterations", C.c_int32), ("usable", C.c_int32),
                ("num_residual_blocks", C.c_int32), ("linear_iterations", C.c_int32)]



class Pose3d(C.Structure):
    _fields_ = [("p", C.c_double * 3), ("q", C.c_double * 4)]


class GraphCloud(C.Structure):
    _fields_ = [("xyzi", C.c_void_p), ("n", C.c_int32), ("seq", C.c_uint32), ("stamp", C.c_uint64), ("frame_id", C.c_char_p)]


class GraphConstraint(C.Structure):
    _fields_ = [("id_begin", C.c_uint64), ("id_end", C.c_uint64), ("t_be", Pose3d), ("information", C.c_double * 36),
                ("type", C.c_int32), ("n_quality", C.c_int32), ("quality_keys", C.POINTER(C.c_char_p)),
                ("quality_values", C.POINTER(C.c_double)), ("info", C.c_char_p)]


# cfear_graph_constraint / cfear_pgo_summary as numpy records, for callers that marshal whole batches at once
GRAPH_CONSTRAINT_DTYPE = np.dtype([("id_begin", "<u8"), ("id_end", "<u8"), ("t_be", "<f8", (7,)), ("information", "<f8", (36,)),
                                   ("type", "<i4"), ("n_quality", "<i4"), ("quality_keys", "<u8"), ("quality_values", "<u8"),
                                   ("info", "<u8")])
PGO_SUMMARY_DTYPE = np.dtype([("initial_cost", "<f8"), ("final_cost", "<f8"), ("iterations", "<i4"), ("usable", "<i4"),
                              ("num_residual_blocks", "<i4"), ("linear_iterations", "<i4")])
assert GRAPH_CONSTRAINT_DTYPE.itemsize == C.sizeof(GraphConstraint) and PGO_SUMMARY_DTYPE.itemsize == C.sizeof(PgoSummary)


class GraphNode(C.Structure):
    _fields_ = [("T", Pose3d), ("Tgt", Pose3d), ("has_Tgt", C.c_int32), ("idx", C.c_uint32), ("stamp", C.c_uint64),
                ("motion", C.c_double * 16), ("cloud_peaks", GraphCloud), ("cloud_nopeaks", GraphCloud),
                ("has_normal", C.c_int32), ("input_is_nopeaks", C.c_int32), ("normal_input", GraphCloud),
                ("cells", C.c_void_p), ("n_cells", C.c_int32), ("radius", C.c_float), ("weight_intensity", C.c_int32),
                ("pad", C.c_int32), ("constraints", C.POINTER(GraphConstraint)), ("n_constraints", C.c_int32), ("pad2", C.c_int32)]


EVAL_NUM_LENGTHS = 8
EVAL_ALIGN = {"none": 0, None: 0, "6dof": 1, "scale": 2, "7dof": 3, "scale_7dof": 4}      # CFEAR_EVAL_ALIGN_*


class EvalParams(C.Structure):      # cfear_eval_params
    _fields_ = [("step_size", C.c_int32), ("alignment", C.c_int32), ("lengths", C.c_double * EVAL_NUM_LENGTHS)]


EVAL_SUMMARY_DTYPE = np.dtype([("ave_t_err", "<f8"), ("ave_r_err", "<f8"), ("ate", "<f8"), ("rpe_trans", "<f8"),
                               ("rpe_trans_dev", "<f8"), ("rpe_rot", "<f8"), ("rpe_rot_dev", "<f8"), ("bias_x", "<f8"),
                               ("bias_y", "<f8"), ("bias_theta", "<f8"), ("rmse_trans", "<f8"),
                               ("seg_t_err", "<f8", (EVAL_NUM_LENGTHS,)), ("seg_r_err", "<f8", (EVAL_NUM_LENGTHS,)),
                               ("align", "<f8", (12,)), ("n_rows", "<i8"), ("seg_count", "<i4", (EVAL_NUM_LENGTHS,)),
                               ("n_poses", "<i4"), ("status", "<i4")])
assert EVAL_SUMMARY_DTYPE.itemsize == 360
EVAL_ROW_DTYPE = np.dtype([("trajectory", "<i4"), ("first_frame", "<i4"), ("last_frame", "<i4"), ("pad", "<i4"),
                           ("length", "<f8"), ("r_err", "<f8"), ("t_err", "<f8"), ("speed", "<f8")])
assert EVAL_ROW_DTYPE.itemsize == 48

SYNC_MODE = {"chained": 0, "independent": 1}     # CFEAR_SYNC_CHAINED, CFEAR_SYNC_INDEPENDENT
SYNC_ROW_DTYPE = np.dtype([("est_index", "<i4"), ("gt_index", "<i4"), ("alpha", "<f8")])      # cfear_sync_row
assert SYNC_ROW_DTYPE.itemsize == 16

LOGREG_MAX_FEATURES = 8


class LogregParams(C.Structure):    # cfear_logreg_params
    _fields_ = [("C", C.c_double), ("class_weight_balanced", C.c_int32), ("fit_intercept", C.c_int32),
                ("max_iterations", C.c_int32), ("pad", C.c_int32)]


class LogregJob(C.Structure):       # cfear_logreg_job
    _fields_ = [("X", C.c_void_p), ("y", C.c_void_p), ("columns", C.POINTER(C.c_int32)), ("row_mask", C.c_void_p),
                ("n_rows", C.c_int64), ("row_stride", C.c_int32), ("n_features", C.c_int32)]


LOGREG_RESULT_DTYPE = np.dtype([("intercept", "<f8"), ("coef", "<f8", (LOGREG_MAX_FEATURES,)), ("objective", "<f8"),
                                ("grad_inf", "<f8"), ("balanced_accuracy", "<f8"), ("n_used", "<i8"), ("n_pos", "<i8"),
                                ("confusion", "<i8", (4,)), ("iterations", "<i4"), ("status", "<i4")])
assert C.sizeof(LogregParams) == 24 and C.sizeof(LogregJob) == 48 and LOGREG_RESULT_DTYPE.itemsize == 152

CLOSURE_MODE = {"gtvicinity": 0, "mini": 1}      # CFEAR_CLOSURE_GTVICINITY, CFEAR_CLOSURE_MINI
CLOSURE_ORIGINS, CLOSURE_TILE = 64, 256           # CFEAR_CLOSURE_ORIGINS, CFEAR_CLOSURE_TILE


class ClosureParams(C.Structure):   # cfear_closure_params
    _fields_ = [("mode", C.c_int32), ("verify_via_odometry", C.c_int32), ("min_d_travel", C.c_double),
                ("max_d_travel", C.c_double), ("max_d_close", C.c_double), ("odom_sigma_error", C.c_double)]


class ClosureCandidate(C.Structure):    # cfear_closure_candidate
    _fields_ = [("to", C.c_int32), ("exhausted", C.c_int32), ("eucl", C.c_double), ("trav", C.c_double), ("rel", C.c_double),
                ("odom_bounds", C.c_double)]


CLOSURE_CANDIDATE_DTYPE = np.dtype([("to", "<i4"), ("exhausted", "<i4"), ("eucl", "<f8"), ("trav", "<f8"), ("rel", "<f8"),
                                    ("odom_bounds", "<f8")])
assert C.sizeof(ClosureParams) == 40 and C.sizeof(ClosureCandidate) == 40 == CLOSURE_CANDIDATE_DTYPE.itemsize

LOOPEVAL_LDS_ROWS = 16384                         # CFEAR_LOOPEVAL_LDS_ROWS


class LoopStatsParams(C.Structure):     # cfear_loop_stats_params
    _fields_ = [("max_distance", C.c_double), ("max_registration_translation", C.c_double),
                ("max_registration_rotation_deg", C.c_double), ("no_loop_distance", C.c_double), ("min_index_gap", C.c_int32),
                ("pad", C.c_int32)]


class LoopCurvesParams(C.Structure):    # cfear_loop_curves_params
    _fields_ = [("p_threshold", C.c_double), ("drop_intermediate", C.c_int32), ("reference_endpoints", C.c_int32)]


LOOP_CANDIDATE_DTYPE = np.dtype([("graph", "<i4"), ("from", "<i4"), ("to", "<i4"), ("guess_nr", "<i4"), ("guess_xyt", "<f8", (3,))])
LOOP_ROW_DTYPE = np.dtype([("diff", "<f8", (3,)), ("closest_loop_distance", "<f8"), ("candidate_loop_distance", "<f8"),
                           ("transl_error", "<f8"), ("rot_error", "<f8"), ("close_xy", "<f8", (2,)), ("id_close", "<i4"),
                           ("is_loop", "<i4"), ("candidate_close", "<i4"), ("prediction_pos_ok", "<i4")])
LOOP_CURVES_RESULT_DTYPE = np.dtype([("auc", "<f8"), ("accuracy", "<f8"), ("precision", "<f8"), ("recall", "<f8"), ("n_pos", "<i8"),
                                     ("n_neg", "<i8"), ("confusion", "<i8", (4,)), ("n_thresholds", "<i4"), ("n_roc", "<i4"),
                                     ("n_pr", "<i4"), ("status", "<i4")])
assert C.sizeof(LoopStatsParams) == 40 and C.sizeof(LoopCurvesParams) == 16
assert LOOP_CANDIDATE_DTYPE.itemsize == 40 and LOOP_ROW_DTYPE.itemsize == 88 and LOOP_CURVES_RESULT_DTYPE.itemsize == 96



class LoopGraphs(C.Structure):          # cfear_loop_graphs
    _fields_ = [("n_graphs", C.c_int32), ("pad", C.c_int32), ("node_off", C.c_void_p), ("table", C.c_void_p), ("peaks_xyzi", C.c_void_p),
                ("peak_off", C.c_void_p), ("poses_xyt", C.c_void_p), ("rel_xyt", C.c_void_p)]


class LoopVerifyParams(C.Structure):    # cfear_loop_verify_params
    _fields_ = [("verify", VerifyParams), ("odom_sigma_error", C.c_double), ("verify_via_odometry", C.c_int32),
                ("transl_guess", C.c_int32), ("speedup", C.c_int32), ("odometry_coupled_closure", C.c_int32)]


LOOP_VERIFY_CANDIDATE_DTYPE = np.dtype([("graph", "<i4"), ("from", "<i4"), ("to", "<i4"), ("guess_nr", "<i4"), ("query", "<i4"),
                                        ("skip", "<i4"), ("guess_xyt", "<f8", (3,)), ("sc_sim", "<f8"), ("odom_term", "<f8")])
LOOP_SPEEDUP_ODOM = 0.7                           # CFEAR_LOOP_SPEEDUP_ODOM
assert C.sizeof(LoopGraphs) == 56 and C.sizeof(LoopVerifyParams) == 184 and LOOP_VERIFY_CANDIDATE_DTYPE.itemsize == 64

GRAPH_MAP_TILE = 256                              # CFEAR_GRAPH_MAP_TILE


class GraphMapParams(C.Structure):      # cfear_graph_map_params
    _fields_ = [("skip_frames", C.c_int32), ("want_gt_map", C.c_int32)]


GRAPH_ALIGN_SUMMARY_DTYPE = np.dtype([("align", "<f8", (12,)), ("ate", "<f8"), ("n_gt", "<i4"), ("status", "<i4")])
GRAPH_MAP_SUMMARY_DTYPE = np.dtype([("map_offset", "<i8"), ("map_points", "<i8"), ("map_gt_offset", "<i8"), ("map_gt_points", "<i8")])
assert C.sizeof(GraphMapParams) == 8 and GRAPH_ALIGN_SUMMARY_DTYPE.itemsize == 112 and GRAPH_MAP_SUMMARY_DTYPE.itemsize == 32

_LIB = None


def lib():
    """Loads libcfear_hip.so; raises if it has not been built (no fallback)."""
    global _LIB
    if _LIB is not None:
        return _LIB
    if not os.path.exists(SO_PATH):
        raise ImportError("libcfear_hip.so not built: run `make -C %s/csrc` (or __graft_entry__.build())" % _HERE)
    # PyTorch-ROCm bundles its own libamdhip64; it must be the process's HIP runtime BEFORE this
    # library is loaded, otherwise two runtimes coexist and torch device pointers / streams cannot be
    # shared with the kernels (torch is plumbing here: device memory, streams, torch.distributed).
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = C.CDLL(SO_PATH)
    vp = C.c_void_p
    L.cfear_abi_version.restype = C.c_int
    L.cfear_status_string.restype = C.c_char_p
    L.cfear_status_string.argtypes = [C.c_int]
    L.cfear_ctx_create.argtypes = [C.c_int, vp, C.POINTER(vp)]
    L.cfear_ctx_destroy.argtypes = [vp]
    L.cfear_ctx_synchronize.argtypes = [vp]
    L.cfear_ctx_get_stream.argtypes = [vp, C.POINTER(C.c_void_p)]
    L.cfear_ctx_set_option.argtypes = [vp, C.c_int32, C.c_int64]
    L.cfear_ctx_get_option.argtypes = [vp, C.c_int32, C.POINTER(C.c_int64)]
    L.cfear_last_error.argtypes = [vp]
    L.cfear_last_error.restype = C.c_char_p
    L.cfear_ctx_profile_enable.argtypes = [vp, C.c_int]
    L.cfear_ctx_profile_read.argtypes = [vp, C.POINTER(C.c_char_p), C.POINTER(C.c_double),
                                         C.POINTER(C.c_int64), C.c_int, C.c_int]
    L.cfear_scan_table_create.argtypes = [vp, C.POINTER(vp), C.c_int32, C.POINTER(vp)]
    L.cfear_scan_table_size.argtypes = [vp]
    L.cfear_scan_table_destroy.argtypes = [vp]
    L.cfear_register_candidates.argtypes = [vp, vp, vp, C.c_int32, vp, vp]
    L.cfear_filter_kstrongest.argtypes = [vp, vp, C.POINTER(PolarDesc), C.POINTER(KStrongParams),
                                          C.POINTER(KStrongOut)]
    L.cfear_filter_cacfar.argtypes = [vp, vp, C.POINTER(PolarDesc), C.POINTER(CacfarParams), vp, vp,
                                      C.c_int32, vp]
    L.cfear_cacfar_plan.argtypes = [C.POINTER(PolarDesc), C.POINTER(CacfarParams), C.c_int32, C.POINTER(CacfarPlan)]
    L.cfear_kstrong_plan.argtypes = [C.POINTER(PolarDesc), C.POINTER(KStrongParams), C.c_uint64, C.POINTER(KStrongPlan)]
    L.cfear_filter_cacfar_rowkeys.argtypes = [vp, vp, C.POINTER(PolarDesc), C.POINTER(CacfarParams), C.c_int32, vp, vp, C.c_int32]
    L.cfear_cen2018_params_default.argtypes = [C.POINTER(Cen2018Params)]
    L.cfear_cen2018_params_default.restype = None
    L.cfear_filter_cen2018.argtypes = [vp, vp, C.POINTER(PolarDesc), C.POINTER(Cen2018Params), vp, vp, C.c_int32, vp, vp, vp]
    L.cfear_cen2019_params_default.argtypes = [C.POINTER(Cen2019Params)]
    L.cfear_cen2019_params_default.restype = None
    L.cfear_filter_cen2019.argtypes = [vp, vp, C.POINTER(PolarDesc), C.POINTER(Cen2019Params), vp, vp, C.c_int32, vp, vp, vp, vp]
    L.cfear_cen2019_order_audit.argtypes = [vp, vp, C.POINTER(PolarDesc), C.POINTER(Cen2019Params), vp, vp, vp, C.c_int32, vp]
    L.cfear_compensate.argtypes = [vp, vp, C.c_int32, C.POINTER(C.c_double), C.c_int32]
    L.cfear_scan_create.argtypes = [vp, vp, C.c_int32, C.POINTER(FeatureParams), C.POINTER(vp)]
    L.cfear_scan_from_cells.argtypes = [vp, vp, C.c_int32, C.POINTER(vp)]
    L.cfear_scan_size.argtypes = [vp]
    L.cfear_scan_get_cells.argtypes = [vp, vp, C.c_int32]
    L.cfear_scan_destroy.argtypes = [vp]
    L.cfear_reg_params_default.argtypes = [C.POINTER(RegParams)]
    L.cfear_reg_params_default.restype = None
    L.cfear_register.argtypes = [vp, C.POINTER(vp), C.c_int32, C.POINTER(C.c_double),
                                 C.POINTER(RegParams), C.POINTER(RegResult)]
    L.cfear_register_batch.argtypes = [vp, C.POINTER(RegJob), C.c_int32, C.POINTER(RegParams), vp]
    L.cfear_get_cost_batch.argtypes = [vp, C.POINTER(RegJob), C.c_int32, C.POINTER(RegParams), vp]
    L.cfear_cov_sampling_params_default.argtypes = [C.POINTER(CovSamplingParams)]
    L.cfear_cov_sampling_params_default.restype = None
    L.cfear_covariance_by_sampling.argtypes = [vp, C.POINTER(vp), C.c_int32, C.POINTER(C.c_double),
                                               C.POINTER(RegParams), C.POINTER(RegResult),
                                               C.POINTER(CovSamplingParams), C.POINTER(C.c_double),
                                               C.POINTER(C.c_double), C.POINTER(C.c_int32)]
    L.cfear_covariance_by_sampling_batch.argtypes = [vp, C.POINTER(RegJob), C.c_int32, C.POINTER(RegParams), vp,
                                                     C.POINTER(CovSamplingParams), vp, vp, vp]
    L.cfear_coral_params_default.argtypes = [C.POINTER(CoralParams)]
    L.cfear_coral_params_default.restype = None
    L.cfear_coral_quality.argtypes = [vp, C.POINTER(CoralJob), C.POINTER(CoralParams), vp, vp]
    L.cfear_coral_quality_batch.argtypes = [vp, C.POINTER(CoralJob), C.c_int32, C.POINTER(CoralParams), vp, vp]
    L.cfear_p2p_quality.argtypes = [vp, C.POINTER(P2pJob), C.c_double, vp, vp]
    L.cfear_p2p_quality_batch.argtypes = [vp, C.POINTER(P2pJob), C.c_int32, C.c_double, vp, vp]
    L.cfear_cart_params_default.argtypes = [C.POINTER(CartParams)]
    L.cfear_cart_params_default.restype = None
    L.cfear_polar_to_cartesian.argtypes = [vp, vp, C.POINTER(PolarDesc), C.POINTER(CartParams), vp]
    L.cfear_cart_quality_batch.argtypes = [vp, C.POINTER(CartJob), C.c_int32, C.c_int32, C.c_float, vp, vp]
    L.cfear_sc_params_default.argtypes = [C.POINTER(ScParams)]
    L.cfear_sc_params_default.restype = None
    L.cfear_sc_descriptors.argtypes = [vp, C.POINTER(ScCloud), C.c_int32, C.POINTER(ScParams), C.POINTER(C.c_double),
                                       C.c_int32, vp, vp, vp]
    L.cfear_sc_distance_batch.argtypes = [vp, vp, C.c_int32, vp, C.c_int32, vp, C.c_int32, C.POINTER(ScParams), vp, vp]
    L.cfear_sc_manager_params_default.argtypes = [C.POINTER(ScManagerParams)]
    L.cfear_sc_manager_params_default.restype = None
    L.cfear_sc_manager_create.argtypes = [vp, C.POINTER(ScManagerParams), C.POINTER(vp)]
    L.cfear_sc_manager_add.argtypes = [vp, vp, C.c_int32, C.POINTER(C.c_double)]
    L.cfear_sc_manager_detect.argtypes = [vp, vp, C.c_int32, C.POINTER(C.c_int32)]
    L.cfear_sc_raw_params_default.argtypes = [C.POINTER(ScRawParams)]
    L.cfear_sc_raw_params_default.restype = None
    L.cfear_sc_raw_descriptors.argtypes = [vp, vp, C.POINTER(PolarDesc), C.POINTER(ScParams), C.POINTER(ScRawParams), vp, vp, vp]
    L.cfear_sc_manager_add_raw.argtypes = [vp, vp, C.POINTER(PolarDesc), C.POINTER(ScRawParams), C.POINTER(C.c_double)]
    L.cfear_sc_local_map_descriptors.argtypes = [vp, C.POINTER(ScNode), C.c_int32, vp, C.c_int32, C.c_int32, C.POINTER(ScParams),
                                                 C.POINTER(C.c_double), C.c_int32, vp, vp, vp]
    L.cfear_sc_detect_sequence.argtypes = [vp, C.POINTER(ScManagerParams), C.POINTER(ScNode), C.c_int32, C.c_int32, C.c_int32,
                                           vp, vp]
    L.cfear_sc_detect_batch.argtypes = [vp, C.POINTER(ScManagerParams), C.POINTER(ScBatch), vp, vp]
    L.cfear_sc_manager_size.argtypes = [vp]
    L.cfear_sc_manager_destroy.argtypes = [vp]
    L.cfear_scan_closest_idx.argtypes = [vp, vp, C.c_int32, C.c_double, vp]
    L.cfear_scan_closest_ties.argtypes = [vp, vp, C.c_int32, C.c_double, vp, vp, vp]
    L.cfear_association_ties_batch.argtypes = [vp, C.POINTER(RegJob), C.c_int32, C.POINTER(RegParams), C.c_int32, vp, vp, C.c_int64]
    L.cfear_voxel_audit_params_default.argtypes = [C.POINTER(VoxelAuditParams)]
    L.cfear_voxel_audit_params_default.restype = None
    L.cfear_voxel_order_audit_batch.argtypes = [vp, vp, vp, vp, C.c_int32, C.POINTER(VoxelAuditParams), vp, vp, C.c_int64, C.POINTER(C.c_int64)]
    L.cfear_scan_surface_path.argtypes = [vp, C.POINTER(C.c_uint32)]
    L.cfear_scan_create_batch.argtypes = [vp, vp, vp, vp, C.c_int32, C.POINTER(FeatureParams), vp, C.c_int32, C.POINTER(vp), vp]
    L.cfear_scan_batch_size.argtypes = [vp]
    L.cfear_scan_batch_get.argtypes = [vp, C.c_int32, C.POINTER(vp)]
    L.cfear_scan_batch_destroy.argtypes = [vp]
    L.cfear_odometry_replay_clouds.argtypes = [vp, C.POINTER(ScCloud), C.POINTER(OdometryParams), vp, vp, C.c_int32, C.c_int32, vp]
    L.cfear_odometry_replay.argtypes = [vp, C.POINTER(PolarDesc), vp, C.POINTER(OdometryParams), vp, vp, C.c_int32, C.c_int32, vp]
    L.cfear_polar_rotate_ccw.argtypes = [vp, vp, C.POINTER(PolarDesc), vp, C.c_int32, C.c_int64]
    L.cfear_verify_params_default.argtypes = [C.POINTER(VerifyParams)]
    L.cfear_verify_params_default.restype = None
    L.cfear_verify_loop_candidates.argtypes = [vp, C.POINTER(VerifyJob), C.c_int32, C.POINTER(VerifyParams), vp]
    L.cfear_verify_apply_constraints.argtypes = [vp, C.c_int32, C.POINTER(VerifyParams), vp]
    L.cfear_loop_verify_params_default.argtypes = [C.POINTER(LoopVerifyParams)]
    L.cfear_loop_verify_params_default.restype = None
    L.cfear_verify_graph_candidates.argtypes = [vp, C.POINTER(LoopGraphs), vp, C.c_int32, C.POINTER(LoopVerifyParams), vp, vp, vp]
    L.cfear_verify_sc_rows.argtypes = [vp, C.POINTER(LoopGraphs), vp, vp, vp, C.c_int32, C.POINTER(LoopVerifyParams), vp, vp, vp,
                                       C.POINTER(C.c_int32)]
    L.cfear_verify_sample_covariances.argtypes = [vp, C.POINTER(LoopGraphs), vp, C.c_int32, C.POINTER(LoopVerifyParams), vp]
    L.cfear_cov_fit_records.argtypes = [vp, vp, vp, C.c_int32, C.POINTER(CovSamplingParams), vp, vp]
    L.cfear_covariance_by_sampling_candidates.argtypes = [vp, vp, vp, C.c_int32, C.POINTER(RegParams), vp, C.POINTER(CovSamplingParams), vp, vp]
    L.cfear_verify_by_odometry.argtypes = [vp, C.c_int32, C.c_double, C.c_int32, C.POINTER(C.c_double)]
    L.cfear_get_cost.argtypes = [vp, C.POINTER(vp), C.c_int32, C.POINTER(C.c_double), C.POINTER(RegParams),
                                 C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_int32,
                                 C.POINTER(C.c_int32), C.POINTER(C.c_double)]
    L.cfear_cost_prepare.argtypes = [vp, C.POINTER(vp), C.c_int32, C.POINTER(C.c_double),
                                     C.POINTER(RegParams), C.c_int32, C.POINTER(vp)]
    L.cfear_cost_num_blocks.argtypes = [vp]
    L.cfear_cost_num_residuals.argtypes = [vp]
    L.cfear_cost_get_blocks.argtypes = [vp, vp, vp]
    L.cfear_cost_evaluate.argtypes = [vp, C.POINTER(C.c_double), vp, vp]
    L.cfear_cost_normal_eq.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_double),
                                       C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.cfear_cost_destroy.argtypes = [vp]
    L.cfear_odometry_params_default.argtypes = [C.POINTER(OdometryParams)]
    L.cfear_odometry_params_default.restype = None
    L.cfear_odometry_process_clouds.argtypes = [vp, C.POINTER(ScCloud), C.POINTER(ScCloud), vp]
    L.cfear_odometry_get_scan.argtypes = [vp, C.c_int32, C.POINTER(vp)]
    L.cfear_odometry_get_cloud.argtypes = [vp, C.c_int32, vp, C.c_int32, C.POINTER(C.c_int32)]
    L.cfear_odometry_get_peaks.argtypes = [vp, C.c_int32, vp, C.c_int32, C.POINTER(C.c_int32)]
    L.cfear_odometry_params_preset.argtypes = [C.POINTER(OdometryParams), C.c_int32, C.c_int32]
    L.cfear_odometry_create.argtypes = [vp, C.c_int32, C.POINTER(PolarDesc), C.POINTER(OdometryParams),
                                        C.POINTER(vp)]
    L.cfear_odometry_process.argtypes = [vp, vp, vp]
    L.cfear_odometry_process_prefetch.argtypes = [vp, vp, vp, vp]
    L.cfear_odometry_process_offsets.argtypes = [vp, vp, vp, vp, vp]
    L.cfear_odometry_discard_prefetch.argtypes = [vp]
    L.cfear_filter_kstrongest_legacy.argtypes = [vp, vp, C.POINTER(PolarDesc), C.c_int32, C.c_double, C.c_double, C.c_double, vp, vp,
                                                 C.c_int32]
    L.cfear_filter_kstrongest_rowkeys.argtypes = [vp, vp, C.POINTER(PolarDesc), C.POINTER(KStrongParams), C.c_int32, vp, vp]
    L.cfear_pgo_params_default.argtypes = [C.POINTER(PgoParams)]
    L.cfear_pgo_params_default.restype = None
    L.cfear_pgo_solve.argtypes = [vp, vp, C.c_int32, vp, C.c_int32, C.POINTER(PgoParams), C.POINTER(PgoSummary)]
    L.cfear_pgo_solve_batch.argtypes = [vp, vp, vp, vp, C.c_int64, vp, vp, C.c_int64, C.c_int32, C.POINTER(PgoParams), vp,
                                        C.POINTER(C.c_int32)]
    L.cfear_shard_range.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    L.cfear_gather_records.argtypes = [vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, vp, vp, vp]
    L.cfear_graph_save.argtypes = [C.c_char_p, C.POINTER(GraphNode), C.c_int32]
    L.cfear_graph_load.argtypes = [C.c_char_p, C.POINTER(vp)]
    L.cfear_graph_size.argtypes = [vp]
    L.cfear_graph_node_at.argtypes = [vp, C.c_int32, C.POINTER(GraphNode)]
    L.cfear_graph_destroy.argtypes = [vp]
    L.cfear_pose3d_from_xyt.argtypes = [C.POINTER(C.c_double), C.POINTER(Pose3d)]
    L.cfear_pose3d_from_xyt.restype = None
    L.cfear_pose3d_to_xyt.argtypes = [C.POINTER(Pose3d), C.POINTER(C.c_double)]
    L.cfear_pose3d_to_xyt.restype = None
    L.cfear_odometry_get_constraint.argtypes = [vp, C.c_int32, C.POINTER(GraphConstraint)]
    L.cfear_keyframe_based_fuse.argtypes = [C.POINTER(C.c_double), C.c_int32, C.c_double, C.c_double]
    L.cfear_acc_vel_sanity_check.argtypes = [C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.cfear_odometry_get_covariance.argtypes = [vp, vp, vp]
    L.cfear_kstrong_rowkeys_derive.argtypes = [vp, vp, vp, vp, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.POINTER(RowkeysClass),
                                               C.c_int32, vp, vp]
    L.cfear_odometry_grid_plan.argtypes = [C.POINTER(PolarDesc), C.POINTER(OdometryParams), C.c_int32, vp, vp, C.c_int32, vp,
                                           C.POINTER(GridTotals), C.c_char_p, C.c_int32]
    L.cfear_odometry_grid_create.argtypes = [vp, C.POINTER(PolarDesc), C.POINTER(OdometryParams), C.c_int32, vp, vp, C.c_int32,
                                             C.POINTER(vp)]
    L.cfear_odometry_grid_process.argtypes = [vp, vp, vp]
    L.cfear_odometry_grid_destroy.argtypes = [vp]
    L.cfear_odometry_destroy.argtypes = [vp]
    L.cfear_rccl_unique_id.argtypes = [vp]
    L.cfear_rccl_comm_init.argtypes = [vp, vp, C.c_int32, C.c_int32, C.POINTER(RcclComm)]
    L.cfear_rccl_comm_destroy.argtypes = [C.POINTER(RcclComm)]
    L.cfear_candidate_pipe_create.argtypes = [vp, vp, C.c_int32, C.c_int32, C.c_int32, C.POINTER(RcclComm), C.c_int32, C.c_int32,
                                              C.POINTER(vp)]
    L.cfear_candidate_pipe_submit.argtypes = [vp, vp, C.c_int32, C.POINTER(RegParams), C.POINTER(C.c_int64)]
    L.cfear_candidate_pipe_collect.argtypes = [vp, C.c_int64, vp]
    L.cfear_candidate_pipe_destroy.argtypes = [vp]
    L.cfear_candidate_pipe_stats.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_int32)]
    L.cfear_eval_params_default.argtypes = [C.POINTER(EvalParams)]
    L.cfear_eval_params_default.restype = None
    L.cfear_eval_trajectories.argtypes = [vp, vp, vp, vp, vp, C.c_int32, C.POINTER(EvalParams), vp, vp, C.c_int64,
                                          C.POINTER(C.c_int64)]
    L.cfear_eval_check.argtypes = [C.POINTER(EvalParams), vp, vp, C.c_int32]
    L.cfear_kitti_read.argtypes = [C.c_char_p, vp, C.c_int64, C.POINTER(C.c_int64)]
    L.cfear_kitti_write.argtypes = [C.c_char_p, vp, C.c_int64]
    L.cfear_kitti_from_xyt.argtypes = [vp, C.c_int64, C.c_int64, vp]
    L.cfear_sync_trajectories.argtypes = [vp, C.c_int32, vp, vp, vp, vp, vp, vp, vp, vp, C.c_int32, vp, vp, vp, vp, vp]
    L.cfear_tum_write.argtypes = [C.c_char_p, vp, vp, C.c_int64]
    L.cfear_cov_write.argtypes = [C.c_char_p, vp, vp, C.c_int64]
    L.cfear_logreg_params_default.argtypes = [C.POINTER(LogregParams)]
    L.cfear_logreg_params_default.restype = None
    L.cfear_logreg_fit_batch.argtypes = [vp, C.POINTER(LogregJob), C.c_int32, C.POINTER(LogregParams), vp]
    L.cfear_closure_params_default.argtypes = [C.POINTER(ClosureParams), C.c_int32]
    L.cfear_closure_params_default.restype = None
    L.cfear_closure_candidates_batch.argtypes = [vp, vp, vp, vp, vp, C.c_int64, C.c_int32, C.POINTER(ClosureParams), vp,
                                                 C.POINTER(C.c_int32)]
    L.cfear_loop_stats_params_default.argtypes = [C.POINTER(LoopStatsParams)]
    L.cfear_loop_stats_params_default.restype = None
    L.cfear_loop_stats_batch.argtypes = [vp, vp, vp, vp, C.c_int64, C.c_int32, vp, C.c_int64, C.POINTER(LoopStatsParams), vp,
                                         C.POINTER(C.c_int64)]
    L.cfear_loop_curves_params_default.argtypes = [C.POINTER(LoopCurvesParams)]
    L.cfear_loop_curves_params_default.restype = None
    L.cfear_loop_curves_batch.argtypes = [vp, vp, vp, vp, vp, C.c_int64, C.c_int32, C.POINTER(LoopCurvesParams), vp, vp, vp, vp, vp, vp,
                                          vp, C.POINTER(C.c_int32)]
    L.cfear_graph_align_batch.argtypes = [vp, vp, vp, vp, vp, C.c_int64, C.c_int32, vp]
    L.cfear_graph_map_batch.argtypes = [vp, vp, vp, vp, vp, C.c_int64, C.c_int32, vp, vp, C.c_int64, C.POINTER(GraphMapParams), vp,
                                        C.c_int64, vp, C.c_int64, vp]
    L.cfear_graph_string_write.argtypes = [C.c_char_p, vp, vp, C.c_int64]
    L.cfear_graph_output_write.argtypes = [C.c_char_p, C.c_char_p, vp, vp, vp, C.c_int64]
    _LIB = L
    return L
