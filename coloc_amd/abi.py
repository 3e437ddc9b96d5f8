"""ctypes binding of include/coloc_hip.h.  Thin: every method is one C-ABI call.

No fallback of any kind: if libcoloc_hip.so is missing or a call fails, CLCError is raised.
"""
import ctypes as C
import os

import numpy as np

_PKG = os.path.dirname(os.path.abspath(__file__))

KP_DTYPE = np.dtype(
    {"names": ["x", "y", "score", "angle", "scale"],
     "formats": ["<i4", "<i4", "u1", "<f4", "u1"],
     "offsets": [0, 4, 8, 12, 16], "itemsize": 20})   # clc_keypoint == reference Keypoint.h:155-163

CLC_OK, CLC_ERR_BAD_ARG, CLC_ERR_CAPACITY, CLC_ERR_HIP, CLC_ERR_NO_DEVICE, CLC_ERR_STATE = range(6)


class CLCError(RuntimeError):
    def __init__(self, status, msg):
        super().__init__("coloc_hip status %d: %s" % (status, msg))
        self.status = status


class DetectorOptions(C.Structure):   # coloc::DetectorOptions, colocData.hpp:29-36
    _fields_ = [("scale_factor", C.c_float), ("scale_levels", C.c_uint8), ("width", C.c_uint32),
                ("height", C.c_uint32), ("maxkp", C.c_uint32), ("thresh", C.c_uint8)]


class MatcherOptions(C.Structure):    # coloc::MatcherOptions, colocData.hpp:38-42
    _fields_ = [("distRatio", C.c_float), ("thresh", C.c_int), ("maxkp", C.c_uint32)]


class McShare(C.Structure):           # clc_mc_share
    _fields_ = [("first", C.c_int32), ("second", C.c_int32), ("q_begin", C.c_uint32), ("nq", C.c_uint32), ("out_offset", C.c_uint32)]


class MatchJob(C.Structure):          # clc_match_job
    _fields_ = [("q_offset", C.c_uint32), ("nq", C.c_uint32), ("t_offset", C.c_uint32), ("nt", C.c_uint32),
                ("out_offset", C.c_uint32), ("threshold", C.c_uint32)]


class PoseJob(C.Structure):
    """clc_pose_job (include/coloc_hip.h)"""
    _fields_ = [("X", C.c_void_p), ("x", C.c_void_p), ("K", C.c_void_p), ("n", C.c_int), ("max_iteration", C.c_int), ("seed", C.c_uint64),
                ("precision", C.c_double), ("refine", C.c_int), ("huber_a", C.c_double),
                ("Rt", C.c_void_p), ("cov", C.c_void_p), ("inlier_mask", C.c_void_p), ("inliers", C.c_void_p),
                ("n_inliers", C.c_int), ("iterations", C.c_int), ("status", C.c_int), ("error_max", C.c_double), ("rmse", C.c_double)]


class CameraK3(C.Structure):
    """clc_camera_k3 (include/coloc_hip.h): Pinhole_Intrinsic_Radial_K3"""
    _fields_ = [("focal", C.c_double), ("ppx", C.c_double), ("ppy", C.c_double), ("k1", C.c_double), ("k2", C.c_double), ("k3", C.c_double)]


class TrackJob(C.Structure):
    """clc_track_job (include/coloc_hip.h)"""
    _fields_ = [("d_match", C.c_void_p), ("nq", C.c_int), ("d_count", C.c_void_p), ("d_kps", C.c_void_p), ("d_feat", C.c_void_p),
                ("feat_stride", C.c_int), ("cam", CameraK3), ("after_stream", C.c_void_p), ("max_iteration", C.c_int), ("seed", C.c_uint64),
                ("precision", C.c_double), ("refine", C.c_int), ("huber_a", C.c_double),
                ("Rt", C.c_void_p), ("cov", C.c_void_p), ("track_query", C.c_void_p), ("track_map", C.c_void_p), ("inliers", C.c_void_p),
                ("inlier_mask", C.c_void_p), ("n_tracks", C.c_int), ("n_inliers", C.c_int), ("iterations", C.c_int), ("status", C.c_int),
                ("error_max", C.c_double), ("rmse", C.c_double)]


class TrackPriorJob(C.Structure):
    """clc_track_prior_job (include/coloc_hip.h)"""
    _fields_ = [("d_match", C.c_void_p), ("nq", C.c_int), ("d_count", C.c_void_p), ("d_kps", C.c_void_p), ("d_feat", C.c_void_p),
                ("feat_stride", C.c_int), ("cam", CameraK3), ("after_stream", C.c_void_p),
                ("Rt_prior", C.c_double * 12), ("gate", C.c_double), ("huber_a", C.c_double), ("rounds", C.c_int), ("max_iter", C.c_int),
                ("min_inliers", C.c_int),
                ("Rt", C.c_void_p), ("cov", C.c_void_p), ("track_query", C.c_void_p), ("track_map", C.c_void_p), ("inlier_mask", C.c_void_p),
                ("n_tracks", C.c_int), ("n_inliers", C.c_int), ("iterations", C.c_int), ("rounds_run", C.c_int), ("converged", C.c_int),
                ("result", C.c_int), ("status", C.c_int), ("rmse", C.c_double)]


class PairJob(C.Structure):
    """clc_pair_job (include/coloc_hip.h)"""
    _fields_ = [("d_match", C.c_void_p), ("nq", C.c_int), ("nt", C.c_int), ("d_count_a", C.c_void_p), ("d_count_b", C.c_void_p),
                ("d_kps_a", C.c_void_p), ("d_feat_a", C.c_void_p), ("feat_stride_a", C.c_int),
                ("d_kps_b", C.c_void_p), ("d_feat_b", C.c_void_p), ("feat_stride_b", C.c_int),
                ("cam_a", CameraK3), ("cam_b", CameraK3), ("after_stream", C.c_void_p),
                ("img_w", C.c_int), ("img_h", C.c_int), ("max_iteration", C.c_int), ("seed", C.c_uint64), ("precision", C.c_double),
                ("M", C.c_void_p), ("F", C.c_void_p), ("pair_q", C.c_void_p), ("pair_t", C.c_void_p), ("x1", C.c_void_p), ("x2", C.c_void_p),
                ("inliers", C.c_void_p), ("inlier_mask", C.c_void_p),
                ("n_pairs", C.c_int), ("n_inliers", C.c_int), ("iterations", C.c_int), ("status", C.c_int),
                ("error_max", C.c_double), ("min_nfa", C.c_double)]


class GuidedJob(C.Structure):
    """clc_guided_job (include/coloc_hip.h)"""
    _fields_ = [("d_q", C.c_void_p), ("nq", C.c_int), ("d_t", C.c_void_p), ("nt", C.c_int), ("d_count_a", C.c_void_p), ("d_count_b", C.c_void_p),
                ("d_kps_a", C.c_void_p), ("d_feat_a", C.c_void_p), ("feat_stride_a", C.c_int),
                ("d_kps_b", C.c_void_p), ("d_feat_b", C.c_void_p), ("feat_stride_b", C.c_int),
                ("cam_a", CameraK3), ("cam_b", CameraK3), ("F", C.c_double * 9), ("band", C.c_float), ("threshold", C.c_int),
                ("d_match", C.c_void_p), ("d_best", C.c_void_p), ("d_second", C.c_void_p), ("d_line", C.c_void_p), ("d_tpos", C.c_void_p)]


class MapGuidedJob(C.Structure):
    """clc_map_guided_job (include/coloc_hip.h)"""
    _fields_ = [("d_q", C.c_void_p), ("nq", C.c_int), ("d_count", C.c_void_p), ("d_kps", C.c_void_p), ("d_feat", C.c_void_p),
                ("feat_stride", C.c_int), ("cam", CameraK3), ("Rt", C.c_double * 12), ("radius", C.c_float), ("threshold", C.c_int),
                ("d_match", C.c_void_p), ("d_best", C.c_void_p), ("d_second", C.c_void_p), ("d_qpos", C.c_void_p), ("d_proj", C.c_void_p)]


class UniqueJob(C.Structure):
    """clc_unique_job (include/coloc_hip.h)"""
    _fields_ = [("d_match", C.c_void_p), ("d_best", C.c_void_p), ("nq", C.c_int), ("nt", C.c_int), ("d_owner", C.c_void_p)]


class ExtendView(C.Structure):
    """clc_extend_view (include/coloc_hip.h)"""
    _fields_ = [("d_desc", C.c_void_p), ("n", C.c_int), ("d_count", C.c_void_p), ("d_kps", C.c_void_p), ("d_feat", C.c_void_p),
                ("feat_stride", C.c_int), ("cam", CameraK3), ("Rt", C.c_double * 12), ("d_track", C.c_void_p)]


class MapExtend(C.Structure):
    """clc_map_extend (include/coloc_hip.h)"""
    _fields_ = [("a", ExtendView), ("b", ExtendView), ("band", C.c_float), ("threshold", C.c_int), ("max_distance", C.c_int),
                ("update_tracks", C.c_int), ("after_stream", C.c_void_p), ("d_new_q", C.c_void_p), ("d_new_t", C.c_void_p),
                ("new_q", C.c_void_p), ("new_t", C.c_void_p), ("X", C.c_void_p), ("F", C.c_double * 9),
                ("map_n_before", C.c_int), ("n_guided", C.c_int), ("n_added", C.c_int), ("n_dropped", C.c_int), ("status", C.c_int)]


MAX_BATCH, MAX_TRACK_PAIRS = 8, 28          # CLC_MAX_BATCH, CLC_MAX_TRACK_PAIRS


class ObserveView(C.Structure):
    """clc_observe_view (include/coloc_hip.h)"""
    _fields_ = [("n", C.c_int), ("d_count", C.c_void_p), ("d_kps", C.c_void_p), ("d_feat", C.c_void_p), ("feat_stride", C.c_int),
                ("cam", CameraK3), ("Rt", C.c_double * 12), ("d_track", C.c_void_p), ("d_counts", C.c_void_p)]


class MapObserve(C.Structure):
    """clc_map_observe (include/coloc_hip.h)"""
    _fields_ = [("view", ObserveView), ("width", C.c_int), ("height", C.c_int), ("gate", C.c_float), ("margin", C.c_float),
                ("after_stream", C.c_void_p), ("epoch", C.c_uint32), ("map_n", C.c_int), ("status", C.c_int)]


class MapCull(C.Structure):
    """clc_map_cull (include/coloc_hip.h)"""
    _fields_ = [("min_visible", C.c_int), ("num", C.c_int), ("den", C.c_int), ("max_idle", C.c_uint32), ("d_flagged", C.c_void_p),
                ("d_track", C.c_void_p * MAX_BATCH), ("track_n", C.c_int * MAX_BATCH), ("n_lists", C.c_int), ("after_stream", C.c_void_p),
                ("d_remap", C.c_void_p), ("h_remap", C.c_void_p),
                ("map_n_before", C.c_int), ("n_kept", C.c_int), ("n_dropped", C.c_int), ("n_flagged", C.c_int), ("n_ratio", C.c_int),
                ("n_idle", C.c_int), ("status", C.c_int)]


# the customary cull rule (clc_map_cull_rule_default): UNTUNED
CULL_RULE_DEFAULT = dict(min_visible=8, num=1, den=4, max_idle=0)


class TracksPair(C.Structure):
    """clc_tracks_pair (include/coloc_hip.h)"""
    _fields_ = [("cam_a", C.c_int32), ("cam_b", C.c_int32), ("d_q", C.c_void_p), ("d_t", C.c_void_p), ("n", C.c_int), ("d_n", C.c_void_p),
                ("d_index", C.c_void_p), ("n_list", C.c_int)]


class TracksJob(C.Structure):
    """clc_tracks_job (include/coloc_hip.h)"""
    _fields_ = [("n_cams", C.c_int), ("rows", C.c_int * MAX_BATCH), ("n_pairs", C.c_int), ("pairs", C.POINTER(TracksPair))]


class MapCamera(C.Structure):
    """clc_map_camera (include/coloc_hip.h)"""
    _fields_ = [("d_kps", C.c_void_p), ("d_feat", C.c_void_p), ("feat_stride", C.c_int), ("cam", CameraK3), ("d_desc", C.c_void_p)]


class MapJob(C.Structure):
    """clc_map_job (include/coloc_hip.h)"""
    _fields_ = [("tracks", TracksJob), ("cams", MapCamera * MAX_BATCH), ("seed_pair", C.c_int), ("Rt_seed_a", C.c_double * 12),
                ("Rt_seed_b", C.c_double * 12), ("after_stream", C.c_void_p), ("origin_R", C.c_double * 9), ("origin_C", C.c_double * 3),
                ("scale", C.c_double), ("track_feat", C.c_void_p), ("map_track", C.c_void_p), ("map_row", C.c_void_p), ("X", C.c_void_p),
                ("n_tracks", C.c_int), ("map_n", C.c_int), ("status", C.c_int), ("entered", C.c_int * MAX_TRACK_PAIRS)]


class MapAlign(C.Structure):
    """clc_map_align (include/coloc_hip.h)"""
    _fields_ = [("d_desc", C.c_void_p), ("d_rows", C.c_void_p), ("d_X", C.c_void_p), ("n_new", C.c_int), ("threshold", C.c_int),
                ("install", C.c_int), ("after_stream", C.c_void_p), ("match", C.c_void_p), ("X", C.c_void_p),
                ("n_old", C.c_int), ("n_common", C.c_int), ("n_terms", C.c_int), ("status", C.c_int), ("scale", C.c_double)]


MAP_ALIGN_OK, MAP_ALIGN_NO_SCALE = 0, 1


class MapAlignSim(C.Structure):
    """clc_map_align_sim (include/coloc_hip.h)"""
    _fields_ = [("d_desc", C.c_void_p), ("d_rows", C.c_void_p), ("d_X", C.c_void_p), ("n_new", C.c_int), ("threshold", C.c_int),
                ("install", C.c_int), ("after_stream", C.c_void_p), ("apply", C.c_int), ("max_iteration", C.c_int), ("seed", C.c_uint64),
                ("precision", C.c_double), ("match", C.c_void_p), ("X", C.c_void_p), ("inlier", C.c_void_p),
                ("n_old", C.c_int), ("n_common", C.c_int), ("n_inliers", C.c_int), ("iterations", C.c_int), ("refit", C.c_int),
                ("status", C.c_int), ("s", C.c_double), ("R", C.c_double * 9), ("t", C.c_double * 3), ("error_max", C.c_double),
                ("min_nfa", C.c_double)]


MAP_SIM_OK, MAP_SIM_NO_MODEL = 0, 1
SIM_APPLY_SCALE, SIM_APPLY_FULL = 0, 1


class MapGrow(C.Structure):
    """clc_map_grow (include/coloc_hip.h)"""
    _fields_ = [("max_iteration", C.c_int), ("seed", C.c_uint64), ("precision", C.c_double), ("resected", C.c_int * MAX_BATCH),
                ("status", C.c_int * MAX_BATCH), ("n_corr", C.c_int * MAX_BATCH), ("n_inliers", C.c_int * MAX_BATCH),
                ("error_max", C.c_double * MAX_BATCH), ("Rt", (C.c_double * 12) * MAX_BATCH), ("n_seed_rows", C.c_int), ("n_added", C.c_int),
                ("map_cam", C.c_void_p), ("map_obs", C.c_void_p)]


GROW_OK, GROW_NO_TRACKS, GROW_NO_POSE, GROW_CAPACITY = 0, 1, 2, 3


class MapBa(C.Structure):
    """clc_map_ba (include/coloc_hip.h)"""
    _fields_ = [("max_iterations", C.c_int), ("huber_a", C.c_double), ("function_tolerance", C.c_double),
                ("status", C.c_int), ("iterations", C.c_int), ("n_cams", C.c_int), ("n_points", C.c_int), ("n_obs", C.c_int),
                ("cost_initial", C.c_double), ("cost_final", C.c_double), ("rmse", C.c_double)]


class BaJob(C.Structure):
    """clc_ba_job (include/coloc_hip.h)"""
    _fields_ = [("n_cams", C.c_int), ("cam_mask", C.c_uint32), ("cam", CameraK3 * MAX_BATCH), ("Rt", (C.c_double * 12) * MAX_BATCH),
                ("n_points", C.c_int), ("d_X", C.c_void_p), ("d_obs", C.c_void_p), ("d_x", C.c_void_p), ("after_stream", C.c_void_p),
                ("ba", MapBa)]


BA_OK, BA_MAX_ITERATIONS, BA_STALLED, BA_BAD_START, BA_EMPTY = 0, 1, 2, 3, 4

ABI_VERSION = 4          # CLC_ABI_VERSION of include/coloc_hip.h
DESC_CACHE_OFF, DESC_CACHE_VERIFY, DESC_CACHE_TRUST = 0, 1, 2

class DescHandle(C.Structure):
    """clc_desc_handle (include/coloc_hip.h): what a publication hands out"""
    _fields_ = [("host", C.c_void_p), ("generation", C.c_uint64), ("count", C.c_uint32), ("slot", C.c_uint32)]


class TwoViewJob(C.Structure):
    """clc_two_view_job (include/coloc_hip.h)"""
    _fields_ = [("x1", C.c_void_p), ("x2", C.c_void_p), ("K1", C.c_void_p), ("K2", C.c_void_p), ("n", C.c_int), ("img_w", C.c_int), ("img_h", C.c_int),
                ("max_iteration", C.c_int), ("seed", C.c_uint64), ("precision", C.c_double),
                ("E", C.c_void_p), ("F", C.c_void_p), ("inlier_mask", C.c_void_p), ("inliers", C.c_void_p),
                ("n_inliers", C.c_int), ("iterations", C.c_int), ("status", C.c_int), ("error_max", C.c_double), ("min_nfa", C.c_double)]


class InterPoseJob(C.Structure):
    """clc_inter_pose_job (include/coloc_hip.h)"""
    _fields_ = [("tv", TwoViewJob), ("map_index", C.c_void_p), ("map_X", C.c_void_p), ("map_n", C.c_int), ("Rt_source", C.c_void_p), ("huber_a", C.c_double),
                ("d_first_desc", C.c_void_p), ("first_feature", C.c_void_p), ("d_map_desc", C.c_void_p), ("match_threshold", C.c_int),
                ("Rt", C.c_double * 12), ("cov", C.c_double * 36), ("rmse", C.c_double), ("scale", C.c_double),
                ("n_front", C.c_int), ("n_common", C.c_int), ("n_refined", C.c_int), ("stage", C.c_int), ("n_map_matches", C.c_int)]


class InterDevJob(C.Structure):
    """clc_inter_dev_job (include/coloc_hip.h)"""
    _fields_ = [("pair", PairJob), ("Rt_source", C.c_void_p), ("huber_a", C.c_double), ("lower_is_b", C.c_int), ("d_first_desc", C.c_void_p),
                ("d_map_desc", C.c_void_p), ("d_map_match_a", C.c_void_p), ("match_threshold", C.c_int),
                ("Rt", C.c_double * 12), ("cov", C.c_double * 36), ("rmse", C.c_double), ("scale", C.c_double),
                ("n_front", C.c_int), ("n_common", C.c_int), ("n_refined", C.c_int), ("stage", C.c_int), ("n_map_matches", C.c_int)]


EXPORTS = [
    "clc_abi_version", "clc_status_string", "clc_ctx_create", "clc_ctx_destroy", "clc_last_error_string",
    "clc_sync", "clc_stream", "clc_pyramid_build", "clc_pyramid_build_dev", "clc_pyramid_level",
    "clc_pyramid_download", "clc_describe", "clc_describe_dev", "clc_keypoints_to_features",
    "clc_match_2nn", "clc_match_2nn_dev", "clc_match_jobs_dev", "clc_set_map", "clc_match_map",
    "clc_pnp_residuals", "clc_pnp_score", "clc_profile_enable", "clc_profile_reset", "clc_profile_read",
    "clc_kernel_name", "clc_detect", "clc_detect_dev", "clc_detect_buffers", "clc_describe_detected_dev",
    "clc_detect_and_describe", "clc_detect_batch_dev", "clc_desc_cache_publish", "clc_desc_cache_clear", "clc_desc_cache_stats", "clc_desc_cache_mode", "clc_desc_handle_live", "clc_detect_and_describe_view", "clc_detect_store_descriptors", "clc_describe_match_pair_dev", "clc_essential_acransac_batch", "clc_inter_pose_batch", "clc_pnp_localize_ac_batch", "clc_match_pairs", "clc_pnp_ransac", "clc_pnp_p3p", "clc_pnp_refine", "clc_pnp_localize", "clc_epipolar_residuals", "clc_epipolar_score", "clc_cov_intersection", "clc_essential_ransac",
    "clc_essential_fivepoint", "clc_describe_batch_dev", "clc_match_map_dev", "clc_k2nn_set_formulation",
    "clc_k2nn_queries_per_block", "clc_k2nn_plan_query", "clc_k2nn_device_info", "clc_pnp_acransac", "clc_pnp_localize_ac", "clc_essential_acransac", "clc_k2nn_clock_check", "clc_ctx_device", "clc_mc_plan", "clc_mc_unique_id",
    "clc_mc_create", "clc_mc_destroy", "clc_mc_last_error_string", "clc_mc_arena", "clc_mc_gather_dev", "clc_mc_match_dev", "clc_mc_virtual_put", "clc_mc_open_peers",
    "clc_mc_gather_enqueue_dev", "clc_mc_match_enqueue_dev", "clc_mc_counts", "clc_mc_set_overlap", "clc_mc_comm_info", "clc_match_jobs_counted_dev",
    "clc_two_view_acransac", "clc_two_view_acransac_batch", "clc_two_view_minimal",
    "clc_match_ratio_2nn", "clc_match_ratio_2nn_dev", "clc_match_ratio_pairs", "clc_match_map_ratio", "clc_match_map_ratio_dev",
    "clc_ratio_matches_to_pairs", "clc_detect_set_selection", "clc_detect_selection",
    "clc_set_map_points", "clc_track_build_dev", "clc_track_localize_dev", "clc_track_localize_batch_dev",
    "clc_pair_build_dev", "clc_pair_filter_dev", "clc_pair_filter_batch_dev",
    "clc_inter_pose_dev", "clc_inter_pose_batch_dev", "clc_inter_front_dev",
    "clc_tracks_build_dev", "clc_map_build_dev", "clc_map_init_batch_dev",
    "clc_map_align_dev", "clc_map_update_batch_dev",
    "clc_map_build_grow_dev", "clc_map_init_grow_batch_dev", "clc_map_update_grow_batch_dev", "clc_map_resect_build_dev",
    "clc_ba_dev", "clc_map_build_grow_ba_dev", "clc_map_init_grow_ba_batch_dev", "clc_map_update_grow_ba_batch_dev",
    "clc_match_guided_dev", "clc_match_guided_batch_dev",
    "clc_match_map_guided_dev", "clc_match_map_guided_batch_dev",
    "clc_match_map_binned_dev", "clc_match_map_binned_batch_dev", "clc_map_bin_build_dev", "clc_map_binned_plan",
    "clc_sim3_acransac", "clc_sim3_minimal", "clc_map_align_sim_dev", "clc_map_update_sim_batch_dev",
    "clc_track_prior_dev", "clc_track_prior_batch_dev", "clc_pnp_refine_prior",
    "clc_match_unique_dev", "clc_match_unique_batch_dev", "clc_match_2nn_unique_dev", "clc_match_map_unique_dev",
    "clc_match_map_binned_unique_dev", "clc_match_2nn_unique",
    "clc_map_extend_dev", "clc_map_extend_batch_dev", "clc_fundamental_from_poses", "clc_append_map_points",
    "clc_map_observe_dev", "clc_map_observe_batch_dev", "clc_map_cull_dev", "clc_map_cull_rule_default", "clc_map_stats_get",
    "clc_cull_map_points",
]
# clc_track_prior_job.result
TRACK_PRIOR_OK, TRACK_PRIOR_FEW = 0, 1
# clc_detect_set_selection: which keypoints a frame with more than maxkp keeps
SELECT_FIRST, SELECT_STRONGEST = 0, 1
# clc_map_binned_plan: what clc_match_map_binned_dev runs for a job
BIN_PLAN_SWEEP, BIN_PLAN_BINNED = 0, 1
KERNELS = ["pyramid_kernel", "clatch_kernel", "k2nn_sweep_kernel", "k2nn_merge_kernel", "pnp_residual_kernel",
           "pnp_score_kernel", "detect_kernels"]

_lib = None


def lib_path():
    return os.environ.get("COLOC_HIP_LIB", os.path.join(_PKG, "lib", "libcoloc_hip.so"))


def _share_torch_hip_runtime():
    """PyTorch wheels bundle their own libamdhip64.so / libhsa-runtime64.so.  Two HIP runtimes in one
    process cannot both own the GPU ("No HIP GPUs are available" in whichever initialises second), so
    when torch is installed its runtime is mapped first and libcoloc_hip.so's DT_NEEDED
    libamdhip64.so.7 resolves to it.  A pure C/C++ host simply uses the system ROCm runtime."""
    if os.environ.get("COLOC_HIP_SYSTEM_RUNTIME"):
        return
    import importlib.util
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.origin:
        return
    cand = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
    if os.path.exists(cand):
        try:
            C.CDLL(cand, mode=C.RTLD_GLOBAL)
        except OSError:
            pass


def load_library():
    """dlopen libcoloc_hip.so; raises (never falls back) when it is absent."""
    global _lib
    if _lib is not None:
        return _lib
    path = lib_path()
    if not os.path.exists(path):
        raise CLCError(-1, "%s not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                           "(hipcc --offload-arch=gfx950); there is no CPU fallback" % path)
    _share_torch_hip_runtime()
    lib = C.CDLL(path)
    # the version BEFORE any symbol an older library does not export is resolved (include/coloc_hip.h CLC_ABI_VERSION)
    got = lib.clc_abi_version() if hasattr(lib, "clc_abi_version") else 0
    if got != ABI_VERSION:
        raise CLCError(-1, "%s reports ABI version %d, this binding needs %d: rebuild it (python -c 'import __graft_entry__ as g; g.build()')"
                       % (path, got, ABI_VERSION))
    lib.clc_status_string.restype = C.c_char_p
    lib.clc_last_error_string.restype = C.c_char_p
    lib.clc_last_error_string.argtypes = [C.c_void_p]
    lib.clc_stream.restype = C.c_void_p
    lib.clc_stream.argtypes = [C.c_void_p]
    lib.clc_ctx_create.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p)]
    lib.clc_ctx_destroy.argtypes = [C.c_void_p]
    lib.clc_sync.argtypes = [C.c_void_p]
    vp, ci, u32, sz = C.c_void_p, C.c_int, C.c_uint32, C.c_size_t
    lib.clc_pyramid_build.argtypes = [vp, vp, u32, u32]
    lib.clc_pyramid_build_dev.argtypes = [vp, vp, u32, u32, sz, vp]
    lib.clc_pyramid_level.argtypes = [vp, ci, C.POINTER(u32), C.POINTER(u32), C.POINTER(sz), C.POINTER(vp)]
    lib.clc_pyramid_download.argtypes = [vp, ci, vp]
    lib.clc_describe.argtypes = [vp, vp, ci, vp]
    lib.clc_describe_dev.argtypes = [vp, vp, ci, vp, vp]
    lib.clc_describe_batch_dev.argtypes = [vp, ci, vp, C.c_uint32, C.c_uint32, C.c_size_t, vp, vp, vp, vp]
    lib.clc_detect_batch_dev.argtypes = [vp, ci, vp, C.c_uint32, C.c_uint32, C.c_size_t, vp, vp, vp, vp]
    lib.clc_desc_cache_publish.argtypes = [vp, vp, vp, ci, vp]
    lib.clc_desc_handle_live.argtypes = [vp]
    lib.clc_detect_and_describe_view.argtypes = [vp, vp, u32, u32, C.POINTER(vp), C.POINTER(vp), C.POINTER(ci), C.POINTER(ci)]
    lib.clc_detect_store_descriptors.argtypes = [vp, vp, ci, vp]
    lib.clc_desc_cache_clear.argtypes = []
    lib.clc_desc_cache_stats.argtypes = [vp, vp]
    lib.clc_desc_cache_mode.argtypes = [vp, ci]
    lib.clc_essential_acransac_batch.argtypes = [vp, vp, ci]
    lib.clc_inter_pose_batch.argtypes = [vp, vp, ci]
    lib.clc_describe_match_pair_dev.argtypes = [vp, vp, C.c_uint32, C.c_uint32, C.c_size_t, vp, vp, vp, ci, vp, vp]
    lib.clc_pnp_localize_ac_batch.argtypes = [vp, vp, ci]
    lib.clc_keypoints_to_features.argtypes = [vp, ci, vp]
    lib.clc_match_2nn.argtypes = [vp, vp, ci, vp, ci, ci, vp, vp, vp]
    lib.clc_match_2nn_dev.argtypes = [vp, vp, ci, vp, ci, ci, vp, vp]
    lib.clc_match_jobs_dev.argtypes = [vp, vp, vp, ci, vp, vp]
    lib.clc_match_pairs.argtypes = [vp, vp, vp, ci, vp, ci, ci, vp]
    lib.clc_set_map.argtypes = [vp, vp, ci]
    lib.clc_match_map_dev.argtypes = [vp, vp, ci, ci, vp, vp]
    lib.clc_match_map.argtypes = [vp, vp, ci, ci, vp]
    cf = C.c_float
    lib.clc_match_ratio_2nn.argtypes = [vp, vp, ci, vp, ci, cf, vp, vp, vp]
    lib.clc_match_ratio_2nn_dev.argtypes = [vp, vp, ci, vp, ci, cf, vp, vp]
    lib.clc_match_ratio_pairs.argtypes = [vp, vp, vp, ci, vp, vp, ci, cf, vp, vp]
    lib.clc_match_map_ratio.argtypes = [vp, vp, ci, vp, vp, cf, vp, vp]
    lib.clc_match_map_ratio_dev.argtypes = [vp, vp, ci, cf, vp, vp]
    lib.clc_ratio_matches_to_pairs.argtypes = [vp, ci, vp, vp, vp, vp]
    lib.clc_pnp_residuals.argtypes = [vp, vp, ci, vp, vp, ci, vp, vp]
    lib.clc_pnp_score.argtypes = [vp, vp, ci, vp, vp, ci, vp, C.c_double, vp, vp]
    lib.clc_detect.argtypes = [vp, vp, ci, C.POINTER(ci), C.POINTER(ci)]
    lib.clc_detect_dev.argtypes = [vp, vp]
    lib.clc_detect_set_selection.argtypes = [vp, ci]
    lib.clc_detect_selection.argtypes = [vp]
    lib.clc_detect_buffers.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)]
    lib.clc_describe_detected_dev.argtypes = [vp, vp, vp]
    lib.clc_detect_and_describe.argtypes = [vp, vp, u32, u32, vp, vp, ci, C.POINTER(ci), C.POINTER(ci)]
    lib.clc_pnp_ransac.argtypes = [vp, vp, vp, ci, vp, vp, ci, C.c_uint64, C.c_double, vp, vp, C.POINTER(ci), C.POINTER(C.c_double)]
    lib.clc_pnp_p3p.argtypes = [vp, vp, vp, ci, vp, vp, ci, vp]
    lib.clc_essential_ransac.argtypes = [vp, vp, vp, ci, vp, vp, vp, ci, C.c_uint64, C.c_double, vp, vp, vp, C.POINTER(ci)]
    lib.clc_essential_fivepoint.argtypes = [vp, vp, vp, ci, vp, vp, vp, ci, vp]
    lib.clc_epipolar_residuals.argtypes = [vp, vp, ci, vp, vp, ci, vp]
    lib.clc_epipolar_score.argtypes = [vp, vp, ci, vp, vp, ci, C.c_double, vp, vp]
    lib.clc_pnp_localize.argtypes = [vp, vp, vp, ci, vp, vp, ci, C.c_uint64, C.c_double, C.c_double, vp, vp, vp, C.POINTER(ci),
                                     C.POINTER(C.c_double)]
    lib.clc_pnp_refine.argtypes = [vp, vp, vp, ci, vp, vp, vp, C.c_double, ci, vp, vp, C.POINTER(C.c_double), C.POINTER(ci)]
    lib.clc_profile_enable.argtypes = [vp, ci]
    lib.clc_profile_reset.argtypes = [vp]
    lib.clc_profile_read.argtypes = [vp, ci, C.POINTER(C.c_double), C.POINTER(ci)]
    lib.clc_kernel_name.restype = C.c_char_p
    dp, ip = C.POINTER(C.c_double), C.POINTER(ci)
    lib.clc_pnp_acransac.argtypes = [vp, vp, vp, ci, vp, ci, C.c_uint64, C.c_double, vp, vp, vp, ip, dp, dp, ip]
    lib.clc_pnp_localize_ac.argtypes = [vp, vp, vp, ci, vp, ci, C.c_uint64, C.c_double, C.c_double, vp, vp, vp, vp, ip, dp, dp]
    lib.clc_essential_acransac.argtypes = [vp, vp, vp, ci, vp, vp, ci, ci, ci, C.c_uint64, C.c_double, vp, vp, vp, vp, ip, dp, dp, ip]
    lib.clc_two_view_acransac.argtypes = [vp, ci, vp, vp, ci, vp, vp, ci, ci, ci, C.c_uint64, C.c_double, vp, vp, vp, vp, ip, dp, dp, ip]
    lib.clc_two_view_acransac_batch.argtypes = [vp, ci, vp, ci]
    lib.clc_two_view_minimal.argtypes = [vp, ci, vp, vp, ci, ci, ci, vp, ci, vp]
    lib.clc_sim3_acransac.argtypes = [vp, vp, vp, ci, ci, C.c_uint64, C.c_double, dp, vp, vp, vp, vp, vp, ip, dp, dp, ip, ip, ip]
    lib.clc_sim3_minimal.argtypes = [vp, vp, vp, ci, vp, ci, vp]
    lib.clc_map_align_sim_dev.argtypes = [vp, vp]
    lib.clc_map_update_sim_batch_dev.argtypes = [vp, vp, ci, vp, vp, vp, vp]
    lib.clc_mc_plan.argtypes = [vp, ci, ci, ci, ci, vp, ci, ip]
    lib.clc_mc_unique_id.argtypes = [vp]
    lib.clc_mc_create.argtypes = [vp, vp, ci, ci, ci, C.POINTER(vp)]
    lib.clc_mc_destroy.argtypes = [vp]
    lib.clc_mc_last_error_string.argtypes = [vp]
    lib.clc_mc_last_error_string.restype = C.c_char_p
    lib.clc_mc_arena.argtypes = [vp, C.POINTER(vp), ip, ip]
    lib.clc_mc_gather_dev.argtypes = [vp, vp, ci, ci, vp, vp]
    lib.clc_mc_virtual_put.argtypes = [vp, ci, vp, ci, vp]
    lib.clc_mc_open_peers.argtypes = [vp, vp]
    lib.clc_mc_match_dev.argtypes = [vp, ci, vp, ci, vp, ci, ip, vp]
    lib.clc_mc_gather_enqueue_dev.argtypes = [vp, vp, ci, vp, ci, vp]
    lib.clc_mc_match_enqueue_dev.argtypes = [vp, ci, vp, ci, vp, ci, ip, vp]
    lib.clc_mc_counts.argtypes = [vp, vp, vp]
    lib.clc_mc_set_overlap.argtypes = [vp, ci]
    lib.clc_mc_comm_info.argtypes = [vp, ip, ip]
    lib.clc_match_jobs_counted_dev.argtypes = [vp, vp, vp, ci, vp, vp, vp, vp, vp]
    lib.clc_k2nn_clock_check.argtypes = [vp, vp, ci, vp, ci, vp, vp, dp, dp, dp, ip]
    lib.clc_k2nn_set_formulation.argtypes = [vp, ci]
    lib.clc_k2nn_queries_per_block.argtypes = [vp]
    lib.clc_k2nn_plan_query.argtypes = [vp, ci, ci, vp]
    lib.clc_k2nn_device_info.argtypes = [vp, vp, vp]
    lib.clc_set_map_points.argtypes = [vp, vp, ci]
    lib.clc_track_build_dev.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp]
    lib.clc_track_localize_dev.argtypes = [vp, vp]
    lib.clc_track_localize_batch_dev.argtypes = [vp, vp, ci]
    lib.clc_track_prior_dev.argtypes = [vp, vp]
    lib.clc_track_prior_batch_dev.argtypes = [vp, vp, ci]
    lib.clc_pnp_refine_prior.argtypes = [vp, vp, vp, ci, vp, vp, C.c_double, C.c_double, ci, ci, ci, vp, vp, vp] + [vp] * 6
    lib.clc_pair_build_dev.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp]
    lib.clc_pair_filter_dev.argtypes = [vp, ci, vp]
    lib.clc_pair_filter_batch_dev.argtypes = [vp, ci, vp, ci]
    lib.clc_inter_pose_dev.argtypes = [vp, vp]
    lib.clc_inter_pose_batch_dev.argtypes = [vp, vp, ci]
    lib.clc_inter_front_dev.argtypes = [vp, vp, vp, ci, vp, ci, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.clc_tracks_build_dev.argtypes = [vp, vp, vp, vp, vp]
    lib.clc_map_build_dev.argtypes = [vp, vp]
    lib.clc_map_init_batch_dev.argtypes = [vp, vp, ci, vp]
    lib.clc_map_align_dev.argtypes = [vp, vp]
    lib.clc_map_update_batch_dev.argtypes = [vp, vp, ci, vp, vp]
    lib.clc_map_build_grow_dev.argtypes = [vp, vp, vp]
    lib.clc_map_init_grow_batch_dev.argtypes = [vp, vp, ci, vp, vp]
    lib.clc_map_update_grow_batch_dev.argtypes = [vp, vp, ci, vp, vp, vp]
    lib.clc_map_resect_build_dev.argtypes = [vp, vp, ci, vp, vp, vp, vp, vp, vp]
    lib.clc_ba_dev.argtypes = [vp, vp]
    lib.clc_map_build_grow_ba_dev.argtypes = [vp, vp, vp, vp]
    lib.clc_map_init_grow_ba_batch_dev.argtypes = [vp, vp, ci, vp, vp, vp]
    lib.clc_map_update_grow_ba_batch_dev.argtypes = [vp, vp, ci, vp, vp, vp, vp]
    lib.clc_match_guided_dev.argtypes = [vp, vp, vp]
    lib.clc_match_guided_batch_dev.argtypes = [vp, vp, ci, vp]
    lib.clc_match_map_guided_dev.argtypes = [vp, vp, vp]
    lib.clc_match_map_guided_batch_dev.argtypes = [vp, vp, ci, vp]
    lib.clc_match_map_binned_dev.argtypes = [vp, vp, vp]
    lib.clc_match_map_binned_batch_dev.argtypes = [vp, vp, ci, vp]
    lib.clc_map_bin_build_dev.argtypes = [vp, vp, vp, vp, vp]
    lib.clc_map_binned_plan.argtypes = [vp, vp, C.c_float, vp, vp]
    lib.clc_match_unique_dev.argtypes = [vp, vp, vp]
    lib.clc_match_unique_batch_dev.argtypes = [vp, vp, ci, vp]
    lib.clc_match_2nn_unique_dev.argtypes = [vp, vp, ci, vp, ci, ci, vp, vp, vp]
    lib.clc_match_map_unique_dev.argtypes = [vp, vp, ci, ci, vp, vp, vp]
    lib.clc_match_map_binned_unique_dev.argtypes = [vp, vp, vp, vp]
    lib.clc_match_2nn_unique.argtypes = [vp, vp, ci, vp, ci, ci, vp, vp]
    lib.clc_map_extend_dev.argtypes = [vp, vp]
    lib.clc_map_extend_batch_dev.argtypes = [vp, vp, ci]
    lib.clc_fundamental_from_poses.argtypes = [vp, vp, vp, vp, vp]
    lib.clc_append_map_points.argtypes = [vp, vp, ci]
    lib.clc_map_observe_dev.argtypes = [vp, vp]
    lib.clc_map_observe_batch_dev.argtypes = [vp, vp, ci]
    lib.clc_map_cull_dev.argtypes = [vp, vp]
    lib.clc_map_cull_rule_default.argtypes = [vp]
    lib.clc_map_stats_get.argtypes = [vp, vp, vp, vp, vp, vp]
    lib.clc_cull_map_points.argtypes = [vp, vp, ci]
    _lib = lib
    return lib


def _p(a):
    # (a.ctypes.data_as(c_void_p) builds two ctypes objects per call, ~2.3 us; a pose solve passes seven pointers.  The caller keeps
    # the array alive across the call.)
    return None if a is None else C.c_void_p(a.ctypes.data)


def cov_intersection(CA, CB, ca, cb):
    """Host-side covariance intersection: returns (omega, fused 3x3 covariance, fused position)."""
    lib = load_library()
    CA = np.ascontiguousarray(CA, dtype=np.float64).reshape(9); CB = np.ascontiguousarray(CB, dtype=np.float64).reshape(9)
    ca = np.ascontiguousarray(ca, dtype=np.float64).reshape(3); cb = np.ascontiguousarray(cb, dtype=np.float64).reshape(3)
    om = C.c_double(); cov = np.zeros(9); pos = np.zeros(3)
    lib.clc_cov_intersection.argtypes = [C.c_void_p] * 4 + [C.POINTER(C.c_double), C.c_void_p, C.c_void_p]
    rc = lib.clc_cov_intersection(_p(CA), _p(CB), _p(ca), _p(cb), C.byref(om), _p(cov), _p(pos))
    if rc != CLC_OK:
        raise CLCError(rc, lib.clc_status_string(rc).decode())
    return om.value, cov.reshape(3, 3), pos


def _xy(xy, n):
    """positions of one descriptor set as (n, 2) float32, or None"""
    if xy is None:
        return None
    xy = np.ascontiguousarray(xy, dtype=np.float32).reshape(-1, 2)
    if xy.shape[0] != n:
        raise ValueError("positions: %d rows for a set of %d descriptors" % (xy.shape[0], n))
    return xy


def ratio_matches_to_pairs(match, xy_db=None, xy_q=None):
    """Host-only clc_ratio_matches_to_pairs: per-query ratio results (database row or -1) -> the de-duplicated, ordered (k, 2) int32
    list of (i_ = database row, j_ = query row); positions (database rows indexed by match, query rows) select the position pass."""
    lib = load_library()
    match = np.ascontiguousarray(match, dtype=np.int32).reshape(-1)
    if xy_db is not None:
        xy_db = np.ascontiguousarray(xy_db, dtype=np.float32).reshape(-1, 2)
    xy_q = _xy(xy_q, match.shape[0])
    out = np.empty((max(match.shape[0], 1), 2), dtype=np.int32)
    n = C.c_int(0)
    rc = lib.clc_ratio_matches_to_pairs(_p(match), match.shape[0], _p(xy_db), _p(xy_q), _p(out), C.byref(n))
    if rc != CLC_OK:
        raise CLCError(rc, "clc_ratio_matches_to_pairs: " + lib.clc_status_string(rc).decode())
    return out[:n.value].copy()


def _two_view_fill(tv, keep, x1, x2, K1, K2, img_wh, max_iteration, seed, precision):
    x1 = np.ascontiguousarray(x1, dtype=np.float64).reshape(-1, 2); x2 = np.ascontiguousarray(x2, dtype=np.float64).reshape(-1, 2)
    K1 = np.ascontiguousarray(K1, dtype=np.float64).reshape(9); K2 = np.ascontiguousarray(K2, dtype=np.float64).reshape(9)
    n = x1.shape[0]
    E, F = np.zeros(9), np.zeros(9)
    mask, inl = np.zeros(max(n, 1), dtype=np.uint8), np.zeros(max(n, 1), dtype=np.int32)
    keep.append((x1, x2, K1, K2, E, F, mask, inl))
    tv.x1, tv.x2, tv.K1, tv.K2, tv.n = x1.ctypes.data, x2.ctypes.data, K1.ctypes.data, K2.ctypes.data, n
    tv.img_w, tv.img_h, tv.max_iteration, tv.seed, tv.precision = int(img_wh[0]), int(img_wh[1]), int(max_iteration), int(seed), float(precision)
    tv.E, tv.F, tv.inlier_mask, tv.inliers = E.ctypes.data, F.ctypes.data, mask.ctypes.data, inl.ctypes.data
    return E, F, mask, inl


def _two_view_result(tv, E, F, mask, inl):
    ok = tv.n_inliers > 0
    return dict(E=E.reshape(3, 3).copy() if ok else None, F=F.reshape(3, 3).copy() if ok else None, mask=mask[:tv.n].astype(bool),
                inliers=inl[:tv.n_inliers].copy(), error_max=tv.error_max, min_nfa=tv.min_nfa, iterations=tv.iterations, status=tv.status)


def essential_acransac_batch(ctxs, problems, max_iteration=256, precision=float("inf")):
    """clc_essential_acransac_batch: problems = [(x1, x2, K1, K2, (w, h), seed), ...], one Context per problem; -> list of result dicts."""
    lib = load_library()
    n = len(problems)
    jobs = (TwoViewJob * n)()
    keep, outs = [], []
    for j, (x1, x2, K1, K2, wh, seed) in zip(jobs, problems):
        outs.append(_two_view_fill(j, keep, x1, x2, K1, K2, wh, max_iteration, seed, precision))
    hs = (C.c_void_p * n)(*[c.h for c in ctxs])
    rc = lib.clc_essential_acransac_batch(hs, jobs, n)
    if rc != CLC_OK:
        raise CLCError(rc, lib.clc_status_string(rc).decode())
    return [_two_view_result(j, *o) for j, o in zip(jobs, outs)]


def two_view_acransac_batch(ctxs, model, problems, max_iteration=256, precision=float("inf")):
    """clc_two_view_acransac_batch: model 'E' | 'F' | 'H'; problems = [(x1, x2, K1, K2, (w, h), seed), ...] (K1 / K2 read for 'E' only), one
    Context per problem; -> list of result dicts, "E" = the model matrix (E, F or H in pixels)."""
    lib = load_library()
    n = len(problems)
    jobs = (TwoViewJob * n)()
    keep, outs = [], []
    for j, (x1, x2, K1, K2, wh, seed) in zip(jobs, problems):
        outs.append(_two_view_fill(j, keep, x1, x2, np.eye(3) if K1 is None else K1, np.eye(3) if K2 is None else K2, wh, max_iteration, seed, precision))
    hs = (C.c_void_p * n)(*[c.h for c in ctxs])
    rc = lib.clc_two_view_acransac_batch(hs, ord(model), jobs, n)
    if rc != CLC_OK:
        raise CLCError(rc, lib.clc_status_string(rc).decode())
    return [_two_view_result(j, *o) for j, o in zip(jobs, outs)]


def inter_pose_batch(ctxs, problems, map_X, max_iteration=256, huber_a=16.0):
    """clc_inter_pose_batch: problems = [dict(x1, x2, K, wh, seed, Rt_source, and map_index (the shortcut) OR d_first_desc, first_feature,
    d_map_desc [, match_threshold] (the reference's chain: device addresses of the lower camera's descriptor block and of the global
    map's descriptors, the correspondences' rows in the former)), ...] (x1 = source frame's features, x2 = the destination's), one
    Context per problem, map_X the global map's points (M x 3); -> list of dicts (two-view result + Rt, cov, rmse, scale, n_front,
    n_common, n_map_matches, stage)."""
    lib = load_library()
    n = len(problems)
    jobs = (InterPoseJob * n)()
    map_X = np.ascontiguousarray(map_X, dtype=np.float64).reshape(-1, 3)
    keep, outs = [map_X], []
    for j, p in zip(jobs, problems):
        outs.append(_two_view_fill(j.tv, keep, p["x1"], p["x2"], p["K"], p["K"], p["wh"], max_iteration, p["seed"], float("inf")))
        rs = np.ascontiguousarray(p["Rt_source"], dtype=np.float64).reshape(12)
        keep.append(rs)
        j.map_X, j.map_n, j.Rt_source, j.huber_a = map_X.ctypes.data, int(map_X.shape[0]), rs.ctypes.data, float(huber_a)
        if p.get("d_first_desc") is not None:
            ff = np.ascontiguousarray(p["first_feature"], dtype=np.int32)
            keep.append(ff)
            j.d_first_desc, j.first_feature, j.d_map_desc = int(p["d_first_desc"]), ff.ctypes.data, int(p["d_map_desc"])
            j.match_threshold = int(p.get("match_threshold", 60))
        elif p.get("map_index") is not None:
            mi = np.ascontiguousarray(p["map_index"], dtype=np.int32)
            keep.append(mi)
            j.map_index = mi.ctypes.data
    hs = (C.c_void_p * n)(*[c.h for c in ctxs])
    rc = lib.clc_inter_pose_batch(hs, jobs, n)
    if rc != CLC_OK:
        raise CLCError(rc, lib.clc_status_string(rc).decode())
    res = []
    for j, o in zip(jobs, outs):
        d = _two_view_result(j.tv, *o)
        d.update(Rt=np.array(j.Rt).reshape(3, 4), cov=np.array(j.cov).reshape(6, 6), rmse=j.rmse, scale=j.scale, n_front=j.n_front,
                 n_common=j.n_common, n_refined=j.n_refined, stage=j.stage, n_map_matches=j.n_map_matches)
        res.append(d)
    return res


def mc_plan(counts, world, rank, grain):
    """clc_mc_plan: the shares of `rank` as a list of (first, second, q_begin, nq, out_offset)."""
    lib = load_library()
    cnt = (C.c_int * len(counts))(*[int(c) for c in counts])
    cap = len(counts) * len(counts) + 2
    out = (McShare * cap)()
    n = C.c_int()
    rc = lib.clc_mc_plan(cnt, len(counts), int(world), int(rank), int(grain), out, cap, C.byref(n))
    if rc != CLC_OK:
        raise CLCError(rc, lib.clc_status_string(rc).decode())
    return [(s.first, s.second, s.q_begin, s.nq, s.out_offset) for s in out[:n.value]]


class MultiCam:
    """clc_mc handle: one rank of the multi-camera exchange + match step (world = 1: no RCCL needed)."""

    def __init__(self, ctx, world=1, rank=0, maxkp=10000, unique_id=None):
        self.lib, self.ctx = load_library(), ctx
        h = C.c_void_p()
        idbuf = (C.c_uint8 * 128)(*unique_id) if unique_id is not None else None
        rc = self.lib.clc_mc_create(ctx.h, idbuf, world, rank, maxkp, C.byref(h))
        if rc != CLC_OK:
            raise CLCError(rc, "clc_mc_create: " + self.lib.clc_status_string(rc).decode())
        self.h, self.world, self.maxkp = h, world, maxkp

    @staticmethod
    def unique_id():
        lib = load_library()
        buf = (C.c_uint8 * 128)()
        rc = lib.clc_mc_unique_id(buf)
        if rc != CLC_OK:
            raise CLCError(rc, "clc_mc_unique_id: " + lib.clc_status_string(rc).decode())
        return bytes(buf)

    def _chk(self, rc):
        if rc != CLC_OK:
            raise CLCError(rc, "%s: %s" % (self.lib.clc_status_string(rc).decode(), self.lib.clc_mc_last_error_string(self.h).decode()))

    def arena(self):
        p = C.c_void_p()
        self._chk(self.lib.clc_mc_arena(self.h, C.byref(p), None, None))
        return p.value

    def gather_dev(self, d_my_desc, my_count, mode=0, stream=None):
        cnt = (C.c_int * self.world)()
        self._chk(self.lib.clc_mc_gather_dev(self.h, d_my_desc, int(my_count), int(mode), cnt, stream))
        return [int(c) for c in cnt]

    def virtual_put(self, other_rank, d_desc, count, stream=None):
        self._chk(self.lib.clc_mc_virtual_put(self.h, int(other_rank), d_desc, int(count), stream))

    def open_peers(self, stream=None):
        """Collective: map the peers' arenas now (the first peer-copy exchange would do it otherwise)."""
        self._chk(self.lib.clc_mc_open_peers(self.h, stream))

    def match_dev(self, threshold, d_match, capacity, stream=None):
        cap = self.world * self.world + 2
        sh = (McShare * cap)()
        n = C.c_int()
        self._chk(self.lib.clc_mc_match_dev(self.h, int(threshold), d_match, int(capacity), sh, cap, C.byref(n), stream))
        return [(s.first, s.second, s.q_begin, s.nq, s.out_offset) for s in sh[:n.value]]

    def gather_enqueue_dev(self, d_my_desc, my_count, mode=0, stream=None, d_my_count=None):
        """Enqueue-only exchange (no host synchronisation); my_count from the host, or d_my_count: device address of an int32."""
        self._chk(self.lib.clc_mc_gather_enqueue_dev(self.h, d_my_desc, int(my_count), d_my_count, int(mode), stream))

    def match_enqueue_dev(self, threshold, d_match, capacity, stream=None):
        """Capacity-planned shares, counts read on the device: pairs with clc_mc_gather_enqueue_dev."""
        cap = self.world * self.world + 2
        sh = (McShare * cap)()
        n = C.c_int()
        self._chk(self.lib.clc_mc_match_enqueue_dev(self.h, int(threshold), d_match, int(capacity), sh, cap, C.byref(n), stream))
        return [(s.first, s.second, s.q_begin, s.nq, s.out_offset) for s in sh[:n.value]]

    def set_overlap(self, on=True):
        """clc_mc_set_overlap: exchange (+ the caller's describe) on one stream, the sweep on another; before the first exchange."""
        self._chk(self.lib.clc_mc_set_overlap(self.h, 1 if on else 0))

    def comm_info(self):
        """(ncclCommCount, ncclCommUserRank) of the communicator behind the handle; (0, -1): none."""
        n, r = C.c_int(), C.c_int()
        self._chk(self.lib.clc_mc_comm_info(self.h, C.byref(n), C.byref(r)))
        return int(n.value), int(r.value)

    def counts(self, stream=None):
        cnt = (C.c_int * self.world)()
        self._chk(self.lib.clc_mc_counts(self.h, cnt, stream))
        return [int(c) for c in cnt]

    def close(self):
        if getattr(self, "h", None):
            self.lib.clc_mc_destroy(self.h)
            self.h = None


def pnp_localize_batch(ctxs, problems, max_iteration=256, seeds=None, precision=float("inf"), refine=True, huber_a=16.0):
    """clc_pnp_localize_ac_batch: problems = [(X, x, K), ...], one context per problem (all on one device); the a-contrario solves run
    interleaved on the GPU, driven by one host thread.  Returns a list of dicts like Context.pnp_acransac's."""
    lib = load_library()
    n = len(problems)
    assert len(ctxs) == n
    jobs = (PoseJob * n)()
    keep = []
    for i, (X, x, K) in enumerate(problems):
        X = np.ascontiguousarray(X, dtype=np.float64); x = np.ascontiguousarray(x, dtype=np.float64)
        K = np.ascontiguousarray(K, dtype=np.float64).reshape(9)
        N = X.shape[0]
        Rt, cov = np.zeros(12), np.zeros(36)
        mask, inl = np.zeros(max(N, 1), dtype=np.uint8), np.zeros(max(N, 1), dtype=np.int32)
        keep.append((X, x, K, Rt, cov, mask, inl))
        j = jobs[i]
        j.X, j.x, j.K, j.n = X.ctypes.data, x.ctypes.data, K.ctypes.data, N
        j.max_iteration, j.seed, j.precision = int(max_iteration), int(seeds[i] if seeds is not None else 1), float(precision)
        j.refine, j.huber_a = (1 if refine else 0), float(huber_a)
        j.Rt, j.cov, j.inlier_mask, j.inliers = Rt.ctypes.data, cov.ctypes.data, mask.ctypes.data, inl.ctypes.data
    hs = (C.c_void_p * n)(*[c.h for c in ctxs])
    rc = lib.clc_pnp_localize_ac_batch(hs, jobs, n)
    if rc != CLC_OK:
        raise CLCError(rc, "clc_pnp_localize_ac_batch: " + lib.clc_status_string(rc).decode())
    out = []
    for i in range(n):
        X, x, K, Rt, cov, mask, inl = keep[i]
        j = jobs[i]
        found = j.n_inliers > 0
        out.append(dict(Rt=Rt.reshape(3, 4) if found else None, cov=cov.reshape(6, 6) if (found and refine) else None,
                        mask=mask[:X.shape[0]].astype(bool), inliers=inl[:j.n_inliers].copy(), error_max=j.error_max, rmse=j.rmse,
                        iterations=j.iterations))
    return out


def _track_fill(j, keep, d_match, nq, cam, d_kps=None, d_feat=None, feat_stride=4, d_count=None, after_stream=None, max_iteration=256,
                seed=1, precision=float("inf"), refine=True, huber_a=16.0, outputs=True):
    """fills a TrackJob; cam = (focal, ppx, ppy, k1, k2, k3); device pointers as integers"""
    j.d_match, j.nq, j.d_count, j.d_kps, j.d_feat, j.feat_stride = d_match, int(nq), d_count, d_kps, d_feat, int(feat_stride)
    j.cam = CameraK3(*[float(v) for v in cam])
    j.after_stream = after_stream
    j.max_iteration, j.seed, j.precision, j.refine, j.huber_a = int(max_iteration), int(seed), float(precision), (1 if refine else 0), float(huber_a)
    if not outputs:
        return None
    n = max(int(nq), 1)
    Rt, cov = np.zeros(12), np.zeros(36)
    tq, tm, inl, mask = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.uint8)
    keep.append((Rt, cov, tq, tm, inl, mask))
    j.Rt, j.cov, j.track_query, j.track_map, j.inliers, j.inlier_mask = (a.ctypes.data for a in (Rt, cov, tq, tm, inl, mask))
    return Rt, cov, tq, tm, inl, mask


def _track_result(j, Rt, cov, tq, tm, inl, mask):
    found = j.n_inliers > 0
    nt = max(min(j.n_tracks, len(tq)), 0)
    return dict(Rt=Rt.reshape(3, 4).copy() if found else None, cov=cov.reshape(6, 6).copy() if (found and j.refine) else None,
                n_tracks=j.n_tracks, track_query=tq[:nt].copy(), track_map=tm[:nt].copy(), inliers=inl[:j.n_inliers].copy(),
                mask=mask[:nt].astype(bool), error_max=j.error_max, rmse=j.rmse, iterations=j.iterations, status=j.status)


def track_localize_batch_dev(ctxs, jobs):
    """clc_track_localize_batch_dev: jobs = [dict(d_match=, nq=, cam=, d_kps= | d_feat=, ...), ...] (the keywords of
    Context.track_localize_dev), job i on ctxs[i], the map points from ctxs[0].  Returns a list of result dicts."""
    lib = load_library()
    n = len(jobs)
    assert len(ctxs) == n
    arr = (TrackJob * n)()
    keep = []
    outs = [_track_fill(arr[i], keep, **jobs[i]) for i in range(n)]
    hs = (C.c_void_p * n)(*[c.h for c in ctxs])
    rc = lib.clc_track_localize_batch_dev(hs, arr, n)
    if rc != CLC_OK:
        raise CLCError(rc, "clc_track_localize_batch_dev: %s: %s" % (lib.clc_status_string(rc).decode(), lib.clc_last_error_string(ctxs[0].h).decode()))
    return [_track_result(arr[i], *outs[i]) for i in range(n)]


def _track_prior_fill(j, keep, d_match, nq, cam, Rt_prior, gate, d_kps=None, d_feat=None, feat_stride=4, d_count=None, after_stream=None,
                      huber_a=16.0, rounds=0, max_iter=0, min_inliers=0):
    """fills a TrackPriorJob; cam = (focal, ppx, ppy, k1, k2, k3); device pointers as integers; Rt_prior (3, 4)"""
    j.d_match, j.nq, j.d_count, j.d_kps, j.d_feat, j.feat_stride = d_match, int(nq), d_count, d_kps, d_feat, int(feat_stride)
    j.cam = CameraK3(*[float(v) for v in cam])
    j.after_stream = after_stream
    j.Rt_prior = (C.c_double * 12)(*[float(v) for v in np.asarray(Rt_prior, dtype=np.float64).reshape(12)])
    j.gate, j.huber_a, j.rounds, j.max_iter, j.min_inliers = float(gate), float(huber_a), int(rounds), int(max_iter), int(min_inliers)
    n = max(int(nq), 1)
    Rt, cov = np.zeros(12), np.zeros(36)
    tq, tm, mask = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.uint8)
    keep.append((Rt, cov, tq, tm, mask))
    j.Rt, j.cov, j.track_query, j.track_map, j.inlier_mask = (a.ctypes.data for a in (Rt, cov, tq, tm, mask))
    return Rt, cov, tq, tm, mask


def _track_prior_result(j, Rt, cov, tq, tm, mask):
    nt = max(min(j.n_tracks, len(tq)), 0)
    return dict(Rt=Rt.reshape(3, 4).copy(), cov=cov.reshape(6, 6).copy(), n_tracks=j.n_tracks, track_query=tq[:nt].copy(),
                track_map=tm[:nt].copy(), mask=mask[:nt].astype(bool), n_inliers=j.n_inliers, iterations=j.iterations,
                rounds_run=j.rounds_run, converged=j.converged, result=j.result, rmse=j.rmse, status=j.status)


def track_prior_batch_dev(ctxs, jobs):
    """clc_track_prior_batch_dev: jobs = [dict(d_match=, nq=, cam=, Rt_prior=, gate=, d_kps= | d_feat=, ...), ...] (the keywords of
    Context.track_prior_dev), job i on ctxs[i], the map points from ctxs[0].  Returns a list of result dicts."""
    lib = load_library()
    n = len(jobs)
    assert len(ctxs) == n
    arr = (TrackPriorJob * max(n, 1))()
    keep = []
    outs = [_track_prior_fill(arr[i], keep, **jobs[i]) for i in range(n)]
    hs = (C.c_void_p * max(n, 1))(*[c.h for c in ctxs])
    rc = lib.clc_track_prior_batch_dev(hs, arr, n)
    if rc != CLC_OK:
        raise CLCError(rc, "clc_track_prior_batch_dev: %s: %s" % (lib.clc_status_string(rc).decode(), lib.clc_last_error_string(ctxs[0].h).decode()))
    return [_track_prior_result(arr[i], *outs[i]) for i in range(n)]


def _pair_fill(j, keep, d_match, nq, nt, cam_a, cam_b, d_kps_a=None, d_feat_a=None, feat_stride_a=4, d_kps_b=None, d_feat_b=None,
               feat_stride_b=4, d_count_a=None, d_count_b=None, after_stream=None, img_wh=(0, 0), max_iteration=256, seed=1,
               precision=float("inf"), outputs=True):
    """fills a PairJob; cam_* = (focal, ppx, ppy, k1, k2, k3); device pointers as integers"""
    j.d_match, j.nq, j.nt, j.d_count_a, j.d_count_b = d_match, int(nq), int(nt), d_count_a, d_count_b
    j.d_kps_a, j.d_feat_a, j.feat_stride_a = d_kps_a, d_feat_a, int(feat_stride_a)
    j.d_kps_b, j.d_feat_b, j.feat_stride_b = d_kps_b, d_feat_b, int(feat_stride_b)
    j.cam_a, j.cam_b = CameraK3(*[float(v) for v in cam_a]), CameraK3(*[float(v) for v in cam_b])
    j.after_stream = after_stream
    j.img_w, j.img_h, j.max_iteration, j.seed, j.precision = int(img_wh[0]), int(img_wh[1]), int(max_iteration), int(seed), float(precision)
    if not outputs:
        return None
    n = max(int(nq), 1)
    M, F, x1, x2 = np.zeros(9), np.zeros(9), np.zeros((n, 2)), np.zeros((n, 2))
    pq, pt, inl, mask = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.uint8)
    keep.append((M, F, pq, pt, x1, x2, inl, mask))
    j.M, j.F, j.pair_q, j.pair_t, j.x1, j.x2, j.inliers, j.inlier_mask = (a.ctypes.data for a in (M, F, pq, pt, x1, x2, inl, mask))
    return M, F, pq, pt, x1, x2, inl, mask


def _pair_result(j, M, F, pq, pt, x1, x2, inl, mask):
    found = j.n_inliers > 0
    n = max(min(j.n_pairs, len(pq)), 0)
    return dict(M=M.reshape(3, 3).copy() if found else None, F=F.reshape(3, 3).copy() if found else None, n_pairs=j.n_pairs,
                pair_q=pq[:n].copy(), pair_t=pt[:n].copy(), x1=x1[:n].copy(), x2=x2[:n].copy(), inliers=inl[:j.n_inliers].copy(),
                mask=mask[:n].astype(bool), error_max=j.error_max, min_nfa=j.min_nfa, iterations=j.iterations, status=j.status)


def _guided_fill(j, d_q, nq, d_t, nt, cam_a, cam_b, F, band, threshold, d_match, d_kps_a=None, d_feat_a=None, feat_stride_a=4, d_kps_b=None,
                 d_feat_b=None, feat_stride_b=4, d_count_a=None, d_count_b=None, d_best=None, d_second=None, d_line=None, d_tpos=None):
    """fills a GuidedJob; cam_* = (focal, ppx, ppy, k1, k2, k3), F = 9 numbers row-major (pixels, x_b^T F x_a = 0); device pointers as integers"""
    j.d_q, j.nq, j.d_t, j.nt, j.d_count_a, j.d_count_b = d_q, int(nq), d_t, int(nt), d_count_a, d_count_b
    j.d_kps_a, j.d_feat_a, j.feat_stride_a = d_kps_a, d_feat_a, int(feat_stride_a)
    j.d_kps_b, j.d_feat_b, j.feat_stride_b = d_kps_b, d_feat_b, int(feat_stride_b)
    j.cam_a, j.cam_b = CameraK3(*[float(v) for v in cam_a]), CameraK3(*[float(v) for v in cam_b])
    j.F = (C.c_double * 9)(*[float(v) for v in np.asarray(F, dtype=np.float64).reshape(9)])
    j.band, j.threshold = float(band), int(threshold)
    j.d_match, j.d_best, j.d_second, j.d_line, j.d_tpos = d_match, d_best, d_second, d_line, d_tpos


def _map_guided_fill(j, d_q, nq, cam, Rt, radius, threshold, d_match, d_kps=None, d_feat=None, feat_stride=4, d_count=None, d_best=None,
                     d_second=None, d_qpos=None, d_proj=None):
    """fills a MapGuidedJob; cam = (focal, ppx, ppy, k1, k2, k3), Rt = 12 numbers, the predicted [R|t] row-major 3 x 4; device pointers as
    integers"""
    j.d_q, j.nq, j.d_count, j.d_kps, j.d_feat, j.feat_stride = d_q, int(nq), d_count, d_kps, d_feat, int(feat_stride)
    j.cam = CameraK3(*[float(v) for v in cam])
    j.Rt = (C.c_double * 12)(*[float(v) for v in np.asarray(Rt, dtype=np.float64).reshape(12)])
    j.radius, j.threshold = float(radius), int(threshold)
    j.d_match, j.d_best, j.d_second, j.d_qpos, j.d_proj = d_match, d_best, d_second, d_qpos, d_proj


def _extend_view_fill(v, d_desc, n, cam, Rt, d_kps=None, d_feat=None, feat_stride=4, d_count=None, d_track=None):
    """fills an ExtendView; cam = (focal, ppx, ppy, k1, k2, k3), Rt = 12 numbers, the view's [R|t] row-major 3 x 4; device pointers as integers"""
    v.d_desc, v.n, v.d_count, v.d_kps, v.d_feat, v.feat_stride = d_desc, int(n), d_count, d_kps, d_feat, int(feat_stride)
    v.cam = CameraK3(*[float(c) for c in cam])
    v.Rt = (C.c_double * 12)(*[float(c) for c in np.asarray(Rt, dtype=np.float64).reshape(12)])
    v.d_track = d_track


def _extend_fill(j, keep, view_a, view_b, band, threshold, max_distance, update_tracks=True, after_stream=None, d_new_q=None, d_new_t=None):
    _extend_view_fill(j.a, **view_a)
    _extend_view_fill(j.b, **view_b)
    j.band, j.threshold, j.max_distance, j.update_tracks, j.after_stream = float(band), int(threshold), int(max_distance), int(bool(update_tracks)), after_stream
    j.d_new_q, j.d_new_t = d_new_q, d_new_t
    n = max(int(view_a["n"]), 1)
    q, t, X = np.full(n, -1, dtype=np.int32), np.full(n, -1, dtype=np.int32), np.zeros((n, 3))
    j.new_q, j.new_t, j.X = _p(q), _p(t), _p(X)
    keep.append((q, t, X))
    return q, t, X


def _extend_result(j, q, t, X):
    n = j.n_added
    return dict(new_q=q[:n].copy(), new_t=t[:n].copy(), X=X[:n].copy(), F=np.array(list(j.F)).reshape(3, 3), map_n_before=j.map_n_before,
                n_guided=j.n_guided, n_added=n, n_dropped=j.n_dropped, status=j.status)


def _observe_fill(j, n, cam, Rt, width, height, gate, margin=0.0, d_kps=None, d_feat=None, feat_stride=4, d_count=None, d_track=None, d_counts=None,
                  after_stream=None):
    """fills a MapObserve; cam = (focal, ppx, ppy, k1, k2, k3), Rt = 12 numbers, the frame's [R|t] row-major 3 x 4; device pointers as integers"""
    v = j.view
    v.n, v.d_count, v.d_kps, v.d_feat, v.feat_stride = int(n), d_count, d_kps, d_feat, int(feat_stride)
    v.cam = CameraK3(*[float(c) for c in cam])
    v.Rt = (C.c_double * 12)(*[float(c) for c in np.asarray(Rt, dtype=np.float64).reshape(12)])
    v.d_track, v.d_counts = d_track, d_counts
    j.width, j.height, j.gate, j.margin, j.after_stream = int(width), int(height), float(gate), float(margin), after_stream


def fundamental_from_poses(cam_a, Rt_a, cam_b, Rt_b):
    """clc_fundamental_from_poses: F (3, 3) of two posed views, x_b^T F x_a = 0 in undistorted pixels; cam = (focal, ppx, ppy, ...),
    Rt = 12 numbers, [R|t] row-major.  Host arithmetic: no context, no GPU."""
    lib = load_library()
    ca, cb = CameraK3(*([float(v) for v in cam_a] + [0.0] * 6)[:6]), CameraK3(*([float(v) for v in cam_b] + [0.0] * 6)[:6])
    Ra, Rb = np.ascontiguousarray(Rt_a, dtype=np.float64).reshape(12), np.ascontiguousarray(Rt_b, dtype=np.float64).reshape(12)
    F = np.zeros(9)
    rc = lib.clc_fundamental_from_poses(C.byref(ca), _p(Ra), C.byref(cb), _p(Rb), _p(F))
    if rc != 0:
        raise CLCError(rc, "clc_fundamental_from_poses: " + lib.clc_status_string(rc).decode())
    return F.reshape(3, 3)


def pair_filter_batch_dev(ctxs, model, jobs):
    """clc_pair_filter_batch_dev: model 'E' | 'F' | 'H'; jobs = [dict(d_match=, nq=, nt=, cam_a=, cam_b=, d_kps_a= | d_feat_a=, ...), ...]
    (the keywords of Context.pair_filter_dev), job i on ctxs[i].  Returns a list of result dicts."""
    lib = load_library()
    n = len(jobs)
    assert len(ctxs) == n
    arr = (PairJob * n)()
    keep = []
    outs = [_pair_fill(arr[i], keep, **jobs[i]) for i in range(n)]
    hs = (C.c_void_p * n)(*[c.h for c in ctxs])
    rc = lib.clc_pair_filter_batch_dev(hs, ord(model), arr, n)
    if rc != CLC_OK:
        raise CLCError(rc, "clc_pair_filter_batch_dev: %s: %s" % (lib.clc_status_string(rc).decode(), lib.clc_last_error_string(ctxs[0].h).decode()))
    return [_pair_result(arr[i], *outs[i]) for i in range(n)]


def _inter_dev_fill(j, keep, Rt_source, huber_a=16.0, lower_is_b=False, d_first_desc=None, d_map_desc=None, d_map_match_a=None,
                    match_threshold=60, **pair):
    """fills an InterDevJob: the keywords of Context.pair_filter_dev for the pair, then the step's own"""
    out = _pair_fill(j.pair, keep, **pair)
    rs = np.ascontiguousarray(Rt_source, dtype=np.float64).reshape(12)
    keep.append(rs)
    j.Rt_source, j.huber_a, j.lower_is_b = rs.ctypes.data, float(huber_a), (1 if lower_is_b else 0)
    j.d_first_desc, j.d_map_desc, j.d_map_match_a, j.match_threshold = d_first_desc, d_map_desc, d_map_match_a, int(match_threshold)
    return out


def _inter_dev_result(j, *out):
    d = _pair_result(j.pair, *out)
    d["E"] = d["M"]
    d.update(Rt=np.array(j.Rt).reshape(3, 4), cov=np.array(j.cov).reshape(6, 6), rmse=j.rmse, scale=j.scale, n_front=j.n_front,
             n_common=j.n_common, n_refined=j.n_refined, stage=j.stage, n_map_matches=j.n_map_matches)
    return d


def inter_pose_batch_dev(ctxs, jobs):
    """clc_inter_pose_batch_dev: jobs = [dict(Rt_source=, d_map_match_a= | d_first_desc=, d_map_desc= [, lower_is_b, match_threshold],
    huber_a=, and the pair's keywords of Context.pair_filter_dev), ...], job i on ctxs[i], the map points from ctxs[0]
    (Context.set_map_points).  Returns a list of dicts shaped like inter_pose_batch's: the pair filter's result + Rt, cov, rmse, scale,
    n_front, n_common, n_refined, n_map_matches, stage."""
    lib = load_library()
    n = len(jobs)
    assert len(ctxs) == n
    arr = (InterDevJob * n)()
    keep = []
    outs = [_inter_dev_fill(arr[i], keep, **jobs[i]) for i in range(n)]
    hs = (C.c_void_p * n)(*[c.h for c in ctxs])
    rc = lib.clc_inter_pose_batch_dev(hs, arr, n)
    if rc != CLC_OK:
        raise CLCError(rc, "clc_inter_pose_batch_dev: %s: %s" % (lib.clc_status_string(rc).decode(), lib.clc_last_error_string(ctxs[0].h).decode()))
    return [_inter_dev_result(arr[i], *outs[i]) for i in range(n)]


def seed_poses(origin_R, origin_C, rel_R, rel_C, scale):
    """The two seed cameras' [R|t] (3 x 4 each) as Reconstructor::triangulatePoints forms them (Reconstructor.hpp:215-221, 247-257):
    camera I = the origin pose (rotation, centre), camera J = relativePoseToAbsolute(origin, Pose3(rel_R, scale * rel_C)) -- R = rel_R
    origin_R, C = origin_C + scale rel_C, t = -R C.  The operations of coloc_amd/csrc/map_math.h in its order, one IEEE operation at a
    time: the same bits as clc_map_init_batch_dev's."""
    Ro = [float(v) for v in np.asarray(origin_R, dtype=np.float64).reshape(9)]
    Co = [float(v) for v in np.asarray(origin_C, dtype=np.float64).reshape(3)]
    Rr = [float(v) for v in np.asarray(rel_R, dtype=np.float64).reshape(9)]
    Cr = [float(v) for v in np.asarray(rel_C, dtype=np.float64).reshape(3)]
    scale = float(scale)
    R = [Rr[3 * r] * Ro[q] + Rr[3 * r + 1] * Ro[3 + q] + Rr[3 * r + 2] * Ro[6 + q] for r in range(3) for q in range(3)]
    Cj = [Co[q] + scale * Cr[q] for q in range(3)]
    Rt_i, Rt_j = np.zeros((3, 4)), np.zeros((3, 4))
    for r in range(3):
        Rt_i[r, :3] = Ro[3 * r:3 * r + 3]
        Rt_j[r, :3] = R[3 * r:3 * r + 3]
        Rt_i[r, 3] = -(Ro[3 * r] * Co[0] + Ro[3 * r + 1] * Co[1] + Ro[3 * r + 2] * Co[2])
        Rt_j[r, 3] = -(R[3 * r] * Cj[0] + R[3 * r + 1] * Cj[1] + R[3 * r + 2] * Cj[2])
    return Rt_i, Rt_j


def tracks_capacity(rows, pairs):
    """tracks the table of clc_tracks_build_dev / clc_map_build_dev has room for: min(sum of n, (sum of rows) / 2)"""
    return min(sum(int(p["n"]) for p in pairs), sum(int(r) for r in rows) // 2)


def _tracks_fill(t, keep, rows, pairs):
    """fills a TracksJob: rows = row capacity per camera, pairs = [dict(cam_a=, cam_b=, d_q=, d_t=, n= [, d_n, d_index, n_list]), ...]"""
    t.n_cams = len(rows)
    for c, r in enumerate(rows[:MAX_BATCH]):
        t.rows[c] = int(r)
    arr = (TracksPair * max(len(pairs), 1))()
    for a, p in zip(arr, pairs):
        a.cam_a, a.cam_b, a.d_q, a.d_t, a.n = int(p["cam_a"]), int(p["cam_b"]), p.get("d_q"), p.get("d_t"), int(p.get("n", 0))
        a.d_n, a.d_index, a.n_list = p.get("d_n"), p.get("d_index"), int(p.get("n_list", 0))
    keep.append(arr)
    t.n_pairs, t.pairs = len(pairs), arr


def _map_fill(j, keep, rows, pairs, cams, seed_pair=0, Rt_seed_a=None, Rt_seed_b=None, after_stream=None, origin_R=None, origin_C=None,
              scale=1.0, outputs=True):
    """fills a MapJob; cams = [dict(cam=(focal, ppx, ppy, k1, k2, k3), d_kps= | d_feat= [, feat_stride], d_desc=), ...]"""
    _tracks_fill(j.tracks, keep, rows, pairs)
    for m, c in zip(j.cams, cams):
        m.d_kps, m.d_feat, m.feat_stride, m.d_desc = c.get("d_kps"), c.get("d_feat"), int(c.get("feat_stride", 4)), c.get("d_desc")
        m.cam = CameraK3(*[float(v) for v in c["cam"]])
    j.seed_pair, j.after_stream, j.scale = int(seed_pair), after_stream, float(scale)
    for dst, src, n in ((j.Rt_seed_a, Rt_seed_a, 12), (j.Rt_seed_b, Rt_seed_b, 12), (j.origin_R, origin_R, 9), (j.origin_C, origin_C, 3)):
        if src is not None:
            dst[:] = [float(v) for v in np.asarray(src, dtype=np.float64).reshape(n)]
    if not outputs:
        return None
    cap = max(sum(int(r) for r in rows) // 2, 1)             # (tracks_capacity before the pairs' counts are known)
    tf = np.full((cap, len(rows)), -1, dtype=np.int32)
    mt, mr, X = np.zeros(cap, dtype=np.int32), np.zeros(cap, dtype=np.int32), np.zeros((cap, 3))
    keep.append((tf, mt, mr, X))
    j.track_feat, j.map_track, j.map_row, j.X = (a.ctypes.data for a in (tf, mt, mr, X))
    return tf, mt, mr, X


def _map_result(j, tf, mt, mr, X):
    n, k = max(j.map_n, 0), max(j.n_tracks, 0)
    return dict(n_tracks=j.n_tracks, map_n=j.map_n, track_feat=tf[:k].copy(), map_track=mt[:n].copy(), map_row=mr[:n].copy(), X=X[:n].copy(),
                seed_pair=j.seed_pair, Rt_seed_a=np.array(j.Rt_seed_a).reshape(3, 4), Rt_seed_b=np.array(j.Rt_seed_b).reshape(3, 4),
                entered=[bool(v) for v in j.entered[:j.tracks.n_pairs]], status=j.status)


def map_init_batch_dev(ctxs, pair_jobs, rows, pair_cams, cams, origin_R=np.eye(3), origin_C=np.zeros(3), scale=1.0):
    """clc_map_init_batch_dev: pair_jobs = [dict(the keywords of Context.pair_filter_dev), ...], job p on ctxs[p] and between the cameras
    pair_cams[p] = (cam_a, cam_b); rows / cams as Context.map_build_dev.  The filters run under 'E'; the pairs with at least 13 inliers
    and a successful chirality vote enter the tracks, the one with the most inliers is the seed; the map is installed on ctxs[0].
    Returns (map result dict with seed_pair / Rt_seed_* / entered, [pair filter result dicts])."""
    return _map_compose("clc_map_init_batch_dev", ctxs, pair_jobs, rows, pair_cams, cams, origin_R, origin_C, scale)


def _steps_fill(keep, rows, ctx, align=None, sim=None, grow=None, ba=None):
    """The optional steps of a map composition, each None (absent) or the tuple of that step's fill arguments -- align: (threshold,); sim,
    grow, ba: those of _sim_fill, _grow_fill, _ba_fill -> [(key, filled struct, its host arrays), ...] in the order the header passes
    them: align or sim, grow, ba.  ctx: the context whose map is replaced (the room for match / inlier is its maxkp)"""
    steps = []
    if align is not None:
        al = MapAlign()
        match = np.full(max(int(ctx.mopts.maxkp), 1), -2, dtype=np.int32)
        al.threshold, al.match = int(align[0]), match.ctypes.data
        steps.append(("align", al, (match, None)))
    if sim is not None:
        a = MapAlignSim()
        steps.append(("sim", a, _sim_fill(a, ctx.mopts.maxkp, *sim) + (None,)))
    if grow is not None:
        g = MapGrow()
        steps.append(("grow", g, _grow_fill(g, keep, rows, *grow)))
    if ba is not None:
        b = MapBa()
        _ba_fill(b, *ba)
        steps.append(("ba", b, ()))
    return steps


def _steps_result(res, j, n_cams, steps):
    """one dict per step of _steps_fill into the map result dict, under the step's key"""
    for key, s, host in steps:
        res[key] = (_align_result(s, *host) if key == "align" else _sim_result(s, *host) if key == "sim" else
                    _grow_result(s, n_cams, j.map_n, *host) if key == "grow" else _ba_result(s))
    return res


def _map_compose(entry, ctxs, pair_jobs, rows, pair_cams, cams, origin_R, origin_C, scale, **steps):
    """What the seven clc_map_*_batch_dev wrappers share: the pair jobs, the map job, the steps' structs (_steps_fill's keywords), the call
    of `entry` and the results.  The sim entry takes all of sim, grow and ba, NULL for an absent one; the others exactly theirs."""
    lib = load_library()
    n = len(pair_jobs)
    assert len(ctxs) == n == len(pair_cams)
    arr = (PairJob * n)()
    keep = []
    outs = [_pair_fill(arr[i], keep, **pair_jobs[i]) for i in range(n)]
    j = MapJob()
    out = _map_fill(j, keep, rows, [dict(cam_a=a, cam_b=b) for a, b in pair_cams], cams, origin_R=origin_R, origin_C=origin_C, scale=scale)
    filled = _steps_fill(keep, rows, ctxs[0], **steps)
    refs = {key: C.byref(s) for key, s, _ in filled}
    args = [refs.get(key) for key in ("sim", "grow", "ba")] if "sim" in refs else list(refs.values())
    hs = (C.c_void_p * n)(*[c.h for c in ctxs])
    rc = getattr(lib, entry)(hs, arr, n, C.byref(j), *args)
    if rc != CLC_OK:
        raise CLCError(rc, "%s: %s: %s" % (entry, lib.clc_status_string(rc).decode(), lib.clc_last_error_string(ctxs[0].h).decode()))
    return _steps_result(_map_result(j, *out), j, len(rows), filled), [_pair_result(arr[i], *outs[i]) for i in range(n)]


def _align_result(a, match, X):
    n_old, n_new = max(a.n_old, 0), max(a.n_new, 0)
    return dict(scale=float(a.scale), n_old=a.n_old, n_common=a.n_common, n_terms=a.n_terms, status=a.status,
                match=None if match is None else match[:n_old].copy(), X=None if X is None else X[:n_new].copy())


def map_update_batch_dev(ctxs, pair_jobs, rows, pair_cams, cams, origin_R=np.eye(3), origin_C=np.zeros(3), scale=1.0, threshold=0):
    """clc_map_update_batch_dev: map_init_batch_dev's arguments; the new map is brought to the scale of the map ctxs[0] holds and replaces
    it.  Returns (map result dict -- X and Rt_seed_* RESCALED -- with an "align" dict: scale, n_old, n_common, n_terms, status, match;
    [pair filter result dicts])."""
    return _map_compose("clc_map_update_batch_dev", ctxs, pair_jobs, rows, pair_cams, cams, origin_R, origin_C, scale, align=(threshold,))


def _sim_fill(a, maxkp, threshold=0, apply=SIM_APPLY_SCALE, sim_max_iteration=0, sim_seed=1, sim_precision=float("inf"), want_match=True):
    """fills the in fields a composition reads of a MapAlignSim; -> (match, inlier) host arrays"""
    a.threshold, a.apply, a.max_iteration, a.seed, a.precision = int(threshold), int(apply), int(sim_max_iteration), int(sim_seed), float(sim_precision)
    match = np.full(max(int(maxkp), 1), -2, dtype=np.int32) if want_match else None
    inlier = np.zeros(max(int(maxkp), 1), dtype=np.uint8)
    a.match, a.inlier = (None if match is None else match.ctypes.data), inlier.ctypes.data
    return match, inlier


def _sim_result(a, match, inlier, X):
    n_old, n_new, n_com = max(a.n_old, 0), max(a.n_new, 0), max(a.n_common, 0)
    return dict(s=float(a.s), R=np.array(a.R).reshape(3, 3), t=np.array(a.t), n_old=a.n_old, n_common=a.n_common, n_inliers=a.n_inliers,
                iterations=a.iterations, refit=a.refit, status=a.status, error_max=float(a.error_max), min_nfa=float(a.min_nfa),
                match=None if match is None else match[:n_old].copy(), inlier=inlier[:n_com].astype(bool),
                X=None if X is None else X[:n_new].copy())


def map_update_sim_batch_dev(ctxs, pair_jobs, rows, pair_cams, cams, origin_R=np.eye(3), origin_C=np.zeros(3), scale=1.0, threshold=0,
                             apply=SIM_APPLY_SCALE, sim_max_iteration=0, sim_seed=1, sim_precision=float("inf"), grow=False, ba=False,
                             max_iteration=256, seed=0, precision=float("inf"), ba_max_iterations=0, huber_a=0.0, function_tolerance=0.0):
    """clc_map_update_sim_batch_dev: map_update_batch_dev (grow=False), map_update_grow_batch_dev (grow=True) or
    map_update_grow_ba_batch_dev (grow=True, ba=True) with the a-contrario similarity in place of the align step.  Returns (map result
    dict -- X, Rt_seed_* and grow["Rt"] under the apply rule -- with a "sim" dict and, as asked, "grow" and "ba"; [pair filter results])."""
    return _map_compose("clc_map_update_sim_batch_dev", ctxs, pair_jobs, rows, pair_cams, cams, origin_R, origin_C, scale,
                        sim=(threshold, apply, sim_max_iteration, sim_seed, sim_precision), grow=(max_iteration, seed, precision) if grow else None,
                        ba=(ba_max_iterations, huber_a, function_tolerance) if ba else None)


def _grow_fill(g, keep, rows, max_iteration=256, seed=0, precision=float("inf")):
    """fills a MapGrow; -> (map_cam, map_obs) host arrays with room as _map_fill's map_track"""
    g.max_iteration, g.seed, g.precision = int(max_iteration), int(seed), float(precision)
    cap = max(sum(int(r) for r in rows) // 2, 1)
    mc, mo = np.full(cap, -1, dtype=np.int32), np.zeros(cap, dtype=np.uint8)
    keep.append((mc, mo))
    g.map_cam, g.map_obs = mc.ctypes.data, mo.ctypes.data
    return mc, mo


def _grow_result(g, n_cams, map_n, mc, mo):
    n = max(map_n, 0)
    return dict(resected=[bool(v) for v in g.resected[:n_cams]], status=list(g.status[:n_cams]), n_corr=list(g.n_corr[:n_cams]),
                n_inliers=list(g.n_inliers[:n_cams]), error_max=[float(v) for v in g.error_max[:n_cams]],
                Rt=[np.array(g.Rt[c]).reshape(3, 4) for c in range(n_cams)], n_seed_rows=g.n_seed_rows, n_added=g.n_added,
                map_cam=mc[:n].copy(), map_obs=mo[:n].copy())


def map_init_grow_batch_dev(ctxs, pair_jobs, rows, pair_cams, cams, origin_R=np.eye(3), origin_C=np.zeros(3), scale=1.0, max_iteration=256, seed=0,
                            precision=float("inf")):
    """clc_map_init_grow_batch_dev: map_init_batch_dev's arguments + the resections' max_iteration / seed / precision; the map grown past
    the seed pair is installed on ctxs[0].  Returns (map result dict with a "grow" dict: resected, status, n_corr, n_inliers, error_max,
    Rt per camera, n_seed_rows, n_added, map_cam, map_obs; [pair filter result dicts])."""
    return _map_compose("clc_map_init_grow_batch_dev", ctxs, pair_jobs, rows, pair_cams, cams, origin_R, origin_C, scale,
                        grow=(max_iteration, seed, precision))


def map_update_grow_batch_dev(ctxs, pair_jobs, rows, pair_cams, cams, origin_R=np.eye(3), origin_C=np.zeros(3), scale=1.0, threshold=0,
                              max_iteration=256, seed=0, precision=float("inf")):
    """clc_map_update_grow_batch_dev: map_update_batch_dev on the grown map.  Returns (map result dict -- X, Rt_seed_* and grow["Rt"]
    RESCALED -- with "align" and "grow" dicts; [pair filter result dicts])."""
    return _map_compose("clc_map_update_grow_batch_dev", ctxs, pair_jobs, rows, pair_cams, cams, origin_R, origin_C, scale,
                        align=(threshold,), grow=(max_iteration, seed, precision))


def _ba_fill(b, max_iterations=0, huber_a=0.0, function_tolerance=0.0):
    b.max_iterations, b.huber_a, b.function_tolerance = int(max_iterations), float(huber_a), float(function_tolerance)


def _ba_result(b):
    return dict(status=b.status, iterations=b.iterations, n_cams=b.n_cams, n_points=b.n_points, n_obs=b.n_obs,
                cost_initial=float(b.cost_initial), cost_final=float(b.cost_final), rmse=float(b.rmse))


def map_init_grow_ba_batch_dev(ctxs, pair_jobs, rows, pair_cams, cams, origin_R=np.eye(3), origin_C=np.zeros(3), scale=1.0, max_iteration=256, seed=0,
                               precision=float("inf"), ba_max_iterations=0, huber_a=0.0, function_tolerance=0.0):
    """clc_map_init_grow_ba_batch_dev: map_init_grow_batch_dev with the grown map bundle-adjusted before it is installed.  Returns (map
    result dict -- X, Rt_seed_* and grow["Rt"] REFINED -- with "grow" and "ba" dicts; [pair filter result dicts])."""
    return _map_compose("clc_map_init_grow_ba_batch_dev", ctxs, pair_jobs, rows, pair_cams, cams, origin_R, origin_C, scale,
                        grow=(max_iteration, seed, precision), ba=(ba_max_iterations, huber_a, function_tolerance))


def map_update_grow_ba_batch_dev(ctxs, pair_jobs, rows, pair_cams, cams, origin_R=np.eye(3), origin_C=np.zeros(3), scale=1.0, threshold=0,
                                 max_iteration=256, seed=0, precision=float("inf"), ba_max_iterations=0, huber_a=0.0, function_tolerance=0.0):
    """clc_map_update_grow_ba_batch_dev: map_update_grow_batch_dev with the grown map bundle-adjusted before the align step.  Returns (map
    result dict -- X, Rt_seed_* and grow["Rt"] REFINED, then RESCALED -- with "align", "grow" and "ba" dicts; [pair filter result dicts])."""
    return _map_compose("clc_map_update_grow_ba_batch_dev", ctxs, pair_jobs, rows, pair_cams, cams, origin_R, origin_C, scale,
                        align=(threshold,), grow=(max_iteration, seed, precision), ba=(ba_max_iterations, huber_a, function_tolerance))


def desc_handle_live(handle):
    """1 while the publication the handle came from still stands (same host address, count and generation)."""
    return bool(load_library().clc_desc_handle_live(C.byref(handle)))


def desc_cache_stats():
    """(hits, misses) of the descriptor cache behind the host-pointer match entry points."""
    lib = load_library()
    h, m = C.c_ulonglong(), C.c_ulonglong()
    lib.clc_desc_cache_stats(C.byref(h), C.byref(m))
    return int(h.value), int(m.value)


def keypoints_to_features(kps):
    lib = load_library()
    kps = np.ascontiguousarray(kps, dtype=KP_DTYPE)
    out = np.zeros((len(kps), 4), dtype=np.float32)
    rc = lib.clc_keypoints_to_features(_p(kps), len(kps), _p(out))
    if rc != CLC_OK:
        raise CLCError(rc, lib.clc_status_string(rc).decode())
    return out


class Context:
    """One clc_ctx: device buffers + stream on one GPU (one per host thread / per rank)."""

    def __init__(self, device=0, width=640, height=480, maxkp=10000, scale_factor=1.2, scale_levels=8,
                 fast_thresh=40, match_thresh=60, detector=True, matcher=True):
        self.lib = load_library()
        self.dopts = DetectorOptions(scale_factor, scale_levels, width, height, maxkp, fast_thresh)
        self.mopts = MatcherOptions(0.8, match_thresh, maxkp)
        h = C.c_void_p()
        rc = self.lib.clc_ctx_create(device, C.byref(self.dopts) if detector else None,
                                     C.byref(self.mopts) if matcher else None, C.byref(h))
        if rc != CLC_OK:
            raise CLCError(rc, "clc_ctx_create: " + self.lib.clc_status_string(rc).decode())
        self.h = h
        self.device = device

    def _chk(self, rc):
        if rc != CLC_OK:
            raise CLCError(rc, "%s: %s" % (self.lib.clc_status_string(rc).decode(),
                                           self.lib.clc_last_error_string(self.h).decode()))

    def close(self):
        if getattr(self, "h", None):
            self.lib.clc_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def sync(self):
        self._chk(self.lib.clc_sync(self.h))

    @property
    def stream(self):
        return self.lib.clc_stream(self.h)

    # -- per-kernel event timing
    def profile_enable(self, on=True, only=None):
        """on=True brackets every kernel with HIP events; only=[kernel names] restricts it."""
        v = 1 if on else 0
        if on and only:
            v = 0
            for name in only:
                v |= 1 << (KERNELS.index(name) + 1)
        self._chk(self.lib.clc_profile_enable(self.h, v))

    def profile_reset(self):
        self._chk(self.lib.clc_profile_reset(self.h))

    def profile_read(self):
        """{kernel name: (total device ms, launches)} since the last reset (synchronises)."""
        out = {}
        for k, name in enumerate(KERNELS):
            ms, cnt = C.c_double(), C.c_int()
            self._chk(self.lib.clc_profile_read(self.h, k, C.byref(ms), C.byref(cnt)))
            out[name] = (ms.value, cnt.value)
        return out

    # -- pyramid
    def pyramid_build(self, img):
        img = np.ascontiguousarray(img, dtype=np.uint8)
        self._chk(self.lib.clc_pyramid_build(self.h, _p(img), img.shape[1], img.shape[0]))

    def pyramid_build_dev(self, d_ptr, width, height, pitch, stream=None):
        self._chk(self.lib.clc_pyramid_build_dev(self.h, d_ptr, width, height, pitch, stream))

    def pyramid_level(self, level):
        w, h, p, d = C.c_uint32(), C.c_uint32(), C.c_size_t(), C.c_void_p()
        self._chk(self.lib.clc_pyramid_level(self.h, level, C.byref(w), C.byref(h), C.byref(p), C.byref(d)))
        return w.value, h.value, p.value, d.value

    def pyramid_download(self, level):
        w, h, _, _ = self.pyramid_level(level)
        out = np.zeros((h, w), dtype=np.uint8)
        self._chk(self.lib.clc_pyramid_download(self.h, level, _p(out)))
        return out

    # -- detect (GPU FAST-9 + NMS + orientation)
    def detect(self, capacity=None):
        """Keypoints of the current pyramid in the reference's order; returns (kps, n_found)."""
        cap = int(capacity if capacity is not None else self.dopts.maxkp)
        kps = np.zeros(cap, dtype=KP_DTYPE)
        n, found = C.c_int(), C.c_int()
        self._chk(self.lib.clc_detect(self.h, _p(kps), cap, C.byref(n), C.byref(found)))
        return kps[:n.value], found.value

    def set_keypoint_selection(self, mode):
        """clc_detect_set_selection: SELECT_FIRST (default: the first maxkp keypoints in level-major order) or SELECT_STRONGEST (the
        maxkp highest corner scores, ties by that order, output still in that order) for every later detect call of this context."""
        self._chk(self.lib.clc_detect_set_selection(self.h, int(mode)))

    @property
    def keypoint_selection(self):
        return self.lib.clc_detect_selection(self.h)

    def detect_dev(self, stream=None):
        self._chk(self.lib.clc_detect_dev(self.h, stream))

    def detect_buffers(self):
        k, c, d = C.c_void_p(), C.c_void_p(), C.c_void_p()
        self._chk(self.lib.clc_detect_buffers(self.h, C.byref(k), C.byref(c), C.byref(d)))
        return k.value, c.value, d.value

    def describe_detected_dev(self, d_desc=None, stream=None):
        self._chk(self.lib.clc_describe_detected_dev(self.h, d_desc, stream))

    def detect_and_describe(self, img, capacity=None):
        img = np.ascontiguousarray(img, dtype=np.uint8)
        cap = int(capacity if capacity is not None else self.dopts.maxkp)
        kps = np.zeros(cap, dtype=KP_DTYPE)
        desc = np.zeros((cap, 64), dtype=np.uint8)
        n, found = C.c_int(), C.c_int()
        self._chk(self.lib.clc_detect_and_describe(self.h, _p(img), img.shape[1], img.shape[0], _p(kps), _p(desc), cap,
                                                   C.byref(n), C.byref(found)))
        return kps[:n.value], desc[:n.value], found.value

    def detect_and_describe_published(self, img):
        """The policy classes' front end: clc_detect_and_describe_view (one enqueue sequence, one synchronisation, results in the
        context's pinned block) + clc_detect_store_descriptors (the frame's one copy into the caller's block, published on the way).
        Returns (keypoints, descriptors, found, DescHandle)."""
        img = np.ascontiguousarray(img, dtype=np.uint8)
        pk, pd, n, found = C.c_void_p(), C.c_void_p(), C.c_int(), C.c_int()
        self._chk(self.lib.clc_detect_and_describe_view(self.h, _p(img), img.shape[1], img.shape[0], C.byref(pk), C.byref(pd), C.byref(n), C.byref(found)))
        kps = np.zeros(n.value, dtype=KP_DTYPE)
        if n.value:
            C.memmove(_p(kps), pk, n.value * 20)
        desc = np.zeros((n.value, 64), dtype=np.uint8)
        handle = DescHandle()
        self._chk(self.lib.clc_detect_store_descriptors(self.h, _p(desc) if n.value else None, n.value, C.byref(handle)))
        return kps, desc, found.value, handle

    def detect_batch_dev(self, d_imgs, width, height, pitch, d_kps, d_counts, d_desc=None, stream=None):
        """Frames of several cameras (lists of device pointers): one pyramid launch, two detector launches and (with d_desc) one
        CLATCH launch; d_kps[b] holds maxkp keypoints, d_counts[b] a uint32 pair {written, found}, d_desc[b] maxkp x 64 B."""
        n = len(d_imgs)
        imgs = (C.c_void_p * n)(*d_imgs)
        kps = (C.c_void_p * n)(*d_kps)
        cnt = (C.c_void_p * n)(*d_counts)
        out = (C.c_void_p * n)(*d_desc) if d_desc is not None else None
        self._chk(self.lib.clc_detect_batch_dev(self.h, n, imgs, width, height, pitch, kps, cnt, out, stream))

    def describe_match_pair_dev(self, d_imgs, width, height, pitch, d_kps, counts, d_desc, threshold, d_match, stream=None):
        """clc_describe_match_pair_dev: pyramid + CLATCH of the pair's two cameras and the sweep camera 0 -> camera 1 as one enqueue."""
        imgs = (C.c_void_p * 2)(*d_imgs)
        kps = (C.c_void_p * 2)(*d_kps)
        cnt = (C.c_int * 2)(*[int(c) for c in counts])
        out = (C.c_void_p * 2)(*d_desc)
        self._chk(self.lib.clc_describe_match_pair_dev(self.h, imgs, width, height, pitch, kps, cnt, out, int(threshold), d_match, stream))

    def desc_cache_mode(self, mode):
        """clc_desc_cache_mode: "off" | "verify" (default: sweep at once, whole-block fold behind it, edited blocks uploaded) | "trust"."""
        self._chk(self.lib.clc_desc_cache_mode(self.h, {"off": DESC_CACHE_OFF, "verify": DESC_CACHE_VERIFY, "trust": DESC_CACHE_TRUST}[mode]))

    def desc_cache_publish(self, h_desc, d_src=None):
        """The rows of numpy block h_desc (n x 64) are on this device at d_src: later host-pointer match calls given this very block
        skip its upload.  d_src None: the rows of this context's last describing call -- the frame detect_and_describe(_published)
        staged (h_desc must hold exactly its first n rows, else CLC_ERR_STATE), or what describe / describe_detected_dev(None) /
        describe_dev into the context's own array left there (at most that many rows, else CLC_ERR_BAD_ARG); after a describe into
        caller buffers there is nothing to publish (CLC_ERR_STATE)."""
        assert h_desc.dtype == np.uint8 and h_desc.flags["C_CONTIGUOUS"]
        handle = DescHandle()
        self._chk(self.lib.clc_desc_cache_publish(self.h, d_src, _p(h_desc), int(h_desc.shape[0]), C.byref(handle)))
        return handle

    # -- describe
    def describe(self, kps):
        kps = np.ascontiguousarray(kps, dtype=KP_DTYPE)
        desc = np.zeros((len(kps), 64), dtype=np.uint8)
        self._chk(self.lib.clc_describe(self.h, _p(kps), len(kps), _p(desc)))
        return desc

    def describe_dev(self, d_kps, n, d_desc, stream=None):
        self._chk(self.lib.clc_describe_dev(self.h, d_kps, n, d_desc, stream))

    def describe_batch_dev(self, d_imgs, width, height, pitch, d_kps, counts, d_desc, stream=None):
        """Frames of several cameras (lists of device pointers / counts) in one pyramid + one CLATCH launch."""
        n = len(d_imgs)
        imgs = (C.c_void_p * n)(*d_imgs)
        kps = (C.c_void_p * n)(*d_kps)
        cnt = (C.c_int * n)(*counts)
        out = (C.c_void_p * n)(*d_desc)
        self._chk(self.lib.clc_describe_batch_dev(self.h, n, imgs, width, height, pitch, kps, cnt, out, stream))

    # -- match
    def set_k2nn_formulation(self, name):
        """"matrix" (FP4 matrix pipe, default) or "popcount" (xor + popcount on the vector ALU): same results."""
        self._chk(self.lib.clc_k2nn_set_formulation(self.h, {"matrix": 0, "popcount": 1}[name]))

    @property
    def k2nn_queries_per_block(self):
        return int(self.lib.clc_k2nn_queries_per_block(self.h))

    def k2nn_device_info(self):
        """clc_k2nn_device_info: what the sweep planner knows about the device and where its unequal shares come from (dict)."""
        info = (C.c_int32 * 8)()
        us = (C.c_float * 4)()
        self._chk(self.lib.clc_k2nn_device_info(self.h, info, us))
        d = dict(zip(("xcds", "cus", "default_target_blocks", "bias_a", "bias_b", "bias_source", "kernel_xcds", "target_blocks_env"), [int(v) for v in info]))
        d["bias_source"] = ("default", "CLC_K2NN_BIAS", "probe")[d["bias_source"]]
        d["probe_us"] = dict(zip(("295:264", "311:256", "326:249", "326:233"), [float(v) for v in us]))
        return d

    def k2nn_plan_query(self, nq, nt):
        """clc_k2nn_plan_query: how one nq x nt pair would be cut into sweep workgroups (dict)."""
        info = (C.c_int32 * 8)()
        self._chk(self.lib.clc_k2nn_plan_query(self.h, int(nq), int(nt), info))
        return dict(zip(("qblocks", "splits", "t_per_split", "atomic_merge", "bias_a_tiles", "bias_b_tiles", "queries_per_block", "target_blocks"),
                        [int(v) for v in info]))

    def k2nn_clock_check(self, d_q, nq, d_t, nt, d_match, stream=None):
        """In-kernel shader clock of one (diagnostic, stamped) sweep: (median GHz, min, max, workgroups)."""
        med, lo, hi, n = C.c_double(), C.c_double(), C.c_double(), C.c_int()
        self._chk(self.lib.clc_k2nn_clock_check(self.h, d_q, nq, d_t, nt, d_match, stream, C.byref(med), C.byref(lo), C.byref(hi), C.byref(n)))
        return med.value, lo.value, hi.value, n.value

    def match_2nn(self, Q, T, threshold=40, want_dist=False):
        Q = np.ascontiguousarray(Q, dtype=np.uint8).reshape(-1, 64)
        T = np.ascontiguousarray(T, dtype=np.uint8).reshape(-1, 64)
        m = np.full(Q.shape[0], -2, dtype=np.int32)
        b = np.zeros(Q.shape[0], dtype=np.uint16) if want_dist else None
        s = np.zeros(Q.shape[0], dtype=np.uint16) if want_dist else None
        self._chk(self.lib.clc_match_2nn(self.h, _p(Q), Q.shape[0], _p(T), T.shape[0], int(threshold), _p(m), _p(b), _p(s)))
        return (m, b, s) if want_dist else m

    def match_2nn_dev(self, d_q, nq, d_t, nt, threshold, d_match, stream=None):
        self._chk(self.lib.clc_match_2nn_dev(self.h, d_q, nq, d_t, nt, int(threshold), d_match, stream))

    def match_jobs_dev(self, d_desc_base, jobs, d_match, stream=None):
        arr = (MatchJob * len(jobs))(*[MatchJob(*j) for j in jobs])
        self._chk(self.lib.clc_match_jobs_dev(self.h, d_desc_base, arr, len(jobs), d_match, stream))

    def match_jobs_counted_dev(self, d_desc_base, jobs, d_cnt_q, d_cnt_t, q_row0, d_match, stream=None):
        """clc_match_jobs_counted_dev: jobs planned on capacities, the row counts of both sets read on the device (lists of device
        addresses of int32 counts, one per job); planned query rows past the count are answered -1."""
        n = len(jobs)
        arr = (MatchJob * n)(*[MatchJob(*j) for j in jobs])
        cq = (C.c_void_p * n)(*d_cnt_q)
        ct = (C.c_void_p * n)(*d_cnt_t)
        r0 = (C.c_uint32 * n)(*q_row0)
        self._chk(self.lib.clc_match_jobs_counted_dev(self.h, d_desc_base, arr, n, cq, ct, r0, d_match, stream))

    def match_pairs(self, descs, pairs, threshold=40):
        """All listed (first, second) pairs over per-camera descriptor arrays; returns a list of int32 arrays."""
        descs = [np.ascontiguousarray(d, dtype=np.uint8).reshape(-1, 64) for d in descs]
        counts = (C.c_int * len(descs))(*[d.shape[0] for d in descs])
        dptr = (C.c_void_p * len(descs))(*[d.ctypes.data for d in descs])
        flat = (C.c_int * (2 * len(pairs)))(*[v for p in pairs for v in p])
        outs = [np.full(descs[a].shape[0], -2, dtype=np.int32) for a, _ in pairs]
        optr = (C.c_void_p * len(pairs))(*[o.ctypes.data for o in outs])
        self._chk(self.lib.clc_match_pairs(self.h, dptr, counts, len(descs), flat, len(pairs), int(threshold), optr))
        return outs

    # -- distance-ratio rule (CPUMatcher, include/coloc_hip.h): ratio is CPUMatcher's 0.8 by default
    def match_ratio(self, Q, T, ratio=0.8, want_dist=False):
        """Per query: the train row or -1 under (float)d1 < ratio^2 (float)d2; same outputs as match_2nn."""
        Q = np.ascontiguousarray(Q, dtype=np.uint8).reshape(-1, 64)
        T = np.ascontiguousarray(T, dtype=np.uint8).reshape(-1, 64)
        m = np.full(Q.shape[0], -2, dtype=np.int32)
        b = np.zeros(Q.shape[0], dtype=np.uint16) if want_dist else None
        s = np.zeros(Q.shape[0], dtype=np.uint16) if want_dist else None
        self._chk(self.lib.clc_match_ratio_2nn(self.h, _p(Q), Q.shape[0], _p(T), T.shape[0], float(ratio), _p(m), _p(b), _p(s)))
        return (m, b, s) if want_dist else m

    def match_ratio_dev(self, d_q, nq, d_t, nt, ratio, d_match, stream=None):
        self._chk(self.lib.clc_match_ratio_2nn_dev(self.h, d_q, nq, d_t, nt, float(ratio), d_match, stream))

    def match_ratio_pairs(self, descs, pairs, ratio=0.8, xys=None):
        """CPUMatcher::computeMatchesPair for every listed (first = database, second = queries) pair; xys: per-camera (n, 2) positions
        or None.  Returns a list of (k, 2) int32 arrays of (i_ = database row, j_ = query row)."""
        descs = [np.ascontiguousarray(d, dtype=np.uint8).reshape(-1, 64) for d in descs]
        ncams = len(descs)
        counts = (C.c_int * ncams)(*[d.shape[0] for d in descs])
        dptr = (C.c_void_p * ncams)(*[d.ctypes.data for d in descs])
        xyp = None
        if xys is not None:
            xys = [_xy(x, d.shape[0]) for x, d in zip(xys, descs)]
            xyp = (C.c_void_p * ncams)(*[None if x is None else x.ctypes.data for x in xys])
        flat = (C.c_int * max(2 * len(pairs), 1))(*[v for p in pairs for v in p])
        outs = [np.empty((max(descs[b].shape[0] if 0 <= b < ncams else 0, 1), 2), dtype=np.int32) for _, b in pairs]
        optr = (C.c_void_p * max(len(pairs), 1))(*[o.ctypes.data for o in outs])
        n = (C.c_int * max(len(pairs), 1))()
        self._chk(self.lib.clc_match_ratio_pairs(self.h, dptr, counts, ncams, xyp, flat, len(pairs), float(ratio), optr, n))
        return [o[:n[p]].copy() for p, o in enumerate(outs)]

    def match_map_ratio(self, Q, ratio=0.8, xy_map=None, xy_q=None):
        """CPUMatcher::matchSceneWithMap: the map of set_map is the database; (k, 2) int32 of (i_ = map row, j_ = query row)."""
        Q = np.ascontiguousarray(Q, dtype=np.uint8).reshape(-1, 64)
        xy_map = None if xy_map is None else np.ascontiguousarray(xy_map, dtype=np.float32).reshape(-1, 2)
        xy_q = _xy(xy_q, Q.shape[0])
        out = np.empty((max(Q.shape[0], 1), 2), dtype=np.int32)
        n = C.c_int(0)
        self._chk(self.lib.clc_match_map_ratio(self.h, _p(Q), Q.shape[0], _p(xy_map), _p(xy_q), float(ratio), _p(out), C.byref(n)))
        return out[:n.value].copy()

    def match_map_ratio_dev(self, d_q, nq, ratio, d_match, stream=None):
        self._chk(self.lib.clc_match_map_ratio_dev(self.h, d_q, nq, float(ratio), d_match, stream))

    def set_map(self, desc):
        desc = np.ascontiguousarray(desc, dtype=np.uint8).reshape(-1, 64)
        self._chk(self.lib.clc_set_map(self.h, _p(desc), desc.shape[0]))

    def set_map_points(self, X):
        """clc_set_map_points: (n, 3) float64, row i = the landmark of map descriptor row i; an empty array clears"""
        X = np.ascontiguousarray(X, dtype=np.float64).reshape(-1, 3)
        self._chk(self.lib.clc_set_map_points(self.h, _p(X) if X.shape[0] else None, X.shape[0]))

    def append_map_points(self, X):
        """clc_append_map_points: (n, 3) float64 behind the points of a context that holds only points (no set_map)"""
        X = np.ascontiguousarray(X, dtype=np.float64).reshape(-1, 3)
        self._chk(self.lib.clc_append_map_points(self.h, _p(X) if X.shape[0] else None, X.shape[0]))

    fundamental_from_poses = staticmethod(fundamental_from_poses)

    def extend_map(self, view_a, view_b, band, threshold, max_distance, update_tracks=True, after_stream=None, d_new_q=None, d_new_t=None):
        """clc_map_extend_dev: the untracked guided matches of two posed views triangulated and appended to the context's map.  A view =
        dict(d_desc, n, cam = (focal, ppx, ppy, k1, k2, k3), Rt (12, host), d_kps or d_feat (+ feat_stride), d_count, d_track); device
        pointers as integers.  Returns dict(new_q, new_t, X (n_added, 3), F, map_n_before, n_guided, n_added, n_dropped, status)."""
        j, keep = MapExtend(), []
        out = _extend_fill(j, keep, view_a, view_b, band, threshold, max_distance, update_tracks, after_stream, d_new_q, d_new_t)
        self._chk(self.lib.clc_map_extend_dev(self.h, C.byref(j)))
        return _extend_result(j, *out)

    def extend_map_batch(self, jobs):
        """clc_map_extend_batch_dev: jobs = [dict(view_a, view_b, band, threshold, max_distance [, update_tracks, after_stream, d_new_q,
        d_new_t]), ...], at most MAX_TRACK_PAIRS, in order on the context's stream with one host wait.  Returns a list of result dicts."""
        n, keep = len(jobs), []
        arr = (MapExtend * max(n, 1))()
        outs = [_extend_fill(arr[i], keep, **jobs[i]) for i in range(n)]
        self._chk(self.lib.clc_map_extend_batch_dev(self.h, arr, n))
        return [_extend_result(arr[i], *outs[i]) for i in range(n)]

    def map_observe_dev(self, **view):
        """clc_map_observe_dev: one frame's map match folded into the map rows' observation statistics; enqueue only, no host wait.
        view = n, cam, Rt, width, height, gate [, margin, d_kps | d_feat (+ feat_stride), d_count, d_track, d_counts, after_stream];
        device pointers as integers.  Returns dict(epoch, map_n, status)."""
        j = MapObserve()
        _observe_fill(j, **view)
        self._chk(self.lib.clc_map_observe_dev(self.h, C.byref(j)))
        return dict(epoch=int(j.epoch), map_n=j.map_n, status=j.status)

    def map_observe_batch_dev(self, views):
        """clc_map_observe_batch_dev: views = [dict as map_observe_dev takes, ...], at most MAX_BATCH, ONE epoch, one pair of launches.
        Returns a list of dict(epoch, map_n, status)."""
        n = len(views)
        arr = (MapObserve * max(n, 1))()
        for i in range(n):
            _observe_fill(arr[i], **views[i])
        self._chk(self.lib.clc_map_observe_batch_dev(self.h, arr, n))
        return [dict(epoch=int(arr[i].epoch), map_n=arr[i].map_n, status=arr[i].status) for i in range(n)]

    def map_cull_dev(self, min_visible=8, num=1, den=4, max_idle=0, d_flagged=None, lists=(), after_stream=None, d_remap=None, want_remap=True):
        """clc_map_cull_dev: rows dropped by the rule, the map compacted in order, lists = [(d_track, n), ...] (device pointers as integers)
        remapped in place.  The defaults are the customary rule (CULL_RULE_DEFAULT), UNTUNED.  Returns dict(remap (map_n_before,) int32 or
        None, map_n_before, n_kept, n_dropped, n_flagged, n_ratio, n_idle, status)."""
        j = MapCull()
        j.min_visible, j.num, j.den, j.max_idle, j.d_flagged = int(min_visible), int(num), int(den), int(max_idle), d_flagged
        j.n_lists = len(lists)
        for i, (d, n) in enumerate(lists[:MAX_BATCH]):
            j.d_track[i], j.track_n[i] = d, int(n)
        j.after_stream, j.d_remap = after_stream, d_remap
        remap = np.full(max(int(self.mopts.maxkp), 1), -7, dtype=np.int32) if want_remap else None      # (a map never has more rows)
        j.h_remap = _p(remap)
        self._chk(self.lib.clc_map_cull_dev(self.h, C.byref(j)))
        return dict(remap=None if remap is None else remap[:j.map_n_before].copy(), map_n_before=j.map_n_before, n_kept=j.n_kept,
                    n_dropped=j.n_dropped, n_flagged=j.n_flagged, n_ratio=j.n_ratio, n_idle=j.n_idle, status=j.status)

    def map_stats(self, counters=True):
        """clc_map_stats_get: dict(visible, found, last_view ((rows,) uint32 each; counters=False: left out), epoch, rows); covers new
        rows first and synchronises the context's stream"""
        epoch, rows = C.c_uint32(0), C.c_int(0)
        self._chk(self.lib.clc_map_stats_get(self.h, None, None, None, C.byref(epoch), C.byref(rows)))
        out = dict(epoch=int(epoch.value), rows=int(rows.value))
        if counters:
            arrs = [np.zeros(max(out["rows"], 1), dtype=np.uint32) for _ in range(3)]
            self._chk(self.lib.clc_map_stats_get(self.h, _p(arrs[0]), _p(arrs[1]), _p(arrs[2]), None, None))
            out.update(visible=arrs[0][:out["rows"]], found=arrs[1][:out["rows"]], last_view=arrs[2][:out["rows"]])
        return out

    def cull_map_points(self, remap):
        """clc_cull_map_points: the points of a context that holds only points compacted by a host remap (one entry per point)"""
        remap = np.ascontiguousarray(remap, dtype=np.int32).reshape(-1)
        self._chk(self.lib.clc_cull_map_points(self.h, _p(remap) if len(remap) else None, len(remap)))

    def tracks_build_dev(self, rows, pairs, d_track_feat, d_n_tracks, stream=None):
        """clc_tracks_build_dev: the multi-view tracks alone, enqueue only.  rows = row capacity per camera; pairs = [dict(cam_a=, cam_b=,
        d_q=, d_t=, n= [, d_n, d_index, n_list]), ...] (device pointers as integers); d_track_feat: int32 [tracks_capacity(rows, pairs)]
        [len(rows)], d_n_tracks: one int32"""
        t = TracksJob()
        keep = []
        _tracks_fill(t, keep, rows, pairs)
        self._chk(self.lib.clc_tracks_build_dev(self.h, C.byref(t), d_track_feat, d_n_tracks, stream))

    def map_build_dev(self, rows, pairs, cams, seed_pair, Rt_seed_a, Rt_seed_b, after_stream=None):
        """clc_map_build_dev: tracks + the seed pair's triangulation, installed as this context's map (the state of set_map +
        set_map_points).  cams = [dict(cam=(focal, ppx, ppy, k1, k2, k3), d_kps= | d_feat= [, feat_stride], d_desc=), ...] per camera;
        Rt_seed_a / Rt_seed_b: [R|t] of the seed pair's two cameras (seed_poses).  Returns a dict: n_tracks, track_feat, map_n, map_track,
        map_row, X."""
        return self._map_build("clc_map_build_dev", rows, pairs, cams, seed_pair, Rt_seed_a, Rt_seed_b, after_stream)

    def _map_build(self, entry, rows, pairs, cams, seed_pair, Rt_seed_a, Rt_seed_b, after_stream, **steps):
        """what the three clc_map_build*_dev wrappers share: the map job, the steps' structs (_steps_fill's grow and ba), the call, the results"""
        j = MapJob()
        keep = []
        out = _map_fill(j, keep, rows, pairs, cams, seed_pair=seed_pair, Rt_seed_a=Rt_seed_a, Rt_seed_b=Rt_seed_b, after_stream=after_stream)
        filled = _steps_fill(keep, rows, self, **steps)
        self._chk(getattr(self.lib, entry)(self.h, C.byref(j), *[C.byref(s) for _, s, _ in filled]))
        return _steps_result(_map_result(j, *out), j, len(rows), filled)

    def map_build_grow_dev(self, rows, pairs, cams, seed_pair, Rt_seed_a, Rt_seed_b, after_stream=None, max_iteration=256, seed=0,
                           precision=float("inf")):
        """clc_map_build_grow_dev: map_build_dev, then every other camera resected against the map (the a-contrario solve of
        pnp_acransac with seed + k for the k-th of them) and its tracks added; the grown map is installed.  Every camera needs d_desc.
        Returns map_build_dev's dict for the GROWN map with a "grow" dict: resected, status, n_corr, n_inliers, error_max, Rt per
        camera, n_seed_rows, n_added, map_cam, map_obs."""
        return self._map_build("clc_map_build_grow_dev", rows, pairs, cams, seed_pair, Rt_seed_a, Rt_seed_b, after_stream,
                               grow=(max_iteration, seed, precision))

    def map_build_grow_ba_dev(self, rows, pairs, cams, seed_pair, Rt_seed_a, Rt_seed_b, after_stream=None, max_iteration=256, seed=0,
                              precision=float("inf"), ba_max_iterations=0, huber_a=0.0, function_tolerance=0.0):
        """clc_map_build_grow_ba_dev: map_build_grow_dev with the grown map -- the valid cameras' poses and every landmark -- bundle-adjusted
        before it is installed.  Returns map_build_grow_dev's dict (X, Rt_seed_* and grow["Rt"] refined) with a "ba" dict: status,
        iterations, n_cams, n_points, n_obs, cost_initial, cost_final, rmse."""
        return self._map_build("clc_map_build_grow_ba_dev", rows, pairs, cams, seed_pair, Rt_seed_a, Rt_seed_b, after_stream,
                               grow=(max_iteration, seed, precision), ba=(ba_max_iterations, huber_a, function_tolerance))

    def ba_dev(self, cams, cam_mask, Rt, n_points, d_X, d_obs, d_x, after_stream=None, max_iterations=0, huber_a=0.0, function_tolerance=0.0):
        """clc_ba_dev: the bundle adjustment alone on arrays in device memory (pointers as integers): cams = [(focal, ppx, ppy, k1, k2,
        k3), ...], Rt (n_cams, 3, 4), d_X n_points x 3 float64 (rewritten), d_obs n_points uint32 masks, d_x n_points x n_cams x 2 float64.
        Returns a dict: clc_map_ba's out fields and Rt (n_cams, 3, 4), refined for the cameras of cam_mask."""
        j = BaJob()
        n = len(cams)
        j.n_cams, j.cam_mask, j.n_points = n, int(cam_mask), int(n_points)
        Rt = np.asarray(Rt, dtype=np.float64).reshape(n, 12)
        for c in range(min(n, MAX_BATCH)):
            j.cam[c] = CameraK3(*[float(v) for v in cams[c]])
            j.Rt[c][:] = [float(v) for v in Rt[c]]
        j.d_X, j.d_obs, j.d_x, j.after_stream = d_X, d_obs, d_x, after_stream
        _ba_fill(j.ba, max_iterations, huber_a, function_tolerance)
        self._chk(self.lib.clc_ba_dev(self.h, C.byref(j)))
        res = _ba_result(j.ba)
        res["Rt"] = np.array([list(j.Rt[c]) for c in range(min(n, MAX_BATCH))]).reshape(-1, 3, 4)
        return res

    def map_resect_build_dev(self, rows, cams, camera, d_X, d_x, d_track, d_row, d_n, stream=None):
        """clc_map_resect_build_dev: the resection list of `camera` on the per-track state of this context's last grown build, enqueue
        only; rows / cams as map_build_dev (the camera's row capacity and 2-D side are read); outputs are device pointers with room
        for rows[camera] entries (d_track / d_row nullable), d_n one int32"""
        j = MapJob()
        keep = []
        _map_fill(j, keep, rows, [], cams, outputs=False)
        self._chk(self.lib.clc_map_resect_build_dev(self.h, C.byref(j), int(camera), d_X, d_x, d_track, d_row, d_n, stream))

    def map_align_dev(self, d_desc, d_X, n_new, d_rows=None, threshold=0, install=True, after_stream=None, want_match=True, want_X=True):
        """clc_map_align_dev: a new map in device memory (row i = row d_rows[i] of d_desc, landmark d_X[i]) brought to the scale of the
        map this context holds and, with install, put in its place.  Returns a dict: scale, n_old, n_common, n_terms, status, match (new
        row of every old row, or -1), X (the rescaled points)."""
        a = MapAlign()
        a.d_desc, a.d_rows, a.d_X, a.n_new, a.threshold, a.install, a.after_stream = d_desc, d_rows, d_X, int(n_new), int(threshold), int(bool(install)), after_stream
        match = np.full(max(int(self.mopts.maxkp), 1), -2, dtype=np.int32) if want_match else None
        X = np.zeros((max(int(n_new), 1), 3)) if want_X else None
        a.match, a.X = (None if match is None else match.ctypes.data), (None if X is None else X.ctypes.data)
        self._chk(self.lib.clc_map_align_dev(self.h, C.byref(a)))
        return _align_result(a, match, X)

    def map_align_sim_dev(self, d_desc, d_X, n_new, d_rows=None, threshold=0, install=True, after_stream=None, apply=SIM_APPLY_SCALE,
                          max_iteration=0, seed=1, precision=float("inf"), want_match=True, want_X=True):
        """clc_map_align_sim_dev: clc_map_align_dev's step under the a-contrario similarity NEW -> OLD over the common features.  Returns a
        dict: s, R, t, n_old, n_common, n_inliers, inlier (flags per common feature), iterations, refit, status, error_max, min_nfa,
        match, X (the transformed points)."""
        a = MapAlignSim()
        a.d_desc, a.d_rows, a.d_X, a.n_new, a.install, a.after_stream = d_desc, d_rows, d_X, int(n_new), int(bool(install)), after_stream
        match, inlier = _sim_fill(a, self.mopts.maxkp, threshold, apply, max_iteration, seed, precision, want_match)
        X = np.zeros((max(int(n_new), 1), 3)) if want_X else None
        a.X = None if X is None else X.ctypes.data
        self._chk(self.lib.clc_map_align_sim_dev(self.h, C.byref(a)))
        return _sim_result(a, match, inlier, X)

    def track_build_dev(self, d_X, d_x, d_query, d_map, d_n, stream=None, **job):
        """clc_track_build_dev: the track kernel alone, enqueue only; job keywords as track_localize_dev (d_match, nq, cam, d_kps | d_feat,
        feat_stride, d_count); outputs are device pointers with room for nq tracks"""
        j = TrackJob()
        _track_fill(j, None, outputs=False, **job)
        self._chk(self.lib.clc_track_build_dev(self.h, C.byref(j), d_X, d_x, d_query, d_map, d_n, stream))

    def track_localize_dev(self, **job):
        """clc_track_localize_dev: setupTracks + localizeImage from device memory.  Keywords: d_match, nq, cam = (focal, ppx, ppy, k1, k2, k3),
        d_kps or d_feat (+ feat_stride), d_count, after_stream, max_iteration, seed, precision, refine, huber_a.  Returns a dict: Rt, cov,
        n_tracks, track_query, track_map, inliers (into the track list), mask, error_max, rmse, iterations."""
        j = TrackJob()
        keep = []
        out = _track_fill(j, keep, **job)
        self._chk(self.lib.clc_track_localize_dev(self.h, C.byref(j)))
        return _track_result(j, *out)

    def track_prior_dev(self, **job):
        """clc_track_prior_dev: the tracks of the frame, then the pose from the PREDICTED pose without a minimal sample.  Keywords: d_match,
        nq, cam = (focal, ppx, ppy, k1, k2, k3), d_kps or d_feat (+ feat_stride), d_count, after_stream, Rt_prior (3, 4), gate (pixels: the
        error_max of the camera's last a-contrario solve), huber_a, rounds, max_iter, min_inliers.  Returns a dict: Rt, cov, n_tracks,
        track_query, track_map, mask, n_inliers, iterations, rounds_run, converged, result (TRACK_PRIOR_OK / TRACK_PRIOR_FEW: run
        match_map_dev + track_localize_dev for the frame), rmse."""
        j = TrackPriorJob()
        keep = []
        out = _track_prior_fill(j, keep, **job)
        self._chk(self.lib.clc_track_prior_dev(self.h, C.byref(j)))
        return _track_prior_result(j, *out)

    def pnp_refine_prior(self, X, x, K, Rt_prior, gate, huber_a=16.0, rounds=0, max_iter=0, min_inliers=0):
        """clc_pnp_refine_prior: the same solve on host arrays.  Returns a dict: Rt (3, 4), cov (6, 6), mask, n_inliers, rmse, iterations,
        rounds_run, converged, result."""
        X = np.ascontiguousarray(X, dtype=np.float64).reshape(-1, 3)
        x = np.ascontiguousarray(x, dtype=np.float64).reshape(-1, 2)
        K = np.ascontiguousarray(K, dtype=np.float64).reshape(9)
        Rt0 = np.ascontiguousarray(Rt_prior, dtype=np.float64).reshape(12)
        n = X.shape[0]
        Rt, cov, mask = np.zeros(12), np.zeros(36), np.zeros(max(n, 1), dtype=np.uint8)
        ni, it, rr, cv, res = (C.c_int() for _ in range(5))
        rmse = C.c_double()
        self._chk(self.lib.clc_pnp_refine_prior(self.h, _p(X) if n else None, _p(x) if n else None, n, _p(K), _p(Rt0), float(gate), float(huber_a),
                                                int(rounds), int(max_iter), int(min_inliers), _p(Rt), _p(cov), _p(mask), C.addressof(ni),
                                                C.addressof(rmse), C.addressof(it), C.addressof(rr), C.addressof(cv), C.addressof(res)))
        return dict(Rt=Rt.reshape(3, 4), cov=cov.reshape(6, 6), mask=mask[:n].astype(bool), n_inliers=ni.value, rmse=rmse.value,
                    iterations=it.value, rounds_run=rr.value, converged=cv.value, result=res.value)

    def pair_build_dev(self, d_x1, d_x2, d_pair_q, d_pair_t, d_n, stream=None, **job):
        """clc_pair_build_dev: the pair kernel alone, enqueue only; job keywords as pair_filter_dev (d_match, nq, nt, cam_a, cam_b,
        d_kps_* | d_feat_*, feat_stride_*, d_count_*); outputs are device pointers with room for nq pairs"""
        j = PairJob()
        _pair_fill(j, None, outputs=False, **job)
        self._chk(self.lib.clc_pair_build_dev(self.h, C.byref(j), d_x1, d_x2, d_pair_q, d_pair_t, d_n, stream))

    def match_guided_dev(self, stream=None, **job):
        """clc_match_guided_dev: K2NN over the train rows within `band` pixels of the query's epipolar line under F, enqueue only.
        Keywords: d_q, nq, d_t, nt, cam_a / cam_b = (focal, ppx, ppy, k1, k2, k3), d_kps_a or d_feat_a (+ feat_stride_a), the same for b,
        d_count_a, d_count_b, F (9, pixels, x_b^T F x_a = 0), band, threshold, d_match and the nullable d_best, d_second, d_line, d_tpos."""
        j = GuidedJob()
        _guided_fill(j, **job)
        self._chk(self.lib.clc_match_guided_dev(self.h, C.byref(j), stream))

    def match_guided_batch_dev(self, jobs, stream=None):
        """clc_match_guided_batch_dev: jobs = [dict(the keywords of match_guided_dev), ...], at most MAX_TRACK_PAIRS, one sweep launch."""
        n = len(jobs)
        arr = (GuidedJob * max(n, 1))()
        for i in range(n):
            _guided_fill(arr[i], **jobs[i])
        self._chk(self.lib.clc_match_guided_batch_dev(self.h, arr, n, stream))

    def match_map_guided_dev(self, stream=None, **job):
        """clc_match_map_guided_dev: K2NN over the map rows whose landmark projects within `radius` pixels of the query under the predicted
        pose, enqueue only.  Keywords: d_q, nq, cam = (focal, ppx, ppy, k1, k2, k3), d_kps or d_feat (+ feat_stride), d_count, Rt (12, the
        predicted [R|t], world to camera), radius, threshold, d_match and the nullable d_best, d_second, d_qpos, d_proj."""
        j = MapGuidedJob()
        _map_guided_fill(j, **job)
        self._chk(self.lib.clc_match_map_guided_dev(self.h, C.byref(j), stream))

    def match_map_guided_batch_dev(self, jobs, stream=None):
        """clc_match_map_guided_batch_dev: jobs = [dict(the keywords of match_map_guided_dev), ...], at most MAX_BATCH (the cameras of one
        frame against the context's map), one prep and one sweep launch."""
        n = len(jobs)
        arr = (MapGuidedJob * max(n, 1))()
        for i in range(n):
            _map_guided_fill(arr[i], **jobs[i])
        self._chk(self.lib.clc_match_map_guided_batch_dev(self.h, arr, n, stream))

    def match_map_binned_dev(self, stream=None, **job):
        """clc_match_map_binned_dev: match_map_guided_dev's job, outputs and bits through a cell grid of the projections instead of the
        whole-map sweep (map_binned_plan tells which of the two a job runs), enqueue only.  The keywords of match_map_guided_dev."""
        j = MapGuidedJob()
        _map_guided_fill(j, **job)
        self._chk(self.lib.clc_match_map_binned_dev(self.h, C.byref(j), stream))

    def match_map_binned_batch_dev(self, jobs, stream=None):
        """clc_match_map_binned_batch_dev: jobs = [dict(the keywords of match_map_guided_dev), ...], at most MAX_BATCH; the BINNED jobs
        share one prep, one bin and one match launch, the SWEEP jobs go through the guided path together."""
        n = len(jobs)
        arr = (MapGuidedJob * max(n, 1))()
        for i in range(n):
            _map_guided_fill(arr[i], **jobs[i])
        self._chk(self.lib.clc_match_map_binned_batch_dev(self.h, arr, n, stream))

    def map_bin_build_dev(self, d_cell_start, d_cell_row, stream=None, **job):
        """clc_map_bin_build_dev: the prep and bin launches of match_map_binned_dev alone, the table copied out: d_cell_start (4357 int32,
        device), d_cell_row (map_n int32, device: the map rows in cell order).  The keywords of match_map_guided_dev."""
        j = MapGuidedJob()
        _map_guided_fill(j, **job)
        self._chk(self.lib.clc_map_bin_build_dev(self.h, C.byref(j), d_cell_start, d_cell_row, stream))

    def map_binned_plan(self, cam, radius):
        """clc_map_binned_plan: dict(plan = BIN_PLAN_SWEEP | BIN_PLAN_BINNED, cells_per_axis, lanes_per_query, cell_side) of
        match_map_binned_dev for cam = (focal, ppx, ppy, k1, k2, k3) and `radius` on this context's map."""
        info = (C.c_int32 * 4)()
        side = C.c_double(0.0)
        c = CameraK3(*[float(v) for v in cam])
        self._chk(self.lib.clc_map_binned_plan(self.h, C.byref(c), C.c_float(radius), info, C.byref(side)))
        return dict(plan=info[0], cells_per_axis=info[1], lanes_per_query=info[2], cell_side=side.value)

    def match_unique_dev(self, d_match, d_best, nq, nt, d_owner=None, stream=None):
        """clc_match_unique_dev: d_match (nq int32, device) made one-to-one IN PLACE from the distances d_best (nq uint16, device) the
        producer wrote beside it -- every train row below nt keeps the claimant with the smallest (distance, query row); d_owner (nullable,
        nt int32, device) receives the inverse list.  Enqueue only."""
        j = UniqueJob(d_match, d_best, int(nq), int(nt), d_owner)
        self._chk(self.lib.clc_match_unique_dev(self.h, C.byref(j), stream))

    def match_unique_batch_dev(self, jobs, stream=None):
        """clc_match_unique_batch_dev: jobs = [dict(d_match, d_best, nq, nt, d_owner=None), ...], at most MAX_TRACK_PAIRS, the same three
        enqueued operations as one call."""
        n = len(jobs)
        arr = (UniqueJob * max(n, 1))()
        for i in range(n):
            jb = jobs[i]
            arr[i] = UniqueJob(jb["d_match"], jb["d_best"], int(jb["nq"]), int(jb["nt"]), jb.get("d_owner"))
        self._chk(self.lib.clc_match_unique_batch_dev(self.h, arr, n, stream))

    def match_2nn_unique_dev(self, d_q, nq, d_t, nt, threshold, d_match, d_owner=None, stream=None):
        """clc_match_2nn_unique_dev: match_2nn_dev and then the one-to-one filter on the same stream."""
        self._chk(self.lib.clc_match_2nn_unique_dev(self.h, d_q, nq, d_t, nt, int(threshold), d_match, d_owner, stream))

    def match_map_unique_dev(self, d_q, nq, threshold, d_match, d_owner=None, stream=None):
        """clc_match_map_unique_dev: match_map_dev and then the one-to-one filter; d_owner: one entry per map row."""
        self._chk(self.lib.clc_match_map_unique_dev(self.h, d_q, nq, int(threshold), d_match, d_owner, stream))

    def match_map_binned_unique_dev(self, d_owner=None, stream=None, **job):
        """clc_match_map_binned_unique_dev: match_map_binned_dev (the keywords of match_map_guided_dev; d_best may be left out) and then
        the one-to-one filter; d_owner: one entry per map row."""
        j = MapGuidedJob()
        _map_guided_fill(j, **job)
        self._chk(self.lib.clc_match_map_binned_unique_dev(self.h, C.byref(j), d_owner, stream))

    def match_unique(self, Q, T, threshold=40):
        """clc_match_2nn_unique on host arrays: (match, owner) -- match_2nn's list made one-to-one, and for every row of T the query that
        keeps it or -1."""
        Q = np.ascontiguousarray(Q, dtype=np.uint8).reshape(-1, 64)
        T = np.ascontiguousarray(T, dtype=np.uint8).reshape(-1, 64)
        m = np.full(Q.shape[0], -2, dtype=np.int32)
        o = np.full(T.shape[0], -2, dtype=np.int32)
        self._chk(self.lib.clc_match_2nn_unique(self.h, _p(Q), Q.shape[0], _p(T), T.shape[0], int(threshold), _p(m), _p(o)))
        return m, o

    def pair_filter_dev(self, model, **job):
        """clc_pair_filter_dev: computeRelativePose's gather + the a-contrario filter of model 'E' | 'F' | 'H' from device memory.  Keywords:
        d_match, nq, nt, cam_a / cam_b = (focal, ppx, ppy, k1, k2, k3), d_kps_a or d_feat_a (+ feat_stride_a), the same for b, d_count_a,
        d_count_b, after_stream, img_wh, max_iteration, seed, precision.  Returns a dict: M (E, F or H in pixels), F, n_pairs, pair_q, pair_t,
        x1, x2 (undistorted pixels), inliers (into the pair list), mask, error_max, min_nfa, iterations."""
        j = PairJob()
        keep = []
        out = _pair_fill(j, keep, **job)
        self._chk(self.lib.clc_pair_filter_dev(self.h, ord(model), C.byref(j)))
        return _pair_result(j, *out)

    def inter_pose_dev(self, **job):
        """clc_inter_pose_dev: the inter-camera step (pair gather, 'E' filter, temporary map, scale, first pose, refinement) from device
        memory.  Keywords: Rt_source, huber_a, EITHER d_map_match_a (the shortcut) OR d_first_desc + d_map_desc [+ lower_is_b,
        match_threshold] (the reference's chain), and the pair's keywords of pair_filter_dev.  The map points are this context's
        (set_map_points).  Returns a dict shaped like inter_pose_batch's."""
        j = InterDevJob()
        keep = []
        out = _inter_dev_fill(j, keep, **job)
        self._chk(self.lib.clc_inter_pose_dev(self.h, C.byref(j)))
        return _inter_dev_result(j, *out)

    def inter_front_dev(self, d_x1, d_x2, n, d_inliers, n_inliers, cam_a, cam_b, motions, d_Xt, d_x2f, d_corr, d_record, d_rows=None,
                        d_first=None, stream=None):
        """clc_inter_front_dev: the chirality vote + temporary map kernel alone, enqueue only; motions = four [R|t] (4 x 3 x 4, host);
        outputs are device pointers with room for n_inliers points, d_record four int32 {n_front, chosen, stage, 1}"""
        ca, cb = CameraK3(*[float(v) for v in cam_a]), CameraK3(*[float(v) for v in cam_b])
        mo = np.ascontiguousarray(motions, dtype=np.float64).reshape(48)
        self._chk(self.lib.clc_inter_front_dev(self.h, d_x1, d_x2, int(n), d_inliers, int(n_inliers), C.byref(ca), C.byref(cb), _p(mo), d_rows,
                                               d_Xt, d_x2f, d_corr, d_first, d_record, stream))

    def match_map_dev(self, d_q, nq, threshold, d_match, stream=None):
        self._chk(self.lib.clc_match_map_dev(self.h, d_q, nq, int(threshold), d_match, stream))

    def match_map(self, Q, threshold=60):
        Q = np.ascontiguousarray(Q, dtype=np.uint8).reshape(-1, 64)
        m = np.full(Q.shape[0], -2, dtype=np.int32)
        self._chk(self.lib.clc_match_map(self.h, _p(Q), Q.shape[0], int(threshold), _p(m)))
        return m

    # -- pnp
    def pnp_residuals(self, Rt, X, x, K):
        Rt = np.ascontiguousarray(Rt, dtype=np.float64).reshape(-1, 12)
        X = np.ascontiguousarray(X, dtype=np.float64).reshape(-1, 3)
        x = np.ascontiguousarray(x, dtype=np.float64).reshape(-1, 2)
        K = np.ascontiguousarray(K, dtype=np.float64).reshape(9)
        err = np.zeros((Rt.shape[0], X.shape[0]), dtype=np.float64)
        self._chk(self.lib.clc_pnp_residuals(self.h, _p(Rt), Rt.shape[0], _p(X), _p(x), X.shape[0], _p(K), _p(err)))
        return err

    def pnp_ransac(self, X, x, K, samples=None, n_samples=256, seed=1, thr2=16.0):
        """Robust pose: (Rt (3,4) or None, inlier mask, cost)."""
        X = np.ascontiguousarray(X, dtype=np.float64).reshape(-1, 3)
        x = np.ascontiguousarray(x, dtype=np.float64).reshape(-1, 2)
        K = np.ascontiguousarray(K, dtype=np.float64).reshape(9)
        if samples is not None:
            samples = np.ascontiguousarray(samples, dtype=np.int32).reshape(-1, 3)
            n_samples = samples.shape[0]
        Rt = np.zeros(12, dtype=np.float64)
        mask = np.zeros(X.shape[0], dtype=np.uint8)
        n, cost = C.c_int(), C.c_double()
        self._chk(self.lib.clc_pnp_ransac(self.h, _p(X), _p(x), X.shape[0], _p(K), _p(samples), int(n_samples), int(seed),
                                          float(thr2), _p(Rt), _p(mask), C.byref(n), C.byref(cost)))
        return (Rt.reshape(3, 4) if n.value > 0 else None), mask.astype(bool), cost.value

    def essential_ransac(self, x1, x2, K1, K2, samples=None, n_samples=256, seed=1, thr2=4.0):
        """Five-point RANSAC: (E (3,3) or None, F (3,3), inlier mask)."""
        x1 = np.ascontiguousarray(x1, dtype=np.float64).reshape(-1, 2)
        x2 = np.ascontiguousarray(x2, dtype=np.float64).reshape(-1, 2)
        K1 = np.ascontiguousarray(K1, dtype=np.float64).reshape(9); K2 = np.ascontiguousarray(K2, dtype=np.float64).reshape(9)
        if samples is not None:
            samples = np.ascontiguousarray(samples, dtype=np.int32).reshape(-1, 5)
            n_samples = samples.shape[0]
        E = np.zeros(9); F = np.zeros(9)
        mask = np.zeros(x1.shape[0], dtype=np.uint8)
        n = C.c_int()
        self._chk(self.lib.clc_essential_ransac(self.h, _p(x1), _p(x2), x1.shape[0], _p(K1), _p(K2), _p(samples), int(n_samples),
                                                int(seed), float(thr2), _p(E), _p(F), _p(mask), C.byref(n)))
        return (E.reshape(3, 3) if n.value > 0 else None), F.reshape(3, 3), mask.astype(bool)

    def essential_fivepoint(self, x1, x2, K1, K2, samples):
        x1 = np.ascontiguousarray(x1, dtype=np.float64).reshape(-1, 2)
        x2 = np.ascontiguousarray(x2, dtype=np.float64).reshape(-1, 2)
        K1 = np.ascontiguousarray(K1, dtype=np.float64).reshape(9); K2 = np.ascontiguousarray(K2, dtype=np.float64).reshape(9)
        samples = np.ascontiguousarray(samples, dtype=np.int32).reshape(-1, 5)
        out = np.zeros((samples.shape[0], 10, 9), dtype=np.float64)
        self._chk(self.lib.clc_essential_fivepoint(self.h, _p(x1), _p(x2), x1.shape[0], _p(K1), _p(K2), _p(samples),
                                                   samples.shape[0], _p(out)))
        return out

    def epipolar_residuals(self, F, x1, x2):
        F = np.ascontiguousarray(F, dtype=np.float64).reshape(-1, 9)
        x1 = np.ascontiguousarray(x1, dtype=np.float64).reshape(-1, 2)
        x2 = np.ascontiguousarray(x2, dtype=np.float64).reshape(-1, 2)
        err = np.zeros((F.shape[0], x1.shape[0]), dtype=np.float64)
        self._chk(self.lib.clc_epipolar_residuals(self.h, _p(F), F.shape[0], _p(x1), _p(x2), x1.shape[0], _p(err)))
        return err

    def epipolar_score(self, F, x1, x2, thr2):
        F = np.ascontiguousarray(F, dtype=np.float64).reshape(-1, 9)
        x1 = np.ascontiguousarray(x1, dtype=np.float64).reshape(-1, 2)
        x2 = np.ascontiguousarray(x2, dtype=np.float64).reshape(-1, 2)
        cnt = np.zeros(F.shape[0], dtype=np.int32); cost = np.zeros(F.shape[0], dtype=np.float64)
        self._chk(self.lib.clc_epipolar_score(self.h, _p(F), F.shape[0], _p(x1), _p(x2), x1.shape[0], float(thr2), _p(cnt), _p(cost)))
        return cnt, cost

    def pnp_localize(self, X, x, K, samples=None, n_samples=256, seed=1, thr2=16.0, huber_a=16.0):
        """ransac + refine in one submission: (Rt (3,4) or None, cov (6,6), inlier mask, rmse)."""
        X = np.ascontiguousarray(X, dtype=np.float64).reshape(-1, 3)
        x = np.ascontiguousarray(x, dtype=np.float64).reshape(-1, 2)
        K = np.ascontiguousarray(K, dtype=np.float64).reshape(9)
        if samples is not None:
            samples = np.ascontiguousarray(samples, dtype=np.int32).reshape(-1, 3)
            n_samples = samples.shape[0]
        Rt = np.zeros(12); cov = np.zeros(36)
        mask = np.zeros(X.shape[0], dtype=np.uint8)
        n, rmse = C.c_int(), C.c_double()
        self._chk(self.lib.clc_pnp_localize(self.h, _p(X), _p(x), X.shape[0], _p(K), _p(samples), int(n_samples), int(seed),
                                            float(thr2), float(huber_a), _p(Rt), _p(cov), _p(mask), C.byref(n), C.byref(rmse)))
        return (Rt.reshape(3, 4) if n.value > 0 else None), cov.reshape(6, 6), mask.astype(bool), rmse.value

    def pnp_acransac(self, X, x, K, max_iteration=256, seed=1, precision=float("inf"), refine=False, huber_a=16.0):
        """A-contrario RANSAC pose (what the reference runs).  Returns a dict: Rt (3,4) or None, mask, inliers (ascending
        residual order), error_max (pixels), min_nfa, iterations [, cov, rmse with refine=True]."""
        X = np.ascontiguousarray(X, dtype=np.float64).reshape(-1, 3)
        x = np.ascontiguousarray(x, dtype=np.float64).reshape(-1, 2)
        K = np.ascontiguousarray(K, dtype=np.float64).reshape(9)
        n = X.shape[0]
        Rt = np.zeros(12); mask = np.zeros(max(n, 1), dtype=np.uint8); inl = np.zeros(max(n, 1), dtype=np.int32)
        ni, its = C.c_int(), C.c_int()
        emax, nfa, rmse = C.c_double(), C.c_double(), C.c_double()
        out = {}
        if refine:
            cov = np.zeros(36)
            self._chk(self.lib.clc_pnp_localize_ac(self.h, _p(X), _p(x), n, _p(K), int(max_iteration), int(seed), float(precision),
                                                   float(huber_a), _p(Rt), _p(cov), _p(mask), _p(inl), C.byref(ni), C.byref(emax),
                                                   C.byref(rmse)))
            out.update(cov=cov.reshape(6, 6), rmse=rmse.value)
        else:
            self._chk(self.lib.clc_pnp_acransac(self.h, _p(X), _p(x), n, _p(K), int(max_iteration), int(seed), float(precision),
                                                _p(Rt), _p(mask), _p(inl), C.byref(ni), C.byref(emax), C.byref(nfa), C.byref(its)))
            out.update(min_nfa=nfa.value, iterations=its.value)
        out.update(Rt=Rt.reshape(3, 4) if ni.value > 0 else None, mask=mask[:n].astype(bool), inliers=inl[:ni.value].copy(),
                   error_max=emax.value)
        return out

    def essential_acransac(self, x1, x2, K1, K2, img_wh, max_iteration=256, seed=1, precision=float("inf")):
        """A-contrario five-point RANSAC (RobustMatcher::filterEssential).  Returns a dict: E, F (3,3) or None, mask, inliers, ..."""
        x1 = np.ascontiguousarray(x1, dtype=np.float64).reshape(-1, 2)
        x2 = np.ascontiguousarray(x2, dtype=np.float64).reshape(-1, 2)
        K1 = np.ascontiguousarray(K1, dtype=np.float64).reshape(9); K2 = np.ascontiguousarray(K2, dtype=np.float64).reshape(9)
        n = x1.shape[0]
        E = np.zeros(9); F = np.zeros(9)
        mask = np.zeros(max(n, 1), dtype=np.uint8); inl = np.zeros(max(n, 1), dtype=np.int32)
        ni, its = C.c_int(), C.c_int()
        emax, nfa = C.c_double(), C.c_double()
        self._chk(self.lib.clc_essential_acransac(self.h, _p(x1), _p(x2), n, _p(K1), _p(K2), int(img_wh[0]), int(img_wh[1]),
                                                  int(max_iteration), int(seed), float(precision), _p(E), _p(F), _p(mask), _p(inl),
                                                  C.byref(ni), C.byref(emax), C.byref(nfa), C.byref(its)))
        ok = ni.value > 0
        return dict(E=E.reshape(3, 3) if ok else None, F=F.reshape(3, 3) if ok else None, mask=mask[:n].astype(bool),
                    inliers=inl[:ni.value].copy(), error_max=emax.value, min_nfa=nfa.value, iterations=its.value)

    def two_view_acransac(self, model, x1, x2, img_wh, K1=None, K2=None, max_iteration=256, seed=1, precision=float("inf")):
        """clc_two_view_acransac: the a-contrario filter under model 'E' (five points; K1, K2 needed), 'F' (seven points) or 'H' (four points).
        Returns a dict: M (3,3: E, F or H in pixels) or None, F (3,3; zeros for 'H') or None, mask, inliers, error_max, min_nfa, iterations."""
        x1 = np.ascontiguousarray(x1, dtype=np.float64).reshape(-1, 2)
        x2 = np.ascontiguousarray(x2, dtype=np.float64).reshape(-1, 2)
        K1 = None if K1 is None else np.ascontiguousarray(K1, dtype=np.float64).reshape(9)
        K2 = None if K2 is None else np.ascontiguousarray(K2, dtype=np.float64).reshape(9)
        n = x1.shape[0]
        M = np.zeros(9); F = np.zeros(9)
        mask = np.zeros(max(n, 1), dtype=np.uint8); inl = np.zeros(max(n, 1), dtype=np.int32)
        ni, its = C.c_int(), C.c_int()
        emax, nfa = C.c_double(), C.c_double()
        self._chk(self.lib.clc_two_view_acransac(self.h, ord(model), _p(x1), _p(x2), n, _p(K1), _p(K2), int(img_wh[0]), int(img_wh[1]),
                                                 int(max_iteration), int(seed), float(precision), _p(M), _p(F), _p(mask), _p(inl),
                                                 C.byref(ni), C.byref(emax), C.byref(nfa), C.byref(its)))
        ok = ni.value > 0
        return dict(M=M.reshape(3, 3) if ok else None, F=F.reshape(3, 3) if ok else None, mask=mask[:n].astype(bool),
                    inliers=inl[:ni.value].copy(), error_max=emax.value, min_nfa=nfa.value, iterations=its.value)

    def two_view_minimal(self, model, x1, x2, img_wh, samples):
        """clc_two_view_minimal: the seven-point ('F') / four-point ('H') models of the given samples (S x 7 | 4 indices), in the
        coordinates conditioned by the image size: array (S, 3 | 1, 9), NaN rows where a sample has fewer real roots."""
        x1 = np.ascontiguousarray(x1, dtype=np.float64).reshape(-1, 2)
        x2 = np.ascontiguousarray(x2, dtype=np.float64).reshape(-1, 2)
        m, M = (7, 3) if model == "F" else (4, 1)
        smp = np.ascontiguousarray(samples, dtype=np.int32).reshape(-1, m)
        out = np.zeros((smp.shape[0], M, 9))
        self._chk(self.lib.clc_two_view_minimal(self.h, ord(model), _p(x1), _p(x2), x1.shape[0], int(img_wh[0]), int(img_wh[1]), _p(smp),
                                                smp.shape[0], _p(out)))
        return out

    def sim3_acransac(self, x_new, x_old, max_iteration=256, seed=1, precision=float("inf")):
        """clc_sim3_acransac: the a-contrario 3-D similarity NEW -> OLD, X_old ~ s R X_new + t.  Returns a dict: found, s, R (3,3), t (3),
        A (3,4) = [sR | t], mask, inliers (ascending residual order), error_max (old-map units), min_nfa, iterations, valid, refit."""
        x_new = np.ascontiguousarray(x_new, dtype=np.float64).reshape(-1, 3)
        x_old = np.ascontiguousarray(x_old, dtype=np.float64).reshape(-1, 3)
        n = x_new.shape[0]
        assert x_old.shape[0] == n
        R = np.zeros(9); t = np.zeros(3); A = np.zeros(12)
        mask = np.zeros(max(n, 1), dtype=np.uint8); inl = np.zeros(max(n, 1), dtype=np.int32)
        ni, its, valid, refit = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        s, emax, nfa = C.c_double(), C.c_double(), C.c_double()
        self._chk(self.lib.clc_sim3_acransac(self.h, _p(x_new), _p(x_old), n, int(max_iteration), int(seed), float(precision), C.byref(s),
                                             _p(R), _p(t), _p(A), _p(mask), _p(inl), C.byref(ni), C.byref(emax), C.byref(nfa), C.byref(its),
                                             C.byref(valid), C.byref(refit)))
        return dict(found=valid.value >= 0, s=s.value, R=R.reshape(3, 3), t=t, A=A.reshape(3, 4), mask=mask[:n].astype(bool),
                    inliers=inl[:ni.value].copy(), n_inliers=ni.value, error_max=emax.value, min_nfa=nfa.value, iterations=its.value,
                    valid=valid.value, refit=refit.value)

    def sim3_minimal(self, x_new, x_old, samples):
        """clc_sim3_minimal: the minimal similarities [sR | t] of the given samples (S x 3 indices): array (S, 12), NaN rows where a
        sample is degenerate or names no correspondence."""
        x_new = np.ascontiguousarray(x_new, dtype=np.float64).reshape(-1, 3)
        x_old = np.ascontiguousarray(x_old, dtype=np.float64).reshape(-1, 3)
        smp = np.ascontiguousarray(samples, dtype=np.int32).reshape(-1, 3)
        out = np.zeros((smp.shape[0], 12))
        self._chk(self.lib.clc_sim3_minimal(self.h, _p(x_new), _p(x_old), x_new.shape[0], _p(smp), smp.shape[0], _p(out)))
        return out

    def pnp_refine(self, X, x, K, Rt0, mask=None, huber_a=16.0, max_iter=50):
        """LM refinement of one pose: returns (Rt (3,4), cov (6,6), rmse, iterations)."""
        X = np.ascontiguousarray(X, dtype=np.float64).reshape(-1, 3)
        x = np.ascontiguousarray(x, dtype=np.float64).reshape(-1, 2)
        K = np.ascontiguousarray(K, dtype=np.float64).reshape(9)
        Rt0 = np.ascontiguousarray(Rt0, dtype=np.float64).reshape(12)
        m = None if mask is None else np.ascontiguousarray(mask, dtype=np.uint8)
        Rt = np.zeros(12); cov = np.zeros(36)
        rmse, it = C.c_double(), C.c_int()
        self._chk(self.lib.clc_pnp_refine(self.h, _p(X), _p(x), X.shape[0], _p(K), _p(m), _p(Rt0), float(huber_a), int(max_iter),
                                          _p(Rt), _p(cov), C.byref(rmse), C.byref(it)))
        return Rt.reshape(3, 4), cov.reshape(6, 6), rmse.value, it.value

    def pnp_p3p(self, X, x, K, samples):
        X = np.ascontiguousarray(X, dtype=np.float64).reshape(-1, 3)
        x = np.ascontiguousarray(x, dtype=np.float64).reshape(-1, 2)
        K = np.ascontiguousarray(K, dtype=np.float64).reshape(9)
        samples = np.ascontiguousarray(samples, dtype=np.int32).reshape(-1, 3)
        out = np.zeros((samples.shape[0], 4, 12), dtype=np.float64)
        self._chk(self.lib.clc_pnp_p3p(self.h, _p(X), _p(x), X.shape[0], _p(K), _p(samples), samples.shape[0], _p(out)))
        return out

    def pnp_score(self, Rt, X, x, K, thr2):
        Rt = np.ascontiguousarray(Rt, dtype=np.float64).reshape(-1, 12)
        X = np.ascontiguousarray(X, dtype=np.float64).reshape(-1, 3)
        x = np.ascontiguousarray(x, dtype=np.float64).reshape(-1, 2)
        K = np.ascontiguousarray(K, dtype=np.float64).reshape(9)
        cnt = np.zeros(Rt.shape[0], dtype=np.int32)
        cost = np.zeros(Rt.shape[0], dtype=np.float64)
        self._chk(self.lib.clc_pnp_score(self.h, _p(Rt), Rt.shape[0], _p(X), _p(x), X.shape[0], _p(K), float(thr2), _p(cnt), _p(cost)))
        return cnt, cost
