"""ctypes binding of libccm_hot.so (the C ABI declared in include/ccm_hot.h).

There is no CPU fallback: if the shared library is missing or a GPU call fails,
the caller gets an exception.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# CCM_HOT_LIB: another build of the same ABI (A/B timing of kernel variants, tools/ab_orb.sh); the ABI version is checked either way
LIB_PATH = os.environ.get("CCM_HOT_LIB") or os.path.join(_HERE, "libccm_hot.so")

CCM_OK = 0
ERRORS = {-1: "CCM_E_ARG", -2: "CCM_E_DEVICE", -3: "CCM_E_NOMEM", -4: "CCM_E_CAPACITY",
          -5: "CCM_E_NUMERIC", -6: "CCM_E_COMM", -7: "CCM_E_STATE"}
COMM_ID_BYTES = 128

KP_DTYPE = np.dtype([("x", "f4"), ("y", "f4"), ("size", "f4"), ("angle", "f4"), ("response", "f4"),
                     ("octave", "i4"), ("class_id", "i4")])

# every symbol include/ccm_hot.h declares (tests check the library exports all of them)
SYMBOLS = [
    "ccm_abi_version", "ccm_create", "ccm_destroy", "ccm_last_error", "ccm_sync", "ccm_stream",
    "ccm_host_register", "ccm_host_unregister", "ccm_profile_enable", "ccm_profile_read",
    "ccm_orb_tables", "ccm_orb_level_sizes", "ccm_orb_extract", "ccm_orb_extract_dev", "ccm_orb_fetch",
    "ccm_orb_result_dev", "ccm_orb_debug_level", "ccm_orb_debug_candidates", "ccm_orb_debug_lane_plan", "ccm_debug_fast_score", "ccm_debug_fc_items",
    "ccm_debug_od_steer", "ccm_descriptor_distance", "ccm_hamming_match", "ccm_hamming_match_dev", "ccm_debug_fp4_tile", "ccm_ratio_test", "ccm_match_bow",
    "ccm_window_candidates", "ccm_search_by_projection", "ccm_search_by_projection_frame", "ccm_search_for_initialization", "ccm_fuse_select", "ccm_fuse_select_batch", "ccm_search_by_sim3", "ccm_search_by_projection_sim3", "ccm_search_by_projection_sim3_batch",
    "ccm_search_for_triangulation", "ccm_voc_create", "ccm_voc_destroy", "ccm_voc_words", "ccm_voc_transform", "ccm_voc_transform_dev",
    "ccm_bow_vector", "ccm_bow_score_l1", "ccm_distinctive_descriptors", "ccm_optimize_sim3", "ccm_optimize_essential_graph", "ccm_correct_map_points",
    "ccm_ba_solve", "ccm_ba_landmark_cuts", "ccm_pose_optimize", "ccm_comm_unique_id", "ccm_comm_init", "ccm_comm_attach", "ccm_comm_destroy",
    "ccm_pose_from_mat4f", "ccm_pose_to_mat4f",
    "ccm_ba_solve_table_frames", "ccm_pose_to_camera", "ccm_frame_get_pose",
    "ccm_frame_create", "ccm_frame_from_extract", "ccm_frame_destroy", "ccm_frame_size", "ccm_frame_set_map_points",
    "ccm_frame_get_map_points", "ccm_frame_debug_grid", "ccm_frame_search_by_projection", "ccm_frame_search_by_projection_frame",
    "ccm_frame_pose_optimize",
    "ccm_frame_set_bow", "ccm_frame_set_camera", "ccm_frame_set_pose", "ccm_frame_debug_bow", "ccm_fuse_select_batch_frames",
    "ccm_map_table_create", "ccm_map_table_destroy", "ccm_map_table_capacity", "ccm_map_table_update", "ccm_map_table_set_order",
    "ccm_map_table_fetch", "ccm_map_table_refresh", "ccm_map_table_correct_frames", "ccm_map_table_attach", "ccm_map_table_handles", "ccm_frame_search_local_points", "ccm_frame_search_local_points_timing", "ccm_frame_pose_optimize_table",
    "ccm_fuse_select_table_frames", "ccm_frame_track_motion_model", "ccm_frame_search_by_projection_keyframe",
    "ccm_frame_relocalize_candidate",
    "ccm_search_by_sim3_table_frames", "ccm_search_by_projection_table_frames",
    "ccm_sim3_solver_create_frames", "ccm_optimize_sim3_table_frames", "ccm_compute_sim3_table_frames",
    "ccm_sim3_ransac_iterations", "ccm_sim3_solver_create", "ccm_sim3_solver_destroy", "ccm_sim3_solver_count", "ccm_sim3_solver_iterate",
    "ccm_sim3_solver_find", "ccm_sim3_solver_estimate", "ccm_sim3_solver_state", "ccm_sim3_solver_hypotheses",
    "ccm_pnp_ransac_parameters", "ccm_pnp_compute_pose", "ccm_pnp_solver_create", "ccm_pnp_solver_destroy", "ccm_pnp_solver_count",
    "ccm_pnp_solver_iterate", "ccm_pnp_solver_find", "ccm_pnp_solver_state", "ccm_pnp_solver_hypotheses", "ccm_pnp_solver_refinements",
    "ccm_pnp_solver_create_frames",
    "ccm_initialize", "ccm_create_new_map_points", "ccm_create_new_map_points_frames",
    "ccm_map_pair_geometry", "ccm_scene_median_depth",
    "ccm_frame_compute_bow", "ccm_frame_search_by_bow", "ccm_search_by_bow_frames",
    "ccm_undistort_points", "ccm_image_bounds", "ccm_frame_from_extract_camera", "ccm_frames_from_extract_camera", "ccm_frame_get_keypoints",
    "ccm_kfdb_create", "ccm_kfdb_destroy", "ccm_kfdb_add", "ccm_kfdb_erase", "ccm_kfdb_clear", "ccm_kfdb_size", "ccm_kfdb_slot", "ccm_kfdb_slots",
    "ccm_kfdb_keys", "ccm_kfdb_query", "ccm_kfdb_query_vector", "ccm_kfdb_query_lds_words", "ccm_kfdb_arena", "ccm_kfdb_last_timing",
    "ccm_kfdb_shortlist", "ccm_kfdb_candidates", "ccm_kfdb_min_score", "ccm_kfdb_reloc_candidates",
    "ccm_covis_create", "ccm_covis_destroy", "ccm_covis_put", "ccm_covis_erase", "ccm_covis_clear", "ccm_covis_size", "ccm_covis_slot",
    "ccm_covis_slots", "ccm_covis_keys", "ccm_covis_query", "ccm_covis_lds_features", "ccm_covis_arena", "ccm_covis_last_timing",
    "ccm_covis_connections",
]


class CcmError(RuntimeError):
    def __init__(self, code, text=""):
        super().__init__("%s (%d): %s" % (ERRORS.get(code, "CCM_E_?"), code, text))
        self.code = code


class OrbParams(C.Structure):
    _fields_ = [("nfeatures", C.c_int), ("scale_factor", C.c_float), ("nlevels", C.c_int),
                ("ini_th_fast", C.c_int), ("min_th_fast", C.c_int)]


class BowOptions(C.Structure):
    _fields_ = [("nnratio", C.c_float), ("check_ori", C.c_int), ("th", C.c_int), ("strict_th", C.c_int)]


class FrameGrid(C.Structure):
    _fields_ = [("n", C.c_int), ("kp_x", C.c_void_p), ("kp_y", C.c_void_p), ("kp_octave", C.c_void_p), ("desc", C.c_void_p),
                ("min_x", C.c_float), ("min_y", C.c_float), ("inv_w", C.c_float), ("inv_h", C.c_float),
                ("grid_cols", C.c_int), ("grid_rows", C.c_int)]


class CameraStruct(C.Structure):                      # ccm_camera
    _fields_ = [(k, C.c_float) for k in ("fx", "fy", "cx", "cy", "k1", "k2", "p1", "p2", "k3")]


class FrameBounds(C.Structure):                       # ccm_frame_bounds
    _fields_ = [(k, C.c_float) for k in ("min_x", "max_x", "min_y", "max_y", "inv_w", "inv_h")]


class BaProblem(C.Structure):
    _fields_ = [("n_poses", C.c_int), ("poses", C.c_void_p), ("fixed", C.c_void_p), ("intr", C.c_void_p),
                ("n_points", C.c_int), ("points", C.c_void_p),
                ("n_edges", C.c_int), ("edge_pose", C.c_void_p), ("edge_point", C.c_void_p),
                ("obs", C.c_void_p), ("info", C.c_void_p)]


class BaTableProblem(C.Structure):                    # ccm_ba_table_problem
    _fields_ = [("n_kf", C.c_int32), ("kfs", C.POINTER(C.c_void_p)), ("poses", C.c_void_p), ("fixed", C.c_void_p), ("intr", C.c_void_p),
                ("publish", C.c_void_p), ("n_points", C.c_int32), ("slot", C.c_void_p), ("obs_first", C.c_void_p), ("obs_kf", C.c_void_p),
                ("obs_feat", C.c_void_p), ("inv_level_sigma2", C.c_void_p), ("n_levels", C.c_int32), ("pos_out", C.c_void_p)]


class PoseProblem(C.Structure):
    _fields_ = [("n_frames", C.c_int), ("poses", C.c_void_p), ("intr", C.c_void_p), ("first", C.c_void_p),
                ("points", C.c_void_p), ("obs", C.c_void_p), ("info", C.c_void_p), ("outlier", C.c_void_p),
                ("n_inliers", C.c_void_p)]


class Sim3Problem(C.Structure):
    _fields_ = [("n_problems", C.c_int), ("sim3", C.c_void_p), ("fix_scale", C.c_void_p), ("K1", C.c_void_p), ("K2", C.c_void_p),
                ("first", C.c_void_p), ("P1", C.c_void_p), ("P2", C.c_void_p), ("obs1", C.c_void_p), ("obs2", C.c_void_p),
                ("info1", C.c_void_p), ("info2", C.c_void_p), ("th2", C.c_void_p), ("inlier", C.c_void_p), ("n_inliers", C.c_void_p)]


class Sim3RansacProblem(C.Structure):
    _fields_ = [("n_solvers", C.c_int32), ("first", C.c_void_p), ("n1", C.c_void_p), ("fix_scale", C.c_void_p), ("K1", C.c_void_p),
                ("K2", C.c_void_p), ("X1", C.c_void_p), ("X2", C.c_void_p), ("max_err1", C.c_void_p), ("max_err2", C.c_void_p),
                ("indices1", C.c_void_p), ("probability", C.c_double), ("min_inliers", C.c_int32), ("max_iterations", C.c_int32),
                ("draws", C.c_void_p), ("best_inliers", C.c_void_p)]


class PnpRansacProblem(C.Structure):                  # ccm_pnp_ransac_problem
    _fields_ = [("n_solvers", C.c_int32), ("first", C.c_void_p), ("n1", C.c_void_p), ("K", C.c_void_p), ("P2D", C.c_void_p),
                ("P3Dw", C.c_void_p), ("sigma2", C.c_void_p), ("kp_index", C.c_void_p), ("probability", C.c_double),
                ("min_inliers", C.c_int32), ("max_iterations", C.c_int32), ("min_set", C.c_int32), ("epsilon", C.c_float),
                ("th2", C.c_float), ("reserve", C.c_int32), ("draws", C.c_void_p), ("flags", C.c_uint32)]


class PnpFramesProblem(C.Structure):                  # ccm_pnp_frames_problem
    _fields_ = [("n_solvers", C.c_int32), ("first", C.c_void_p), ("K", C.c_void_p), ("feature", C.c_void_p), ("slot", C.c_void_p),
                ("level_sigma2", C.c_void_p), ("n_levels", C.c_int32), ("probability", C.c_double),
                ("min_inliers", C.c_int32), ("max_iterations", C.c_int32), ("min_set", C.c_int32), ("epsilon", C.c_float),
                ("th2", C.c_float), ("reserve", C.c_int32), ("draws", C.c_void_p), ("flags", C.c_uint32)]


class InitializerProblem(C.Structure):
    _fields_ = [("n1", C.c_int32), ("kp1_xy", C.c_void_p), ("n2", C.c_int32), ("kp2_xy", C.c_void_p), ("matches12", C.c_void_p),
                ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float), ("sigma", C.c_float),
                ("max_iterations", C.c_int32), ("min_parallax", C.c_float), ("min_triangulated", C.c_int32), ("draws", C.c_void_p)]


class InitializerTap(C.Structure):
    _fields_ = [("H21", C.c_void_p), ("H12", C.c_void_p), ("F21", C.c_void_p), ("score_h", C.c_void_p), ("score_f", C.c_void_p),
                ("mask_h", C.c_void_p), ("mask_f", C.c_void_p), ("sets", C.c_void_p), ("n_candidates", C.c_int32),
                ("cand_R", C.c_float * 72), ("cand_t", C.c_float * 24), ("cand_n_good", C.c_int32 * 8), ("cand_parallax", C.c_float * 8),
                ("cand_flags", C.c_void_p), ("cand_cos", C.c_void_p), ("cand_p3d", C.c_void_p)]


class InitializerResult(C.Structure):
    _fields_ = [("initialized", C.c_int32), ("model", C.c_int32), ("score_h", C.c_float), ("score_f", C.c_float),
                ("best_h", C.c_int32), ("best_f", C.c_int32), ("n_matches", C.c_int32), ("R21", C.c_float * 9), ("t21", C.c_float * 3),
                ("p3d", C.c_void_p), ("triangulated", C.c_void_p), ("tap", C.POINTER(InitializerTap))]


class MapKeyframe(C.Structure):
    _fields_ = [("n", C.c_int32), ("kp_x", C.c_void_p), ("kp_y", C.c_void_p), ("kp_octave", C.c_void_p), ("desc", C.c_void_p),
                ("node", C.c_void_p), ("has_mp", C.c_void_p), ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float),
                ("Tcw", C.c_void_p), ("Ow", C.c_void_p), ("scale_factors", C.c_void_p), ("level_sigma2", C.c_void_p), ("n_levels", C.c_int32)]


class NewPointsProblem(C.Structure):
    _fields_ = [("current", C.POINTER(MapKeyframe)), ("n_kf", C.c_int32), ("neighbours", C.POINTER(MapKeyframe)), ("F12", C.c_void_p),
                ("epipole", C.c_void_p), ("median_depth", C.c_void_p)]


class NewPointsTap(C.Structure):
    _fields_ = [("match", C.c_void_p), ("status", C.c_void_p), ("x3d_all", C.c_void_p)]


class NewPointsResult(C.Structure):
    _fields_ = [("n_new", C.c_int32), ("kf", C.c_void_p), ("idx1", C.c_void_p), ("idx2", C.c_void_p), ("x3d", C.c_void_p),
                ("first", C.c_void_p), ("tap", C.POINTER(NewPointsTap))]


class NewPointsFrames(C.Structure):
    _fields_ = [("current", C.c_void_p), ("n_kf", C.c_int32), ("neighbours", C.POINTER(C.c_void_p)), ("F12", C.c_void_p),
                ("epipole", C.c_void_p), ("median_depth", C.c_void_p)]


# CCM_NP_* of include/ccm_hot.h: what became of (neighbour k, feature i1) in ccm_create_new_map_points
NP_STATUS = ("SKIPPED_KF", "HAS_MP", "NO_MATCH", "LOW_PARALLAX", "W_ZERO", "NONFINITE", "BEHIND_1", "BEHIND_2", "REPROJ_1", "REPROJ_2",
             "ZERO_DIST", "SCALE", "OK", "SUPERSEDED")


MP_LIVE, MP_BAD, MP_HAS_OBS = 1, 2, 4          # CCM_MP_* of include/ccm_hot.h


class MapUpdate(C.Structure):
    _fields_ = [("n", C.c_int32), ("slot", C.c_void_p), ("pos", C.c_void_p), ("normal", C.c_void_p), ("min_dist", C.c_void_p),
                ("max_dist", C.c_void_p), ("desc", C.c_void_p), ("flags", C.c_void_p)]


MPR_DESCRIPTOR, MPR_NORMAL_DEPTH = 1, 2        # CCM_MPR_* of include/ccm_hot.h


class MapRefresh(C.Structure):
    _fields_ = [("n", C.c_int32), ("slot", C.c_void_p), ("pos", C.c_void_p), ("flags", C.c_void_p), ("n_kf", C.c_int32),
                ("kfs", C.POINTER(C.c_void_p)), ("obs_first", C.c_void_p), ("obs_kf", C.c_void_p), ("obs_feat", C.c_void_p),
                ("ref_kf", C.c_void_p), ("ref_feat", C.c_void_p), ("what", C.c_int32)]


class MapRefreshResult(C.Structure):
    _fields_ = [("best", C.c_void_p), ("normal", C.c_void_p), ("min_dist", C.c_void_p), ("max_dist", C.c_void_p)]


MC_SIM3, MC_RIGID = 0, 1                       # CCM_MC_* of include/ccm_hot.h: transform
MC_POSES_FIRST, MC_IN_ORDER = 0, 1             # order


class MapCorrect(C.Structure):
    _fields_ = [("n_kf", C.c_int32), ("kfs", C.POINTER(C.c_void_p)), ("n_moved", C.c_int32), ("transform", C.c_int32), ("order", C.c_int32),
                ("sim3_before", C.c_void_p), ("sim3_after", C.c_void_p), ("Tcw_after", C.c_void_p), ("Ow_after", C.c_void_p),
                ("n_points", C.c_int32), ("slot", C.c_void_p), ("owner", C.c_void_p), ("obs_first", C.c_void_p), ("obs_kf", C.c_void_p),
                ("obs_feat", C.c_void_p), ("ref_kf", C.c_void_p), ("ref_feat", C.c_void_p), ("pos_out", C.c_void_p),
                ("normal_out", C.c_void_p), ("min_dist_out", C.c_void_p), ("max_dist_out", C.c_void_p)]


class SlpParams(C.Structure):
    _fields_ = [("Tcw", C.c_float * 12), ("Ow", C.c_float * 3), ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float),
                ("min_x", C.c_float), ("max_x", C.c_float), ("min_y", C.c_float), ("max_y", C.c_float), ("viewing_cos_limit", C.c_float),
                ("log_scale_factor", C.c_float), ("n_levels", C.c_int32), ("scale_factors", C.c_void_p), ("th", C.c_float),
                ("nnratio", C.c_float)]


class SlpResult(C.Structure):
    _fields_ = [("n_to_match", C.c_int32), ("in_view_cap", C.c_int32), ("in_view_slot", C.c_void_p), ("proj_x", C.c_void_p),
                ("proj_y", C.c_void_p), ("level", C.c_void_p), ("view_cos", C.c_void_p), ("match", C.c_void_p), ("mp_id", C.c_void_p),
                ("occupied", C.c_void_p)]


class TmmParams(C.Structure):
    _fields_ = [("Tcw", C.c_float * 12), ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float),
                ("min_x", C.c_float), ("max_x", C.c_float), ("min_y", C.c_float), ("max_y", C.c_float), ("n_levels", C.c_int32),
                ("scale_factors", C.c_void_p), ("th", C.c_float), ("retry_below", C.c_int32), ("min_matches", C.c_int32),
                ("check_ori", C.c_int32), ("orb_dist", C.c_int32), ("last_outlier", C.c_void_p), ("inv_level_sigma2", C.c_void_p),
                ("intr", C.c_void_p)]


class TmmResult(C.Structure):
    _fields_ = [("n_matches", C.c_int32), ("passes", C.c_int32), ("posed", C.c_int32), ("n_inliers", C.c_int32),
                ("n_matches_map", C.c_int32), ("pose7", C.c_double * 7), ("match", C.c_void_p), ("mp_id", C.c_void_p),
                ("outlier", C.c_void_p), ("u", C.c_void_p), ("v", C.c_void_p), ("valid", C.c_void_p)]


class RelocView(C.Structure):                         # ccm_reloc_view
    _fields_ = [("Tcw", C.c_float * 12), ("Ow", C.c_float * 3), ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float),
                ("min_x", C.c_float), ("max_x", C.c_float), ("min_y", C.c_float), ("max_y", C.c_float), ("n_levels", C.c_int32),
                ("scale_factors", C.c_void_p), ("log_scale_factor", C.c_float)]


class RelocSearchResult(C.Structure):                 # ccm_reloc_search_result
    _fields_ = [("n_matches", C.c_int32), ("match", C.c_void_p), ("mp_id", C.c_void_p), ("u", C.c_void_p), ("v", C.c_void_p),
                ("level", C.c_void_p), ("valid", C.c_void_p)]


RELOC_POSE1, RELOC_SEARCH1, RELOC_POSE2, RELOC_SEARCH2, RELOC_POSE3 = 1, 2, 4, 8, 16      # CCM_RELOC_*


class RelocParams(C.Structure):                       # ccm_reloc_params
    _fields_ = [("Tcw", C.c_void_p), ("n_matched", C.c_int32), ("feature", C.c_void_p), ("slot", C.c_void_p), ("intr", C.c_void_p),
                ("inv_level_sigma2", C.c_void_p), ("view", RelocView), ("min_good", C.c_int32), ("enough", C.c_int32),
                ("narrow_above", C.c_int32), ("th1", C.c_float), ("dist1", C.c_int32), ("th2", C.c_float), ("dist2", C.c_int32),
                ("check_ori", C.c_int32)]


class RelocResult(C.Structure):                       # ccm_reloc_result
    _fields_ = [("success", C.c_int32), ("n_good", C.c_int32), ("stages", C.c_int32), ("n_add1", C.c_int32), ("n_add2", C.c_int32),
                ("pose7", C.c_double * 7), ("mp_id", C.c_void_p), ("outlier", C.c_void_p)]


FG_GATES = ("SEARCHED", "SKIPPED", "IN_KEYFRAME", "BEHIND", "OUTSIDE", "DISTANCE", "ANGLE", "EMPTY_KF")   # CCM_FG_* of include/ccm_hot.h


class FuseView(C.Structure):
    _fields_ = [("kf", C.c_void_p), ("Tcw", C.c_float * 12), ("Ow", C.c_float * 3), ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float),
                ("cy", C.c_float), ("min_x", C.c_float), ("max_x", C.c_float), ("min_y", C.c_float), ("max_y", C.c_float)]


class FuseTableProblem(C.Structure):
    _fields_ = [("n_kf", C.c_int32), ("views", C.POINTER(FuseView)), ("n_points", C.c_int32), ("slot", C.c_void_p), ("skip", C.c_void_p),
                ("log_scale_factor", C.c_float), ("n_levels", C.c_int32), ("scale_factors", C.c_void_p), ("inv_level_sigma2", C.c_void_p),
                ("th", C.c_float), ("chi2_check", C.c_int32), ("accept_th", C.c_int32)]


class FuseTableResult(C.Structure):
    _fields_ = [("best_idx", C.c_void_p), ("best_dist", C.c_void_p), ("gate", C.c_void_p), ("u", C.c_void_p), ("v", C.c_void_p),
                ("level", C.c_void_p), ("n_searched", C.c_int32)]


SG_GATES = ("SEARCHED", "NO_POINT", "MATCHED", "BAD", "BEHIND", "OUTSIDE", "DISTANCE", "EMPTY_KF")             # CCM_SG_*
LG_GATES = ("SEARCHED", "SKIPPED", "ALREADY_FOUND", "BEHIND", "OUTSIDE", "DISTANCE", "ANGLE", "EMPTY_KF")   # CCM_LG_*


class Sim3SearchPair(C.Structure):
    _fields_ = [("kf1", C.c_void_p), ("kf2", C.c_void_p), ("T1w", C.c_float * 12), ("T2w", C.c_float * 12), ("S21", C.c_float * 12),
                ("S12", C.c_float * 12), ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float),
                ("bounds1", C.c_float * 4), ("bounds2", C.c_float * 4), ("matched12", C.c_void_p), ("matched_idx2", C.c_void_p)]


class Sim3SearchProblem(C.Structure):
    _fields_ = [("n_pairs", C.c_int32), ("pairs", C.POINTER(Sim3SearchPair)), ("th", C.c_float),
                ("log_scale_factor1", C.c_float), ("n_levels1", C.c_int32), ("scale_factors1", C.c_void_p),
                ("log_scale_factor2", C.c_float), ("n_levels2", C.c_int32), ("scale_factors2", C.c_void_p)]


class Sim3SearchResult(C.Structure):
    _fields_ = [("match12", C.c_void_p), ("n_found", C.c_void_p),
                ("gate1", C.c_void_p), ("u1", C.c_void_p), ("v1", C.c_void_p), ("level1", C.c_void_p), ("sel1", C.c_void_p),
                ("gate2", C.c_void_p), ("u2", C.c_void_p), ("v2", C.c_void_p), ("level2", C.c_void_p), ("sel2", C.c_void_p)]


class Sim3FramesPair(C.Structure):                    # ccm_sim3_frames_pair
    _fields_ = [("kf1", C.c_void_p), ("kf2", C.c_void_p), ("T1w", C.c_float * 12), ("T2w", C.c_float * 12), ("K1", C.c_float * 4), ("K2", C.c_float * 4)]


class Sim3SolverFramesProblem(C.Structure):           # ccm_sim3_solver_frames_problem
    _fields_ = [("n_solvers", C.c_int32), ("pairs", C.POINTER(Sim3FramesPair)), ("first", C.c_void_p), ("fix_scale", C.c_void_p),
                ("feature1", C.c_void_p), ("feature2", C.c_void_p), ("n_levels1", C.c_int32), ("max_err_level1", C.c_void_p),
                ("n_levels2", C.c_int32), ("max_err_level2", C.c_void_p), ("probability", C.c_double), ("min_inliers", C.c_int32),
                ("max_iterations", C.c_int32), ("draws", C.c_void_p), ("best_inliers", C.c_void_p)]


class Sim3OptFramesProblem(C.Structure):              # ccm_sim3_opt_frames_problem
    _fields_ = [("n_problems", C.c_int32), ("pairs", C.POINTER(Sim3FramesPair)), ("first", C.c_void_p), ("fix_scale", C.c_void_p),
                ("th2", C.c_void_p), ("feature1", C.c_void_p), ("feature2", C.c_void_p), ("n_levels1", C.c_int32),
                ("inv_level_sigma2_1", C.c_void_p), ("n_levels2", C.c_int32), ("inv_level_sigma2_2", C.c_void_p)]


class Sim3OptFramesResult(C.Structure):               # ccm_sim3_opt_frames_result
    _fields_ = [("sim3", C.c_void_p), ("inlier", C.c_void_p), ("n_inliers", C.c_void_p)]


class ComputeSim3Pair(C.Structure):                   # ccm_compute_sim3_pair
    _fields_ = [("search", Sim3SearchPair), ("K2", C.c_float * 4), ("sim3", C.c_double * 8), ("fix_scale", C.c_int32), ("th2", C.c_float)]


class ComputeSim3Problem(C.Structure):                # ccm_compute_sim3_problem
    _fields_ = [("n_pairs", C.c_int32), ("pairs", C.POINTER(ComputeSim3Pair)), ("th", C.c_float),
                ("log_scale_factor1", C.c_float), ("n_levels1", C.c_int32), ("scale_factors1", C.c_void_p), ("inv_level_sigma2_1", C.c_void_p),
                ("log_scale_factor2", C.c_float), ("n_levels2", C.c_int32), ("scale_factors2", C.c_void_p), ("inv_level_sigma2_2", C.c_void_p)]


class ComputeSim3Result(C.Structure):                 # ccm_compute_sim3_result
    _fields_ = [("search", Sim3SearchResult), ("pruned", C.c_void_p), ("n_correspondences", C.c_void_p), ("n_inliers", C.c_void_p),
                ("sim3", C.c_void_p), ("corr", C.c_void_p), ("inlier", C.c_void_p)]


class LoopView(C.Structure):
    _fields_ = [("view", FuseView), ("matched_slot", C.c_void_p)]


class LoopProjectionProblem(C.Structure):
    _fields_ = [("n_kf", C.c_int32), ("views", C.POINTER(LoopView)), ("n_points", C.c_int32), ("slot", C.c_void_p),
                ("log_scale_factor", C.c_float), ("n_levels", C.c_int32), ("scale_factors", C.c_void_p), ("th", C.c_float)]


class LoopProjectionResult(C.Structure):
    _fields_ = [("best_idx", C.c_void_p), ("observed", C.c_void_p), ("matched_slot", C.c_void_p), ("n_matches", C.c_void_p),
                ("gate", C.c_void_p), ("u", C.c_void_p), ("v", C.c_void_p), ("level", C.c_void_p), ("best_dist", C.c_void_p)]


class EssentialGraph(C.Structure):
    _fields_ = [("n_vertices", C.c_int), ("sim3", C.c_void_p), ("fixed", C.c_void_p), ("fix_scale", C.c_int), ("n_edges", C.c_int),
                ("edge_i", C.c_void_p), ("edge_j", C.c_void_p), ("measurement", C.c_void_p), ("iterations", C.c_int),
                ("iterations_done", C.c_int), ("chi2_initial", C.c_double), ("chi2_final", C.c_double),
                ("factor_blocks", C.c_int), ("factor_rounds", C.c_int), ("solver_bytes", C.c_int64)]


class BaOptions(C.Structure):
    _fields_ = [("iterations", C.c_int), ("huber_delta", C.c_double), ("iterations2", C.c_int),
                ("outlier_chi2", C.c_double), ("stop_flag", C.c_void_p), ("pcg_tol", C.c_double)]


class BaResult(C.Structure):
    _fields_ = [("iterations_done", C.c_int), ("trials", C.c_int), ("chi2_initial", C.c_double),
                ("chi2_final", C.c_double), ("lambda_final", C.c_double), ("stopped", C.c_int),
                ("t_linearize", C.c_double), ("t_schur", C.c_double), ("t_solve", C.c_double),
                ("t_update", C.c_double), ("edge_outlier", C.c_void_p),
                ("schur_blocks", C.c_int32), ("schur_pairs", C.c_int64), ("pcg_iterations", C.c_int32),
                ("pcg_fallbacks", C.c_int32), ("pcg_pipelined", C.c_int32)]


COVIS_WEIGHTS, COVIS_REDUNDANCY = 1, 2          # CCM_COVIS_* of include/ccm_hot.h


class CovisResult(C.Structure):                       # ccm_covis_result
    _fields_ = [("th_obs", C.c_int32), ("weights", C.c_void_p), ("n_mps", C.c_void_p), ("n_redundant", C.c_void_p),
                ("skipped", C.c_void_p), ("seq", C.c_void_p)]


ABI_VERSION = 3        # CCM_ABI_VERSION of the include/ccm_hot.h these ctypes structures were written against
_lib = None


def load():
    """Load libccm_hot.so; raises if it has not been built (run __graft_entry__.build())."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError("%s not found: build it with `make -C motioncheck_ccm_slam_amd/csrc` "
                          "(or __graft_entry__.build()); there is no CPU fallback" % LIB_PATH)
    lib = C.CDLL(LIB_PATH)
    # the structures below mirror include/ccm_hot.h at this version; a stale library would read and write past them
    if lib.ccm_abi_version() != ABI_VERSION:
        raise ImportError("%s has ABI version %d, this package mirrors version %d of include/ccm_hot.h: rebuild it"
                          % (LIB_PATH, lib.ccm_abi_version(), ABI_VERSION))
    lib.ccm_create.restype = C.c_void_p
    lib.ccm_create.argtypes = [C.c_int, C.c_int]
    lib.ccm_destroy.argtypes = [C.c_void_p]
    lib.ccm_destroy.restype = None
    lib.ccm_last_error.restype = C.c_char_p
    lib.ccm_last_error.argtypes = [C.c_void_p]
    lib.ccm_sync.argtypes = [C.c_void_p]
    lib.ccm_stream.restype = C.c_void_p
    lib.ccm_stream.argtypes = [C.c_void_p]
    vp = C.c_void_p
    lib.ccm_host_register.argtypes = [vp, vp, C.c_size_t]
    lib.ccm_host_unregister.argtypes = [vp, vp]
    lib.ccm_profile_enable.argtypes = [vp, C.c_int]
    lib.ccm_profile_read.argtypes = [vp, vp, vp]
    lib.ccm_orb_tables.argtypes = [C.POINTER(OrbParams)] + [vp] * 6
    lib.ccm_orb_level_sizes.argtypes = [C.POINTER(OrbParams), C.c_int, C.c_int, vp, vp]
    lib.ccm_orb_extract.argtypes = [vp, C.POINTER(OrbParams), vp, C.c_int, C.c_int, C.c_int, C.c_size_t, C.c_int,
                                    vp, vp, vp, C.c_int]
    lib.ccm_orb_extract_dev.argtypes = [vp, C.POINTER(OrbParams), vp, C.c_int, C.c_int, C.c_int, C.c_size_t,
                                        C.c_int, C.c_int]
    lib.ccm_orb_fetch.argtypes = [vp, vp, vp, vp]
    lib.ccm_orb_result_dev.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(C.c_int)]
    lib.ccm_orb_debug_level.argtypes = [vp, C.c_int, C.c_int, vp, C.c_int]
    lib.ccm_orb_debug_candidates.argtypes = [vp, C.c_int, C.c_int, vp, vp, C.c_int]
    if hasattr(lib, "ccm_orb_debug_lane_plan"):        # (an older build timed through CCM_HOT_LIB has no lanes to plan)
        lib.ccm_orb_debug_lane_plan.argtypes = [C.c_int, C.c_int, C.c_int, vp, vp, vp, C.c_int]
    if hasattr(lib, "ccm_debug_fast_score"):           # (likewise)
        lib.ccm_debug_fast_score.argtypes = [vp, C.c_int, C.c_int, vp, vp]
    if hasattr(lib, "ccm_debug_fc_items"):             # (likewise)
        lib.ccm_debug_fc_items.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, vp, C.c_int]
    if hasattr(lib, "ccm_debug_od_steer"):             # (likewise)
        lib.ccm_debug_od_steer.argtypes = [vp, vp, vp, C.c_int, vp, vp, vp]
    lib.ccm_descriptor_distance.argtypes = [vp, vp]
    lib.ccm_hamming_match.argtypes = [vp, vp, C.c_int, vp, C.c_int, C.c_int, vp, vp, vp, vp, vp]
    lib.ccm_hamming_match_dev.argtypes = [vp, vp, C.c_int, C.c_size_t, vp, C.c_int, C.c_size_t, C.c_int,
                                          vp, vp, vp, vp, vp]
    lib.ccm_debug_fp4_tile.argtypes = [vp, vp, vp, vp, vp]
    lib.ccm_ratio_test.argtypes = [C.c_int, C.c_int, C.c_float, C.c_int, C.c_int]
    lib.ccm_match_bow.argtypes = [vp, C.POINTER(BowOptions), vp, vp, vp, vp, C.c_int, vp, vp, vp, vp, C.c_int, vp]
    lib.ccm_window_candidates.argtypes = [vp, C.POINTER(FrameGrid), C.c_int, vp, vp, vp, vp, vp, vp, C.c_int, vp, vp, vp]
    lib.ccm_search_by_projection.argtypes = [vp, C.POINTER(FrameGrid), vp, C.c_int, vp, vp, vp, vp, vp, vp, vp, vp, C.c_float, C.c_float, vp]
    lib.ccm_search_by_projection_frame.argtypes = [vp, C.POINTER(FrameGrid), vp, vp, C.c_int, vp, vp, vp, vp, vp, vp, vp, vp, C.c_float, C.c_int, C.c_int, vp]
    lib.ccm_search_for_initialization.argtypes = [vp, C.c_int, vp, vp, vp, C.POINTER(FrameGrid), vp, vp, C.c_int, C.c_float, C.c_int, vp]
    lib.ccm_fuse_select.argtypes = [vp, C.POINTER(FrameGrid), vp, vp, C.c_int, vp, vp, vp, vp, vp, C.c_float, C.c_int, C.c_int, vp, vp]
    lib.ccm_fuse_select_batch.argtypes = [vp, C.c_int, vp, vp, vp, vp, vp, vp, vp, vp, vp, C.c_float, C.c_int, C.c_int, vp, vp]
    lib.ccm_search_by_sim3.argtypes = [vp, C.POINTER(FrameGrid), vp, C.POINTER(FrameGrid), vp] + [vp] * 10 + [C.c_float, vp]
    lib.ccm_search_by_projection_sim3.argtypes = [vp, C.POINTER(FrameGrid), vp, C.c_int] + [vp] * 7 + [C.c_float, vp]
    lib.ccm_search_by_projection_sim3_batch.argtypes = [vp, C.c_int, vp, vp, vp] + [vp] * 7 + [C.c_float, vp, vp]
    lib.ccm_search_for_triangulation.argtypes = [vp] * 7 + [C.c_int] + [vp] * 7 + [C.c_int, vp, C.c_float, C.c_float, vp, vp, C.c_int, vp]
    lib.ccm_voc_create.argtypes = [vp, C.c_int, C.c_int, C.c_int, vp, vp, vp, C.POINTER(vp)]
    lib.ccm_voc_destroy.argtypes = [vp]; lib.ccm_voc_destroy.restype = None
    lib.ccm_voc_words.argtypes = [vp]
    lib.ccm_voc_transform.argtypes = [vp, vp, C.c_int, C.c_int, vp, vp, vp]
    lib.ccm_voc_transform_dev.argtypes = [vp, vp, C.c_int, C.c_int, vp, vp, vp]
    lib.ccm_bow_vector.argtypes = [C.c_int, vp, vp, vp, C.c_int, C.c_int, vp, vp, vp]
    lib.ccm_bow_score_l1.argtypes = [C.c_int, vp, vp, C.c_int, vp, vp]; lib.ccm_bow_score_l1.restype = C.c_double
    lib.ccm_distinctive_descriptors.argtypes = [vp, vp, vp, vp, C.c_int, vp]
    lib.ccm_ba_solve.argtypes = [vp, C.POINTER(BaProblem), C.POINTER(BaOptions), C.POINTER(BaResult)]
    lib.ccm_ba_landmark_cuts.argtypes = [vp, C.c_int, C.c_int, C.c_int, vp]
    lib.ccm_comm_attach.argtypes = [vp, vp, C.c_int, C.c_int]
    lib.ccm_pose_optimize.argtypes = [vp, C.POINTER(PoseProblem)]
    lib.ccm_optimize_sim3.argtypes = [vp, C.POINTER(Sim3Problem)]
    lib.ccm_optimize_essential_graph.argtypes = [vp, C.POINTER(EssentialGraph)]
    lib.ccm_correct_map_points.argtypes = [vp, C.c_int, vp, vp, C.c_int, vp, vp]
    lib.ccm_comm_unique_id.argtypes = [vp]
    lib.ccm_comm_init.argtypes = [vp, vp, C.c_int, C.c_int]
    lib.ccm_comm_destroy.argtypes = [vp]
    lib.ccm_pose_from_mat4f.argtypes = [vp, vp]
    lib.ccm_pose_to_mat4f.argtypes = [vp, vp]
    if hasattr(lib, "ccm_ba_solve_table_frames"):      # (an older build timed through CCM_HOT_LIB has no table route)
        lib.ccm_ba_solve_table_frames.argtypes = [vp, vp, C.POINTER(BaTableProblem), C.POINTER(BaOptions), C.POINTER(BaResult)]
        lib.ccm_pose_to_camera.argtypes = [vp, vp, vp]
        lib.ccm_frame_get_pose.argtypes = [vp, vp, vp]
    lib.ccm_frame_create.argtypes = [vp, C.POINTER(FrameGrid), vp, C.POINTER(vp)]
    lib.ccm_frame_from_extract.argtypes = [vp, C.c_int, C.c_int, vp, vp, C.c_float, C.c_float, C.c_float, C.c_float, C.c_int, C.c_int,
                                           C.POINTER(vp)]
    lib.ccm_undistort_points.argtypes = [C.POINTER(CameraStruct), C.c_int, vp, vp, vp, vp]
    lib.ccm_image_bounds.argtypes = [C.POINTER(CameraStruct), C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(FrameBounds)]
    lib.ccm_frame_from_extract_camera.argtypes = [vp, C.c_int, C.c_int, C.POINTER(CameraStruct), C.POINTER(FrameBounds), C.c_int, C.c_int,
                                                  C.POINTER(vp)]
    lib.ccm_frames_from_extract_camera.argtypes = [vp, C.c_int, C.c_int, C.POINTER(CameraStruct), C.POINTER(FrameBounds), C.c_int, C.c_int,
                                                   C.POINTER(vp)]
    lib.ccm_frame_get_keypoints.argtypes = [vp, vp, vp]
    lib.ccm_frame_destroy.argtypes = [vp]; lib.ccm_frame_destroy.restype = None
    lib.ccm_frame_size.argtypes = [vp]
    lib.ccm_frame_set_map_points.argtypes = [vp, vp]
    lib.ccm_frame_get_map_points.argtypes = [vp, vp]
    lib.ccm_frame_debug_grid.argtypes = [vp, vp, vp]
    lib.ccm_frame_search_by_projection.argtypes = [vp, vp, vp, C.c_int] + [vp] * 9 + [C.c_float, C.c_float, vp]
    lib.ccm_frame_search_by_projection_frame.argtypes = [vp, vp, vp, vp, C.c_int] + [vp] * 9 + [C.c_float, C.c_int, C.c_int, vp]
    lib.ccm_frame_pose_optimize.argtypes = [vp, vp, C.c_int, vp, vp, C.c_int, vp, vp, vp, vp]
    lib.ccm_frame_set_bow.argtypes = [vp, vp]
    lib.ccm_frame_set_camera.argtypes = [vp, C.c_float, C.c_float, C.c_float, C.c_float, vp, vp, C.c_int]
    lib.ccm_frame_set_pose.argtypes = [vp, vp, vp]
    lib.ccm_frame_debug_bow.argtypes = [vp, vp, vp, vp]
    lib.ccm_fuse_select_batch_frames.argtypes = [vp, C.c_int, C.POINTER(vp), vp, vp, vp, vp, vp, vp, vp, vp, C.c_float, C.c_int, C.c_int, vp, vp]
    lib.ccm_map_table_create.argtypes = [vp, C.c_int, C.POINTER(vp)]
    lib.ccm_map_table_destroy.argtypes = [vp]; lib.ccm_map_table_destroy.restype = None
    lib.ccm_map_table_capacity.argtypes = [vp]
    lib.ccm_map_table_attach.argtypes = [vp, vp, C.POINTER(vp)]
    lib.ccm_map_table_handles.argtypes = [vp]
    lib.ccm_map_table_update.argtypes = [vp, vp, C.POINTER(MapUpdate)]
    lib.ccm_map_table_set_order.argtypes = [vp, vp, C.c_int, vp]
    lib.ccm_map_table_fetch.argtypes = [vp, vp, C.c_int] + [vp] * 8
    lib.ccm_map_table_refresh.argtypes = [vp, vp, C.POINTER(MapRefresh), C.POINTER(MapRefreshResult)]
    lib.ccm_map_table_correct_frames.argtypes = [vp, vp, C.POINTER(MapCorrect)]
    lib.ccm_frame_search_local_points.argtypes = [vp, vp, vp, C.POINTER(SlpParams), C.POINTER(SlpResult)]
    lib.ccm_frame_search_local_points_timing.argtypes = [vp, vp]
    lib.ccm_frame_pose_optimize_table.argtypes = [vp, vp, vp, vp, C.c_int, vp, vp, vp, vp]
    lib.ccm_fuse_select_table_frames.argtypes = [vp, vp, C.POINTER(FuseTableProblem), C.POINTER(FuseTableResult)]
    lib.ccm_search_by_sim3_table_frames.argtypes = [vp, vp, C.POINTER(Sim3SearchProblem), C.POINTER(Sim3SearchResult)]
    lib.ccm_search_by_projection_table_frames.argtypes = [vp, vp, C.POINTER(LoopProjectionProblem), C.POINTER(LoopProjectionResult)]
    lib.ccm_frame_track_motion_model.argtypes = [vp, vp, vp, vp, C.POINTER(TmmParams), C.POINTER(TmmResult)]
    lib.ccm_frame_search_by_projection_keyframe.argtypes = [vp, vp, vp, vp, C.POINTER(RelocView), C.c_float, C.c_int, C.c_int, C.c_int, vp,
                                                            C.POINTER(RelocSearchResult)]
    lib.ccm_frame_relocalize_candidate.argtypes = [vp, vp, vp, vp, C.POINTER(RelocParams), C.POINTER(RelocResult)]
    lib.ccm_sim3_ransac_iterations.argtypes =[C.c_int, C.c_double, C.c_int, C.c_int]
    lib.ccm_sim3_solver_create.argtypes = [vp, C.POINTER(Sim3RansacProblem), C.POINTER(vp)]
    lib.ccm_sim3_solver_create_frames.argtypes = [vp, vp, C.POINTER(Sim3SolverFramesProblem), C.POINTER(vp)]
    lib.ccm_optimize_sim3_table_frames.argtypes = [vp, vp, C.POINTER(Sim3OptFramesProblem), C.POINTER(Sim3OptFramesResult)]
    lib.ccm_compute_sim3_table_frames.argtypes = [vp, vp, C.POINTER(ComputeSim3Problem), C.POINTER(ComputeSim3Result)]
    lib.ccm_sim3_solver_destroy.argtypes = [vp]; lib.ccm_sim3_solver_destroy.restype = None
    lib.ccm_sim3_solver_count.argtypes = [vp]
    lib.ccm_sim3_solver_iterate.argtypes = [vp, C.c_int, C.c_int, vp, vp, vp, vp, vp]
    lib.ccm_sim3_solver_find.argtypes = [vp, C.c_int, vp, vp, vp, vp]
    lib.ccm_sim3_solver_estimate.argtypes = [vp, C.c_int, vp, vp, vp]
    lib.ccm_sim3_solver_state.argtypes = [vp, C.c_int, vp, vp, vp, vp]
    lib.ccm_sim3_solver_hypotheses.argtypes = [vp, C.c_int, vp, vp, vp, vp]
    if hasattr(lib, "ccm_pnp_solver_create"):          # (an older build timed through CCM_HOT_LIB has no PnPsolver)
        lib.ccm_pnp_ransac_parameters.argtypes = [C.c_int, C.c_double, C.c_int, C.c_int, C.c_int, C.c_float, vp, vp, vp]
        lib.ccm_pnp_compute_pose.argtypes = [C.c_int, vp, vp, vp, vp, vp]
        lib.ccm_pnp_solver_create.argtypes = [vp, C.POINTER(PnpRansacProblem), C.POINTER(vp)]
        lib.ccm_pnp_solver_destroy.argtypes = [vp]; lib.ccm_pnp_solver_destroy.restype = None
        lib.ccm_pnp_solver_count.argtypes = [vp]
        lib.ccm_pnp_solver_iterate.argtypes = [vp, C.c_int, C.c_int, vp, vp, vp, vp, vp]
        lib.ccm_pnp_solver_find.argtypes = [vp, C.c_int, vp, vp, vp, vp]
        lib.ccm_pnp_solver_state.argtypes = [vp, C.c_int, vp, vp, vp, vp, vp]
        lib.ccm_pnp_solver_hypotheses.argtypes = [vp, C.c_int, vp, vp, vp, vp, vp]
        lib.ccm_pnp_solver_refinements.argtypes = [vp, C.c_int, vp, vp, vp, vp, vp]
        lib.ccm_pnp_solver_create_frames.argtypes = [vp, vp, vp, C.POINTER(PnpFramesProblem), C.POINTER(vp)]
    lib.ccm_initialize.argtypes = [vp, C.POINTER(InitializerProblem), C.POINTER(InitializerResult)]
    lib.ccm_create_new_map_points.argtypes = [vp, C.POINTER(NewPointsProblem), C.POINTER(NewPointsResult)]
    lib.ccm_create_new_map_points_frames.argtypes = [vp, C.POINTER(NewPointsFrames), C.POINTER(NewPointsResult)]
    if hasattr(lib, "ccm_map_pair_geometry"):          # (an older build timed through CCM_HOT_LIB has no host definitions)
        lib.ccm_map_pair_geometry.argtypes = [vp, vp, vp, vp, vp, vp, vp]
        lib.ccm_scene_median_depth.argtypes = [C.c_int, vp, C.c_int, vp, vp, vp, vp, vp]
    lib.ccm_frame_compute_bow.argtypes = [vp, vp, vp, C.c_int, vp, vp, vp]
    lib.ccm_frame_search_by_bow.argtypes = [vp, vp, vp, C.POINTER(BowOptions), vp, C.c_int, vp]
    lib.ccm_search_by_bow_frames.argtypes = [vp, vp, C.c_int, C.POINTER(vp), C.POINTER(BowOptions), vp, vp, vp, vp, vp]
    if hasattr(lib, "ccm_kfdb_create"):                # (an older build timed through CCM_HOT_LIB has no KeyFrameDatabase)
        lib.ccm_kfdb_create.argtypes = [vp, C.c_int, C.c_int64, C.POINTER(vp)]
        lib.ccm_kfdb_destroy.argtypes = [vp]; lib.ccm_kfdb_destroy.restype = None
        lib.ccm_kfdb_add.argtypes = [vp, C.c_int64, C.c_int, vp, vp]
        lib.ccm_kfdb_erase.argtypes = [vp, C.c_int64]
        lib.ccm_kfdb_clear.argtypes = [vp]
        lib.ccm_kfdb_size.argtypes = [vp]
        lib.ccm_kfdb_slot.argtypes = [vp, C.c_int64]
        lib.ccm_kfdb_slots.argtypes = [vp]
        lib.ccm_kfdb_keys.argtypes = [vp, C.c_int, vp, vp]
        lib.ccm_kfdb_query.argtypes = [vp, vp, C.c_int64, C.c_int, vp, vp, vp, vp]
        lib.ccm_kfdb_query_vector.argtypes = [vp, vp, C.c_int, vp, vp, C.c_int, vp, vp, vp, vp]
        lib.ccm_kfdb_query_lds_words.argtypes = []
        lib.ccm_kfdb_arena.argtypes = [vp, vp, vp, vp]
        lib.ccm_kfdb_last_timing.argtypes = [vp, vp]
        lib.ccm_kfdb_shortlist.argtypes = [C.c_int, vp, vp, vp, vp, vp, C.c_int, C.c_float, C.c_int, vp, vp]
        lib.ccm_kfdb_candidates.argtypes = [C.c_int, vp, vp, vp, vp, C.c_int, C.c_float, C.c_int, C.c_int, vp, vp, vp]
        lib.ccm_kfdb_reloc_candidates.argtypes = [C.c_int, vp, vp, vp, C.c_int, vp, vp, vp, vp]
        lib.ccm_kfdb_min_score.argtypes = [C.c_int, vp, vp, C.c_int, vp]; lib.ccm_kfdb_min_score.restype = C.c_float
    if hasattr(lib, "ccm_covis_create"):               # (an older build timed through CCM_HOT_LIB has no covisibility index)
        lib.ccm_covis_create.argtypes = [vp, C.c_int64, C.POINTER(vp)]
        lib.ccm_covis_destroy.argtypes = [vp]; lib.ccm_covis_destroy.restype = None
        lib.ccm_covis_put.argtypes = [vp, C.c_int64, C.c_int, vp, vp]
        lib.ccm_covis_erase.argtypes = [vp, C.c_int64]
        lib.ccm_covis_clear.argtypes = [vp]
        lib.ccm_covis_size.argtypes = [vp]
        lib.ccm_covis_slot.argtypes = [vp, C.c_int64]
        lib.ccm_covis_slots.argtypes = [vp]
        lib.ccm_covis_keys.argtypes = [vp, C.c_int, vp, vp]
        lib.ccm_covis_query.argtypes = [vp, vp, vp, C.c_int, vp, C.c_int, C.c_int, C.POINTER(CovisResult)]
        lib.ccm_covis_lds_features.argtypes = []
        lib.ccm_covis_arena.argtypes = [vp, vp, vp, vp]
        lib.ccm_covis_last_timing.argtypes = [vp, vp]
        lib.ccm_covis_connections.argtypes = [C.c_int, vp, vp, C.c_int, C.c_int, vp, vp]
    _lib = lib
    return lib


def ptr(a):
    if a is None:
        return None
    if isinstance(a, int):
        return C.c_void_p(a)
    return a.ctypes.data_as(C.c_void_p)


class Context:
    """One ccm_ctx: a HIP stream plus device workspaces.  Not thread-safe; one per calling thread."""

    def __init__(self, device: int = 0):
        self.lib = load()
        self.handle = self.lib.ccm_create(int(device), 0)
        if not self.handle:
            raise CcmError(-2, "ccm_create(%d) failed: no such HIP device" % device)
        self.device = device

    def check(self, rc: int) -> int:
        if rc < 0:
            raise CcmError(rc, self.lib.ccm_last_error(self.handle).decode(errors="replace"))
        return rc

    PROF_LABELS = ("k_pyr_resize", "k_fast_score", "k_cell_nms", "k_octree", "k_orient_desc", "k_hamming_bf",
                   "ba_linearize", "ba_dinv_y", "k_sp_schur_blocks", "k_sp_bschur", "k_ba_backsub")

    def host_register(self, arr):
        """Page-lock a numpy array the caller keeps re-using as an input / output buffer (ccm_host_register)."""
        self.check(self.lib.ccm_host_register(self.handle, ptr(arr), C.c_size_t(arr.nbytes)))

    def host_unregister(self, arr):
        self.check(self.lib.ccm_host_unregister(self.handle, ptr(arr)))

    def profile(self, on: bool):
        self.check(self.lib.ccm_profile_enable(self.handle, int(on)))

    def profile_read(self):
        """{kernel: (total_ms, launches)} since the last read (HIP events on this context's stream)."""
        ms = np.zeros(len(self.PROF_LABELS), "f4"); n = np.zeros(len(self.PROF_LABELS), "i4")
        self.check(self.lib.ccm_profile_read(self.handle, ptr(ms), ptr(n)))
        return {k: (float(ms[i]), int(n[i])) for i, k in enumerate(self.PROF_LABELS)}

    def sync(self):
        self.check(self.lib.ccm_sync(self.handle))

    @property
    def stream(self) -> int:
        return self.lib.ccm_stream(self.handle)

    def close(self):
        if getattr(self, "handle", None):
            self.lib.ccm_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


_default_ctx = {}


def default_context(device: int = 0) -> Context:
    if device not in _default_ctx:
        _default_ctx[device] = Context(device)
    return _default_ctx[device]
