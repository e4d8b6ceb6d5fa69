"""The C ABI as Python sees it: the two record dtypes, a ctypes mirror of every struct of include/plp_front.h (tests/test_abi_and_model.py pins
their fields and sizes to the header), and the enums and limits copied from it."""

import ctypes as C

import numpy as np

from ._core import _VP


KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"),
                     ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])
assert KP_DTYPE.itemsize == 28


KL_DTYPE = np.dtype([("angle", "<f4"), ("class_id", "<i4"), ("octave", "<i4"), ("pt_x", "<f4"), ("pt_y", "<f4"), ("response", "<f4"),
                     ("size", "<f4"), ("startPointX", "<f4"), ("startPointY", "<f4"), ("endPointX", "<f4"), ("endPointY", "<f4"),
                     ("sPointInOctaveX", "<f4"), ("sPointInOctaveY", "<f4"), ("ePointInOctaveX", "<f4"), ("ePointInOctaveY", "<f4"),
                     ("lineLength", "<f4"), ("numOfPixels", "<i4")])
assert KL_DTYPE.itemsize == 68
LINE_CAP = 2048


class orb_params_c(C.Structure):
    _fields_ = [("max_num_keypts", C.c_uint32), ("scale_factor", C.c_float), ("num_levels", C.c_uint32),
                ("ini_fast_thr", C.c_uint32), ("min_fast_thr", C.c_uint32), ("mask_rects", C.c_void_p),
                ("n_mask_rects", C.c_int32)]


SEED_ORDER_STABLE, SEED_ORDER_LIBSTDCXX = 0, 1          # plp_seed_order (include/plp_front.h)


class camera_c(C.Structure):
    """plp_camera: camera::perspective intrinsics, distortion, focal_x_baseline"""
    _fields_ = [(k, C.c_double) for k in ("fx", "fy", "cx", "cy", "k1", "k2", "p1", "p2", "k3", "focal_x_baseline")]


CAMERA_PERSPECTIVE, CAMERA_FISHEYE, CAMERA_EQUIRECTANGULAR = 0, 1, 2     # plp_camera_model_type (camera::model_type_t)
CAMERA_MODEL_NAMES = {"perspective": CAMERA_PERSPECTIVE, "fisheye": CAMERA_FISHEYE, "equirectangular": CAMERA_EQUIRECTANGULAR}   # camera/base.cc:81-98


class camera_model_c(C.Structure):
    """plp_camera_model: any of the reference's three camera models"""
    _fields_ = [("model", C.c_int32), ("cols", C.c_int32), ("rows", C.c_int32)] + \
               [(k, C.c_double) for k in ("fx", "fy", "cx", "cy", "k1", "k2", "p1", "p2", "k3", "k4", "focal_x_baseline")]


SETUP_MONOCULAR, SETUP_STEREO, SETUP_RGBD = 0, 1, 2     # camera::setup_type_t (camera/base.h:41-46)


class observe_args_c(C.Structure):
    """plp_observe_args"""
    _fields_ = [("camera", camera_model_c), ("img_bounds", C.c_float * 4), ("ray_cos_thr", C.c_float), ("log_scale_factor", C.c_float),
                ("num_levels", C.c_int32), ("B", C.c_int32), ("m_cap", C.c_int32),
                ("pose", _VP), ("counts", _VP), ("pos_w", _VP), ("obs_mean_normal", _VP), ("min_valid_dist", _VP), ("max_valid_dist", _VP), ("skip", _VP),
                ("out_reproj", _VP), ("out_reproj2", _VP), ("out_x_right", _VP), ("out_level", _VP), ("out_valid", _VP), ("out_num_valid", _VP)]


class last_frame_args_c(C.Structure):
    """plp_last_frame_args"""
    _fields_ = [("camera", camera_model_c), ("img_bounds", C.c_float * 4), ("setup_type", C.c_int32), ("true_baseline", C.c_double),
                ("B", C.c_int32), ("m_cap", C.c_int32),
                ("counts", _VP), ("pose_curr", _VP), ("pose_last", _VP), ("pos_w", _VP), ("skip", _VP), ("keypts", _VP), ("keylines", _VP),
                ("out_reproj", _VP), ("out_reproj2", _VP), ("out_x_right", _VP), ("out_x_right2", _VP), ("out_level", _VP), ("out_angle", _VP),
                ("out_valid", _VP), ("out_direction", _VP), ("out_num_valid", _VP)]


class project_args_c(C.Structure):
    """plp_project_args"""
    _fields_ = [("camera", camera_model_c), ("img_bounds", C.c_float * 4), ("log_scale_factor", C.c_float), ("num_levels", C.c_int32),
                ("B", C.c_int32), ("m_cap", C.c_int32), ("shared_landmarks", C.c_int32), ("dist_mode", C.c_int32), ("ray_test", C.c_int32),
                ("line_dist_mode", C.c_int32),
                ("pose", _VP), ("counts", _VP), ("pos_w", _VP), ("obs_mean_normal", _VP), ("min_valid_dist", _VP), ("max_valid_dist", _VP), ("skip", _VP),
                ("out_reproj_d", _VP), ("out_reproj2_d", _VP), ("out_reproj", _VP), ("out_reproj2", _VP), ("out_x_right", _VP), ("out_x_right2", _VP),
                ("out_level", _VP), ("out_valid", _VP), ("out_status", _VP), ("out_num_valid", _VP)]


PROJECT_DIST_CENTER, PROJECT_DIST_CAMERA = 0, 1           # plp_project_dist_mode
PROJECT_LINE_ENDPOINTS, PROJECT_LINE_MIDPOINT = 0, 1      # plp_project_line_dist_mode
# plp_project_status: where the reference leaves an iteration of the fuse / Sim3 / relocalisation loops
PROJECT_KEPT, PROJECT_SKIPPED, PROJECT_NOT_IN_IMAGE, PROJECT_MIDPOINT_OUT, PROJECT_DISTANCE, PROJECT_RAY = range(6)


class stereo_keylines_args_c(C.Structure):
    """plp_stereo_keylines_args"""
    _fields_ = [("B", C.c_int32), ("cap_left", C.c_int32), ("cap_right", C.c_int32),
                ("keylines_left", _VP), ("counts_left", _VP), ("keylines_right", _VP), ("counts_right", _VP), ("train_idx", _VP), ("dist", _VP),
                ("out_good_match", _VP), ("out_kl_depths", _VP), ("out_kl_x_right", _VP)]


class keylines_3d_args_c(C.Structure):
    """plp_keylines_3d_args"""
    _fields_ = [("camera", camera_model_c), ("setup_type", C.c_int32), ("B", C.c_int32), ("cap", C.c_int32), ("cap_right", C.c_int32),
                ("counts", _VP), ("pose", _VP), ("keylines", _VP), ("kl_depths", _VP), ("good_match", _VP), ("keylines_right", _VP),
                ("counts_right", _VP), ("out_pos_w", _VP), ("out_valid", _VP)]


class median_depth_args_c(C.Structure):
    """plp_median_depth_args"""
    _fields_ = [("F", C.c_int32), ("m_cap", C.c_int32), ("abs_flag", C.c_int32),
                ("pose", _VP), ("pos_w", _VP), ("valid", _VP), ("counts", _VP), ("out_median", _VP), ("out_count", _VP)]


class keyline_pairs_args_c(C.Structure):
    """plp_keyline_pairs_args"""
    _fields_ = [("camera", camera_model_c), ("setup_type", C.c_int32), ("true_baseline", C.c_double),
                ("scale_factors", _VP), ("level_sigma_sq", _VP), ("num_levels", C.c_int32), ("scale_factor", C.c_float),
                ("rays_parallax_deg_thr", C.c_float), ("dist_thr", C.c_float), ("endpoint_thr", C.c_float), ("angle_thr", C.c_float),
                ("skip_occupied", C.c_int32), ("F", C.c_int32), ("cap", C.c_int32), ("kp_cap", C.c_int32),
                ("keylines", _VP), ("counts", _VP), ("line_functions", _VP), ("kl_x_right", _VP), ("kp_depths", _VP), ("kp_counts", _VP),
                ("pose", _VP), ("median_depth", _VP), ("lines_3d", _VP), ("occupied", _VP),
                ("P", C.c_int32), ("G", C.c_int32), ("pairs", _VP), ("group_offsets", _VP), ("train_idx", _VP), ("dist", _VP),
                ("out_match", _VP), ("out_pos_w", _VP), ("out_status", _VP), ("out_occupied_cur", _VP)]


# plp_keyline_pair_status: where the reference leaves an iteration of triangulate_line_with_two_keyframes
(KLP_CREATED, KLP_GATE_DISTANCE, KLP_GATE_ENDPOINTS, KLP_GATE_ANGLE, KLP_OCCUPIED_CUR, KLP_OCCUPIED_NGH, KLP_NO_PARALLAX, KLP_TOO_CLOSE,
 KLP_TOO_LONG, KLP_DEPTH, KLP_REPROJ_MID, KLP_REPROJ_END, KLP_SCALE, KLP_NON_FINITE, KLP_KP_DEPTH_RANGE) = range(15)
KLP_MAPPING = dict(dist_thr=50.0, endpoint_thr=400.0, angle_thr=20.0, skip_occupied=1)       # mapping_module.cc:506, :529, :564
KLP_INITIALIZER = dict(dist_thr=30.0, endpoint_thr=200.0, angle_thr=5.0, skip_occupied=0)    # module/initializer.cc:585-667


class pair_geometry_args_c(C.Structure):
    """plp_keyframe_pair_geometry_args"""
    _fields_ = [("camera", camera_model_c), ("setup_type", C.c_int32), ("true_baseline", C.c_double), ("F", C.c_int32), ("P", C.c_int32),
                ("pose", _VP), ("median_depth", _VP), ("pairs", _VP), ("out_skip", _VP), ("out_epipolar", _VP), ("out_baseline", _VP)]


class keypoint_pairs_args_c(C.Structure):
    """plp_keypoint_pairs_args"""
    _fields_ = [("camera", camera_model_c), ("setup_type", C.c_int32), ("true_baseline", C.c_double),
                ("scale_factors", _VP), ("level_sigma_sq", _VP), ("num_levels", C.c_int32), ("scale_factor", C.c_float),
                ("rays_parallax_deg_thr", C.c_float), ("F", C.c_int32), ("cap", C.c_int32), ("m_cap", C.c_int32), ("P", C.c_int32),
                ("keypts", _VP), ("bearings", _VP), ("x_right", _VP), ("depths", _VP), ("counts", _VP), ("pose", _VP), ("pairs", _VP),
                ("match_q", _VP), ("q_feature", _VP), ("pair_skip", _VP),
                ("out_idx_1", _VP), ("out_pos_w", _VP), ("out_status", _VP), ("occupied_1_io", _VP), ("occupied_2_io", _VP)]


# plp_keypoint_pair_status: where the reference leaves an iteration of triangulate_with_two_keyframes
(KPP_CREATED, KPP_PAIR_SKIPPED, KPP_NO_MATCH, KPP_NO_PARALLAX, KPP_DEPTH, KPP_REPROJ_1, KPP_REPROJ_2, KPP_SCALE, KPP_NON_FINITE,
 KPP_INDEX_RANGE) = range(10)


class landmark_geometry_args_c(C.Structure):
    """plp_landmark_geometry_args"""
    _fields_ = [("F", C.c_int32), ("cap", C.c_int32), ("pose", _VP), ("counts", _VP), ("keypts", _VP), ("keylines", _VP),
                ("scale_factors", _VP), ("num_levels", C.c_int32), ("scale_factors_lsd", _VP), ("num_levels_lsd", C.c_int32), ("L", C.c_int32),
                ("pos_w", _VP), ("ref_kf", _VP), ("skip", _VP), ("obs_offsets", _VP), ("obs_kf", _VP), ("obs_idx", _VP),
                ("out_mean_normal", _VP), ("out_min_valid_dist", _VP), ("out_max_valid_dist", _VP), ("out_status", _VP)]


# plp_landmark_geometry_status: where landmark::update_normal_and_depth / Line::update_information leave a landmark
LG_UPDATED, LG_SKIPPED, LG_NO_OBSERVATIONS, LG_REF_NOT_OBSERVED, LG_INDEX_RANGE, LG_OCTAVE_RANGE = range(6)


class sim3_ransac_args_c(C.Structure):
    """plp_sim3_ransac_args"""
    _fields_ = [("camera", camera_model_c), ("P", C.c_int32), ("n_cap", C.c_int32), ("fix_scale", C.c_int32), ("min_num_inliers", C.c_int32),
                ("iters", C.c_int32), ("seed", C.c_uint64), ("level_sigma_sq_1", _VP), ("level_sigma_sq_2", _VP), ("num_levels", C.c_int32),
                ("counts", _VP), ("valid", _VP), ("pos_w_1", _VP), ("pos_w_2", _VP), ("octave_1", _VP), ("octave_2", _VP), ("pose_1", _VP), ("pose_2", _VP),
                ("samples", _VP), ("out_status", _VP), ("out_num_common", _VP), ("out_rot_12", _VP), ("out_trans_12", _VP), ("out_scale_12", _VP),
                ("out_num_inliers", _VP), ("out_best_iter", _VP), ("out_inliers", _VP), ("out_hyp_inliers", _VP)]


class plane_ransac_args_c(C.Structure):
    """plp_plane_ransac_args"""
    _fields_ = [("mode", C.c_int32), ("P", C.c_int32), ("n_cap", C.c_int32), ("points_per_ransac", C.c_int32), ("min_points_before_ransac", C.c_int32),
                ("iters", C.c_int32), ("inliers_ratio_thr", C.c_double), ("seed", C.c_uint64), ("m_cap", C.c_int32), ("counts", _VP), ("pos_w", _VP),
                ("flags", _VP), ("dist_thresh", _VP), ("error_thresh", _VP), ("best_error_in", _VP), ("equation_in", _VP), ("samples", _VP),
                ("out_status", _VP), ("out_flags", _VP), ("out_equation", _VP), ("out_best_error", _VP), ("out_best_iter", _VP), ("out_last_iter", _VP),
                ("out_num_inliers", _VP), ("out_inliers", _VP), ("out_hyp_residual", _VP), ("out_hyp_inliers", _VP), ("out_hyp_error", _VP)]


class plane_refine_args_c(C.Structure):
    """plp_plane_refine_args"""
    _fields_ = [("M", C.c_int32), ("NP", C.c_int32), ("pos_w", _VP), ("lm_plane", _VP), ("flags", _VP), ("equation", _VP), ("active", _VP),
                ("dist_thresh", _VP), ("out_changed", _VP)]


class plane_refinement_args_c(C.Structure):
    """plp_plane_refinement_args"""
    _fields_ = [("G", C.c_int32), ("NP_cap", C.c_int32), ("n_cap", C.c_int32), ("L", C.c_int32), ("merge_cap", C.c_int32), ("stages", C.c_int32),
                ("points_per_ransac", C.c_int32), ("iters", C.c_int32), ("offset_delta_factor", C.c_int32), ("dot_product_threshold", C.c_double),
                ("seed", C.c_uint64), ("pl_state", _VP), ("pl_equation", _VP), ("pl_best_error", _VP), ("pl_count", _VP), ("pl_lm", _VP), ("pos_w", _VP),
                ("lm_erased", _VP), ("lm_owner", _VP), ("dist_thresh", _VP), ("error_thresh", _VP), ("out_status", _VP), ("out_was_merged", _VP),
                ("out_planes_changed", _VP), ("out_points_changed", _VP), ("out_removed", _VP), ("out_num_merges", _VP), ("out_merges", _VP),
                ("out_num_updates", _VP), ("out_update_status", _VP), ("out_lm_changed", _VP)]


class pnp_ransac_args_c(C.Structure):
    """plp_pnp_ransac_args"""
    _fields_ = [("P", C.c_int32), ("n_cap", C.c_int32), ("min_num_inliers", C.c_int32), ("iters", C.c_int32), ("recompute", C.c_int32),
                ("seed", C.c_uint64), ("scale_factors", _VP), ("num_levels", C.c_int32), ("counts", _VP), ("valid", _VP), ("bearing", _VP), ("pos_w", _VP),
                ("octave", _VP), ("samples", _VP), ("out_status", _VP), ("out_num_matches", _VP), ("out_rot_cw", _VP), ("out_trans_cw", _VP),
                ("out_num_inliers", _VP), ("out_best_iter", _VP), ("out_inliers", _VP), ("out_hyp_inliers", _VP)]


class essential_ransac_args_c(C.Structure):
    """plp_essential_ransac_args"""
    _fields_ = [("P", C.c_int32), ("n_cap", C.c_int32), ("m_cap", C.c_int32), ("iters", C.c_int32), ("recompute", C.c_int32), ("seed", C.c_uint64),
                ("counts_1", _VP), ("counts_2", _VP), ("bearing_1", _VP), ("bearing_2", _VP), ("match", _VP), ("samples", _VP), ("out_status", _VP),
                ("out_num_matches", _VP), ("out_E_21", _VP), ("out_score", _VP), ("out_num_inliers", _VP), ("out_best_iter", _VP), ("out_inliers", _VP),
                ("out_hyp_score", _VP)]


class perspective_ransac_args_c(C.Structure):
    """plp_perspective_ransac_args"""
    _fields_ = [("P", C.c_int32), ("n_cap", C.c_int32), ("m_cap", C.c_int32), ("iters", C.c_int32), ("recompute", C.c_int32), ("seed", C.c_uint64),
                ("counts_1", _VP), ("counts_2", _VP), ("undist_1", _VP), ("undist_2", _VP), ("match", _VP), ("samples_h", _VP), ("samples_f", _VP),
                ("given_H_21", _VP), ("given_H_num_inliers", _VP), ("out_status_h", _VP), ("out_status_f", _VP), ("out_num_matches", _VP), ("out_H_21", _VP),
                ("out_F_21", _VP), ("out_score_h", _VP), ("out_score_f", _VP), ("out_best_iter_h", _VP), ("out_best_iter_f", _VP), ("out_num_inliers_h", _VP),
                ("out_num_inliers_f", _VP), ("out_rel_score_h", _VP), ("out_choice", _VP), ("out_inliers", _VP), ("out_inliers_h", _VP), ("out_inliers_f", _VP),
                ("out_hyp_score_h", _VP), ("out_hyp_score_f", _VP)]


class perspective_pose_args_c(C.Structure):
    """plp_perspective_pose_args"""
    _fields_ = [("camera", camera_model_c), ("img_bounds", C.c_float * 4), ("P", C.c_int32), ("n_cap", C.c_int32), ("m_cap", C.c_int32),
                ("min_num_triangulated", C.c_int32), ("parallax_deg_thr", C.c_float), ("reproj_err_thr", C.c_float), ("counts_1", _VP), ("counts_2", _VP),
                ("in_choice", _VP), ("H_21", _VP), ("F_21", _VP), ("inliers", _VP), ("match", _VP), ("bearing_1", _VP), ("bearing_2", _VP), ("undist_1", _VP),
                ("undist_2", _VP), ("out_status", _VP), ("out_rot_ref_to_cur", _VP), ("out_trans_ref_to_cur", _VP), ("out_hypothesis", _VP), ("out_num_valid", _VP),
                ("out_parallax_deg", _VP), ("out_triangulated_pts", _VP), ("out_is_triangulated", _VP), ("out_hyp_is_triangulated", _VP)]


class two_view_pose_args_c(C.Structure):
    """plp_two_view_pose_args"""
    _fields_ = [("camera", camera_model_c), ("img_bounds", C.c_float * 4), ("P", C.c_int32), ("n_cap", C.c_int32), ("m_cap", C.c_int32),
                ("min_num_triangulated", C.c_int32), ("parallax_deg_thr", C.c_float), ("reproj_err_thr", C.c_float), ("depth_is_positive", C.c_int32),
                ("counts_1", _VP), ("counts_2", _VP), ("in_status", _VP), ("E_21", _VP), ("inliers", _VP), ("match", _VP), ("bearing_1", _VP), ("bearing_2", _VP),
                ("undist_1", _VP), ("undist_2", _VP), ("out_status", _VP), ("out_rot_ref_to_cur", _VP), ("out_trans_ref_to_cur", _VP), ("out_hypothesis", _VP),
                ("out_num_valid", _VP), ("out_parallax_deg", _VP), ("out_triangulated_pts", _VP), ("out_is_triangulated", _VP), ("out_hyp_is_triangulated", _VP)]


class pose_optimize_args_c(C.Structure):
    """plp_pose_optimize_args"""
    _fields_ = [("camera", camera_model_c), ("setup_type", C.c_int32), ("B", C.c_int32), ("n_cap", C.c_int32), ("l_cap", C.c_int32),
                ("num_trials", C.c_int32), ("num_each_iter", C.c_int32), ("pose_stride", C.c_int32), ("inv_level_sigma_sq", _VP), ("num_levels", C.c_int32),
                ("inv_level_sigma_sq_lsd", _VP), ("num_levels_lsd", C.c_int32), ("pose_in", _VP), ("counts", _VP), ("line_counts", _VP), ("valid", _VP),
                ("undist", _VP), ("x_right", _VP), ("pos_w", _VP), ("line_valid", _VP), ("keylines", _VP), ("pos_w_lines", _VP), ("out_status", _VP),
                ("out_pose", _VP), ("out_num_init_obs", _VP), ("out_num_valid", _VP), ("out_outlier", _VP), ("out_outlier_lines", _VP),
                ("out_trial_info", _VP), ("out_trial_chi2", _VP)]


class transform_optimize_args_c(C.Structure):
    """plp_transform_optimize_args"""
    _fields_ = [("camera", camera_model_c), ("fix_scale", C.c_int32), ("num_iter", C.c_int32), ("chi_sq", C.c_float), ("P", C.c_int32), ("n_cap", C.c_int32),
                ("inv_level_sigma_sq_1", _VP), ("inv_level_sigma_sq_2", _VP), ("num_levels", C.c_int32), ("counts", _VP), ("valid", _VP), ("pos_w_1", _VP),
                ("pos_w_2", _VP), ("undist_1", _VP), ("undist_2", _VP), ("pose_1", _VP), ("pose_2", _VP), ("rot_12", _VP), ("trans_12", _VP), ("scale_12", _VP),
                ("out_status", _VP), ("out_num_valid", _VP), ("out_num_inliers", _VP), ("out_rot_12", _VP), ("out_trans_12", _VP), ("out_scale_12", _VP),
                ("out_world_to_1", _VP), ("out_kept", _VP), ("out_round_info", _VP), ("out_round_chi2", _VP)]


class local_ba_args_c(C.Structure):
    """plp_local_ba_args"""
    _fields_ = [("camera", camera_model_c), ("setup_type", C.c_int32), ("num_first_iter", C.c_int32), ("num_second_iter", C.c_int32), ("G", C.c_int32),
                ("F", C.c_int32), ("L", C.c_int32), ("T", C.c_int32), ("kp_stride", C.c_int32), ("pose_stride", C.c_int32), ("inv_level_sigma_sq", _VP),
                ("num_levels", C.c_int32), ("pose", _VP), ("kf_erased", _VP), ("kf_is_origin", _VP), ("undist", _VP), ("x_right", _VP), ("counts", _VP),
                ("pos_w", _VP), ("lm_erased", _VP), ("obs_offsets", _VP), ("obs_kf", _VP), ("obs_idx", _VP), ("kf_local", _VP), ("out_status", _VP),
                ("out_kf_role", _VP), ("out_lm_role", _VP), ("out_pose", _VP), ("out_pos_w", _VP), ("out_outlier", _VP), ("out_round_info", _VP),
                ("out_round_chi2", _VP)]


class local_ba_lines_args_c(C.Structure):
    """plp_local_ba_lines_args"""
    _fields_ = [("points", local_ba_args_c), ("LL", C.c_int32), ("TL", C.c_int32), ("kl_stride", C.c_int32), ("num_levels_lsd", C.c_int32)] + [(k, _VP) for k in (
        "inv_level_sigma_sq_lsd", "keylines", "kl_counts", "pluecker", "line_erased", "obs_offsets_lines", "obs_kf_lines", "obs_idx_lines", "out_line_role",
        "out_pluecker", "out_outlier_lines")]


class global_ba_args_c(C.Structure):
    """plp_global_ba_args"""
    _fields_ = [("camera", camera_model_c), ("setup_type", C.c_int32), ("num_iter", C.c_int32), ("use_huber_kernel", C.c_int32), ("F", C.c_int32), ("L", C.c_int32),
                ("T", C.c_int32), ("kp_stride", C.c_int32), ("pose_stride", C.c_int32), ("inv_level_sigma_sq", _VP), ("num_levels", C.c_int32)] + [(k, _VP) for k in (
        "pose", "kf_erased", "kf_is_origin", "undist", "x_right", "counts", "pos_w", "lm_erased", "obs_offsets", "obs_kf", "obs_idx", "stop", "out_status",
        "out_kf_optimized", "out_lm_optimized", "out_pose", "out_pos_w", "out_info", "out_chi2")]


class loop_ba_propagate_args_c(C.Structure):
    """plp_loop_ba_propagate_args"""
    _fields_ = [("F", C.c_int32), ("L", C.c_int32), ("pose_stride", C.c_int32)] + [(k, _VP) for k in (
        "pose", "kf_erased", "kf_is_origin", "kf_parent", "kf_optimized", "pose_after", "pos_w", "lm_erased", "ref_kf", "lm_optimized", "pos_after", "out_pose",
        "out_pose_before", "out_kf_status", "out_pos_w", "out_lm_status")]


class pose_graph_args_c(C.Structure):
    """plp_pose_graph_args"""
    _fields_ = [(k, C.c_int32) for k in ("G", "F", "pose_stride", "conn_cap", "covis_cap", "edge_cap", "env_cap", "max_iter")] + [(k, _VP) for k in (
        "pose", "kf_erased", "kf_id", "kf_parent", "kf_conn", "kf_conn_w", "kf_n_conn", "kf_covis", "kf_covis_w", "kf_n_covis", "kf_loop_offsets", "kf_loop",
        "loop_kf", "curr_kf", "fix_scale", "pre_offsets", "pre_row", "pre_sim3", "non_offsets", "non_row", "non_sim3", "lc_offsets", "lc_owner", "lc_target",
        "out_status", "out_num_edges", "out_edges", "out_sim3_cw", "out_corrected_wc", "out_pose", "out_info", "out_chi2")]


class correct_landmarks_args_c(C.Structure):
    """plp_correct_landmarks_args"""
    _fields_ = [("L", C.c_int32), ("F", C.c_int32)] + [(k, _VP) for k in ("pos_w", "lm_erased", "ref_kf", "kf_erased", "sim3_cw", "corrected_wc", "out_pos_w",
                                                                         "out_status")]


class local_map_args_c(C.Structure):
    """plp_local_map_args"""
    _fields_ = [("B", C.c_int32), ("F", C.c_int32), ("C", C.c_int32), ("L", C.c_int32), ("LL", C.c_int32), ("T", C.c_int32), ("cap", C.c_int32),
                ("lcap", C.c_int32), ("fcap", C.c_int32), ("flcap", C.c_int32), ("frm_stride", C.c_int32), ("frm_stride_lines", C.c_int32),
                ("max_num_local_keyfrms", C.c_int32), ("k_cap", C.c_int32), ("m_cap", C.c_int32), ("ml_cap", C.c_int32), ("workspace_bytes", C.c_int64),
                ("kf_erased", _VP), ("kf_covis", _VP), ("kf_parent", _VP), ("kf_children_offsets", _VP), ("kf_children", _VP), ("kf_lm", _VP),
                ("kf_counts", _VP), ("kf_lm_lines", _VP), ("kf_kl_counts", _VP), ("obs_offsets", _VP), ("obs_kf", _VP), ("lm_erased", _VP),
                ("lm_erased_lines", _VP), ("frm_lm", _VP), ("frm_counts", _VP), ("frm_lm_lines", _VP), ("frm_kl_counts", _VP), ("out_status", _VP),
                ("out_num_first", _VP), ("out_num_kf", _VP), ("out_local_kf", _VP), ("out_first_weight", _VP), ("out_nearest_kf", _VP),
                ("out_num_lm", _VP), ("out_local_lm", _VP), ("out_held", _VP), ("out_num_lines", _VP), ("out_local_lines", _VP), ("out_held_lines", _VP)]


class cull_keyframes_args_c(C.Structure):
    """plp_cull_keyframes_args"""
    _fields_ = [("F", C.c_int32), ("L", C.c_int32), ("T", C.c_int32), ("cap", C.c_int32), ("kp_stride", C.c_int32), ("G", C.c_int32), ("Cv", C.c_int32),
                ("origin_id", C.c_uint32), ("is_monocular", C.c_int32), ("kf_lm", _VP), ("kf_counts", _VP), ("undist", _VP), ("x_right", _VP),
                ("depths", _VP), ("depth_thr", _VP), ("kf_id", _VP), ("kf_erased", _VP), ("kf_cannot_erase", _VP), ("obs_offsets", _VP), ("obs_kf", _VP),
                ("obs_idx", _VP), ("lm_erased", _VP), ("lm_num_obs", _VP), ("cur_kf", _VP), ("covis_offsets", _VP), ("covis", _VP),
                ("out_num_removed", _VP), ("out_decision", _VP), ("out_num_valid", _VP), ("out_num_redundant", _VP), ("out_kf_removed", _VP),
                ("out_lm_erased", _VP)]


class cull_landmarks_args_c(C.Structure):
    """plp_cull_landmarks_args"""
    _fields_ = [("R", C.c_int32), ("N", C.c_int32), ("L", C.c_int32), ("fresh_offsets", _VP), ("fresh", _VP), ("lm_erased", _VP), ("num_observed", _VP),
                ("num_observable", _VP), ("first_kf_id", _VP), ("num_obs", _VP), ("owning_plane", _VP), ("cur_kf_id", _VP), ("num_obs_thr", _VP),
                ("out_state", _VP), ("out_num_removed", _VP), ("out_num_fresh", _VP), ("out_fresh", _VP)]


class covisibility_update_args_c(C.Structure):
    """plp_covisibility_update_args"""
    _fields_ = [("F", C.c_int32), ("L", C.c_int32), ("T", C.c_int32), ("cap", C.c_int32), ("conn_cap", C.c_int32), ("covis_cap", C.c_int32),
                ("G", C.c_int32), ("kf_lm", _VP), ("kf_counts", _VP), ("obs_offsets", _VP), ("obs_kf", _VP), ("lm_erased", _VP), ("kf_id", _VP),
                ("kf_conn", _VP), ("kf_conn_w", _VP), ("kf_n_conn", _VP), ("kf_covis", _VP), ("kf_covis_w", _VP), ("kf_n_covis", _VP),
                ("kf_parent", _VP), ("kf_parent_unset", _VP), ("owners", _VP), ("out_status", _VP), ("out_nearest", _VP), ("out_max_weight", _VP),
                ("out_touched", _VP)]


class covisibility_erase_args_c(C.Structure):
    """plp_covisibility_erase_args"""
    _fields_ = [("F", C.c_int32), ("conn_cap", C.c_int32), ("covis_cap", C.c_int32), ("kf_conn", _VP), ("kf_conn_w", _VP), ("kf_n_conn", _VP),
                ("kf_covis", _VP), ("kf_covis_w", _VP), ("kf_n_covis", _VP), ("erased", _VP), ("out_status", _VP), ("out_touched", _VP)]


class bow_query_args_c(C.Structure):
    """plp_bow_query_args"""
    _fields_ = [("scoring", C.c_int32), ("n_words", C.c_uint32), ("N", C.c_int32), ("stride", C.c_int32), ("db_word", _VP), ("db_value", _VP),
                ("db_n", _VP), ("db_alive", _VP), ("Q", C.c_int32), ("q_stride", C.c_int32), ("q_word", _VP), ("q_value", _VP), ("q_n", _VP),
                ("reject", _VP), ("min_score", _VP), ("covis_cap", C.c_int32), ("covis", _VP), ("n_covis", _VP), ("out_common", _VP),
                ("out_score", _VP), ("out_total", _VP), ("out_best_kf", _VP), ("out_final", _VP), ("out_n_final", _VP), ("out_max_common", _VP),
                ("out_best_total", _VP), ("out_status", _VP)]


class bow_score_pairs_args_c(C.Structure):
    """plp_bow_score_pairs_args"""
    _fields_ = [("scoring", C.c_int32), ("NA", C.c_int32), ("stride_a", C.c_int32), ("a_word", _VP), ("a_value", _VP), ("a_n", _VP),
                ("NB", C.c_int32), ("stride_b", C.c_int32), ("b_word", _VP), ("b_value", _VP), ("b_n", _VP), ("P", C.c_int32), ("a_row", _VP),
                ("b_row", _VP), ("out_score", _VP)]


# plp_bow_query_status: where acquire_loop_candidates / acquire_relocalization_candidates leave a query
BOW_CANDIDATES, BOW_NO_COMMON_WORDS, BOW_NO_SCORE, BOW_BELOW_MIN_SCORE = range(4)
BOW_BITMAP_WORDS = 1310720          # up to this n_words the count kernel tests bits of an LDS bitmap, above it bisects the query's words
# the outputs of plp_bow_query_*: name -> (per row?, dtype)
BOW_QUERY_OUTPUTS = dict(common=(True, np.uint32), score=(True, np.float32), total=(True, np.float32), best_kf=(True, np.int32), final=(True, np.uint8),
                         n_final=(False, np.int32), max_common=(False, np.uint32), best_total=(False, np.float32), status=(False, np.uint8))


def _struct(cls, fields, ptrs):
    a = cls()
    for k, v in fields.items():
        setattr(a, k, v)
    for k, v in ptrs.items():
        setattr(a, k, v)
    return a


class match_grid_c(C.Structure):
    _fields_ = [("min_x", C.c_float), ("min_y", C.c_float), ("inv_cell_width", C.c_double), ("inv_cell_height", C.c_double),
                ("cols", C.c_int32), ("rows", C.c_int32)]


class match_args_c(C.Structure):
    _fields_ = [("mode", C.c_int32), ("B", C.c_int32), ("n_cap", C.c_int32), ("m_cap", C.c_int32),
                ("t_kps", _VP), ("t_desc", _VP), ("t_x_right", _VP), ("t_occupied", _VP), ("t_angle", _VP), ("t_counts", _VP),
                ("q_valid", _VP), ("q_reproj", _VP), ("q_x_right", _VP), ("q_level", _VP), ("q_angle", _VP), ("q_desc", _VP),
                ("q_has_obs", _VP), ("q_counts", _VP),
                ("margin", C.c_float), ("lowe_ratio", C.c_float), ("direction", C.c_int32), ("check_orientation", C.c_int32),
                ("num_levels", C.c_int32), ("scale_factors", _VP), ("grid", match_grid_c),
                ("t_kl", _VP), ("t_kp_octave", _VP), ("t_x_right2", _VP), ("q_reproj2", _VP), ("q_x_right2", _VP),
                ("is_rgbd", C.c_int32), ("num_levels_lsd", C.c_int32),
                ("q_group", _VP), ("t_group", _VP), ("q_reproj_d", _VP), ("inv_level_sigma_sq", _VP), ("out_query_best", _VP),
                ("hamm_dist_thr", C.c_int32), ("level_window", C.c_int32), ("flags", C.c_int32),
                ("q_reproj2_d", _VP), ("q_bearing", _VP), ("t_bearing", _VP), ("epipolar", _VP),
                ("out_match", _VP), ("out_num", _VP), ("q_desc_stride", C.c_int32), ("t_count_hint", C.c_int32), ("directions", _VP)]


MODE_LANDMARKS, MODE_LAST_FRAME, MODE_BRUTE_FORCE, MODE_LANDMARKS_LINE, MODE_LAST_FRAME_LINE, MODE_BOW, MODE_FUSE, MODE_FUSE_LINE, MODE_TRIANGULATION = 0, 1, 2, 3, 4, 5, 6, 7, 8
FLAG_NO_CHI2, FLAG_SIGNED_LEVEL, FLAG_UNSIGNED_LEVEL, FLAG_MARK_INVALIDATED = 1, 2, 4, 8


class bow_tree_c(C.Structure):
    _fields_ = [("n_nodes", C.c_int32), ("L", C.c_int32), ("child_offset", _VP), ("children", _VP), ("node_desc", _VP), ("node_weight", _VP),
                ("node_word", _VP), ("accumulate", C.c_int32), ("norm", C.c_int32)]


# DBoW2 enums (BowVector.h): WeightingType and ScoringType
TF_IDF, TF, IDF, BINARY = 0, 1, 2, 3
L1_NORM, L2_NORM, CHI_SQUARE, KL, BHATTACHARYYA, DOT_PRODUCT = 0, 1, 2, 3, 4, 5


# plp_sim3_status: where sim3_solver::find_via_ransac leaves a problem
SIM3_OK, SIM3_TOO_FEW_POINTS, SIM3_TOO_FEW_INLIERS = range(3)


# plp_plane_mode, plp_plane_status, the landmark byte and out_flags of plp_plane_ransac_* (include/plp_front.h)
PLANE_CREATE, PLANE_UPDATE = range(2)
PLANE_OK, PLANE_TOO_FEW_POINTS, PLANE_NO_ELIGIBLE, PLANE_NOT_FOUND, PLANE_ERROR_ABOVE_THRESHOLD, PLANE_TOO_FEW_LEFT = range(6)
PLANE_LM_ERASED, PLANE_LM_OWNED = 1, 2
PLANE_FLAG_INVALID, PLANE_FLAG_NEED_REFINEMENT, PLANE_FLAG_GATED = 1, 2, 4
# plp_plane_refinement_status, the state byte of a plane row and the stage mask of plp_plane_refinement_*
PLANE_REFINEMENT_OK, PLANE_REFINEMENT_TOO_FEW_PLANES, PLANE_REFINEMENT_OVERFLOW = range(3)
PLANE_ROW_IN_DB, PLANE_ROW_VALID, PLANE_ROW_NEED_REFINEMENT = 1, 2, 4
PLANE_STAGE_MERGE, PLANE_STAGE_REFINE_PLANES, PLANE_STAGE_REFINE_POINTS, PLANE_STAGE_ALL = 1, 2, 4, 7
PLANE_REFINEMENT_MAX_ROWS = 4096    # NP_cap: the state bytes and the compacted vector of a problem are LDS tables
PLANE_REFINEMENT_NO_UPDATE = 255    # out_update_status of a row no update touched


# plp_pnp_status: where pnp_solver::find_via_ransac leaves a problem
PNP_OK, PNP_TOO_FEW_MATCHES, PNP_TOO_FEW_INLIERS = range(3)


# plp_essential_status: where essential_solver::find_via_ransac leaves a problem
ESSENTIAL_OK, ESSENTIAL_TOO_FEW_MATCHES, ESSENTIAL_INVALID = range(3)
# plp_perspective_status: where homography_solver / fundamental_solver leave a problem; plp_perspective_choice: what initialize::perspective takes
PERSPECTIVE_OK, PERSPECTIVE_TOO_FEW_MATCHES, PERSPECTIVE_INVALID = range(3)
PERSPECTIVE_CHOICE_NONE, PERSPECTIVE_CHOICE_H, PERSPECTIVE_CHOICE_F = range(3)
PERSPECTIVE_POSE_NO_DECOMPOSITION = 5      # plp_perspective_pose_status: beside the TWO_VIEW_* values, homography_solver::decompose returned false
# plp_two_view_status: where bearing_vector::reconstruct_with_E leaves a problem
TWO_VIEW_OK, TWO_VIEW_NO_SOLUTION, TWO_VIEW_TOO_FEW_TRIANGULATED, TWO_VIEW_AMBIGUOUS, TWO_VIEW_SMALL_PARALLAX = range(5)


# plp_pose_opt_status: where pose_optimizer::optimize leaves a frame
POSE_OPT_OK, POSE_OPT_TOO_FEW_OBS = range(2)
# why a trial's optimize() ended (trial_info[..., 3]); 0 = the trial was not run
POSE_OPT_END_ITERATIONS, POSE_OPT_END_TRIES, POSE_OPT_END_RHO_ZERO = 1, 2, 3


# plp_transform_opt_status: where transform_optimizer::optimize leaves a problem
TRANSFORM_OPT_OK, TRANSFORM_OPT_TOO_FEW_INLIERS = range(2)


# plp_local_ba_status / plp_local_ba_kf_role
LOCAL_BA_OK, LOCAL_BA_NO_EDGES, LOCAL_BA_TOO_MANY_FREE = range(3)
LOCAL_BA_KF_NONE, LOCAL_BA_KF_FREE, LOCAL_BA_KF_ORIGIN, LOCAL_BA_KF_FIXED = range(4)
LOCAL_BA_MAX_FREE = 64

# plp_global_ba_status / plp_loop_ba_kf_status / plp_loop_ba_lm_status
GLOBAL_BA_OK, GLOBAL_BA_NO_EDGES, GLOBAL_BA_STOPPED = range(3)
LOOP_BA_KF_NOT_REACHED, LOOP_BA_KF_OPTIMIZED, LOOP_BA_KF_PROPAGATED, LOOP_BA_KF_ERASED = range(4)
LOOP_BA_LM_NO_REF, LOOP_BA_LM_OPTIMIZED, LOOP_BA_LM_MOVED, LOOP_BA_LM_ERASED = range(4)
GLOBAL_BA_MAX_KF, GLOBAL_BA_PANEL, GLOBAL_BA_ROWS = 4096, 32, 64


# plp_pose_graph_status / plp_pose_graph_edge_type / plp_correct_landmark_status
POSE_GRAPH_OK, POSE_GRAPH_NO_EDGES, POSE_GRAPH_ENVELOPE_TOO_LARGE, POSE_GRAPH_TOO_MANY_EDGES, POSE_GRAPH_BAD_LOOP_KF = range(5)
POSE_GRAPH_EDGE_LOOP_CONNECTION, POSE_GRAPH_EDGE_PARENT, POSE_GRAPH_EDGE_LOOP, POSE_GRAPH_EDGE_COVIS = range(1, 5)
CORRECT_LM_OK, CORRECT_LM_ERASED, CORRECT_LM_NO_VERTEX = range(3)
POSE_GRAPH_MAX_KF, POSE_GRAPH_MAX_EDGES, POSE_GRAPH_MAX_ENV, POSE_GRAPH_MAX_PROBLEMS = 1024, 1 << 14, 1 << 16, 16


# plp_local_map_status
LOCAL_MAP_OK, LOCAL_MAP_NO_KEYFRAMES, LOCAL_MAP_KF_OVERFLOW, LOCAL_MAP_LM_OVERFLOW, LOCAL_MAP_LINE_OVERFLOW = range(5)
LOCAL_MAP_MAX_KF = 8192             # F: the weights of a frame are an LDS table of that many counters
LOCAL_MAP_MAX_SLOTS = 8192          # cap, lcap, fcap, flcap
LOCAL_MAP_MAX_FRAMES = 65535        # B


# plp_cull_keyframe_decision and plp_cull_landmark_state
CULL_KF_SKIP_ORIGIN, CULL_KF_SKIP_WINDOW, CULL_KF_KEPT, CULL_KF_REMOVED, CULL_KF_REMOVED_HELD, CULL_KF_ABSENT = range(6)
CULL_HOLD, CULL_DROP, CULL_ERASE = range(3)
CULL_MAX_KF = 8192                  # F: the removed set of a problem is an LDS bitmap
CULL_MAX_SLOTS = 8192               # cap
CULL_MAX_PROBLEMS = 65535           # G


# plp_covisibility_status
COVIS_OK, COVIS_NO_SHARED, COVIS_ROW_ABSENT, COVIS_DUPLICATE, COVIS_OVERFLOW = range(5)
COVIS_MAX_KF = 8192                 # F, G, conn_cap, covis_cap: the weights of an owner are an LDS table
COVIS_MAX_SLOTS = 8192              # cap
COVIS_WEIGHT_THR = 15               # weight_thr_
