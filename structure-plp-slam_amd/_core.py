"""Paths, status codes, the loader of libplp_front.so with the table of every symbol include/plp_front.h declares, and the build.  The
library handle lives here and nowhere else."""

import ctypes as C
import os
import pathlib
import subprocess


_PKG = pathlib.Path(__file__).resolve().parent
ROOT = _PKG.parent
LIB_PATH = pathlib.Path(os.environ["PLP_FRONT_LIB"]).resolve() if os.environ.get("PLP_FRONT_LIB") else _PKG / "libplp_front.so"   # PLP_FRONT_LIB: an experiment's build (tools/build_variant.sh)


PLP_OK, PLP_ERR_INVALID_ARG, PLP_ERR_NO_DEVICE, PLP_ERR_HIP, PLP_ERR_CAPACITY, PLP_ERR_OVERFLOW, PLP_ERR_UNSUPPORTED = range(7)


class PlpError(RuntimeError):
    def __init__(self, status, detail):
        super().__init__(f"plp_front status {status}: {detail}")
        self.status = status


def build(verbose=False):
    """Compile libplp_front.so for gfx950 (hipcc cross-compiles without a GPU)."""
    r = subprocess.run(["make", "-j", str(min(8, os.cpu_count() or 1)), "-C", str(_PKG / "csrc")], capture_output=not verbose, text=True)
    if r.returncode != 0:
        raise RuntimeError("building libplp_front.so failed:\n" + (r.stdout or "") + (r.stderr or ""))
    return LIB_PATH


_lib = None

# every symbol include/plp_front.h declares: (name, restype, argtypes)
_VP, _I32, _SZ = C.c_void_p, C.c_int32, C.c_size_t
_API = [
    ("plp_strerror", C.c_char_p, [C.c_int]),
    ("plp_last_error", C.c_char_p, []),
    ("plp_version", C.c_int, []),
    ("plp_device_count", C.c_int, []),
    ("plp_orb_default_params", None, [_VP]),
    ("plp_orb_create", C.c_int, [_VP, C.c_int, _VP]),
    ("plp_orb_destroy", None, [_VP]),
    ("plp_orb_set_param", C.c_int, [_VP, C.c_int, C.c_double]),
    ("plp_orb_get_param", C.c_int, [_VP, C.c_int, _VP]),
    ("plp_orb_get_tables", C.c_int, [_VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    ("plp_orb_extract", C.c_int, [_VP, _VP, _I32, _I32, _SZ, _VP, _SZ, _VP, _VP, _I32, _VP]),
    ("plp_orb_extract_batch_device", C.c_int, [_VP, _VP, _I32, _I32, _I32, _SZ, _SZ, _VP, _SZ, _SZ, _VP, _VP, _I32, _VP, _VP]),
    ("plp_orb_last_batch_status", C.c_int, [_VP]),
    ("plp_orb_set_profiling", C.c_int, [_VP, _I32]),
    ("plp_orb_get_stage_times", C.c_int, [_VP, _VP, _VP]),
    ("plp_orb_pyramid_level_size", C.c_int, [_VP, _I32, _VP, _VP]),
    ("plp_orb_pyramid_host", C.c_int, [_VP, _I32, _I32, _VP, _SZ]),
    ("plp_orb_debug_read", C.c_int, [_VP, C.c_int, _I32, _I32, _VP, _SZ, _VP]),
    ("plp_model_quadtree_host", _I32, [_VP, _I32, _I32, _I32, C.c_uint32, _VP]),
    ("plp_model_quadtree_rank_sort_host", _I32, [_VP, _I32, _I32, _VP]),
    ("plp_model_sincos_host", _I32, [_VP, C.c_int64, _VP, _VP, _VP]),
    ("plp_model_index_sort_host", _I32, [_VP, _I32, _I32, _VP]),
    ("plp_model_null_vector4_host", _I32, [_VP, _I32, _VP, _VP]),
    ("plp_line_create", C.c_int, [C.c_int, _VP]),
    ("plp_line_destroy", None, [_VP]),
    ("plp_line_extract", C.c_int, [_VP, _VP, _I32, _I32, _SZ, _VP, _VP, _VP, _I32, _VP]),
    ("plp_line_extract_batch_device", C.c_int, [_VP, _VP, _I32, _I32, _I32, _SZ, _SZ, _VP, _VP, _VP, _I32, _VP, _VP]),
    ("plp_line_last_batch_status", C.c_int, [_VP]),
    ("plp_line_set_profiling", C.c_int, [_VP, _I32]),
    ("plp_line_set_grow_waves", C.c_int, [_VP, _I32]),
    ("plp_line_set_seed_order", C.c_int, [_VP, _I32]),
    ("plp_line_get_seed_order", C.c_int, [_VP, _VP]),
    ("plp_line_trim", C.c_int, [_VP]),
    ("plp_model_seed_introsort_host", _I32, [_VP, C.c_int64, _I32, C.c_uint32]),
    ("plp_seed_introsort_debug", C.c_int, [_I32, _VP, C.c_int64, _I32, C.c_uint32, _I32, _VP]),
    ("plp_seed_sort_tile_ranks", _I32, [C.c_int64, C.c_int64, _I32, _VP]),
    ("plp_line_get_stage_times", C.c_int, [_VP, _VP, _VP]),
    ("plp_line_debug_read", C.c_int, [_VP, C.c_int, _I32, _VP, _SZ, _VP]),
    ("plp_line_scaled_size", C.c_int, [_VP, _VP, _VP]),
    ("plp_line_debug_grow_profile", C.c_int, [_VP, _VP]),
    ("plp_matcher_create", C.c_int, [C.c_int, _VP]),
    ("plp_matcher_destroy", None, [_VP]),
    ("plp_match_device", C.c_int, [_VP, _VP, _VP]),
    ("plp_match_host", C.c_int, [_VP, _VP]),
    ("plp_match_debug_counters", C.c_int, [_VP, _VP]),
    ("plp_match_debug_plan", C.c_int, [_VP, _VP]),
    ("plp_match_area_host", C.c_int, [_VP, _VP, _VP, _I32, _VP, _VP, _I32, _VP, _VP, _I32, C.c_float, _I32, _VP, _VP]),
    ("plp_convert_to_grayscale_device", C.c_int, [_VP, _VP, _I32, _I32, C.c_size_t, C.c_size_t, _I32, _I32, _I32, _VP, C.c_size_t, C.c_size_t, _VP]),
    ("plp_convert_to_true_depth_device", C.c_int, [_VP, _VP, _I32, _I32, _I32, C.c_size_t, C.c_size_t, C.c_double, _I32, _VP, C.c_size_t, C.c_size_t, _VP]),
    ("plp_rectify_map_device", C.c_int, [_VP, _VP, _VP, _I32, _VP, _VP, _I32, _I32, _VP, _VP, C.c_size_t, _VP]),
    ("plp_rectify_map_fisheye_device", C.c_int, [_VP, _VP, _VP, _VP, _VP, _I32, _I32, _VP, _VP, C.c_size_t, _VP]),
    ("plp_remap_linear_device", C.c_int, [_VP, _VP, _I32, _I32, C.c_size_t, C.c_size_t, _VP, _VP, C.c_size_t, _I32, _I32, _I32, _VP, C.c_size_t, C.c_size_t, _VP]),
    ("plp_bow_vocab_create", C.c_int, [C.c_int, _VP, _VP]),
    ("plp_bow_vocab_destroy", None, [_VP]),
    ("plp_bow_transform_device", C.c_int, [_VP, _VP, _VP, _I32, _I32, _I32, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    ("plp_bow_transform_host", C.c_int, [_VP, _VP, _I32, _I32, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    ("plp_bow_query_device", C.c_int, [_VP, _VP, _VP]),
    ("plp_bow_query_host", C.c_int, [_VP, _VP]),
    ("plp_bow_score_pairs_device", C.c_int, [_VP, _VP, _VP]),
    ("plp_bow_score_pairs_host", C.c_int, [_VP, _VP]),
    ("plp_model_bow_score_host", C.c_double, [_VP, _VP, _I32, _VP, _VP, _I32]),
    ("plp_color_vote_device", C.c_int, [_VP, _VP, _I32, _I32, C.c_size_t, C.c_size_t, _VP, _VP, _VP, _I32, _I32, _I32, _VP, _VP]),
    ("plp_landmark_descriptor_device", C.c_int, [_VP, _VP, _VP, _I32, _VP, _VP]),
    ("plp_landmark_descriptor_host", C.c_int, [_VP, _VP, _VP, _I32, _VP]),
    ("plp_post_extract_device", C.c_int, [_VP, _VP, _VP, _VP, _I32, _I32, _VP, _I32, _I32, C.c_size_t, C.c_size_t, _VP, _VP, _VP, _VP, _VP, _VP, _I32, _VP, _VP, _VP]),
    ("plp_post_extract_host", C.c_int, [_VP, _VP, _VP, _I32, _VP, _I32, _I32, C.c_size_t, _VP, _VP, _VP, _VP, _VP, _I32, _VP, _VP]),
    ("plp_post_extract_model_device", C.c_int, [_VP, _VP, _VP, _VP, _I32, _I32, _VP, _I32, _I32, C.c_size_t, C.c_size_t, _VP, _VP, _VP, _VP, _VP, _VP, _I32, _VP, _VP, _VP]),
    ("plp_post_extract_model_host", C.c_int, [_VP, _VP, _VP, _I32, _VP, _I32, _I32, C.c_size_t, _VP, _VP, _VP, _VP, _VP, _I32, _VP, _VP]),
    ("plp_observe_landmarks_device", C.c_int, [_VP, _VP, _VP]),
    ("plp_observe_landmarks_host", C.c_int, [_VP, _VP]),
    ("plp_observe_landmark_lines_device", C.c_int, [_VP, _VP, _VP]),
    ("plp_observe_landmark_lines_host", C.c_int, [_VP, _VP]),
    ("plp_project_last_frame_device", C.c_int, [_VP, _VP, _VP]),
    ("plp_project_last_frame_host", C.c_int, [_VP, _VP]),
    ("plp_project_last_frame_lines_device", C.c_int, [_VP, _VP, _VP]),
    ("plp_project_last_frame_lines_host", C.c_int, [_VP, _VP]),
    ("plp_project_landmarks_device", C.c_int, [_VP, _VP, _VP]),
    ("plp_project_landmarks_host", C.c_int, [_VP, _VP]),
    ("plp_project_landmark_lines_device", C.c_int, [_VP, _VP, _VP]),
    ("plp_project_landmark_lines_host", C.c_int, [_VP, _VP]),
    ("plp_stereo_keylines_device", C.c_int, [_VP, _VP, _VP]),
    ("plp_stereo_keylines_host", C.c_int, [_VP, _VP]),
    ("plp_keylines_3d_device", C.c_int, [_VP, _VP, _VP]),
    ("plp_keylines_3d_host", C.c_int, [_VP, _VP]),
    ("plp_median_depth_device", C.c_int, [_VP, _VP, _VP]),
    ("plp_median_depth_host", C.c_int, [_VP, _VP]),
    ("plp_triangulate_keyline_pairs_device", C.c_int, [_VP, _VP, _VP]),
    ("plp_triangulate_keyline_pairs_host", C.c_int, [_VP, _VP]),
    ("plp_keyframe_pair_geometry_device", C.c_int, [_VP, _VP, _VP]),
    ("plp_keyframe_pair_geometry_host", C.c_int, [_VP, _VP]),
    ("plp_triangulate_keypoint_pairs_device", C.c_int, [_VP, _VP, _VP]),
    ("plp_triangulate_keypoint_pairs_host", C.c_int, [_VP, _VP]),
    ("plp_landmark_geometry_device", C.c_int, [_VP, _VP, _VP]),
    ("plp_landmark_geometry_host", C.c_int, [_VP, _VP]),
    ("plp_landmark_line_geometry_device", C.c_int, [_VP, _VP, _VP]),
    ("plp_landmark_line_geometry_host", C.c_int, [_VP, _VP]),
    ("plp_model_landmark_geometry_host", _I32, [_VP, _I32]),
    ("plp_sim3_ransac_device", C.c_int, [_VP, _VP, _VP]),
    ("plp_sim3_ransac_host", C.c_int, [_VP, _VP]),
    ("plp_model_sim3_ransac_host", _I32, [_VP]),
    ("plp_model_horn_sim3_host", _I32, [_VP, _VP, _I32, _I32, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    ("plp_model_sym_eig4_max_host", _I32, [_VP, _I32, _VP, _VP]),
    ("plp_model_sim3_draw_host", _I32, [C.c_uint64, _I32, _I32, _I32, _I32, _VP]),
    ("plp_pnp_ransac_device", C.c_int, [_VP, _VP, _VP]),
    ("plp_pnp_ransac_host", C.c_int, [_VP, _VP]),
    ("plp_model_pnp_ransac_host", _I32, [_VP]),
    ("plp_model_epnp_host", _I32, [_VP, _VP, _VP, _I32, _VP, _VP, _VP, _VP, _VP]),
    ("plp_model_sym_jacobi_host", _I32, [_VP, _I32, _I32, _VP, _VP, _VP]),
    ("plp_model_lstsq6_host", _I32, [_VP, _VP, _I32, _I32, _VP, _VP]),
    ("plp_model_rot_from_abt_host", _I32, [_VP, _I32, _VP, _VP]),
    ("plp_model_pnp_draw_host", _I32, [C.c_uint64, _I32, _I32, _I32, _I32, _VP]),
    ("plp_model_pnp_thresholds_host", _I32, [_VP, _I32, _VP]),
    ("plp_essential_ransac_device", C.c_int, [_VP, _VP, _VP]),
    ("plp_essential_ransac_host", C.c_int, [_VP, _VP]),
    ("plp_model_essential_ransac_host", _I32, [_VP]),
    ("plp_model_essential_fit_host", _I32, [_VP, _VP, _VP, _I32, _VP, _VP]),
    ("plp_model_essential_check_host", _I32, [_VP, _VP, _VP, _I32, _I32, _VP, _I32, _VP, _VP, _VP]),
    ("plp_model_essential_draw_host", _I32, [C.c_uint64, _I32, _I32, _I32, _I32, _VP]),
    ("plp_two_view_pose_device", C.c_int, [_VP, _VP, _VP]),
    ("plp_two_view_pose_host", C.c_int, [_VP, _VP]),
    ("plp_model_two_view_pose_host", _I32, [_VP]),
    ("plp_model_essential_decompose_host", _I32, [_VP, _I32, _VP, _VP]),
    ("plp_model_check_pose_host", _I32, [_VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    ("plp_perspective_ransac_device", C.c_int, [_VP, _VP, _VP]),
    ("plp_perspective_ransac_host", C.c_int, [_VP, _VP]),
    ("plp_model_perspective_ransac_host", _I32, [_VP]),
    ("plp_model_normalize_keypoints_host", _I32, [_VP, _I32, _VP, _VP, _VP]),
    ("plp_model_homography_fit_host", _I32, [_VP, _VP, _VP, _I32, _VP, _VP]),
    ("plp_model_fundamental_fit_host", _I32, [_VP, _VP, _VP, _I32, _VP, _VP]),
    ("plp_model_homography_check_host", _I32, [_VP, _VP, _VP, _I32, _I32, _VP, _I32, _VP, _VP, _VP]),
    ("plp_model_fundamental_check_host", _I32, [_VP, _VP, _VP, _I32, _I32, _VP, _I32, _VP, _VP, _VP]),
    ("plp_model_perspective_draw_host", _I32, [_I32, C.c_uint64, _I32, _I32, _I32, _I32, _VP]),
    ("plp_perspective_pose_device", C.c_int, [_VP, _VP, _VP]),
    ("plp_perspective_pose_host", C.c_int, [_VP, _VP]),
    ("plp_model_perspective_pose_host", _I32, [_VP]),
    ("plp_model_homography_decompose_host", _I32, [_VP, _VP, _I32, _VP, _VP, _VP]),
    ("plp_pose_optimize_device", C.c_int, [_VP, _VP, _VP]),
    ("plp_pose_optimize_host", C.c_int, [_VP, _VP]),
    ("plp_model_pose_optimize_host", _I32, [_VP]),
    ("plp_model_pose_linearize_host", _I32, [_VP, _I32, _VP, _VP, _VP, _VP, _VP]),
    ("plp_model_se3_exp_host", _I32, [_VP, _VP, _I32, _VP]),
    ("plp_model_chol6_host", _I32, [_VP, _VP, _VP, _I32, _VP, _VP]),
    ("plp_model_pose_sincos_host", _I32, [_VP, _I32, _VP, _VP]),
    ("plp_transform_optimize_device", C.c_int, [_VP, _VP, _VP]),
    ("plp_transform_optimize_host", C.c_int, [_VP, _VP]),
    ("plp_model_transform_optimize_host", _I32, [_VP]),
    ("plp_model_transform_linearize_host", _I32, [_VP, _VP, _VP, _VP]),
    ("plp_model_sim3_exp_host", _I32, [_VP, _VP, _I32, _I32, _VP]),
    ("plp_model_chol7_host", _I32, [_VP, _VP, _VP, _I32, _VP, _VP]),
    ("plp_model_pose_exp_host", _I32, [_VP, _I32, _VP]),
    ("plp_local_ba_device", C.c_int, [_VP, _VP, _VP]),
    ("plp_local_ba_host", C.c_int, [_VP, _VP]),
    ("plp_model_local_ba_host", _I32, [_VP]),
    ("plp_local_map_device", C.c_int, [_VP, _VP, _VP]),
    ("plp_local_map_host", C.c_int, [_VP, _VP]),
    ("plp_model_local_map_host", _I32, [_VP]),
    ("plp_model_local_ba_linearize_host", _I32, [_VP, _I32, _VP, _VP, _VP, _VP, _VP, _VP]),
    ("plp_model_local_ba_solve_host", _I32, [_I32, _I32, _I32, _VP, _VP, _VP, _VP, _VP, C.c_double, _VP, _VP]),
    ("plp_model_inv3_host", _I32, [_VP, _I32, _VP, _VP]),
    ("plp_local_ba_lines_device", C.c_int, [_VP, _VP, _VP]),
    ("plp_local_ba_lines_host", C.c_int, [_VP, _VP]),
    ("plp_model_local_ba_lines_host", _I32, [_VP]),
    ("plp_model_line_oplus_host", _I32, [_VP, _VP, _I32, _VP]),
    ("plp_model_local_ba_lines_linearize_host", _I32, [_VP, _I32, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    ("plp_model_local_ba_lines_solve_host", _I32, [_I32] * 5 + [_VP] * 9 + [C.c_double, _VP, _VP, _VP]),
    ("plp_lbd_match_1nn_host", C.c_int, [_VP, _VP, _I32, _VP, _I32, _VP, _VP]),
    ("plp_lbd_match_1nn_device", C.c_int, [_VP, _VP, _VP, _I32, _VP, _VP, _I32, _I32, _VP, _VP, _VP]),
    ("plp_stereo_compute", C.c_int, [_VP, _VP, _VP, _I32, _VP, _I32, _VP, _VP, C.c_float, C.c_float, _VP, _VP]),
    ("plp_stereo_compute_batch_device", C.c_int, [_VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _I32, _I32, C.c_float, C.c_float, _VP, _VP, _VP]),
    ("plp_hamming_matrix_device", C.c_int, [_VP, _VP, _I32, _VP, _I32, _VP, _VP]),
    ("plp_hamming_matrix_host", C.c_int, [_VP, _VP, _I32, _VP, _I32, _VP]),
    ("plp_replay_point_queries_device", C.c_int, [_VP, _VP, _I32, _I32, _I32, C.c_float, C.c_float, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    ("plp_pack_rows_device", C.c_int, [_VP, _VP, _I32, _I32, _I32, _VP, _VP, _I32, _VP]),
    ("plp_replay_line_queries_device", C.c_int, [_VP, _VP, _I32, _I32, _I32, C.c_float, C.c_float, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _I32, _VP, _VP]),
    ("plp_plane_ransac_device", C.c_int, [_VP, _VP, _VP]),
    ("plp_plane_ransac_host", C.c_int, [_VP, _VP]),
    ("plp_model_plane_ransac_host", _I32, [_VP]),
    ("plp_model_plane_fit_host", _I32, [_VP, _I32, _VP, _VP, _I32, _VP, _VP, _VP]),
    ("plp_model_plane_draw_host", _I32, [C.c_uint64, _I32, _I32, _I32, _I32, _I32, _VP]),
    ("plp_plane_refine_points_device", C.c_int, [_VP, _VP, _VP]),
    ("plp_plane_refine_points_host", C.c_int, [_VP, _VP]),
    ("plp_model_plane_refine_points_host", _I32, [_VP]),
    ("plp_plane_refinement_device", C.c_int, [_VP, _VP, _VP]),
    ("plp_plane_refinement_host", C.c_int, [_VP, _VP]),
    ("plp_model_plane_refinement_host", _I32, [_VP]),
    ("plp_cull_keyframes_device", C.c_int, [_VP, _VP, _VP]),
    ("plp_cull_keyframes_host", C.c_int, [_VP, _VP]),
    ("plp_model_cull_keyframes_host", _I32, [_VP]),
    ("plp_cull_landmarks_device", C.c_int, [_VP, _VP, _VP]),
    ("plp_cull_landmarks_host", C.c_int, [_VP, _VP]),
    ("plp_model_cull_landmarks_host", _I32, [_VP]),
    ("plp_covisibility_update_device", C.c_int, [_VP, _VP, _VP]),
    ("plp_covisibility_update_host", C.c_int, [_VP, _VP]),
    ("plp_model_covisibility_update_host", _I32, [_VP]),
    ("plp_covisibility_erase_device", C.c_int, [_VP, _VP, _VP]),
    ("plp_covisibility_erase_host", C.c_int, [_VP, _VP]),
    ("plp_model_covisibility_erase_host", _I32, [_VP]),
    ("plp_pose_graph_optimize_device", C.c_int, [_VP, _VP, _VP]),
    ("plp_pose_graph_optimize_host", C.c_int, [_VP, _VP]),
    ("plp_model_pose_graph_optimize_host", _I32, [_VP]),
    ("plp_model_pose_graph_edges_host", _I32, [_VP]),
    ("plp_model_sim3_log_host", _I32, [_VP, _I32, _VP]),
    ("plp_model_pose_log_host", _I32, [_VP, _I32, _VP]),
    ("plp_model_pose_acos_host", _I32, [_VP, _I32, _VP]),
    ("plp_model_block_chol7_host", _I32, [_I32, _VP, _VP, _VP, C.c_double, _VP]),
    ("plp_correct_landmarks_device", C.c_int, [_VP, _VP, _VP]),
    ("plp_correct_landmarks_host", C.c_int, [_VP, _VP]),
    ("plp_model_correct_landmarks_host", _I32, [_VP]),
    ("plp_trim_line_endpoints_device", C.c_int, [_VP, _VP, _VP]),
    ("plp_trim_line_endpoints_host", C.c_int, [_VP, _VP]),
    ("plp_model_trim_line_endpoints_host", _I32, [_VP]),
    ("plp_correct_landmark_lines_device", C.c_int, [_VP, _VP, _VP]),
    ("plp_correct_landmark_lines_host", C.c_int, [_VP, _VP]),
    ("plp_model_correct_landmark_lines_host", _I32, [_VP]),
    ("plp_loop_ba_propagate_lines_device", C.c_int, [_VP, _VP, _VP]),
    ("plp_loop_ba_propagate_lines_host", C.c_int, [_VP, _VP]),
    ("plp_model_loop_ba_propagate_lines_host", _I32, [_VP]),
    ("plp_global_ba_device", C.c_int, [_VP, _VP, _VP]),
    ("plp_global_ba_host", C.c_int, [_VP, _VP]),
    ("plp_model_global_ba_host", _I32, [_VP]),
    ("plp_loop_ba_propagate_device", C.c_int, [_VP, _VP, _VP]),
    ("plp_loop_ba_propagate_host", C.c_int, [_VP, _VP]),
    ("plp_model_loop_ba_propagate_host", _I32, [_VP]),
    ("plp_model_chol_dense_host", _I32, [_I32, _VP, _VP, C.c_double, _VP, _VP]),
    ("plp_chol_dense_host", C.c_int, [_VP, _I32, _VP, _VP, C.c_double, _VP, _VP]),
]


def api_symbols():
    return [n for n, _, _ in _API]


def lib():
    """Load libplp_front.so; raises if it has not been built (no fallback path exists)."""
    global _lib
    if _lib is None:
        if not LIB_PATH.exists():
            raise FileNotFoundError(f"{LIB_PATH} is missing: run __graft_entry__.build() (hipcc --offload-arch=gfx950)")
        try:
            # PyTorch bundles its own HIP/HSA runtime; a process must hold exactly one.  Loading torch first
            # makes libplp_front.so (NEEDED libamdhip64.so.7) bind to that copy instead of /opt/rocm's.
            import torch  # noqa: F401
        except ImportError:
            pass
        L = C.CDLL(str(LIB_PATH))
        for name, res, args in _API:
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def _check(status):
    if status != PLP_OK:
        raise PlpError(status, lib().plp_last_error().decode())


def _p(a):
    return a.ctypes.data_as(C.c_void_p)
