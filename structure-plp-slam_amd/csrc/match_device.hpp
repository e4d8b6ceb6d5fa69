// Problem descriptor shared by the matcher kernels and their host driver (array form of the
// reference's point matchers; see include/plp_front.h for the field meanings).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/plp_front.h"

namespace plp {

constexpr int kMatchK = 8;          // best candidates kept per query by k_match_topk

struct StagedTarget { float x, y; uint32_t packed; uint32_t t; };   // packed = octave | cell col << 8 | cell row << 16

struct MatchProblem {
    int mode;                        // plp_match_mode
    int n_cap, m_cap;                // per-problem strides of the target / query arrays
    int q_desc_stride;               // rows between two problems in q_desc (= m_cap unless the caller's queries overlap, plp_front.h)
    // targets = key points of the current frame (B x n_cap)
    const plp_keypoint* t_kps;       // undist_keypts_ (NULL in brute-force mode)
    const uint8_t* t_desc;           // descriptors_, 32 B rows
    const float* t_x_right;          // stereo_x_right_ (NULL: none)
    const uint8_t* t_occupied;       // key point already holds an observed landmark (NULL: none)
    const float* t_angle;            // brute-force mode: keypts_1[.].angle
    const int32_t* t_counts;         // per-problem n (NULL: n_cap)
    const plp_keyline* t_kl;         // line modes: key lines (replaces t_kps)
    const int32_t* t_kp_octave;      // line modes: the key-point octave read with a line index (reference quirk)
    const float* t_x_right2;         // line modes: second stereo coordinate
    const float* q_reproj2;          // line modes: reprojected end point
    const float* q_x_right2;
    int is_rgbd, num_levels_lsd;
    const int32_t* q_group; const int32_t* t_group;   // BOW mode: node id per feature
    const double* q_reproj_d;        // FUSE mode: f64 reprojection
    float inv_level_sigma_sq[16];    // FUSE mode
    int32_t* out_query_best;         // FUSE mode: B x m_cap
    int hamm_dist_thr, level_window, flags;
    const double* q_reproj2_d;       // FUSE_LINE
    const double* q_bearing; const double* t_bearing; const double* epipolar;   // TRIANGULATION
    // queries = landmarks / last-frame key points / key-frame key points (B x m_cap), reference order
    const uint8_t* q_valid;          // NULL: all valid
    const float* q_reproj;           // x, y
    const float* q_x_right;
    const int32_t* q_level;
    const float* q_angle;
    const uint8_t* q_desc;
    const uint8_t* q_has_obs;        // NULL: every accepted query blocks its key point
    const int32_t* q_counts;         // per-problem m (NULL: m_cap)
    // parameters
    float margin, lowe_ratio;
    int direction, check_orientation, num_levels;
    const int32_t* directions;       // LAST_FRAME[_LINE]: per-problem direction (NULL: `direction` for all)
    float scale_factors[16];
    float grid_min_x, grid_min_y;
    double inv_cell_w, inv_cell_h;
    int grid_cols, grid_rows;
    // scratch + outputs
    uint32_t* klist;                 // B x m_cap x kMatchK, packed distance<<20 | octave<<16 | target (sorted)
    uint32_t* klist2;                // B x m_cap x kMatchK: ranks kMatchK+1 .. 2 kMatchK of a query with more than kMatchK candidates (k_match_topk_cells only)
    int32_t* kcount;                 // B x m_cap
    int32_t* claim;                  // B x m_cap
    int32_t* full_list;              // B x m_cap
    StagedTarget* sorted;            // B x n_cap: free in-grid targets bucketed by grid row
    float* sorted_xr;                // B x n_cap
    uint16_t* cell_start;            // B x 4104: first position of every grid cell in `sorted`
    int sorted_valid;                // set by launch_match when k_match_prep ran
    int lds_targets;                 // targets of a frame k_match_topk_cells holds in LDS (<= n_cap; plp_match_args.t_count_hint), the rest is read from `sorted`
    int32_t* dbg;                    // 4 counters: exact rescans, resolve rounds (accumulated)
    int32_t* out_match;              // B x n_cap: query index per key point, -1 = none
    int32_t* out_num;                // B
};

struct MihRanks { uint8_t rank[256]; };   // enumeration rank of an 8-bit flip pattern inside its popcount class (Mihasher::query)
void launch_lbd_match_1nn(hipStream_t st, const uint8_t* q, const int32_t* q_counts, int nq_cap, const uint8_t* t, const int32_t* t_counts,
                          int nt_cap, const MihRanks& R, int32_t* out_idx, int32_t* out_dist, int B);
// The kernels of one matcher call: a top-k kernel and a resolve kernel, chosen from the mode, B, n_cap, the LDS staging size and the grid shape.
// plan_match() is the one place that decides; launch_match() launches what it returns and plp_match_debug_plan reports it.
enum MatchFamily { kFamAny = 0, kFamLine = 1, kFamGroup = 2, kFamPoint = 3, kFamGrid = 4 };   // kFamGrid: the two windowed point modes after k_match_prep
enum MatchTopk { kTopkNone = 0, kTopkCells = 1, kTopkLds = 2, kTopkLanes = 3, kTopkGeneric = 4, kTopkFuse = 5 };
enum MatchResolve { kResolveNone = 0, kResolveSorted = 1, kResolveGeneric = 2 };
struct MatchPlan {
    int topk;        // MatchTopk: k_match_prep + k_match_topk_cells, k_match_topk_lds, k_match_topk_lanes<family>, k_match_topk<family>, k_match_fuse
    int family;      // MatchFamily of the templated kernels (kFamGrid: the sorted resolve; kFamAny: k_match_fuse)
    int qpb;         // queries per workgroup of k_match_topk_cells / k_match_topk_lds, 0 for the others
    int resolve;     // MatchResolve: k_match_resolve_sorted, k_match_resolve_generic<family>, none (fuse modes)
    size_t staged;   // dynamic LDS of the top-k kernel (cells, lds)
};
// reads P.mode, n_cap, m_cap, lds_targets, t_x_right (NULL or not), grid_cols, grid_rows
MatchPlan plan_match(const MatchProblem& P, int B);
void launch_match(hipStream_t st, const MatchProblem& P, int B);
hipError_t configure_match_kernels();   // per-device kernel attributes (dynamic LDS of k_match_resolve)
struct AreaArgs {
    const plp_keypoint *kps1, *kps2; const uint8_t *desc1, *desc2; int n1, n2;
    float grid_min_x, grid_min_y; double inv_cell_w, inv_cell_h; int grid_cols, grid_rows;
    float* prev_pts; float margin, lowe_ratio; int check_orientation;
    int32_t* matched_2_in_1; int32_t* num_matches;
    uint32_t* scratch;   // n2 x 2 words: matched distance, matched idx_1
};
void launch_match_area(hipStream_t st, const AreaArgs& A);
void launch_hamming_matrix(hipStream_t st, const uint8_t* q, int nq, const uint8_t* t, int nt, uint16_t* dist);

// post-extract step (post_kernels.hip)
struct PostArgs {
    double fx, fy, cx, cy;            // camera::perspective doubles (bearings)
    double fx_f, fy_f, cx_f, cy_f;    // the float-rounded matrix cv::undistortPoints sees
    double k[5];                      // float-rounded k1, k2, p1, p2, k3
    double fxb;                       // focal_x_baseline_
    const plp_keypoint* kps; const int32_t* counts; int cap;
    const float* depth; size_t depth_step, depth_frame_stride;
    plp_keypoint* undist; double* bearings; float* x_right; float* depths;
    const plp_keyline* kl; const int32_t* kl_counts; int kl_cap; float* kl_depths; float* kl_x_right;
    int model;                        // plp_camera_model_type: which instantiation of k_post_extract runs (0 = perspective)
    float cols_f, rows_f;             // equirectangular: (float)cols_, (float)rows_ (unsigned int -> float in pt.x / cols_)
};
void launch_post_extract(hipStream_t st, const PostArgs& A, int B);

// local-landmark visibility (observe_kernels.hip, plp_observe_landmark[_line]s_*)
struct ObserveArgs {
    int model;                        // plp_camera_model_type: which instantiation runs
    double fx, fy, cx, cy, fxb;       // camera::perspective / fisheye doubles (reproject_to_image)
    double cols_d, rows_d;            // equirectangular: cols_, rows_ (unsigned int -> double)
    float bounds[4];                  // img_bounds_ min_x, max_x, min_y, max_y
    float ray_cos_thr, log_sf;
    int num_levels, m_cap;
    const double* pose; const int32_t* counts; const double* pos_w; const double* normal;
    const float* min_dist; const float* max_dist; const uint8_t* skip;
    float* reproj; float* reproj2; float* x_right; int32_t* level; uint8_t* valid; int32_t* num_valid;
    // last-frame queries (plp_project_last_frame[_lines]_*): pose = the current frame's, the last frame's features instead of the landmark tests
    const double* pose_last; const plp_keypoint* kps; const plp_keyline* kl;
    float* angle; float* x_right2; int32_t* direction;
    int setup_type; double true_baseline;
};
// all four return the first error of their calls (the points launchers zero num_valid before their kernels add to it)
hipError_t launch_observe_points(hipStream_t st, const ObserveArgs& A, int B);
hipError_t launch_observe_lines(hipStream_t st, const ObserveArgs& A, int B);
hipError_t launch_last_frame_points(hipStream_t st, const ObserveArgs& A, int B);
hipError_t launch_last_frame_lines(hipStream_t st, const ObserveArgs& A, int B);
// fuse, Sim3 and relocalisation queries (project_kernels.hip, plp_project_landmark[_line]s_*); the camera fields are named as ObserveArgs
// names them: reproject<MODEL> (reproject.hpp) reads either
struct ProjectArgs {
    int model;
    double fx, fy, cx, cy, fxb;
    double cols_d, rows_d;
    float bounds[4];
    float log_sf;
    int num_levels, m_cap;
    int shared, dist_mode, ray_test, line_dist_mode;
    const double* pose; const int32_t* counts; const double* pos_w; const double* normal;
    const float* min_dist; const float* max_dist; const uint8_t* skip;
    double* reproj_d; double* reproj2_d; float* reproj; float* reproj2; float* x_right; float* x_right2;
    int32_t* level; uint8_t* valid; uint8_t* status; int32_t* num_valid;
};
// both return the first error of their calls (the points launcher zeroes num_valid before its kernel adds to it)
hipError_t launch_project_points(hipStream_t st, const ProjectArgs& A, int B);
hipError_t launch_project_lines(hipStream_t st, const ProjectArgs& A, int B);
// stereo key-line association (plp_stereo_keylines_*, stereo_line_kernels.hip): left / right key lines, the 1-NN result (left = query)
struct StereoKeylineArgs {
    int cap_l, cap_r;
    const plp_keyline* kl_l; const int32_t* counts_l; const plp_keyline* kl_r; const int32_t* counts_r;
    const int32_t* train_idx; const int32_t* dist;
    int32_t* good; float* depths; float* x_right;
};
// 3-D key lines (plp_keylines_3d_*, stereo_line_kernels.hip): camera::perspective doubles, fx_inv_ / fy_inv_ = 1.0 / fx, 1.0 / fy as the
// constructor forms them (perspective.cc:42)
struct Keylines3dArgs {
    double fx, fy, cx, cy, fxb, fx_inv, fy_inv;
    int setup_type, cap, cap_r;
    const int32_t* counts; const double* pose; const plp_keyline* kl; const float* kl_depths;
    const int32_t* good_match; const plp_keyline* kl_r; const int32_t* counts_r;
    double* pos_w; uint8_t* valid;
};
// both return the first error of their launch
hipError_t launch_stereo_keylines(hipStream_t st, const StereoKeylineArgs& A, int B);
hipError_t launch_keylines_3d(hipStream_t st, const Keylines3dArgs& A, int B);
// key-frame pair line triangulation (plp_median_depth_* / plp_triangulate_keyline_pairs_*, keyline_pair_kernels.hip)
struct MedianDepthArgs {
    int m_cap, abs_flag;
    const double* pose; const double* pos_w; const uint8_t* valid; const int32_t* counts;
    float* median; int32_t* count;
};
struct KeylinePairArgs {
    double fx, fy, cx, cy;            // camera::perspective doubles
    double half_baseline;             // true_baseline_ / 2.0
    int setup_type, num_levels, skip_occupied;
    int F, cap, kp_cap, P, G;
    float cos_thr;                    // cos_rays_parallax_thr_, the float of cos(thr * M_PI / 180.0)
    float dist_thr, endpoint_thr, angle_thr;
    float ratio_factor;               // 2.0f * scale_factor_
    float scale_factors[16], level_sigma_sq[16];
    const plp_keyline* kl; const int32_t* counts; const double* line_fn; const float* x_right; const float* kp_depths; const int32_t* kp_counts;
    const double* pose; const float* median; const double* lines_3d; const uint8_t* occupied;
    const int32_t* pairs; const int32_t* group_offsets; const int32_t* train_idx; const int32_t* dist;
    int32_t* out_match; double* out_pos_w; uint8_t* out_status; uint8_t* out_occ_cur;
};
// both return the first error of their launches (the second: the geometry kernel, then the resolve kernel, on the same stream)
hipError_t launch_median_depth(hipStream_t st, const MedianDepthArgs& A, int F);
hipError_t launch_keyline_pairs(hipStream_t st, const KeylinePairArgs& A);
// key-frame pair point triangulation (plp_keyframe_pair_geometry_* / plp_triangulate_keypoint_pairs_*, keypoint_pair_kernels.hip)
struct PairGeometryArgs {
    int model, setup_type, F, P;
    double true_baseline;
    const double* pose; const float* median; const int32_t* pairs;
    uint8_t* out_skip; double* out_epipolar; double* out_baseline;
};
struct KeypointPairArgs {
    int model;                        // plp_camera_model_type: which instantiation runs
    double fx, fy, cx, cy, fxb;       // the camera fields reproject<MODEL> (reproject.hpp) reads, named as ObserveArgs names them
    double cols_d, rows_d;
    float bounds[4];                  // read by reproject<MODEL> for a result this step ignores: zero
    double fx_inv, fy_inv;            // 1.0 / fx, 1.0 / fy as the constructors form them (perspective.cc:42, fisheye.cc:42)
    double half_baseline;             // true_baseline_ / 2.0
    int setup_type, num_levels;
    int F, cap, m_cap, P, p0;         // p0: the first pair of this launch
    float cos_thr;                    // cos_rays_parallax_thr_, the float of cos(thr * M_PI / 180.0)
    float ratio_factor;               // 2.0f * scale_factor_
    float scale_factors[16], level_sigma_sq[16];
    const plp_keypoint* kps; const double* bearings; const float* x_right; const float* depths; const int32_t* counts;
    const double* pose; const int32_t* pairs; const int32_t* match_q; const int32_t* q_feature; const uint8_t* pair_skip;
    int32_t* out_idx_1; double* out_pos_w; uint8_t* out_status; uint8_t* occ1; uint8_t* occ2;
};
// both return the first error of their launches
hipError_t launch_pair_geometry(hipStream_t st, const PairGeometryArgs& A);
hipError_t launch_keypoint_pairs(hipStream_t st, const KeypointPairArgs& A);
void launch_to_gray(hipStream_t st, const uint8_t* src, int rows, int cols, size_t src_step, size_t src_fs, int channels, int bgr, int B, uint8_t* dst,
                    size_t dst_step, size_t dst_fs);
void launch_to_depth(hipStream_t st, const void* src, int is_u16, int rows, int cols, size_t src_step, size_t src_fs, float scale, int B, float* dst,
                     size_t dst_step, size_t dst_fs);
void launch_color_vote(hipStream_t st, const uint8_t* mask, int rows, int cols, size_t step, size_t fs, const plp_keypoint* undist, const uint8_t* valid,
                       const int32_t* counts, int cap, int B, int check3, int32_t* labels);
void launch_landmark_descriptor(hipStream_t st, const uint8_t* descs, const int32_t* offsets, int L, int32_t* best_idx);
struct RectifyArgs {
    double ir[9];                     // (K_rect * R)^-1
    double d[12];                     // k1 k2 p1 p2 k3 k4 k5 k6 s1 s2 s3 s4
    double fx, fy, u0, v0;            // the unrectified camera
    int rows, cols;
    float* map_x; float* map_y; size_t map_step;
};
void launch_rectify_map(hipStream_t st, const RectifyArgs& A, bool fisheye);
void launch_remap_linear(hipStream_t st, const uint8_t* src, int rows, int cols, size_t step, size_t fs, const float* map_x, const float* map_y,
                         size_t map_step, int drows, int dcols, int B, uint8_t* dst, size_t dst_step, size_t dst_fs);

}  // namespace plp
