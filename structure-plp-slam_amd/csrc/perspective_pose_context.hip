// Host driver + C ABI of the matcher context: map initialisation of the perspective and fisheye cameras, from the chosen matrix to the pose
// (include/plp_front.h: plp_perspective_pose_*; perspective_pose_kernels.hip, perspective_init.hpp)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "matcher_context.hpp"
#include "perspective_init.hpp"

using namespace plp;

extern "C" {

namespace {
plp_status pp_check_args(const plp_perspective_pose_args* a) {
    if (!a) return set_error(PLP_ERR_INVALID_ARG, "NULL argument");
    if (plp_status s = check_camera_model(&a->camera, false)) return s;
    if (a->camera.model != PLP_CAMERA_PERSPECTIVE && a->camera.model != PLP_CAMERA_FISHEYE)
        return set_error(PLP_ERR_UNSUPPORTED, "the equirectangular camera has no camera matrix (initialize/perspective.cc:176-199)");
    if (a->P < 0 || a->n_cap < 0 || a->m_cap < 0 || a->min_num_triangulated < 0)
        return set_error(PLP_ERR_INVALID_ARG, "P, n_cap, m_cap and min_num_triangulated must not be negative");
    if (a->n_cap > kPerspMaxSlots) return set_error(PLP_ERR_UNSUPPORTED, "more than 8192 slots per problem");
    if (a->P > 65535) return set_error(PLP_ERR_UNSUPPORTED, "more than 65535 problems in one call");
    if (a->P == 0 || a->n_cap == 0) return PLP_OK;
    if (!a->in_choice || !a->H_21 || !a->F_21 || !a->inliers || !a->match || !a->bearing_1 || !a->undist_1 || (a->m_cap > 0 && (!a->bearing_2 || !a->undist_2)))
        return set_error(PLP_ERR_INVALID_ARG, "in_choice, H_21, F_21, inliers, match, bearing_1, bearing_2, undist_1, undist_2 are required");
    if (!a->out_status || !a->out_rot_ref_to_cur || !a->out_trans_ref_to_cur || !a->out_hypothesis || !a->out_num_valid || !a->out_parallax_deg ||
        !a->out_triangulated_pts || !a->out_is_triangulated)
        return set_error(PLP_ERR_INVALID_ARG, "every output but out_hyp_is_triangulated is required");
    return PLP_OK;
}

PerspPoseArgs pp_args(const plp_perspective_pose_args* a) {
    PerspPoseArgs B{};
    TvArgs& A = B.tv;
    set_camera(A, a->camera);
    for (int i = 0; i < 4; ++i) A.bounds[i] = a->img_bounds[i];
    A.P = a->P; A.n_cap = a->n_cap; A.m_cap = a->m_cap; A.min_num_triangulated = a->min_num_triangulated; A.depth_is_positive = 1;   // perspective.cc:141, :166
    A.parallax_deg_thr = a->parallax_deg_thr; A.reproj_err_thr = a->reproj_err_thr;
    A.inliers = a->inliers; A.match = a->match; A.counts_1 = a->counts_1; A.counts_2 = a->counts_2; A.bearing_1 = a->bearing_1;
    A.bearing_2 = a->bearing_2; A.undist_1 = a->undist_1; A.undist_2 = a->undist_2;
    A.out_status = a->out_status; A.out_rot = a->out_rot_ref_to_cur; A.out_trans = a->out_trans_ref_to_cur; A.out_hypothesis = a->out_hypothesis;
    A.out_num_valid = a->out_num_valid; A.out_parallax_deg = a->out_parallax_deg; A.out_pts = a->out_triangulated_pts;
    A.out_is_triangulated = a->out_is_triangulated; A.out_hyp_is_triangulated = a->out_hyp_is_triangulated;
    B.in_choice = a->in_choice; B.H_21 = a->H_21; B.F_21 = a->F_21;
    return B;
}

// the arrays of the call; the rooms are the points and flags of the hypotheses
extern "C++" template <class R> void pp_plan(R& r, plp_matcher* c, PerspPoseArgs& B) {
    TvArgs& A = B.tv;
    const size_t P = (size_t)A.P, M = (size_t)A.n_cap, M2 = (size_t)A.m_cap, NH = (size_t)kPerspMaxHyp;
    r.in(B.in_choice, P); r.in(B.H_21, P * 9); r.in(B.F_21, P * 9); r.in(A.inliers, P * M); r.in(A.match, P * M); r.in(A.counts_1, P); r.in(A.counts_2, P);
    r.in(A.bearing_1, P * M * 3); r.in(A.bearing_2, P * M2 * 3); r.in(A.undist_1, P * M); r.in(A.undist_2, P * M2);
    r.out(A.out_status, P, false); r.out(A.out_rot, P * 9, false); r.out(A.out_trans, P * 3, false); r.out(A.out_hypothesis, P, false);
    r.out(A.out_num_valid, P * NH, false); r.out(A.out_parallax_deg, P * NH, false); r.out(A.out_pts, P * M * 3); r.out(A.out_is_triangulated, P * M);
    r.out(A.out_hyp_is_triangulated, P * NH * M);
    r.room(c->persp_pts, B.ctx_pts, P * NH * M * 3); r.room(c->persp_flag, B.ctx_flag, P * NH * M);
}

// check_pose (base.cc:123-243) of the host build for problem p under a pose of 12 doubles: num_valid, parallax_deg, per slot the point and the flag
extern "C++" template <int MODEL> int pp_model_check_pose(const TvArgs& A, int p, const double* pose12, const double* coef, float& parallax_deg, double* pts, uint8_t* flag) {
    const int count_1 = clamp_count(A.counts_1, p, A.n_cap), count_2 = clamp_count(A.counts_2, p, A.m_cap);
    const size_t row = (size_t)p * A.n_cap;
    double c[3];
    tv_center(pose12, c);
    std::vector<uint32_t> keys;
    for (int slot = 0; slot < count_1; ++slot) {
        double pos[3] = {0.0, 0.0, 0.0};
        int code = 0;
        const int m = A.match[row + slot];
        if (A.inliers[row + slot] != 0 && m >= 0 && m < count_2) {
            const size_t s2 = (size_t)p * A.m_cap + m;
            float cosp = 0.0f;
            code = tv_check<MODEL>(A, pose12, c, A.bearing_1 + 3 * (row + slot), A.bearing_2 + 3 * s2, A.undist_1[row + slot].x, A.undist_1[row + slot].y,
                                   A.undist_2[s2].x, A.undist_2[s2].y, pos, cosp);
            if (code >= kTvValidSmall) keys.push_back(tv_key(cosp));
        }
        const bool tri = code == kTvValid;
        flag[slot] = tri ? 1 : 0;
        for (int i = 0; i < 3; ++i) pts[3 * (size_t)slot + i] = tri ? pos[i] : 0.0;
    }
    const int num = (int)keys.size();
    parallax_deg = 0.0f;
    if (num > 0) {                                                  // :230-236
        std::sort(keys.begin(), keys.end());
        parallax_deg = tv_parallax_deg(tv_unkey(keys[(size_t)std::min(kTvSortRank, num - 1)]), coef);
    }
    return num;
}

// one problem of the host build
void pp_model_problem(const PerspPoseArgs& B, int p, const double* coef) {
    const TvArgs& A = B.tv;
    const int count_1 = clamp_count(A.counts_1, p, A.n_cap);
    const size_t row = (size_t)p * A.n_cap, M = (size_t)A.n_cap;
    const int choice = B.in_choice[p];
    PerspPoseWs w;
    double poses[kPerspMaxHyp * 12] = {0};
    std::vector<double> pts(kPerspMaxHyp * M * 3, 0.0);
    std::vector<uint8_t> flag(kPerspMaxHyp * M, 0);
    int num_valid[kPerspMaxHyp] = {0}, chosen = -1, status = PLP_TWO_VIEW_NO_SOLUTION, nh = 0;
    float parallax[kPerspMaxHyp] = {0.0f};
    persp_cam_matrix(A, w.K);
    if (choice == PLP_PERSPECTIVE_CHOICE_H) {
        nh = hom_decompose(B.H_21 + (size_t)9 * p, w, poses) ? 8 : 0;
        status = PLP_PERSPECTIVE_POSE_NO_DECOMPOSITION;
    } else if (choice == PLP_PERSPECTIVE_CHOICE_F) {
        fund_decompose(B.F_21 + (size_t)9 * p, w, poses);
        nh = 4;
    }
    for (int h = 0; h < nh; ++h)
        num_valid[h] = A.model == PLP_CAMERA_PERSPECTIVE
                           ? pp_model_check_pose<PLP_CAMERA_PERSPECTIVE>(A, p, poses + 12 * h, coef, parallax[h], pts.data() + h * M * 3, flag.data() + h * M)
                           : pp_model_check_pose<PLP_CAMERA_FISHEYE>(A, p, poses + 12 * h, coef, parallax[h], pts.data() + h * M * 3, flag.data() + h * M);
    if (nh > 0) status = persp_select(num_valid, parallax, nh, A.min_num_triangulated, A.parallax_deg_thr, chosen);
    A.out_status[p] = (uint8_t)status;
    A.out_hypothesis[p] = chosen;
    for (int i = 0; i < 9; ++i) A.out_rot[(size_t)9 * p + i] = chosen >= 0 ? persp_out(poses[12 * chosen + i]) : 0.0;
    for (int i = 0; i < 3; ++i) A.out_trans[(size_t)3 * p + i] = chosen >= 0 ? persp_out(poses[12 * chosen + 9 + i]) : 0.0;
    for (int h = 0; h < kPerspMaxHyp; ++h) { A.out_num_valid[(size_t)kPerspMaxHyp * p + h] = num_valid[h]; A.out_parallax_deg[(size_t)kPerspMaxHyp * p + h] = parallax[h]; }
    for (int slot = 0; slot < count_1; ++slot) {
        const bool tri = chosen >= 0 && flag[chosen * M + slot] != 0;
        A.out_is_triangulated[row + slot] = tri ? 1 : 0;
        for (int i = 0; i < 3; ++i) A.out_pts[3 * (row + slot) + i] = tri ? pts[(chosen * M + slot) * 3 + i] : 0.0;
        if (A.out_hyp_is_triangulated)
            for (int h = 0; h < kPerspMaxHyp; ++h) A.out_hyp_is_triangulated[((size_t)p * kPerspMaxHyp + h) * M + slot] = flag[h * M + slot];
    }
}
}  // namespace

plp_status plp_perspective_pose_device(plp_matcher* c, const plp_perspective_pose_args* a, void* hip_stream) {
    if (!c) return set_error(PLP_ERR_INVALID_ARG, "ctx is NULL");
    if (plp_status s = pp_check_args(a)) return s;
    if (a->P == 0 || a->n_cap == 0) return PLP_OK;
    return device_call(c, hip_stream, pp_args(a), pp_plan<DeviceRooms>, launch_perspective_pose);
}

plp_status plp_perspective_pose_host(plp_matcher* c, const plp_perspective_pose_args* a) {
    if (!c) return set_error(PLP_ERR_INVALID_ARG, "ctx is NULL");
    if (plp_status s = pp_check_args(a)) return s;
    if (a->P == 0 || a->n_cap == 0) return PLP_OK;
    return host_call(c, pp_args(a), pp_plan<Stage>, launch_perspective_pose);
}

// the host builds (no HIP call)
int32_t plp_model_perspective_pose_host(const plp_perspective_pose_args* a) {
    if (pp_check_args(a) != PLP_OK) return -1;
    if (a->P == 0 || a->n_cap == 0) return a->P;
    const PerspPoseArgs B = pp_args(a);
    double coef[kPgCoefs];
    pg_coef_init(coef);
    for (int p = 0; p < B.tv.P; ++p) pp_model_problem(B, p, coef);
    return B.tv.P;
}

int32_t plp_model_homography_decompose_host(const double* H_21, const double* cam_matrix, int32_t n, uint8_t* out_ok, double* out_rots, double* out_trans) {
    if (n < 0 || (n > 0 && (!H_21 || !cam_matrix || !out_ok || !out_rots || !out_trans))) return -1;
    PerspPoseWs w;
    for (int32_t i = 0; i < n; ++i) {
        double poses[kPerspMaxHyp * 12] = {0};
        for (int e = 0; e < 9; ++e) w.K[e] = cam_matrix[e];
        const bool ok = hom_decompose(H_21 + 9 * (size_t)i, w, poses);
        out_ok[i] = ok ? 1 : 0;
        for (int h = 0; h < 8; ++h) {
            for (int e = 0; e < 9; ++e) out_rots[(8 * (size_t)i + h) * 9 + e] = ok ? poses[12 * h + e] : 0.0;
            for (int e = 0; e < 3; ++e) out_trans[(8 * (size_t)i + h) * 3 + e] = ok ? poses[12 * h + 9 + e] : 0.0;
        }
    }
    return n;
}

}  // extern "C"
