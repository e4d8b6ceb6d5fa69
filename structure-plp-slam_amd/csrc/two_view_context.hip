// Host driver + C ABI of the matcher context: map initialisation, from the essential matrix to the pose (include/plp_front.h:
// plp_two_view_pose_*; two_view_kernels.hip, two_view.hpp)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "matcher_context.hpp"
#include "two_view.hpp"

using namespace plp;

extern "C" {

namespace {
plp_status tv_check_args(const plp_two_view_pose_args* a) {
    if (!a) return set_error(PLP_ERR_INVALID_ARG, "NULL argument");
    if (plp_status s = check_camera_model(&a->camera, false)) return s;
    if (a->P < 0 || a->n_cap < 0 || a->m_cap < 0 || a->min_num_triangulated < 0)
        return set_error(PLP_ERR_INVALID_ARG, "P, n_cap, m_cap and min_num_triangulated must not be negative");
    if (a->n_cap > kEssMaxSlots) return set_error(PLP_ERR_UNSUPPORTED, "more than 8192 slots per problem");
    if (a->P > 65535) return set_error(PLP_ERR_UNSUPPORTED, "more than 65535 problems in one call");
    if (a->P == 0 || a->n_cap == 0) return PLP_OK;
    if (!a->E_21 || !a->inliers || !a->match || !a->bearing_1 || !a->undist_1 || (a->m_cap > 0 && (!a->bearing_2 || !a->undist_2)))
        return set_error(PLP_ERR_INVALID_ARG, "E_21, inliers, match, bearing_1, bearing_2, undist_1, undist_2 are required");
    if (!a->out_status || !a->out_rot_ref_to_cur || !a->out_trans_ref_to_cur || !a->out_hypothesis || !a->out_num_valid || !a->out_parallax_deg ||
        !a->out_triangulated_pts || !a->out_is_triangulated)
        return set_error(PLP_ERR_INVALID_ARG, "every output but out_hyp_is_triangulated is required");
    return PLP_OK;
}

TvArgs tv_args(const plp_two_view_pose_args* a) {
    TvArgs A{};
    set_camera(A, a->camera);
    for (int i = 0; i < 4; ++i) A.bounds[i] = a->img_bounds[i];
    A.P = a->P; A.n_cap = a->n_cap; A.m_cap = a->m_cap; A.min_num_triangulated = a->min_num_triangulated; A.depth_is_positive = a->depth_is_positive != 0;
    A.parallax_deg_thr = a->parallax_deg_thr; A.reproj_err_thr = a->reproj_err_thr;
    A.E_21 = a->E_21; A.inliers = a->inliers; A.match = a->match; A.counts_1 = a->counts_1; A.counts_2 = a->counts_2; A.bearing_1 = a->bearing_1;
    A.bearing_2 = a->bearing_2; A.undist_1 = a->undist_1; A.undist_2 = a->undist_2; A.in_status = a->in_status;
    A.out_status = a->out_status; A.out_rot = a->out_rot_ref_to_cur; A.out_trans = a->out_trans_ref_to_cur; A.out_hypothesis = a->out_hypothesis;
    A.out_num_valid = a->out_num_valid; A.out_parallax_deg = a->out_parallax_deg; A.out_pts = a->out_triangulated_pts;
    A.out_is_triangulated = a->out_is_triangulated; A.out_hyp_is_triangulated = a->out_hyp_is_triangulated;
    return A;
}

// the arrays of the call; the rooms are the points and flags of the four hypotheses
extern "C++" template <class R> void tv_plan(R& r, plp_matcher* c, TvArgs& A) {
    const size_t P = (size_t)A.P, M = (size_t)A.n_cap, M2 = (size_t)A.m_cap;
    r.in(A.E_21, P * 9); r.in(A.inliers, P * M); r.in(A.match, P * M); r.in(A.counts_1, P); r.in(A.counts_2, P); r.in(A.bearing_1, P * M * 3);
    r.in(A.bearing_2, P * M2 * 3); r.in(A.undist_1, P * M); r.in(A.undist_2, P * M2); r.in(A.in_status, P);
    r.out(A.out_status, P, false); r.out(A.out_rot, P * 9, false); r.out(A.out_trans, P * 3, false); r.out(A.out_hypothesis, P, false);
    r.out(A.out_num_valid, P * 4, false); r.out(A.out_parallax_deg, P * 4, false); r.out(A.out_pts, P * M * 3); r.out(A.out_is_triangulated, P * M);
    r.out(A.out_hyp_is_triangulated, P * 4 * M);
    r.room(c->tv_pts, A.ctx_pts, P * 4 * M * 3); r.room(c->tv_flag, A.ctx_flag, P * 4 * M);
}

// check_pose (base.cc:123-243) of the host build for problem p under (R, t) given as 12 doubles: num_valid, parallax_deg, and per slot the
// point, the flag and the code (pts / flag / code: count_1 entries written, may be NULL)
extern "C++" template <int MODEL> int tv_model_check_pose(const TvArgs& A, int p, const double* pose12, const double* coef, float& parallax_deg, double* pts, uint8_t* flag,
                                                          uint8_t* codes) {
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
        if (flag) flag[slot] = tri ? 1 : 0;
        if (pts)
            for (int i = 0; i < 3; ++i) pts[3 * (size_t)slot + i] = tri ? pos[i] : 0.0;
        if (codes) codes[slot] = (uint8_t)code;
    }
    const int num = (int)keys.size();
    parallax_deg = 0.0f;
    if (num > 0) {                                                  // :230-236
        std::sort(keys.begin(), keys.end());
        parallax_deg = tv_parallax_deg(tv_unkey(keys[(size_t)std::min(kTvSortRank, num - 1)]), coef);
    }
    return num;
}
int tv_model_check_pose_any(const TvArgs& A, int p, const double* pose12, const double* coef, float& parallax_deg, double* pts, uint8_t* flag, uint8_t* codes) {
    if (A.model == PLP_CAMERA_PERSPECTIVE) return tv_model_check_pose<PLP_CAMERA_PERSPECTIVE>(A, p, pose12, coef, parallax_deg, pts, flag, codes);
    if (A.model == PLP_CAMERA_FISHEYE) return tv_model_check_pose<PLP_CAMERA_FISHEYE>(A, p, pose12, coef, parallax_deg, pts, flag, codes);
    return tv_model_check_pose<PLP_CAMERA_EQUIRECTANGULAR>(A, p, pose12, coef, parallax_deg, pts, flag, codes);
}

// one problem of the host build
void tv_model_problem(const TvArgs& A, int p, const double* coef) {
    const int count_1 = clamp_count(A.counts_1, p, A.n_cap);
    const size_t row = (size_t)p * A.n_cap, M = (size_t)A.n_cap;
    const bool solved = !(A.in_status && A.in_status[p] != 0);
    double ws[kTvDecomposeDoubles], rots[18], trans[3], pose12[12];
    std::vector<double> pts(4 * M * 3, 0.0);
    std::vector<uint8_t> flag(4 * M, 0);
    int num_valid[4] = {0, 0, 0, 0}, chosen = -1, status = PLP_TWO_VIEW_NO_SOLUTION;
    float parallax[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (solved) {
        tv_decompose(A.E_21 + (size_t)9 * p, ws, rots, trans);
        for (int h = 0; h < 4; ++h) {
            tv_hypothesis(rots, trans, h, pose12);
            num_valid[h] = tv_model_check_pose_any(A, p, pose12, coef, parallax[h], pts.data() + h * M * 3, flag.data() + h * M, nullptr);
        }
        status = tv_select(num_valid, parallax, A.min_num_triangulated, A.parallax_deg_thr, chosen);
    }
    A.out_status[p] = (uint8_t)status;
    A.out_hypothesis[p] = chosen;
    if (chosen >= 0) tv_hypothesis(rots, trans, chosen, pose12);
    for (int i = 0; i < 9; ++i) A.out_rot[(size_t)9 * p + i] = chosen >= 0 ? pose12[i] : 0.0;
    for (int i = 0; i < 3; ++i) A.out_trans[(size_t)3 * p + i] = chosen >= 0 ? pose12[9 + i] : 0.0;
    for (int h = 0; h < 4; ++h) { A.out_num_valid[(size_t)4 * p + h] = num_valid[h]; A.out_parallax_deg[(size_t)4 * p + h] = parallax[h]; }
    for (int slot = 0; slot < count_1; ++slot) {
        const bool tri = chosen >= 0 && flag[chosen * M + slot] != 0;
        A.out_is_triangulated[row + slot] = tri ? 1 : 0;
        for (int i = 0; i < 3; ++i) A.out_pts[3 * (row + slot) + i] = tri ? pts[(chosen * M + slot) * 3 + i] : 0.0;
        if (A.out_hyp_is_triangulated)
            for (int h = 0; h < 4; ++h) A.out_hyp_is_triangulated[((size_t)p * 4 + h) * M + slot] = flag[h * M + slot];
    }
}
}  // namespace

plp_status plp_two_view_pose_device(plp_matcher* c, const plp_two_view_pose_args* a, void* hip_stream) {
    if (!c) return set_error(PLP_ERR_INVALID_ARG, "ctx is NULL");
    if (plp_status s = tv_check_args(a)) return s;
    if (a->P == 0 || a->n_cap == 0) return PLP_OK;
    return device_call(c, hip_stream, tv_args(a), tv_plan<DeviceRooms>, launch_two_view_pose);
}

plp_status plp_two_view_pose_host(plp_matcher* c, const plp_two_view_pose_args* a) {
    if (!c) return set_error(PLP_ERR_INVALID_ARG, "ctx is NULL");
    if (plp_status s = tv_check_args(a)) return s;
    if (a->P == 0 || a->n_cap == 0) return PLP_OK;
    return host_call(c, tv_args(a), tv_plan<Stage>, launch_two_view_pose);
}

// the host builds of two_view.hpp (no HIP call)
int32_t plp_model_two_view_pose_host(const plp_two_view_pose_args* a) {
    if (tv_check_args(a) != PLP_OK) return -1;
    if (a->P == 0 || a->n_cap == 0) return a->P;
    const TvArgs A = tv_args(a);
    double coef[kPgCoefs];
    pg_coef_init(coef);
    for (int p = 0; p < A.P; ++p) tv_model_problem(A, p, coef);
    return A.P;
}

int32_t plp_model_essential_decompose_host(const double* E_21, int32_t n, double* out_rots, double* out_trans) {
    if (n < 0 || (n > 0 && (!E_21 || !out_rots || !out_trans))) return -1;
    double ws[kTvDecomposeDoubles];
    for (int32_t i = 0; i < n; ++i) tv_decompose(E_21 + 9 * (size_t)i, ws, out_rots + 18 * (size_t)i, out_trans + 3 * (size_t)i);
    return n;
}

int32_t plp_model_check_pose_host(const plp_two_view_pose_args* a, const double* rot, const double* trans, int32_t* out_num_valid, float* out_parallax_deg,
                                  double* out_pts, uint8_t* out_is_triangulated, uint8_t* out_code) {
    if (!a || !rot || !trans || !out_num_valid || !out_parallax_deg) return -1;
    if (check_camera_model(&a->camera, false) != PLP_OK || a->P < 1 || a->n_cap < 0 || a->m_cap < 0 || a->n_cap > kEssMaxSlots) return -1;
    if (a->n_cap > 0 && (!a->inliers || !a->match || !a->bearing_1 || !a->undist_1 || (a->m_cap > 0 && (!a->bearing_2 || !a->undist_2)))) return -1;
    const TvArgs A = tv_args(a);
    double coef[kPgCoefs], pose12[12];
    pg_coef_init(coef);
    for (int i = 0; i < 9; ++i) pose12[i] = rot[i];
    for (int i = 0; i < 3; ++i) pose12[9 + i] = trans[i];
    *out_num_valid = tv_model_check_pose_any(A, 0, pose12, coef, *out_parallax_deg, out_pts, out_is_triangulated, out_code);
    return 1;
}

}  // extern "C"
