// What the entries of the two local adjusters share (local_ba_context.hip: plp_local_ba_*; local_ba_lines_context.hip: plp_local_ba_lines_*): the
// argument checks of plp_local_ba_args, its kernel arguments, the plan of its arrays and the one-problem state of the host builds.
#pragma once
#include <cmath>
#include <vector>

#include "matcher_context.hpp"
#include "local_ba.hpp"

namespace {
using namespace plp;

// host: the arrays are host memory, so the observation list and the number of free key frames are checked as well
plp_status la_check(const plp_local_ba_args* a, bool outputs, bool host) {
    if (!a) return set_error(PLP_ERR_INVALID_ARG, "NULL argument");
    if (a->camera.model != PLP_CAMERA_PERSPECTIVE && a->camera.model != PLP_CAMERA_FISHEYE && a->camera.model != PLP_CAMERA_EQUIRECTANGULAR)
        return set_error(PLP_ERR_INVALID_ARG, "unknown camera model");
    if (a->setup_type < 0 || a->setup_type > 2) return set_error(PLP_ERR_INVALID_ARG, "setup_type must be 0, 1 or 2");
    if (a->G < 0 || a->F < 0 || a->L < 0 || a->T < 0 || a->kp_stride < 0) return set_error(PLP_ERR_INVALID_ARG, "G, F, L, T and kp_stride must not be negative");
    if (a->num_first_iter < 1 || a->num_second_iter < 1) return set_error(PLP_ERR_INVALID_ARG, "num_first_iter and num_second_iter must be positive");
    if (a->pose_stride < 12) return set_error(PLP_ERR_INVALID_ARG, "pose_stride must be at least 12");
    if (a->num_levels < 1 || a->num_levels > 16 || !a->inv_level_sigma_sq) return set_error(PLP_ERR_INVALID_ARG, "num_levels must be 1 .. 16, inv_level_sigma_sq is required");
    if (a->camera.model == PLP_CAMERA_EQUIRECTANGULAR) return set_error(PLP_ERR_UNSUPPORTED, "the equirectangular reprojection edge is not implemented (DESIGN.md D17)");
    if (!std::isfinite(a->camera.fx) || !std::isfinite(a->camera.fy) || !std::isfinite(a->camera.cx) || !std::isfinite(a->camera.cy) || a->camera.fx == 0 || a->camera.fy == 0)
        return set_error(PLP_ERR_INVALID_ARG, "fx, fy, cx, cy must be finite, fx and fy non-zero");
    if (a->F > kLaMaxKf) return set_error(PLP_ERR_UNSUPPORTED, "more than 1024 key frames in the table");
    if (a->L > kLaMaxObs || a->T > kLaMaxObs) return set_error(PLP_ERR_UNSUPPORTED, "more than 2^18 landmarks or observations");
    if (a->G > kLaMaxProblems || (long long)a->G * a->T > kLaMaxWork || (long long)a->G * a->L > kLaMaxWork)
        return set_error(PLP_ERR_UNSUPPORTED, "more than 256 problems, or G * T or G * L above 2^22");
    if (a->G == 0) return PLP_OK;
    if (!a->obs_offsets) return set_error(PLP_ERR_INVALID_ARG, "obs_offsets is required");
    if (a->F > 0 && (!a->kf_local || !a->pose || (a->kp_stride > 0 && !a->undist))) return set_error(PLP_ERR_INVALID_ARG, "kf_local, pose and undist are required");
    if (a->L > 0 && !a->pos_w) return set_error(PLP_ERR_INVALID_ARG, "pos_w is required");
    if (a->T > 0 && (!a->obs_kf || !a->obs_idx)) return set_error(PLP_ERR_INVALID_ARG, "obs_kf and obs_idx are required");
    if (outputs) {
        if (!a->out_status || (a->F > 0 && (!a->out_kf_role || !a->out_pose)) || (a->L > 0 && (!a->out_lm_role || !a->out_pos_w)) || (a->T > 0 && !a->out_outlier))
            return set_error(PLP_ERR_INVALID_ARG, "out_status, out_kf_role, out_lm_role, out_pose, out_pos_w, out_outlier are required");
    }
    if (host) {
        if (a->obs_offsets[0] != 0 || a->obs_offsets[a->L] != a->T) return set_error(PLP_ERR_INVALID_ARG, "obs_offsets must rise from 0 to T");
        for (int l = 0; l < a->L; ++l)
            if (a->obs_offsets[l + 1] < a->obs_offsets[l]) return set_error(PLP_ERR_INVALID_ARG, "obs_offsets must rise from 0 to T");
        for (int g = 0; g < a->G; ++g) {
            int n = 0;
            for (int f = 0; f < a->F; ++f)
                n += a->kf_local[(size_t)g * a->F + f] && !(a->kf_erased && a->kf_erased[f]) && !(a->kf_is_origin && a->kf_is_origin[f]);
            if (n > kLaMaxFree) return set_error(PLP_ERR_UNSUPPORTED, "more than 64 free key frames in a problem");
        }
    }
    return PLP_OK;
}

LaArgs la_args(const plp_local_ba_args* a) {
    LaArgs A{};
    A.G = a->G; A.F = a->F; A.L = a->L; A.T = a->T; A.kp_stride = a->kp_stride; A.pose_stride = a->pose_stride; A.num_levels = a->num_levels;
    A.mono_setup = a->setup_type == 0; A.it1 = a->num_first_iter; A.it2 = a->num_second_iter;
    A.cam = pose_cam(a->camera.fx, a->camera.fy, a->camera.cx, a->camera.cy, a->camera.focal_x_baseline);
    A.delta_2d = (double)std::sqrt(kPoseChiSq2D); A.delta_3d = (double)std::sqrt(kPoseChiSq3D);
    for (int l = 0; l < 16; ++l) A.inv_sigma_sq[l] = l < A.num_levels ? a->inv_level_sigma_sq[l] : 0.0f;
    A.pose = a->pose; A.kf_erased = a->kf_erased; A.kf_is_origin = a->kf_is_origin; A.undist = a->undist; A.x_right = a->x_right; A.counts = a->counts;
    A.pos_w = a->pos_w; A.lm_erased = a->lm_erased; A.obs_offsets = a->obs_offsets; A.obs_kf = a->obs_kf; A.obs_idx = a->obs_idx; A.kf_local = a->kf_local;
    A.out_status = a->out_status; A.out_kf_role = a->out_kf_role; A.out_lm_role = a->out_lm_role; A.out_pose = a->out_pose; A.out_pos_w = a->out_pos_w;
    A.out_outlier = a->out_outlier; A.out_round_info = a->out_round_info; A.out_round_chi2 = a->out_round_chi2;
    return A;
}

// the arrays of the call; the rooms are what the steps hand to one another
template <class R> void la_plan(R& r, plp_matcher* c, LaArgs& A) {
    const size_t G = (size_t)A.G, F = (size_t)A.F, L = (size_t)A.L, T = (size_t)A.T, K = (size_t)A.kp_stride;
    r.in(A.pose, F * A.pose_stride); r.in(A.kf_erased, F); r.in(A.kf_is_origin, F); r.in(A.undist, F * K); r.in(A.x_right, F * K); r.in(A.counts, F);
    r.in(A.pos_w, L * 3); r.in(A.lm_erased, L); r.in(A.obs_offsets, L + 1); r.in(A.obs_kf, T); r.in(A.obs_idx, T); r.in(A.kf_local, G * F);
    r.out(A.out_status, G); r.out(A.out_kf_role, G * F); r.out(A.out_lm_role, G * L); r.out(A.out_pose, G * F * 15); r.out(A.out_pos_w, G * L * 3);
    r.out(A.out_outlier, G * T); r.out(A.out_round_info, G * 8); r.out(A.out_round_chi2, G * 4);
    r.room(c->la_d, A.ctx_d, G * la_doubles(A.F, A.L, A.T)); r.room(c->la_i, A.ctx_i, G * la_ints(A.T)); r.room(c->la_b, A.ctx_b, G * la_bytes(A.F, A.L, A.T) + 16);
}

// the state of the host builds: one problem's worth
struct LaHostCtx {
    std::vector<double> d; std::vector<int32_t> i; std::vector<uint8_t> b;
    void bind(LaArgs& A) {
        d.assign(la_doubles(A.F, A.L, A.T), 0.0); i.assign(la_ints(A.T), 0); b.assign(la_bytes(A.F, A.L, A.T) + 1, 0);
        A.ctx_d = d.data(); A.ctx_i = i.data(); A.ctx_b = b.data();
    }
};
// problem g of A with a context that holds one problem: the tables are shared, the per-problem arrays shifted
LaArgs la_one(const LaArgs& A, int g) {
    LaArgs B = A;
    B.G = 1;
    B.kf_local = A.kf_local ? A.kf_local + (size_t)g * A.F : nullptr;
    B.out_status = A.out_status ? A.out_status + g : nullptr;
    B.out_kf_role = A.out_kf_role ? A.out_kf_role + (size_t)g * A.F : nullptr;
    B.out_lm_role = A.out_lm_role ? A.out_lm_role + (size_t)g * A.L : nullptr;
    B.out_pose = A.out_pose ? A.out_pose + (size_t)g * A.F * 15 : nullptr;
    B.out_pos_w = A.out_pos_w ? A.out_pos_w + (size_t)g * A.L * 3 : nullptr;
    B.out_outlier = A.out_outlier ? A.out_outlier + (size_t)g * A.T : nullptr;
    B.out_round_info = A.out_round_info ? A.out_round_info + (size_t)g * 8 : nullptr;
    B.out_round_chi2 = A.out_round_chi2 ? A.out_round_chi2 + (size_t)g * 4 : nullptr;
    return B;
}

// ---- the model entries of both adjusters (plp_model_local_ba[_lines]_{linearize,solve}_host): the shared body over the extension `ext`
// (LaNoLines, or LlLines with the lines' tables filled by the caller)

// the first linearisation of round 1 of the prepared problem B and the outputs both adjusters give; false: the problem has no edges
template <class X> bool la_model_linearize(const LaArgs& B, const LaView& V, LaShared& sh, X& ext, bool robust, int32_t* out_free_kf, double* out_hpp,
                                           double* out_hll, double* out_chi2) {
    LaTeamHost par;
    if (out_free_kf) for (int i = 0; i < kLaMaxFree; ++i) out_free_kf[i] = -1;
    if (V.hdr()[kLaHStatus] != PLP_LOCAL_BA_OK) { if (out_chi2) out_chi2[0] = 0.0; return false; }
    sh.cam = B.cam; sh.delta = B.mono_setup ? B.delta_2d : B.delta_3d;
    la_round_setup(B, V, sh, par, ext);
    ext.perturb(V, par);
    la_edge_pass(B, V, sh, par, true, robust);
    ext.edge_pass(V, par, true, robust);
    la_sums(B, V, sh, par, true);
    ext.sums(V, par, true);
    sh.acc = 0.0;
    la_chain(B, V, sh, par, 0, kLaLmPart);
    ext.chain(par, 0);
    if (out_chi2) out_chi2[0] = sh.acc;
    for (int i = 0; i < sh.nfa; ++i) {
        if (out_free_kf) out_free_kf[i] = sh.akf[i];
        if (out_hpp) for (int t = 0; t < 27; ++t) out_hpp[27 * i + t] = la_p(V, i, t);
    }
    for (int l = 0; l < B.L; ++l)
        if (out_hll && V.lm_act()[l]) for (int t = 0; t < 9; ++t) out_hll[(size_t)9 * l + t] = la_l(V, l, kLaLmH + t);
    return true;
}

// the edges (pose, vertex) of given blocks: poses -1 .. P - 1, vertices 0 .. M - 1 in rising order
bool la_model_edges_ok(int P, int M, int E, const int32_t* e_pose, const int32_t* e_v) {
    if (M < 0 || M > kLaMaxObs || E < 0 || E > kLaMaxObs || (E > 0 && (!e_pose || !e_v))) return false;
    for (int e = 0; e < E; ++e)
        if (e_pose[e] < -1 || e_pose[e] >= P || e_v[e] < 0 || e_v[e] >= M || (e > 0 && e_v[e] < e_v[e - 1])) return false;
    return true;
}
// ... and their observation list
std::vector<int32_t> la_model_offsets(int M, int E, const int32_t* e_v) {
    std::vector<int32_t> off(M + 1, 0);
    for (int e = 0; e < E; ++e) off[e_v[e] + 1] += 1;
    for (int l = 0; l < M; ++l) off[l + 1] += off[l];
    return off;
}

// one damped solve of given blocks as a problem B of P + 1 key frames (row P: the constant pose), M landmarks and E observations; the return
// value is sh.ok
template <class X> int32_t la_model_solve(const LaArgs& B, const LaView& V, LaShared& sh, X& ext, const double* hpp, const double* hll, const int32_t* e_pose,
                                          const int32_t* e_lm, const double* w, double lambda, double* out_xp, double* out_xl) {
    LaTeamHost par;
    const int P = B.F - 1, M = B.L, E = B.T;
    V.hdr()[kLaHNf] = P;
    for (int i = 0; i < P; ++i) V.hdr()[kLaHFl + i] = i;
    for (int l = 0; l < M; ++l) V.lm_role()[l] = 1;
    for (int e = 0; e < E; ++e) { V.e_kf()[e] = e_pose[e] < 0 ? P : e_pose[e]; V.e_l()[e] = e_lm[e]; V.lvl()[e] = 0; }
    la_round_setup(B, V, sh, par, ext);
    for (int i = 0; i < sh.nfa; ++i) for (int t = 0; t < 27; ++t) la_p(V, i, t) = hpp[27 * sh.akf[i] + t];
    for (int l = 0; l < M; ++l) for (int t = 0; t < 9; ++t) la_l(V, l, kLaLmH + t) = hll[(size_t)9 * l + t];
    for (int e = 0; e < E; ++e) for (int k = 0; k < 18; ++k) la_e(V, e, kLaRowW + k) = w[(size_t)18 * e + k];
    sh.lambda = lambda;
    la_solve_system(B, V, sh, par, ext);
    for (int i = 0; i < 6 * P; ++i) out_xp[i] = 0.0;
    for (int i = 0; i < sh.nfa; ++i) for (int k = 0; k < 6; ++k) out_xp[6 * sh.akf[i] + k] = sh.x[6 * i + k];
    for (int l = 0; l < M; ++l) for (int k = 0; k < 3; ++k) out_xl[(size_t)3 * l + k] = V.lm_act()[l] ? la_l(V, l, kLaLmX + k) : 0.0;
    return sh.ok ? 1 : 0;
}
}  // namespace
