// Host driver + C ABI of the matcher context: Sim3 refinement of loop candidates: optimize::transform_optimizer (include/plp_front.h: plp_transform_optimize_*; transform_opt_kernels.hip, transform_opt.hpp)
#include <hip/hip_runtime.h>

#include <cmath>
#include <vector>

#include "matcher_context.hpp"
#include "transform_opt.hpp"

using namespace plp;

extern "C" {

namespace {
// outputs: the required output pointers too (the entries that optimise); false: the inputs alone (plp_model_transform_linearize_host writes none of them)
plp_status tf_check(const plp_transform_optimize_args* a, bool outputs = true) {
    if (!a) return set_error(PLP_ERR_INVALID_ARG, "NULL argument");
    if (a->camera.model != PLP_CAMERA_PERSPECTIVE && a->camera.model != PLP_CAMERA_FISHEYE && a->camera.model != PLP_CAMERA_EQUIRECTANGULAR)
        return set_error(PLP_ERR_INVALID_ARG, "unknown camera model");
    if (a->P < 0 || a->n_cap < 0) return set_error(PLP_ERR_INVALID_ARG, "P and n_cap must not be negative");
    if (a->num_iter < 1) return set_error(PLP_ERR_INVALID_ARG, "num_iter must be positive");
    if (!(a->chi_sq > 0.0f)) return set_error(PLP_ERR_INVALID_ARG, "chi_sq must be positive");
    if (a->num_levels < 1 || a->num_levels > 16 || !a->inv_level_sigma_sq_1 || !a->inv_level_sigma_sq_2)
        return set_error(PLP_ERR_INVALID_ARG, "num_levels must be 1 .. 16, inv_level_sigma_sq_1 and _2 are required");
    if (a->camera.model == PLP_CAMERA_EQUIRECTANGULAR) return set_error(PLP_ERR_UNSUPPORTED, "the equirectangular reprojection edges are not implemented (DESIGN.md D16)");
    if (!std::isfinite(a->camera.fx) || !std::isfinite(a->camera.fy) || !std::isfinite(a->camera.cx) || !std::isfinite(a->camera.cy) || a->camera.fx == 0 || a->camera.fy == 0)
        return set_error(PLP_ERR_INVALID_ARG, "fx, fy, cx, cy must be finite, fx and fy non-zero");
    if (a->n_cap > kTfMaxSlots) return set_error(PLP_ERR_UNSUPPORTED, "more than 8192 slots per problem");
    if (a->P > 65535) return set_error(PLP_ERR_UNSUPPORTED, "more than 65535 problems in one call");
    if (a->P == 0) return PLP_OK;
    if (!a->pose_1 || !a->pose_2 || !a->rot_12 || !a->trans_12 || !a->scale_12) return set_error(PLP_ERR_INVALID_ARG, "pose_1, pose_2, rot_12, trans_12, scale_12 are required");
    if (a->n_cap > 0 && (!a->valid || !a->pos_w_1 || !a->pos_w_2 || !a->undist_1 || !a->undist_2))
        return set_error(PLP_ERR_INVALID_ARG, "valid, pos_w_1, pos_w_2, undist_1, undist_2 are required");
    if (!outputs) return PLP_OK;
    if (!a->out_status || !a->out_num_valid || !a->out_num_inliers || !a->out_rot_12 || !a->out_trans_12 || !a->out_scale_12)
        return set_error(PLP_ERR_INVALID_ARG, "out_status, out_num_valid, out_num_inliers, out_rot_12, out_trans_12, out_scale_12 are required");
    if (a->n_cap > 0 && !a->out_kept) return set_error(PLP_ERR_INVALID_ARG, "out_kept is required");
    return PLP_OK;
}

TfArgs tf_args(const plp_transform_optimize_args* a) {
    TfArgs A{};
    A.P = a->P; A.n_cap = a->n_cap; A.num_iter = a->num_iter; A.fix_scale = a->fix_scale != 0; A.num_levels = a->num_levels;
    A.cam = pose_cam(a->camera.fx, a->camera.fy, a->camera.cx, a->camera.cy, 0.0);
    A.chi_sq = (double)a->chi_sq; A.delta = (double)std::sqrt(a->chi_sq);         // const float sqrt_chi_sq = std::sqrt(chi_sq)
    for (int l = 0; l < 16; ++l) {
        A.inv_sigma_sq_1[l] = l < A.num_levels ? a->inv_level_sigma_sq_1[l] : 0.0f;
        A.inv_sigma_sq_2[l] = l < A.num_levels ? a->inv_level_sigma_sq_2[l] : 0.0f;
    }
    A.counts = a->counts; A.valid = a->valid; A.pos_w_1 = a->pos_w_1; A.pos_w_2 = a->pos_w_2; A.undist_1 = a->undist_1; A.undist_2 = a->undist_2;
    A.pose_1 = a->pose_1; A.pose_2 = a->pose_2; A.rot_12 = a->rot_12; A.trans_12 = a->trans_12; A.scale_12 = a->scale_12;
    A.out_status = a->out_status; A.out_num_valid = a->out_num_valid; A.out_num_inliers = a->out_num_inliers; A.out_rot_12 = a->out_rot_12;
    A.out_trans_12 = a->out_trans_12; A.out_scale_12 = a->out_scale_12; A.out_world_to_1 = a->out_world_to_1; A.out_kept = a->out_kept;
    A.out_round_info = a->out_round_info; A.out_round_chi2 = a->out_round_chi2;
    return A;
}

// the arrays of the call; the rooms are what the launches hand to one another
extern "C++" template <class R> void tf_plan(R& r, plp_matcher* c, TfArgs& A) {
    const size_t P = (size_t)A.P, N = (size_t)A.n_cap;
    r.in(A.counts, P); r.in(A.valid, P * N); r.in(A.pos_w_1, P * N * 3); r.in(A.pos_w_2, P * N * 3); r.in(A.undist_1, P * N); r.in(A.undist_2, P * N);
    r.in(A.pose_1, P * 15); r.in(A.pose_2, P * 15); r.in(A.rot_12, P * 9); r.in(A.trans_12, P * 3); r.in(A.scale_12, P);
    r.out(A.out_status, P, false); r.out(A.out_num_valid, P, false); r.out(A.out_num_inliers, P, false); r.out(A.out_rot_12, P * 9, false);
    r.out(A.out_trans_12, P * 3, false); r.out(A.out_scale_12, P, false); r.out(A.out_world_to_1, P * 13, false); r.out(A.out_kept, P * N);
    r.out(A.out_round_info, P * 8, false); r.out(A.out_round_chi2, P * 4, false);
    r.room(c->tf_slot, A.ctx_slot, P * N + 1); r.room(c->tf_chi2, A.ctx_chi2, 2 * P * N + kTfCtxDoubles * P); r.room(c->tf_n, A.ctx_n, kTfCtxInts * P);
    r.room(c->tf_level, A.ctx_level, P * N + 1); r.room(c->tf_edge, A.ctx_edge, 12 * P * N + 1);
}

// the matches of one problem of the host build, in rank order
struct TfEdges {
    std::vector<int> slot;
    std::vector<uint8_t> level;                 // 1 = dropped (both edges at level 1)
    std::vector<double> chi2;                   // [2 k] forward, [2 k + 1] backward: of the last evaluation
};
void tf_model_edges(const TfArgs& A, int p, TfEdges& E) {
    const size_t row = (size_t)p * A.n_cap;
    const int count = tf_count(A, p);
    for (int s = 0; s < count; ++s)
        if (tf_observation(A, row + s)) E.slot.push_back(s);
    E.level.assign(E.slot.size(), 0);
    E.chi2.assign(2 * E.slot.size(), 0.0);
}
// one pass over the kept matches: sums[36] at the linearisation W.sims / W.invs when lin, else sums[35] alone at entry 14
void tf_model_pass(const TfArgs& A, int p, TfWork& W, TfEdges& E, bool lin, double* sums) {
    for (int t = 0; t < kTfTerms; ++t) sums[t] = 0.0;
    double T[kTfTerms];
    for (size_t k = 0; k < E.slot.size(); ++k) {
        if (E.level[k]) continue;
        const size_t s = (size_t)p * A.n_cap + E.slot[k];
        for (int dir = 0; dir < 2; ++dir) {
            const plp_keypoint& kp = dir ? A.undist_2[s] : A.undist_1[s];
            const double w = (double)(dir ? A.inv_sigma_sq_2[kp.octave] : A.inv_sigma_sq_1[kp.octave]);
            const double* sims = dir ? W.invs : W.sims;
            double x, y, z;
            tf_to_camera((dir ? A.pose_1 : A.pose_2) + (size_t)15 * p, (dir ? A.pos_w_1 : A.pos_w_2) + 3 * s, x, y, z);
            if (lin) {
                E.chi2[2 * k + dir] = tf_edge_terms(sims, A.cam, x, y, z, (double)kp.x, (double)kp.y, w, A.delta, T, 1);
                for (int t = 0; t < kTfTerms; ++t) sums[t] = sums[t] + T[t];
            } else {
                double e0, e1, rho0, rho1;
                const double c = tf_edge_error(sims + 8 * 14, A.cam, x, y, z, (double)kp.x, (double)kp.y, w, e0, e1);
                pose_huber(c, A.delta, rho0, rho1);
                E.chi2[2 * k + dir] = c;
                sums[35] = sums[35] + rho0;
            }
        }
    }
}
void tf_model_linearize(const TfArgs& A, TfWork& W) {
    for (int i = 0; i < kTfSims; ++i) {
        tf_perturb(W.est, i, A.fix_scale != 0, W.sims + 8 * i);
        tf_inverse(W.sims + 8 * i, W.invs + 8 * i);
    }
}

// one problem of the host build: the kernels' steps, one edge after the other
void tf_model_problem(const TfArgs& A, int p) {
    const size_t row = (size_t)p * A.n_cap;
    TfEdges E;
    tf_model_edges(A, p, E);
    const int n = (int)E.slot.size();
    for (int s : E.slot) A.out_kept[row + s] = 1;
    if (A.out_round_info) for (int i = 0; i < 8; ++i) A.out_round_info[(size_t)8 * p + i] = 0;
    if (A.out_round_chi2) for (int i = 0; i < 4; ++i) A.out_round_chi2[(size_t)4 * p + i] = 0.0;
    TfWork W{};
    double est0[8];
    tf_est_from_input(A.rot_12 + (size_t)9 * p, A.trans_12 + (size_t)3 * p, A.scale_12[p], est0);
    for (int i = 0; i < 8; ++i) W.est[i] = est0[i];
    W.ni = 2.0;
    if (n == 0) { tf_write_result(A, p, est0, true, 0, 0); return; }
    const bool fix = A.fix_scale != 0;
    int left = n;
    double sums[kTfTerms];
    for (int round = 0; round < 2; ++round) {
        const int iters = tf_round_iters(round, A.num_iter);
        W.iterations = 0; W.rejected = 0; W.end = 0;
        for (int it = 0; it < iters; ++it) {
            tf_model_linearize(A, W);
            tf_model_pass(A, p, W, E, true, W.sum);
            lev_begin<kTfDim>(W, it);
            do {
                tf_lm_solve(W);
                tf_lm_update(W, fix);
                tf_model_pass(A, p, W, E, false, sums);
                lev_decide_vertex<kTfDim, 8>(W, sums[35]);
            } while (W.go_on);
            W.iterations += 1;
            W.end = lev_end(W);
            if (W.end) break;
        }
        int drops = 0;
        for (int k = 0; k < n; ++k) {
            if (E.level[k]) continue;
            if (tf_drop(round, A.chi_sq, E.chi2[2 * k], E.chi2[2 * k + 1])) {
                E.level[k] = 1; A.out_kept[row + E.slot[k]] = 0;
                ++drops;
            }
        }
        left -= drops;
        if (A.out_round_info) {
            int32_t* ri = A.out_round_info + (size_t)8 * p + 4 * round;
            ri[0] = W.iterations; ri[1] = W.rejected; ri[2] = drops; ri[3] = W.end ? W.end : kLevEndIterations;
        }
        if (A.out_round_chi2) {
            double* rc = A.out_round_chi2 + (size_t)4 * p + 2 * round;
            rc[0] = W.current_chi; rc[1] = W.lambda;
        }
        if (round == 0 && left < kTfMinInliers) { tf_write_result(A, p, est0, true, n, 0); return; }
    }
    tf_write_result(A, p, W.est, false, n, left);
}
}  // namespace

plp_status plp_transform_optimize_device(plp_matcher* c, const plp_transform_optimize_args* a, void* hip_stream) {
    if (!c) return set_error(PLP_ERR_INVALID_ARG, "ctx is NULL");
    if (plp_status s = tf_check(a)) return s;
    if (a->P == 0) return PLP_OK;
    return device_call(c, hip_stream, tf_args(a), tf_plan<DeviceRooms>, launch_transform_optimize);
}

plp_status plp_transform_optimize_host(plp_matcher* c, const plp_transform_optimize_args* a) {
    if (!c) return set_error(PLP_ERR_INVALID_ARG, "ctx is NULL");
    if (plp_status s = tf_check(a)) return s;
    if (a->P == 0) return PLP_OK;
    return host_call(c, tf_args(a), tf_plan<Stage>, launch_transform_optimize);
}

// the host builds of transform_opt.hpp (no HIP call)
int32_t plp_model_transform_optimize_host(const plp_transform_optimize_args* a) {
    if (plp_status s = tf_check(a)) return -(int32_t)s;
    const TfArgs A = tf_args(a);
    for (int p = 0; p < A.P; ++p) tf_model_problem(A, p);
    return A.P;
}

int32_t plp_model_transform_linearize_host(const plp_transform_optimize_args* a, const uint8_t* active, double* out_sums, double* out_chi2) {
    if (plp_status s = tf_check(a, false)) return -(int32_t)s;
    if (a->P > 0 && !out_sums) return -(int32_t)set_error(PLP_ERR_INVALID_ARG, "out_sums is required");
    const TfArgs A = tf_args(a);
    for (int p = 0; p < A.P; ++p) {
        TfEdges E;
        tf_model_edges(A, p, E);
        for (size_t k = 0; k < E.slot.size(); ++k) E.level[k] = active && !active[(size_t)p * A.n_cap + E.slot[k]];
        TfWork W{};
        tf_est_from_input(A.rot_12 + (size_t)9 * p, A.trans_12 + (size_t)3 * p, A.scale_12[p], W.est);
        tf_model_linearize(A, W);
        tf_model_pass(A, p, W, E, true, out_sums + (size_t)kTfTerms * p);
        if (out_chi2)
            for (size_t k = 0; k < E.slot.size(); ++k)
                if (!E.level[k]) {
                    out_chi2[2 * ((size_t)p * A.n_cap + E.slot[k])] = E.chi2[2 * k];
                    out_chi2[2 * ((size_t)p * A.n_cap + E.slot[k]) + 1] = E.chi2[2 * k + 1];
                }
    }
    return A.P;
}

int32_t plp_model_sim3_exp_host(const double* update, const double* est, int32_t fix_scale, int32_t n, double* out) {
    if (n < 0 || (n > 0 && (!update || !est || !out))) return -1;
    for (int32_t i = 0; i < n; ++i) tf_oplus(update + 7 * (size_t)i, fix_scale != 0, est + 8 * (size_t)i, out + 8 * (size_t)i);
    return n;
}

int32_t plp_model_chol7_host(const double* H, const double* b, const double* lambda, int32_t n, double* out_x, int32_t* out_ok) {
    if (n < 0 || (n > 0 && (!H || !b || !lambda || !out_x || !out_ok))) return -1;
    for (int32_t i = 0; i < n; ++i) {
        double Lf[49] = {0}, y[7] = {0};
        out_ok[i] = lev_chol<kTfDim>(H + 28 * (size_t)i, b + 7 * (size_t)i, lambda[i], Lf, y, out_x + 7 * (size_t)i) ? 1 : 0;
    }
    return n;
}

int32_t plp_model_pose_exp_host(const double* x, int32_t n, double* out) {
    if (n < 0 || (n > 0 && (!x || !out))) return -1;
    for (int32_t i = 0; i < n; ++i) out[i] = pose_exp(x[i]);
    return n;
}

}  // extern "C"
