// Host driver + C ABI of the matcher context: per-frame pose optimisation: optimize::pose_optimizer[_extended_line] (include/plp_front.h: plp_pose_optimize_*; pose_opt_kernels.hip, pose_opt.hpp)
#include <hip/hip_runtime.h>

#include <cmath>
#include <vector>

#include "matcher_context.hpp"
#include "pose_opt.hpp"

using namespace plp;

extern "C" {

namespace {
plp_status pose_check(const plp_pose_optimize_args* a) {
    if (!a) return set_error(PLP_ERR_INVALID_ARG, "NULL argument");
    if (a->camera.model != PLP_CAMERA_PERSPECTIVE && a->camera.model != PLP_CAMERA_FISHEYE && a->camera.model != PLP_CAMERA_EQUIRECTANGULAR)
        return set_error(PLP_ERR_INVALID_ARG, "unknown camera model");
    if (a->setup_type < 0 || a->setup_type > 2) return set_error(PLP_ERR_INVALID_ARG, "setup_type must be 0, 1 or 2");
    if (a->B < 0 || a->n_cap < 0 || a->l_cap < 0) return set_error(PLP_ERR_INVALID_ARG, "B, n_cap and l_cap must not be negative");
    if (a->num_trials < 1 || a->num_each_iter < 1) return set_error(PLP_ERR_INVALID_ARG, "num_trials and num_each_iter must be positive");
    if (a->pose_stride < 12) return set_error(PLP_ERR_INVALID_ARG, "pose_stride must be at least 12");
    if (a->num_levels < 1 || a->num_levels > 16 || !a->inv_level_sigma_sq) return set_error(PLP_ERR_INVALID_ARG, "num_levels must be 1 .. 16, inv_level_sigma_sq is required");
    if (a->l_cap > 0 && (a->num_levels_lsd < 1 || a->num_levels_lsd > 16 || !a->inv_level_sigma_sq_lsd))
        return set_error(PLP_ERR_INVALID_ARG, "with lines num_levels_lsd must be 1 .. 16 and inv_level_sigma_sq_lsd is required");
    if (a->camera.model == PLP_CAMERA_EQUIRECTANGULAR) return set_error(PLP_ERR_UNSUPPORTED, "the equirectangular pose edge is not implemented (DESIGN.md D15)");
    if (!(a->camera.fx != 0) || !(a->camera.fy != 0)) return set_error(PLP_ERR_INVALID_ARG, "fx, fy must be non-zero");
    if (a->n_cap > kPoseMaxSlots || a->l_cap > kPoseMaxSlots) return set_error(PLP_ERR_UNSUPPORTED, "more than 8192 slots per frame");
    if (a->B > 65535) return set_error(PLP_ERR_UNSUPPORTED, "more than 65535 frames in one call");
    if (a->B == 0) return PLP_OK;
    if (!a->pose_in || !a->out_status || !a->out_pose || !a->out_num_init_obs || !a->out_num_valid)
        return set_error(PLP_ERR_INVALID_ARG, "pose_in, out_status, out_pose, out_num_init_obs, out_num_valid are required");
    if (a->n_cap > 0 && (!a->valid || !a->undist || !a->pos_w || !a->out_outlier)) return set_error(PLP_ERR_INVALID_ARG, "valid, undist, pos_w, out_outlier are required");
    if (a->l_cap > 0 && (!a->line_valid || !a->keylines || !a->pos_w_lines || !a->out_outlier_lines))
        return set_error(PLP_ERR_INVALID_ARG, "line_valid, keylines, pos_w_lines, out_outlier_lines are required");
    return PLP_OK;
}

PoseArgs pose_args(const plp_pose_optimize_args* a) {
    PoseArgs A{};
    A.B = a->B; A.n_cap = a->n_cap; A.l_cap = a->l_cap; A.num_trials = a->num_trials; A.num_each_iter = a->num_each_iter;
    A.mono_setup = a->setup_type == 0; A.pose_stride = a->pose_stride; A.num_levels = a->num_levels; A.num_levels_lsd = a->l_cap > 0 ? a->num_levels_lsd : 0;
    A.cam = pose_cam(a->camera.fx, a->camera.fy, a->camera.cx, a->camera.cy, a->camera.focal_x_baseline);
    A.delta_2d = (double)std::sqrt(kPoseChiSq2D); A.delta_3d = (double)std::sqrt(kPoseChiSq3D);     // const float sqrt_chi_sq_2D = std::sqrt(chi_sq_2D)
    for (int l = 0; l < 16; ++l) {
        A.inv_sigma_sq[l] = l < A.num_levels ? a->inv_level_sigma_sq[l] : 0.0f;
        A.inv_sigma_sq_lsd[l] = l < A.num_levels_lsd ? a->inv_level_sigma_sq_lsd[l] : 0.0f;
    }
    A.pose_in = a->pose_in; A.counts = a->counts; A.line_counts = a->line_counts; A.valid = a->valid; A.undist = a->undist; A.x_right = a->x_right;
    A.pos_w = a->pos_w; A.line_valid = a->line_valid; A.keylines = a->keylines; A.pos_w_lines = a->pos_w_lines;
    A.out_status = a->out_status; A.out_pose = a->out_pose; A.out_num_init_obs = a->out_num_init_obs; A.out_num_valid = a->out_num_valid;
    A.out_outlier = a->out_outlier; A.out_outlier_lines = a->out_outlier_lines; A.out_trial_info = a->out_trial_info; A.out_trial_chi2 = a->out_trial_chi2;
    return A;
}

// the arrays of the call; the rooms are what the launches hand to one another
extern "C++" template <class R> void pose_plan(R& r, plp_matcher* c, PoseArgs& A) {
    const size_t B = (size_t)A.B, N = (size_t)A.n_cap, L = (size_t)A.l_cap, T = (size_t)A.num_trials;
    r.in(A.pose_in, (B - 1) * A.pose_stride + 12); r.in(A.counts, B); r.in(A.line_counts, B);
    r.in(A.valid, B * N); r.in(A.undist, B * N); r.in(A.x_right, B * N); r.in(A.pos_w, B * N * 3);
    r.in(A.line_valid, B * L); r.in(A.keylines, B * L); r.in(A.pos_w_lines, B * L * 6);
    r.out(A.out_status, B, false); r.out(A.out_pose, B * 15, false); r.out(A.out_num_init_obs, B, false); r.out(A.out_num_valid, B, false);
    r.out(A.out_outlier, B * N); r.out(A.out_outlier_lines, B * L); r.out(A.out_trial_info, B * T * 4, false); r.out(A.out_trial_chi2, B * T * 2, false);
    r.room(c->pose_slot, A.ctx_slot, B * N + 1); r.room(c->pose_slot_lines, A.ctx_slot_lines, B * L + 1);
    r.room(c->pose_chi2, A.ctx_chi2, B * (N + L) + 1); r.room(c->pose_n, A.ctx_n, B * 2);
}

// the edges of one frame of the host build, in rank order
struct PoseEdges {
    std::vector<int> slot, lslot;
    std::vector<uint8_t> level, llevel;         // 1 = outlier (edge level 1)
    std::vector<double> chi2, lchi2;            // of the last evaluation
};
void pose_model_edges(const PoseArgs& A, int b, bool lines, PoseEdges& E) {
    const size_t row = (size_t)b * A.n_cap, lrow = (size_t)b * A.l_cap;
    const int count = pose_count(A, b);
    for (int s = 0; s < count; ++s)
        if (A.valid[row + s] && (unsigned)A.undist[row + s].octave < (unsigned)A.num_levels) E.slot.push_back(s);
    if (lines) {
        const int lcount = pose_line_count(A, b);
        for (int s = 0; s < lcount; ++s)
            if (A.line_valid[lrow + s] && (unsigned)A.keylines[lrow + s].octave < (unsigned)A.num_levels_lsd) E.lslot.push_back(s);
    }
    E.level.assign(E.slot.size(), 0); E.llevel.assign(E.lslot.size(), 0);
    E.chi2.assign(E.slot.size(), 0.0); E.lchi2.assign(E.lslot.size(), 0.0);
}
double pose_model_point_chi2(const PoseArgs& A, int b, int slot, const double* est) {
    const size_t s = (size_t)b * A.n_cap + slot;
    const float xr = A.x_right ? A.x_right[s] : -1.0f;
    double x, y, z, e0, e1, e2;
    return pose_point_error(est, A.cam, A.pos_w + 3 * s, (double)A.undist[s].x, (double)A.undist[s].y, (double)xr, xr < 0.0f,
                            (double)A.inv_sigma_sq[A.undist[s].octave], x, y, z, e0, e1, e2);
}
double pose_model_line_chi2(const PoseArgs& A, int b, int slot, const double* est) {
    const size_t s = (size_t)b * A.l_cap + slot;
    const plp_keyline& kl = A.keylines[s];
    double e0, e1;
    return pose_line_error(est, A.cam, A.pos_w_lines + 6 * s, (double)kl.startPointX, (double)kl.startPointY, (double)kl.endPointX, (double)kl.endPointY,
                           (double)A.inv_sigma_sq_lsd[kl.octave], e0, e1);
}
// one pass over the active edges at W.est: sums[28] when lin, else sums[27] alone; stores the chi2 of every active edge
void pose_model_pass(const PoseArgs& A, int b, PoseWork& W, PoseEdges& E, bool robust, bool lin, double* sums) {
    const double delta_pt = A.mono_setup ? A.delta_2d : A.delta_3d;
    for (int t = 0; t < kPoseTerms; ++t) sums[t] = 0.0;
    double T[kPoseTerms];
    if (lin && !E.lslot.empty())
        for (int i = 0; i < 12; ++i) pose_perturb(W.est, i, W.pert + 7 * i);
    for (size_t k = 0; k < E.slot.size(); ++k) {
        if (E.level[k]) continue;
        const size_t s = (size_t)b * A.n_cap + E.slot[k];
        if (lin) {
            const float xr = A.x_right ? A.x_right[s] : -1.0f;
            E.chi2[k] = pose_point_terms(W.est, A.cam, A.pos_w + 3 * s, (double)A.undist[s].x, (double)A.undist[s].y, (double)xr, xr < 0.0f,
                                         (double)A.inv_sigma_sq[A.undist[s].octave], robust, delta_pt, T, 1);
            for (int t = 0; t < kPoseTerms; ++t) sums[t] = sums[t] + T[t];
        } else {
            const double chi2 = pose_model_point_chi2(A, b, E.slot[k], W.est);
            double rho0 = chi2, rho1 = 1.0;
            if (robust) pose_huber(chi2, delta_pt, rho0, rho1);
            E.chi2[k] = chi2;
            sums[27] = sums[27] + rho0;
        }
    }
    for (size_t k = 0; k < E.lslot.size(); ++k) {
        if (E.llevel[k]) continue;
        const size_t s = (size_t)b * A.l_cap + E.lslot[k];
        if (lin) {
            const plp_keyline& kl = A.keylines[s];
            E.lchi2[k] = pose_line_terms(W.est, W.pert, A.cam, A.pos_w_lines + 6 * s, (double)kl.startPointX, (double)kl.startPointY, (double)kl.endPointX,
                                         (double)kl.endPointY, (double)A.inv_sigma_sq_lsd[kl.octave], robust, A.delta_2d, T, 1);
            for (int t = 0; t < kPoseTerms; ++t) sums[t] = sums[t] + T[t];
        } else {
            const double chi2 = pose_model_line_chi2(A, b, E.lslot[k], W.est);
            double rho0 = chi2, rho1 = 1.0;
            if (robust) pose_huber(chi2, A.delta_2d, rho0, rho1);
            E.lchi2[k] = chi2;
            sums[27] = sums[27] + rho0;
        }
    }
}

// one frame of the host build: the kernels' steps, one edge after the other
void pose_model_frame(const PoseArgs& A, int b) {
    const size_t row = (size_t)b * A.n_cap, lrow = (size_t)b * A.l_cap;
    const int T = A.num_trials;
    PoseEdges E;
    pose_model_edges(A, b, false, E);
    const int n = (int)E.slot.size();
    for (int s : E.slot) A.out_outlier[row + s] = 0;
    if (A.out_trial_info) for (int i = 0; i < 4 * T; ++i) A.out_trial_info[(size_t)4 * T * b + i] = 0;
    if (A.out_trial_chi2) for (int i = 0; i < 2 * T; ++i) A.out_trial_chi2[(size_t)2 * T * b + i] = 0.0;
    const double* in = A.pose_in + (size_t)b * A.pose_stride;
    double* out = A.out_pose + (size_t)15 * b;
    A.out_num_init_obs[b] = n;
    if (n < kPoseMinObs) {
        for (int i = 0; i < 12; ++i) out[i] = in[i];
        for (int i = 0; i < 3; ++i) out[12 + i] = ((-in[i]) * in[9] + (-in[3 + i]) * in[10]) + (-in[6 + i]) * in[11];
        A.out_status[b] = PLP_POSE_OPT_TOO_FEW_OBS;
        A.out_num_valid[b] = 0;
        return;
    }
    if (A.l_cap > 0) {
        E = PoseEdges();
        pose_model_edges(A, b, true, E);
        for (int s : E.lslot) A.out_outlier_lines[lrow + s] = 0;
    }
    PoseWork W{};
    pose_est_from_pose(in, W.est);
    W.ni = 2.0;
    int num_bad = 0;
    double sums[kPoseTerms];
    for (int trial = 0; trial < T; ++trial) {
        const bool robust = pose_trial_robust(trial, T);
        W.iterations = 0; W.rejected = 0; W.end = 0;
        for (int it = 0; it < A.num_each_iter; ++it) {
            pose_model_pass(A, b, W, E, robust, true, W.sum);
            lev_begin<6>(W, it);
            do {
                pose_lm_try(W);
                pose_model_pass(A, b, W, E, robust, false, sums);
                lev_decide_vertex<6, 7>(W, sums[27]);
            } while (W.go_on);
            W.iterations += 1;
            W.end = lev_end(W);
            if (W.end) break;
        }
        num_bad = 0;
        for (int k = 0; k < n; ++k) {
            const size_t s = row + E.slot[k];
            const float xr = A.x_right ? A.x_right[s] : -1.0f;
            const double chi2 = E.level[k] ? pose_model_point_chi2(A, b, E.slot[k], W.est) : E.chi2[k];
            const bool bad = (double)(xr < 0.0f ? kPoseChiSq2D : kPoseChiSq3D) < chi2;
            E.level[k] = bad; A.out_outlier[s] = bad;
            num_bad += bad;
        }
        const bool stop = n - num_bad < kPoseMinObs;
        if (!stop)
            for (size_t k = 0; k < E.lslot.size(); ++k) {
                const double chi2 = E.llevel[k] ? pose_model_line_chi2(A, b, E.lslot[k], W.est) : E.lchi2[k];
                const bool bad = (double)kPoseChiSq2D < chi2;
                E.llevel[k] = bad; A.out_outlier_lines[lrow + E.lslot[k]] = bad;
            }
        if (A.out_trial_info) {
            int32_t* ti = A.out_trial_info + ((size_t)T * b + trial) * 4;
            ti[0] = W.iterations; ti[1] = W.rejected; ti[2] = num_bad; ti[3] = W.end ? W.end : kLevEndIterations;
        }
        if (A.out_trial_chi2) {
            double* tc = A.out_trial_chi2 + ((size_t)T * b + trial) * 2;
            tc[0] = W.current_chi; tc[1] = W.lambda;
        }
        if (stop) break;
    }
    pose_pose_from_est(W.est, out);
    A.out_status[b] = PLP_POSE_OPT_OK;
    A.out_num_valid[b] = n - num_bad;
}
}  // namespace

plp_status plp_pose_optimize_device(plp_matcher* c, const plp_pose_optimize_args* a, void* hip_stream) {
    if (!c) return set_error(PLP_ERR_INVALID_ARG, "ctx is NULL");
    if (plp_status s = pose_check(a)) return s;
    if (a->B == 0) return PLP_OK;
    return device_call(c, hip_stream, pose_args(a), pose_plan<DeviceRooms>, launch_pose_optimize);
}

plp_status plp_pose_optimize_host(plp_matcher* c, const plp_pose_optimize_args* a) {
    if (!c) return set_error(PLP_ERR_INVALID_ARG, "ctx is NULL");
    if (plp_status s = pose_check(a)) return s;
    if (a->B == 0) return PLP_OK;
    return host_call(c, pose_args(a), pose_plan<Stage>, launch_pose_optimize);
}

// the host builds of pose_opt.hpp (no HIP call)
int32_t plp_model_pose_optimize_host(const plp_pose_optimize_args* a) {
    if (plp_status s = pose_check(a)) return -(int32_t)s;
    const PoseArgs A = pose_args(a);
    for (int b = 0; b < A.B; ++b) pose_model_frame(A, b);
    return A.B;
}

int32_t plp_model_pose_linearize_host(const plp_pose_optimize_args* a, int32_t robust, const uint8_t* active, const uint8_t* active_lines,
                                      double* out_sums, double* out_chi2, double* out_chi2_lines) {
    if (plp_status s = pose_check(a)) return -(int32_t)s;
    if (a->B > 0 && !out_sums) return -(int32_t)set_error(PLP_ERR_INVALID_ARG, "out_sums is required");
    const PoseArgs A = pose_args(a);
    for (int b = 0; b < A.B; ++b) {
        PoseEdges E;
        pose_model_edges(A, b, A.l_cap > 0, E);
        for (size_t k = 0; k < E.slot.size(); ++k) E.level[k] = active && !active[(size_t)b * A.n_cap + E.slot[k]];
        for (size_t k = 0; k < E.lslot.size(); ++k) E.llevel[k] = active_lines && !active_lines[(size_t)b * A.l_cap + E.lslot[k]];
        PoseWork W{};
        pose_est_from_pose(A.pose_in + (size_t)b * A.pose_stride, W.est);
        pose_model_pass(A, b, W, E, robust != 0, true, out_sums + (size_t)kPoseTerms * b);
        if (out_chi2)
            for (size_t k = 0; k < E.slot.size(); ++k)
                if (!E.level[k]) out_chi2[(size_t)b * A.n_cap + E.slot[k]] = E.chi2[k];
        if (out_chi2_lines)
            for (size_t k = 0; k < E.lslot.size(); ++k)
                if (!E.llevel[k]) out_chi2_lines[(size_t)b * A.l_cap + E.lslot[k]] = E.lchi2[k];
    }
    return A.B;
}

int32_t plp_model_se3_exp_host(const double* update, const double* est, int32_t n, double* out) {
    if (n < 0 || (n > 0 && (!update || !est || !out))) return -1;
    for (int32_t i = 0; i < n; ++i) pose_oplus(update + 6 * (size_t)i, est + 7 * (size_t)i, out + 7 * (size_t)i);
    return n;
}

int32_t plp_model_chol6_host(const double* H, const double* b, const double* lambda, int32_t n, double* out_x, int32_t* out_ok) {
    if (n < 0 || (n > 0 && (!H || !b || !lambda || !out_x || !out_ok))) return -1;
    for (int32_t i = 0; i < n; ++i) {
        double Lf[36] = {0}, y[6] = {0};
        out_ok[i] = lev_chol<6>(H + 21 * (size_t)i, b + 6 * (size_t)i, lambda[i], Lf, y, out_x + 6 * (size_t)i) ? 1 : 0;
    }
    return n;
}

int32_t plp_model_pose_sincos_host(const double* x, int32_t n, double* out_sin, double* out_cos) {
    if (n < 0 || (n > 0 && (!x || !out_sin || !out_cos))) return -1;
    for (int32_t i = 0; i < n; ++i) pose_sincos(x[i], out_sin[i], out_cos[i]);
    return n;
}

}  // extern "C"
