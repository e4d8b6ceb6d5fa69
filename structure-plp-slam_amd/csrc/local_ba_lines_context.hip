// Host driver + C ABI of the matcher context: local bundle adjustment with line landmarks: optimize::local_bundle_adjuster_extended_line
// (include/plp_front.h: plp_local_ba_lines_*; local_ba_lines_kernels.hip, local_ba_lines.hpp)
#include <hip/hip_runtime.h>

#include <vector>

#include "local_ba_entry.hpp"
#include "local_ba_lines.hpp"

using namespace plp;

extern "C" {

namespace {
// the checks of `points` are plp_local_ba_*'s own; the lines' follow their pattern
plp_status ll_check(const plp_local_ba_lines_args* a, bool outputs, bool host) {
    if (!a) return set_error(PLP_ERR_INVALID_ARG, "NULL argument");
    if (plp_status s = la_check(&a->points, outputs, host)) return s;
    if (a->LL < 0 || a->TL < 0 || a->kl_stride < 0) return set_error(PLP_ERR_INVALID_ARG, "LL, TL and kl_stride must not be negative");
    if (a->num_levels_lsd < 1 || a->num_levels_lsd > 16 || !a->inv_level_sigma_sq_lsd)
        return set_error(PLP_ERR_INVALID_ARG, "num_levels_lsd must be 1 .. 16, inv_level_sigma_sq_lsd is required");
    const int G = a->points.G, F = a->points.F;
    if (a->LL > kLaMaxObs || a->TL > kLaMaxObs) return set_error(PLP_ERR_UNSUPPORTED, "more than 2^18 lines or line observations");
    if ((long long)G * a->TL > kLaMaxWork || (long long)G * a->LL > kLaMaxWork) return set_error(PLP_ERR_UNSUPPORTED, "G * TL or G * LL above 2^22");
    if (G == 0) return PLP_OK;
    if (!a->obs_offsets_lines) return set_error(PLP_ERR_INVALID_ARG, "obs_offsets_lines is required");
    if (a->LL > 0 && !a->pluecker) return set_error(PLP_ERR_INVALID_ARG, "pluecker is required");
    if (a->TL > 0 && (!a->obs_kf_lines || !a->obs_idx_lines)) return set_error(PLP_ERR_INVALID_ARG, "obs_kf_lines and obs_idx_lines are required");
    if (F > 0 && a->kl_stride > 0 && !a->keylines) return set_error(PLP_ERR_INVALID_ARG, "keylines is required");
    if (outputs && ((a->LL > 0 && (!a->out_line_role || !a->out_pluecker)) || (a->TL > 0 && !a->out_outlier_lines)))
        return set_error(PLP_ERR_INVALID_ARG, "out_line_role, out_pluecker and out_outlier_lines are required");
    if (host) {
        if (a->obs_offsets_lines[0] != 0 || a->obs_offsets_lines[a->LL] != a->TL) return set_error(PLP_ERR_INVALID_ARG, "obs_offsets_lines must rise from 0 to TL");
        for (int l = 0; l < a->LL; ++l)
            if (a->obs_offsets_lines[l + 1] < a->obs_offsets_lines[l]) return set_error(PLP_ERR_INVALID_ARG, "obs_offsets_lines must rise from 0 to TL");
    }
    return PLP_OK;
}

LlArgs ll_args(const plp_local_ba_lines_args* a) {
    LlArgs A{};
    A.p = la_args(&a->points);
    A.LL = a->LL; A.TL = a->TL; A.kl_stride = a->kl_stride; A.num_levels_lsd = a->num_levels_lsd;
    for (int l = 0; l < 16; ++l) A.inv_sigma_sq_lsd[l] = l < A.num_levels_lsd ? a->inv_level_sigma_sq_lsd[l] : 0.0f;
    A.keylines = a->keylines; A.kl_counts = a->kl_counts; A.pluecker = a->pluecker; A.line_erased = a->line_erased;
    A.obs_offsets_lines = a->obs_offsets_lines; A.obs_kf_lines = a->obs_kf_lines; A.obs_idx_lines = a->obs_idx_lines;
    A.out_line_role = a->out_line_role; A.out_pluecker = a->out_pluecker; A.out_outlier_lines = a->out_outlier_lines;
    return A;
}

// the lines' state lies behind the G problems' state of local_ba.hpp in the same three rooms (ll_offsets)
extern "C++" template <class R> void ll_plan(R& r, plp_matcher* c, LlArgs& A) {
    const size_t G = (size_t)A.p.G, F = (size_t)A.p.F, L = (size_t)A.p.L, T = (size_t)A.p.T, K = (size_t)A.p.kp_stride;
    const size_t LL = (size_t)A.LL, TL = (size_t)A.TL, KL = (size_t)A.kl_stride;
    LaArgs& B = A.p;
    r.in(B.pose, F * B.pose_stride); r.in(B.kf_erased, F); r.in(B.kf_is_origin, F); r.in(B.undist, F * K); r.in(B.x_right, F * K); r.in(B.counts, F);
    r.in(B.pos_w, L * 3); r.in(B.lm_erased, L); r.in(B.obs_offsets, L + 1); r.in(B.obs_kf, T); r.in(B.obs_idx, T); r.in(B.kf_local, G * F);
    r.in(A.keylines, F * KL); r.in(A.kl_counts, F); r.in(A.pluecker, LL * 6); r.in(A.line_erased, LL); r.in(A.obs_offsets_lines, LL + 1);
    r.in(A.obs_kf_lines, TL); r.in(A.obs_idx_lines, TL);
    r.out(B.out_status, G); r.out(B.out_kf_role, G * F); r.out(B.out_lm_role, G * L); r.out(B.out_pose, G * F * 15); r.out(B.out_pos_w, G * L * 3);
    r.out(B.out_outlier, G * T); r.out(B.out_round_info, G * 8); r.out(B.out_round_chi2, G * 4);
    r.out(A.out_line_role, G * LL); r.out(A.out_pluecker, G * LL * 6); r.out(A.out_outlier_lines, G * TL);
    r.room(c->la_d, B.ctx_d, G * (la_doubles(B.F, B.L, B.T) + ll_doubles(A.LL, A.TL)));
    r.room(c->la_i, B.ctx_i, G * (la_ints(B.T) + ll_ints(A.TL)));
    r.room(c->la_b, B.ctx_b, G * (la_bytes(B.F, B.L, B.T) + ll_bytes(A.LL, A.TL)) + 16);
}

// the state of the host builds: one problem's worth
struct LlHostCtx {
    std::vector<double> d; std::vector<int32_t> i; std::vector<uint8_t> b;
    void bind(LlArgs& A) {
        d.assign(la_doubles(A.p.F, A.p.L, A.p.T) + ll_doubles(A.LL, A.TL), 0.0); i.assign(la_ints(A.p.T) + ll_ints(A.TL), 0);
        b.assign(la_bytes(A.p.F, A.p.L, A.p.T) + ll_bytes(A.LL, A.TL) + 1, 0);
        A.p.ctx_d = d.data(); A.p.ctx_i = i.data(); A.p.ctx_b = b.data();
    }
};
LlArgs ll_one(const LlArgs& A, int g) {
    LlArgs B = A;
    B.p = la_one(A.p, g);
    B.out_line_role = A.out_line_role ? A.out_line_role + (size_t)g * A.LL : nullptr;
    B.out_pluecker = A.out_pluecker ? A.out_pluecker + (size_t)g * A.LL * 6 : nullptr;
    B.out_outlier_lines = A.out_outlier_lines ? A.out_outlier_lines + (size_t)g * A.TL : nullptr;
    return B;
}
}  // namespace

plp_status plp_local_ba_lines_device(plp_matcher* c, const plp_local_ba_lines_args* a, void* hip_stream) {
    if (!c) return set_error(PLP_ERR_INVALID_ARG, "ctx is NULL");
    if (plp_status s = ll_check(a, true, false)) return s;
    if (a->points.G == 0) return PLP_OK;
    return device_call(c, hip_stream, ll_args(a), ll_plan<DeviceRooms>, launch_local_ba_lines);
}

plp_status plp_local_ba_lines_host(plp_matcher* c, const plp_local_ba_lines_args* a) {
    if (!c) return set_error(PLP_ERR_INVALID_ARG, "ctx is NULL");
    if (plp_status s = ll_check(a, true, true)) return s;
    if (a->points.G == 0) return PLP_OK;
    return host_call(c, ll_args(a), ll_plan<Stage>, launch_local_ba_lines);
}

// the host builds of local_ba_lines.hpp (no HIP call)
int32_t plp_model_local_ba_lines_host(const plp_local_ba_lines_args* a) {
    if (plp_status s = ll_check(a, true, true)) return -(int32_t)s;
    const LlArgs A = ll_args(a);
    for (int g = 0; g < A.p.G; ++g) {
        LlArgs B = ll_one(A, g);
        LlHostCtx ctx;
        ctx.bind(B);
        LlShared sh{};
        LaTeamHost par;
        ll_prepare(B, 0, sh, par);
        ll_solve(B, 0, sh, par);
        ll_finish(B, 0, par);
    }
    return A.p.G;
}

int32_t plp_model_line_oplus_host(const double* line, const double* update, int32_t n, double* out) {
    if (n < 0 || (n > 0 && (!line || !update || !out))) return -1;
    for (int32_t i = 0; i < n; ++i) ll_oplus(line + 6 * (size_t)i, update + 4 * (size_t)i, out + 6 * (size_t)i);
    return n;
}

int32_t plp_model_local_ba_lines_linearize_host(const plp_local_ba_lines_args* a, int32_t robust, int32_t* out_free_kf, double* out_hpp, double* out_hll,
                                                double* out_hnn, double* out_w_lines, double* out_chi2, double* out_edge_chi2_lines) {
    if (plp_status s = ll_check(a, false, true)) return -(int32_t)s;
    if (a->points.G != 1) return -(int32_t)set_error(PLP_ERR_INVALID_ARG, "G must be 1");
    LlArgs B = ll_args(a);
    LlHostCtx ctx;
    ctx.bind(B);
    LlShared sh{};
    LaTeamHost par;
    ll_prepare(B, 0, sh, par);
    LaOff O;
    la_offsets(B.p, 0, O);
    const LaView V = la_view(B.p, O);
    LlOff Q;
    ll_offsets(B, 0, Q);
    const LlView W = ll_view(B, Q);
    LlLines lines{{B.LL, B.TL, B.obs_offsets_lines}, W, sh};
    sh.delta_lines = B.p.delta_2d;
    if (!la_model_linearize(B.p, V, sh.s, lines, robust != 0, out_free_kf, out_hpp, out_hll, out_chi2)) return 0;
    for (int l = 0; l < B.LL; ++l)
        if (out_hnn && W.act()[l]) for (int t = 0; t < 14; ++t) out_hnn[(size_t)14 * l + t] = ll_l(W, l, kLlLnH + t);
    for (int t = 0; t < B.TL; ++t) {
        if (W.e_kf()[t] < 0) continue;
        if (out_edge_chi2_lines) out_edge_chi2_lines[t] = ll_e(W, t, kLlRowChi);
        if (out_w_lines && sh.s.kf2ai[W.e_kf()[t]] >= 0) for (int k = 0; k < 24; ++k) out_w_lines[(size_t)24 * t + k] = ll_e(W, t, kLlRowW + k);
    }
    return sh.s.nfa;
}

int32_t plp_model_local_ba_lines_solve_host(int32_t P, int32_t M, int32_t N, int32_t E3, int32_t E4, const double* hpp, const double* hll, const double* hnn,
                                            const int32_t* e_pose, const int32_t* e_lm, const double* w, const int32_t* e_pose_lines, const int32_t* e_line,
                                            const double* w_lines, double lambda, double* out_xp, double* out_xl, double* out_xn) {
    if (P < 0 || P > kLaMaxFree || !la_model_edges_ok(P, M, E3, e_pose, e_lm) || !la_model_edges_ok(P, N, E4, e_pose_lines, e_line) || (P > 0 && (!hpp || !out_xp)) ||
        (M > 0 && (!hll || !out_xl)) || (N > 0 && (!hnn || !out_xn)) || (E3 > 0 && !w) || (E4 > 0 && !w_lines)) return -1;
    // the lines' blocks beside la_model_solve's problem: N lines and their E4 observations
    LlArgs B{};
    B.p.G = 1; B.p.F = P + 1; B.p.L = M; B.p.T = E3; B.LL = N; B.TL = E4;
    const std::vector<int32_t> off = la_model_offsets(M, E3, e_lm), offl = la_model_offsets(N, E4, e_line);
    B.p.obs_offsets = off.data(); B.obs_offsets_lines = offl.data();
    LlHostCtx ctx;
    ctx.bind(B);
    LlShared sh{};
    LaOff O;
    la_offsets(B.p, 0, O);
    LlOff Q;
    ll_offsets(B, 0, Q);
    const LlView W = ll_view(B, Q);
    for (int l = 0; l < N; ++l) W.role()[l] = 1;
    for (int e = 0; e < E4; ++e) { W.e_kf()[e] = e_pose_lines[e] < 0 ? P : e_pose_lines[e]; W.e_l()[e] = e_line[e]; W.lvl()[e] = 0; }
    for (int l = 0; l < N; ++l) for (int t = 0; t < 14; ++t) ll_l(W, l, kLlLnH + t) = hnn[(size_t)14 * l + t];
    for (int e = 0; e < E4; ++e) for (int k = 0; k < 24; ++k) ll_e(W, e, kLlRowW + k) = w_lines[(size_t)24 * e + k];
    LlLines lines{{B.LL, B.TL, B.obs_offsets_lines}, W, sh};
    const int32_t ok = la_model_solve(B.p, la_view(B.p, O), sh.s, lines, hpp, hll, e_pose, e_lm, w, lambda, out_xp, out_xl);
    for (int l = 0; l < N; ++l) for (int k = 0; k < 4; ++k) out_xn[(size_t)4 * l + k] = W.act()[l] ? ll_l(W, l, kLlLnX + k) : 0.0;
    return ok;
}

}  // extern "C"
