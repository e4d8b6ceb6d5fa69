// Host driver + C ABI of the matcher context: local bundle adjustment: optimize::local_bundle_adjuster (include/plp_front.h: plp_local_ba_*; local_ba_kernels.hip, local_ba.hpp)
#include <hip/hip_runtime.h>

#include <vector>

#include "local_ba_entry.hpp"

using namespace plp;

extern "C" {

plp_status plp_local_ba_device(plp_matcher* c, const plp_local_ba_args* a, void* hip_stream) {
    if (!c) return set_error(PLP_ERR_INVALID_ARG, "ctx is NULL");
    if (plp_status s = la_check(a, true, false)) return s;
    if (a->G == 0) return PLP_OK;
    return device_call(c, hip_stream, la_args(a), la_plan<DeviceRooms>, launch_local_ba);
}

plp_status plp_local_ba_host(plp_matcher* c, const plp_local_ba_args* a) {
    if (!c) return set_error(PLP_ERR_INVALID_ARG, "ctx is NULL");
    if (plp_status s = la_check(a, true, true)) return s;
    if (a->G == 0) return PLP_OK;
    return host_call(c, la_args(a), la_plan<Stage>, launch_local_ba);
}

// the host builds of local_ba.hpp (no HIP call)
int32_t plp_model_local_ba_host(const plp_local_ba_args* a) {
    if (plp_status s = la_check(a, true, true)) return -(int32_t)s;
    const LaArgs A = la_args(a);
    for (int g = 0; g < A.G; ++g) {
        LaArgs B = la_one(A, g);
        LaHostCtx ctx;
        ctx.bind(B);
        LaShared sh{};
        LaTeamHost par;
        la_prepare(B, 0, sh, par);
        la_solve(B, 0, sh, par);
        la_finish(B, 0, par);
    }
    return A.G;
}

int32_t plp_model_local_ba_linearize_host(const plp_local_ba_args* a, int32_t robust, int32_t* out_free_kf, double* out_hpp, double* out_hll, double* out_w,
                                          double* out_chi2, double* out_edge_chi2) {
    if (plp_status s = la_check(a, false, true)) return -(int32_t)s;
    if (a->G != 1) return -(int32_t)set_error(PLP_ERR_INVALID_ARG, "G must be 1");
    LaArgs B = la_args(a);
    LaHostCtx ctx;
    ctx.bind(B);
    LaShared sh{};
    LaTeamHost par;
    la_prepare(B, 0, sh, par);
    LaOff O;
    la_offsets(B, 0, O);
    const LaView V = la_view(B, O);
    if (out_free_kf) for (int i = 0; i < kLaMaxFree; ++i) out_free_kf[i] = -1;
    if (V.hdr()[kLaHStatus] != PLP_LOCAL_BA_OK) { if (out_chi2) out_chi2[0] = 0.0; return 0; }
    sh.cam = B.cam; sh.delta = B.mono_setup ? B.delta_2d : B.delta_3d;
    la_round_setup(B, V, sh, par);
    la_edge_pass(B, V, sh, par, true, robust != 0);
    la_sums(B, V, sh, par, true);
    sh.acc = 0.0;
    la_chain(B, V, sh, par, 0, kLaLmPart);
    if (out_chi2) out_chi2[0] = sh.acc;
    for (int i = 0; i < sh.nfa; ++i) {
        if (out_free_kf) out_free_kf[i] = sh.akf[i];
        if (out_hpp) for (int t = 0; t < 27; ++t) out_hpp[27 * i + t] = la_p(V, i, t);
    }
    for (int l = 0; l < B.L; ++l)
        if (out_hll && V.lm_act()[l]) for (int t = 0; t < 9; ++t) out_hll[(size_t)9 * l + t] = la_l(V, l, kLaLmH + t);
    for (int t = 0; t < B.T; ++t) {
        if (V.e_kf()[t] < 0) continue;
        if (out_edge_chi2) out_edge_chi2[t] = la_e(V, t, kLaRowChi);
        if (out_w && sh.kf2ai[V.e_kf()[t]] >= 0) for (int k = 0; k < 18; ++k) out_w[(size_t)18 * t + k] = la_e(V, t, kLaRowW + k);
    }
    return sh.nfa;
}

int32_t plp_model_local_ba_solve_host(int32_t P, int32_t M, int32_t E, const double* hpp, const double* hll, const int32_t* e_pose, const int32_t* e_lm,
                                      const double* w, double lambda, double* out_xp, double* out_xl) {
    if (P < 0 || P > kLaMaxFree || M < 0 || M > kLaMaxObs || E < 0 || E > kLaMaxObs || (P > 0 && (!hpp || !out_xp)) || (M > 0 && (!hll || !out_xl)) ||
        (E > 0 && (!e_pose || !e_lm || !w))) return -1;
    for (int e = 0; e < E; ++e)
        if (e_pose[e] < -1 || e_pose[e] >= P || e_lm[e] < 0 || e_lm[e] >= M || (e > 0 && e_lm[e] < e_lm[e - 1])) return -1;
    // the blocks as a problem of P + 1 key frames (row P: the constant pose), M landmarks and E observations
    LaArgs B{};
    B.G = 1; B.F = P + 1; B.L = M; B.T = E;
    std::vector<int32_t> off(M + 1, 0);
    for (int e = 0; e < E; ++e) off[e_lm[e] + 1] += 1;
    for (int l = 0; l < M; ++l) off[l + 1] += off[l];
    B.obs_offsets = off.data();
    LaHostCtx ctx;
    ctx.bind(B);
    LaShared sh{};
    LaTeamHost par;
    LaOff O;
    la_offsets(B, 0, O);
    const LaView V = la_view(B, O);
    V.hdr()[kLaHNf] = P;
    for (int i = 0; i < P; ++i) V.hdr()[kLaHFl + i] = i;
    for (int l = 0; l < M; ++l) V.lm_role()[l] = 1;
    for (int e = 0; e < E; ++e) { V.e_kf()[e] = e_pose[e] < 0 ? P : e_pose[e]; V.e_l()[e] = e_lm[e]; V.lvl()[e] = 0; }
    la_round_setup(B, V, sh, par);
    for (int i = 0; i < sh.nfa; ++i) for (int t = 0; t < 27; ++t) la_p(V, i, t) = hpp[27 * sh.akf[i] + t];
    for (int l = 0; l < M; ++l) for (int t = 0; t < 9; ++t) la_l(V, l, kLaLmH + t) = hll[(size_t)9 * l + t];
    for (int e = 0; e < E; ++e) for (int k = 0; k < 18; ++k) la_e(V, e, kLaRowW + k) = w[(size_t)18 * e + k];
    sh.lambda = lambda;
    la_solve_system(B, V, sh, par);
    for (int i = 0; i < 6 * P; ++i) out_xp[i] = 0.0;
    for (int i = 0; i < sh.nfa; ++i) for (int k = 0; k < 6; ++k) out_xp[6 * sh.akf[i] + k] = sh.x[6 * i + k];
    for (int l = 0; l < M; ++l) for (int k = 0; k < 3; ++k) out_xl[(size_t)3 * l + k] = V.lm_act()[l] ? la_l(V, l, kLaLmX + k) : 0.0;
    return sh.ok ? 1 : 0;
}

int32_t plp_model_inv3_host(const double* a, int32_t n, double* out, int32_t* out_ok) {
    if (n < 0 || (n > 0 && (!a || !out || !out_ok))) return -1;
    for (int32_t i = 0; i < n; ++i) out_ok[i] = la_inv3(a + 6 * (size_t)i, out + 6 * (size_t)i) ? 1 : 0;
    return n;
}

}  // extern "C"
