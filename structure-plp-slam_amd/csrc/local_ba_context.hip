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
    LaNoLines none;
    if (!la_model_linearize(B, V, sh, none, robust != 0, out_free_kf, out_hpp, out_hll, out_chi2)) return 0;
    for (int t = 0; t < B.T; ++t) {
        if (V.e_kf()[t] < 0) continue;
        if (out_edge_chi2) out_edge_chi2[t] = la_e(V, t, kLaRowChi);
        if (out_w && sh.kf2ai[V.e_kf()[t]] >= 0) for (int k = 0; k < 18; ++k) out_w[(size_t)18 * t + k] = la_e(V, t, kLaRowW + k);
    }
    return sh.nfa;
}

int32_t plp_model_local_ba_solve_host(int32_t P, int32_t M, int32_t E, const double* hpp, const double* hll, const int32_t* e_pose, const int32_t* e_lm,
                                      const double* w, double lambda, double* out_xp, double* out_xl) {
    if (P < 0 || P > kLaMaxFree || !la_model_edges_ok(P, M, E, e_pose, e_lm) || (P > 0 && (!hpp || !out_xp)) || (M > 0 && (!hll || !out_xl)) || (E > 0 && !w)) return -1;
    LaArgs B{};
    B.G = 1; B.F = P + 1; B.L = M; B.T = E;
    const std::vector<int32_t> off = la_model_offsets(M, E, e_lm);
    B.obs_offsets = off.data();
    LaHostCtx ctx;
    ctx.bind(B);
    LaShared sh{};
    LaOff O;
    la_offsets(B, 0, O);
    LaNoLines none;
    return la_model_solve(B, la_view(B, O), sh, none, hpp, hll, e_pose, e_lm, w, lambda, out_xp, out_xl);
}

int32_t plp_model_inv3_host(const double* a, int32_t n, double* out, int32_t* out_ok) {
    if (n < 0 || (n > 0 && (!a || !out || !out_ok))) return -1;
    for (int32_t i = 0; i < n; ++i) out_ok[i] = la_inv3(a + 6 * (size_t)i, out + 6 * (size_t)i) ? 1 : 0;
    return n;
}

}  // extern "C"
