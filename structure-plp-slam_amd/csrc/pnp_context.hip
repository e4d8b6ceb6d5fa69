// Host driver + C ABI of the matcher context: relocalisation: solve::pnp_solver (include/plp_front.h: plp_pnp_ransac_*; pnp_kernels.hip, pnp.hpp)
#include <hip/hip_runtime.h>

#include <vector>

#include "matcher_context.hpp"
#include "pnp.hpp"

using namespace plp;

extern "C" {

namespace {
plp_status pnp_check(const plp_pnp_ransac_args* a) {
    if (!a) return set_error(PLP_ERR_INVALID_ARG, "NULL argument");
    if (a->P < 0 || a->n_cap < 0) return set_error(PLP_ERR_INVALID_ARG, "P and n_cap must not be negative");
    if (a->iters < 1 || a->min_num_inliers < 0) return set_error(PLP_ERR_INVALID_ARG, "iters must be positive, min_num_inliers non-negative");
    if (a->num_levels < 1 || a->num_levels > 16 || !a->scale_factors) return set_error(PLP_ERR_INVALID_ARG, "num_levels must be 1 .. 16, scale_factors is required");
    if (a->n_cap > kPnpMaxSlots) return set_error(PLP_ERR_UNSUPPORTED, "more than 8192 slots per problem");
    if (a->P > 65535) return set_error(PLP_ERR_UNSUPPORTED, "more than 65535 problems in one call");
    if (a->P == 0 || a->n_cap == 0) return PLP_OK;
    if (!a->valid || !a->bearing || !a->pos_w || !a->octave) return set_error(PLP_ERR_INVALID_ARG, "valid, bearing, pos_w, octave are required");
    if (!a->out_status || !a->out_num_matches || !a->out_rot_cw || !a->out_trans_cw || !a->out_num_inliers || !a->out_best_iter)
        return set_error(PLP_ERR_INVALID_ARG, "out_status, out_num_matches, out_rot_cw, out_trans_cw, out_num_inliers, out_best_iter are required");
    return PLP_OK;
}

PnpArgs pnp_args(const plp_pnp_ransac_args* a) {
    PnpArgs A{};
    A.P = a->P; A.n_cap = a->n_cap; A.iters = a->iters; A.min_num_inliers = a->min_num_inliers; A.recompute = a->recompute != 0;
    A.num_levels = a->num_levels; A.seed = a->seed;
    for (int l = 0; l < 16; ++l) A.thr[l] = l < a->num_levels ? pnp_level_threshold(a->scale_factors[l]) : 0.0f;
    A.valid = a->valid; A.bearing = a->bearing; A.pos_w = a->pos_w; A.octave = a->octave; A.counts = a->counts; A.samples = a->samples;
    A.out_status = a->out_status; A.out_num_matches = a->out_num_matches; A.out_rot_cw = a->out_rot_cw; A.out_trans_cw = a->out_trans_cw;
    A.out_num_inliers = a->out_num_inliers; A.out_best_iter = a->out_best_iter; A.out_inliers = a->out_inliers; A.out_hyp_inliers = a->out_hyp_inliers;
    return A;
}

// the arrays of the call; the rooms are what the launches hand to one another
extern "C++" template <class R> void pnp_plan(R& r, plp_matcher* c, PnpArgs& A) {
    const size_t P = (size_t)A.P, M = (size_t)A.n_cap, I = (size_t)A.iters;
    r.in(A.valid, P * M); r.in(A.bearing, P * M * 3); r.in(A.pos_w, P * M * 3); r.in(A.octave, P * M); r.in(A.counts, P); r.in(A.samples, P * I * 4);
    r.out(A.out_status, P, false); r.out(A.out_num_matches, P, false); r.out(A.out_rot_cw, P * 9, false); r.out(A.out_trans_cw, P * 3, false);
    r.out(A.out_num_inliers, P, false); r.out(A.out_best_iter, P, false); r.out(A.out_inliers, P * M); r.out(A.out_hyp_inliers, P * I, false);
    r.room(c->pnp_ctx, A.ctx, P * kPnpCtxInts); r.room(c->pnp_slot, A.ctx_slot, P * M); r.room(c->pnp_hyp, A.ctx_hyp, P * kPnpHypDoubles * I);
    r.room(c->pnp_corr, A.ctx_corr, P * M * kPnpCorrDoubles); r.room(c->pnp_pose, A.ctx_pose, P * 12); r.room(c->pnp_sign, A.ctx_sign, P);
}

// compute_pose (:230-290) of the host build for nc >= 1 correspondences held kPnpCorrDoubles apart; returns the chosen approximation 0 .. 2
int pnp_model_pose(PnpWork& W, double* corr, int nc, int sign0) {
    std::vector<double> G(144), V(144);
    pnp_pose_front(W, corr, corr + 3, corr + 5, kPnpCorrDoubles, nc);
    pnp_null_space(W, G.data(), V.data());
    return pnp_pose_back(W, corr, corr + 3, corr + 5, corr + 9, kPnpCorrDoubles, nc, sign0);
}

// one problem of the host build: the kernels' steps, one hypothesis and one match after the other
void pnp_model_problem(const PnpArgs& A, int p) {
    const int count = clamp_count(A.counts, p, A.n_cap);
    const size_t row = (size_t)p * A.n_cap;
    std::vector<int> slot_of;
    for (int s = 0; s < count; ++s)
        if (A.valid[row + s]) slot_of.push_back(s);
    const int n = (int)slot_of.size();
    auto inlier = [&](const double* R, const double* t, int k) {
        const size_t s = row + slot_of[k];
        const int o = A.octave[s];
        const bool lv = (unsigned)o < (unsigned)A.num_levels;
        return pnp_inlier(R, t, A.pos_w + 3 * s, A.bearing + 3 * s, lv ? A.thr[o] : 0.0f, !lv);
    };
    int best_count = 0, best_iter = -1;
    double best[12] = {0};
    std::vector<uint8_t> best_flags((size_t)n, 0), flags((size_t)n, 0);
    std::vector<double> corr((size_t)(n > 4 ? n : 4) * kPnpCorrDoubles);
    PnpWork W;
    const bool enough = !(n < 4 || n < A.min_num_inliers);          // :76
    for (int it = 0; it < A.iters; ++it) {
        int num = 0;
        int idx[4];
        if (enough && ransac_sample<4>(A, p, it, n, idx)) {
            int nc = 0, sign0 = 0;
            for (int k = 0; k < 4; ++k) {
                const size_t s = row + slot_of[idx[k]];
                int sg;
                if (pnp_add_correspondence(A.pos_w + 3 * s, A.bearing + 3 * s, corr.data() + nc * kPnpCorrDoubles, corr.data() + nc * kPnpCorrDoubles + 3, sg)) {
                    if (nc == 0) sign0 = sg;
                    ++nc;
                }
            }
            if (nc > 0) {
                const int N = pnp_model_pose(W, corr.data(), nc, sign0);
                for (int k = 0; k < n; ++k) { flags[k] = inlier(W.Rs + 9 * N, W.ts + 3 * N, k) ? 1 : 0; num += flags[k]; }
                if (best_count < num) {                             // :117
                    best_count = num; best_iter = it; best_flags = flags;
                    for (int i = 0; i < 9; ++i) best[i] = W.Rs[9 * N + i];
                    for (int i = 0; i < 3; ++i) best[9 + i] = W.ts[3 * N + i];
                }
            }
        }
        if (A.out_hyp_inliers) A.out_hyp_inliers[(size_t)p * A.iters + it] = num;
    }
    const bool ok = enough && best_count > A.min_num_inliers;       // :126
    const bool have = ok && best_iter >= 0;
    if (have && A.recompute) {                                      // :136-152
        int nc = 0, sign0 = 0;
        for (int k = 0; k < n; ++k) {
            if (!best_flags[k]) continue;
            const size_t s = row + slot_of[k];
            int sg;
            if (pnp_add_correspondence(A.pos_w + 3 * s, A.bearing + 3 * s, corr.data() + (size_t)nc * kPnpCorrDoubles, corr.data() + (size_t)nc * kPnpCorrDoubles + 3, sg)) {
                if (nc == 0) sign0 = sg;
                ++nc;
            }
        }
        if (nc > 0) {
            const int N = pnp_model_pose(W, corr.data(), nc, sign0);
            for (int i = 0; i < 9; ++i) best[i] = W.Rs[9 * N + i];
            for (int i = 0; i < 3; ++i) best[9 + i] = W.ts[3 * N + i];
        }
    }
    A.out_status[p] = !enough ? PLP_PNP_TOO_FEW_MATCHES : ok ? PLP_PNP_OK : PLP_PNP_TOO_FEW_INLIERS;
    A.out_num_matches[p] = n;
    A.out_num_inliers[p] = best_count;
    A.out_best_iter[p] = ok ? best_iter : -1;
    for (int i = 0; i < 9; ++i) A.out_rot_cw[(size_t)9 * p + i] = have ? best[i] : 0.0;
    for (int i = 0; i < 3; ++i) A.out_trans_cw[(size_t)3 * p + i] = have ? best[9 + i] : 0.0;
    if (A.out_inliers) {
        for (int s = 0; s < count; ++s) A.out_inliers[row + s] = 0;
        if (have)
            for (int k = 0; k < n; ++k) A.out_inliers[row + slot_of[k]] = best_flags[k];
    }
}
}  // namespace

plp_status plp_pnp_ransac_device(plp_matcher* c, const plp_pnp_ransac_args* a, void* hip_stream) {
    if (!c) return set_error(PLP_ERR_INVALID_ARG, "ctx is NULL");
    if (plp_status s = pnp_check(a)) return s;
    if (a->P == 0 || a->n_cap == 0) return PLP_OK;
    return device_call(c, hip_stream, pnp_args(a), pnp_plan<DeviceRooms>, launch_pnp_ransac);
}

plp_status plp_pnp_ransac_host(plp_matcher* c, const plp_pnp_ransac_args* a) {
    if (!c) return set_error(PLP_ERR_INVALID_ARG, "ctx is NULL");
    if (plp_status s = pnp_check(a)) return s;
    if (a->P == 0 || a->n_cap == 0) return PLP_OK;
    return host_call(c, pnp_args(a), pnp_plan<Stage>, launch_pnp_ransac);
}

// the host builds of pnp.hpp (no HIP call)
int32_t plp_model_pnp_ransac_host(const plp_pnp_ransac_args* a) {
    if (pnp_check(a) != PLP_OK) return -1;
    if (a->P == 0 || a->n_cap == 0) return a->P;
    const PnpArgs A = pnp_args(a);
    for (int p = 0; p < A.P; ++p) pnp_model_problem(A, p);
    return A.P;
}

int32_t plp_model_epnp_host(const double* pos_w, const double* bearing, const int32_t* offsets, int32_t n, double* out_rot, double* out_trans,
                            double* out_err, int32_t* out_N, int32_t* out_sweeps) {
    if (n < 0 || (n > 0 && (!offsets || !out_rot || !out_trans || !out_err || !out_N))) return -1;
    for (int32_t i = 0; i < n; ++i)
        if (offsets[i + 1] < offsets[i] || offsets[i] < 0 || (offsets[i + 1] > offsets[i] && (!pos_w || !bearing))) return -1;
    PnpWork W;
    for (int32_t i = 0; i < n; ++i) {
        const int m = offsets[i + 1] - offsets[i];
        std::vector<double> corr((size_t)(m > 0 ? m : 1) * kPnpCorrDoubles);
        int nc = 0, sign0 = 0;
        for (int k = 0; k < m; ++k) {
            const size_t s = (size_t)offsets[i] + k;
            int sg;
            if (pnp_add_correspondence(pos_w + 3 * s, bearing + 3 * s, corr.data() + (size_t)nc * kPnpCorrDoubles, corr.data() + (size_t)nc * kPnpCorrDoubles + 3, sg)) {
                if (nc == 0) sign0 = sg;
                ++nc;
            }
        }
        for (int k = 0; k < 8; ++k) W.sweeps[k] = 0;
        int N = -1;
        if (nc > 0) N = pnp_model_pose(W, corr.data(), nc, sign0);
        for (int k = 0; k < 9; ++k) out_rot[9 * (size_t)i + k] = N >= 0 ? W.Rs[9 * N + k] : 0.0;
        for (int k = 0; k < 3; ++k) out_trans[3 * (size_t)i + k] = N >= 0 ? W.ts[3 * N + k] : 0.0;
        out_err[i] = N >= 0 ? W.err[N] : 0.0;
        out_N[i] = N + 1;
        if (out_sweeps)
            for (int k = 0; k < 8; ++k) out_sweeps[8 * (size_t)i + k] = W.sweeps[k];
    }
    return n;
}

int32_t plp_model_sym_jacobi_host(const double* A, int32_t dim, int32_t n, double* out_vals, double* out_ut, int32_t* out_sweeps) {
    if ((dim != 3 && dim != 12) || n < 0 || (n > 0 && (!A || !out_vals || !out_ut))) return -1;
    std::vector<double> G((size_t)dim * dim), V((size_t)dim * dim), key((size_t)dim);
    for (int32_t i = 0; i < n; ++i) {
        const int sweeps = sym_jacobi(A + (size_t)i * dim * dim, dim, G.data(), V.data(), key.data(), out_vals + (size_t)i * dim, out_ut + (size_t)i * dim * dim);
        if (out_sweeps) out_sweeps[i] = sweeps;
    }
    return n;
}

int32_t plp_model_lstsq6_host(const double* A, const double* b, int32_t k, int32_t n, double* out_x, int32_t* out_sweeps) {
    if (k < 3 || k > 5 || n < 0 || (n > 0 && (!A || !b || !out_x))) return -1;
    double G[30], V[25], key[5];
    for (int32_t i = 0; i < n; ++i) {
        for (int r = 0; r < 6; ++r)
            for (int c = 0; c < k; ++c) G[6 * c + r] = A[((size_t)i * 6 + r) * k + c];
        const int sweeps = lstsq6(G, b + 6 * (size_t)i, k, V, key, out_x + (size_t)i * k);
        if (out_sweeps) out_sweeps[i] = sweeps;
    }
    return n;
}

int32_t plp_model_rot_from_abt_host(const double* Abt, int32_t n, double* out_rot, int32_t* out_sweeps) {
    if (n < 0 || (n > 0 && (!Abt || !out_rot))) return -1;
    double G[9], V[9], key[3], U[9];
    for (int32_t i = 0; i < n; ++i) {
        const int sweeps = rot_from_abt(Abt + 9 * (size_t)i, G, V, key, U, out_rot + 9 * (size_t)i);
        if (out_sweeps) out_sweeps[i] = sweeps;
    }
    return n;
}

int32_t plp_model_pnp_draw_host(uint64_t seed, int32_t p, int32_t iter0, int32_t n_iters, int32_t num_matches, int32_t* out) {
    return ransac_draw_rows<4>(seed, p, iter0, n_iters, num_matches, out);
}

int32_t plp_model_pnp_thresholds_host(const float* scale_factors, int32_t num_levels, float* out) {
    if (num_levels < 0 || (num_levels > 0 && (!scale_factors || !out))) return -1;
    for (int32_t l = 0; l < num_levels; ++l) out[l] = pnp_level_threshold(scale_factors[l]);
    return num_levels;
}

}  // extern "C"
