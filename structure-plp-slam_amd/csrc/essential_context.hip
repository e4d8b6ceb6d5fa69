// Host driver + C ABI of the matcher context: map initialisation and the robust match: solve::essential_solver (include/plp_front.h:
// plp_essential_ransac_*; essential_kernels.hip, essential.hpp)
#include <hip/hip_runtime.h>

#include <vector>

#include "essential.hpp"
#include "matcher_context.hpp"

using namespace plp;

extern "C" {

namespace {
plp_status ess_check(const plp_essential_ransac_args* a) {
    if (!a) return set_error(PLP_ERR_INVALID_ARG, "NULL argument");
    if (a->P < 0 || a->n_cap < 0 || a->m_cap < 0) return set_error(PLP_ERR_INVALID_ARG, "P, n_cap and m_cap must not be negative");
    if (a->iters < 1) return set_error(PLP_ERR_INVALID_ARG, "iters must be positive");
    if (a->n_cap > kEssMaxSlots) return set_error(PLP_ERR_UNSUPPORTED, "more than 8192 slots per problem");
    if (a->P > 65535) return set_error(PLP_ERR_UNSUPPORTED, "more than 65535 problems in one call");
    if (a->iters > kEssMaxIters) return set_error(PLP_ERR_UNSUPPORTED, "more than 65536 iterations");
    if (a->P == 0 || a->n_cap == 0) return PLP_OK;
    if (!a->bearing_1 || !a->match || (a->m_cap > 0 && !a->bearing_2)) return set_error(PLP_ERR_INVALID_ARG, "bearing_1, bearing_2, match are required");
    if (!a->out_status || !a->out_num_matches || !a->out_E_21 || !a->out_score || !a->out_num_inliers || !a->out_best_iter)
        return set_error(PLP_ERR_INVALID_ARG, "out_status, out_num_matches, out_E_21, out_score, out_num_inliers, out_best_iter are required");
    return PLP_OK;
}

EssArgs ess_args(const plp_essential_ransac_args* a) {
    EssArgs A{};
    A.P = a->P; A.n_cap = a->n_cap; A.m_cap = a->m_cap; A.iters = a->iters; A.recompute = a->recompute != 0; A.seed = a->seed;
    A.bearing_1 = a->bearing_1; A.bearing_2 = a->bearing_2; A.match = a->match; A.counts_1 = a->counts_1; A.counts_2 = a->counts_2; A.samples = a->samples;
    A.out_status = a->out_status; A.out_num_matches = a->out_num_matches; A.out_E_21 = a->out_E_21; A.out_score = a->out_score;
    A.out_num_inliers = a->out_num_inliers; A.out_best_iter = a->out_best_iter; A.out_inliers = a->out_inliers; A.out_hyp_score = a->out_hyp_score;
    return A;
}

// the arrays of the call; the rooms are what the launches hand to one another
extern "C++" template <class R> void ess_plan(R& r, plp_matcher* c, EssArgs& A) {
    const size_t P = (size_t)A.P, M = (size_t)A.n_cap, M2 = (size_t)A.m_cap, I = (size_t)A.iters;
    r.in(A.bearing_1, P * M * 3); r.in(A.bearing_2, P * M2 * 3); r.in(A.match, P * M); r.in(A.counts_1, P); r.in(A.counts_2, P); r.in(A.samples, P * I * 8);
    r.out(A.out_status, P, false); r.out(A.out_num_matches, P, false); r.out(A.out_E_21, P * 9, false); r.out(A.out_score, P, false);
    r.out(A.out_num_inliers, P, false); r.out(A.out_best_iter, P, false); r.out(A.out_inliers, P * M); r.out(A.out_hyp_score, P * I, false);
    r.room(c->ess_ctx, A.ctx, P * kEssCtxInts); r.room(c->ess_slot, A.ctx_slot, P * M); r.room(c->ess_hyp, A.ctx_hyp, P * kEssHypDoubles * I);
    r.room(c->ess_pairs, A.ctx_pairs, P * M * kEssPairDoubles); r.room(c->ess_E, A.ctx_E, P * 9); r.room(c->ess_code, A.ctx_code, P * M); r.room(c->ess_key, A.ctx_key, P);
}

struct EssScratch { double M[81], G[81], V[81], null9[9], key[3]; };

// check_inliers (:196-253) of the host build over the matches held as bearing pairs: the score; code[k] as ess_residuals gives it
float ess_model_check(const double* E, const double* pairs, int n, uint8_t* code) {
    float score = 0;
    for (int k = 0; k < n; ++k) {
        float r2, r1;
        const int c = ess_residuals(E, pairs + (size_t)k * kEssPairDoubles, pairs + (size_t)k * kEssPairDoubles + 3, r2, r1);
        score = ess_score_add(score, c, r2, r1);
        code[k] = (uint8_t)c;
    }
    return score;
}

// one problem of the host build: the kernels' steps, one hypothesis and one match after the other
void ess_model_problem(const EssArgs& A, int p) {
    const int count_1 = clamp_count(A.counts_1, p, A.n_cap), count_2 = clamp_count(A.counts_2, p, A.m_cap);
    const size_t row = (size_t)p * A.n_cap;
    std::vector<int> slot_of;
    for (int s = 0; s < count_1; ++s)
        if (ess_matched(A, p, s, count_2)) slot_of.push_back(s);
    const int n = (int)slot_of.size();
    std::vector<double> pairs((size_t)(n > 0 ? n : 1) * kEssPairDoubles), fit((size_t)(n > kEssMinSet ? n : kEssMinSet) * kEssPairDoubles);
    for (int k = 0; k < n; ++k)
        for (int c = 0; c < 3; ++c) {
            pairs[(size_t)k * kEssPairDoubles + c] = A.bearing_1[3 * (row + slot_of[k]) + c];
            pairs[(size_t)k * kEssPairDoubles + 3 + c] = A.bearing_2[3 * ((size_t)p * A.m_cap + A.match[row + slot_of[k]]) + c];
        }
    const bool enough = n >= kEssMinSet;                            // :45
    float best_score = 0.0f;                                        // :52
    int best_iter = -1;
    double best_E[9] = {0};
    std::vector<uint8_t> best_code((size_t)n, 0), code((size_t)n, 0);
    EssScratch S;
    double E[9];
    for (int it = 0; it < A.iters; ++it) {
        float score = 0;
        int idx[8];
        if (enough && ransac_sample<kEssMinSet>(A, p, it, n, idx)) {
            for (int k = 0; k < 8; ++k)                             // :73-78
                for (int c = 0; c < kEssPairDoubles; ++c) fit[(size_t)k * kEssPairDoubles + c] = pairs[(size_t)idx[k] * kEssPairDoubles + c];
            ess_fit(fit.data(), kEssPairDoubles, kEssMinSet, S.M, S.G, S.V, S.null9, S.key, E, nullptr);   // :81
            score = ess_model_check(E, pairs.data(), n, code.data());                                     // :84
            if (best_score < score) {                               // :87
                best_score = score; best_iter = it; best_code = code;
                for (int i = 0; i < 9; ++i) best_E[i] = E[i];
            }
        }
        if (A.out_hyp_score) A.out_hyp_score[(size_t)p * A.iters + it] = score;
    }
    int num = 0;
    for (int k = 0; k < n; ++k) num += best_code[k] == 3 ? 1 : 0;
    const bool valid = enough && best_score > 0.0f && num >= kEssMinSet;   // :96
    if (valid && A.recompute) {                                     // :103-118
        int nc = 0;
        for (int k = 0; k < n; ++k)
            if (best_code[k] == 3) {
                for (int c = 0; c < kEssPairDoubles; ++c) fit[(size_t)nc * kEssPairDoubles + c] = pairs[(size_t)k * kEssPairDoubles + c];
                ++nc;
            }
        ess_fit(fit.data(), kEssPairDoubles, nc, S.M, S.G, S.V, S.null9, S.key, best_E, nullptr);
        best_score = ess_model_check(best_E, pairs.data(), n, best_code.data());
        num = 0;
        for (int k = 0; k < n; ++k) num += best_code[k] == 3 ? 1 : 0;
    }
    A.out_status[p] = !enough ? PLP_ESSENTIAL_TOO_FEW_MATCHES : valid ? PLP_ESSENTIAL_OK : PLP_ESSENTIAL_INVALID;
    A.out_num_matches[p] = n;
    for (int i = 0; i < 9; ++i) A.out_E_21[(size_t)9 * p + i] = valid ? best_E[i] : 0.0;
    A.out_score[p] = valid ? best_score : 0.0f;
    A.out_num_inliers[p] = valid ? num : 0;
    A.out_best_iter[p] = valid ? best_iter : -1;
    if (A.out_inliers) {
        for (int s = 0; s < count_1; ++s) A.out_inliers[row + s] = 0;
        if (valid)
            for (int k = 0; k < n; ++k) A.out_inliers[row + slot_of[k]] = best_code[k] == 3 ? 1 : 0;
    }
}
}  // namespace

plp_status plp_essential_ransac_device(plp_matcher* c, const plp_essential_ransac_args* a, void* hip_stream) {
    if (!c) return set_error(PLP_ERR_INVALID_ARG, "ctx is NULL");
    if (plp_status s = ess_check(a)) return s;
    if (a->P == 0 || a->n_cap == 0) return PLP_OK;
    return device_call(c, hip_stream, ess_args(a), ess_plan<DeviceRooms>, launch_essential_ransac);
}

plp_status plp_essential_ransac_host(plp_matcher* c, const plp_essential_ransac_args* a) {
    if (!c) return set_error(PLP_ERR_INVALID_ARG, "ctx is NULL");
    if (plp_status s = ess_check(a)) return s;
    if (a->P == 0 || a->n_cap == 0) return PLP_OK;
    return host_call(c, ess_args(a), ess_plan<Stage>, launch_essential_ransac);
}

// the host builds of essential.hpp (no HIP call)
int32_t plp_model_essential_ransac_host(const plp_essential_ransac_args* a) {
    if (ess_check(a) != PLP_OK) return -1;
    if (a->P == 0 || a->n_cap == 0) return a->P;
    const EssArgs A = ess_args(a);
    for (int p = 0; p < A.P; ++p) ess_model_problem(A, p);
    return A.P;
}

int32_t plp_model_essential_fit_host(const double* bearing_1, const double* bearing_2, const int32_t* offsets, int32_t n, double* out_E_21, int32_t* out_sweeps) {
    if (n < 0 || (n > 0 && (!offsets || !out_E_21))) return -1;
    for (int32_t i = 0; i < n; ++i)
        if (offsets[i + 1] < offsets[i] || offsets[i] < 0 || (offsets[i + 1] > offsets[i] && (!bearing_1 || !bearing_2))) return -1;
    EssScratch S;
    for (int32_t i = 0; i < n; ++i) {
        const int m = offsets[i + 1] - offsets[i];
        std::vector<double> fit((size_t)(m > 0 ? m : 1) * kEssPairDoubles);
        for (int k = 0; k < m; ++k)
            for (int c = 0; c < 3; ++c) {
                fit[(size_t)k * kEssPairDoubles + c] = bearing_1[3 * ((size_t)offsets[i] + k) + c];
                fit[(size_t)k * kEssPairDoubles + 3 + c] = bearing_2[3 * ((size_t)offsets[i] + k) + c];
            }
        int sw[2];
        ess_fit(fit.data(), kEssPairDoubles, m, S.M, S.G, S.V, S.null9, S.key, out_E_21 + 9 * (size_t)i, sw);
        if (out_sweeps) { out_sweeps[2 * (size_t)i] = sw[0]; out_sweeps[2 * (size_t)i + 1] = sw[1]; }
    }
    return n;
}

int32_t plp_model_essential_check_host(const double* bearing_1, const double* bearing_2, const int32_t* match, int32_t n_cap, int32_t m_cap, const double* E_21,
                                       int32_t n, float* out_score, int32_t* out_num_inliers, uint8_t* out_inliers) {
    if (n < 0 || n_cap < 0 || m_cap < 0 || (n_cap > 0 && (!bearing_1 || !match)) || (n > 0 && (!E_21 || !out_score || !out_num_inliers))) return -1;
    std::vector<int> slot_of;
    for (int s = 0; s < n_cap; ++s)
        if (match[s] >= 0 && match[s] < m_cap) slot_of.push_back(s);
    const int nm = (int)slot_of.size();
    if (nm > 0 && !bearing_2) return -1;
    std::vector<double> pairs((size_t)(nm > 0 ? nm : 1) * kEssPairDoubles);
    for (int k = 0; k < nm; ++k)
        for (int c = 0; c < 3; ++c) {
            pairs[(size_t)k * kEssPairDoubles + c] = bearing_1[3 * (size_t)slot_of[k] + c];
            pairs[(size_t)k * kEssPairDoubles + 3 + c] = bearing_2[3 * (size_t)match[slot_of[k]] + c];
        }
    std::vector<uint8_t> code((size_t)nm);
    for (int32_t i = 0; i < n; ++i) {
        out_score[i] = ess_model_check(E_21 + 9 * (size_t)i, pairs.data(), nm, code.data());
        int num = 0;
        for (int k = 0; k < nm; ++k) num += code[k] == 3 ? 1 : 0;
        out_num_inliers[i] = num;
        if (out_inliers) {
            for (int s = 0; s < n_cap; ++s) out_inliers[(size_t)i * n_cap + s] = 0;
            for (int k = 0; k < nm; ++k) out_inliers[(size_t)i * n_cap + slot_of[k]] = code[k] == 3 ? 1 : 0;
        }
    }
    return n;
}

int32_t plp_model_essential_draw_host(uint64_t seed, int32_t p, int32_t iter0, int32_t n_iters, int32_t num_matches, int32_t* out) {
    return ransac_draw_rows<kEssMinSet>(seed, p, iter0, n_iters, num_matches, out);
}

}  // extern "C"
