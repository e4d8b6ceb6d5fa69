// Host driver + C ABI of the matcher context: map initialisation of the perspective and fisheye cameras, the homography and the fundamental RANSAC and
// the choice between them (include/plp_front.h: plp_perspective_ransac_*; perspective_init_kernels.hip, perspective_init.hpp)
#include <hip/hip_runtime.h>

#include <vector>

#include "matcher_context.hpp"
#include "perspective_init.hpp"

using namespace plp;

extern "C" {

namespace {
plp_status persp_check(const plp_perspective_ransac_args* a) {
    if (!a) return set_error(PLP_ERR_INVALID_ARG, "NULL argument");
    if (a->P < 0 || a->n_cap < 0 || a->m_cap < 0) return set_error(PLP_ERR_INVALID_ARG, "P, n_cap and m_cap must not be negative");
    if (a->iters < 1) return set_error(PLP_ERR_INVALID_ARG, "iters must be positive");
    if ((a->given_H_21 != nullptr) != (a->given_H_num_inliers != nullptr))
        return set_error(PLP_ERR_INVALID_ARG, "given_H_21 and given_H_num_inliers go together");
    if (a->n_cap > kPerspMaxSlots) return set_error(PLP_ERR_UNSUPPORTED, "more than 8192 slots per problem");
    if (a->P > 65535) return set_error(PLP_ERR_UNSUPPORTED, "more than 65535 problems in one call");
    if (a->iters > kPerspMaxIters) return set_error(PLP_ERR_UNSUPPORTED, "more than 65536 iterations");
    if (a->P == 0 || a->n_cap == 0) return PLP_OK;
    if (!a->undist_1 || !a->match || (a->m_cap > 0 && !a->undist_2)) return set_error(PLP_ERR_INVALID_ARG, "undist_1, undist_2, match are required");
    if (!a->out_status_h || !a->out_status_f || !a->out_num_matches || !a->out_H_21 || !a->out_F_21 || !a->out_score_h || !a->out_score_f || !a->out_best_iter_h ||
        !a->out_best_iter_f || !a->out_num_inliers_h || !a->out_num_inliers_f || !a->out_rel_score_h || !a->out_choice || !a->out_inliers)
        return set_error(PLP_ERR_INVALID_ARG, "every output but out_inliers_h, out_inliers_f, out_hyp_score_h, out_hyp_score_f is required");
    return PLP_OK;
}

PerspArgs persp_args(const plp_perspective_ransac_args* a) {
    PerspArgs A{};
    A.P = a->P; A.n_cap = a->n_cap; A.m_cap = a->m_cap; A.iters = a->iters; A.recompute = a->recompute != 0; A.seed = a->seed;
    A.undist_1 = a->undist_1; A.undist_2 = a->undist_2; A.match = a->match; A.counts_1 = a->counts_1; A.counts_2 = a->counts_2;
    A.samples_h = a->samples_h; A.samples_f = a->samples_f; A.given_H_21 = a->given_H_21; A.given_H_num_inliers = a->given_H_num_inliers;
    A.out_status_h = a->out_status_h; A.out_status_f = a->out_status_f; A.out_num_matches = a->out_num_matches; A.out_H_21 = a->out_H_21; A.out_F_21 = a->out_F_21;
    A.out_score_h = a->out_score_h; A.out_score_f = a->out_score_f; A.out_best_iter_h = a->out_best_iter_h; A.out_best_iter_f = a->out_best_iter_f;
    A.out_num_inliers_h = a->out_num_inliers_h; A.out_num_inliers_f = a->out_num_inliers_f; A.out_rel_score_h = a->out_rel_score_h; A.out_choice = a->out_choice;
    A.out_inliers = a->out_inliers; A.out_inliers_h = a->out_inliers_h; A.out_inliers_f = a->out_inliers_f; A.out_hyp_score_h = a->out_hyp_score_h;
    A.out_hyp_score_f = a->out_hyp_score_f;
    return A;
}

// the arrays of the call; the rooms are what the launches hand to one another
extern "C++" template <class R> void persp_plan(R& r, plp_matcher* c, PerspArgs& A) {
    const size_t P = (size_t)A.P, M = (size_t)A.n_cap, M2 = (size_t)A.m_cap, I = (size_t)A.iters;
    r.in(A.undist_1, P * M); r.in(A.undist_2, P * M2); r.in(A.match, P * M); r.in(A.counts_1, P); r.in(A.counts_2, P); r.in(A.samples_h, P * I * 8);
    r.in(A.samples_f, P * I * 8); r.in(A.given_H_21, P * 9); r.in(A.given_H_num_inliers, P);
    r.out(A.out_status_h, P, false); r.out(A.out_status_f, P, false); r.out(A.out_num_matches, P, false); r.out(A.out_H_21, P * 9, false);
    r.out(A.out_F_21, P * 9, false); r.out(A.out_score_h, P, false); r.out(A.out_score_f, P, false); r.out(A.out_best_iter_h, P, false);
    r.out(A.out_best_iter_f, P, false); r.out(A.out_num_inliers_h, P, false); r.out(A.out_num_inliers_f, P, false); r.out(A.out_rel_score_h, P, false);
    r.out(A.out_choice, P, false); r.out(A.out_inliers, P * M); r.out(A.out_inliers_h, P * M); r.out(A.out_inliers_f, P * M);
    r.out(A.out_hyp_score_h, P * I, false); r.out(A.out_hyp_score_f, P * I, false);
    r.room(c->persp_ctx, A.ctx, P * kPerspCtxInts); r.room(c->persp_norm, A.ctx_norm, P * kPerspNormFloats); r.room(c->persp_T, A.ctx_T, P * kPerspTDoubles);
    r.room(c->persp_slot, A.ctx_slot, P * M); r.room(c->persp_hyp, A.ctx_hyp, P * 2 * kPerspHypDoubles * I);
    r.room(c->persp_pairs, A.ctx_pairs, P * 2 * M * kPerspPairDoubles); r.room(c->persp_M, A.ctx_M, P * 2 * 18); r.room(c->persp_code, A.ctx_code, P * 2 * M);
    r.room(c->persp_key, A.ctx_key, P * 2);
}

// solve::normalize of the host build: nrm (mean_x, mean_y, 1 / dev_x, 1 / dev_y), every sum in key-point order
void persp_model_normalize(const plp_keypoint* kp, int n, float* nrm) {
    float sx = 0, sy = 0;
    for (int i = 0; i < n; ++i) { sx += kp[i].x; sy += kp[i].y; }
    nrm[0] = persp_mean(sx, n); nrm[1] = persp_mean(sy, n);
    float dx = 0, dy = 0;
    for (int i = 0; i < n; ++i) { dx += persp_dev_term(kp[i].x, nrm[0]); dy += persp_dev_term(kp[i].y, nrm[1]); }
    nrm[2] = persp_inv_dev(persp_mean(dx, n)); nrm[3] = persp_inv_dev(persp_mean(dy, n));
}

// check_inliers of the host build over the matches held as four floats each: the score; code[k] as persp_residuals gives it
float persp_model_check(int solver, const double* M, const float* pts, int n, uint8_t* code) {
    float score = 0;
    for (int k = 0; k < n; ++k) {
        float ca, cb;
        const int c = persp_residuals(solver, M, pts[4 * k], pts[4 * k + 1], pts[4 * k + 2], pts[4 * k + 3], ca, cb);
        score = persp_score_add(score, c, ca, cb);
        code[k] = (uint8_t)c;
    }
    return score;
}

struct PerspSolved { bool valid; float score; int num, best_iter; double M[18]; std::vector<uint8_t> code; };

// one solver of one problem of the host build: the kernels' steps, one hypothesis and one match after the other.  pts: n x 4 as the key points hold
// them, npairs: n x 4 normalised and widened.
void persp_model_solver(const PerspArgs& A, int p, int solver, int n, const float* pts, const double* npairs, const double* T, PerspSolved& R) {
    R.valid = false; R.score = 0.0f; R.num = 0; R.best_iter = -1;
    for (double& v : R.M) v = 0.0;
    R.code.assign((size_t)n, 0);
    float* out_hyp = solver == kPerspH ? A.out_hyp_score_h : A.out_hyp_score_f;
    const bool enough = n >= kPerspMinSet;
    const bool given = solver == kPerspH && persp_given(A, p);
    PerspScratch S;
    if (given) {
        if (out_hyp)
            for (int it = 0; it < A.iters; ++it) out_hyp[(size_t)p * A.iters + it] = 0.0f;
        if (!enough) return;
        for (int i = 0; i < 9; ++i) R.M[i] = A.given_H_21[(size_t)9 * p + i];
        persp_inv3(R.M, R.M + 9);
        R.score = persp_model_check(solver, R.M, pts, n, R.code.data());                      // homography_solver.cc:398
        for (int k = 0; k < n; ++k) R.num += R.code[k] == 3 ? 1 : 0;
        R.valid = R.score > 0.0f && A.given_H_num_inliers[p] >= kPerspMinSet;                 // :401-402
        return;
    }
    std::vector<double> fit((size_t)(n > kPerspMinSet ? n : kPerspMinSet) * kPerspPairDoubles);
    std::vector<uint8_t> code((size_t)n, 0);
    double M[18];
    for (int it = 0; it < A.iters; ++it) {
        float score = 0;
        int idx[8];
        if (enough && persp_sample(A, solver, p, it, n, idx)) {
            for (int k = 0; k < 8; ++k)                             // :107-112
                for (int c = 0; c < kPerspPairDoubles; ++c) fit[(size_t)k * kPerspPairDoubles + c] = npairs[(size_t)idx[k] * kPerspPairDoubles + c];
            persp_fit(solver, fit.data(), kPerspMinSet, T, S, M, nullptr);                    // :115-116
            score = persp_model_check(solver, M, pts, n, code.data());                        // :119
            if (R.score < score) {                                  // :122
                R.score = score; R.best_iter = it; R.code = code;
                for (int i = 0; i < 18; ++i) R.M[i] = M[i];
            }
        }
        if (out_hyp) out_hyp[(size_t)p * A.iters + it] = persp_out(score);
    }
    if (!enough) return;
    for (int k = 0; k < n; ++k) R.num += R.code[k] == 3 ? 1 : 0;
    R.valid = R.score > 0.0f && R.num >= kPerspMinSet;              // :131
    if (R.valid && A.recompute) {                                   // :138-154
        int nc = 0;
        for (int k = 0; k < n; ++k)
            if (R.code[k] == 3) {
                for (int c = 0; c < kPerspPairDoubles; ++c) fit[(size_t)nc * kPerspPairDoubles + c] = npairs[(size_t)k * kPerspPairDoubles + c];
                ++nc;
            }
        persp_fit(solver, fit.data(), nc, T, S, R.M, nullptr);
        R.score = persp_model_check(solver, R.M, pts, n, R.code.data());
        R.num = 0;
        for (int k = 0; k < n; ++k) R.num += R.code[k] == 3 ? 1 : 0;
    }
}

void persp_model_problem(const PerspArgs& A, int p) {
    const int count_1 = clamp_count(A.counts_1, p, A.n_cap), count_2 = clamp_count(A.counts_2, p, A.m_cap);
    const size_t row = (size_t)p * A.n_cap, row2 = (size_t)p * A.m_cap;
    std::vector<int> slot_of;
    for (int s = 0; s < count_1; ++s)
        if (persp_matched(A, p, s, count_2)) slot_of.push_back(s);
    const int n = (int)slot_of.size();
    float nrm[kPerspNormFloats];
    persp_model_normalize(A.undist_1 + row, count_1, nrm);
    persp_model_normalize(count_2 > 0 ? A.undist_2 + row2 : nullptr, count_2, nrm + 4);
    double T[kPerspTDoubles], T2[9];
    persp_transform(nrm, T);
    persp_transform(nrm + 4, T2);
    persp_inv3(T2, T + 9);
    persp_transpose3(T2, T + 18);
    std::vector<float> pts((size_t)(n > 0 ? n : 1) * 4);
    std::vector<double> npairs((size_t)(n > 0 ? n : 1) * kPerspPairDoubles);
    for (int k = 0; k < n; ++k) {
        const plp_keypoint& k1 = A.undist_1[row + slot_of[k]];
        const plp_keypoint& k2 = A.undist_2[row2 + A.match[row + slot_of[k]]];
        pts[4 * (size_t)k] = k1.x; pts[4 * (size_t)k + 1] = k1.y; pts[4 * (size_t)k + 2] = k2.x; pts[4 * (size_t)k + 3] = k2.y;
        npairs[4 * (size_t)k] = (double)persp_normalized(k1.x, nrm[0], nrm[2]); npairs[4 * (size_t)k + 1] = (double)persp_normalized(k1.y, nrm[1], nrm[3]);
        npairs[4 * (size_t)k + 2] = (double)persp_normalized(k2.x, nrm[4], nrm[6]); npairs[4 * (size_t)k + 3] = (double)persp_normalized(k2.y, nrm[5], nrm[7]);
    }
    PerspSolved R[2];
    for (int s = 0; s < 2; ++s) persp_model_solver(A, p, s, n, pts.data(), npairs.data(), T, R[s]);
    const bool enough = n >= kPerspMinSet;
    for (int s = 0; s < 2; ++s) {
        const bool given = s == kPerspH && persp_given(A, p);
        (s == kPerspH ? A.out_status_h : A.out_status_f)[p] = !enough ? PLP_PERSPECTIVE_TOO_FEW_MATCHES : R[s].valid ? PLP_PERSPECTIVE_OK : PLP_PERSPECTIVE_INVALID;
        for (int i = 0; i < 9; ++i) (s == kPerspH ? A.out_H_21 : A.out_F_21)[(size_t)9 * p + i] = R[s].valid ? persp_out(R[s].M[i]) : 0.0;
        (s == kPerspH ? A.out_score_h : A.out_score_f)[p] = persp_out(R[s].score);
        (s == kPerspH ? A.out_num_inliers_h : A.out_num_inliers_f)[p] = R[s].valid ? R[s].num : 0;
        (s == kPerspH ? A.out_best_iter_h : A.out_best_iter_f)[p] = R[s].valid && !given ? R[s].best_iter : -1;
    }
    float rel;
    const int choice = persp_choice(R[0].score, R[1].score, R[0].valid, R[1].valid, rel);
    A.out_num_matches[p] = n;
    A.out_rel_score_h[p] = persp_out(rel);
    A.out_choice[p] = (uint8_t)choice;
    for (int o = 0; o < 3; ++o) {
        uint8_t* out = o == 0 ? A.out_inliers : o == 1 ? A.out_inliers_h : A.out_inliers_f;
        if (!out) continue;
        const int s = o == 0 ? (choice == PLP_PERSPECTIVE_CHOICE_F ? kPerspF : kPerspH) : o - 1;
        const bool on = o == 0 ? choice != PLP_PERSPECTIVE_CHOICE_NONE : R[s].valid;
        for (int q = 0; q < count_1; ++q) out[row + q] = 0;
        if (on)
            for (int k = 0; k < n; ++k) out[row + slot_of[k]] = R[s].code[k] == 3 ? 1 : 0;
    }
}

// the offsets of a fit entry are ascending and start at or above 0
bool persp_offsets_ok(const int32_t* offsets, int32_t n, const void* a, const void* b) {
    for (int32_t i = 0; i < n; ++i)
        if (offsets[i + 1] < offsets[i] || offsets[i] < 0 || (offsets[i + 1] > offsets[i] && (!a || !b))) return false;
    return true;
}

int32_t persp_model_fit(int solver, const float* pts_1, const float* pts_2, const int32_t* offsets, int32_t n, double* out, int32_t* out_sweeps) {
    if (n < 0 || (n > 0 && (!offsets || !out))) return -1;
    if (!persp_offsets_ok(offsets, n, pts_1, pts_2)) return -1;
    const double T[kPerspTDoubles] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 1, 0, 0, 0, 1, 0, 0, 0, 1, 1, 0, 0, 0, 1, 0, 0, 0, 1};   // no de-normalisation
    PerspScratch S;
    for (int32_t i = 0; i < n; ++i) {
        const int m = offsets[i + 1] - offsets[i];
        std::vector<double> fit((size_t)(m > 0 ? m : 1) * kPerspPairDoubles);
        for (int k = 0; k < m; ++k) {
            const size_t r = (size_t)offsets[i] + k;
            fit[4 * (size_t)k] = (double)pts_1[2 * r]; fit[4 * (size_t)k + 1] = (double)pts_1[2 * r + 1];
            fit[4 * (size_t)k + 2] = (double)pts_2[2 * r]; fit[4 * (size_t)k + 3] = (double)pts_2[2 * r + 1];
        }
        double M[18];
        int sw;
        persp_fit(solver, fit.data(), m, T, S, M, &sw);
        for (int e = 0; e < 9; ++e) out[9 * (size_t)i + e] = M[e];
        if (out_sweeps) out_sweeps[i] = sw;
    }
    return n;
}

int32_t persp_model_check_entry(int solver, const plp_keypoint* undist_1, const plp_keypoint* undist_2, const int32_t* match, int32_t n_cap, int32_t m_cap,
                                const double* Ms, int32_t n, float* out_score, int32_t* out_num_inliers, uint8_t* out_inliers) {
    if (n < 0 || n_cap < 0 || m_cap < 0 || (n_cap > 0 && (!undist_1 || !match)) || (n > 0 && (!Ms || !out_score || !out_num_inliers))) return -1;
    std::vector<int> slot_of;
    for (int s = 0; s < n_cap; ++s)
        if (match[s] >= 0 && match[s] < m_cap) slot_of.push_back(s);
    const int nm = (int)slot_of.size();
    if (nm > 0 && !undist_2) return -1;
    std::vector<float> pts((size_t)(nm > 0 ? nm : 1) * 4);
    for (int k = 0; k < nm; ++k) {
        const plp_keypoint& k1 = undist_1[slot_of[k]];
        const plp_keypoint& k2 = undist_2[match[slot_of[k]]];
        pts[4 * (size_t)k] = k1.x; pts[4 * (size_t)k + 1] = k1.y; pts[4 * (size_t)k + 2] = k2.x; pts[4 * (size_t)k + 3] = k2.y;
    }
    std::vector<uint8_t> code((size_t)nm);
    for (int32_t i = 0; i < n; ++i) {
        double M[18];
        for (int e = 0; e < 9; ++e) { M[e] = Ms[9 * (size_t)i + e]; M[9 + e] = 0.0; }
        if (solver == kPerspH) persp_inv3(M, M + 9);
        out_score[i] = persp_model_check(solver, M, pts.data(), nm, code.data());
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
}  // namespace

plp_status plp_perspective_ransac_device(plp_matcher* c, const plp_perspective_ransac_args* a, void* hip_stream) {
    if (!c) return set_error(PLP_ERR_INVALID_ARG, "ctx is NULL");
    if (plp_status s = persp_check(a)) return s;
    if (a->P == 0 || a->n_cap == 0) return PLP_OK;
    return device_call(c, hip_stream, persp_args(a), persp_plan<DeviceRooms>, launch_perspective_ransac);
}

plp_status plp_perspective_ransac_host(plp_matcher* c, const plp_perspective_ransac_args* a) {
    if (!c) return set_error(PLP_ERR_INVALID_ARG, "ctx is NULL");
    if (plp_status s = persp_check(a)) return s;
    if (a->P == 0 || a->n_cap == 0) return PLP_OK;
    return host_call(c, persp_args(a), persp_plan<Stage>, launch_perspective_ransac);
}

// the host builds of perspective_init.hpp (no HIP call)
int32_t plp_model_perspective_ransac_host(const plp_perspective_ransac_args* a) {
    if (persp_check(a) != PLP_OK) return -1;
    if (a->P == 0 || a->n_cap == 0) return a->P;
    const PerspArgs A = persp_args(a);
    for (int p = 0; p < A.P; ++p) persp_model_problem(A, p);
    return A.P;
}

int32_t plp_model_normalize_keypoints_host(const plp_keypoint* keypts, int32_t n, float* out_normalized, float* out_stats, double* out_transform) {
    if (n < 0 || (n > 0 && !keypts) || !out_stats || !out_transform) return -1;
    persp_model_normalize(keypts, n, out_stats);
    persp_transform(out_stats, out_transform);
    if (out_normalized)
        for (int32_t i = 0; i < n; ++i) {
            out_normalized[2 * (size_t)i] = persp_normalized(keypts[i].x, out_stats[0], out_stats[2]);
            out_normalized[2 * (size_t)i + 1] = persp_normalized(keypts[i].y, out_stats[1], out_stats[3]);
        }
    return n;
}

int32_t plp_model_homography_fit_host(const float* pts_1, const float* pts_2, const int32_t* offsets, int32_t n, double* out_H_21, int32_t* out_sweeps) {
    return persp_model_fit(kPerspH, pts_1, pts_2, offsets, n, out_H_21, out_sweeps);
}
int32_t plp_model_fundamental_fit_host(const float* pts_1, const float* pts_2, const int32_t* offsets, int32_t n, double* out_F_21, int32_t* out_sweeps) {
    return persp_model_fit(kPerspF, pts_1, pts_2, offsets, n, out_F_21, out_sweeps);
}
int32_t plp_model_homography_check_host(const plp_keypoint* undist_1, const plp_keypoint* undist_2, const int32_t* match, int32_t n_cap, int32_t m_cap,
                                        const double* H_21, int32_t n, float* out_score, int32_t* out_num_inliers, uint8_t* out_inliers) {
    return persp_model_check_entry(kPerspH, undist_1, undist_2, match, n_cap, m_cap, H_21, n, out_score, out_num_inliers, out_inliers);
}
int32_t plp_model_fundamental_check_host(const plp_keypoint* undist_1, const plp_keypoint* undist_2, const int32_t* match, int32_t n_cap, int32_t m_cap,
                                         const double* F_21, int32_t n, float* out_score, int32_t* out_num_inliers, uint8_t* out_inliers) {
    return persp_model_check_entry(kPerspF, undist_1, undist_2, match, n_cap, m_cap, F_21, n, out_score, out_num_inliers, out_inliers);
}
int32_t plp_model_perspective_draw_host(int32_t solver, uint64_t seed, int32_t p, int32_t iter0, int32_t n_iters, int32_t num_matches, int32_t* out) {
    if (solver != kPerspH && solver != kPerspF) return -1;
    return ransac_draw_rows<kPerspMinSet>(seed, p + solver * kPerspStreamOfF, iter0, n_iters, num_matches, out);
}

}  // extern "C"
