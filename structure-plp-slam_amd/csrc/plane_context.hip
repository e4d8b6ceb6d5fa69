// Host driver + C ABI of the matcher context: plane fitting: Planar_Mapping_module's RANSAC and refine_points (include/plp_front.h:
// plp_plane_ransac_*, plp_plane_refine_points_*; plane_kernels.hip, plane_fit.hpp)
#include <hip/hip_runtime.h>

#include <vector>

#include "matcher_context.hpp"
#include "plane_fit.hpp"

using namespace plp;

extern "C" {

namespace {
plp_status plane_check(const plp_plane_ransac_args* a) {
    if (!a) return set_error(PLP_ERR_INVALID_ARG, "NULL argument");
    if (a->mode != PLP_PLANE_CREATE && a->mode != PLP_PLANE_UPDATE) return set_error(PLP_ERR_INVALID_ARG, "mode must be PLP_PLANE_CREATE or PLP_PLANE_UPDATE");
    if (a->P < 0 || a->n_cap < 0) return set_error(PLP_ERR_INVALID_ARG, "P and n_cap must not be negative");
    if (a->iters < 1 || a->points_per_ransac < 1 || a->min_points_before_ransac < 0)
        return set_error(PLP_ERR_INVALID_ARG, "iters and points_per_ransac must be positive, min_points_before_ransac non-negative");
    if (a->n_cap > kPlaneMaxSlots) return set_error(PLP_ERR_UNSUPPORTED, "more than 8192 slots per problem");
    if (a->P > 65535) return set_error(PLP_ERR_UNSUPPORTED, "more than 65535 problems in one call");
    if (a->iters > kPlaneMaxIters) return set_error(PLP_ERR_UNSUPPORTED, "more than 1024 iterations");
    if (a->samples && a->m_cap < plane_sample_size(a->mode, a->n_cap, a->points_per_ransac))
        return set_error(PLP_ERR_INVALID_ARG, "m_cap is below the sample size of a problem of n_cap slots");
    if (a->P == 0 || a->n_cap == 0) return PLP_OK;
    if (!a->pos_w || !a->flags || !a->dist_thresh || !a->error_thresh) return set_error(PLP_ERR_INVALID_ARG, "pos_w, flags, dist_thresh, error_thresh are required");
    if (a->mode == PLP_PLANE_UPDATE && (!a->best_error_in || !a->equation_in))
        return set_error(PLP_ERR_INVALID_ARG, "best_error_in and equation_in are required for PLP_PLANE_UPDATE");
    if (!a->out_status || !a->out_flags || !a->out_equation || !a->out_best_error || !a->out_best_iter || !a->out_last_iter || !a->out_num_inliers || !a->out_inliers)
        return set_error(PLP_ERR_INVALID_ARG, "out_status, out_flags, out_equation, out_best_error, out_best_iter, out_last_iter, out_num_inliers, out_inliers are required");
    return PLP_OK;
}

PlaneArgs plane_args(const plp_plane_ransac_args* a) {
    PlaneArgs A{};
    A.mode = a->mode; A.P = a->P; A.n_cap = a->n_cap; A.iters = a->iters; A.points_per_ransac = a->points_per_ransac;
    A.min_points_before_ransac = a->min_points_before_ransac; A.m_cap = a->m_cap; A.inliers_ratio_thr = a->inliers_ratio_thr; A.seed = a->seed;
    A.counts = a->counts; A.pos_w = a->pos_w; A.flags = a->flags; A.dist_thresh = a->dist_thresh; A.error_thresh = a->error_thresh;
    A.best_error_in = a->best_error_in; A.equation_in = a->equation_in; A.samples = a->samples;
    A.out_status = a->out_status; A.out_flags = a->out_flags; A.out_equation = a->out_equation; A.out_best_error = a->out_best_error;
    A.out_best_iter = a->out_best_iter; A.out_last_iter = a->out_last_iter; A.out_num_inliers = a->out_num_inliers; A.out_inliers = a->out_inliers;
    A.out_hyp_residual = a->out_hyp_residual; A.out_hyp_inliers = a->out_hyp_inliers; A.out_hyp_error = a->out_hyp_error;
    return A;
}

// the arrays of the call; the room is what the launches hand to one another
extern "C++" template <class R> void plane_plan(R& r, plp_matcher* c, PlaneArgs& A) {
    const size_t P = (size_t)A.P, M = (size_t)A.n_cap, I = (size_t)A.iters;
    r.in(A.counts, P); r.in(A.pos_w, P * M * 3); r.in(A.flags, P * M); r.in(A.dist_thresh, P); r.in(A.error_thresh, P); r.in(A.best_error_in, P);
    r.in(A.equation_in, P * 4); r.in(A.samples, P * I * (size_t)(A.m_cap > 0 ? A.m_cap : 0));
    r.out(A.out_status, P, false); r.out(A.out_flags, P, false); r.out(A.out_equation, P * 4); r.out(A.out_best_error, P);
    r.out(A.out_best_iter, P, false); r.out(A.out_last_iter, P, false); r.out(A.out_num_inliers, P, false); r.out(A.out_inliers, P * M);
    r.out(A.out_hyp_residual, P * I, false); r.out(A.out_hyp_inliers, P * I, false); r.out(A.out_hyp_error, P * I, false);
    r.room(c->plane_hyp, A.ctx_hyp, P * I * kPlaneHypDoubles);
}

// one problem of the host build: the kernels' steps, one hypothesis and one point after the other
void plane_model_problem(const PlaneArgs& A, int p) {
    const int n = clamp_count(A.counts, p, A.n_cap), I = A.iters;
    const size_t row = (size_t)p * A.n_cap;
    const double* pos = A.pos_w + 3 * row;
    std::vector<int> elig, live;
    for (int s = 0; s < n; ++s) {
        if (plane_eligible(A.mode, A.flags[row + s])) elig.push_back(s);
        if (plane_live(A.flags[row + s])) live.push_back(s);
    }
    const int n_elig = (int)elig.size();
    int flags = 0;
    const int early = plane_early_status(A, n, n_elig, flags);
    if (early != PLP_PLANE_OK) {
        A.out_status[p] = (uint8_t)early; A.out_flags[p] = (uint8_t)flags;
        if (A.mode == PLP_PLANE_UPDATE) {
            for (int i = 0; i < 4; ++i) A.out_equation[4 * (size_t)p + i] = A.equation_in[4 * (size_t)p + i];
            A.out_best_error[p] = A.best_error_in[p];
        }
        A.out_best_iter[p] = -1; A.out_last_iter[p] = -1; A.out_num_inliers[p] = 0;
        for (int s = 0; s < n; ++s) A.out_inliers[row + s] = 0;
        for (int it = 0; it < I; ++it) {
            if (A.out_hyp_residual) A.out_hyp_residual[(size_t)p * I + it] = 0.0;
            if (A.out_hyp_inliers) A.out_hyp_inliers[(size_t)p * I + it] = 0;
            if (A.out_hyp_error) A.out_hyp_error[(size_t)p * I + it] = kPlaneMax;
        }
        return;
    }
    const int m = plane_sample_size(A.mode, n, A.points_per_ransac);
    const double thr = A.dist_thresh[p];
    PlaneHostTeam T;
    std::vector<double> eq_s((size_t)4 * I), eq_r((size_t)4 * I, 0.0), res((size_t)I), err((size_t)I, kPlaneMax);
    std::vector<int> cnt((size_t)I, 0);
    std::vector<uint8_t> tried((size_t)I, 0);
    std::vector<int> list;
    for (int it = 0; it < I; ++it) {
        int sweeps;
        plane_fit(T, [&](int k, double x[3]) {
            const int rank = A.samples ? A.samples[((size_t)p * I + it) * A.m_cap + k] : ransac_draw_one(A.seed, p, it, k, n_elig);
            if ((unsigned)rank >= (unsigned)n_elig) return false;
            const double* w = pos + 3 * (size_t)elig[rank];
            x[0] = w[0]; x[1] = w[1]; x[2] = w[2];
            return true;
        }, m, &eq_s[4 * (size_t)it], res[it], sweeps);
        const double abs_n = plane_abs_n(&eq_s[4 * (size_t)it]);
        list.clear();
        for (int s : live)
            if (plane_distance(&eq_s[4 * (size_t)it], abs_n, pos + 3 * (size_t)s) < thr) list.push_back(s);
        cnt[it] = (int)list.size();
        tried[it] = plane_refit_gate(A, n, cnt[it]) ? 1 : 0;
        if (tried[it])
            plane_fit(T, [&](int k, double x[3]) {
                const double* w = pos + 3 * (size_t)list[k];
                x[0] = w[0]; x[1] = w[1]; x[2] = w[2];
                return true;
            }, cnt[it], &eq_r[4 * (size_t)it], err[it], sweeps);
        if (A.out_hyp_residual) A.out_hyp_residual[(size_t)p * I + it] = res[it];
        if (A.out_hyp_inliers) A.out_hyp_inliers[(size_t)p * I + it] = cnt[it];
        if (A.out_hyp_error) A.out_hyp_error[(size_t)p * I + it] = err[it];
    }
    const PlaneReplay R = plane_replay(A.mode, I, A.mode == PLP_PLANE_UPDATE ? A.best_error_in[p] : 0.0, A.error_thresh[p],
                                       [&](int i) { return res[i]; }, [&](int i) { return tried[i] != 0; }, [&](int i) { return err[i]; });
    int status = plane_late_status(A.mode, R, A.error_thresh[p], flags);
    const double* eq = R.last_refit ? &eq_r[4 * (size_t)R.last_iter] : &eq_s[4 * (size_t)R.last_iter];
    int num = 0;
    for (int s = 0; s < n; ++s) A.out_inliers[row + s] = 0;
    if (status == PLP_PLANE_OK) {                                                          // step [4] (:564-579, :704-720)
        const double* eq_b = &eq_s[4 * (size_t)R.best_iter];
        const double abs_b = plane_abs_n(eq_b), abs_n = plane_abs_n(eq);
        for (int s : live)
            if (plane_distance(eq_b, abs_b, pos + 3 * (size_t)s) < thr && plane_distance(eq, abs_n, pos + 3 * (size_t)s) < thr) {
                A.out_inliers[row + s] = 1;
                ++num;
            }
        if (A.mode == PLP_PLANE_UPDATE && num < A.points_per_ransac) { status = PLP_PLANE_TOO_FEW_LEFT; flags = PLP_PLANE_FLAG_INVALID; }   // :722
    }
    A.out_status[p] = (uint8_t)status; A.out_flags[p] = (uint8_t)flags;
    for (int i = 0; i < 4; ++i) A.out_equation[4 * (size_t)p + i] = eq[i];
    A.out_best_error[p] = R.plane_error;
    A.out_best_iter[p] = R.best_iter; A.out_last_iter[p] = R.last_iter; A.out_num_inliers[p] = num;
}

plp_status refine_check(const plp_plane_refine_args* a) {
    if (!a) return set_error(PLP_ERR_INVALID_ARG, "NULL argument");
    if (a->M < 0 || a->NP < 0) return set_error(PLP_ERR_INVALID_ARG, "M and NP must not be negative");
    if (a->M == 0) return PLP_OK;
    if (!a->pos_w || !a->lm_plane || !a->flags || !a->dist_thresh || !a->out_changed)
        return set_error(PLP_ERR_INVALID_ARG, "pos_w, lm_plane, flags, dist_thresh, out_changed are required");
    if (a->NP > 0 && (!a->equation || !a->active)) return set_error(PLP_ERR_INVALID_ARG, "equation and active are required");
    return PLP_OK;
}

PlaneRefineArgs refine_args(const plp_plane_refine_args* a) {
    PlaneRefineArgs A{};
    A.M = a->M; A.NP = a->NP; A.pos_w = a->pos_w; A.lm_plane = a->lm_plane; A.flags = a->flags; A.equation = a->equation; A.active = a->active;
    A.dist_thresh = a->dist_thresh; A.out_changed = a->out_changed;
    return A;
}

extern "C++" template <class R> void refine_plan(R& r, plp_matcher*, PlaneRefineArgs& A) {
    const size_t M = (size_t)A.M, NP = (size_t)A.NP;
    r.out(A.pos_w, M * 3); r.in(A.lm_plane, M); r.in(A.flags, M); r.in(A.equation, NP * 4); r.in(A.active, NP); r.in(A.dist_thresh, 1);
    r.out(A.out_changed, M, false);
}
}  // namespace

plp_status plp_plane_ransac_device(plp_matcher* c, const plp_plane_ransac_args* a, void* hip_stream) {
    if (!c) return set_error(PLP_ERR_INVALID_ARG, "ctx is NULL");
    if (plp_status s = plane_check(a)) return s;
    if (a->P == 0 || a->n_cap == 0) return PLP_OK;
    return device_call(c, hip_stream, plane_args(a), plane_plan<DeviceRooms>, launch_plane_ransac);
}

plp_status plp_plane_ransac_host(plp_matcher* c, const plp_plane_ransac_args* a) {
    if (!c) return set_error(PLP_ERR_INVALID_ARG, "ctx is NULL");
    if (plp_status s = plane_check(a)) return s;
    if (a->P == 0 || a->n_cap == 0) return PLP_OK;
    return host_call(c, plane_args(a), plane_plan<Stage>, launch_plane_ransac);
}

plp_status plp_plane_refine_points_device(plp_matcher* c, const plp_plane_refine_args* a, void* hip_stream) {
    if (!c) return set_error(PLP_ERR_INVALID_ARG, "ctx is NULL");
    if (plp_status s = refine_check(a)) return s;
    if (a->M == 0) return PLP_OK;
    return device_call(c, hip_stream, refine_args(a), refine_plan<DeviceRooms>, launch_plane_refine_points);
}

plp_status plp_plane_refine_points_host(plp_matcher* c, const plp_plane_refine_args* a) {
    if (!c) return set_error(PLP_ERR_INVALID_ARG, "ctx is NULL");
    if (plp_status s = refine_check(a)) return s;
    if (a->M == 0) return PLP_OK;
    return host_call(c, refine_args(a), refine_plan<Stage>, launch_plane_refine_points);
}

// the host builds of plane_fit.hpp (no HIP call)
int32_t plp_model_plane_ransac_host(const plp_plane_ransac_args* a) {
    if (plane_check(a) != PLP_OK) return -1;
    if (a->P == 0 || a->n_cap == 0) return a->P;
    const PlaneArgs A = plane_args(a);
    for (int p = 0; p < A.P; ++p) plane_model_problem(A, p);
    return A.P;
}

int32_t plp_model_plane_fit_host(const double* pos_w, int32_t n_points, const int32_t* indices, const int32_t* offsets, int32_t n,
                                 double* out_equation, double* out_residual, int32_t* out_sweeps) {
    if (n < 0 || n_points < 0 || (n > 0 && (!offsets || !out_equation || !out_residual))) return -1;
    PlaneHostTeam T;
    for (int32_t l = 0; l < n; ++l) {
        const int32_t b = offsets[l], m = offsets[l + 1] - b;
        if (m < 0 || (m > 0 && (!indices || !pos_w))) return -1;
        int sweeps = 0;
        double* eq = out_equation + 4 * (size_t)l;
        if (m == 0) {
            eq[0] = eq[1] = eq[2] = eq[3] = 0.0;
            out_residual[l] = kPlaneMax;
        } else {
            plane_fit(T, [&](int k, double x[3]) {
                const int32_t i = indices[b + k];
                if ((uint32_t)i >= (uint32_t)n_points) return false;
                x[0] = pos_w[3 * (size_t)i]; x[1] = pos_w[3 * (size_t)i + 1]; x[2] = pos_w[3 * (size_t)i + 2];
                return true;
            }, m, eq, out_residual[l], sweeps);
        }
        if (out_sweeps) out_sweeps[l] = sweeps;
    }
    return n;
}

int32_t plp_model_plane_draw_host(uint64_t seed, int32_t p, int32_t iter0, int32_t n_iters, int32_t m, int32_t n_eligible, int32_t* out) {
    if (n_iters < 0 || m < 0 || n_eligible < 1 || ((size_t)n_iters * (size_t)m > 0 && !out)) return -1;
    for (int32_t i = 0; i < n_iters; ++i)
        for (int32_t k = 0; k < m; ++k) out[(size_t)i * m + k] = ransac_draw_one(seed, p, iter0 + i, k, n_eligible);
    return n_iters;
}

int32_t plp_model_plane_refine_points_host(const plp_plane_refine_args* a) {
    if (refine_check(a) != PLP_OK) return -1;
    const PlaneRefineArgs A = refine_args(a);
    for (int i = 0; i < A.M; ++i) plane_refine_landmark(A, i);
    return A.M;
}

}  // extern "C"
