// Host driver + C ABI of the matcher context: loop candidates: solve::sim3_solver (include/plp_front.h: plp_sim3_ransac_*; sim3_kernels.hip, sim3.hpp)
#include <hip/hip_runtime.h>

#include <vector>

#include "matcher_context.hpp"
#include "sim3.hpp"

using namespace plp;

extern "C" {

namespace {
plp_status sim3_check(const plp_sim3_ransac_args* a) {
    if (!a) return set_error(PLP_ERR_INVALID_ARG, "NULL argument");
    if (plp_status s = check_camera_model(&a->camera, false)) return s;
    if (a->P < 0 || a->n_cap < 0) return set_error(PLP_ERR_INVALID_ARG, "P and n_cap must not be negative");
    if (a->iters < 1 || a->min_num_inliers < 0) return set_error(PLP_ERR_INVALID_ARG, "iters must be positive, min_num_inliers non-negative");
    if (a->num_levels < 1 || a->num_levels > 16 || !a->level_sigma_sq_1 || !a->level_sigma_sq_2)
        return set_error(PLP_ERR_INVALID_ARG, "num_levels must be 1 .. 16, level_sigma_sq_1 and level_sigma_sq_2 are required");
    if (a->n_cap > kSim3MaxSlots) return set_error(PLP_ERR_UNSUPPORTED, "more than 8192 slots per problem");
    if (a->P > 65535) return set_error(PLP_ERR_UNSUPPORTED, "more than 65535 problems in one call");
    if (a->P == 0 || a->n_cap == 0) return PLP_OK;
    if (!a->valid || !a->pos_w_1 || !a->pos_w_2 || !a->octave_1 || !a->octave_2 || !a->pose_1 || !a->pose_2)
        return set_error(PLP_ERR_INVALID_ARG, "valid, pos_w_1, pos_w_2, octave_1, octave_2, pose_1, pose_2 are required");
    if (!a->out_status || !a->out_num_common || !a->out_rot_12 || !a->out_trans_12 || !a->out_scale_12 || !a->out_num_inliers || !a->out_best_iter)
        return set_error(PLP_ERR_INVALID_ARG, "out_status, out_num_common, out_rot_12, out_trans_12, out_scale_12, out_num_inliers, out_best_iter are required");
    return PLP_OK;
}

Sim3Args sim3_args(const plp_sim3_ransac_args* a) {
    Sim3Args A{};
    set_camera(A, a->camera);
    A.P = a->P; A.n_cap = a->n_cap; A.iters = a->iters; A.fix_scale = a->fix_scale != 0; A.min_num_inliers = a->min_num_inliers;
    A.num_levels = a->num_levels; A.seed = a->seed;
    fill_levels(A.level_sigma_sq_1, a->level_sigma_sq_1, a->num_levels);
    fill_levels(A.level_sigma_sq_2, a->level_sigma_sq_2, a->num_levels);
    A.valid = a->valid; A.pos_w_1 = a->pos_w_1; A.pos_w_2 = a->pos_w_2; A.octave_1 = a->octave_1; A.octave_2 = a->octave_2; A.counts = a->counts;
    A.pose_1 = a->pose_1; A.pose_2 = a->pose_2; A.samples = a->samples;
    A.out_status = a->out_status; A.out_num_common = a->out_num_common; A.out_rot_12 = a->out_rot_12; A.out_trans_12 = a->out_trans_12;
    A.out_scale_12 = a->out_scale_12; A.out_num_inliers = a->out_num_inliers; A.out_best_iter = a->out_best_iter; A.out_inliers = a->out_inliers;
    A.out_hyp_inliers = a->out_hyp_inliers;
    return A;
}

// the arrays of the call; the rooms are what the launches hand to one another
extern "C++" template <class R> void sim3_plan(R& r, plp_matcher* c, Sim3Args& A) {
    const size_t P = (size_t)A.P, M = (size_t)A.n_cap, I = (size_t)A.iters;
    r.in(A.valid, P * M); r.in(A.pos_w_1, P * M * 3); r.in(A.pos_w_2, P * M * 3); r.in(A.octave_1, P * M); r.in(A.octave_2, P * M); r.in(A.counts, P);
    r.in(A.pose_1, P * 15); r.in(A.pose_2, P * 15); r.in(A.samples, P * I * 3);
    r.out(A.out_status, P, false); r.out(A.out_num_common, P, false); r.out(A.out_rot_12, P * 9, false); r.out(A.out_trans_12, P * 3, false);
    r.out(A.out_scale_12, P, false); r.out(A.out_num_inliers, P, false); r.out(A.out_best_iter, P, false); r.out(A.out_inliers, P * M);
    r.out(A.out_hyp_inliers, P * I, false);
    r.room(c->sim3_ctx, A.ctx, P * kSim3CtxInts); r.room(c->sim3_hyp, A.ctx_hyp, P * kSim3HypDoubles * I);
}

// one problem of the host build: the kernel's steps, one hypothesis and one point after the other
extern "C++" template <int MODEL> void sim3_model_problem(const Sim3Args& A, int p) {
    const int count = clamp_count(A.counts, p, A.n_cap);
    const size_t row = (size_t)p * A.n_cap;
    const double* P1 = A.pose_1 + (size_t)15 * p;
    const double* P2 = A.pose_2 + (size_t)15 * p;
    std::vector<int> slot_of;
    for (int s = 0; s < count; ++s)
        if (A.valid[row + s]) slot_of.push_back(s);
    const int n = (int)slot_of.size();
    std::vector<Sim3Point> pts((size_t)n);
    for (int k = 0; k < n; ++k) pts[k] = sim3_point<MODEL>(A, P1, P2, A.level_sigma_sq_1, A.level_sigma_sq_2, p, slot_of[k]);
    int best_count = 0, best_iter = -1;
    Sim3Hyp best{};
    std::vector<uint8_t> best_flags((size_t)n, 0), flags((size_t)n, 0);
    const bool enough = !(n < 3 || n < A.min_num_inliers);          // :130
    for (int it = 0; it < A.iters; ++it) {
        int num = 0;
        if (enough) {
            int idx[3];
            if (ransac_sample<3>(A, p, it, n, idx)) {
                const int slot[3] = {slot_of[idx[0]], slot_of[idx[1]], slot_of[idx[2]]};
                Sim3Hyp H;
                sim3_hypothesis(A, P1, P2, p, slot, H);
                double m21[12], m12[12];
                sim3_pose_row(H.rot_21, H.trans_21, H.scale_21, m21);
                sim3_pose_row(H.rot_12, H.trans_12, H.scale_12, m12);
                for (int k = 0; k < n; ++k) {
                    const Sim3Point& q = pts[k];
                    flags[k] = sim3_inlier<MODEL>(A, m21, m12, q.x1, q.x2, q.u1, q.v1, q.u2, q.v2, q.thr_1, q.thr_2, q.never) ? 1 : 0;
                    num += flags[k];
                }
                if (best_count < num) { best_count = num; best_iter = it; best = H; best_flags = flags; }   // :168
            }
        }
        if (A.out_hyp_inliers) A.out_hyp_inliers[(size_t)p * A.iters + it] = num;
    }
    const bool ok = enough && !(best_count < A.min_num_inliers);    // :177
    A.out_status[p] = !enough ? PLP_SIM3_TOO_FEW_POINTS : ok ? PLP_SIM3_OK : PLP_SIM3_TOO_FEW_INLIERS;
    A.out_num_common[p] = n;
    A.out_num_inliers[p] = best_count;
    A.out_best_iter[p] = ok ? best_iter : -1;
    const bool have = ok && best_iter >= 0;
    for (int i = 0; i < 9; ++i) A.out_rot_12[(size_t)9 * p + i] = have ? best.rot_12[i] : 0.0;
    for (int i = 0; i < 3; ++i) A.out_trans_12[(size_t)3 * p + i] = have ? best.trans_12[i] : 0.0;
    A.out_scale_12[p] = have ? best.scale_12 : 0.0f;
    if (A.out_inliers) {
        for (int s = 0; s < count; ++s) A.out_inliers[row + s] = 0;
        if (have)
            for (int k = 0; k < n; ++k) A.out_inliers[row + slot_of[k]] = best_flags[k];
    }
}
}  // namespace

plp_status plp_sim3_ransac_device(plp_matcher* c, const plp_sim3_ransac_args* a, void* hip_stream) {
    if (!c) return set_error(PLP_ERR_INVALID_ARG, "ctx is NULL");
    if (plp_status s = sim3_check(a)) return s;
    if (a->P == 0 || a->n_cap == 0) return PLP_OK;
    return device_call(c, hip_stream, sim3_args(a), sim3_plan<DeviceRooms>, launch_sim3_ransac);
}

plp_status plp_sim3_ransac_host(plp_matcher* c, const plp_sim3_ransac_args* a) {
    if (!c) return set_error(PLP_ERR_INVALID_ARG, "ctx is NULL");
    if (plp_status s = sim3_check(a)) return s;
    if (a->P == 0 || a->n_cap == 0) return PLP_OK;
    return host_call(c, sim3_args(a), sim3_plan<Stage>, launch_sim3_ransac);
}

// the host builds of sim3.hpp (no HIP call)
int32_t plp_model_sim3_ransac_host(const plp_sim3_ransac_args* a) {
    if (sim3_check(a) != PLP_OK) return -1;
    if (a->P == 0 || a->n_cap == 0) return a->P;
    const Sim3Args A = sim3_args(a);
    for (int p = 0; p < A.P; ++p) {
        if (A.model == PLP_CAMERA_PERSPECTIVE) sim3_model_problem<PLP_CAMERA_PERSPECTIVE>(A, p);
        else if (A.model == PLP_CAMERA_FISHEYE) sim3_model_problem<PLP_CAMERA_FISHEYE>(A, p);
        else sim3_model_problem<PLP_CAMERA_EQUIRECTANGULAR>(A, p);
    }
    return A.P;
}

int32_t plp_model_horn_sim3_host(const double* pts_1, const double* pts_2, int32_t n, int32_t fix_scale, double* out_rot_12, double* out_trans_12,
                                 float* out_scale_12, double* out_rot_21, double* out_trans_21, float* out_scale_21, int32_t* out_sweeps) {
    if (n < 0 || (n > 0 && (!pts_1 || !pts_2 || !out_rot_12 || !out_trans_12 || !out_scale_12 || !out_rot_21 || !out_trans_21 || !out_scale_21))) return -1;
    for (int32_t i = 0; i < n; ++i) {
        Sim3Hyp H;
        horn_sim3(pts_1 + 9 * (size_t)i, pts_2 + 9 * (size_t)i, fix_scale != 0, H);
        for (int k = 0; k < 9; ++k) { out_rot_12[9 * (size_t)i + k] = H.rot_12[k]; out_rot_21[9 * (size_t)i + k] = H.rot_21[k]; }
        for (int k = 0; k < 3; ++k) { out_trans_12[3 * (size_t)i + k] = H.trans_12[k]; out_trans_21[3 * (size_t)i + k] = H.trans_21[k]; }
        out_scale_12[i] = H.scale_12; out_scale_21[i] = H.scale_21;
        if (out_sweeps) out_sweeps[i] = H.sweeps;
    }
    return n;
}

int32_t plp_model_sim3_draw_host(uint64_t seed, int32_t p, int32_t iter0, int32_t n_iters, int32_t num_common, int32_t* out) {
    return ransac_draw_rows<3>(seed, p, iter0, n_iters, num_common, out);
}

int32_t plp_model_sym_eig4_max_host(const double* N, int32_t n, double* out_v, int32_t* out_sweeps) {
    if (n < 0 || (n > 0 && (!N || !out_v))) return -1;
    for (int32_t i = 0; i < n; ++i) {
        const int sweeps = sym_eig4_max(N + 16 * (size_t)i, out_v + 4 * (size_t)i);
        if (out_sweeps) out_sweeps[i] = sweeps;
    }
    return n;
}

}  // extern "C"
