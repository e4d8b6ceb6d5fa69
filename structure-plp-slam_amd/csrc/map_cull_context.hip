// Host driver + C ABI of the matcher context: map culling: module::local_map_cleaner (include/plp_front.h: plp_cull_keyframes_*,
// plp_cull_landmarks_*; map_cull_kernels.hip, map_cull.hpp)
#include <hip/hip_runtime.h>

#include <vector>

#include "matcher_context.hpp"
#include "map_cull.hpp"

using namespace plp;

extern "C" {

namespace {
bool rises(const int32_t* off, int n, int end) {
    if (off[0] != 0 || off[n] != end) return false;
    for (int i = 0; i < n; ++i)
        if (off[i + 1] < off[i]) return false;
    return true;
}

// host: the arrays are host memory, so the two offset tables are checked as well
plp_status ck_check(const plp_cull_keyframes_args* a, bool host) {
    if (!a) return set_error(PLP_ERR_INVALID_ARG, "NULL argument");
    if (a->F < 0 || a->L < 0 || a->T < 0 || a->cap < 0 || a->kp_stride < 0 || a->G < 0 || a->Cv < 0)
        return set_error(PLP_ERR_INVALID_ARG, "F, L, T, cap, kp_stride, G and Cv must not be negative");
    if (a->kp_stride && a->kp_stride < a->cap) return set_error(PLP_ERR_INVALID_ARG, "kp_stride must be 0 or at least cap");
    if (a->F > kCullMaxKf) return set_error(PLP_ERR_UNSUPPORTED, "more than 8192 key frames: the removed set is an LDS bitmap");
    if (a->cap > kCullMaxSlots) return set_error(PLP_ERR_UNSUPPORTED, "more than 8192 slots per row");
    if (a->G > kCullMaxProblems) return set_error(PLP_ERR_UNSUPPORTED, "more than 65535 problems");
    if (a->G == 0) return PLP_OK;
    const bool slots = a->F > 0 && a->cap > 0;
    if (!a->cur_kf || !a->covis_offsets || (a->Cv > 0 && !a->covis)) return set_error(PLP_ERR_INVALID_ARG, "cur_kf, covis_offsets and covis are required");
    if (a->F > 0 && !a->kf_id) return set_error(PLP_ERR_INVALID_ARG, "kf_id is required");
    if (slots && (!a->kf_lm || !a->undist)) return set_error(PLP_ERR_INVALID_ARG, "kf_lm and undist are required");
    if (!a->obs_offsets || (a->T > 0 && (!a->obs_kf || !a->obs_idx))) return set_error(PLP_ERR_INVALID_ARG, "obs_offsets, obs_kf and obs_idx are required");
    if (!a->is_monocular && ((slots && !a->depths) || (a->F > 0 && !a->depth_thr)))
        return set_error(PLP_ERR_INVALID_ARG, "depths and depth_thr are required unless is_monocular");
    if (!a->out_num_removed || (a->Cv > 0 && (!a->out_decision || !a->out_num_valid || !a->out_num_redundant)))
        return set_error(PLP_ERR_INVALID_ARG, "out_num_removed, out_decision, out_num_valid and out_num_redundant are required");
    if (host) {
        if (!rises(a->obs_offsets, a->L, a->T)) return set_error(PLP_ERR_INVALID_ARG, "obs_offsets must rise from 0 to T");
        if (!rises(a->covis_offsets, a->G, a->Cv)) return set_error(PLP_ERR_INVALID_ARG, "covis_offsets must rise from 0 to Cv");
    }
    return PLP_OK;
}

CullArgs ck_args(const plp_cull_keyframes_args* a) {
    CullArgs A{};
    A.F = a->F; A.L = a->L; A.T = a->T; A.cap = a->cap; A.kp_stride = a->kp_stride ? a->kp_stride : a->cap; A.G = a->G; A.Cv = a->Cv;
    A.mono = a->is_monocular != 0; A.origin_id = a->origin_id;
    A.kf_lm = a->kf_lm; A.kf_counts = a->kf_counts; A.undist = a->undist; A.x_right = a->x_right; A.depths = a->depths; A.depth_thr = a->depth_thr;
    A.kf_id = a->kf_id; A.kf_cannot_erase = a->kf_cannot_erase;
    A.obs_offsets = a->obs_offsets; A.obs_kf = a->obs_kf; A.obs_idx = a->obs_idx; A.lm_erased = a->lm_erased; A.lm_num_obs = a->lm_num_obs;
    A.cur_kf = a->cur_kf; A.covis_offsets = a->covis_offsets; A.covis = a->covis;
    A.out_num_removed = a->out_num_removed; A.out_decision = a->out_decision; A.out_num_valid = a->out_num_valid;
    A.out_num_redundant = a->out_num_redundant; A.out_kf_removed = a->out_kf_removed; A.out_lm_erased = a->out_lm_erased;
    A.words = (A.F + 31) / 32;
    return A;
}

// The arrays of the call.  The rooms are the snapshot counts of every entry and, when the dead landmarks are asked for, every problem's final
// removed set.  A room is asked for only where it is used: a context buffer of no element is still a pointer, and A.rem must stay NULL for the
// replay not to store the sets.
extern "C++" template <class R> void ck_plan(R& r, plp_matcher* c, CullArgs& A) {
    const size_t F = (size_t)A.F, L = (size_t)A.L, T = (size_t)A.T, G = (size_t)A.G, Cv = (size_t)A.Cv, K = F * A.kp_stride;
    r.in(A.kf_lm, F * A.cap); r.in(A.kf_counts, F); r.in(A.undist, K); r.in(A.x_right, K); r.in(A.depths, K); r.in(A.depth_thr, F);
    r.in(A.kf_id, F); r.in(A.kf_cannot_erase, F);
    r.in(A.obs_offsets, L + 1); r.in(A.obs_kf, T); r.in(A.obs_idx, T); r.in(A.lm_erased, L); r.in(A.lm_num_obs, L);
    r.in(A.cur_kf, G); r.in(A.covis_offsets, G + 1); r.in(A.covis, Cv);
    r.out(A.out_num_removed, G); r.out(A.out_decision, Cv); r.out(A.out_num_valid, Cv); r.out(A.out_num_redundant, Cv);
    r.out(A.out_kf_removed, G * F); r.out(A.out_lm_erased, G * L);
    if (A.Cv > 0) r.room(c->cull_cnt, A.cnt, Cv * 2);
    if (cull_mask_rows(A) > 0) r.room(c->cull_rem, A.rem, G * A.words);
}

plp_status cl_check(const plp_cull_landmarks_args* a, bool host) {
    if (!a) return set_error(PLP_ERR_INVALID_ARG, "NULL argument");
    if (a->R < 0 || a->N < 0 || a->L < 0) return set_error(PLP_ERR_INVALID_ARG, "R, N and L must not be negative");
    if (a->R == 0) return PLP_OK;
    if (!a->fresh_offsets || !a->cur_kf_id || !a->num_obs_thr || !a->out_num_removed || !a->out_num_fresh)
        return set_error(PLP_ERR_INVALID_ARG, "fresh_offsets, cur_kf_id, num_obs_thr, out_num_removed and out_num_fresh are required");
    if (a->N > 0 && (!a->fresh || !a->out_state || !a->out_fresh)) return set_error(PLP_ERR_INVALID_ARG, "fresh, out_state and out_fresh are required");
    if (a->L > 0 && (!a->num_observed || !a->num_observable || !a->first_kf_id || !a->num_obs))
        return set_error(PLP_ERR_INVALID_ARG, "num_observed, num_observable, first_kf_id and num_obs are required");
    if (host && !rises(a->fresh_offsets, a->R, a->N)) return set_error(PLP_ERR_INVALID_ARG, "fresh_offsets must rise from 0 to N");
    return PLP_OK;
}

CullLmArgs cl_args(const plp_cull_landmarks_args* a) {
    CullLmArgs A{};
    A.R = a->R; A.N = a->N; A.L = a->L;
    A.fresh_offsets = a->fresh_offsets; A.fresh = a->fresh; A.lm_erased = a->lm_erased; A.num_observed = a->num_observed;
    A.num_observable = a->num_observable; A.first_kf_id = a->first_kf_id; A.num_obs = a->num_obs; A.owning_plane = a->owning_plane;
    A.cur_kf_id = a->cur_kf_id; A.num_obs_thr = a->num_obs_thr;
    A.out_state = a->out_state; A.out_num_removed = a->out_num_removed; A.out_num_fresh = a->out_num_fresh; A.out_fresh = a->out_fresh;
    return A;
}

extern "C++" template <class R> void cl_plan(R& r, plp_matcher*, CullLmArgs& A) {
    const size_t R_ = (size_t)A.R, N = (size_t)A.N, L = (size_t)A.L;
    r.in(A.fresh_offsets, R_ + 1); r.in(A.fresh, N); r.in(A.lm_erased, L); r.in(A.num_observed, L); r.in(A.num_observable, L);
    r.in(A.first_kf_id, L); r.in(A.num_obs, L); r.in(A.owning_plane, L); r.in(A.cur_kf_id, R_); r.in(A.num_obs_thr, R_);
    r.out(A.out_state, N); r.out(A.out_num_removed, R_); r.out(A.out_num_fresh, R_); r.out(A.out_fresh, N);
}
}  // namespace

plp_status plp_cull_keyframes_device(plp_matcher* c, const plp_cull_keyframes_args* a, void* hip_stream) {
    if (!c) return set_error(PLP_ERR_INVALID_ARG, "ctx is NULL");
    if (plp_status s = ck_check(a, false)) return s;
    if (a->G == 0) return PLP_OK;
    return device_call(c, hip_stream, ck_args(a), ck_plan<DeviceRooms>, launch_cull_keyframes);
}

plp_status plp_cull_keyframes_host(plp_matcher* c, const plp_cull_keyframes_args* a) {
    if (!c) return set_error(PLP_ERR_INVALID_ARG, "ctx is NULL");
    if (plp_status s = ck_check(a, true)) return s;
    if (a->G == 0) return PLP_OK;
    return host_call(c, ck_args(a), ck_plan<Stage>, launch_cull_keyframes);
}

// the host build of map_cull.hpp (no HIP call): the replay alone, which counts every entry itself
int32_t plp_model_cull_keyframes_host(const plp_cull_keyframes_args* a) {
    if (plp_status s = ck_check(a, true)) return -(int32_t)s;
    CullArgs A = ck_args(a);
    std::vector<CullShared> shared(1);
    LmTeamHost par;
    const int rows = cull_mask_rows(A);
    for (int g = 0; g < A.G; ++g) {
        cull_replay(A, g, shared[0], par);
        for (int i = 0; i < rows; ++i) cull_masks(A, g, i, shared[0].rem);
    }
    return A.G;
}

plp_status plp_cull_landmarks_device(plp_matcher* c, const plp_cull_landmarks_args* a, void* hip_stream) {
    if (!c) return set_error(PLP_ERR_INVALID_ARG, "ctx is NULL");
    if (plp_status s = cl_check(a, false)) return s;
    if (a->R == 0) return PLP_OK;
    return device_call(c, hip_stream, cl_args(a), cl_plan<DeviceRooms>, launch_cull_landmarks);
}

plp_status plp_cull_landmarks_host(plp_matcher* c, const plp_cull_landmarks_args* a) {
    if (!c) return set_error(PLP_ERR_INVALID_ARG, "ctx is NULL");
    if (plp_status s = cl_check(a, true)) return s;
    if (a->R == 0) return PLP_OK;
    return host_call(c, cl_args(a), cl_plan<Stage>, launch_cull_landmarks);
}

int32_t plp_model_cull_landmarks_host(const plp_cull_landmarks_args* a) {
    if (plp_status s = cl_check(a, true)) return -(int32_t)s;
    const CullLmArgs A = cl_args(a);
    CullSharedLm sh{};
    LmTeamHost par;
    for (int r = 0; r < A.R; ++r) cull_states(A, r, sh, par);
    return A.R;
}

}  // extern "C"
