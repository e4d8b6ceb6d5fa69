// Host driver + C ABI of the matcher context: the covisibility graph: data::graph_node (include/plp_front.h: plp_covisibility_update_*,
// plp_covisibility_erase_*; covisibility_kernels.hip, covisibility.hpp)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "matcher_context.hpp"
#include "covisibility.hpp"

using namespace plp;

extern "C" {

namespace {
static bool cv_rises(const int32_t* off, int n, int end) {
    if (off[0] != 0 || off[n] != end) return false;
    for (int i = 0; i < n; ++i)
        if (off[i + 1] < off[i]) return false;
    return true;
}

// what both calls share: the sizes and the state tables
plp_status cv_check_state(int32_t F, int32_t conn_cap, int32_t covis_cap, const void* conn, const void* conn_w, const void* n_conn, const void* covis,
                          const void* covis_w, const void* n_covis) {
    if (F > kCvMaxKf) return set_error(PLP_ERR_UNSUPPORTED, "more than 8192 key frames: the weights of an owner are an LDS table");
    if (conn_cap > kCvMaxKf || covis_cap > kCvMaxKf) return set_error(PLP_ERR_UNSUPPORTED, "conn_cap and covis_cap above 8192");
    if (F > 0 && (!n_conn || !n_covis)) return set_error(PLP_ERR_INVALID_ARG, "kf_n_conn and kf_n_covis are required");
    if (F > 0 && conn_cap > 0 && (!conn || !conn_w)) return set_error(PLP_ERR_INVALID_ARG, "kf_conn and kf_conn_w are required");
    if (F > 0 && covis_cap > 0 && (!covis || !covis_w)) return set_error(PLP_ERR_INVALID_ARG, "kf_covis and kf_covis_w are required");
    return PLP_OK;
}

// host: the arrays are host memory, so the offsets and the owners are checked as well
plp_status cu_check(const plp_covisibility_update_args* a, bool host) {
    if (!a) return set_error(PLP_ERR_INVALID_ARG, "NULL argument");
    if (a->F < 0 || a->L < 0 || a->T < 0 || a->cap < 0 || a->G < 0 || a->conn_cap < 0 || a->covis_cap < 0)
        return set_error(PLP_ERR_INVALID_ARG, "F, L, T, cap, G, conn_cap and covis_cap must not be negative");
    if (a->cap > kCvMaxSlots) return set_error(PLP_ERR_UNSUPPORTED, "more than 8192 slots per row");
    if (a->G > kCvMaxKf) return set_error(PLP_ERR_UNSUPPORTED, "more than 8192 owners: they are distinct key frames");
    if (plp_status s = cv_check_state(a->F, a->conn_cap, a->covis_cap, a->kf_conn, a->kf_conn_w, a->kf_n_conn, a->kf_covis, a->kf_covis_w, a->kf_n_covis))
        return s;
    if (a->G == 0) return PLP_OK;
    if (!a->owners || !a->out_status) return set_error(PLP_ERR_INVALID_ARG, "owners and out_status are required");
    if (a->F > 0 && (!a->kf_id || !a->kf_parent || !a->kf_parent_unset)) return set_error(PLP_ERR_INVALID_ARG, "kf_id, kf_parent and kf_parent_unset are required");
    if (a->F > 0 && a->cap > 0 && !a->kf_lm) return set_error(PLP_ERR_INVALID_ARG, "kf_lm is required");
    if (!a->obs_offsets || (a->T > 0 && !a->obs_kf)) return set_error(PLP_ERR_INVALID_ARG, "obs_offsets and obs_kf are required");
    if (host) {
        if (!cv_rises(a->obs_offsets, a->L, a->T)) return set_error(PLP_ERR_INVALID_ARG, "obs_offsets must rise from 0 to T");
        std::vector<int32_t> o(a->owners, a->owners + a->G);
        std::sort(o.begin(), o.end());
        if (std::adjacent_find(o.begin(), o.end()) != o.end()) return set_error(PLP_ERR_INVALID_ARG, "an owner appears twice");
    }
    return PLP_OK;
}

CvArgs cu_args(const plp_covisibility_update_args* a) {
    CvArgs A{};
    A.F = a->F; A.L = a->L; A.T = a->T; A.cap = a->cap; A.G = a->G; A.conn_cap = a->conn_cap; A.covis_cap = a->covis_cap;
    A.kf_lm = a->kf_lm; A.kf_counts = a->kf_counts; A.obs_offsets = a->obs_offsets; A.obs_kf = a->obs_kf; A.lm_erased = a->lm_erased; A.kf_id = a->kf_id;
    A.kf_conn = a->kf_conn; A.kf_conn_w = a->kf_conn_w; A.kf_n_conn = a->kf_n_conn; A.kf_covis = a->kf_covis; A.kf_covis_w = a->kf_covis_w;
    A.kf_n_covis = a->kf_n_covis; A.kf_parent = a->kf_parent; A.kf_parent_unset = a->kf_parent_unset;
    A.owners = a->owners;
    A.out_status = a->out_status; A.out_nearest = a->out_nearest; A.out_max_weight = a->out_max_weight; A.out_touched = a->out_touched;
    return A;
}

// the state tables of either call
extern "C++" template <class R> void cv_state_plan(R& r, CvArgs& A) {
    const size_t F = (size_t)A.F;
    r.out(A.kf_conn, F * A.conn_cap); r.out(A.kf_conn_w, F * A.conn_cap); r.out(A.kf_n_conn, F);
    r.out(A.kf_covis, F * A.covis_cap); r.out(A.kf_covis_w, F * A.covis_cap); r.out(A.kf_n_covis, F);
}

// the arrays of the update; the room is what the launches hand to one another, one block of i32
extern "C++" template <class R> void cu_plan(R& r, plp_matcher* c, CvArgs& A) {
    const size_t F = (size_t)A.F, L = (size_t)A.L, T = (size_t)A.T, G = (size_t)A.G;
    r.in(A.kf_lm, F * A.cap); r.in(A.kf_counts, F); r.in(A.obs_offsets, L + 1); r.in(A.obs_kf, T); r.in(A.lm_erased, L); r.in(A.kf_id, F);
    cv_state_plan(r, A);
    r.out(A.kf_parent, F); r.out(A.kf_parent_unset, F);
    r.in(A.owners, G);
    r.out(A.out_status, G); r.out(A.out_nearest, G); r.out(A.out_max_weight, G); r.out(A.out_touched, F);
    r.room(c->covis_ws, A.pos_of, cv_scratch_words(A.F, A.G, A.conn_cap, A.covis_cap));
}

// the room's parts, once its device address is known, then the launches
static hipError_t cu_run(hipStream_t st, CvArgs& A) {
    cv_scratch_split(A);
    return launch_covisibility_update(st, A);
}

plp_status ce_check(const plp_covisibility_erase_args* a) {
    if (!a) return set_error(PLP_ERR_INVALID_ARG, "NULL argument");
    if (a->F < 0 || a->conn_cap < 0 || a->covis_cap < 0) return set_error(PLP_ERR_INVALID_ARG, "F, conn_cap and covis_cap must not be negative");
    if (plp_status s = cv_check_state(a->F, a->conn_cap, a->covis_cap, a->kf_conn, a->kf_conn_w, a->kf_n_conn, a->kf_covis, a->kf_covis_w, a->kf_n_covis))
        return s;
    if (a->F == 0) return PLP_OK;
    if (!a->erased || !a->out_status) return set_error(PLP_ERR_INVALID_ARG, "erased and out_status are required");
    return PLP_OK;
}

CvArgs ce_args(const plp_covisibility_erase_args* a) {
    CvArgs A{};
    A.F = a->F; A.conn_cap = a->conn_cap; A.covis_cap = a->covis_cap;
    A.kf_conn = a->kf_conn; A.kf_conn_w = a->kf_conn_w; A.kf_n_conn = a->kf_n_conn; A.kf_covis = a->kf_covis; A.kf_covis_w = a->kf_covis_w;
    A.kf_n_covis = a->kf_n_covis;
    A.erased = a->erased; A.out_status = a->out_status; A.out_touched = a->out_touched;
    return A;
}

extern "C++" template <class R> void ce_plan(R& r, plp_matcher*, CvArgs& A) {
    const size_t F = (size_t)A.F;
    cv_state_plan(r, A);
    r.in(A.erased, F);
    r.out(A.out_status, F); r.out(A.out_touched, F);
}
}  // namespace

plp_status plp_covisibility_update_device(plp_matcher* c, const plp_covisibility_update_args* a, void* hip_stream) {
    if (!c) return set_error(PLP_ERR_INVALID_ARG, "ctx is NULL");
    if (plp_status s = cu_check(a, false)) return s;
    if (a->G == 0) return PLP_OK;
    return device_call(c, hip_stream, cu_args(a), cu_plan<DeviceRooms>, cu_run);
}

plp_status plp_covisibility_update_host(plp_matcher* c, const plp_covisibility_update_args* a) {
    if (!c) return set_error(PLP_ERR_INVALID_ARG, "ctx is NULL");
    if (plp_status s = cu_check(a, true)) return s;
    if (a->G == 0) return PLP_OK;
    return host_call(c, cu_args(a), cu_plan<Stage>, cu_run);
}

// the host build of covisibility.hpp (no HIP call): every owner, then every key frame
int32_t plp_model_covisibility_update_host(const plp_covisibility_update_args* a) {
    if (plp_status s = cu_check(a, true)) return -(int32_t)s;
    CvArgs A = cu_args(a);
    std::vector<int32_t> ws(cv_scratch_words(A.F, A.G, A.conn_cap, A.covis_cap), -1);
    A.pos_of = ws.data();
    cv_scratch_split(A);
    std::vector<CvShared> shared(1);
    LmTeamHost par;
    for (int p = 0; p < A.G; ++p) cv_count(A, p, shared[0], par);
    if (A.G > 0)
        for (int j = 0; j < A.F; ++j) cv_apply(A, j, shared[0], par);
    return A.G;
}

plp_status plp_covisibility_erase_device(plp_matcher* c, const plp_covisibility_erase_args* a, void* hip_stream) {
    if (!c) return set_error(PLP_ERR_INVALID_ARG, "ctx is NULL");
    if (plp_status s = ce_check(a)) return s;
    if (a->F == 0) return PLP_OK;
    return device_call(c, hip_stream, ce_args(a), ce_plan<DeviceRooms>, launch_covisibility_erase);
}

plp_status plp_covisibility_erase_host(plp_matcher* c, const plp_covisibility_erase_args* a) {
    if (!c) return set_error(PLP_ERR_INVALID_ARG, "ctx is NULL");
    if (plp_status s = ce_check(a)) return s;
    if (a->F == 0) return PLP_OK;
    return host_call(c, ce_args(a), ce_plan<Stage>, launch_covisibility_erase);
}

int32_t plp_model_covisibility_erase_host(const plp_covisibility_erase_args* a) {
    if (plp_status s = ce_check(a)) return -(int32_t)s;
    CvArgs A = ce_args(a);
    std::vector<CvShared> shared(1);
    LmTeamHost par;
    for (A.phase = 0; A.phase < 2; ++A.phase)
        for (int j = 0; j < A.F; ++j) cv_erase(A, j, shared[0], par);
    return A.F;
}

}  // extern "C"
