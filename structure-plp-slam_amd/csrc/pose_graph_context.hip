// Host driver + C ABI of the matcher context: loop closing: optimize::graph_optimizer (include/plp_front.h: plp_pose_graph_optimize_*, plp_correct_landmarks_*; pose_graph_kernels.hip, pose_graph.hpp)
#include <hip/hip_runtime.h>

#include <vector>

#include "matcher_context.hpp"
#include "pose_graph.hpp"

using namespace plp;

extern "C" {

namespace {
// host: the arrays are host memory, so the offset lists are checked as well
plp_status pg_check(const plp_pose_graph_args* a, bool host) {
    if (!a) return set_error(PLP_ERR_INVALID_ARG, "NULL argument");
    if (a->G < 0 || a->F < 0 || a->conn_cap < 0 || a->covis_cap < 0 || a->max_iter < 0) return set_error(PLP_ERR_INVALID_ARG, "G, F, conn_cap, covis_cap and max_iter must not be negative");
    if (a->pose_stride < 12) return set_error(PLP_ERR_INVALID_ARG, "pose_stride must be at least 12");
    if (a->edge_cap < 1 || a->env_cap < 1) return set_error(PLP_ERR_INVALID_ARG, "edge_cap and env_cap must be positive");
    if (a->G > kPgMaxProblems) return set_error(PLP_ERR_UNSUPPORTED, "more than 16 problems");
    if (a->F > kPgMaxKf) return set_error(PLP_ERR_UNSUPPORTED, "more than 1024 key frames in the table");
    if (a->edge_cap > kPgMaxEdges || a->env_cap > kPgMaxEnv) return set_error(PLP_ERR_UNSUPPORTED, "edge_cap above 16384 or env_cap above 65536");
    if (a->conn_cap > kPgMaxList || a->covis_cap > kPgMaxList) return set_error(PLP_ERR_UNSUPPORTED, "conn_cap or covis_cap above 65536");
    if (a->G == 0) return PLP_OK;
    if (!a->loop_kf || !a->curr_kf || !a->out_status) return set_error(PLP_ERR_INVALID_ARG, "loop_kf, curr_kf and out_status are required");
    if (a->F > 0 && (!a->pose || !a->kf_id || !a->kf_parent || !a->kf_n_conn || !a->kf_n_covis || (a->conn_cap > 0 && (!a->kf_conn || !a->kf_conn_w)) ||
                     (a->covis_cap > 0 && (!a->kf_covis || !a->kf_covis_w))))
        return set_error(PLP_ERR_INVALID_ARG, "pose, kf_id, kf_parent and the graph tables are required");
    if ((a->pre_offsets && (!a->pre_row || !a->pre_sim3)) || (a->non_offsets && (!a->non_row || !a->non_sim3)) || (a->lc_offsets && (!a->lc_owner || !a->lc_target)) ||
        (a->kf_loop_offsets && !a->kf_loop))
        return set_error(PLP_ERR_INVALID_ARG, "a list with offsets needs its arrays");
    if (host) {
        auto rises = [](const int32_t* o, int n) {
            if (!o) return true;
            if (o[0] != 0 || o[n] > kPgMaxList) return false;
            for (int i = 0; i < n; ++i) if (o[i + 1] < o[i]) return false;
            return true;
        };
        if (!rises(a->pre_offsets, a->G) || !rises(a->non_offsets, a->G) || !rises(a->lc_offsets, a->G) || !rises(a->kf_loop_offsets, a->F))
            return set_error(PLP_ERR_INVALID_ARG, "an offset list must rise from 0, to at most 65536");
    }
    return PLP_OK;
}

PgArgs pg_args(const plp_pose_graph_args* a) {
    PgArgs A{};
    A.G = a->G; A.F = a->F; A.pose_stride = a->pose_stride; A.conn_cap = a->conn_cap; A.covis_cap = a->covis_cap; A.edge_cap = a->edge_cap; A.env_cap = a->env_cap;
    A.max_iter = a->max_iter;
    A.pose = a->pose; A.kf_erased = a->kf_erased; A.kf_id = a->kf_id; A.kf_parent = a->kf_parent; A.kf_conn = a->kf_conn; A.kf_conn_w = a->kf_conn_w;
    A.kf_n_conn = a->kf_n_conn; A.kf_covis = a->kf_covis; A.kf_covis_w = a->kf_covis_w; A.kf_n_covis = a->kf_n_covis; A.kf_loop_offsets = a->kf_loop_offsets;
    A.kf_loop = a->kf_loop; A.loop_kf = a->loop_kf; A.curr_kf = a->curr_kf; A.fix_scale = a->fix_scale; A.pre_offsets = a->pre_offsets; A.pre_row = a->pre_row;
    A.pre_sim3 = a->pre_sim3; A.non_offsets = a->non_offsets; A.non_row = a->non_row; A.non_sim3 = a->non_sim3; A.lc_offsets = a->lc_offsets;
    A.lc_owner = a->lc_owner; A.lc_target = a->lc_target;
    A.out_status = a->out_status; A.out_num_edges = a->out_num_edges; A.out_edges = a->out_edges; A.out_sim3_cw = a->out_sim3_cw;
    A.out_corrected_wc = a->out_corrected_wc; A.out_pose = a->out_pose; A.out_info = a->out_info; A.out_chi2 = a->out_chi2;
    return A;
}

// the arrays of the call; the rooms are what the steps hand to one another
extern "C++" template <class R> void pg_plan(R& r, plp_matcher* c, PgArgs& A) {
    const size_t G = (size_t)A.G, F = (size_t)A.F;
    const size_t n_loop = list_end(r, A.kf_loop_offsets, A.F), n_pre = list_end(r, A.pre_offsets, A.G);
    const size_t n_non = list_end(r, A.non_offsets, A.G), n_lc = list_end(r, A.lc_offsets, A.G);
    r.in(A.pose, F * A.pose_stride); r.in(A.kf_erased, F); r.in(A.kf_id, F); r.in(A.kf_parent, F); r.in(A.kf_conn, F * A.conn_cap); r.in(A.kf_conn_w, F * A.conn_cap);
    r.in(A.kf_n_conn, F); r.in(A.kf_covis, F * A.covis_cap); r.in(A.kf_covis_w, F * A.covis_cap); r.in(A.kf_n_covis, F); r.in(A.kf_loop_offsets, F + 1);
    r.in(A.kf_loop, n_loop); r.in(A.loop_kf, G); r.in(A.curr_kf, G); r.in(A.fix_scale, G); r.in(A.pre_offsets, G + 1); r.in(A.pre_row, n_pre);
    r.in(A.pre_sim3, n_pre * 8); r.in(A.non_offsets, G + 1); r.in(A.non_row, n_non); r.in(A.non_sim3, n_non * 8); r.in(A.lc_offsets, G + 1); r.in(A.lc_owner, n_lc);
    r.in(A.lc_target, n_lc);
    r.out(A.out_status, G); r.out(A.out_num_edges, G); r.out(A.out_edges, G * A.edge_cap * 3); r.out(A.out_sim3_cw, G * F * 8); r.out(A.out_corrected_wc, G * F * 8);
    r.out(A.out_pose, G * F * 15); r.out(A.out_info, G * 4); r.out(A.out_chi2, G * 2);
    r.room(c->pg_d, A.ctx_d, G * pg_doubles(A.F, A.edge_cap, A.env_cap)); r.room(c->pg_i, A.ctx_i, G * pg_ints(A.F, A.edge_cap, A.env_cap));
}

// the host build of problem g with a state that holds one problem: ctx_base shifts the state's index, the inputs and outputs stay at g
void pg_model(const PgArgs& A, int g, bool edges_only) {
    PgArgs B = A;
    std::vector<double> d(pg_doubles(A.F, A.edge_cap, A.env_cap), 0.0);
    std::vector<int32_t> i(pg_ints(A.F, A.edge_cap, A.env_cap), 0);
    B.ctx_d = d.data(); B.ctx_i = i.data(); B.ctx_base = g;
    if (edges_only) { B.edges_only = 1; B.out_corrected_wc = nullptr; B.out_pose = nullptr; B.out_info = nullptr; B.out_chi2 = nullptr; }
    static thread_local PgShared sh;
    PgTeamHost par;
    pg_prepare(B, g, sh, par);
    if (!edges_only) pg_solve(B, g, sh, par);
    pg_finish(B, g, par);
}

plp_status pgl_check(const plp_correct_landmarks_args* a) {
    if (!a) return set_error(PLP_ERR_INVALID_ARG, "NULL argument");
    if (a->L < 0 || a->F < 0) return set_error(PLP_ERR_INVALID_ARG, "L and F must not be negative");
    if (a->F > kPgMaxKf) return set_error(PLP_ERR_UNSUPPORTED, "more than 1024 key frames in the table");
    if (a->L > 0 && (!a->pos_w || !a->ref_kf || !a->out_pos_w || !a->out_status || (a->F > 0 && (!a->sim3_cw || !a->corrected_wc))))
        return set_error(PLP_ERR_INVALID_ARG, "pos_w, ref_kf, sim3_cw, corrected_wc, out_pos_w and out_status are required");
    return PLP_OK;
}
PgLmArgs pgl_args(const plp_correct_landmarks_args* a) {
    PgLmArgs A{};
    A.L = a->L; A.F = a->F; A.pos_w = a->pos_w; A.lm_erased = a->lm_erased; A.ref_kf = a->ref_kf; A.kf_erased = a->kf_erased; A.sim3_cw = a->sim3_cw;
    A.corrected_wc = a->corrected_wc; A.out_pos_w = a->out_pos_w; A.out_status = a->out_status;
    return A;
}

extern "C++" template <class R> void pgl_plan(R& r, plp_matcher*, PgLmArgs& A) {
    const size_t L = (size_t)A.L, F = (size_t)A.F;
    r.in(A.pos_w, L * 3); r.in(A.lm_erased, L); r.in(A.ref_kf, L); r.in(A.kf_erased, F); r.in(A.sim3_cw, F * 8); r.in(A.corrected_wc, F * 8);
    r.out(A.out_pos_w, L * 3); r.out(A.out_status, L);
}
}  // namespace

plp_status plp_pose_graph_optimize_device(plp_matcher* c, const plp_pose_graph_args* a, void* hip_stream) {
    if (!c) return set_error(PLP_ERR_INVALID_ARG, "ctx is NULL");
    if (plp_status s = pg_check(a, false)) return s;
    if (a->G == 0) return PLP_OK;
    return device_call(c, hip_stream, pg_args(a), pg_plan<DeviceRooms>, launch_pose_graph);
}

plp_status plp_pose_graph_optimize_host(plp_matcher* c, const plp_pose_graph_args* a) {
    if (!c) return set_error(PLP_ERR_INVALID_ARG, "ctx is NULL");
    if (plp_status s = pg_check(a, true)) return s;
    if (a->G == 0) return PLP_OK;
    return host_call(c, pg_args(a), pg_plan<Stage>, launch_pose_graph);
}

// the host builds of pose_graph.hpp (no HIP call)
int32_t plp_model_pose_graph_optimize_host(const plp_pose_graph_args* a) {
    if (plp_status s = pg_check(a, true)) return -(int32_t)s;
    const PgArgs A = pg_args(a);
    for (int g = 0; g < A.G; ++g) pg_model(A, g, false);
    return A.G;
}

int32_t plp_model_pose_graph_edges_host(const plp_pose_graph_args* a) {
    if (plp_status s = pg_check(a, true)) return -(int32_t)s;
    const PgArgs A = pg_args(a);
    for (int g = 0; g < A.G; ++g) pg_model(A, g, true);
    return A.G;
}

int32_t plp_model_sim3_log_host(const double* sim3, int32_t n, double* out7) {
    if (n < 0 || (n > 0 && (!sim3 || !out7))) return -1;
    double c[kPgCoefs];
    pg_coef_init(c);
    for (int32_t i = 0; i < n; ++i) sim3_log(sim3 + 8 * (size_t)i, out7 + 7 * (size_t)i, c);
    return n;
}

int32_t plp_model_pose_log_host(const double* x, int32_t n, double* out) {
    if (n < 0 || (n > 0 && (!x || !out))) return -1;
    double c[kPgCoefs];
    pg_coef_init(c);
    for (int32_t i = 0; i < n; ++i) out[i] = pose_log(x[i], c);
    return n;
}

int32_t plp_model_pose_acos_host(const double* x, int32_t n, double* out) {
    if (n < 0 || (n > 0 && (!x || !out))) return -1;
    double c[kPgCoefs];
    pg_coef_init(c);
    for (int32_t i = 0; i < n; ++i) out[i] = pose_acos(x[i], c);
    return n;
}

int32_t plp_model_block_chol7_host(int32_t n, const int32_t* first, const double* env, const double* b, double lambda, double* out_x) {
    if (n < 0 || n > kPgMaxKf || (n > 0 && (!first || !env || !b || !out_x))) return -1;
    long long blocks = 0;
    for (int i = 0; i < n; ++i) {
        if (first[i] < 0 || first[i] > i) return -1;
        blocks += i - first[i] + 1;
    }
    if (n == 0) return 1;
    PgArgs B{};
    B.G = 1; B.F = n; B.edge_cap = 1; B.env_cap = (int)blocks;
    std::vector<double> d(pg_doubles(B.F, B.edge_cap, B.env_cap), 0.0);
    std::vector<int32_t> iv(pg_ints(B.F, B.edge_cap, B.env_cap), 0);
    B.ctx_d = d.data(); B.ctx_i = iv.data();
    static thread_local PgShared sh;
    PgTeamHost par;
    pg_offsets(B, 0, sh.O);
    const PgView V{B.ctx_d, B.ctx_i, &sh.O};
    int q = 0;
    for (int i = 0; i < n; ++i) { sh.first[i] = (int16_t)first[i]; sh.eoff[i] = q; q += i - first[i] + 1; }
    sh.eoff[n] = q; sh.n = n; sh.N = 7 * n; sh.nenv = q; sh.lambda = lambda;
    for (size_t k = 0; k < (size_t)49 * q; ++k) V.H()[k] = env[k];
    for (int p = 0; p < 7 * n; ++p) V.b()[p] = b[p];
    pg_solve_system(V, sh, par);
    for (int p = 0; p < 7 * n; ++p) out_x[p] = V.x()[p];
    return sh.ok ? 1 : 0;
}

plp_status plp_correct_landmarks_device(plp_matcher* c, const plp_correct_landmarks_args* a, void* hip_stream) {
    if (!c) return set_error(PLP_ERR_INVALID_ARG, "ctx is NULL");
    if (plp_status s = pgl_check(a)) return s;
    if (a->L == 0) return PLP_OK;
    return device_call(c, hip_stream, pgl_args(a), pgl_plan<DeviceRooms>, launch_correct_landmarks);
}

plp_status plp_correct_landmarks_host(plp_matcher* c, const plp_correct_landmarks_args* a) {
    if (!c) return set_error(PLP_ERR_INVALID_ARG, "ctx is NULL");
    if (plp_status s = pgl_check(a)) return s;
    if (a->L == 0) return PLP_OK;
    return host_call(c, pgl_args(a), pgl_plan<Stage>, launch_correct_landmarks);
}

int32_t plp_model_correct_landmarks_host(const plp_correct_landmarks_args* a) {
    if (plp_status s = pgl_check(a)) return -(int32_t)s;
    const PgLmArgs A = pgl_args(a);
    for (int l = 0; l < A.L; ++l) pg_correct_landmark(A, l);
    return A.L;
}

}  // extern "C"
