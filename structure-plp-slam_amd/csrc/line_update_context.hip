// Host driver + C ABI of the matcher context: the line map update (include/plp_front.h: plp_trim_line_endpoints_*, plp_correct_landmark_lines_*,
// plp_loop_ba_propagate_lines_*; line_update_kernels.hip, line_update.hpp)
#include <hip/hip_runtime.h>

#include <cmath>

#include "line_update.hpp"
#include "matcher_context.hpp"

using namespace plp;

extern "C" {

namespace {
// host: the arrays are host memory, so the offset list is checked as well
plp_status lt_check(const plp_trim_line_endpoints_args* a, bool host) {
    if (!a) return set_error(PLP_ERR_INVALID_ARG, "NULL argument");
    if (a->camera.model != PLP_CAMERA_PERSPECTIVE && a->camera.model != PLP_CAMERA_FISHEYE && a->camera.model != PLP_CAMERA_EQUIRECTANGULAR)
        return set_error(PLP_ERR_INVALID_ARG, "unknown camera model");
    if (a->camera.model != PLP_CAMERA_PERSPECTIVE) return set_error(PLP_ERR_UNSUPPORTED, "the end-point trim needs the perspective camera (graph_optimizer.cc:442)");
    if (!(a->camera.fx != 0) || !(a->camera.fy != 0) || !std::isfinite(a->camera.fx) || !std::isfinite(a->camera.fy) || !std::isfinite(a->camera.cx) ||
        !std::isfinite(a->camera.cy))
        return set_error(PLP_ERR_INVALID_ARG, "fx, fy must be non-zero, fx, fy, cx, cy finite");
    if (a->mode != PLP_TRIM_DEPTH_POSITIVE && a->mode != PLP_TRIM_MAX_CHANGE) return set_error(PLP_ERR_INVALID_ARG, "mode must be a plp_trim_mode");
    if (a->L < 0 || a->F < 0 || a->cap < 0) return set_error(PLP_ERR_INVALID_ARG, "L, F and cap must not be negative");
    if (a->pose_stride < 12) return set_error(PLP_ERR_INVALID_ARG, "pose_stride must be at least 12");
    if (a->L == 0) return PLP_OK;
    if (!a->pluecker || !a->ref_kf || !a->obs_offsets || !a->out_pos_w || !a->out_status || !a->out_erase)
        return set_error(PLP_ERR_INVALID_ARG, "pluecker, ref_kf, obs_offsets, out_pos_w, out_status and out_erase are required");
    if (a->F > 0 && (!a->pose || (a->cap > 0 && !a->keylines))) return set_error(PLP_ERR_INVALID_ARG, "pose and keylines are required");
    if (a->mode == PLP_TRIM_MAX_CHANGE && (!a->pos_w_old || (a->F > 0 && !a->median_depth)))
        return set_error(PLP_ERR_INVALID_ARG, "PLP_TRIM_MAX_CHANGE needs pos_w_old and median_depth");
    if (host) {
        if (a->obs_offsets[0] != 0) return set_error(PLP_ERR_INVALID_ARG, "obs_offsets must start at 0");
        for (int l = 0; l < a->L; ++l)
            if (a->obs_offsets[l + 1] < a->obs_offsets[l]) return set_error(PLP_ERR_INVALID_ARG, "obs_offsets must not decrease");
        if (a->obs_offsets[a->L] > 0 && (!a->obs_kf || !a->obs_idx)) return set_error(PLP_ERR_INVALID_ARG, "obs_kf and obs_idx are required");
    }
    return PLP_OK;
}
LineTrimArgs lt_args(const plp_trim_line_endpoints_args* a) {
    LineTrimArgs A{};
    A.L = a->L; A.F = a->F; A.cap = a->cap; A.pose_stride = a->pose_stride; A.mode = a->mode;
    A.fx = a->camera.fx; A.fy = a->camera.fy; A.cx = a->camera.cx; A.cy = a->camera.cy; A.max_change = a->max_change;
    A.pluecker = a->pluecker; A.ref_kf = a->ref_kf; A.skip = a->skip; A.obs_offsets = a->obs_offsets; A.obs_kf = a->obs_kf; A.obs_idx = a->obs_idx;
    A.pose = a->pose; A.kf_erased = a->kf_erased; A.kl = a->keylines; A.counts = a->counts;
    A.pos_w_old = a->mode == PLP_TRIM_MAX_CHANGE ? a->pos_w_old : nullptr; A.median = a->mode == PLP_TRIM_MAX_CHANGE ? a->median_depth : nullptr;
    A.out_pos_w = a->out_pos_w; A.out_status = a->out_status; A.out_erase = a->out_erase;
    return A;
}

plp_status lc_check(const plp_correct_landmark_lines_args* a) {
    if (!a) return set_error(PLP_ERR_INVALID_ARG, "NULL argument");
    if (a->L < 0 || a->F < 0) return set_error(PLP_ERR_INVALID_ARG, "L and F must not be negative");
    if (a->F > kLineUpdateMaxKfPg) return set_error(PLP_ERR_UNSUPPORTED, "more than 1024 key frames in the table");
    if (a->L > 0 && (!a->pluecker || !a->ref_kf || !a->out_pluecker || !a->out_status || (a->F > 0 && (!a->sim3_cw || !a->corrected_wc))))
        return set_error(PLP_ERR_INVALID_ARG, "pluecker, ref_kf, sim3_cw, corrected_wc, out_pluecker and out_status are required");
    return PLP_OK;
}
LineCorrectArgs lc_args(const plp_correct_landmark_lines_args* a) {
    LineCorrectArgs A{};
    A.L = a->L; A.F = a->F; A.pluecker = a->pluecker; A.lm_erased = a->lm_erased; A.ref_kf = a->ref_kf; A.corr_kf = a->corr_kf; A.kf_erased = a->kf_erased;
    A.sim3_cw = a->sim3_cw; A.corrected_wc = a->corrected_wc; A.out_pluecker = a->out_pluecker; A.out_status = a->out_status;
    return A;
}

plp_status lq_check(const plp_loop_ba_propagate_lines_args* a) {
    if (!a) return set_error(PLP_ERR_INVALID_ARG, "NULL argument");
    if (a->L < 0 || a->F < 0) return set_error(PLP_ERR_INVALID_ARG, "L and F must not be negative");
    if (a->F > kLineUpdateMaxKfBa) return set_error(PLP_ERR_UNSUPPORTED, "more than 4096 key frames in the table");
    if (a->L > 0 && (!a->pluecker || !a->ref_kf || !a->out_pluecker || !a->out_status || (a->line_optimized && !a->pluecker_after) ||
                     (a->F > 0 && (!a->pose_after || !a->pose_before || !a->kf_status))))
        return set_error(PLP_ERR_INVALID_ARG, "pluecker, ref_kf, pose_after, pose_before, kf_status, out_pluecker and out_status are required, pluecker_after with line_optimized");
    return PLP_OK;
}
LinePropagateArgs lq_args(const plp_loop_ba_propagate_lines_args* a) {
    LinePropagateArgs A{};
    A.L = a->L; A.F = a->F; A.pose_after = a->pose_after; A.pose_before = a->pose_before; A.kf_status = a->kf_status; A.pluecker = a->pluecker;
    A.lm_erased = a->lm_erased; A.ref_kf = a->ref_kf; A.line_optimized = a->line_optimized; A.pluecker_after = a->line_optimized ? a->pluecker_after : nullptr;
    A.out_pluecker = a->out_pluecker; A.out_status = a->out_status;
    return A;
}

// An output of these calls may be one of its inputs (out_pos_w and pos_w_old, out_pluecker and pluecker): one block then serves both, as one
// array serves both in the device form.  The plan leaves such an input out, as NULL, and the run points it at the output's block.
extern "C++" template <class R> void lt_plan(R& r, plp_matcher*, LineTrimArgs& A) {
    const size_t L = (size_t)A.L, F = (size_t)A.F, T = list_end(r, A.obs_offsets, A.L);
    r.in(A.pluecker, L * 6); r.in(A.ref_kf, L); r.in(A.skip, L); r.in(A.obs_offsets, L + 1); r.in(A.obs_kf, T); r.in(A.obs_idx, T);
    r.in(A.pose, F * A.pose_stride); r.in(A.kf_erased, F); r.in(A.kl, F * A.cap); r.in(A.counts, F); r.in(A.median, F);
    if ((const void*)A.pos_w_old == (const void*)A.out_pos_w) A.pos_w_old = nullptr;
    r.in(A.pos_w_old, L * 6);
    r.out(A.out_pos_w, L * 6); r.out(A.out_status, L); r.out(A.out_erase, L);
}
static hipError_t lt_run(hipStream_t st, LineTrimArgs& A) {
    if (A.mode == PLP_TRIM_MAX_CHANGE && !A.pos_w_old) A.pos_w_old = A.out_pos_w;
    return launch_trim_line_endpoints(st, A);
}

extern "C++" template <class R> void lc_plan(R& r, plp_matcher*, LineCorrectArgs& A) {
    const size_t L = (size_t)A.L, F = (size_t)A.F;
    if ((const void*)A.pluecker == (const void*)A.out_pluecker) A.pluecker = nullptr;
    r.in(A.pluecker, L * 6);
    r.in(A.lm_erased, L); r.in(A.ref_kf, L); r.in(A.corr_kf, L); r.in(A.kf_erased, F); r.in(A.sim3_cw, F * 8); r.in(A.corrected_wc, F * 8);
    r.out(A.out_pluecker, L * 6); r.out(A.out_status, L);
}
static hipError_t lc_run(hipStream_t st, LineCorrectArgs& A) {
    if (!A.pluecker) A.pluecker = A.out_pluecker;
    return launch_correct_landmark_lines(st, A);
}

extern "C++" template <class R> void lq_plan(R& r, plp_matcher*, LinePropagateArgs& A) {
    const size_t L = (size_t)A.L, F = (size_t)A.F;
    r.in(A.pose_after, F * 15); r.in(A.pose_before, F * 12); r.in(A.kf_status, F);
    if ((const void*)A.pluecker == (const void*)A.out_pluecker) A.pluecker = nullptr;
    r.in(A.pluecker, L * 6);
    r.in(A.lm_erased, L); r.in(A.ref_kf, L); r.in(A.line_optimized, L); r.in(A.pluecker_after, L * 6);
    r.out(A.out_pluecker, L * 6); r.out(A.out_status, L);
}
static hipError_t lq_run(hipStream_t st, LinePropagateArgs& A) {
    if (!A.pluecker) A.pluecker = A.out_pluecker;
    return launch_loop_ba_propagate_lines(st, A);
}
}  // namespace

plp_status plp_trim_line_endpoints_device(plp_matcher* c, const plp_trim_line_endpoints_args* a, void* hip_stream) {
    if (!c) return set_error(PLP_ERR_INVALID_ARG, "ctx is NULL");
    if (plp_status s = lt_check(a, false)) return s;
    if (a->L == 0) return PLP_OK;
    return device_call(c, hip_stream, lt_args(a), lt_plan<DeviceRooms>, lt_run);
}

plp_status plp_trim_line_endpoints_host(plp_matcher* c, const plp_trim_line_endpoints_args* a) {
    if (!c) return set_error(PLP_ERR_INVALID_ARG, "ctx is NULL");
    if (plp_status s = lt_check(a, true)) return s;
    if (a->L == 0) return PLP_OK;
    return host_call(c, lt_args(a), lt_plan<Stage>, lt_run);
}

int32_t plp_model_trim_line_endpoints_host(const plp_trim_line_endpoints_args* a) {
    if (plp_status s = lt_check(a, true)) return -(int32_t)s;
    const LineTrimArgs A = lt_args(a);
    for (int l = 0; l < A.L; ++l) line_trim_item(A, l);
    return A.L;
}

plp_status plp_correct_landmark_lines_device(plp_matcher* c, const plp_correct_landmark_lines_args* a, void* hip_stream) {
    if (!c) return set_error(PLP_ERR_INVALID_ARG, "ctx is NULL");
    if (plp_status s = lc_check(a)) return s;
    if (a->L == 0) return PLP_OK;
    return device_call(c, hip_stream, lc_args(a), lc_plan<DeviceRooms>, lc_run);
}

plp_status plp_correct_landmark_lines_host(plp_matcher* c, const plp_correct_landmark_lines_args* a) {
    if (!c) return set_error(PLP_ERR_INVALID_ARG, "ctx is NULL");
    if (plp_status s = lc_check(a)) return s;
    if (a->L == 0) return PLP_OK;
    return host_call(c, lc_args(a), lc_plan<Stage>, lc_run);
}

int32_t plp_model_correct_landmark_lines_host(const plp_correct_landmark_lines_args* a) {
    if (plp_status s = lc_check(a)) return -(int32_t)s;
    const LineCorrectArgs A = lc_args(a);
    for (int l = 0; l < A.L; ++l) line_correct_item(A, l);
    return A.L;
}

plp_status plp_loop_ba_propagate_lines_device(plp_matcher* c, const plp_loop_ba_propagate_lines_args* a, void* hip_stream) {
    if (!c) return set_error(PLP_ERR_INVALID_ARG, "ctx is NULL");
    if (plp_status s = lq_check(a)) return s;
    if (a->L == 0) return PLP_OK;
    return device_call(c, hip_stream, lq_args(a), lq_plan<DeviceRooms>, lq_run);
}

plp_status plp_loop_ba_propagate_lines_host(plp_matcher* c, const plp_loop_ba_propagate_lines_args* a) {
    if (!c) return set_error(PLP_ERR_INVALID_ARG, "ctx is NULL");
    if (plp_status s = lq_check(a)) return s;
    if (a->L == 0) return PLP_OK;
    return host_call(c, lq_args(a), lq_plan<Stage>, lq_run);
}

int32_t plp_model_loop_ba_propagate_lines_host(const plp_loop_ba_propagate_lines_args* a) {
    if (plp_status s = lq_check(a)) return -(int32_t)s;
    const LinePropagateArgs A = lq_args(a);
    for (int l = 0; l < A.L; ++l) line_propagate_item(A, l);
    return A.L;
}

}  // extern "C"
