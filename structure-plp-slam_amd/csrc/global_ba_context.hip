// Host driver + C ABI of the matcher context: global bundle adjustment and the loop adjuster's map update (include/plp_front.h: plp_global_ba_*,
// plp_loop_ba_propagate_*, plp_model_* host builds; global_ba_kernels.hip, global_ba.hpp)
#include <hip/hip_runtime.h>

#include <cmath>
#include <vector>

#include "matcher_context.hpp"
#include "global_ba.hpp"

using namespace plp;

extern "C" {

namespace {

plp_status gb_check(const plp_global_ba_args* a, bool host) {
    if (!a) return set_error(PLP_ERR_INVALID_ARG, "NULL argument");
    if (a->camera.model != PLP_CAMERA_PERSPECTIVE && a->camera.model != PLP_CAMERA_FISHEYE && a->camera.model != PLP_CAMERA_EQUIRECTANGULAR)
        return set_error(PLP_ERR_INVALID_ARG, "unknown camera model");
    if (a->setup_type < 0 || a->setup_type > 2) return set_error(PLP_ERR_INVALID_ARG, "setup_type must be 0, 1 or 2");
    if (a->F < 0 || a->L < 0 || a->T < 0 || a->kp_stride < 0) return set_error(PLP_ERR_INVALID_ARG, "F, L, T and kp_stride must not be negative");
    if (a->num_iter < 1) return set_error(PLP_ERR_INVALID_ARG, "num_iter must be positive");
    if (a->pose_stride < 12) return set_error(PLP_ERR_INVALID_ARG, "pose_stride must be at least 12");
    if (a->num_levels < 1 || a->num_levels > 16 || !a->inv_level_sigma_sq) return set_error(PLP_ERR_INVALID_ARG, "num_levels must be 1 .. 16, inv_level_sigma_sq is required");
    if (a->camera.model == PLP_CAMERA_EQUIRECTANGULAR) return set_error(PLP_ERR_UNSUPPORTED, "the equirectangular reprojection edge is not implemented (DESIGN.md D23)");
    if (!std::isfinite(a->camera.fx) || !std::isfinite(a->camera.fy) || !std::isfinite(a->camera.cx) || !std::isfinite(a->camera.cy) || a->camera.fx == 0 || a->camera.fy == 0)
        return set_error(PLP_ERR_INVALID_ARG, "fx, fy, cx, cy must be finite, fx and fy non-zero");
    if (a->F > kGbMaxKf) return set_error(PLP_ERR_UNSUPPORTED, "more than 4096 key frames in the table");
    if (a->L > kGbMaxLm || a->T > kGbMaxObs) return set_error(PLP_ERR_UNSUPPORTED, "more than 2^20 landmarks or 2^22 observations");
    if (!a->obs_offsets) return set_error(PLP_ERR_INVALID_ARG, "obs_offsets is required");
    if (a->F > 0 && (!a->pose || (a->kp_stride > 0 && !a->undist))) return set_error(PLP_ERR_INVALID_ARG, "pose and undist are required");
    if (a->L > 0 && !a->pos_w) return set_error(PLP_ERR_INVALID_ARG, "pos_w is required");
    if (a->T > 0 && (!a->obs_kf || !a->obs_idx)) return set_error(PLP_ERR_INVALID_ARG, "obs_kf and obs_idx are required");
    if (!a->out_status || (a->F > 0 && (!a->out_kf_optimized || !a->out_pose)) || (a->L > 0 && (!a->out_lm_optimized || !a->out_pos_w)))
        return set_error(PLP_ERR_INVALID_ARG, "out_status, out_kf_optimized, out_lm_optimized, out_pose, out_pos_w are required");
    if (host) {
        if (a->obs_offsets[0] != 0 || a->obs_offsets[a->L] != a->T) return set_error(PLP_ERR_INVALID_ARG, "obs_offsets must rise from 0 to T");
        for (int l = 0; l < a->L; ++l)
            if (a->obs_offsets[l + 1] < a->obs_offsets[l]) return set_error(PLP_ERR_INVALID_ARG, "obs_offsets must rise from 0 to T");
    }
    return PLP_OK;
}

GbArgs gb_args(const plp_global_ba_args* a) {
    GbArgs A{};
    A.F = a->F; A.L = a->L; A.T = a->T; A.kp_stride = a->kp_stride; A.pose_stride = a->pose_stride; A.num_levels = a->num_levels; A.robust = a->use_huber_kernel != 0;
    A.cam = pose_cam(a->camera.fx, a->camera.fy, a->camera.cx, a->camera.cy, a->camera.focal_x_baseline);
    A.delta = a->setup_type == 0 ? (double)std::sqrt(kPoseChiSq2D) : (double)std::sqrt(kPoseChiSq3D);
    for (int l = 0; l < 16; ++l) A.inv_sigma_sq[l] = l < A.num_levels ? a->inv_level_sigma_sq[l] : 0.0f;
    A.pose = a->pose; A.kf_erased = a->kf_erased; A.kf_is_origin = a->kf_is_origin; A.undist = a->undist; A.x_right = a->x_right; A.counts = a->counts;
    A.pos_w = a->pos_w; A.lm_erased = a->lm_erased; A.obs_offsets = a->obs_offsets; A.obs_kf = a->obs_kf; A.obs_idx = a->obs_idx;
    A.out_status = a->out_status; A.out_kf_optimized = a->out_kf_optimized; A.out_lm_optimized = a->out_lm_optimized; A.out_pose = a->out_pose;
    A.out_pos_w = a->out_pos_w; A.out_info = a->out_info; A.out_chi2 = a->out_chi2;
    return A;
}

extern "C++" template <class R> void gb_plan(R& r, plp_matcher*, GbArgs& A) {
    const size_t F = (size_t)A.F, L = (size_t)A.L, T = (size_t)A.T, K = (size_t)A.kp_stride;
    r.in(A.pose, F * A.pose_stride); r.in(A.kf_erased, F); r.in(A.kf_is_origin, F); r.in(A.undist, F * K); r.in(A.x_right, F * K); r.in(A.counts, F);
    r.in(A.pos_w, L * 3); r.in(A.lm_erased, L); r.in(A.obs_offsets, L + 1); r.in(A.obs_kf, T); r.in(A.obs_idx, T);
    r.out(A.out_status, 1); r.out(A.out_kf_optimized, F); r.out(A.out_lm_optimized, L); r.out(A.out_pose, F * 15); r.out(A.out_pos_w, L * 3);
    r.out(A.out_info, 4); r.out(A.out_chi2, 3);
}

// the run on the device, between the launches: the record comes back through pinned memory, one copy and one synchronisation of the stream
struct GbDeviceDriver {
    plp_matcher* c; hipStream_t st; GbArgs& A; int P = 0; hipError_t err = hipSuccess;
    GbRec read() {
        GbRec* pin = static_cast<GbRec*>(c->gb_pin.p);
        if (err == hipSuccess) err = hipMemcpyAsync(pin, A.rec, sizeof(GbRec), hipMemcpyDeviceToHost, st);
        if (err == hipSuccess) err = hipStreamSynchronize(st);
        if (err != hipSuccess) { GbRec r{}; r.end = 1; return r; }       // ends the loop; the entry reports err
        return *pin;
    }
    void lin(int it) { if (err == hipSuccess) err = gb_launch_lin(st, A, P, it); }
    GbRec try_step() {
        if (err == hipSuccess) err = gb_launch_try(st, A, P);
        return read();
    }
};

// the whole run of either form, which holds its state in the context's buffers and waits for the stream: the host reads the record between the launches
plp_status gb_run_device(plp_matcher* c, GbArgs& A, hipStream_t st, int iters, const volatile int32_t* stop) {
    PLP_HIP(c->gb_d.reserve(gb_doubles(A.F, A.L, A.T) * sizeof(double)));
    PLP_HIP(c->gb_i.reserve(gb_ints(A.F, A.T) * sizeof(int32_t)));
    PLP_HIP(c->gb_b.reserve(gb_bytes(A.F, A.L)));
    PLP_HIP(c->gb_rec.reserve(sizeof(GbRec)));
    PLP_HIP(c->gb_pin.reserve(sizeof(GbRec)));
    gb_bind(A, static_cast<double*>(c->gb_d.p), static_cast<int32_t*>(c->gb_i.p), static_cast<uint8_t*>(c->gb_b.p));
    A.rec = static_cast<GbRec*>(c->gb_rec.p);
    GbDeviceDriver drv{c, st, A};
    PLP_HIP(gb_launch_prepare(st, A));
    const GbRec r0 = drv.read();
    PLP_HIP(drv.err);
    if (r0.status == PLP_GLOBAL_BA_OK) {
        drv.P = r0.P;
        A.n = 6 * r0.P;
        PLP_HIP(c->gb_S.reserve((size_t)A.n * A.n * sizeof(double)));
        A.S = static_cast<double*>(c->gb_S.p);
        PLP_HIP(gb_launch_fill(st, A, drv.P));
        gb_loop(drv, iters, stop);
        PLP_HIP(drv.err);
    }
    PLP_HIP(gb_launch_finish(st, A, stop && *stop));
    PLP_HIP(hipStreamSynchronize(st));
    return PLP_OK;
}

plp_status lp_check(const plp_loop_ba_propagate_args* a) {
    if (!a) return set_error(PLP_ERR_INVALID_ARG, "NULL argument");
    if (a->F < 0 || a->L < 0) return set_error(PLP_ERR_INVALID_ARG, "F and L must not be negative");
    if (a->pose_stride < 12) return set_error(PLP_ERR_INVALID_ARG, "pose_stride must be at least 12");
    if (a->F > kGbMaxKf || a->L > kGbMaxLm) return set_error(PLP_ERR_UNSUPPORTED, "more than 4096 key frames or 2^20 landmarks");
    if (a->F > 0 && (!a->pose || !a->kf_parent || !a->kf_optimized || !a->pose_after || !a->out_pose || !a->out_pose_before || !a->out_kf_status))
        return set_error(PLP_ERR_INVALID_ARG, "pose, kf_parent, kf_optimized, pose_after, out_pose, out_pose_before and out_kf_status are required");
    if (a->L > 0 && (!a->pos_w || !a->ref_kf || !a->lm_optimized || !a->pos_after || !a->out_pos_w || !a->out_lm_status))
        return set_error(PLP_ERR_INVALID_ARG, "pos_w, ref_kf, lm_optimized, pos_after, out_pos_w and out_lm_status are required");
    return PLP_OK;
}
LpArgs lp_args(const plp_loop_ba_propagate_args* a) {
    LpArgs A{};
    A.F = a->F; A.L = a->L; A.pose_stride = a->pose_stride;
    A.pose = a->pose; A.kf_erased = a->kf_erased; A.kf_is_origin = a->kf_is_origin; A.kf_parent = a->kf_parent; A.kf_optimized = a->kf_optimized; A.pose_after = a->pose_after;
    A.pos_w = a->pos_w; A.lm_erased = a->lm_erased; A.ref_kf = a->ref_kf; A.lm_optimized = a->lm_optimized; A.pos_after = a->pos_after;
    A.out_pose = a->out_pose; A.out_pose_before = a->out_pose_before; A.out_kf_status = a->out_kf_status; A.out_pos_w = a->out_pos_w; A.out_lm_status = a->out_lm_status;
    return A;
}

extern "C++" template <class R> void lp_plan(R& r, plp_matcher*, LpArgs& A) {
    const size_t F = (size_t)A.F, L = (size_t)A.L;
    r.in(A.pose, F * A.pose_stride); r.in(A.kf_erased, F); r.in(A.kf_is_origin, F); r.in(A.kf_parent, F); r.in(A.kf_optimized, F); r.in(A.pose_after, F * 15);
    r.in(A.pos_w, L * 3); r.in(A.lm_erased, L); r.in(A.ref_kf, L); r.in(A.lm_optimized, L); r.in(A.pos_after, L * 3);
    r.out(A.out_pose, F * 15); r.out(A.out_pose_before, F * 12); r.out(A.out_kf_status, F); r.out(A.out_pos_w, L * 3); r.out(A.out_lm_status, L);
}
}  // namespace

plp_status plp_global_ba_device(plp_matcher* c, const plp_global_ba_args* a, void* hip_stream) {
    if (!c) return set_error(PLP_ERR_INVALID_ARG, "ctx is NULL");
    if (plp_status s = gb_check(a, false)) return s;
    return device_call(c, hip_stream, gb_args(a), gb_plan<DeviceRooms>,
                       [=](hipStream_t st, GbArgs& A) { return gb_run_device(c, A, st, a->num_iter, a->stop); });
}

plp_status plp_global_ba_host(plp_matcher* c, const plp_global_ba_args* a) {
    if (!c) return set_error(PLP_ERR_INVALID_ARG, "ctx is NULL");
    if (plp_status s = gb_check(a, true)) return s;
    return host_call(c, gb_args(a), gb_plan<Stage>, [=](hipStream_t st, GbArgs& A) { return gb_run_device(c, A, st, a->num_iter, a->stop); });
}

int32_t plp_model_global_ba_host(const plp_global_ba_args* a) {
    if (plp_status s = gb_check(a, true)) return -(int32_t)s;
    GbArgs A = gb_args(a);
    gb_run_host(A, a->num_iter, a->stop);
    return 1;
}

plp_status plp_loop_ba_propagate_device(plp_matcher* c, const plp_loop_ba_propagate_args* a, void* hip_stream) {
    if (!c) return set_error(PLP_ERR_INVALID_ARG, "ctx is NULL");
    if (plp_status s = lp_check(a)) return s;
    return device_call(c, hip_stream, lp_args(a), lp_plan<DeviceRooms>, lp_launch);
}

plp_status plp_loop_ba_propagate_host(plp_matcher* c, const plp_loop_ba_propagate_args* a) {
    if (!c) return set_error(PLP_ERR_INVALID_ARG, "ctx is NULL");
    if (plp_status s = lp_check(a)) return s;
    return host_call(c, lp_args(a), lp_plan<Stage>, lp_launch);
}

int32_t plp_model_loop_ba_propagate_host(const plp_loop_ba_propagate_args* a) {
    if (plp_status s = lp_check(a)) return -(int32_t)s;
    const LpArgs A = lp_args(a);
    for (int f = 0; f < A.F; ++f) lp_kf_out(A, f);
    for (int l = 0; l < A.L; ++l) lp_lm_item(A, l);
    return 1;
}

int32_t plp_model_chol_dense_host(int32_t n, const double* Ain, const double* b, double lambda, double* out_x, int32_t* out_ok) {
    if (n < 0 || !out_ok || (n > 0 && (!Ain || !b || !out_x))) return -1;
    std::vector<double> S(Ain, Ain + (size_t)n * n);
    for (int j = 0; j < n; ++j) S[(size_t)j * n + j] = S[(size_t)j * n + j] + lambda;
    const bool ok = gb_chol_host(S.data(), n);
    for (int j = 0; j < n; ++j) out_x[j] = ok ? b[j] : 0.0;
    if (ok) gb_subst_host(S.data(), n, out_x);
    out_ok[0] = ok ? 1 : 0;
    return n;
}

plp_status plp_chol_dense_host(plp_matcher* c, int32_t n, const double* Ain, const double* b, double lambda, double* out_x, int32_t* out_ok) {
    if (!c) return set_error(PLP_ERR_INVALID_ARG, "ctx is NULL");
    if (n < 0 || n > 6 * kGbMaxKf || !out_ok || (n > 0 && (!Ain || !b || !out_x))) return set_error(PLP_ERR_INVALID_ARG, "n must be 0 .. 24576, A, b, out_x and out_ok are required");
    if (n == 0) { out_ok[0] = 1; return PLP_OK; }
    std::vector<double> S(Ain, Ain + (size_t)n * n);
    for (int j = 0; j < n; ++j) S[(size_t)j * n + j] = S[(size_t)j * n + j] + lambda;
    std::lock_guard<std::mutex> lk(c->mu);
    PLP_HIP(hipSetDevice(c->device));
    PLP_HIP(c->gb_S.reserve((size_t)n * n * sizeof(double)));
    PLP_HIP(c->gb_d.reserve((size_t)n * sizeof(double)));
    PLP_HIP(c->gb_rec.reserve(sizeof(GbRec)));
    GbRec rec{};
    rec.ok = 1;
    PLP_HIP(hipMemcpyAsync(c->gb_S.p, S.data(), (size_t)n * n * sizeof(double), hipMemcpyHostToDevice, c->stream));
    PLP_HIP(hipMemcpyAsync(c->gb_d.p, b, (size_t)n * sizeof(double), hipMemcpyHostToDevice, c->stream));
    PLP_HIP(hipMemcpyAsync(c->gb_rec.p, &rec, sizeof(GbRec), hipMemcpyHostToDevice, c->stream));
    PLP_HIP(gb_launch_chol(c->stream, static_cast<double*>(c->gb_S.p), static_cast<double*>(c->gb_d.p), n, static_cast<GbRec*>(c->gb_rec.p)));
    PLP_HIP(hipMemcpyAsync(out_x, c->gb_d.p, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    PLP_HIP(hipMemcpyAsync(&rec, c->gb_rec.p, sizeof(GbRec), hipMemcpyDeviceToHost, c->stream));
    PLP_HIP(hipStreamSynchronize(c->stream));
    out_ok[0] = rec.ok ? 1 : 0;
    return PLP_OK;
}

}  // extern "C"
