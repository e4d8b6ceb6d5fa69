// Host driver + C ABI of the array-form Hamming matchers (include/plp_front.h): the matchers, the query builders, the pair triangulation, BoW and
// the side kernels.  The solvers' entries of the same context are in sim3_, pnp_, essential_, two_view_, pose_opt_, transform_opt_, local_ba_, local_map_,
// plane_, map_cull_, covisibility_, pose_graph_, global_ba_ and line_update_context.hip; matcher_context.hpp holds what all of them run through.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <mutex>
#include <vector>

#include "bow_database.hpp"
#include "bow_score.hpp"
#include "landmark_geometry.hpp"
#include "libstdcxx_sort.hpp"
#include "match_device.hpp"
#include "matcher_context.hpp"

using namespace plp;

namespace {

// An EMPTY side -- a frame without key points / key lines (n_cap = 0) or an empty set of landmarks / queries (m_cap = 0): nothing can match, the reference's loops do not
// run (projection.cc, robust.cc, fuse.cc: every matcher starts from `unsigned int num_matches = 0` and iterates over the landmarks).  The result is defined without a
// kernel: every out_match slot -1, every out_num 0 (fuse modes: every out_query_best -1).  Returns 1 when the call is such a call and well-formed, 0 otherwise.
int empty_side(const plp_match_args* a) {
    if (!a || a->B <= 0 || a->n_cap < 0 || a->m_cap < 0 || (a->n_cap > 0 && a->m_cap > 0)) return 0;
    if (a->mode < PLP_MATCH_MODE_LANDMARKS || a->mode > PLP_MATCH_MODE_TRIANGULATION) return 0;
    const bool fuse = a->mode == PLP_MATCH_MODE_FUSE || a->mode == PLP_MATCH_MODE_FUSE_LINE;
    if (fuse ? (a->m_cap > 0 && !a->out_query_best) : (!a->out_num || (a->n_cap > 0 && !a->out_match))) return 0;
    return 1;
}

plp_status check_args(const plp_match_args* a) {
    if (!a) return set_error(PLP_ERR_INVALID_ARG, "args is NULL");
    if (a->B <= 0 || a->n_cap <= 0 || a->m_cap <= 0) return set_error(PLP_ERR_INVALID_ARG, "B must be positive, n_cap and m_cap non-negative (with the outputs an empty side needs)");
    if (a->n_cap > 8192) return set_error(PLP_ERR_UNSUPPORTED, "more than 8192 key points per frame");
    if (!a->t_desc || !a->q_desc) return set_error(PLP_ERR_INVALID_ARG, "descriptor arrays are required");
    if (a->mode != PLP_MATCH_MODE_FUSE && a->mode != PLP_MATCH_MODE_FUSE_LINE && (!a->out_match || !a->out_num)) return set_error(PLP_ERR_INVALID_ARG, "output arrays are required");
    if (a->mode == PLP_MATCH_MODE_BRUTE_FORCE) {
        if (a->check_orientation && (!a->t_angle || !a->q_angle)) return set_error(PLP_ERR_INVALID_ARG, "check_orientation needs t_angle and q_angle");
    } else if (a->mode == PLP_MATCH_MODE_LANDMARKS || a->mode == PLP_MATCH_MODE_LAST_FRAME) {
        if (!a->t_kps || !a->q_reproj || !a->q_level || !a->scale_factors) return set_error(PLP_ERR_INVALID_ARG, "t_kps, q_reproj, q_level, scale_factors are required");
        if (a->num_levels <= 0 || a->num_levels > 16) return set_error(PLP_ERR_INVALID_ARG, "num_levels must be in [1,16]");
        if (a->grid.cols <= 0 || a->grid.rows <= 0 || a->grid.cols * a->grid.rows > 4096) return set_error(PLP_ERR_INVALID_ARG, "grid must have 1..4096 cells");
        if (a->mode == PLP_MATCH_MODE_LAST_FRAME && a->check_orientation && !a->q_angle) return set_error(PLP_ERR_INVALID_ARG, "check_orientation needs q_angle");
    } else if (a->mode == PLP_MATCH_MODE_LANDMARKS_LINE || a->mode == PLP_MATCH_MODE_LAST_FRAME_LINE) {
        if (!a->t_kl || !a->q_reproj || !a->q_reproj2 || !a->q_level || !a->scale_factors) return set_error(PLP_ERR_INVALID_ARG, "t_kl, q_reproj, q_reproj2, q_level, scale_factors are required");
        if (a->mode == PLP_MATCH_MODE_LANDMARKS_LINE && !a->t_kp_octave) return set_error(PLP_ERR_INVALID_ARG, "t_kp_octave is required");
        if (a->num_levels <= 0 || a->num_levels > 16) return set_error(PLP_ERR_INVALID_ARG, "num_levels must be in [1,16]");
    } else if (a->mode == PLP_MATCH_MODE_BOW) {
        if (!a->q_group || !a->t_group) return set_error(PLP_ERR_INVALID_ARG, "q_group and t_group are required");
        if (a->check_orientation && (!a->t_angle || !a->q_angle)) return set_error(PLP_ERR_INVALID_ARG, "check_orientation needs t_angle and q_angle");
    } else if (a->mode == PLP_MATCH_MODE_FUSE) {
        if (!a->t_kps || !a->q_reproj_d || !a->q_level || !a->scale_factors || !a->inv_level_sigma_sq || !a->out_query_best) return set_error(PLP_ERR_INVALID_ARG, "t_kps, q_reproj_d, q_level, scale_factors, inv_level_sigma_sq, out_query_best are required");
        if (a->num_levels <= 0 || a->num_levels > 16) return set_error(PLP_ERR_INVALID_ARG, "num_levels must be in [1,16]");
        if (a->grid.cols <= 0 || a->grid.rows <= 0 || a->grid.cols * a->grid.rows > 4096) return set_error(PLP_ERR_INVALID_ARG, "grid must have 1..4096 cells");
    } else if (a->mode == PLP_MATCH_MODE_FUSE_LINE) {
        if (!a->t_kl || !a->q_reproj_d || !a->q_reproj2_d || !a->q_level || !a->scale_factors || !a->inv_level_sigma_sq || !a->out_query_best) return set_error(PLP_ERR_INVALID_ARG, "t_kl, q_reproj_d, q_reproj2_d, q_level, scale_factors, inv_level_sigma_sq, out_query_best are required");
        if (a->num_levels <= 0 || a->num_levels > 16) return set_error(PLP_ERR_INVALID_ARG, "num_levels must be in [1,16]");
    } else if (a->mode == PLP_MATCH_MODE_TRIANGULATION) {
        if (!a->q_group || !a->t_group || !a->q_bearing || !a->t_bearing || !a->epipolar || !a->q_level || !a->scale_factors) return set_error(PLP_ERR_INVALID_ARG, "q_group, t_group, q_bearing, t_bearing, epipolar, q_level, scale_factors are required");
        if (a->num_levels <= 0 || a->num_levels > 16) return set_error(PLP_ERR_INVALID_ARG, "num_levels must be in [1,16]");
        if (a->check_orientation && (!a->t_angle || !a->q_angle)) return set_error(PLP_ERR_INVALID_ARG, "check_orientation needs t_angle and q_angle");
    } else return set_error(PLP_ERR_INVALID_ARG, "unknown mode");
    if (a->hamm_dist_thr < 0 || a->hamm_dist_thr > 256 || a->level_window < 0 || a->level_window > 2) return set_error(PLP_ERR_INVALID_ARG, "hamm_dist_thr / level_window out of range");
    return PLP_OK;
}

// targets of a frame k_match_topk_cells keeps in LDS (plp_match_args.t_count_hint)
int lds_targets_of(const plp_match_args* a) { return a->t_count_hint > 0 ? std::min(a->t_count_hint, a->n_cap) : a->n_cap; }

plp_status run_device(plp_matcher* c, const plp_match_args* a, hipStream_t st) {
    PLP_HIP(hipSetDevice(c->device));
    const size_t qn = (size_t)a->B * a->m_cap;
    PLP_HIP(c->klist.reserve(qn * kMatchK * 4));
    PLP_HIP(c->klist2.reserve(qn * kMatchK * 4));
    PLP_HIP(c->kcount.reserve(qn * 4));
    PLP_HIP(c->claim.reserve(qn * 4));
    PLP_HIP(c->full_list.reserve(qn * 4));
    const size_t tn_ = (size_t)a->B * a->n_cap;
    PLP_HIP(c->sorted.reserve(tn_ * sizeof(StagedTarget)));
    PLP_HIP(c->sorted_xr.reserve(tn_ * 4));
    PLP_HIP(c->row_start.reserve((size_t)a->B * 4104 * 2));
    if (!c->dbg.p) { PLP_HIP(c->dbg.reserve(16)); PLP_HIP(hipMemsetAsync(c->dbg.p, 0, 16, st)); }
    MatchProblem P{};
    P.mode = a->mode; P.n_cap = a->n_cap; P.m_cap = a->m_cap; P.q_desc_stride = a->q_desc_stride > 0 ? a->q_desc_stride : a->m_cap;
    P.t_kps = (a->mode == PLP_MATCH_MODE_LANDMARKS || a->mode == PLP_MATCH_MODE_LAST_FRAME || a->mode == PLP_MATCH_MODE_FUSE) ? a->t_kps : nullptr;
    P.q_group = a->q_group; P.t_group = a->t_group; P.q_reproj_d = a->q_reproj_d; P.out_query_best = a->out_query_best;
    P.hamm_dist_thr = a->hamm_dist_thr; P.level_window = a->level_window; P.flags = a->flags;
    P.q_reproj2_d = a->q_reproj2_d; P.q_bearing = a->q_bearing; P.t_bearing = a->t_bearing; P.epipolar = a->epipolar;
    fill_levels(P.inv_level_sigma_sq, a->inv_level_sigma_sq, a->num_levels);
    P.t_desc = a->t_desc; P.t_x_right = a->t_x_right; P.t_occupied = a->t_occupied; P.t_angle = a->t_angle; P.t_counts = a->t_counts;
    P.q_valid = a->q_valid; P.q_reproj = a->q_reproj; P.q_x_right = a->q_x_right; P.q_level = a->q_level; P.q_angle = a->q_angle;
    P.q_desc = a->q_desc; P.q_has_obs = a->q_has_obs; P.q_counts = a->q_counts;
    P.t_kl = a->t_kl; P.t_kp_octave = a->t_kp_octave; P.t_x_right2 = a->t_x_right2; P.q_reproj2 = a->q_reproj2; P.q_x_right2 = a->q_x_right2;
    P.is_rgbd = a->is_rgbd; P.num_levels_lsd = a->num_levels_lsd;
    P.margin = a->margin; P.lowe_ratio = a->lowe_ratio; P.direction = a->direction;
    P.directions = (a->mode == PLP_MATCH_MODE_LAST_FRAME || a->mode == PLP_MATCH_MODE_LAST_FRAME_LINE) ? a->directions : nullptr;
    P.check_orientation = a->check_orientation;
    P.num_levels = a->num_levels;
    fill_levels(P.scale_factors, a->scale_factors, a->num_levels);
    P.grid_min_x = a->grid.min_x; P.grid_min_y = a->grid.min_y; P.inv_cell_w = a->grid.inv_cell_width; P.inv_cell_h = a->grid.inv_cell_height;
    P.grid_cols = a->grid.cols; P.grid_rows = a->grid.rows;
    P.klist = (uint32_t*)c->klist.p; P.klist2 = (uint32_t*)c->klist2.p; P.kcount = (int32_t*)c->kcount.p; P.claim = (int32_t*)c->claim.p; P.full_list = (int32_t*)c->full_list.p;
    P.sorted = (StagedTarget*)c->sorted.p; P.sorted_xr = (float*)c->sorted_xr.p; P.cell_start = (uint16_t*)c->row_start.p; P.dbg = (int32_t*)c->dbg.p;
    P.out_match = a->out_match; P.out_num = a->out_num;
    P.lds_targets = lds_targets_of(a);
    launch_match(st, P, a->B);
    PLP_HIP(hipGetLastError());
    return PLP_OK;
}

}  // namespace

extern "C" {

plp_status plp_matcher_create(int device, plp_matcher** out) {
    if (!out) return set_error(PLP_ERR_INVALID_ARG, "out is NULL");
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n == 0) return set_error(PLP_ERR_NO_DEVICE, "no HIP device visible: the matchers have no CPU fallback");
    if (device < 0 || device >= n) return set_error(PLP_ERR_INVALID_ARG, "device index out of range");
    PLP_HIP(hipSetDevice(device));
    PLP_HIP(configure_match_kernels());
    plp_matcher* c = new plp_matcher();
    c->device = device;
    if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) { delete c; return set_error(PLP_ERR_HIP, "hipStreamCreate failed"); }
    *out = c;
    return PLP_OK;
}

void plp_matcher_destroy(plp_matcher* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->stream) { (void)hipStreamSynchronize(c->stream); (void)hipStreamDestroy(c->stream); }
    delete c;
}

plp_status plp_match_device(plp_matcher* c, const plp_match_args* a, void* hip_stream) {
    if (!c) return set_error(PLP_ERR_INVALID_ARG, "ctx is NULL");
    if (empty_side(a)) {
        std::lock_guard<std::mutex> lk(c->mu);
        PLP_HIP(hipSetDevice(c->device));
        hipStream_t st = (hipStream_t)hip_stream;
        if (a->mode == PLP_MATCH_MODE_FUSE || a->mode == PLP_MATCH_MODE_FUSE_LINE) {
            if (a->m_cap > 0) PLP_HIP(hipMemsetAsync(a->out_query_best, 0xFF, (size_t)a->B * a->m_cap * 4, st));
            return PLP_OK;
        }
        if (a->n_cap > 0) PLP_HIP(hipMemsetAsync(a->out_match, 0xFF, (size_t)a->B * a->n_cap * 4, st));
        PLP_HIP(hipMemsetAsync(a->out_num, 0, (size_t)a->B * 4, st));
        return PLP_OK;
    }
    PLP_TRY(check_args(a));
    std::lock_guard<std::mutex> lk(c->mu);
    return run_device(c, a, (hipStream_t)hip_stream);
}

plp_status plp_match_host(plp_matcher* c, const plp_match_args* a) {
    if (!c) return set_error(PLP_ERR_INVALID_ARG, "ctx is NULL");
    if (empty_side(a)) {
        if (a->mode == PLP_MATCH_MODE_FUSE || a->mode == PLP_MATCH_MODE_FUSE_LINE) { std::fill_n(a->out_query_best, (size_t)a->B * a->m_cap, -1); return PLP_OK; }
        std::fill_n(a->out_match, (size_t)a->B * a->n_cap, -1);
        std::fill_n(a->out_num, (size_t)a->B, 0);
        return PLP_OK;
    }
    PLP_TRY(check_args(a));
    if (a->q_desc_stride != 0 && a->q_desc_stride != a->m_cap) return set_error(PLP_ERR_UNSUPPORTED, "q_desc_stride is a device-path option (overlapping query windows of a batched replay)");
    std::lock_guard<std::mutex> lk(c->mu);
    PLP_HIP(hipSetDevice(c->device));
    const size_t B = (size_t)a->B, tn = B * a->n_cap, qn = B * a->m_cap;
    plp_match_args d = *a;
    Stage s(c->stage, c->stream);
    s.in(d.t_kps, tn); s.in(d.t_desc, tn * 32); s.in(d.t_x_right, tn); s.in(d.t_occupied, tn); s.in(d.t_angle, tn); s.in(d.t_counts, B);
    s.in(d.q_valid, qn); s.in(d.q_reproj, qn * 2); s.in(d.q_x_right, qn); s.in(d.q_level, qn); s.in(d.q_angle, qn); s.in(d.q_desc, qn * 32);
    s.in(d.q_has_obs, qn); s.in(d.q_counts, B); s.in(d.t_kl, tn); s.in(d.t_kp_octave, tn); s.in(d.t_x_right2, tn); s.in(d.q_reproj2, qn * 2);
    s.in(d.q_x_right2, qn); s.in(d.q_group, qn); s.in(d.t_group, tn); s.in(d.q_reproj_d, qn * 2); s.in(d.q_reproj2_d, qn * 2);
    s.in(d.q_bearing, qn * 3); s.in(d.t_bearing, tn * 3); s.in(d.epipolar, B * 12); s.in(d.directions, B);
    // Only the mode's own result comes back; the other outputs are device-only regions (out_query_best: when the caller passes one).  Without
    // counts every slot of the result is written: nothing to keep.  out_num is written for every problem.
    if (a->mode == PLP_MATCH_MODE_FUSE || a->mode == PLP_MATCH_MODE_FUSE_LINE) {
        s.out(d.out_query_best, qn, a->q_counts != nullptr);
        s.room(d.out_match, tn); s.room(d.out_num, B);
    } else {
        s.room(d.out_query_best, a->out_query_best ? qn : 0);
        s.out(d.out_match, tn, a->t_counts != nullptr); s.out(d.out_num, B, false);
    }
    PLP_TRY(s.upload());
    PLP_TRY(run_device(c, &d, c->stream));
    return s.finish();
}

// order in which Mihasher::query enumerates the bit-flip patterns with s ones inside a b-bit substring
// (binary_descriptor_matcher.cpp:671-735): rank[pattern] = position inside its popcount class
static MihRanks mih_ranks() {
    MihRanks R;
    for (int i = 0; i < 256; ++i) R.rank[i] = 255;
    const int curb = 8;
    for (int s = 0; s <= 8; ++s) {
        int power[16];
        unsigned long long bitstr = 0;
        for (int i = 0; i < s; ++i) power[i] = i;
        power[s] = curb + 1;
        int bit = s - 1, pos = 0;
        while (true) {
            if (bit != -1) {
                bitstr ^= (power[bit] == bit) ? 1ull << power[bit] : 3ull << (power[bit] - 1);
                power[bit]++;
                bit--;
            } else {
                if (bitstr < 256 && R.rank[bitstr] == 255) R.rank[bitstr] = (uint8_t)std::min(pos, 254);
                ++pos;
                while (++bit < s && power[bit] == power[bit + 1] - 1) {
                    bitstr ^= 1ull << (power[bit] - 1);
                    power[bit] = bit;
                }
                if (bit == s) break;
            }
        }
    }
    return R;
}

plp_status plp_lbd_match_1nn_device(plp_matcher* c, const uint8_t* d_q, const int32_t* d_q_counts, int32_t nq_cap, const uint8_t* d_t,
                                    const int32_t* d_t_counts, int32_t nt_cap, int32_t B, int32_t* d_train_idx, int32_t* d_dist, void* hip_stream) {
    if (!c || !d_q || !d_t || !d_train_idx || !d_dist) return set_error(PLP_ERR_INVALID_ARG, "NULL argument");
    if (nq_cap <= 0 || nt_cap <= 0 || B <= 0 || nt_cap > 65535) return set_error(PLP_ERR_INVALID_ARG, "bad sizes");
    PLP_HIP(hipSetDevice(c->device));
    static const MihRanks R = mih_ranks();
    launch_lbd_match_1nn((hipStream_t)hip_stream, d_q, d_q_counts, nq_cap, d_t, d_t_counts, nt_cap, R, d_train_idx, d_dist, B);
    PLP_HIP(hipGetLastError());
    return PLP_OK;
}

plp_status plp_lbd_match_1nn_host(plp_matcher* c, const uint8_t* q, int32_t nq, const uint8_t* t, int32_t nt, int32_t* train_idx, int32_t* dist) {
    if (!c || !q || !t || !train_idx || !dist) return set_error(PLP_ERR_INVALID_ARG, "NULL argument");
    if (nq <= 0 || nt <= 0) return PLP_OK;   // the reference prints an error and returns with `matches` untouched (:201-205)
    if (nt > 65535) return set_error(PLP_ERR_UNSUPPORTED, "more than 65535 train descriptors (16-bit index in the tie-break key)");
    struct { const uint8_t *q, *t; int32_t *train_idx, *dist; } A{q, t, train_idx, dist};
    return host_call(
        c, A, [=](Stage& s, plp_matcher*, auto& A) { s.in(A.q, (size_t)nq * 32); s.in(A.t, (size_t)nt * 32); s.out(A.train_idx, nq, false); s.out(A.dist, nq, false); },
        [=](hipStream_t st, auto& A) {
            static const MihRanks R = mih_ranks();
            launch_lbd_match_1nn(st, A.q, nullptr, nq, A.t, nullptr, nt, R, A.train_idx, A.dist, 1);
            return hipGetLastError();
        });
}

plp_status plp_match_area_host(plp_matcher* c, const plp_keypoint* kps_1, const uint8_t* desc_1, int32_t n1, const plp_keypoint* kps_2,
                               const uint8_t* desc_2, int32_t n2, const plp_match_grid* grid, float* prev_matched_pts, int32_t margin,
                               float lowe_ratio, int32_t check_orientation, int32_t* matched_2_in_1, int32_t* num_matches) {
    if (!c || !grid || !matched_2_in_1 || !num_matches) return set_error(PLP_ERR_INVALID_ARG, "NULL argument");
    if (n1 <= 0) { *num_matches = 0; return PLP_OK; }
    // refusals come before anything is written: the tie-break key holds the cell index (at most 65535) and idx_2 in 16 bits each
    if (!kps_1 || !desc_1 || !prev_matched_pts || n2 < 0 || (n2 > 0 && (!kps_2 || !desc_2)) || n2 > 65535) return set_error(PLP_ERR_INVALID_ARG, "bad argument");
    if (grid->cols <= 0 || grid->rows <= 0 || (int64_t)grid->cols * grid->rows > 65536) return set_error(PLP_ERR_INVALID_ARG, "grid must have a positive extent and at most 65536 cells");
    AreaArgs A{};
    A.kps1 = kps_1; A.desc1 = desc_1; A.kps2 = kps_2; A.desc2 = desc_2; A.n1 = n1; A.n2 = n2;
    A.grid_min_x = grid->min_x; A.grid_min_y = grid->min_y; A.inv_cell_w = grid->inv_cell_width; A.inv_cell_h = grid->inv_cell_height;
    A.grid_cols = grid->cols; A.grid_rows = grid->rows;
    A.prev_pts = prev_matched_pts; A.margin = (float)margin; A.lowe_ratio = lowe_ratio; A.check_orientation = check_orientation;
    A.matched_2_in_1 = matched_2_in_1; A.num_matches = num_matches;
    return host_call(
        c, A,
        [=](Stage& s, plp_matcher*, AreaArgs& A) {   // n2 == 0: the kernel reads no key point of frame 2 and no scratch
            s.in(A.kps1, n1); s.in(A.desc1, (size_t)n1 * 32); s.in(A.kps2, n2); s.in(A.desc2, (size_t)n2 * 32);
            s.out(A.matched_2_in_1, n1, false); s.out(A.prev_pts, (size_t)n1 * 2); s.out(A.num_matches, 1, false); s.room(A.scratch, (size_t)n2 * 2);
        },
        [](hipStream_t st, AreaArgs& A) { launch_match_area(st, A); return hipGetLastError(); });
}

namespace {
PostArgs post_args(const plp_camera* cam) {
    PostArgs A{};
    A.fx = cam->fx; A.fy = cam->fy; A.cx = cam->cx; A.cy = cam->cy;
    // cv_cam_matrix_ / cv_dist_params_ are cv::Mat_<float> (camera/perspective.cc:47-48)
    A.fx_f = (double)(float)cam->fx; A.fy_f = (double)(float)cam->fy; A.cx_f = (double)(float)cam->cx; A.cy_f = (double)(float)cam->cy;
    const double k[5] = {cam->k1, cam->k2, cam->p1, cam->p2, cam->k3};
    for (int i = 0; i < 5; ++i) A.k[i] = (double)(float)k[i];
    A.fxb = cam->focal_x_baseline;
    return A;
}

// plp_camera_model -> PostArgs, as the three constructors store the camera (perspective.cc:47-48, fisheye.cc:47-48, equirectangular.cc:36)
PostArgs model_post_args(const plp_camera_model* cam) {
    PostArgs A{};
    A.model = cam->model;
    if (cam->model == PLP_CAMERA_EQUIRECTANGULAR) {
        A.cols_f = (float)(unsigned)cam->cols; A.rows_f = (float)(unsigned)cam->rows;
        return A;
    }
    const plp_camera p{cam->fx, cam->fy, cam->cx, cam->cy, cam->k1, cam->k2, cam->p1, cam->p2, cam->k3, cam->focal_x_baseline};
    const PostArgs P = post_args(&p);
    A.fx = P.fx; A.fy = P.fy; A.cx = P.cx; A.cy = P.cy; A.fx_f = P.fx_f; A.fy_f = P.fy_f; A.cx_f = P.cx_f; A.cy_f = P.cy_f;
    A.fxb = P.fxb;
    if (cam->model == PLP_CAMERA_FISHEYE) {   // cv_dist_params_ = (k1, k2, k3, k4) as cv::Mat_<float>
        const double k[4] = {cam->k1, cam->k2, cam->k3, cam->k4};
        for (int i = 0; i < 4; ++i) A.k[i] = (double)(float)k[i];
    } else {
        for (int i = 0; i < 5; ++i) A.k[i] = P.k[i];
    }
    return A;
}

plp_status post_extract_device(plp_matcher* c, const PostArgs& cam_args, const plp_keypoint* d_kps, const int32_t* d_counts, int32_t cap,
                               int32_t B, const float* d_depth, int32_t rows, int32_t cols, size_t depth_step, size_t depth_frame_stride,
                               plp_keypoint* d_undist, double* d_bearings, float* d_x_right, float* d_depths,
                               const plp_keyline* d_kl, const int32_t* d_kl_counts, int32_t kl_cap, float* d_kl_depths,
                               float* d_kl_x_right, void* hip_stream);
plp_status post_extract_host(plp_matcher* c, const PostArgs& cam_args, const plp_keypoint* kps, int32_t n, const float* depth, int32_t rows,
                             int32_t cols, size_t depth_step, plp_keypoint* undist, double* bearings, float* x_right, float* depths,
                             const plp_keyline* kl, int32_t n_kl, float* kl_depths, float* kl_x_right);
}  // namespace

plp_status check_camera_model(const plp_camera_model* cam, bool depth_or_lines) {
    if (!cam) return set_error(PLP_ERR_INVALID_ARG, "NULL argument");
    switch (cam->model) {
    case PLP_CAMERA_PERSPECTIVE:
    case PLP_CAMERA_FISHEYE:
        if (!(cam->fx != 0) || !(cam->fy != 0)) return set_error(PLP_ERR_INVALID_ARG, "fx, fy must be non-zero");
        return PLP_OK;
    case PLP_CAMERA_EQUIRECTANGULAR:
        if (cam->cols <= 0 || cam->rows <= 0) return set_error(PLP_ERR_INVALID_ARG, "cols, rows must be positive");
        if (depth_or_lines) return set_error(PLP_ERR_UNSUPPORTED, "the equirectangular camera is monocular: no depth, no key lines");
        return PLP_OK;
    default:
        return set_error(PLP_ERR_INVALID_ARG, "unknown camera model");
    }
}

plp_status plp_post_extract_device(plp_matcher* c, const plp_camera* cam, const plp_keypoint* d_kps, const int32_t* d_counts, int32_t cap,
                                   int32_t B, const float* d_depth, int32_t rows, int32_t cols, size_t depth_step, size_t depth_frame_stride,
                                   plp_keypoint* d_undist, double* d_bearings, float* d_x_right, float* d_depths,
                                   const plp_keyline* d_kl, const int32_t* d_kl_counts, int32_t kl_cap, float* d_kl_depths,
                                   float* d_kl_x_right, void* hip_stream) {
    if (!c || !cam) return set_error(PLP_ERR_INVALID_ARG, "NULL argument");
    if (B <= 0 || (d_kps && cap <= 0) || (d_kl && kl_cap <= 0)) return set_error(PLP_ERR_INVALID_ARG, "bad sizes");
    if (!d_kps && !d_kl) return PLP_OK;
    if (d_kps && !d_undist) return set_error(PLP_ERR_INVALID_ARG, "d_undist is required with d_kps");
    if (d_depth && (rows <= 0 || cols <= 0 || depth_step < (size_t)cols * 4)) return set_error(PLP_ERR_INVALID_ARG, "bad depth geometry");
    if (d_kl && (!d_depth || !d_kl_depths || !d_kl_x_right)) return set_error(PLP_ERR_INVALID_ARG, "key lines need depth, d_kl_depths, d_kl_x_right");
    if (!(cam->fx != 0) || !(cam->fy != 0)) return set_error(PLP_ERR_INVALID_ARG, "fx, fy must be non-zero");
    return post_extract_device(c, post_args(cam), d_kps, d_counts, cap, B, d_depth, rows, cols, depth_step, depth_frame_stride, d_undist, d_bearings,
                               d_x_right, d_depths, d_kl, d_kl_counts, kl_cap, d_kl_depths, d_kl_x_right, hip_stream);
}

plp_status plp_post_extract_model_device(plp_matcher* c, const plp_camera_model* cam, const plp_keypoint* d_kps, const int32_t* d_counts,
                                         int32_t cap, int32_t B, const float* d_depth, int32_t rows, int32_t cols, size_t depth_step,
                                         size_t depth_frame_stride, plp_keypoint* d_undist, double* d_bearings, float* d_x_right, float* d_depths,
                                         const plp_keyline* d_kl, const int32_t* d_kl_counts, int32_t kl_cap, float* d_kl_depths,
                                         float* d_kl_x_right, void* hip_stream) {
    if (!c) return set_error(PLP_ERR_INVALID_ARG, "NULL argument");
    if (plp_status s = check_camera_model(cam, d_depth || d_kl)) return s;
    return post_extract_device(c, model_post_args(cam), d_kps, d_counts, cap, B, d_depth, rows, cols, depth_step, depth_frame_stride, d_undist, d_bearings,
                               d_x_right, d_depths, d_kl, d_kl_counts, kl_cap, d_kl_depths, d_kl_x_right, hip_stream);
}

plp_status plp_post_extract_host(plp_matcher* c, const plp_camera* cam, const plp_keypoint* kps, int32_t n, const float* depth, int32_t rows,
                                 int32_t cols, size_t depth_step, plp_keypoint* undist, double* bearings, float* x_right, float* depths,
                                 const plp_keyline* kl, int32_t n_kl, float* kl_depths, float* kl_x_right) {
    if (!c || !cam) return set_error(PLP_ERR_INVALID_ARG, "NULL argument");
    return post_extract_host(c, post_args(cam), kps, n, depth, rows, cols, depth_step, undist, bearings, x_right, depths, kl, n_kl, kl_depths, kl_x_right);
}

plp_status plp_post_extract_model_host(plp_matcher* c, const plp_camera_model* cam, const plp_keypoint* kps, int32_t n, const float* depth,
                                       int32_t rows, int32_t cols, size_t depth_step, plp_keypoint* undist, double* bearings, float* x_right,
                                       float* depths, const plp_keyline* kl, int32_t n_kl, float* kl_depths, float* kl_x_right) {
    if (!c) return set_error(PLP_ERR_INVALID_ARG, "NULL argument");
    if (plp_status s = check_camera_model(cam, depth || kl || n_kl > 0)) return s;
    return post_extract_host(c, model_post_args(cam), kps, n, depth, rows, cols, depth_step, undist, bearings, x_right, depths, kl, n_kl, kl_depths, kl_x_right);
}

namespace {
plp_status post_extract_device(plp_matcher* c, const PostArgs& cam_args, const plp_keypoint* d_kps, const int32_t* d_counts, int32_t cap,
                               int32_t B, const float* d_depth, int32_t rows, int32_t cols, size_t depth_step, size_t depth_frame_stride,
                               plp_keypoint* d_undist, double* d_bearings, float* d_x_right, float* d_depths,
                               const plp_keyline* d_kl, const int32_t* d_kl_counts, int32_t kl_cap, float* d_kl_depths,
                               float* d_kl_x_right, void* hip_stream) {
    if (B <= 0 || (d_kps && cap <= 0) || (d_kl && kl_cap <= 0)) return set_error(PLP_ERR_INVALID_ARG, "bad sizes");
    if (!d_kps && !d_kl) return PLP_OK;
    if (d_kps && !d_undist) return set_error(PLP_ERR_INVALID_ARG, "d_undist is required with d_kps");
    if (d_depth && (rows <= 0 || cols <= 0 || depth_step < (size_t)cols * 4)) return set_error(PLP_ERR_INVALID_ARG, "bad depth geometry");
    if (d_kl && (!d_depth || !d_kl_depths || !d_kl_x_right)) return set_error(PLP_ERR_INVALID_ARG, "key lines need depth, d_kl_depths, d_kl_x_right");
    PostArgs A = cam_args;
    A.kps = d_kps; A.counts = d_counts; A.cap = d_kps ? cap : 0;
    A.depth = d_depth; A.depth_step = depth_step; A.depth_frame_stride = depth_frame_stride;
    A.undist = d_undist; A.bearings = d_bearings; A.x_right = d_x_right; A.depths = d_depths;
    A.kl = d_kl; A.kl_counts = d_kl_counts; A.kl_cap = d_kl ? kl_cap : 0; A.kl_depths = d_kl_depths; A.kl_x_right = d_kl_x_right;
    return device_call(c, hip_stream, A, NoArrays{}, [B](hipStream_t st, PostArgs& A) { launch_post_extract(st, A, B); return hipGetLastError(); });
}

plp_status post_extract_host(plp_matcher* c, const PostArgs& cam_args, const plp_keypoint* kps, int32_t n, const float* depth, int32_t rows,
                             int32_t cols, size_t depth_step, plp_keypoint* undist, double* bearings, float* x_right, float* depths,
                             const plp_keyline* kl, int32_t n_kl, float* kl_depths, float* kl_x_right) {
    if (n < 0 || n_kl < 0) return set_error(PLP_ERR_INVALID_ARG, "negative count");
    if (n == 0 && n_kl == 0) return PLP_OK;
    if (n > 0 && (!kps || !undist)) return set_error(PLP_ERR_INVALID_ARG, "kps and undist are required");
    if (n_kl > 0 && (!kl || !depth || !kl_depths || !kl_x_right)) return set_error(PLP_ERR_INVALID_ARG, "key lines need depth and both outputs");
    if (depth && (rows <= 0 || cols <= 0 || depth_step < (size_t)cols * 4)) return set_error(PLP_ERR_INVALID_ARG, "bad depth geometry");
    std::lock_guard<std::mutex> lk(c->mu);
    PLP_HIP(hipSetDevice(c->device));
    PostArgs A = cam_args;
    A.kps = kps; A.cap = n; A.undist = undist; A.bearings = bearings;
    const bool stereo = depth && x_right && depths;
    A.x_right = stereo ? x_right : nullptr; A.depths = stereo ? depths : nullptr;
    A.kl = kl; A.kl_cap = n_kl; A.kl_depths = kl_depths; A.kl_x_right = kl_x_right;
    A.depth_step = (size_t)cols * 4;
    const size_t px = depth ? (size_t)rows * cols : 0;
    Stage s(c->stage, c->stream);   // n == 0 / n_kl == 0: the kernel tests kps / kl before it touches that side's outputs
    s.in(A.kps, n); s.out(A.undist, n, false); s.out(A.bearings, (size_t)n * 3, false); s.out(A.x_right, n, false); s.out(A.depths, n, false);
    s.in(A.kl, n_kl); s.out(A.kl_depths, (size_t)n_kl * 2); s.out(A.kl_x_right, (size_t)n_kl * 2);   // skipped lines keep the caller's values
    float* img = nullptr;
    s.room(img, px);
    PLP_TRY(s.upload());
    A.depth = img;
    if (depth) {   // the depth image through a page-locked buffer with slack (plp_common.hpp HostPinned): no 2-D copy reads the caller's pageable memory
        PLP_HIP(c->pin.reserve(px * sizeof(float)));
        c->pin.pack(0, reinterpret_cast<const uint8_t*>(depth), depth_step, rows, cols * 4);
        PLP_HIP(hipMemcpyAsync(img, c->pin.p, px * sizeof(float), hipMemcpyHostToDevice, c->stream));
    }
    launch_post_extract(c->stream, A, 1);
    PLP_HIP(hipGetLastError());
    return s.finish();
}
}  // namespace

// ---- local-landmark visibility (include/plp_front.h: plp_observe_landmark[_line]s_*; kernels in observe_kernels.hip)
namespace {
plp_status observe_check(plp_matcher* c, const plp_observe_args* a, bool lines) {
    if (!c || !a) return set_error(PLP_ERR_INVALID_ARG, "NULL argument");
    if (plp_status s = check_camera_model(&a->camera, false)) return s;
    if (a->B <= 0 || a->m_cap < 0 || a->num_levels <= 0) return set_error(PLP_ERR_INVALID_ARG, "B and num_levels must be positive, m_cap non-negative");
    if (!a->pose || !a->pos_w || !a->out_reproj || !a->out_valid) return set_error(PLP_ERR_INVALID_ARG, "pose, pos_w, out_reproj, out_valid are required");
    const bool scale = lines || a->obs_mean_normal;
    if (scale && (!a->min_valid_dist || !a->max_valid_dist || !a->out_level))
        return set_error(PLP_ERR_INVALID_ARG, "min_valid_dist, max_valid_dist, out_level are required (points: unless obs_mean_normal is NULL)");
    if (lines && !a->out_reproj2) return set_error(PLP_ERR_INVALID_ARG, "out_reproj2 is required for lines");
    return PLP_OK;
}

ObserveArgs observe_args(const plp_observe_args* a, bool lines) {
    ObserveArgs A{};
    set_camera(A, a->camera);
    std::copy_n(a->img_bounds, 4, A.bounds);
    A.ray_cos_thr = a->ray_cos_thr; A.log_sf = a->log_scale_factor; A.num_levels = a->num_levels; A.m_cap = a->m_cap;
    A.pose = a->pose; A.counts = a->counts; A.pos_w = a->pos_w; A.normal = lines ? nullptr : a->obs_mean_normal;
    const bool scale = lines || a->obs_mean_normal;
    A.min_dist = scale ? a->min_valid_dist : nullptr; A.max_dist = scale ? a->max_valid_dist : nullptr; A.skip = a->skip;
    A.reproj = a->out_reproj; A.reproj2 = lines ? a->out_reproj2 : nullptr; A.x_right = lines ? nullptr : a->out_x_right;
    A.level = scale ? a->out_level : nullptr; A.valid = a->out_valid; A.num_valid = a->out_num_valid;
    return A;
}

// a launch_* function that takes the number of problems (frames) after the arguments, as a run
extern "C++" template <class Args> auto run_of(hipError_t (*launch)(hipStream_t, const Args&, int), int B) {
    return [=](hipStream_t st, const Args& A) { return launch(st, A, B); };
}

// the device form of a call without a landmark slot (m_cap == 0), where the reference's loop does not run: only the counts are cleared
static plp_status clear_num_valid_device(plp_matcher* c, int32_t* d_num_valid, int B, void* hip_stream) {
    return device_call(c, hip_stream, NoArgs{}, NoArrays{},
                       [=](hipStream_t st, NoArgs&) { return d_num_valid ? hipMemsetAsync(d_num_valid, 0, (size_t)B * 4, st) : hipSuccess; });
}

// the arrays of a call of B problems, points or lines
extern "C++" auto observe_plan(int B_, bool lines) {
    return [=](auto& r, plp_matcher*, ObserveArgs& A) {
        const size_t B = (size_t)B_, BM = B * A.m_cap;
        r.in(A.pose, B * 15); r.in(A.counts, B); r.in(A.pos_w, BM * (lines ? 6 : 3)); r.in(A.normal, BM * 3);
        r.in(A.min_dist, BM); r.in(A.max_dist, BM); r.in(A.skip, BM);
        r.out(A.reproj, BM * 2); r.out(A.reproj2, BM * 2); r.out(A.x_right, BM); r.out(A.level, BM); r.out(A.valid, BM); r.out(A.num_valid, B);
    };
}

plp_status observe_device(plp_matcher* c, const plp_observe_args* a, bool lines, void* hip_stream) {
    if (plp_status s = observe_check(c, a, lines)) return s;
    if (a->m_cap == 0) return clear_num_valid_device(c, a->out_num_valid, a->B, hip_stream);
    return device_call(c, hip_stream, observe_args(a, lines), observe_plan(a->B, lines), run_of(lines ? launch_observe_lines : launch_observe_points, a->B));
}

plp_status observe_host(plp_matcher* c, const plp_observe_args* a, bool lines) {
    if (plp_status s = observe_check(c, a, lines)) return s;
    if (a->m_cap == 0) {
        if (a->out_num_valid) std::memset(a->out_num_valid, 0, (size_t)a->B * 4);
        return PLP_OK;
    }
    return host_call(c, observe_args(a, lines), observe_plan(a->B, lines), run_of(lines ? launch_observe_lines : launch_observe_points, a->B));
}
}  // namespace

plp_status plp_observe_landmarks_device(plp_matcher* c, const plp_observe_args* a, void* hip_stream) { return observe_device(c, a, false, hip_stream); }
plp_status plp_observe_landmarks_host(plp_matcher* c, const plp_observe_args* a) { return observe_host(c, a, false); }
plp_status plp_observe_landmark_lines_device(plp_matcher* c, const plp_observe_args* a, void* hip_stream) { return observe_device(c, a, true, hip_stream); }
plp_status plp_observe_landmark_lines_host(plp_matcher* c, const plp_observe_args* a) { return observe_host(c, a, true); }

// ---- last-frame queries (include/plp_front.h: plp_project_last_frame[_lines]_*; kernels in observe_kernels.hip)
namespace {
plp_status last_frame_check(plp_matcher* c, const plp_last_frame_args* a, bool lines) {
    if (!c || !a) return set_error(PLP_ERR_INVALID_ARG, "NULL argument");
    if (plp_status s = check_camera_model(&a->camera, false)) return s;
    if (a->setup_type < 0 || a->setup_type > 2) return set_error(PLP_ERR_INVALID_ARG, "setup_type must be 0 (monocular), 1 (stereo) or 2 (RGB-D)");
    if (a->B <= 0 || a->m_cap < 0) return set_error(PLP_ERR_INVALID_ARG, "B must be positive, m_cap non-negative");
    if (!a->pose_curr || !a->pose_last || !a->pos_w || !a->out_reproj || !a->out_level || !a->out_valid || !a->out_direction)
        return set_error(PLP_ERR_INVALID_ARG, "pose_curr, pose_last, pos_w, out_reproj, out_level, out_valid, out_direction are required");
    if (lines ? (!a->keylines || !a->out_reproj2) : !a->keypts)
        return set_error(PLP_ERR_INVALID_ARG, lines ? "keylines and out_reproj2 are required for lines" : "keypts is required for points");
    return PLP_OK;
}

ObserveArgs last_frame_args(const plp_last_frame_args* a, bool lines) {
    ObserveArgs A{};
    set_camera(A, a->camera);
    std::copy_n(a->img_bounds, 4, A.bounds);
    A.m_cap = a->m_cap; A.setup_type = a->setup_type; A.true_baseline = a->true_baseline;
    A.pose = a->pose_curr; A.pose_last = a->pose_last; A.counts = a->counts; A.pos_w = a->pos_w; A.skip = a->skip;
    A.kps = lines ? nullptr : a->keypts; A.kl = lines ? a->keylines : nullptr;
    A.reproj = a->out_reproj; A.reproj2 = lines ? a->out_reproj2 : nullptr; A.x_right = a->out_x_right; A.x_right2 = lines ? a->out_x_right2 : nullptr;
    A.level = a->out_level; A.angle = lines ? nullptr : a->out_angle; A.valid = a->out_valid; A.direction = a->out_direction; A.num_valid = a->out_num_valid;
    return A;
}

// the arrays of a call of B problems, points or lines.  m_cap == 0: nothing per slot is staged, the kernels still write every problem's direction and num_valid
extern "C++" auto last_frame_plan(int B_, bool lines) {
    return [=](auto& r, plp_matcher*, ObserveArgs& A) {
        const size_t B = (size_t)B_, BM = B * A.m_cap;
        r.in(A.pose, B * 15); r.in(A.pose_last, B * 15); r.in(A.counts, B); r.in(A.pos_w, BM * (lines ? 6 : 3)); r.in(A.skip, BM);
        r.in(A.kps, BM); r.in(A.kl, BM);
        r.out(A.reproj, BM * 2); r.out(A.reproj2, BM * 2); r.out(A.x_right, BM); r.out(A.x_right2, BM); r.out(A.level, BM); r.out(A.angle, BM);
        r.out(A.valid, BM); r.out(A.direction, B); r.out(A.num_valid, B);
    };
}

plp_status last_frame_device(plp_matcher* c, const plp_last_frame_args* a, bool lines, void* hip_stream) {
    if (plp_status s = last_frame_check(c, a, lines)) return s;
    return device_call(c, hip_stream, last_frame_args(a, lines), last_frame_plan(a->B, lines), run_of(lines ? launch_last_frame_lines : launch_last_frame_points, a->B));
}

plp_status last_frame_host(plp_matcher* c, const plp_last_frame_args* a, bool lines) {
    if (plp_status s = last_frame_check(c, a, lines)) return s;
    return host_call(c, last_frame_args(a, lines), last_frame_plan(a->B, lines), run_of(lines ? launch_last_frame_lines : launch_last_frame_points, a->B));
}
}  // namespace

plp_status plp_project_last_frame_device(plp_matcher* c, const plp_last_frame_args* a, void* hip_stream) { return last_frame_device(c, a, false, hip_stream); }
plp_status plp_project_last_frame_host(plp_matcher* c, const plp_last_frame_args* a) { return last_frame_host(c, a, false); }
plp_status plp_project_last_frame_lines_device(plp_matcher* c, const plp_last_frame_args* a, void* hip_stream) { return last_frame_device(c, a, true, hip_stream); }
plp_status plp_project_last_frame_lines_host(plp_matcher* c, const plp_last_frame_args* a) { return last_frame_host(c, a, true); }

// ---- fuse, Sim3 and relocalisation queries (include/plp_front.h: plp_project_landmark[_line]s_*; kernels in project_kernels.hip)
namespace {
plp_status project_check(plp_matcher* c, const plp_project_args* a, bool lines) {
    if (!c || !a) return set_error(PLP_ERR_INVALID_ARG, "NULL argument");
    if (plp_status s = check_camera_model(&a->camera, false)) return s;
    if (a->B <= 0 || a->m_cap < 0 || a->num_levels <= 0) return set_error(PLP_ERR_INVALID_ARG, "B and num_levels must be positive, m_cap non-negative");
    if (!a->pose || !a->pos_w || !a->min_valid_dist || !a->max_valid_dist || !a->out_valid)
        return set_error(PLP_ERR_INVALID_ARG, "pose, pos_w, min_valid_dist, max_valid_dist, out_valid are required");
    if (!a->out_reproj_d && !a->out_reproj) return set_error(PLP_ERR_INVALID_ARG, "one of out_reproj_d and out_reproj is required");
    if (a->dist_mode != PLP_PROJECT_DIST_CENTER && a->dist_mode != PLP_PROJECT_DIST_CAMERA) return set_error(PLP_ERR_INVALID_ARG, "unknown dist_mode");
    if (lines) {
        if (a->line_dist_mode != PLP_PROJECT_LINE_ENDPOINTS && a->line_dist_mode != PLP_PROJECT_LINE_MIDPOINT)
            return set_error(PLP_ERR_INVALID_ARG, "unknown line_dist_mode");
        if (a->dist_mode != PLP_PROJECT_DIST_CENTER || a->ray_test) return set_error(PLP_ERR_INVALID_ARG, "lines take PLP_PROJECT_DIST_CENTER and no ray_test");
        if ((a->out_reproj_d && !a->out_reproj2_d) || (a->out_reproj && !a->out_reproj2))
            return set_error(PLP_ERR_INVALID_ARG, "lines need the end-point array of every start-point array (out_reproj2_d, out_reproj2)");
    } else if (a->ray_test && (!a->obs_mean_normal || a->dist_mode != PLP_PROJECT_DIST_CENTER)) {
        return set_error(PLP_ERR_INVALID_ARG, "ray_test needs obs_mean_normal and PLP_PROJECT_DIST_CENTER");
    }
    if (a->B > 65535) return set_error(PLP_ERR_UNSUPPORTED, "more than 65535 problems in one call");
    return PLP_OK;
}

ProjectArgs project_args(const plp_project_args* a, bool lines) {
    ProjectArgs A{};
    set_camera(A, a->camera);
    std::copy_n(a->img_bounds, 4, A.bounds);
    A.log_sf = a->log_scale_factor; A.num_levels = a->num_levels; A.m_cap = a->m_cap;
    A.shared = a->shared_landmarks ? 1 : 0; A.dist_mode = a->dist_mode; A.ray_test = (!lines && a->ray_test) ? 1 : 0; A.line_dist_mode = a->line_dist_mode;
    A.pose = a->pose; A.counts = a->counts; A.pos_w = a->pos_w; A.normal = (!lines && a->ray_test) ? a->obs_mean_normal : nullptr;
    A.min_dist = a->min_valid_dist; A.max_dist = a->max_valid_dist; A.skip = a->skip;
    A.reproj_d = a->out_reproj_d; A.reproj2_d = (lines && a->out_reproj_d) ? a->out_reproj2_d : nullptr;
    A.reproj = a->out_reproj; A.reproj2 = (lines && a->out_reproj) ? a->out_reproj2 : nullptr;
    A.x_right = a->out_x_right; A.x_right2 = lines ? a->out_x_right2 : nullptr;
    A.level = a->out_level; A.valid = a->out_valid; A.status = a->out_status; A.num_valid = a->out_num_valid;
    return A;
}

// the arrays of a call of B problems, points or lines
extern "C++" auto project_plan(int B_, bool lines) {
    return [=](auto& r, plp_matcher*, ProjectArgs& A) {
        const size_t B = (size_t)B_, M = (size_t)A.m_cap, BM = B * M;
        const size_t LM = A.shared ? M : BM;   // rows of the landmark tables
        r.in(A.pose, B * 15); r.in(A.counts, B); r.in(A.pos_w, LM * (lines ? 6 : 3)); r.in(A.normal, LM * 3);
        r.in(A.min_dist, LM); r.in(A.max_dist, LM); r.in(A.skip, BM);
        r.out(A.reproj_d, BM * 2); r.out(A.reproj2_d, BM * 2); r.out(A.reproj, BM * 2); r.out(A.reproj2, BM * 2); r.out(A.x_right, BM); r.out(A.x_right2, BM);
        r.out(A.level, BM); r.out(A.valid, BM); r.out(A.status, BM); r.out(A.num_valid, B);
    };
}

plp_status project_device(plp_matcher* c, const plp_project_args* a, bool lines, void* hip_stream) {
    if (plp_status s = project_check(c, a, lines)) return s;
    if (a->m_cap == 0) return clear_num_valid_device(c, a->out_num_valid, a->B, hip_stream);
    return device_call(c, hip_stream, project_args(a, lines), project_plan(a->B, lines), run_of(lines ? launch_project_lines : launch_project_points, a->B));
}

plp_status project_host(plp_matcher* c, const plp_project_args* a, bool lines) {
    if (plp_status s = project_check(c, a, lines)) return s;
    if (a->m_cap == 0) {
        if (a->out_num_valid) std::memset(a->out_num_valid, 0, (size_t)a->B * 4);
        return PLP_OK;
    }
    return host_call(c, project_args(a, lines), project_plan(a->B, lines), run_of(lines ? launch_project_lines : launch_project_points, a->B));
}
}  // namespace

plp_status plp_project_landmarks_device(plp_matcher* c, const plp_project_args* a, void* hip_stream) { return project_device(c, a, false, hip_stream); }
plp_status plp_project_landmarks_host(plp_matcher* c, const plp_project_args* a) { return project_host(c, a, false); }
plp_status plp_project_landmark_lines_device(plp_matcher* c, const plp_project_args* a, void* hip_stream) { return project_device(c, a, true, hip_stream); }
plp_status plp_project_landmark_lines_host(plp_matcher* c, const plp_project_args* a) { return project_host(c, a, true); }

// ---- stereo key lines (include/plp_front.h: plp_stereo_keylines_*, plp_keylines_3d_*; kernels in stereo_line_kernels.hip)
namespace {
plp_status stereo_keylines_check(plp_matcher* c, const plp_stereo_keylines_args* a) {
    if (!c || !a) return set_error(PLP_ERR_INVALID_ARG, "NULL argument");
    if (a->B <= 0 || a->cap_left < 0 || a->cap_right < 0) return set_error(PLP_ERR_INVALID_ARG, "B must be positive, cap_left and cap_right non-negative");
    if (!a->out_good_match || !a->out_kl_depths || !a->out_kl_x_right)
        return set_error(PLP_ERR_INVALID_ARG, "out_good_match, out_kl_depths, out_kl_x_right are required");
    if (a->cap_left > 0 && !a->keylines_left) return set_error(PLP_ERR_INVALID_ARG, "keylines_left is required");
    if (a->cap_left > 0 && a->cap_right > 0 && (!a->keylines_right || !a->train_idx || !a->dist))
        return set_error(PLP_ERR_INVALID_ARG, "keylines_right, train_idx, dist are required when both sides have slots");
    return PLP_OK;
}

StereoKeylineArgs stereo_keylines_args(const plp_stereo_keylines_args* a) {
    StereoKeylineArgs A{};
    A.cap_l = a->cap_left; A.cap_r = a->cap_right;
    A.kl_l = a->keylines_left; A.counts_l = a->counts_left; A.kl_r = a->keylines_right; A.counts_r = a->counts_right;
    A.train_idx = a->train_idx; A.dist = a->dist;
    A.good = a->out_good_match; A.depths = a->out_kl_depths; A.x_right = a->out_kl_x_right;
    if (A.cap_r == 0) { A.kl_r = nullptr; A.counts_r = nullptr; A.train_idx = nullptr; A.dist = nullptr; }   // not read: every slot -1
    return A;
}

plp_status keylines_3d_check(plp_matcher* c, const plp_keylines_3d_args* a) {
    if (!c || !a) return set_error(PLP_ERR_INVALID_ARG, "NULL argument");
    if (plp_status s = check_camera_model(&a->camera, true)) return s;
    if (a->camera.model != PLP_CAMERA_PERSPECTIVE) return set_error(PLP_ERR_UNSUPPORTED, "3-D key lines need the perspective camera (frame.cc:957)");
    if (a->setup_type != 1 && a->setup_type != 2) return set_error(PLP_ERR_INVALID_ARG, "setup_type must be 1 (stereo) or 2 (RGB-D)");
    if (a->B <= 0 || a->cap < 0 || a->cap_right < 0) return set_error(PLP_ERR_INVALID_ARG, "B must be positive, cap and cap_right non-negative");
    if (!a->pose || !a->keylines || !a->out_pos_w) return set_error(PLP_ERR_INVALID_ARG, "pose, keylines, out_pos_w are required");
    if (a->setup_type == 2 && !a->kl_depths) return set_error(PLP_ERR_INVALID_ARG, "kl_depths is required for RGB-D");
    if (a->setup_type == 1 && (!a->good_match || (a->cap_right > 0 && !a->keylines_right)))
        return set_error(PLP_ERR_INVALID_ARG, "good_match (and keylines_right when cap_right > 0) are required for stereo");
    return PLP_OK;
}

Keylines3dArgs keylines_3d_args(const plp_keylines_3d_args* a) {
    Keylines3dArgs A{};
    const plp_camera_model& cm = a->camera;
    A.fx = cm.fx; A.fy = cm.fy; A.cx = cm.cx; A.cy = cm.cy; A.fxb = cm.focal_x_baseline;
    A.fx_inv = 1.0 / cm.fx; A.fy_inv = 1.0 / cm.fy;   // perspective.cc:42
    A.setup_type = a->setup_type; A.cap = a->cap; A.cap_r = a->cap_right;
    A.counts = a->counts; A.pose = a->pose; A.kl = a->keylines;
    const bool rgbd = a->setup_type == 2;
    A.kl_depths = rgbd ? a->kl_depths : nullptr;
    A.good_match = rgbd ? nullptr : a->good_match;
    A.kl_r = rgbd || a->cap_right == 0 ? nullptr : a->keylines_right;
    A.counts_r = rgbd || a->cap_right == 0 ? nullptr : a->counts_right;
    A.pos_w = a->out_pos_w; A.valid = a->out_valid;
    return A;
}

extern "C++" auto stereo_keylines_plan(int B_) {
    return [=](auto& r, plp_matcher*, StereoKeylineArgs& A) {
        const size_t B = (size_t)B_, L = (size_t)A.cap_l, R = (size_t)A.cap_r;
        r.in(A.kl_l, B * L); r.in(A.counts_l, B); r.in(A.kl_r, B * R); r.in(A.counts_r, B); r.in(A.train_idx, B * L); r.in(A.dist, B * L);
        r.out(A.good, B * L); r.out(A.depths, B * L * 2); r.out(A.x_right, B * L * 2);
    };
}
extern "C++" auto keylines_3d_plan(int B_) {
    return [=](auto& r, plp_matcher*, Keylines3dArgs& A) {
        const size_t B = (size_t)B_, M = (size_t)A.cap, R = (size_t)A.cap_r;
        r.in(A.counts, B); r.in(A.pose, B * 15); r.in(A.kl, B * M); r.in(A.kl_depths, B * M * 2); r.in(A.good_match, B * M); r.in(A.kl_r, B * R);
        r.in(A.counts_r, B); r.out(A.pos_w, B * M * 6); r.out(A.valid, B * M);
    };
}
}  // namespace

plp_status plp_stereo_keylines_device(plp_matcher* c, const plp_stereo_keylines_args* a, void* hip_stream) {
    if (plp_status s = stereo_keylines_check(c, a)) return s;
    if (a->cap_left == 0) return PLP_OK;   // no left key line: nothing to write
    return device_call(c, hip_stream, stereo_keylines_args(a), stereo_keylines_plan(a->B), run_of(launch_stereo_keylines, a->B));
}

plp_status plp_stereo_keylines_host(plp_matcher* c, const plp_stereo_keylines_args* a) {
    if (plp_status s = stereo_keylines_check(c, a)) return s;
    if (a->cap_left == 0) return PLP_OK;
    return host_call(c, stereo_keylines_args(a), stereo_keylines_plan(a->B), run_of(launch_stereo_keylines, a->B));
}

plp_status plp_keylines_3d_device(plp_matcher* c, const plp_keylines_3d_args* a, void* hip_stream) {
    if (plp_status s = keylines_3d_check(c, a)) return s;
    if (a->cap == 0) return PLP_OK;
    return device_call(c, hip_stream, keylines_3d_args(a), keylines_3d_plan(a->B), run_of(launch_keylines_3d, a->B));
}

plp_status plp_keylines_3d_host(plp_matcher* c, const plp_keylines_3d_args* a) {
    if (plp_status s = keylines_3d_check(c, a)) return s;
    if (a->cap == 0) return PLP_OK;
    return host_call(c, keylines_3d_args(a), keylines_3d_plan(a->B), run_of(launch_keylines_3d, a->B));
}

// ---- key-frame pair line triangulation (include/plp_front.h: plp_median_depth_*, plp_triangulate_keyline_pairs_*; keyline_pair_kernels.hip)
namespace {
constexpr int kKeylinePairCap = 8192;   // the matchers' envelope; the resolve kernel's two LDS arrays stay under 48 KB

plp_status median_depth_check(plp_matcher* c, const plp_median_depth_args* a) {
    if (!c || !a) return set_error(PLP_ERR_INVALID_ARG, "NULL argument");
    if (a->F <= 0 || a->m_cap < 0) return set_error(PLP_ERR_INVALID_ARG, "F must be positive, m_cap non-negative");
    if (!a->pose || !a->out_median || !a->out_count) return set_error(PLP_ERR_INVALID_ARG, "pose, out_median, out_count are required");
    if (a->m_cap > 0 && !a->pos_w) return set_error(PLP_ERR_INVALID_ARG, "pos_w is required");
    if (a->m_cap > kKeylinePairCap) return set_error(PLP_ERR_UNSUPPORTED, "m_cap above 8192");
    return PLP_OK;
}

MedianDepthArgs median_depth_args(const plp_median_depth_args* a) {
    MedianDepthArgs A{};
    A.m_cap = a->m_cap; A.abs_flag = a->abs_flag ? 1 : 0;
    A.pose = a->pose; A.pos_w = a->pos_w; A.valid = a->m_cap ? a->valid : nullptr; A.counts = a->m_cap ? a->counts : nullptr;
    A.median = a->out_median; A.count = a->out_count;
    return A;
}

bool keyline_pairs_empty(const plp_keyline_pairs_args* a) { return a->cap == 0 || a->P == 0 || a->G == 0; }

plp_status keyline_pairs_check(plp_matcher* c, const plp_keyline_pairs_args* a) {
    if (!c || !a) return set_error(PLP_ERR_INVALID_ARG, "NULL argument");
    if (plp_status s = check_camera_model(&a->camera, true)) return s;
    if (a->camera.model != PLP_CAMERA_PERSPECTIVE)
        return set_error(PLP_ERR_UNSUPPORTED, "the line triangulator needs the perspective camera (two_view_triangulator_line.cc:43)");
    if (a->setup_type < 0 || a->setup_type > 2) return set_error(PLP_ERR_INVALID_ARG, "setup_type must be 0, 1 or 2");
    if (a->num_levels < 1 || a->num_levels > 16) return set_error(PLP_ERR_INVALID_ARG, "num_levels must be 1 .. 16");
    if (a->F <= 0 || a->cap < 0 || a->kp_cap < 0 || a->P < 0 || a->G < 0)
        return set_error(PLP_ERR_INVALID_ARG, "F must be positive, cap, kp_cap, P and G non-negative");
    if (!a->scale_factors || !a->level_sigma_sq) return set_error(PLP_ERR_INVALID_ARG, "scale_factors and level_sigma_sq are required");
    if (a->cap > kKeylinePairCap) return set_error(PLP_ERR_UNSUPPORTED, "cap above 8192");
    if (keyline_pairs_empty(a)) return PLP_OK;
    if ((int64_t)a->P * a->cap > ((int64_t)1 << 31)) return set_error(PLP_ERR_UNSUPPORTED, "P x cap above 2^31");
    if (!a->keylines || !a->line_functions || !a->kl_x_right || !a->pose || !a->median_depth || !a->occupied || !a->pairs || !a->group_offsets ||
        !a->train_idx || !a->dist)
        return set_error(PLP_ERR_INVALID_ARG, "keylines, line_functions, kl_x_right, pose, median_depth, occupied, pairs, group_offsets, train_idx, dist are required");
    if (!a->out_match || !a->out_pos_w || !a->out_status || !a->out_occupied_cur)
        return set_error(PLP_ERR_INVALID_ARG, "out_match, out_pos_w, out_status, out_occupied_cur are required");
    if (a->kp_cap > 0 && !a->kp_depths) return set_error(PLP_ERR_INVALID_ARG, "kp_depths is required when kp_cap > 0");
    if (a->setup_type != 0 && !a->lines_3d) return set_error(PLP_ERR_INVALID_ARG, "lines_3d is required for a stereo or RGB-D setup");
    return PLP_OK;
}

plp_status check_pairs_in_table(const int32_t* pairs, int P, int F) {
    for (int p = 0; p < P; ++p)
        for (int k = 0; k < 2; ++k)
            if (pairs[2 * p + k] < 0 || pairs[2 * p + k] >= F) return set_error(PLP_ERR_INVALID_ARG, "a pair names a key frame outside the table");
    return PLP_OK;
}

// the preconditions of the _device path, checked where the lists are host memory
plp_status keyline_pairs_check_groups(const plp_keyline_pairs_args* a) {
    int prev = 0;
    for (int g = 0; g <= a->G; ++g) {
        const int o = a->group_offsets[g];
        if (o < prev || o > a->P) return set_error(PLP_ERR_INVALID_ARG, "group_offsets must be non-decreasing inside [0, P]");
        prev = o;
    }
    PLP_TRY(check_pairs_in_table(a->pairs, a->P, a->F));
    std::vector<uint8_t> seen((size_t)a->F);
    for (int g = 0; g < a->G; ++g) {
        const int b = a->group_offsets[g], e = a->group_offsets[g + 1];
        for (int p = b; p < e; ++p) {
            const int f1 = a->pairs[2 * p], f2 = a->pairs[2 * p + 1];
            if (f1 != a->pairs[2 * b]) return set_error(PLP_ERR_INVALID_ARG, "the pairs of a group must share kf1");
            if (f2 == f1 || seen[f2]) return set_error(PLP_ERR_INVALID_ARG, "the pairs of a group must have pairwise distinct kf2 != kf1");
            seen[f2] = 1;
        }
        for (int p = b; p < e; ++p) seen[a->pairs[2 * p + 1]] = 0;
    }
    return PLP_OK;
}

KeylinePairArgs keyline_pairs_args(const plp_keyline_pairs_args* a) {
    KeylinePairArgs A{};
    const plp_camera_model& cm = a->camera;
    A.fx = cm.fx; A.fy = cm.fy; A.cx = cm.cx; A.cy = cm.cy;
    A.half_baseline = a->true_baseline / 2.0;
    A.setup_type = a->setup_type; A.num_levels = a->num_levels; A.skip_occupied = a->skip_occupied ? 1 : 0;
    A.F = a->F; A.cap = a->cap; A.kp_cap = a->kp_cap; A.P = a->P; A.G = a->G;
    A.cos_thr = (float)std::cos(a->rays_parallax_deg_thr * M_PI / 180.0);   // two_view_triangulator_line.cc:41 into the float of .h:112
    A.dist_thr = a->dist_thr; A.endpoint_thr = a->endpoint_thr; A.angle_thr = a->angle_thr;
    A.ratio_factor = 2.0f * a->scale_factor;
    fill_levels(A.scale_factors, a->scale_factors, a->num_levels);
    fill_levels(A.level_sigma_sq, a->level_sigma_sq, a->num_levels);
    A.kl = a->keylines; A.counts = a->counts; A.line_fn = a->line_functions; A.x_right = a->kl_x_right;
    A.kp_depths = a->kp_cap ? a->kp_depths : nullptr; A.kp_counts = a->kp_cap ? a->kp_counts : nullptr;
    A.pose = a->pose; A.median = a->median_depth; A.lines_3d = a->setup_type != 0 ? a->lines_3d : nullptr; A.occupied = a->occupied;
    A.pairs = a->pairs; A.group_offsets = a->group_offsets; A.train_idx = a->train_idx; A.dist = a->dist;
    A.out_match = a->out_match; A.out_pos_w = a->out_pos_w; A.out_status = a->out_status; A.out_occ_cur = a->out_occupied_cur;
    return A;
}

extern "C++" auto median_depth_plan(int F_) {
    return [=](auto& r, plp_matcher*, MedianDepthArgs& A) {
        const size_t F = (size_t)F_, M = (size_t)A.m_cap;
        r.in(A.pose, F * 15); r.in(A.pos_w, F * M * 3); r.in(A.valid, F * M); r.in(A.counts, F); r.out(A.median, F); r.out(A.count, F);
    };
}
extern "C++" template <class R> void keyline_pairs_plan(R& r, plp_matcher*, KeylinePairArgs& A) {
    const size_t F = (size_t)A.F, M = (size_t)A.cap, K = (size_t)A.kp_cap, P = (size_t)A.P, G = (size_t)A.G;
    r.in(A.kl, F * M); r.in(A.counts, F); r.in(A.line_fn, F * M * 3); r.in(A.x_right, F * M * 2); r.in(A.kp_depths, F * K); r.in(A.kp_counts, F);
    r.in(A.pose, F * 15); r.in(A.median, F); r.in(A.lines_3d, F * M * 6); r.in(A.occupied, F * M); r.in(A.pairs, P * 2); r.in(A.group_offsets, G + 1);
    r.in(A.train_idx, P * M); r.in(A.dist, P * M);
    r.out(A.out_match, P * M); r.out(A.out_pos_w, P * M * 6); r.out(A.out_status, P * M); r.out(A.out_occ_cur, G * M);
}
}  // namespace

plp_status plp_median_depth_device(plp_matcher* c, const plp_median_depth_args* a, void* hip_stream) {
    if (plp_status s = median_depth_check(c, a)) return s;
    return device_call(c, hip_stream, median_depth_args(a), median_depth_plan(a->F), run_of(launch_median_depth, a->F));
}

plp_status plp_median_depth_host(plp_matcher* c, const plp_median_depth_args* a) {
    if (plp_status s = median_depth_check(c, a)) return s;
    return host_call(c, median_depth_args(a), median_depth_plan(a->F), run_of(launch_median_depth, a->F));
}

plp_status plp_triangulate_keyline_pairs_device(plp_matcher* c, const plp_keyline_pairs_args* a, void* hip_stream) {
    if (plp_status s = keyline_pairs_check(c, a)) return s;
    if (keyline_pairs_empty(a)) return PLP_OK;
    return device_call(c, hip_stream, keyline_pairs_args(a), keyline_pairs_plan<DeviceRooms>, launch_keyline_pairs);
}

plp_status plp_triangulate_keyline_pairs_host(plp_matcher* c, const plp_keyline_pairs_args* a) {
    if (plp_status s = keyline_pairs_check(c, a)) return s;
    if (keyline_pairs_empty(a)) return PLP_OK;
    if (plp_status s = keyline_pairs_check_groups(a)) return s;
    return host_call(c, keyline_pairs_args(a), keyline_pairs_plan<Stage>, launch_keyline_pairs);
}

// ---- key-frame pair point triangulation (include/plp_front.h: plp_keyframe_pair_geometry_*, plp_triangulate_keypoint_pairs_*; keypoint_pair_kernels.hip)
namespace {
plp_status pair_geometry_check(plp_matcher* c, const plp_keyframe_pair_geometry_args* a) {
    if (!c || !a) return set_error(PLP_ERR_INVALID_ARG, "NULL argument");
    if (plp_status s = check_camera_model(&a->camera, false)) return s;
    if (a->setup_type < 0 || a->setup_type > 2) return set_error(PLP_ERR_INVALID_ARG, "setup_type must be 0, 1 or 2");
    if (a->F <= 0 || a->P < 0) return set_error(PLP_ERR_INVALID_ARG, "F must be positive, P non-negative");
    if (a->P == 0) return PLP_OK;
    if (!a->pose || !a->pairs || !a->out_skip || !a->out_epipolar || !a->out_baseline)
        return set_error(PLP_ERR_INVALID_ARG, "pose, pairs, out_skip, out_epipolar, out_baseline are required");
    if (a->setup_type == 0 && !a->median_depth) return set_error(PLP_ERR_INVALID_ARG, "median_depth is required for a monocular setup");
    return PLP_OK;
}

PairGeometryArgs pair_geometry_args(const plp_keyframe_pair_geometry_args* a) {
    PairGeometryArgs A{};
    A.model = a->camera.model; A.setup_type = a->setup_type; A.F = a->F; A.P = a->P;
    A.true_baseline = a->true_baseline;
    A.pose = a->pose; A.median = a->setup_type == 0 ? a->median_depth : nullptr; A.pairs = a->pairs;
    A.out_skip = a->out_skip; A.out_epipolar = a->out_epipolar; A.out_baseline = a->out_baseline;
    return A;
}

bool keypoint_pairs_empty(const plp_keypoint_pairs_args* a) { return a->cap == 0 || a->P == 0; }

plp_status keypoint_pairs_check(plp_matcher* c, const plp_keypoint_pairs_args* a) {
    if (!c || !a) return set_error(PLP_ERR_INVALID_ARG, "NULL argument");
    if (plp_status s = check_camera_model(&a->camera, false)) return s;
    if (a->setup_type < 0 || a->setup_type > 2) return set_error(PLP_ERR_INVALID_ARG, "setup_type must be 0, 1 or 2");
    if (a->setup_type != 0 && a->camera.model == PLP_CAMERA_EQUIRECTANGULAR)
        return set_error(PLP_ERR_UNSUPPORTED, "stereo or RGB-D with the equirectangular camera is not implemented (keyframe.cc:637)");
    if (a->num_levels < 1 || a->num_levels > 16) return set_error(PLP_ERR_INVALID_ARG, "num_levels must be 1 .. 16");
    if (a->F <= 0 || a->cap < 0 || a->m_cap <= 0 || a->P < 0) return set_error(PLP_ERR_INVALID_ARG, "F and m_cap must be positive, cap and P non-negative");
    if (!a->scale_factors || !a->level_sigma_sq) return set_error(PLP_ERR_INVALID_ARG, "scale_factors and level_sigma_sq are required");
    if (a->cap > kKeylinePairCap) return set_error(PLP_ERR_UNSUPPORTED, "cap above 8192");
    if (keypoint_pairs_empty(a)) return PLP_OK;
    if ((int64_t)a->P * std::max(a->cap, a->m_cap) > ((int64_t)1 << 31)) return set_error(PLP_ERR_UNSUPPORTED, "P x max(cap, m_cap) above 2^31");
    if (!a->keypts || !a->bearings || !a->pose || !a->pairs || !a->match_q) return set_error(PLP_ERR_INVALID_ARG, "keypts, bearings, pose, pairs, match_q are required");
    if (!a->out_idx_1 || !a->out_pos_w || !a->out_status) return set_error(PLP_ERR_INVALID_ARG, "out_idx_1, out_pos_w, out_status are required");
    if (a->setup_type != 0 && (!a->x_right || !a->depths)) return set_error(PLP_ERR_INVALID_ARG, "x_right and depths are required for a stereo or RGB-D setup");
    return PLP_OK;
}

KeypointPairArgs keypoint_pairs_args(const plp_keypoint_pairs_args* a) {
    KeypointPairArgs A{};
    const plp_camera_model& cm = a->camera;
    set_camera(A, cm);
    if (cm.model != PLP_CAMERA_EQUIRECTANGULAR) { A.fx_inv = 1.0 / cm.fx; A.fy_inv = 1.0 / cm.fy; }
    A.half_baseline = a->true_baseline / 2.0;
    A.setup_type = a->setup_type; A.num_levels = a->num_levels;
    A.F = a->F; A.cap = a->cap; A.m_cap = a->m_cap; A.P = a->P;
    A.cos_thr = (float)std::cos(a->rays_parallax_deg_thr * M_PI / 180.0);   // two_view_triangulator.cc:42 into the float of .h:110
    A.ratio_factor = 2.0f * a->scale_factor;
    fill_levels(A.scale_factors, a->scale_factors, a->num_levels);
    fill_levels(A.level_sigma_sq, a->level_sigma_sq, a->num_levels);
    const bool stereo = a->setup_type != 0;
    A.kps = a->keypts; A.bearings = a->bearings; A.x_right = stereo ? a->x_right : nullptr; A.depths = stereo ? a->depths : nullptr;
    A.counts = a->counts; A.pose = a->pose; A.pairs = a->pairs; A.match_q = a->match_q; A.q_feature = a->q_feature; A.pair_skip = a->pair_skip;
    A.out_idx_1 = a->out_idx_1; A.out_pos_w = a->out_pos_w; A.out_status = a->out_status; A.occ1 = a->occupied_1_io; A.occ2 = a->occupied_2_io;
    return A;
}

extern "C++" template <class R> void pair_geometry_plan(R& r, plp_matcher*, PairGeometryArgs& A) {
    const size_t F = (size_t)A.F, P = (size_t)A.P;
    r.in(A.pose, F * 15); r.in(A.median, F); r.in(A.pairs, P * 2); r.out(A.out_skip, P); r.out(A.out_epipolar, P * 12); r.out(A.out_baseline, P);
}
extern "C++" template <class R> void keypoint_pairs_plan(R& r, plp_matcher*, KeypointPairArgs& A) {
    const size_t F = (size_t)A.F, M = (size_t)A.cap, Q = (size_t)A.m_cap, P = (size_t)A.P;
    r.in(A.kps, F * M); r.in(A.bearings, F * M * 3); r.in(A.x_right, F * M); r.in(A.depths, F * M); r.in(A.counts, F); r.in(A.pose, F * 15);
    r.in(A.pairs, P * 2); r.in(A.match_q, P * M); r.in(A.q_feature, P * Q); r.in(A.pair_skip, P);
    r.out(A.out_idx_1, P * M); r.out(A.out_pos_w, P * M * 3); r.out(A.out_status, P * M); r.out(A.occ1, P * M); r.out(A.occ2, P * M);
}
}  // namespace

plp_status plp_keyframe_pair_geometry_device(plp_matcher* c, const plp_keyframe_pair_geometry_args* a, void* hip_stream) {
    if (plp_status s = pair_geometry_check(c, a)) return s;
    if (a->P == 0) return PLP_OK;
    return device_call(c, hip_stream, pair_geometry_args(a), pair_geometry_plan<DeviceRooms>, launch_pair_geometry);
}

plp_status plp_keyframe_pair_geometry_host(plp_matcher* c, const plp_keyframe_pair_geometry_args* a) {
    if (plp_status s = pair_geometry_check(c, a)) return s;
    if (a->P == 0) return PLP_OK;
    if (plp_status s = check_pairs_in_table(a->pairs, a->P, a->F)) return s;
    return host_call(c, pair_geometry_args(a), pair_geometry_plan<Stage>, launch_pair_geometry);
}

plp_status plp_triangulate_keypoint_pairs_device(plp_matcher* c, const plp_keypoint_pairs_args* a, void* hip_stream) {
    if (plp_status s = keypoint_pairs_check(c, a)) return s;
    if (keypoint_pairs_empty(a)) return PLP_OK;
    return device_call(c, hip_stream, keypoint_pairs_args(a), keypoint_pairs_plan<DeviceRooms>, launch_keypoint_pairs);
}

plp_status plp_triangulate_keypoint_pairs_host(plp_matcher* c, const plp_keypoint_pairs_args* a) {
    if (plp_status s = keypoint_pairs_check(c, a)) return s;
    if (keypoint_pairs_empty(a)) return PLP_OK;
    if (plp_status s = check_pairs_in_table(a->pairs, a->P, a->F)) return s;
    return host_call(c, keypoint_pairs_args(a), keypoint_pairs_plan<Stage>, launch_keypoint_pairs);
}

// ---- landmark normals and valid distance ranges (include/plp_front.h: plp_landmark[_line]_geometry_*; landmark_geometry_kernels.hip)
namespace {
plp_status landmark_geometry_check(const plp_landmark_geometry_args* a, bool lines) {
    if (!a) return set_error(PLP_ERR_INVALID_ARG, "NULL argument");
    if (a->F <= 0 || a->cap < 0 || a->L < 0) return set_error(PLP_ERR_INVALID_ARG, "F must be positive, cap and L non-negative");
    if (a->num_levels < 1 || a->num_levels > 16 || !a->scale_factors) return set_error(PLP_ERR_INVALID_ARG, "num_levels must be 1 .. 16, scale_factors is required");
    if (lines && (a->num_levels_lsd < 1 || a->num_levels_lsd > 16 || a->num_levels_lsd > a->num_levels || !a->scale_factors_lsd))
        return set_error(PLP_ERR_INVALID_ARG, "num_levels_lsd must be 1 .. min(16, num_levels), scale_factors_lsd is required");
    if (a->L == 0) return PLP_OK;
    if (!a->pose || !a->pos_w || !a->ref_kf || !a->obs_offsets || !a->obs_kf || !a->obs_idx)
        return set_error(PLP_ERR_INVALID_ARG, "pose, pos_w, ref_kf, obs_offsets, obs_kf, obs_idx are required");
    if (!a->out_min_valid_dist || !a->out_max_valid_dist || !a->out_status || (!lines && !a->out_mean_normal))
        return set_error(PLP_ERR_INVALID_ARG, "out_min_valid_dist, out_max_valid_dist, out_status (points: out_mean_normal) are required");
    if (a->cap > 0 && !(lines ? (const void*)a->keylines : (const void*)a->keypts)) return set_error(PLP_ERR_INVALID_ARG, "keypts (lines: keylines) is required");
    return PLP_OK;
}

// the host entries' view of the lists (HOST pointers)
plp_status landmark_geometry_check_offsets(const plp_landmark_geometry_args* a) {
    if (a->obs_offsets[0] != 0) return set_error(PLP_ERR_INVALID_ARG, "obs_offsets must start at 0");
    for (int l = 0; l < a->L; ++l)
        if (a->obs_offsets[l + 1] < a->obs_offsets[l]) return set_error(PLP_ERR_INVALID_ARG, "obs_offsets must not decrease");
    if (a->obs_offsets[a->L] > INT32_MAX - 256) return set_error(PLP_ERR_UNSUPPORTED, "more than 2^31 - 257 observations");
    return PLP_OK;
}

LandmarkGeometryArgs landmark_geometry_args(const plp_landmark_geometry_args* a, bool lines) {
    LandmarkGeometryArgs A{};
    A.F = a->F; A.cap = a->cap; A.L = a->L; A.num_levels = a->num_levels; A.num_levels_lsd = lines ? a->num_levels_lsd : 1;
    fill_levels(A.scale_factors, a->scale_factors, a->num_levels);
    fill_levels(A.scale_factors_lsd, lines ? a->scale_factors_lsd : nullptr, A.num_levels_lsd);
    A.pose = a->pose; A.counts = a->counts; A.kps = lines ? nullptr : a->keypts; A.kl = lines ? a->keylines : nullptr;
    A.pos_w = a->pos_w; A.ref_kf = a->ref_kf; A.skip = a->skip; A.obs_offsets = a->obs_offsets; A.obs_kf = a->obs_kf; A.obs_idx = a->obs_idx;
    A.normal = lines ? nullptr : a->out_mean_normal; A.min_dist = a->out_min_valid_dist; A.max_dist = a->out_max_valid_dist; A.status = a->out_status;
    return A;
}

extern "C++" auto landmark_geometry_plan(bool lines) {
    return [=](auto& r, plp_matcher*, LandmarkGeometryArgs& A) {
        const size_t F = (size_t)A.F, M = (size_t)A.cap, L = (size_t)A.L, T = list_end(r, A.obs_offsets, A.L);
        r.in(A.pose, F * 15); r.in(A.counts, F); r.in(A.kps, F * M); r.in(A.kl, F * M); r.in(A.pos_w, L * (lines ? 6 : 3)); r.in(A.ref_kf, L); r.in(A.skip, L);
        r.in(A.obs_offsets, L + 1); r.in(A.obs_kf, T); r.in(A.obs_idx, T);
        r.out(A.normal, L * 3); r.out(A.min_dist, L); r.out(A.max_dist, L); r.out(A.status, L);
    };
}

plp_status landmark_geometry_device(plp_matcher* c, const plp_landmark_geometry_args* a, void* hip_stream, bool lines) {
    if (!c) return set_error(PLP_ERR_INVALID_ARG, "ctx is NULL");
    if (plp_status s = landmark_geometry_check(a, lines)) return s;
    if (a->L == 0) return PLP_OK;
    return device_call(c, hip_stream, landmark_geometry_args(a, lines), landmark_geometry_plan(lines),
                       lines ? launch_landmark_geometry_lines : launch_landmark_geometry_points);
}

plp_status landmark_geometry_host(plp_matcher* c, const plp_landmark_geometry_args* a, bool lines) {
    if (!c) return set_error(PLP_ERR_INVALID_ARG, "ctx is NULL");
    if (plp_status s = landmark_geometry_check(a, lines)) return s;
    if (a->L == 0) return PLP_OK;
    if (plp_status s = landmark_geometry_check_offsets(a)) return s;
    return host_call(c, landmark_geometry_args(a, lines), landmark_geometry_plan(lines),
                     lines ? launch_landmark_geometry_lines : launch_landmark_geometry_points);
}
}  // namespace

plp_status plp_landmark_geometry_device(plp_matcher* c, const plp_landmark_geometry_args* a, void* hip_stream) {
    return landmark_geometry_device(c, a, hip_stream, false);
}
plp_status plp_landmark_geometry_host(plp_matcher* c, const plp_landmark_geometry_args* a) { return landmark_geometry_host(c, a, false); }
plp_status plp_landmark_line_geometry_device(plp_matcher* c, const plp_landmark_geometry_args* a, void* hip_stream) {
    return landmark_geometry_device(c, a, hip_stream, true);
}
plp_status plp_landmark_line_geometry_host(plp_matcher* c, const plp_landmark_geometry_args* a) { return landmark_geometry_host(c, a, true); }

// the host build of landmark_geometry.hpp: the loops of the two kernels, one landmark after the other (no HIP call)
int32_t plp_model_landmark_geometry_host(const plp_landmark_geometry_args* a, int32_t lines) {
    if (landmark_geometry_check(a, lines != 0) != PLP_OK) return -1;
    if (a->L == 0) return 0;
    if (landmark_geometry_check_offsets(a) != PLP_OK) return -1;
    const LandmarkGeometryArgs A = landmark_geometry_args(a, lines != 0);
    for (int l = 0; l < A.L; ++l) {
        if (lines) { A.status[l] = lg_line(A, l); continue; }
        const int beg = A.obs_offsets[l], end = A.obs_offsets[l + 1], ref = A.ref_kf[l];
        const double* p = A.pos_w + (size_t)3 * l;
        double sx = 0.0, sy = 0.0, sz = 0.0;
        int found = -1;
        bool bad = false;
        for (int o = beg; o < end; ++o) {
            const int kf = A.obs_kf[o];
            if ((unsigned)kf >= (unsigned)A.F) { bad = true; continue; }
            const double* cc = A.pose + (size_t)15 * kf + 12;
            const LgVec3 u = lg_normalized(p[0] - cc[0], p[1] - cc[1], p[2] - cc[2]);
            sx = sx + u.x; sy = sy + u.y; sz = sz + u.z;
            if (found < 0 && kf == ref) found = o;
        }
        A.status[l] = lg_point_finish(A, l, end - beg, sx, sy, sz, found, bad);
    }
    return A.L;
}

// ---- place recognition (include/plp_front.h: plp_bow_query_*, plp_bow_score_pairs_*; bow_database_kernels.hip)
namespace {
plp_status bow_scoring_check(int32_t scoring) {
    if (scoring < 0 || scoring > 5) return set_error(PLP_ERR_INVALID_ARG, "scoring must be a DBoW2 ScoringType, 0 .. 5");
    if (scoring != 0) return set_error(PLP_ERR_UNSUPPORTED, "only L1_NORM scoring (0) is implemented");
    return PLP_OK;
}

plp_status bow_query_check(const plp_bow_query_args* a) {
    if (!a) return set_error(PLP_ERR_INVALID_ARG, "NULL argument");
    if (a->N < 0 || a->Q < 0) return set_error(PLP_ERR_INVALID_ARG, "N and Q must not be negative");
    if (a->stride < 1 || a->stride > 8192 || a->q_stride < 1 || a->q_stride > 8192) return set_error(PLP_ERR_INVALID_ARG, "stride and q_stride must be 1 .. 8192");
    if (a->covis_cap < 0 || a->covis_cap > 16) return set_error(PLP_ERR_INVALID_ARG, "covis_cap must be 0 .. 16");
    if (a->n_words == 0) return set_error(PLP_ERR_INVALID_ARG, "n_words must be positive");
    if (plp_status s = bow_scoring_check(a->scoring)) return s;
    if (a->Q > 65535) return set_error(PLP_ERR_UNSUPPORTED, "more than 65535 queries in one call");
    if (a->N > 0 && (!a->db_word || !a->db_value || !a->db_n)) return set_error(PLP_ERR_INVALID_ARG, "db_word, db_value, db_n are required");
    if (a->Q > 0 && (!a->q_word || !a->q_value || !a->q_n)) return set_error(PLP_ERR_INVALID_ARG, "q_word, q_value, q_n are required");
    if (a->N > 0 && a->covis_cap > 0 && a->n_covis && !a->covis) return set_error(PLP_ERR_INVALID_ARG, "covis is required beside n_covis");
    return PLP_OK;
}

BowQueryArgs bow_query_args(const plp_bow_query_args* a) {
    BowQueryArgs A{};
    A.n_words = a->n_words; A.N = a->N; A.stride = a->stride; A.Q = a->Q; A.q_stride = a->q_stride; A.covis_cap = a->covis_cap;
    A.db_word = a->db_word; A.db_value = a->db_value; A.db_n = a->db_n; A.db_alive = a->db_alive;
    A.q_word = a->q_word; A.q_value = a->q_value; A.q_n = a->q_n; A.reject = a->reject; A.min_score = a->min_score;
    A.covis = a->covis; A.n_covis = a->covis_cap > 0 ? a->n_covis : nullptr;
    A.common = a->out_common; A.score = a->out_score; A.total = a->out_total; A.best_kf = a->out_best_kf; A.final_mask = a->out_final;
    A.max_common = a->out_max_common; A.n_final = a->out_n_final; A.best_total = a->out_best_total; A.status = a->out_status;
    return A;
}

plp_status bow_pairs_check(const plp_bow_score_pairs_args* a) {
    if (!a) return set_error(PLP_ERR_INVALID_ARG, "NULL argument");
    if (a->NA < 0 || a->NB < 0 || a->P < 0) return set_error(PLP_ERR_INVALID_ARG, "NA, NB and P must not be negative");
    if (a->stride_a < 1 || a->stride_a > 8192 || a->stride_b < 1 || a->stride_b > 8192) return set_error(PLP_ERR_INVALID_ARG, "stride_a and stride_b must be 1 .. 8192");
    if (plp_status s = bow_scoring_check(a->scoring)) return s;
    if (a->NA > 0 && (!a->a_word || !a->a_value || !a->a_n)) return set_error(PLP_ERR_INVALID_ARG, "a_word, a_value, a_n are required");
    if (a->NB > 0 && (!a->b_word || !a->b_value || !a->b_n)) return set_error(PLP_ERR_INVALID_ARG, "b_word, b_value, b_n are required");
    if (a->P > 0 && (!a->a_row || !a->b_row || !a->out_score)) return set_error(PLP_ERR_INVALID_ARG, "a_row, b_row, out_score are required");
    return PLP_OK;
}

BowPairsArgs bow_pairs_args(const plp_bow_score_pairs_args* a) {
    BowPairsArgs A{};
    A.NA = a->NA; A.stride_a = a->stride_a; A.NB = a->NB; A.stride_b = a->stride_b; A.P = a->P;
    A.a_word = a->a_word; A.a_value = a->a_value; A.a_n = a->a_n; A.b_word = a->b_word; A.b_value = a->b_value; A.b_n = a->b_n;
    A.a_row = a->a_row; A.b_row = a->b_row; A.out_score = a->out_score;
    return A;
}

extern "C++" template <class R> void bow_pairs_plan(R& r, plp_matcher*, BowPairsArgs& A) {
    const size_t NA = (size_t)A.NA, NB = (size_t)A.NB, P = (size_t)A.P;
    r.in(A.a_word, NA * A.stride_a); r.in(A.a_value, NA * A.stride_a); r.in(A.a_n, NA);
    r.in(A.b_word, NB * A.stride_b); r.in(A.b_value, NB * A.stride_b); r.in(A.b_n, NB);
    r.in(A.a_row, P); r.in(A.b_row, P);
    r.out(A.out_score, P, false);
}
}  // namespace

plp_status plp_bow_query_device(plp_matcher* c, const plp_bow_query_args* a, void* hip_stream) {
    if (!c) return set_error(PLP_ERR_INVALID_ARG, "ctx is NULL");
    if (plp_status s = bow_query_check(a)) return s;
    if (a->Q == 0) return PLP_OK;
    std::lock_guard<std::mutex> lk(c->mu);
    PLP_HIP(hipSetDevice(c->device));
    BowQueryArgs A = bow_query_args(a);
    // the per-row arrays the kernels hand to each other live in the context where the caller passed NULL
    const size_t QN = (size_t)a->Q * (size_t)a->N, al = 256;
    const size_t b4 = (QN * 4 + al - 1) / al * al, b1 = (QN + al - 1) / al * al, bq = ((size_t)a->Q * 4 + al - 1) / al * al;
    size_t need = 0;
    if (!A.common) need += b4;
    if (!A.score) need += b4;
    if (!A.total) need += b4;
    if (!A.best_kf) need += b4;
    if (!A.final_mask) need += b1;
    if (!A.max_common) need += bq;
    if (need) {
        PLP_HIP(c->bow_scratch.reserve(need));
        uint8_t* p = static_cast<uint8_t*>(c->bow_scratch.p);
        if (!A.common) { A.common = reinterpret_cast<uint32_t*>(p); p += b4; }
        if (!A.score) { A.score = reinterpret_cast<float*>(p); p += b4; }
        if (!A.total) { A.total = reinterpret_cast<float*>(p); p += b4; }
        if (!A.best_kf) { A.best_kf = reinterpret_cast<int32_t*>(p); p += b4; }
        if (!A.final_mask) { A.final_mask = p; p += b1; }
        if (!A.max_common) { A.max_common = reinterpret_cast<uint32_t*>(p); p += bq; }
    }
    PLP_HIP(launch_bow_query((hipStream_t)hip_stream, A));
    return PLP_OK;
}

plp_status plp_bow_query_host(plp_matcher* c, const plp_bow_query_args* a) {
    if (!c) return set_error(PLP_ERR_INVALID_ARG, "ctx is NULL");
    if (plp_status s = bow_query_check(a)) return s;
    if (a->Q == 0) return PLP_OK;
    const size_t N = (size_t)a->N, Q = (size_t)a->Q, QN = Q * N;
    BowQueryArgs A = bow_query_args(a);
    std::lock_guard<std::mutex> lk(c->mu);
    PLP_HIP(hipSetDevice(c->device));
    Stage s(c->stage, c->stream);
    s.in(A.db_word, N * a->stride); s.in(A.db_value, N * a->stride); s.in(A.db_n, N); s.in(A.db_alive, N);
    s.in(A.q_word, Q * a->q_stride); s.in(A.q_value, Q * a->q_stride); s.in(A.q_n, Q); s.in(A.reject, QN); s.in(A.min_score, Q);
    s.in(A.covis, N * a->covis_cap); s.in(A.n_covis, N);
    // every slot of every output is written: keep = false; an output the caller left out is a device-only region
    if (A.common) s.out(A.common, QN, false); else s.room(A.common, QN);
    if (A.score) s.out(A.score, QN, false); else s.room(A.score, QN);
    if (A.total) s.out(A.total, QN, false); else s.room(A.total, QN);
    if (A.best_kf) s.out(A.best_kf, QN, false); else s.room(A.best_kf, QN);
    if (A.final_mask) s.out(A.final_mask, QN, false); else s.room(A.final_mask, QN);
    if (A.max_common) s.out(A.max_common, Q, false); else s.room(A.max_common, Q);
    s.out(A.n_final, Q, false); s.out(A.best_total, Q, false); s.out(A.status, Q, false);
    PLP_TRY(s.upload());
    PLP_HIP(launch_bow_query(c->stream, A));
    return s.finish();
}

plp_status plp_bow_score_pairs_device(plp_matcher* c, const plp_bow_score_pairs_args* a, void* hip_stream) {
    if (!c) return set_error(PLP_ERR_INVALID_ARG, "ctx is NULL");
    if (plp_status s = bow_pairs_check(a)) return s;
    if (a->P == 0) return PLP_OK;
    return device_call(c, hip_stream, bow_pairs_args(a), bow_pairs_plan<DeviceRooms>, launch_bow_score_pairs);
}

plp_status plp_bow_score_pairs_host(plp_matcher* c, const plp_bow_score_pairs_args* a) {
    if (!c) return set_error(PLP_ERR_INVALID_ARG, "ctx is NULL");
    if (plp_status s = bow_pairs_check(a)) return s;
    if (a->P == 0) return PLP_OK;
    return host_call(c, bow_pairs_args(a), bow_pairs_plan<Stage>, launch_bow_score_pairs);
}

// the host build of bow_score.hpp (no HIP call)
double plp_model_bow_score_host(const uint32_t* wa, const double* va, int32_t na, const uint32_t* wb, const double* vb, int32_t nb) {
    if (na < 0 || nb < 0 || (na > 0 && (!wa || !va)) || (nb > 0 && (!wb || !vb))) return -1.0;
    return bow_l1_score(wa, va, na, wb, vb, nb);
}

plp_status plp_convert_to_grayscale_device(plp_matcher* c, const uint8_t* d_src, int32_t rows, int32_t cols, size_t src_step,
                                           size_t src_frame_stride, int32_t channels, int32_t color_order, int32_t B, uint8_t* d_gray,
                                           size_t gray_step, size_t gray_frame_stride, void* hip_stream) {
    if (!c || !d_src || !d_gray) return set_error(PLP_ERR_INVALID_ARG, "NULL argument");
    if (rows <= 0 || cols <= 0 || B <= 0 || (channels != 3 && channels != 4) || (color_order != 0 && color_order != 1) ||
        src_step < (size_t)cols * channels || gray_step < (size_t)cols) return set_error(PLP_ERR_INVALID_ARG, "bad geometry");
    return device_call(c, hip_stream, NoArgs{}, NoArrays{}, [=](hipStream_t st, NoArgs&) {
        launch_to_gray(st, d_src, rows, cols, src_step, src_frame_stride, channels, color_order, B, d_gray, gray_step, gray_frame_stride);
        return hipGetLastError();
    });
}

plp_status plp_convert_to_true_depth_device(plp_matcher* c, const void* d_src, int32_t src_is_u16, int32_t rows, int32_t cols, size_t src_step,
                                            size_t src_frame_stride, double depthmap_factor, int32_t B, float* d_dst, size_t dst_step,
                                            size_t dst_frame_stride, void* hip_stream) {
    if (!c || !d_src || !d_dst) return set_error(PLP_ERR_INVALID_ARG, "NULL argument");
    if (rows <= 0 || cols <= 0 || B <= 0 || src_step < (size_t)cols * (src_is_u16 ? 2 : 4) || dst_step < (size_t)cols * 4)
        return set_error(PLP_ERR_INVALID_ARG, "bad geometry");
    return device_call(c, hip_stream, NoArgs{}, NoArrays{}, [=](hipStream_t st, NoArgs&) {
        launch_to_depth(st, d_src, src_is_u16 != 0, rows, cols, src_step, src_frame_stride, (float)(1.0 / depthmap_factor), B, d_dst, dst_step, dst_frame_stride);
        return hipGetLastError();
    });
}

static plp_status rectify_map_impl(plp_matcher* c, const double* K, const double* D, int32_t n_dist, const double* R, const plp_camera* rect_cam,
                                   int32_t rows, int32_t cols, float* d_map_x, float* d_map_y, size_t map_step, void* hip_stream, bool fisheye) {
    if (!c || !K || !R || !rect_cam || !d_map_x || !d_map_y || (n_dist > 0 && !D)) return set_error(PLP_ERR_INVALID_ARG, "NULL argument");
    if (rows <= 0 || cols <= 0 || map_step < (size_t)cols * 4 || (map_step & 3)) return set_error(PLP_ERR_INVALID_ARG, "bad geometry");
    if (fisheye ? n_dist != 4 : (n_dist != 0 && n_dist != 4 && n_dist != 5 && n_dist != 8 && n_dist != 12))
        return set_error(PLP_ERR_INVALID_ARG, fisheye ? "the fisheye model takes 4 distortion coefficients" : "distortion vector must have 0, 4, 5, 8 or 12 entries");
    RectifyArgs A{};
    // iR = (K_rect * R)^-1, K_rect float-rounded; closed-form 3x3 inverse in the order cv::Matx evaluates it
    const double Ar[9] = {(double)(float)rect_cam->fx, 0, (double)(float)rect_cam->cx, 0, (double)(float)rect_cam->fy, (double)(float)rect_cam->cy, 0, 0, 1};
    double m[9];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            double s = 0;
            for (int k = 0; k < 3; ++k) s += Ar[i * 3 + k] * R[k * 3 + j];
            m[i * 3 + j] = s;
        }
    double det = m[0] * (m[4] * m[8] - m[7] * m[5]) - m[1] * (m[3] * m[8] - m[6] * m[5]) + m[2] * (m[3] * m[7] - m[6] * m[4]);
    if (det == 0) return set_error(PLP_ERR_INVALID_ARG, "K_rect * R is singular");
    det = 1 / det;
    A.ir[0] = (m[4] * m[8] - m[5] * m[7]) * det; A.ir[1] = (m[2] * m[7] - m[1] * m[8]) * det; A.ir[2] = (m[1] * m[5] - m[2] * m[4]) * det;
    A.ir[3] = (m[5] * m[6] - m[3] * m[8]) * det; A.ir[4] = (m[0] * m[8] - m[2] * m[6]) * det; A.ir[5] = (m[2] * m[3] - m[0] * m[5]) * det;
    A.ir[6] = (m[3] * m[7] - m[4] * m[6]) * det; A.ir[7] = (m[1] * m[6] - m[0] * m[7]) * det; A.ir[8] = (m[0] * m[4] - m[1] * m[3]) * det;
    for (int i = 0; i < n_dist; ++i) A.d[i] = D[i];
    A.fx = K[0]; A.fy = K[4]; A.u0 = K[2]; A.v0 = K[5];
    A.rows = rows; A.cols = cols; A.map_x = d_map_x; A.map_y = d_map_y; A.map_step = map_step;
    return device_call(c, hip_stream, A, NoArrays{}, [=](hipStream_t st, RectifyArgs& A) { launch_rectify_map(st, A, fisheye); return hipGetLastError(); });
}

plp_status plp_rectify_map_device(plp_matcher* c, const double* K, const double* D, int32_t n_dist, const double* R, const plp_camera* rect_cam,
                                  int32_t rows, int32_t cols, float* d_map_x, float* d_map_y, size_t map_step, void* hip_stream) {
    return rectify_map_impl(c, K, D, n_dist, R, rect_cam, rows, cols, d_map_x, d_map_y, map_step, hip_stream, false);
}

plp_status plp_rectify_map_fisheye_device(plp_matcher* c, const double* K, const double* D4, const double* R, const plp_camera* rect_cam, int32_t rows,
                                          int32_t cols, float* d_map_x, float* d_map_y, size_t map_step, void* hip_stream) {
    return rectify_map_impl(c, K, D4, 4, R, rect_cam, rows, cols, d_map_x, d_map_y, map_step, hip_stream, true);
}

plp_status plp_remap_linear_device(plp_matcher* c, const uint8_t* d_src, int32_t rows, int32_t cols, size_t src_step, size_t src_frame_stride,
                                   const float* d_map_x, const float* d_map_y, size_t map_step, int32_t dst_rows, int32_t dst_cols, int32_t B,
                                   uint8_t* d_dst, size_t dst_step, size_t dst_frame_stride, void* hip_stream) {
    if (!c || !d_src || !d_map_x || !d_map_y || !d_dst) return set_error(PLP_ERR_INVALID_ARG, "NULL argument");
    if (rows <= 0 || cols <= 0 || dst_rows <= 0 || dst_cols <= 0 || B <= 0 || rows > 32767 || cols > 32767 || src_step < (size_t)cols ||
        dst_step < (size_t)dst_cols || map_step < (size_t)dst_cols * 4 || (map_step & 3))
        return set_error(PLP_ERR_INVALID_ARG, "bad geometry");
    return device_call(c, hip_stream, NoArgs{}, NoArrays{}, [=](hipStream_t st, NoArgs&) {
        launch_remap_linear(st, d_src, rows, cols, src_step, src_frame_stride, d_map_x, d_map_y, map_step, dst_rows, dst_cols, B, d_dst, dst_step, dst_frame_stride);
        return hipGetLastError();
    });
}

plp_status plp_color_vote_device(plp_matcher* c, const uint8_t* d_mask, int32_t rows, int32_t cols, size_t mask_step,
                                 size_t mask_frame_stride, const plp_keypoint* d_undist, const uint8_t* d_valid, const int32_t* d_counts,
                                 int32_t cap, int32_t B, int32_t check_3x3_window, int32_t* d_labels, void* hip_stream) {
    if (!c || !d_mask || !d_undist || !d_labels) return set_error(PLP_ERR_INVALID_ARG, "NULL argument");
    if (rows <= 0 || cols <= 0 || cap <= 0 || B <= 0 || mask_step < (size_t)cols * 3) return set_error(PLP_ERR_INVALID_ARG, "bad geometry");
    return device_call(c, hip_stream, NoArgs{}, NoArrays{}, [=](hipStream_t st, NoArgs&) {
        launch_color_vote(st, d_mask, rows, cols, mask_step, mask_frame_stride, d_undist, d_valid, d_counts, cap, B, check_3x3_window != 0, d_labels);
        return hipGetLastError();
    });
}

namespace {
struct LandmarkDescriptorArgs { const uint8_t* descs; const int32_t* offsets; int32_t L; int32_t* best_idx; };
extern "C++" template <class R> void landmark_descriptor_plan(R& r, plp_matcher*, LandmarkDescriptorArgs& A) {   // no row at all: the kernel reads no descriptor
    r.in(A.descs, list_end(r, A.offsets, A.L) * 32); r.in(A.offsets, (size_t)A.L + 1); r.out(A.best_idx, A.L, false);
}
static hipError_t landmark_descriptor_run(hipStream_t st, const LandmarkDescriptorArgs& A) {
    launch_landmark_descriptor(st, A.descs, A.offsets, A.L, A.best_idx);
    return hipGetLastError();
}
}  // namespace

plp_status plp_landmark_descriptor_device(plp_matcher* c, const uint8_t* d_descs, const int32_t* d_offsets, int32_t L, int32_t* d_best_idx,
                                          void* hip_stream) {
    if (!c || !d_offsets || !d_best_idx || L < 0) return set_error(PLP_ERR_INVALID_ARG, "bad argument");
    if (L == 0) return PLP_OK;
    return device_call(c, hip_stream, LandmarkDescriptorArgs{d_descs, d_offsets, L, d_best_idx}, landmark_descriptor_plan<DeviceRooms>, landmark_descriptor_run);
}

plp_status plp_landmark_descriptor_host(plp_matcher* c, const uint8_t* descs, const int32_t* offsets, int32_t L, int32_t* best_idx) {
    if (!c || !offsets || !best_idx || L < 0) return set_error(PLP_ERR_INVALID_ARG, "bad argument");
    if (L == 0) return PLP_OK;
    const int64_t total = offsets[L];
    if (total < 0 || (total > 0 && !descs)) return set_error(PLP_ERR_INVALID_ARG, "bad offsets / descs");
    for (int l = 0; l < L; ++l)
        if (offsets[l + 1] < offsets[l] || offsets[l + 1] - offsets[l] > 1024) return set_error(PLP_ERR_UNSUPPORTED, "offsets must ascend, at most 1024 rows per landmark");
    return host_call(c, LandmarkDescriptorArgs{descs, offsets, L, best_idx}, landmark_descriptor_plan<Stage>, landmark_descriptor_run);
}

plp_status plp_match_debug_plan(const plp_match_args* a, int32_t* out4) {
    if (!a || !out4) return set_error(PLP_ERR_INVALID_ARG, "NULL argument");
    for (int i = 0; i < 4; ++i) out4[i] = 0;
    if (a->mode < PLP_MATCH_MODE_LANDMARKS || a->mode > PLP_MATCH_MODE_TRIANGULATION) return set_error(PLP_ERR_INVALID_ARG, "unknown mode");
    if (a->B <= 0 || a->n_cap < 0 || a->m_cap < 0) return set_error(PLP_ERR_INVALID_ARG, "B must be positive, n_cap and m_cap non-negative");
    if (a->n_cap > 8192) return set_error(PLP_ERR_UNSUPPORTED, "more than 8192 key points per frame");
    if (a->n_cap == 0 || a->m_cap == 0) return PLP_OK;   // an empty side: no kernel runs
    MatchProblem P{};
    P.mode = a->mode; P.n_cap = a->n_cap; P.m_cap = a->m_cap; P.t_x_right = a->t_x_right;
    P.grid_cols = a->grid.cols; P.grid_rows = a->grid.rows;
    P.lds_targets = lds_targets_of(a);
    const MatchPlan pl = plan_match(P, a->B);
    out4[0] = pl.topk; out4[1] = pl.family; out4[2] = pl.qpb; out4[3] = pl.resolve;
    return PLP_OK;
}

plp_status plp_match_debug_counters(plp_matcher* c, int64_t* out4) {
    if (!c || !out4) return set_error(PLP_ERR_INVALID_ARG, "NULL argument");
    std::lock_guard<std::mutex> lk(c->mu);
    PLP_HIP(hipSetDevice(c->device));
    int32_t v[4] = {0, 0, 0, 0};
    if (c->dbg.p) PLP_HIP(hipMemcpy(v, c->dbg.p, 16, hipMemcpyDeviceToHost));
    for (int i = 0; i < 4; ++i) out4[i] = v[i];
    return PLP_OK;
}

plp_status plp_hamming_matrix_device(plp_matcher* c, const uint8_t* d_q, int32_t nq, const uint8_t* d_t, int32_t nt, uint16_t* d_dist,
                                     void* hip_stream) {
    if (!c || !d_q || !d_t || !d_dist) return set_error(PLP_ERR_INVALID_ARG, "NULL argument");
    if (nq <= 0 || nt <= 0) return PLP_OK;
    PLP_HIP(hipSetDevice(c->device));
    launch_hamming_matrix((hipStream_t)hip_stream, d_q, nq, d_t, nt, d_dist);
    PLP_HIP(hipGetLastError());
    return PLP_OK;
}

plp_status plp_hamming_matrix_host(plp_matcher* c, const uint8_t* q, int32_t nq, const uint8_t* t, int32_t nt, uint16_t* dist) {
    if (!c || !q || !t || !dist) return set_error(PLP_ERR_INVALID_ARG, "NULL argument");
    if (nq <= 0 || nt <= 0) return PLP_OK;
    struct { const uint8_t *q, *t; uint16_t* dist; } A{q, t, dist};
    return host_call(
        c, A, [=](Stage& s, plp_matcher*, auto& A) { s.in(A.q, (size_t)nq * 32); s.in(A.t, (size_t)nt * 32); s.out(A.dist, (size_t)nq * nt, false); },
        [=](hipStream_t st, auto& A) { launch_hamming_matrix(st, A.q, nq, A.t, nt, A.dist); return hipGetLastError(); });
}

// Host model of the bin ranking inside the matchers' orientation check (csrc/libstdcxx_sort.hpp), callable without a GPU: the
// indices 0..n-1 (n <= 64) as std::sort orders them by bin size, descending.  depth_limit < 0: the library's own recursion budget.
int32_t plp_model_index_sort_host(const int32_t* sizes, int32_t n, int32_t depth_limit, uint32_t* idx) {
    if (!sizes || !idx || n < 0 || n > 64) return -1;
    int ws[48];
    plp::libstdcxx::index_sort_by_size(sizes, n, idx, ws, depth_limit);
    return n;
}

}  // extern "C"
