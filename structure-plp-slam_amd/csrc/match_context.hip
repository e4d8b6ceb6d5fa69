// Host driver + C ABI of the array-form Hamming matchers (include/plp_front.h).
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
#include "local_ba.hpp"
#include "local_map.hpp"
#include "match_device.hpp"
#include "plp_common.hpp"
#include "pnp.hpp"
#include "pose_opt.hpp"
#include "sim3.hpp"
#include "transform_opt.hpp"

using namespace plp;

struct plp_matcher {
    int device = 0;
    hipStream_t stream = nullptr;
    DevBuf klist, klist2, kcount, claim, full_list, sorted, sorted_xr, row_start, dbg;  // scratch of the device path
    DevBuf stage;                            // one slab for the host-pointer path
    DevBuf bow_scratch;                      // plp_bow_query_device: the per-row arrays the caller did not ask for
    DevBuf sim3_ctx, sim3_hyp;               // plp_sim3_ransac_device: what its launches hand to one another
    DevBuf pnp_ctx, pnp_slot, pnp_hyp, pnp_corr, pnp_pose, pnp_sign;   // plp_pnp_ransac_device: likewise
    DevBuf pose_slot, pose_slot_lines, pose_chi2, pose_n;              // plp_pose_optimize_device: likewise
    DevBuf tf_slot, tf_chi2, tf_n, tf_level, tf_edge;                                   // plp_transform_optimize_device: likewise
    DevBuf la_d, la_i, la_b;                                                            // plp_local_ba_device: likewise
    DevBuf lm_ws;                                                                       // plp_local_map_device: the mark table of a chunk of frames
    HostPinned pin;                          // page-locked staging of host images (post-extract depth)
    std::mutex mu;
};

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

// a kernel-argument table of 16 pyramid levels from the caller's num_levels floats (NULL: none), 1 past them
void fill_levels(float (&dst)[16], const float* src, int num_levels) {
    for (int i = 0; i < 16; ++i) dst[i] = (src && i < num_levels) ? src[i] : 1.0f;
}

// the camera fields reproject<MODEL> (reproject.hpp) reads, which ObserveArgs, ProjectArgs and KeypointPairArgs name alike
template <class Args> void set_camera(Args& A, const plp_camera_model& cm) {
    A.model = cm.model;
    A.fx = cm.fx; A.fy = cm.fy; A.cx = cm.cx; A.cy = cm.cy; A.fxb = cm.focal_x_baseline;
    A.cols_d = (double)(unsigned)cm.cols; A.rows_d = (double)(unsigned)cm.rows;
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
    std::lock_guard<std::mutex> lk(c->mu);
    PLP_HIP(hipSetDevice(c->device));
    const uint8_t *d_q = q, *d_t = t;   // device addresses after upload()
    int32_t *d_train_idx = train_idx, *d_dist = dist;
    Stage s(c->stage, c->stream);
    s.in(d_q, (size_t)nq * 32); s.in(d_t, (size_t)nt * 32); s.out(d_train_idx, nq, false); s.out(d_dist, nq, false);
    PLP_TRY(s.upload());
    static const MihRanks R = mih_ranks();
    launch_lbd_match_1nn(c->stream, d_q, nullptr, nq, d_t, nullptr, nt, R, d_train_idx, d_dist, 1);
    PLP_HIP(hipGetLastError());
    return s.finish();
}

plp_status plp_match_area_host(plp_matcher* c, const plp_keypoint* kps_1, const uint8_t* desc_1, int32_t n1, const plp_keypoint* kps_2,
                               const uint8_t* desc_2, int32_t n2, const plp_match_grid* grid, float* prev_matched_pts, int32_t margin,
                               float lowe_ratio, int32_t check_orientation, int32_t* matched_2_in_1, int32_t* num_matches) {
    if (!c || !grid || !matched_2_in_1 || !num_matches) return set_error(PLP_ERR_INVALID_ARG, "NULL argument");
    *num_matches = 0;
    if (n1 <= 0) return PLP_OK;
    if (!kps_1 || !desc_1 || !prev_matched_pts || n2 < 0 || (n2 > 0 && (!kps_2 || !desc_2)) || n2 > 65535) return set_error(PLP_ERR_INVALID_ARG, "bad argument");
    std::lock_guard<std::mutex> lk(c->mu);
    PLP_HIP(hipSetDevice(c->device));
    AreaArgs A{};
    A.kps1 = kps_1; A.desc1 = desc_1; A.kps2 = kps_2; A.desc2 = desc_2; A.n1 = n1; A.n2 = n2;
    A.grid_min_x = grid->min_x; A.grid_min_y = grid->min_y; A.inv_cell_w = grid->inv_cell_width; A.inv_cell_h = grid->inv_cell_height;
    A.grid_cols = grid->cols; A.grid_rows = grid->rows;
    A.prev_pts = prev_matched_pts; A.margin = (float)margin; A.lowe_ratio = lowe_ratio; A.check_orientation = check_orientation;
    A.matched_2_in_1 = matched_2_in_1; A.num_matches = num_matches;
    Stage s(c->stage, c->stream);   // n2 == 0: the kernel reads no key point of frame 2 and no scratch
    s.in(A.kps1, n1); s.in(A.desc1, (size_t)n1 * 32); s.in(A.kps2, n2); s.in(A.desc2, (size_t)n2 * 32);
    s.out(A.matched_2_in_1, n1, false); s.out(A.prev_pts, (size_t)n1 * 2); s.out(A.num_matches, 1, false); s.room(A.scratch, (size_t)n2 * 2);
    PLP_TRY(s.upload());
    launch_match_area(c->stream, A);
    PLP_HIP(hipGetLastError());
    return s.finish();
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

plp_status post_extract_device(plp_matcher* c, const PostArgs& cam_args, const plp_keypoint* d_kps, const int32_t* d_counts, int32_t cap,
                               int32_t B, const float* d_depth, int32_t rows, int32_t cols, size_t depth_step, size_t depth_frame_stride,
                               plp_keypoint* d_undist, double* d_bearings, float* d_x_right, float* d_depths,
                               const plp_keyline* d_kl, const int32_t* d_kl_counts, int32_t kl_cap, float* d_kl_depths,
                               float* d_kl_x_right, void* hip_stream);
plp_status post_extract_host(plp_matcher* c, const PostArgs& cam_args, const plp_keypoint* kps, int32_t n, const float* depth, int32_t rows,
                             int32_t cols, size_t depth_step, plp_keypoint* undist, double* bearings, float* x_right, float* depths,
                             const plp_keyline* kl, int32_t n_kl, float* kl_depths, float* kl_x_right);
}  // namespace

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
    std::lock_guard<std::mutex> lk(c->mu);
    PLP_HIP(hipSetDevice(c->device));
    PostArgs A = cam_args;
    A.kps = d_kps; A.counts = d_counts; A.cap = d_kps ? cap : 0;
    A.depth = d_depth; A.depth_step = depth_step; A.depth_frame_stride = depth_frame_stride;
    A.undist = d_undist; A.bearings = d_bearings; A.x_right = d_x_right; A.depths = d_depths;
    A.kl = d_kl; A.kl_counts = d_kl_counts; A.kl_cap = d_kl ? kl_cap : 0; A.kl_depths = d_kl_depths; A.kl_x_right = d_kl_x_right;
    launch_post_extract((hipStream_t)hip_stream, A, B);
    PLP_HIP(hipGetLastError());
    return PLP_OK;
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

plp_status observe_device(plp_matcher* c, const plp_observe_args* a, bool lines, void* hip_stream) {
    if (plp_status s = observe_check(c, a, lines)) return s;
    std::lock_guard<std::mutex> lk(c->mu);
    PLP_HIP(hipSetDevice(c->device));
    hipStream_t st = (hipStream_t)hip_stream;
    if (a->m_cap == 0) {   // no landmark slot: the reference's loop does not run
        if (a->out_num_valid) PLP_HIP(hipMemsetAsync(a->out_num_valid, 0, (size_t)a->B * 4, st));
        return PLP_OK;
    }
    const ObserveArgs A = observe_args(a, lines);
    PLP_HIP(lines ? launch_observe_lines(st, A, a->B) : launch_observe_points(st, A, a->B));
    return PLP_OK;
}

// host pointers: every array staged through the context's slab (plp_common.hpp Stage), the device path's kernel, the outputs copied back
plp_status observe_host(plp_matcher* c, const plp_observe_args* a, bool lines) {
    if (plp_status s = observe_check(c, a, lines)) return s;
    const size_t B = (size_t)a->B, M = (size_t)a->m_cap, BM = B * M;
    if (M == 0) {
        if (a->out_num_valid) std::memset(a->out_num_valid, 0, B * 4);
        return PLP_OK;
    }
    ObserveArgs A = observe_args(a, lines);
    std::lock_guard<std::mutex> lk(c->mu);
    PLP_HIP(hipSetDevice(c->device));
    Stage s(c->stage, c->stream);
    s.in(A.pose, B * 15); s.in(A.counts, B); s.in(A.pos_w, BM * (lines ? 6 : 3)); s.in(A.normal, BM * 3);
    s.in(A.min_dist, BM); s.in(A.max_dist, BM); s.in(A.skip, BM);
    s.out(A.reproj, BM * 2); s.out(A.reproj2, BM * 2); s.out(A.x_right, BM); s.out(A.level, BM); s.out(A.valid, BM); s.out(A.num_valid, B);
    PLP_TRY(s.upload());
    PLP_HIP(lines ? launch_observe_lines(c->stream, A, a->B) : launch_observe_points(c->stream, A, a->B));
    return s.finish();
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

plp_status last_frame_device(plp_matcher* c, const plp_last_frame_args* a, bool lines, void* hip_stream) {
    if (plp_status s = last_frame_check(c, a, lines)) return s;
    std::lock_guard<std::mutex> lk(c->mu);
    PLP_HIP(hipSetDevice(c->device));
    const ObserveArgs A = last_frame_args(a, lines);
    PLP_HIP(lines ? launch_last_frame_lines((hipStream_t)hip_stream, A, a->B) : launch_last_frame_points((hipStream_t)hip_stream, A, a->B));
    return PLP_OK;
}

// m_cap == 0: nothing per slot is staged, the kernels still write every problem's direction and num_valid
plp_status last_frame_host(plp_matcher* c, const plp_last_frame_args* a, bool lines) {
    if (plp_status s = last_frame_check(c, a, lines)) return s;
    const size_t B = (size_t)a->B, BM = B * a->m_cap;
    ObserveArgs A = last_frame_args(a, lines);
    std::lock_guard<std::mutex> lk(c->mu);
    PLP_HIP(hipSetDevice(c->device));
    Stage s(c->stage, c->stream);
    s.in(A.pose, B * 15); s.in(A.pose_last, B * 15); s.in(A.counts, B); s.in(A.pos_w, BM * (lines ? 6 : 3)); s.in(A.skip, BM);
    s.in(A.kps, BM); s.in(A.kl, BM);
    s.out(A.reproj, BM * 2); s.out(A.reproj2, BM * 2); s.out(A.x_right, BM); s.out(A.x_right2, BM); s.out(A.level, BM); s.out(A.angle, BM);
    s.out(A.valid, BM); s.out(A.direction, B); s.out(A.num_valid, B);
    PLP_TRY(s.upload());
    PLP_HIP(lines ? launch_last_frame_lines(c->stream, A, a->B) : launch_last_frame_points(c->stream, A, a->B));
    return s.finish();
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

plp_status project_device(plp_matcher* c, const plp_project_args* a, bool lines, void* hip_stream) {
    if (plp_status s = project_check(c, a, lines)) return s;
    std::lock_guard<std::mutex> lk(c->mu);
    PLP_HIP(hipSetDevice(c->device));
    hipStream_t st = (hipStream_t)hip_stream;
    if (a->m_cap == 0) {   // no landmark slot: the reference's loop does not run
        if (a->out_num_valid) PLP_HIP(hipMemsetAsync(a->out_num_valid, 0, (size_t)a->B * 4, st));
        return PLP_OK;
    }
    const ProjectArgs A = project_args(a, lines);
    PLP_HIP(lines ? launch_project_lines(st, A, a->B) : launch_project_points(st, A, a->B));
    return PLP_OK;
}

plp_status project_host(plp_matcher* c, const plp_project_args* a, bool lines) {
    if (plp_status s = project_check(c, a, lines)) return s;
    const size_t B = (size_t)a->B, M = (size_t)a->m_cap, BM = B * M;
    if (M == 0) {
        if (a->out_num_valid) std::memset(a->out_num_valid, 0, B * 4);
        return PLP_OK;
    }
    ProjectArgs A = project_args(a, lines);
    const size_t LM = A.shared ? M : BM;   // rows of the landmark tables
    std::lock_guard<std::mutex> lk(c->mu);
    PLP_HIP(hipSetDevice(c->device));
    Stage s(c->stage, c->stream);
    s.in(A.pose, B * 15); s.in(A.counts, B); s.in(A.pos_w, LM * (lines ? 6 : 3)); s.in(A.normal, LM * 3);
    s.in(A.min_dist, LM); s.in(A.max_dist, LM); s.in(A.skip, BM);
    s.out(A.reproj_d, BM * 2); s.out(A.reproj2_d, BM * 2); s.out(A.reproj, BM * 2); s.out(A.reproj2, BM * 2); s.out(A.x_right, BM); s.out(A.x_right2, BM);
    s.out(A.level, BM); s.out(A.valid, BM); s.out(A.status, BM); s.out(A.num_valid, B);
    PLP_TRY(s.upload());
    PLP_HIP(lines ? launch_project_lines(c->stream, A, a->B) : launch_project_points(c->stream, A, a->B));
    return s.finish();
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
}  // namespace

plp_status plp_stereo_keylines_device(plp_matcher* c, const plp_stereo_keylines_args* a, void* hip_stream) {
    if (plp_status s = stereo_keylines_check(c, a)) return s;
    if (a->cap_left == 0) return PLP_OK;   // no left key line: nothing to write
    std::lock_guard<std::mutex> lk(c->mu);
    PLP_HIP(hipSetDevice(c->device));
    PLP_HIP(launch_stereo_keylines((hipStream_t)hip_stream, stereo_keylines_args(a), a->B));
    return PLP_OK;
}

plp_status plp_stereo_keylines_host(plp_matcher* c, const plp_stereo_keylines_args* a) {
    if (plp_status s = stereo_keylines_check(c, a)) return s;
    if (a->cap_left == 0) return PLP_OK;
    const size_t B = (size_t)a->B, L = (size_t)a->cap_left, R = (size_t)a->cap_right;
    StereoKeylineArgs A = stereo_keylines_args(a);
    std::lock_guard<std::mutex> lk(c->mu);
    PLP_HIP(hipSetDevice(c->device));
    Stage s(c->stage, c->stream);
    s.in(A.kl_l, B * L); s.in(A.counts_l, B); s.in(A.kl_r, B * R); s.in(A.counts_r, B); s.in(A.train_idx, B * L); s.in(A.dist, B * L);
    s.out(A.good, B * L); s.out(A.depths, B * L * 2); s.out(A.x_right, B * L * 2);
    PLP_TRY(s.upload());
    PLP_HIP(launch_stereo_keylines(c->stream, A, a->B));
    return s.finish();
}

plp_status plp_keylines_3d_device(plp_matcher* c, const plp_keylines_3d_args* a, void* hip_stream) {
    if (plp_status s = keylines_3d_check(c, a)) return s;
    if (a->cap == 0) return PLP_OK;
    std::lock_guard<std::mutex> lk(c->mu);
    PLP_HIP(hipSetDevice(c->device));
    PLP_HIP(launch_keylines_3d((hipStream_t)hip_stream, keylines_3d_args(a), a->B));
    return PLP_OK;
}

plp_status plp_keylines_3d_host(plp_matcher* c, const plp_keylines_3d_args* a) {
    if (plp_status s = keylines_3d_check(c, a)) return s;
    if (a->cap == 0) return PLP_OK;
    const size_t B = (size_t)a->B, M = (size_t)a->cap, R = (size_t)a->cap_right;
    Keylines3dArgs A = keylines_3d_args(a);
    std::lock_guard<std::mutex> lk(c->mu);
    PLP_HIP(hipSetDevice(c->device));
    Stage s(c->stage, c->stream);
    s.in(A.counts, B); s.in(A.pose, B * 15); s.in(A.kl, B * M); s.in(A.kl_depths, B * M * 2); s.in(A.good_match, B * M); s.in(A.kl_r, B * R);
    s.in(A.counts_r, B); s.out(A.pos_w, B * M * 6); s.out(A.valid, B * M);
    PLP_TRY(s.upload());
    PLP_HIP(launch_keylines_3d(c->stream, A, a->B));
    return s.finish();
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
}  // namespace

plp_status plp_median_depth_device(plp_matcher* c, const plp_median_depth_args* a, void* hip_stream) {
    if (plp_status s = median_depth_check(c, a)) return s;
    std::lock_guard<std::mutex> lk(c->mu);
    PLP_HIP(hipSetDevice(c->device));
    PLP_HIP(launch_median_depth((hipStream_t)hip_stream, median_depth_args(a), a->F));
    return PLP_OK;
}

plp_status plp_median_depth_host(plp_matcher* c, const plp_median_depth_args* a) {
    if (plp_status s = median_depth_check(c, a)) return s;
    const size_t F = (size_t)a->F, M = (size_t)a->m_cap;
    MedianDepthArgs A = median_depth_args(a);
    std::lock_guard<std::mutex> lk(c->mu);
    PLP_HIP(hipSetDevice(c->device));
    Stage s(c->stage, c->stream);
    s.in(A.pose, F * 15); s.in(A.pos_w, F * M * 3); s.in(A.valid, F * M); s.in(A.counts, F); s.out(A.median, F); s.out(A.count, F);
    PLP_TRY(s.upload());
    PLP_HIP(launch_median_depth(c->stream, A, a->F));
    return s.finish();
}

plp_status plp_triangulate_keyline_pairs_device(plp_matcher* c, const plp_keyline_pairs_args* a, void* hip_stream) {
    if (plp_status s = keyline_pairs_check(c, a)) return s;
    if (keyline_pairs_empty(a)) return PLP_OK;
    std::lock_guard<std::mutex> lk(c->mu);
    PLP_HIP(hipSetDevice(c->device));
    PLP_HIP(launch_keyline_pairs((hipStream_t)hip_stream, keyline_pairs_args(a)));
    return PLP_OK;
}

plp_status plp_triangulate_keyline_pairs_host(plp_matcher* c, const plp_keyline_pairs_args* a) {
    if (plp_status s = keyline_pairs_check(c, a)) return s;
    if (keyline_pairs_empty(a)) return PLP_OK;
    if (plp_status s = keyline_pairs_check_groups(a)) return s;
    const size_t F = (size_t)a->F, M = (size_t)a->cap, K = (size_t)a->kp_cap, P = (size_t)a->P, G = (size_t)a->G;
    KeylinePairArgs A = keyline_pairs_args(a);
    std::lock_guard<std::mutex> lk(c->mu);
    PLP_HIP(hipSetDevice(c->device));
    Stage s(c->stage, c->stream);
    s.in(A.kl, F * M); s.in(A.counts, F); s.in(A.line_fn, F * M * 3); s.in(A.x_right, F * M * 2); s.in(A.kp_depths, F * K); s.in(A.kp_counts, F);
    s.in(A.pose, F * 15); s.in(A.median, F); s.in(A.lines_3d, F * M * 6); s.in(A.occupied, F * M); s.in(A.pairs, P * 2); s.in(A.group_offsets, G + 1);
    s.in(A.train_idx, P * M); s.in(A.dist, P * M);
    s.out(A.out_match, P * M); s.out(A.out_pos_w, P * M * 6); s.out(A.out_status, P * M); s.out(A.out_occ_cur, G * M);
    PLP_TRY(s.upload());
    PLP_HIP(launch_keyline_pairs(c->stream, A));
    return s.finish();
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
}  // namespace

plp_status plp_keyframe_pair_geometry_device(plp_matcher* c, const plp_keyframe_pair_geometry_args* a, void* hip_stream) {
    if (plp_status s = pair_geometry_check(c, a)) return s;
    if (a->P == 0) return PLP_OK;
    std::lock_guard<std::mutex> lk(c->mu);
    PLP_HIP(hipSetDevice(c->device));
    PLP_HIP(launch_pair_geometry((hipStream_t)hip_stream, pair_geometry_args(a)));
    return PLP_OK;
}

plp_status plp_keyframe_pair_geometry_host(plp_matcher* c, const plp_keyframe_pair_geometry_args* a) {
    if (plp_status s = pair_geometry_check(c, a)) return s;
    if (a->P == 0) return PLP_OK;
    if (plp_status s = check_pairs_in_table(a->pairs, a->P, a->F)) return s;
    const size_t F = (size_t)a->F, P = (size_t)a->P;
    PairGeometryArgs A = pair_geometry_args(a);
    std::lock_guard<std::mutex> lk(c->mu);
    PLP_HIP(hipSetDevice(c->device));
    Stage s(c->stage, c->stream);
    s.in(A.pose, F * 15); s.in(A.median, F); s.in(A.pairs, P * 2); s.out(A.out_skip, P); s.out(A.out_epipolar, P * 12); s.out(A.out_baseline, P);
    PLP_TRY(s.upload());
    PLP_HIP(launch_pair_geometry(c->stream, A));
    return s.finish();
}

plp_status plp_triangulate_keypoint_pairs_device(plp_matcher* c, const plp_keypoint_pairs_args* a, void* hip_stream) {
    if (plp_status s = keypoint_pairs_check(c, a)) return s;
    if (keypoint_pairs_empty(a)) return PLP_OK;
    std::lock_guard<std::mutex> lk(c->mu);
    PLP_HIP(hipSetDevice(c->device));
    PLP_HIP(launch_keypoint_pairs((hipStream_t)hip_stream, keypoint_pairs_args(a)));
    return PLP_OK;
}

plp_status plp_triangulate_keypoint_pairs_host(plp_matcher* c, const plp_keypoint_pairs_args* a) {
    if (plp_status s = keypoint_pairs_check(c, a)) return s;
    if (keypoint_pairs_empty(a)) return PLP_OK;
    if (plp_status s = check_pairs_in_table(a->pairs, a->P, a->F)) return s;
    const size_t F = (size_t)a->F, M = (size_t)a->cap, Q = (size_t)a->m_cap, P = (size_t)a->P;
    KeypointPairArgs A = keypoint_pairs_args(a);
    std::lock_guard<std::mutex> lk(c->mu);
    PLP_HIP(hipSetDevice(c->device));
    Stage s(c->stage, c->stream);
    s.in(A.kps, F * M); s.in(A.bearings, F * M * 3); s.in(A.x_right, F * M); s.in(A.depths, F * M); s.in(A.counts, F); s.in(A.pose, F * 15);
    s.in(A.pairs, P * 2); s.in(A.match_q, P * M); s.in(A.q_feature, P * Q); s.in(A.pair_skip, P);
    s.out(A.out_idx_1, P * M); s.out(A.out_pos_w, P * M * 3); s.out(A.out_status, P * M); s.out(A.occ1, P * M); s.out(A.occ2, P * M);
    PLP_TRY(s.upload());
    PLP_HIP(launch_keypoint_pairs(c->stream, A));
    return s.finish();
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

plp_status landmark_geometry_device(plp_matcher* c, const plp_landmark_geometry_args* a, void* hip_stream, bool lines) {
    if (!c) return set_error(PLP_ERR_INVALID_ARG, "ctx is NULL");
    if (plp_status s = landmark_geometry_check(a, lines)) return s;
    if (a->L == 0) return PLP_OK;
    std::lock_guard<std::mutex> lk(c->mu);
    PLP_HIP(hipSetDevice(c->device));
    const LandmarkGeometryArgs A = landmark_geometry_args(a, lines);
    PLP_HIP(lines ? launch_landmark_geometry_lines((hipStream_t)hip_stream, A) : launch_landmark_geometry_points((hipStream_t)hip_stream, A));
    return PLP_OK;
}

plp_status landmark_geometry_host(plp_matcher* c, const plp_landmark_geometry_args* a, bool lines) {
    if (!c) return set_error(PLP_ERR_INVALID_ARG, "ctx is NULL");
    if (plp_status s = landmark_geometry_check(a, lines)) return s;
    if (a->L == 0) return PLP_OK;
    if (plp_status s = landmark_geometry_check_offsets(a)) return s;
    const size_t F = (size_t)a->F, M = (size_t)a->cap, L = (size_t)a->L, T = (size_t)a->obs_offsets[a->L];
    LandmarkGeometryArgs A = landmark_geometry_args(a, lines);
    std::lock_guard<std::mutex> lk(c->mu);
    PLP_HIP(hipSetDevice(c->device));
    Stage s(c->stage, c->stream);
    s.in(A.pose, F * 15); s.in(A.counts, F); s.in(A.kps, F * M); s.in(A.kl, F * M); s.in(A.pos_w, L * (lines ? 6 : 3)); s.in(A.ref_kf, L); s.in(A.skip, L);
    s.in(A.obs_offsets, L + 1); s.in(A.obs_kf, T); s.in(A.obs_idx, T);
    s.out(A.normal, L * 3); s.out(A.min_dist, L); s.out(A.max_dist, L); s.out(A.status, L);
    PLP_TRY(s.upload());
    PLP_HIP(lines ? launch_landmark_geometry_lines(c->stream, A) : launch_landmark_geometry_points(c->stream, A));
    return s.finish();
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
    std::lock_guard<std::mutex> lk(c->mu);
    PLP_HIP(hipSetDevice(c->device));
    PLP_HIP(launch_bow_score_pairs((hipStream_t)hip_stream, bow_pairs_args(a)));
    return PLP_OK;
}

plp_status plp_bow_score_pairs_host(plp_matcher* c, const plp_bow_score_pairs_args* a) {
    if (!c) return set_error(PLP_ERR_INVALID_ARG, "ctx is NULL");
    if (plp_status s = bow_pairs_check(a)) return s;
    if (a->P == 0) return PLP_OK;
    BowPairsArgs A = bow_pairs_args(a);
    std::lock_guard<std::mutex> lk(c->mu);
    PLP_HIP(hipSetDevice(c->device));
    Stage s(c->stage, c->stream);
    s.in(A.a_word, (size_t)a->NA * a->stride_a); s.in(A.a_value, (size_t)a->NA * a->stride_a); s.in(A.a_n, (size_t)a->NA);
    s.in(A.b_word, (size_t)a->NB * a->stride_b); s.in(A.b_value, (size_t)a->NB * a->stride_b); s.in(A.b_n, (size_t)a->NB);
    s.in(A.a_row, (size_t)a->P); s.in(A.b_row, (size_t)a->P);
    s.out(A.out_score, (size_t)a->P, false);
    PLP_TRY(s.upload());
    PLP_HIP(launch_bow_score_pairs(c->stream, A));
    return s.finish();
}

// the host build of bow_score.hpp (no HIP call)
double plp_model_bow_score_host(const uint32_t* wa, const double* va, int32_t na, const uint32_t* wb, const double* vb, int32_t nb) {
    if (na < 0 || nb < 0 || (na > 0 && (!wa || !va)) || (nb > 0 && (!wb || !vb))) return -1.0;
    return bow_l1_score(wa, va, na, wb, vb, nb);
}

// ---- loop candidates: solve::sim3_solver (include/plp_front.h: plp_sim3_ransac_*; sim3_kernels.hip, sim3.hpp)
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

// one problem of the host build: the kernel's steps, one hypothesis and one point after the other
extern "C++" template <int MODEL> void sim3_model_problem(const Sim3Args& A, int p) {
    const int count = sim3_count(A, p);
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
            if (sim3_sample(A, p, it, n, idx)) {
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
    std::lock_guard<std::mutex> lk(c->mu);
    PLP_HIP(hipSetDevice(c->device));
    Sim3Args A = sim3_args(a);
    PLP_HIP(c->sim3_ctx.reserve((size_t)a->P * kSim3CtxInts * sizeof(int32_t)));
    PLP_HIP(c->sim3_hyp.reserve((size_t)a->P * kSim3HypDoubles * a->iters * sizeof(double)));
    A.ctx = (int32_t*)c->sim3_ctx.p; A.ctx_hyp = (double*)c->sim3_hyp.p;
    PLP_HIP(launch_sim3_ransac((hipStream_t)hip_stream, A));
    return PLP_OK;
}

plp_status plp_sim3_ransac_host(plp_matcher* c, const plp_sim3_ransac_args* a) {
    if (!c) return set_error(PLP_ERR_INVALID_ARG, "ctx is NULL");
    if (plp_status s = sim3_check(a)) return s;
    if (a->P == 0 || a->n_cap == 0) return PLP_OK;
    const size_t P = (size_t)a->P, M = (size_t)a->n_cap, I = (size_t)a->iters;
    Sim3Args A = sim3_args(a);
    std::lock_guard<std::mutex> lk(c->mu);
    PLP_HIP(hipSetDevice(c->device));
    Stage s(c->stage, c->stream);
    s.in(A.valid, P * M); s.in(A.pos_w_1, P * M * 3); s.in(A.pos_w_2, P * M * 3); s.in(A.octave_1, P * M); s.in(A.octave_2, P * M); s.in(A.counts, P);
    s.in(A.pose_1, P * 15); s.in(A.pose_2, P * 15); s.in(A.samples, P * I * 3);
    s.out(A.out_status, P, false); s.out(A.out_num_common, P, false); s.out(A.out_rot_12, P * 9, false); s.out(A.out_trans_12, P * 3, false);
    s.out(A.out_scale_12, P, false); s.out(A.out_num_inliers, P, false); s.out(A.out_best_iter, P, false); s.out(A.out_inliers, P * M);
    s.out(A.out_hyp_inliers, P * I, false); s.room(A.ctx, P * kSim3CtxInts); s.room(A.ctx_hyp, P * kSim3HypDoubles * I);
    PLP_TRY(s.upload());
    PLP_HIP(launch_sim3_ransac(c->stream, A));
    return s.finish();
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
    if (n_iters < 0 || num_common < 3 || (n_iters > 0 && !out)) return -1;
    for (int32_t i = 0; i < n_iters; ++i) {
        int idx[3];
        sim3_draw(seed, p, iter0 + i, num_common, idx);
        out[3 * (size_t)i] = idx[0]; out[3 * (size_t)i + 1] = idx[1]; out[3 * (size_t)i + 2] = idx[2];
    }
    return n_iters;
}

int32_t plp_model_sym_eig4_max_host(const double* N, int32_t n, double* out_v, int32_t* out_sweeps) {
    if (n < 0 || (n > 0 && (!N || !out_v))) return -1;
    for (int32_t i = 0; i < n; ++i) {
        const int sweeps = sym_eig4_max(N + 16 * (size_t)i, out_v + 4 * (size_t)i);
        if (out_sweeps) out_sweeps[i] = sweeps;
    }
    return n;
}

// ---- relocalisation: solve::pnp_solver (include/plp_front.h: plp_pnp_ransac_*; pnp_kernels.hip, pnp.hpp)
namespace {
plp_status pnp_check(const plp_pnp_ransac_args* a) {
    if (!a) return set_error(PLP_ERR_INVALID_ARG, "NULL argument");
    if (a->P < 0 || a->n_cap < 0) return set_error(PLP_ERR_INVALID_ARG, "P and n_cap must not be negative");
    if (a->iters < 1 || a->min_num_inliers < 0) return set_error(PLP_ERR_INVALID_ARG, "iters must be positive, min_num_inliers non-negative");
    if (a->num_levels < 1 || a->num_levels > 16 || !a->scale_factors) return set_error(PLP_ERR_INVALID_ARG, "num_levels must be 1 .. 16, scale_factors is required");
    if (a->n_cap > kPnpMaxSlots) return set_error(PLP_ERR_UNSUPPORTED, "more than 8192 slots per problem");
    if (a->P > 65535) return set_error(PLP_ERR_UNSUPPORTED, "more than 65535 problems in one call");
    if (a->P == 0 || a->n_cap == 0) return PLP_OK;
    if (!a->valid || !a->bearing || !a->pos_w || !a->octave) return set_error(PLP_ERR_INVALID_ARG, "valid, bearing, pos_w, octave are required");
    if (!a->out_status || !a->out_num_matches || !a->out_rot_cw || !a->out_trans_cw || !a->out_num_inliers || !a->out_best_iter)
        return set_error(PLP_ERR_INVALID_ARG, "out_status, out_num_matches, out_rot_cw, out_trans_cw, out_num_inliers, out_best_iter are required");
    return PLP_OK;
}

PnpArgs pnp_args(const plp_pnp_ransac_args* a) {
    PnpArgs A{};
    A.P = a->P; A.n_cap = a->n_cap; A.iters = a->iters; A.min_num_inliers = a->min_num_inliers; A.recompute = a->recompute != 0;
    A.num_levels = a->num_levels; A.seed = a->seed;
    for (int l = 0; l < 16; ++l) A.thr[l] = l < a->num_levels ? pnp_level_threshold(a->scale_factors[l]) : 0.0f;
    A.valid = a->valid; A.bearing = a->bearing; A.pos_w = a->pos_w; A.octave = a->octave; A.counts = a->counts; A.samples = a->samples;
    A.out_status = a->out_status; A.out_num_matches = a->out_num_matches; A.out_rot_cw = a->out_rot_cw; A.out_trans_cw = a->out_trans_cw;
    A.out_num_inliers = a->out_num_inliers; A.out_best_iter = a->out_best_iter; A.out_inliers = a->out_inliers; A.out_hyp_inliers = a->out_hyp_inliers;
    return A;
}

// compute_pose (:230-290) of the host build for nc >= 1 correspondences held kPnpCorrDoubles apart; returns the chosen approximation 0 .. 2
int pnp_model_pose(PnpWork& W, double* corr, int nc, int sign0) {
    std::vector<double> G(144), V(144);
    pnp_pose_front(W, corr, corr + 3, corr + 5, kPnpCorrDoubles, nc);
    pnp_null_space(W, G.data(), V.data());
    return pnp_pose_back(W, corr, corr + 3, corr + 5, corr + 9, kPnpCorrDoubles, nc, sign0);
}

// one problem of the host build: the kernels' steps, one hypothesis and one match after the other
void pnp_model_problem(const PnpArgs& A, int p) {
    const int count = pnp_count(A, p);
    const size_t row = (size_t)p * A.n_cap;
    std::vector<int> slot_of;
    for (int s = 0; s < count; ++s)
        if (A.valid[row + s]) slot_of.push_back(s);
    const int n = (int)slot_of.size();
    auto inlier = [&](const double* R, const double* t, int k) {
        const size_t s = row + slot_of[k];
        const int o = A.octave[s];
        const bool lv = (unsigned)o < (unsigned)A.num_levels;
        return pnp_inlier(R, t, A.pos_w + 3 * s, A.bearing + 3 * s, lv ? A.thr[o] : 0.0f, !lv);
    };
    int best_count = 0, best_iter = -1;
    double best[12] = {0};
    std::vector<uint8_t> best_flags((size_t)n, 0), flags((size_t)n, 0);
    std::vector<double> corr((size_t)(n > 4 ? n : 4) * kPnpCorrDoubles);
    PnpWork W;
    const bool enough = !(n < 4 || n < A.min_num_inliers);          // :76
    for (int it = 0; it < A.iters; ++it) {
        int num = 0;
        int idx[4];
        if (enough && pnp_sample(A, p, it, n, idx)) {
            int nc = 0, sign0 = 0;
            for (int k = 0; k < 4; ++k) {
                const size_t s = row + slot_of[idx[k]];
                int sg;
                if (pnp_add_correspondence(A.pos_w + 3 * s, A.bearing + 3 * s, corr.data() + nc * kPnpCorrDoubles, corr.data() + nc * kPnpCorrDoubles + 3, sg)) {
                    if (nc == 0) sign0 = sg;
                    ++nc;
                }
            }
            if (nc > 0) {
                const int N = pnp_model_pose(W, corr.data(), nc, sign0);
                for (int k = 0; k < n; ++k) { flags[k] = inlier(W.Rs + 9 * N, W.ts + 3 * N, k) ? 1 : 0; num += flags[k]; }
                if (best_count < num) {                             // :117
                    best_count = num; best_iter = it; best_flags = flags;
                    for (int i = 0; i < 9; ++i) best[i] = W.Rs[9 * N + i];
                    for (int i = 0; i < 3; ++i) best[9 + i] = W.ts[3 * N + i];
                }
            }
        }
        if (A.out_hyp_inliers) A.out_hyp_inliers[(size_t)p * A.iters + it] = num;
    }
    const bool ok = enough && best_count > A.min_num_inliers;       // :126
    const bool have = ok && best_iter >= 0;
    if (have && A.recompute) {                                      // :136-152
        int nc = 0, sign0 = 0;
        for (int k = 0; k < n; ++k) {
            if (!best_flags[k]) continue;
            const size_t s = row + slot_of[k];
            int sg;
            if (pnp_add_correspondence(A.pos_w + 3 * s, A.bearing + 3 * s, corr.data() + (size_t)nc * kPnpCorrDoubles, corr.data() + (size_t)nc * kPnpCorrDoubles + 3, sg)) {
                if (nc == 0) sign0 = sg;
                ++nc;
            }
        }
        if (nc > 0) {
            const int N = pnp_model_pose(W, corr.data(), nc, sign0);
            for (int i = 0; i < 9; ++i) best[i] = W.Rs[9 * N + i];
            for (int i = 0; i < 3; ++i) best[9 + i] = W.ts[3 * N + i];
        }
    }
    A.out_status[p] = !enough ? PLP_PNP_TOO_FEW_MATCHES : ok ? PLP_PNP_OK : PLP_PNP_TOO_FEW_INLIERS;
    A.out_num_matches[p] = n;
    A.out_num_inliers[p] = best_count;
    A.out_best_iter[p] = ok ? best_iter : -1;
    for (int i = 0; i < 9; ++i) A.out_rot_cw[(size_t)9 * p + i] = have ? best[i] : 0.0;
    for (int i = 0; i < 3; ++i) A.out_trans_cw[(size_t)3 * p + i] = have ? best[9 + i] : 0.0;
    if (A.out_inliers) {
        for (int s = 0; s < count; ++s) A.out_inliers[row + s] = 0;
        if (have)
            for (int k = 0; k < n; ++k) A.out_inliers[row + slot_of[k]] = best_flags[k];
    }
}
}  // namespace

plp_status plp_pnp_ransac_device(plp_matcher* c, const plp_pnp_ransac_args* a, void* hip_stream) {
    if (!c) return set_error(PLP_ERR_INVALID_ARG, "ctx is NULL");
    if (plp_status s = pnp_check(a)) return s;
    if (a->P == 0 || a->n_cap == 0) return PLP_OK;
    std::lock_guard<std::mutex> lk(c->mu);
    PLP_HIP(hipSetDevice(c->device));
    PnpArgs A = pnp_args(a);
    const size_t P = (size_t)a->P, M = (size_t)a->n_cap;
    PLP_HIP(c->pnp_ctx.reserve(P * kPnpCtxInts * sizeof(int32_t)));
    PLP_HIP(c->pnp_slot.reserve(P * M * sizeof(uint16_t)));
    PLP_HIP(c->pnp_hyp.reserve(P * kPnpHypDoubles * a->iters * sizeof(double)));
    PLP_HIP(c->pnp_corr.reserve(P * M * kPnpCorrDoubles * sizeof(double)));
    PLP_HIP(c->pnp_pose.reserve(P * 12 * sizeof(double)));
    PLP_HIP(c->pnp_sign.reserve(P * sizeof(int32_t)));
    A.ctx = (int32_t*)c->pnp_ctx.p; A.ctx_slot = (uint16_t*)c->pnp_slot.p; A.ctx_hyp = (double*)c->pnp_hyp.p; A.ctx_corr = (double*)c->pnp_corr.p;
    A.ctx_pose = (double*)c->pnp_pose.p; A.ctx_sign = (int32_t*)c->pnp_sign.p;
    PLP_HIP(launch_pnp_ransac((hipStream_t)hip_stream, A));
    return PLP_OK;
}

plp_status plp_pnp_ransac_host(plp_matcher* c, const plp_pnp_ransac_args* a) {
    if (!c) return set_error(PLP_ERR_INVALID_ARG, "ctx is NULL");
    if (plp_status s = pnp_check(a)) return s;
    if (a->P == 0 || a->n_cap == 0) return PLP_OK;
    const size_t P = (size_t)a->P, M = (size_t)a->n_cap, I = (size_t)a->iters;
    PnpArgs A = pnp_args(a);
    std::lock_guard<std::mutex> lk(c->mu);
    PLP_HIP(hipSetDevice(c->device));
    Stage s(c->stage, c->stream);
    s.in(A.valid, P * M); s.in(A.bearing, P * M * 3); s.in(A.pos_w, P * M * 3); s.in(A.octave, P * M); s.in(A.counts, P); s.in(A.samples, P * I * 4);
    s.out(A.out_status, P, false); s.out(A.out_num_matches, P, false); s.out(A.out_rot_cw, P * 9, false); s.out(A.out_trans_cw, P * 3, false);
    s.out(A.out_num_inliers, P, false); s.out(A.out_best_iter, P, false); s.out(A.out_inliers, P * M); s.out(A.out_hyp_inliers, P * I, false);
    s.room(A.ctx, P * kPnpCtxInts); s.room(A.ctx_slot, P * M); s.room(A.ctx_hyp, P * kPnpHypDoubles * I); s.room(A.ctx_corr, P * M * kPnpCorrDoubles);
    s.room(A.ctx_pose, P * 12); s.room(A.ctx_sign, P);
    PLP_TRY(s.upload());
    PLP_HIP(launch_pnp_ransac(c->stream, A));
    return s.finish();
}

// the host builds of pnp.hpp (no HIP call)
int32_t plp_model_pnp_ransac_host(const plp_pnp_ransac_args* a) {
    if (pnp_check(a) != PLP_OK) return -1;
    if (a->P == 0 || a->n_cap == 0) return a->P;
    const PnpArgs A = pnp_args(a);
    for (int p = 0; p < A.P; ++p) pnp_model_problem(A, p);
    return A.P;
}

int32_t plp_model_epnp_host(const double* pos_w, const double* bearing, const int32_t* offsets, int32_t n, double* out_rot, double* out_trans,
                            double* out_err, int32_t* out_N, int32_t* out_sweeps) {
    if (n < 0 || (n > 0 && (!offsets || !out_rot || !out_trans || !out_err || !out_N))) return -1;
    for (int32_t i = 0; i < n; ++i)
        if (offsets[i + 1] < offsets[i] || offsets[i] < 0 || (offsets[i + 1] > offsets[i] && (!pos_w || !bearing))) return -1;
    PnpWork W;
    for (int32_t i = 0; i < n; ++i) {
        const int m = offsets[i + 1] - offsets[i];
        std::vector<double> corr((size_t)(m > 0 ? m : 1) * kPnpCorrDoubles);
        int nc = 0, sign0 = 0;
        for (int k = 0; k < m; ++k) {
            const size_t s = (size_t)offsets[i] + k;
            int sg;
            if (pnp_add_correspondence(pos_w + 3 * s, bearing + 3 * s, corr.data() + (size_t)nc * kPnpCorrDoubles, corr.data() + (size_t)nc * kPnpCorrDoubles + 3, sg)) {
                if (nc == 0) sign0 = sg;
                ++nc;
            }
        }
        for (int k = 0; k < 8; ++k) W.sweeps[k] = 0;
        int N = -1;
        if (nc > 0) N = pnp_model_pose(W, corr.data(), nc, sign0);
        for (int k = 0; k < 9; ++k) out_rot[9 * (size_t)i + k] = N >= 0 ? W.Rs[9 * N + k] : 0.0;
        for (int k = 0; k < 3; ++k) out_trans[3 * (size_t)i + k] = N >= 0 ? W.ts[3 * N + k] : 0.0;
        out_err[i] = N >= 0 ? W.err[N] : 0.0;
        out_N[i] = N + 1;
        if (out_sweeps)
            for (int k = 0; k < 8; ++k) out_sweeps[8 * (size_t)i + k] = W.sweeps[k];
    }
    return n;
}

int32_t plp_model_sym_jacobi_host(const double* A, int32_t dim, int32_t n, double* out_vals, double* out_ut, int32_t* out_sweeps) {
    if ((dim != 3 && dim != 12) || n < 0 || (n > 0 && (!A || !out_vals || !out_ut))) return -1;
    std::vector<double> G((size_t)dim * dim), V((size_t)dim * dim), key((size_t)dim);
    for (int32_t i = 0; i < n; ++i) {
        const int sweeps = sym_jacobi(A + (size_t)i * dim * dim, dim, G.data(), V.data(), key.data(), out_vals + (size_t)i * dim, out_ut + (size_t)i * dim * dim);
        if (out_sweeps) out_sweeps[i] = sweeps;
    }
    return n;
}

int32_t plp_model_lstsq6_host(const double* A, const double* b, int32_t k, int32_t n, double* out_x, int32_t* out_sweeps) {
    if (k < 3 || k > 5 || n < 0 || (n > 0 && (!A || !b || !out_x))) return -1;
    double G[30], V[25], key[5];
    for (int32_t i = 0; i < n; ++i) {
        for (int r = 0; r < 6; ++r)
            for (int c = 0; c < k; ++c) G[6 * c + r] = A[((size_t)i * 6 + r) * k + c];
        const int sweeps = lstsq6(G, b + 6 * (size_t)i, k, V, key, out_x + (size_t)i * k);
        if (out_sweeps) out_sweeps[i] = sweeps;
    }
    return n;
}

int32_t plp_model_rot_from_abt_host(const double* Abt, int32_t n, double* out_rot, int32_t* out_sweeps) {
    if (n < 0 || (n > 0 && (!Abt || !out_rot))) return -1;
    double G[9], V[9], key[3], U[9];
    for (int32_t i = 0; i < n; ++i) {
        const int sweeps = rot_from_abt(Abt + 9 * (size_t)i, G, V, key, U, out_rot + 9 * (size_t)i);
        if (out_sweeps) out_sweeps[i] = sweeps;
    }
    return n;
}

int32_t plp_model_pnp_draw_host(uint64_t seed, int32_t p, int32_t iter0, int32_t n_iters, int32_t num_matches, int32_t* out) {
    if (n_iters < 0 || num_matches < 4 || (n_iters > 0 && !out)) return -1;
    for (int32_t i = 0; i < n_iters; ++i) {
        int idx[4];
        pnp_draw(seed, p, iter0 + i, num_matches, idx);
        for (int k = 0; k < 4; ++k) out[4 * (size_t)i + k] = idx[k];
    }
    return n_iters;
}

int32_t plp_model_pnp_thresholds_host(const float* scale_factors, int32_t num_levels, float* out) {
    if (num_levels < 0 || (num_levels > 0 && (!scale_factors || !out))) return -1;
    for (int32_t l = 0; l < num_levels; ++l) out[l] = pnp_level_threshold(scale_factors[l]);
    return num_levels;
}

// ---- per-frame pose optimisation: optimize::pose_optimizer[_extended_line] (include/plp_front.h: plp_pose_optimize_*; pose_opt_kernels.hip, pose_opt.hpp)
namespace {
plp_status pose_check(const plp_pose_optimize_args* a) {
    if (!a) return set_error(PLP_ERR_INVALID_ARG, "NULL argument");
    if (a->camera.model != PLP_CAMERA_PERSPECTIVE && a->camera.model != PLP_CAMERA_FISHEYE && a->camera.model != PLP_CAMERA_EQUIRECTANGULAR)
        return set_error(PLP_ERR_INVALID_ARG, "unknown camera model");
    if (a->setup_type < 0 || a->setup_type > 2) return set_error(PLP_ERR_INVALID_ARG, "setup_type must be 0, 1 or 2");
    if (a->B < 0 || a->n_cap < 0 || a->l_cap < 0) return set_error(PLP_ERR_INVALID_ARG, "B, n_cap and l_cap must not be negative");
    if (a->num_trials < 1 || a->num_each_iter < 1) return set_error(PLP_ERR_INVALID_ARG, "num_trials and num_each_iter must be positive");
    if (a->pose_stride < 12) return set_error(PLP_ERR_INVALID_ARG, "pose_stride must be at least 12");
    if (a->num_levels < 1 || a->num_levels > 16 || !a->inv_level_sigma_sq) return set_error(PLP_ERR_INVALID_ARG, "num_levels must be 1 .. 16, inv_level_sigma_sq is required");
    if (a->l_cap > 0 && (a->num_levels_lsd < 1 || a->num_levels_lsd > 16 || !a->inv_level_sigma_sq_lsd))
        return set_error(PLP_ERR_INVALID_ARG, "with lines num_levels_lsd must be 1 .. 16 and inv_level_sigma_sq_lsd is required");
    if (a->camera.model == PLP_CAMERA_EQUIRECTANGULAR) return set_error(PLP_ERR_UNSUPPORTED, "the equirectangular pose edge is not implemented (DESIGN.md D15)");
    if (!(a->camera.fx != 0) || !(a->camera.fy != 0)) return set_error(PLP_ERR_INVALID_ARG, "fx, fy must be non-zero");
    if (a->n_cap > kPoseMaxSlots || a->l_cap > kPoseMaxSlots) return set_error(PLP_ERR_UNSUPPORTED, "more than 8192 slots per frame");
    if (a->B > 65535) return set_error(PLP_ERR_UNSUPPORTED, "more than 65535 frames in one call");
    if (a->B == 0) return PLP_OK;
    if (!a->pose_in || !a->out_status || !a->out_pose || !a->out_num_init_obs || !a->out_num_valid)
        return set_error(PLP_ERR_INVALID_ARG, "pose_in, out_status, out_pose, out_num_init_obs, out_num_valid are required");
    if (a->n_cap > 0 && (!a->valid || !a->undist || !a->pos_w || !a->out_outlier)) return set_error(PLP_ERR_INVALID_ARG, "valid, undist, pos_w, out_outlier are required");
    if (a->l_cap > 0 && (!a->line_valid || !a->keylines || !a->pos_w_lines || !a->out_outlier_lines))
        return set_error(PLP_ERR_INVALID_ARG, "line_valid, keylines, pos_w_lines, out_outlier_lines are required");
    return PLP_OK;
}

PoseArgs pose_args(const plp_pose_optimize_args* a) {
    PoseArgs A{};
    A.B = a->B; A.n_cap = a->n_cap; A.l_cap = a->l_cap; A.num_trials = a->num_trials; A.num_each_iter = a->num_each_iter;
    A.mono_setup = a->setup_type == 0; A.pose_stride = a->pose_stride; A.num_levels = a->num_levels; A.num_levels_lsd = a->l_cap > 0 ? a->num_levels_lsd : 0;
    A.cam = pose_cam(a->camera.fx, a->camera.fy, a->camera.cx, a->camera.cy, a->camera.focal_x_baseline);
    A.delta_2d = (double)std::sqrt(kPoseChiSq2D); A.delta_3d = (double)std::sqrt(kPoseChiSq3D);     // const float sqrt_chi_sq_2D = std::sqrt(chi_sq_2D)
    for (int l = 0; l < 16; ++l) {
        A.inv_sigma_sq[l] = l < A.num_levels ? a->inv_level_sigma_sq[l] : 0.0f;
        A.inv_sigma_sq_lsd[l] = l < A.num_levels_lsd ? a->inv_level_sigma_sq_lsd[l] : 0.0f;
    }
    A.pose_in = a->pose_in; A.counts = a->counts; A.line_counts = a->line_counts; A.valid = a->valid; A.undist = a->undist; A.x_right = a->x_right;
    A.pos_w = a->pos_w; A.line_valid = a->line_valid; A.keylines = a->keylines; A.pos_w_lines = a->pos_w_lines;
    A.out_status = a->out_status; A.out_pose = a->out_pose; A.out_num_init_obs = a->out_num_init_obs; A.out_num_valid = a->out_num_valid;
    A.out_outlier = a->out_outlier; A.out_outlier_lines = a->out_outlier_lines; A.out_trial_info = a->out_trial_info; A.out_trial_chi2 = a->out_trial_chi2;
    return A;
}

// the edges of one frame of the host build, in rank order
struct PoseEdges {
    std::vector<int> slot, lslot;
    std::vector<uint8_t> level, llevel;         // 1 = outlier (edge level 1)
    std::vector<double> chi2, lchi2;            // of the last evaluation
};
void pose_model_edges(const PoseArgs& A, int b, bool lines, PoseEdges& E) {
    const size_t row = (size_t)b * A.n_cap, lrow = (size_t)b * A.l_cap;
    const int count = pose_count(A, b);
    for (int s = 0; s < count; ++s)
        if (A.valid[row + s] && (unsigned)A.undist[row + s].octave < (unsigned)A.num_levels) E.slot.push_back(s);
    if (lines) {
        const int lcount = pose_line_count(A, b);
        for (int s = 0; s < lcount; ++s)
            if (A.line_valid[lrow + s] && (unsigned)A.keylines[lrow + s].octave < (unsigned)A.num_levels_lsd) E.lslot.push_back(s);
    }
    E.level.assign(E.slot.size(), 0); E.llevel.assign(E.lslot.size(), 0);
    E.chi2.assign(E.slot.size(), 0.0); E.lchi2.assign(E.lslot.size(), 0.0);
}
double pose_model_point_chi2(const PoseArgs& A, int b, int slot, const double* est) {
    const size_t s = (size_t)b * A.n_cap + slot;
    const float xr = A.x_right ? A.x_right[s] : -1.0f;
    double x, y, z, e0, e1, e2;
    return pose_point_error(est, A.cam, A.pos_w + 3 * s, (double)A.undist[s].x, (double)A.undist[s].y, (double)xr, xr < 0.0f,
                            (double)A.inv_sigma_sq[A.undist[s].octave], x, y, z, e0, e1, e2);
}
double pose_model_line_chi2(const PoseArgs& A, int b, int slot, const double* est) {
    const size_t s = (size_t)b * A.l_cap + slot;
    const plp_keyline& kl = A.keylines[s];
    double e0, e1;
    return pose_line_error(est, A.cam, A.pos_w_lines + 6 * s, (double)kl.startPointX, (double)kl.startPointY, (double)kl.endPointX, (double)kl.endPointY,
                           (double)A.inv_sigma_sq_lsd[kl.octave], e0, e1);
}
// one pass over the active edges at W.est: sums[28] when lin, else sums[27] alone; stores the chi2 of every active edge
void pose_model_pass(const PoseArgs& A, int b, PoseWork& W, PoseEdges& E, bool robust, bool lin, double* sums) {
    const double delta_pt = A.mono_setup ? A.delta_2d : A.delta_3d;
    for (int t = 0; t < kPoseTerms; ++t) sums[t] = 0.0;
    double T[kPoseTerms];
    if (lin && !E.lslot.empty())
        for (int i = 0; i < 12; ++i) pose_perturb(W.est, i, W.pert + 7 * i);
    for (size_t k = 0; k < E.slot.size(); ++k) {
        if (E.level[k]) continue;
        const size_t s = (size_t)b * A.n_cap + E.slot[k];
        if (lin) {
            const float xr = A.x_right ? A.x_right[s] : -1.0f;
            E.chi2[k] = pose_point_terms(W.est, A.cam, A.pos_w + 3 * s, (double)A.undist[s].x, (double)A.undist[s].y, (double)xr, xr < 0.0f,
                                         (double)A.inv_sigma_sq[A.undist[s].octave], robust, delta_pt, T, 1);
            for (int t = 0; t < kPoseTerms; ++t) sums[t] = sums[t] + T[t];
        } else {
            const double chi2 = pose_model_point_chi2(A, b, E.slot[k], W.est);
            double rho0 = chi2, rho1 = 1.0;
            if (robust) pose_huber(chi2, delta_pt, rho0, rho1);
            E.chi2[k] = chi2;
            sums[27] = sums[27] + rho0;
        }
    }
    for (size_t k = 0; k < E.lslot.size(); ++k) {
        if (E.llevel[k]) continue;
        const size_t s = (size_t)b * A.l_cap + E.lslot[k];
        if (lin) {
            const plp_keyline& kl = A.keylines[s];
            E.lchi2[k] = pose_line_terms(W.est, W.pert, A.cam, A.pos_w_lines + 6 * s, (double)kl.startPointX, (double)kl.startPointY, (double)kl.endPointX,
                                         (double)kl.endPointY, (double)A.inv_sigma_sq_lsd[kl.octave], robust, A.delta_2d, T, 1);
            for (int t = 0; t < kPoseTerms; ++t) sums[t] = sums[t] + T[t];
        } else {
            const double chi2 = pose_model_line_chi2(A, b, E.lslot[k], W.est);
            double rho0 = chi2, rho1 = 1.0;
            if (robust) pose_huber(chi2, A.delta_2d, rho0, rho1);
            E.lchi2[k] = chi2;
            sums[27] = sums[27] + rho0;
        }
    }
}

// one frame of the host build: the kernels' steps, one edge after the other
void pose_model_frame(const PoseArgs& A, int b) {
    const size_t row = (size_t)b * A.n_cap, lrow = (size_t)b * A.l_cap;
    const int T = A.num_trials;
    PoseEdges E;
    pose_model_edges(A, b, false, E);
    const int n = (int)E.slot.size();
    for (int s : E.slot) A.out_outlier[row + s] = 0;
    if (A.out_trial_info) for (int i = 0; i < 4 * T; ++i) A.out_trial_info[(size_t)4 * T * b + i] = 0;
    if (A.out_trial_chi2) for (int i = 0; i < 2 * T; ++i) A.out_trial_chi2[(size_t)2 * T * b + i] = 0.0;
    const double* in = A.pose_in + (size_t)b * A.pose_stride;
    double* out = A.out_pose + (size_t)15 * b;
    A.out_num_init_obs[b] = n;
    if (n < kPoseMinObs) {
        for (int i = 0; i < 12; ++i) out[i] = in[i];
        for (int i = 0; i < 3; ++i) out[12 + i] = ((-in[i]) * in[9] + (-in[3 + i]) * in[10]) + (-in[6 + i]) * in[11];
        A.out_status[b] = PLP_POSE_OPT_TOO_FEW_OBS;
        A.out_num_valid[b] = 0;
        return;
    }
    if (A.l_cap > 0) {
        E = PoseEdges();
        pose_model_edges(A, b, true, E);
        for (int s : E.lslot) A.out_outlier_lines[lrow + s] = 0;
    }
    PoseWork W{};
    pose_est_from_pose(in, W.est);
    W.ni = 2.0;
    int num_bad = 0;
    double sums[kPoseTerms];
    for (int trial = 0; trial < T; ++trial) {
        const bool robust = pose_trial_robust(trial, T);
        W.iterations = 0; W.rejected = 0; W.end = 0;
        for (int it = 0; it < A.num_each_iter; ++it) {
            pose_model_pass(A, b, W, E, robust, true, W.sum);
            pose_lm_begin(W, it);
            do {
                pose_lm_try(W);
                pose_model_pass(A, b, W, E, robust, false, sums);
                pose_lm_decide(W, sums[27]);
            } while (W.go_on);
            W.iterations += 1;
            W.end = pose_lm_end(W);
            if (W.end) break;
        }
        num_bad = 0;
        for (int k = 0; k < n; ++k) {
            const size_t s = row + E.slot[k];
            const float xr = A.x_right ? A.x_right[s] : -1.0f;
            const double chi2 = E.level[k] ? pose_model_point_chi2(A, b, E.slot[k], W.est) : E.chi2[k];
            const bool bad = (double)(xr < 0.0f ? kPoseChiSq2D : kPoseChiSq3D) < chi2;
            E.level[k] = bad; A.out_outlier[s] = bad;
            num_bad += bad;
        }
        const bool stop = n - num_bad < kPoseMinObs;
        if (!stop)
            for (size_t k = 0; k < E.lslot.size(); ++k) {
                const double chi2 = E.llevel[k] ? pose_model_line_chi2(A, b, E.lslot[k], W.est) : E.lchi2[k];
                const bool bad = (double)kPoseChiSq2D < chi2;
                E.llevel[k] = bad; A.out_outlier_lines[lrow + E.lslot[k]] = bad;
            }
        if (A.out_trial_info) {
            int32_t* ti = A.out_trial_info + ((size_t)T * b + trial) * 4;
            ti[0] = W.iterations; ti[1] = W.rejected; ti[2] = num_bad; ti[3] = W.end ? W.end : kPoseEndIterations;
        }
        if (A.out_trial_chi2) {
            double* tc = A.out_trial_chi2 + ((size_t)T * b + trial) * 2;
            tc[0] = W.current_chi; tc[1] = W.lambda;
        }
        if (stop) break;
    }
    pose_pose_from_est(W.est, out);
    A.out_status[b] = PLP_POSE_OPT_OK;
    A.out_num_valid[b] = n - num_bad;
}
}  // namespace

plp_status plp_pose_optimize_device(plp_matcher* c, const plp_pose_optimize_args* a, void* hip_stream) {
    if (!c) return set_error(PLP_ERR_INVALID_ARG, "ctx is NULL");
    if (plp_status s = pose_check(a)) return s;
    if (a->B == 0) return PLP_OK;
    std::lock_guard<std::mutex> lk(c->mu);
    PLP_HIP(hipSetDevice(c->device));
    PoseArgs A = pose_args(a);
    const size_t B = (size_t)a->B, N = (size_t)a->n_cap, L = (size_t)a->l_cap;
    PLP_HIP(c->pose_slot.reserve((B * N + 1) * sizeof(uint16_t)));
    PLP_HIP(c->pose_slot_lines.reserve((B * L + 1) * sizeof(uint16_t)));
    PLP_HIP(c->pose_chi2.reserve((B * (N + L) + 1) * sizeof(double)));
    PLP_HIP(c->pose_n.reserve(B * 2 * sizeof(int32_t)));
    A.ctx_slot = (uint16_t*)c->pose_slot.p; A.ctx_slot_lines = (uint16_t*)c->pose_slot_lines.p; A.ctx_chi2 = (double*)c->pose_chi2.p; A.ctx_n = (int32_t*)c->pose_n.p;
    PLP_HIP(launch_pose_optimize((hipStream_t)hip_stream, A));
    return PLP_OK;
}

plp_status plp_pose_optimize_host(plp_matcher* c, const plp_pose_optimize_args* a) {
    if (!c) return set_error(PLP_ERR_INVALID_ARG, "ctx is NULL");
    if (plp_status s = pose_check(a)) return s;
    if (a->B == 0) return PLP_OK;
    const size_t B = (size_t)a->B, N = (size_t)a->n_cap, L = (size_t)a->l_cap, T = (size_t)a->num_trials;
    PoseArgs A = pose_args(a);
    std::lock_guard<std::mutex> lk(c->mu);
    PLP_HIP(hipSetDevice(c->device));
    Stage s(c->stage, c->stream);
    s.in(A.pose_in, (B - 1) * a->pose_stride + 12); s.in(A.counts, B); s.in(A.line_counts, B);
    s.in(A.valid, B * N); s.in(A.undist, B * N); s.in(A.x_right, B * N); s.in(A.pos_w, B * N * 3);
    s.in(A.line_valid, B * L); s.in(A.keylines, B * L); s.in(A.pos_w_lines, B * L * 6);
    s.out(A.out_status, B, false); s.out(A.out_pose, B * 15, false); s.out(A.out_num_init_obs, B, false); s.out(A.out_num_valid, B, false);
    s.out(A.out_outlier, B * N); s.out(A.out_outlier_lines, B * L); s.out(A.out_trial_info, B * T * 4, false); s.out(A.out_trial_chi2, B * T * 2, false);
    s.room(A.ctx_slot, B * N + 1); s.room(A.ctx_slot_lines, B * L + 1); s.room(A.ctx_chi2, B * (N + L) + 1); s.room(A.ctx_n, B * 2);
    PLP_TRY(s.upload());
    PLP_HIP(launch_pose_optimize(c->stream, A));
    return s.finish();
}

// the host builds of pose_opt.hpp (no HIP call)
int32_t plp_model_pose_optimize_host(const plp_pose_optimize_args* a) {
    if (plp_status s = pose_check(a)) return -(int32_t)s;
    const PoseArgs A = pose_args(a);
    for (int b = 0; b < A.B; ++b) pose_model_frame(A, b);
    return A.B;
}

int32_t plp_model_pose_linearize_host(const plp_pose_optimize_args* a, int32_t robust, const uint8_t* active, const uint8_t* active_lines,
                                      double* out_sums, double* out_chi2, double* out_chi2_lines) {
    if (plp_status s = pose_check(a)) return -(int32_t)s;
    if (a->B > 0 && !out_sums) return -(int32_t)set_error(PLP_ERR_INVALID_ARG, "out_sums is required");
    const PoseArgs A = pose_args(a);
    for (int b = 0; b < A.B; ++b) {
        PoseEdges E;
        pose_model_edges(A, b, A.l_cap > 0, E);
        for (size_t k = 0; k < E.slot.size(); ++k) E.level[k] = active && !active[(size_t)b * A.n_cap + E.slot[k]];
        for (size_t k = 0; k < E.lslot.size(); ++k) E.llevel[k] = active_lines && !active_lines[(size_t)b * A.l_cap + E.lslot[k]];
        PoseWork W{};
        pose_est_from_pose(A.pose_in + (size_t)b * A.pose_stride, W.est);
        pose_model_pass(A, b, W, E, robust != 0, true, out_sums + (size_t)kPoseTerms * b);
        if (out_chi2)
            for (size_t k = 0; k < E.slot.size(); ++k)
                if (!E.level[k]) out_chi2[(size_t)b * A.n_cap + E.slot[k]] = E.chi2[k];
        if (out_chi2_lines)
            for (size_t k = 0; k < E.lslot.size(); ++k)
                if (!E.llevel[k]) out_chi2_lines[(size_t)b * A.l_cap + E.lslot[k]] = E.lchi2[k];
    }
    return A.B;
}

int32_t plp_model_se3_exp_host(const double* update, const double* est, int32_t n, double* out) {
    if (n < 0 || (n > 0 && (!update || !est || !out))) return -1;
    for (int32_t i = 0; i < n; ++i) pose_oplus(update + 6 * (size_t)i, est + 7 * (size_t)i, out + 7 * (size_t)i);
    return n;
}

int32_t plp_model_chol6_host(const double* H, const double* b, const double* lambda, int32_t n, double* out_x, int32_t* out_ok) {
    if (n < 0 || (n > 0 && (!H || !b || !lambda || !out_x || !out_ok))) return -1;
    for (int32_t i = 0; i < n; ++i) {
        double Lf[36] = {0}, y[6] = {0};
        out_ok[i] = pose_chol6(H + 21 * (size_t)i, b + 6 * (size_t)i, lambda[i], Lf, y, out_x + 6 * (size_t)i) ? 1 : 0;
    }
    return n;
}

int32_t plp_model_pose_sincos_host(const double* x, int32_t n, double* out_sin, double* out_cos) {
    if (n < 0 || (n > 0 && (!x || !out_sin || !out_cos))) return -1;
    for (int32_t i = 0; i < n; ++i) pose_sincos(x[i], out_sin[i], out_cos[i]);
    return n;
}

// ---- Sim3 refinement of loop candidates: optimize::transform_optimizer (include/plp_front.h: plp_transform_optimize_*; transform_opt_kernels.hip, transform_opt.hpp)
namespace {
// outputs: the required output pointers too (the entries that optimise); false: the inputs alone (plp_model_transform_linearize_host writes none of them)
plp_status tf_check(const plp_transform_optimize_args* a, bool outputs = true) {
    if (!a) return set_error(PLP_ERR_INVALID_ARG, "NULL argument");
    if (a->camera.model != PLP_CAMERA_PERSPECTIVE && a->camera.model != PLP_CAMERA_FISHEYE && a->camera.model != PLP_CAMERA_EQUIRECTANGULAR)
        return set_error(PLP_ERR_INVALID_ARG, "unknown camera model");
    if (a->P < 0 || a->n_cap < 0) return set_error(PLP_ERR_INVALID_ARG, "P and n_cap must not be negative");
    if (a->num_iter < 1) return set_error(PLP_ERR_INVALID_ARG, "num_iter must be positive");
    if (!(a->chi_sq > 0.0f)) return set_error(PLP_ERR_INVALID_ARG, "chi_sq must be positive");
    if (a->num_levels < 1 || a->num_levels > 16 || !a->inv_level_sigma_sq_1 || !a->inv_level_sigma_sq_2)
        return set_error(PLP_ERR_INVALID_ARG, "num_levels must be 1 .. 16, inv_level_sigma_sq_1 and _2 are required");
    if (a->camera.model == PLP_CAMERA_EQUIRECTANGULAR) return set_error(PLP_ERR_UNSUPPORTED, "the equirectangular reprojection edges are not implemented (DESIGN.md D16)");
    if (!std::isfinite(a->camera.fx) || !std::isfinite(a->camera.fy) || !std::isfinite(a->camera.cx) || !std::isfinite(a->camera.cy) || a->camera.fx == 0 || a->camera.fy == 0)
        return set_error(PLP_ERR_INVALID_ARG, "fx, fy, cx, cy must be finite, fx and fy non-zero");
    if (a->n_cap > kTfMaxSlots) return set_error(PLP_ERR_UNSUPPORTED, "more than 8192 slots per problem");
    if (a->P > 65535) return set_error(PLP_ERR_UNSUPPORTED, "more than 65535 problems in one call");
    if (a->P == 0) return PLP_OK;
    if (!a->pose_1 || !a->pose_2 || !a->rot_12 || !a->trans_12 || !a->scale_12) return set_error(PLP_ERR_INVALID_ARG, "pose_1, pose_2, rot_12, trans_12, scale_12 are required");
    if (a->n_cap > 0 && (!a->valid || !a->pos_w_1 || !a->pos_w_2 || !a->undist_1 || !a->undist_2))
        return set_error(PLP_ERR_INVALID_ARG, "valid, pos_w_1, pos_w_2, undist_1, undist_2 are required");
    if (!outputs) return PLP_OK;
    if (!a->out_status || !a->out_num_valid || !a->out_num_inliers || !a->out_rot_12 || !a->out_trans_12 || !a->out_scale_12)
        return set_error(PLP_ERR_INVALID_ARG, "out_status, out_num_valid, out_num_inliers, out_rot_12, out_trans_12, out_scale_12 are required");
    if (a->n_cap > 0 && !a->out_kept) return set_error(PLP_ERR_INVALID_ARG, "out_kept is required");
    return PLP_OK;
}

TfArgs tf_args(const plp_transform_optimize_args* a) {
    TfArgs A{};
    A.P = a->P; A.n_cap = a->n_cap; A.num_iter = a->num_iter; A.fix_scale = a->fix_scale != 0; A.num_levels = a->num_levels;
    A.cam = pose_cam(a->camera.fx, a->camera.fy, a->camera.cx, a->camera.cy, 0.0);
    A.chi_sq = (double)a->chi_sq; A.delta = (double)std::sqrt(a->chi_sq);         // const float sqrt_chi_sq = std::sqrt(chi_sq)
    for (int l = 0; l < 16; ++l) {
        A.inv_sigma_sq_1[l] = l < A.num_levels ? a->inv_level_sigma_sq_1[l] : 0.0f;
        A.inv_sigma_sq_2[l] = l < A.num_levels ? a->inv_level_sigma_sq_2[l] : 0.0f;
    }
    A.counts = a->counts; A.valid = a->valid; A.pos_w_1 = a->pos_w_1; A.pos_w_2 = a->pos_w_2; A.undist_1 = a->undist_1; A.undist_2 = a->undist_2;
    A.pose_1 = a->pose_1; A.pose_2 = a->pose_2; A.rot_12 = a->rot_12; A.trans_12 = a->trans_12; A.scale_12 = a->scale_12;
    A.out_status = a->out_status; A.out_num_valid = a->out_num_valid; A.out_num_inliers = a->out_num_inliers; A.out_rot_12 = a->out_rot_12;
    A.out_trans_12 = a->out_trans_12; A.out_scale_12 = a->out_scale_12; A.out_world_to_1 = a->out_world_to_1; A.out_kept = a->out_kept;
    A.out_round_info = a->out_round_info; A.out_round_chi2 = a->out_round_chi2;
    return A;
}

// the matches of one problem of the host build, in rank order
struct TfEdges {
    std::vector<int> slot;
    std::vector<uint8_t> level;                 // 1 = dropped (both edges at level 1)
    std::vector<double> chi2;                   // [2 k] forward, [2 k + 1] backward: of the last evaluation
};
void tf_model_edges(const TfArgs& A, int p, TfEdges& E) {
    const size_t row = (size_t)p * A.n_cap;
    const int count = tf_count(A, p);
    for (int s = 0; s < count; ++s)
        if (tf_observation(A, row + s)) E.slot.push_back(s);
    E.level.assign(E.slot.size(), 0);
    E.chi2.assign(2 * E.slot.size(), 0.0);
}
// one pass over the kept matches: sums[36] at the linearisation W.sims / W.invs when lin, else sums[35] alone at entry 14
void tf_model_pass(const TfArgs& A, int p, TfWork& W, TfEdges& E, bool lin, double* sums) {
    for (int t = 0; t < kTfTerms; ++t) sums[t] = 0.0;
    double T[kTfTerms];
    for (size_t k = 0; k < E.slot.size(); ++k) {
        if (E.level[k]) continue;
        const size_t s = (size_t)p * A.n_cap + E.slot[k];
        for (int dir = 0; dir < 2; ++dir) {
            const plp_keypoint& kp = dir ? A.undist_2[s] : A.undist_1[s];
            const double w = (double)(dir ? A.inv_sigma_sq_2[kp.octave] : A.inv_sigma_sq_1[kp.octave]);
            const double* sims = dir ? W.invs : W.sims;
            double x, y, z;
            tf_to_camera((dir ? A.pose_1 : A.pose_2) + (size_t)15 * p, (dir ? A.pos_w_1 : A.pos_w_2) + 3 * s, x, y, z);
            if (lin) {
                E.chi2[2 * k + dir] = tf_edge_terms(sims, A.cam, x, y, z, (double)kp.x, (double)kp.y, w, A.delta, T, 1);
                for (int t = 0; t < kTfTerms; ++t) sums[t] = sums[t] + T[t];
            } else {
                double e0, e1, rho0, rho1;
                const double c = tf_edge_error(sims + 8 * 14, A.cam, x, y, z, (double)kp.x, (double)kp.y, w, e0, e1);
                pose_huber(c, A.delta, rho0, rho1);
                E.chi2[2 * k + dir] = c;
                sums[35] = sums[35] + rho0;
            }
        }
    }
}
void tf_model_linearize(const TfArgs& A, TfWork& W) {
    for (int i = 0; i < kTfSims; ++i) {
        tf_perturb(W.est, i, A.fix_scale != 0, W.sims + 8 * i);
        tf_inverse(W.sims + 8 * i, W.invs + 8 * i);
    }
}

// one problem of the host build: the kernels' steps, one edge after the other
void tf_model_problem(const TfArgs& A, int p) {
    const size_t row = (size_t)p * A.n_cap;
    TfEdges E;
    tf_model_edges(A, p, E);
    const int n = (int)E.slot.size();
    for (int s : E.slot) A.out_kept[row + s] = 1;
    if (A.out_round_info) for (int i = 0; i < 8; ++i) A.out_round_info[(size_t)8 * p + i] = 0;
    if (A.out_round_chi2) for (int i = 0; i < 4; ++i) A.out_round_chi2[(size_t)4 * p + i] = 0.0;
    TfWork W{};
    double est0[8];
    tf_est_from_input(A.rot_12 + (size_t)9 * p, A.trans_12 + (size_t)3 * p, A.scale_12[p], est0);
    for (int i = 0; i < 8; ++i) W.est[i] = est0[i];
    W.ni = 2.0;
    if (n == 0) { tf_write_result(A, p, est0, true, 0, 0); return; }
    const bool fix = A.fix_scale != 0;
    int left = n;
    double sums[kTfTerms];
    for (int round = 0; round < 2; ++round) {
        const int iters = tf_round_iters(round, A.num_iter);
        W.iterations = 0; W.rejected = 0; W.end = 0;
        for (int it = 0; it < iters; ++it) {
            tf_model_linearize(A, W);
            tf_model_pass(A, p, W, E, true, W.sum);
            tf_lm_begin(W, it);
            do {
                tf_lm_solve(W);
                tf_lm_update(W, fix);
                tf_model_pass(A, p, W, E, false, sums);
                tf_lm_decide(W, sums[35]);
            } while (W.go_on);
            W.iterations += 1;
            W.end = tf_lm_end(W);
            if (W.end) break;
        }
        int drops = 0;
        for (int k = 0; k < n; ++k) {
            if (E.level[k]) continue;
            if (tf_drop(round, A.chi_sq, E.chi2[2 * k], E.chi2[2 * k + 1])) {
                E.level[k] = 1; A.out_kept[row + E.slot[k]] = 0;
                ++drops;
            }
        }
        left -= drops;
        if (A.out_round_info) {
            int32_t* ri = A.out_round_info + (size_t)8 * p + 4 * round;
            ri[0] = W.iterations; ri[1] = W.rejected; ri[2] = drops; ri[3] = W.end ? W.end : kPoseEndIterations;
        }
        if (A.out_round_chi2) {
            double* rc = A.out_round_chi2 + (size_t)4 * p + 2 * round;
            rc[0] = W.current_chi; rc[1] = W.lambda;
        }
        if (round == 0 && left < kTfMinInliers) { tf_write_result(A, p, est0, true, n, 0); return; }
    }
    tf_write_result(A, p, W.est, false, n, left);
}
}  // namespace

plp_status plp_transform_optimize_device(plp_matcher* c, const plp_transform_optimize_args* a, void* hip_stream) {
    if (!c) return set_error(PLP_ERR_INVALID_ARG, "ctx is NULL");
    if (plp_status s = tf_check(a)) return s;
    if (a->P == 0) return PLP_OK;
    std::lock_guard<std::mutex> lk(c->mu);
    PLP_HIP(hipSetDevice(c->device));
    TfArgs A = tf_args(a);
    const size_t P = (size_t)a->P, N = (size_t)a->n_cap;
    PLP_HIP(c->tf_slot.reserve((P * N + 1) * sizeof(uint16_t)));
    PLP_HIP(c->tf_chi2.reserve((2 * P * N + kTfCtxDoubles * P) * sizeof(double)));
    PLP_HIP(c->tf_n.reserve(kTfCtxInts * P * sizeof(int32_t)));
    PLP_HIP(c->tf_level.reserve(P * N + 1));
    PLP_HIP(c->tf_edge.reserve((12 * P * N + 1) * sizeof(double)));
    A.ctx_slot = (uint16_t*)c->tf_slot.p; A.ctx_chi2 = (double*)c->tf_chi2.p; A.ctx_n = (int32_t*)c->tf_n.p;
    A.ctx_level = (uint8_t*)c->tf_level.p; A.ctx_edge = (double*)c->tf_edge.p;
    PLP_HIP(launch_transform_optimize((hipStream_t)hip_stream, A));
    return PLP_OK;
}

plp_status plp_transform_optimize_host(plp_matcher* c, const plp_transform_optimize_args* a) {
    if (!c) return set_error(PLP_ERR_INVALID_ARG, "ctx is NULL");
    if (plp_status s = tf_check(a)) return s;
    if (a->P == 0) return PLP_OK;
    const size_t P = (size_t)a->P, N = (size_t)a->n_cap;
    TfArgs A = tf_args(a);
    std::lock_guard<std::mutex> lk(c->mu);
    PLP_HIP(hipSetDevice(c->device));
    Stage s(c->stage, c->stream);
    s.in(A.counts, P); s.in(A.valid, P * N); s.in(A.pos_w_1, P * N * 3); s.in(A.pos_w_2, P * N * 3); s.in(A.undist_1, P * N); s.in(A.undist_2, P * N);
    s.in(A.pose_1, P * 15); s.in(A.pose_2, P * 15); s.in(A.rot_12, P * 9); s.in(A.trans_12, P * 3); s.in(A.scale_12, P);
    s.out(A.out_status, P, false); s.out(A.out_num_valid, P, false); s.out(A.out_num_inliers, P, false); s.out(A.out_rot_12, P * 9, false);
    s.out(A.out_trans_12, P * 3, false); s.out(A.out_scale_12, P, false); s.out(A.out_world_to_1, P * 13, false); s.out(A.out_kept, P * N);
    s.out(A.out_round_info, P * 8, false); s.out(A.out_round_chi2, P * 4, false);
    s.room(A.ctx_slot, P * N + 1); s.room(A.ctx_chi2, 2 * P * N + kTfCtxDoubles * P); s.room(A.ctx_n, kTfCtxInts * P); s.room(A.ctx_level, P * N + 1); s.room(A.ctx_edge, 12 * P * N + 1);
    PLP_TRY(s.upload());
    PLP_HIP(launch_transform_optimize(c->stream, A));
    return s.finish();
}

// the host builds of transform_opt.hpp (no HIP call)
int32_t plp_model_transform_optimize_host(const plp_transform_optimize_args* a) {
    if (plp_status s = tf_check(a)) return -(int32_t)s;
    const TfArgs A = tf_args(a);
    for (int p = 0; p < A.P; ++p) tf_model_problem(A, p);
    return A.P;
}

int32_t plp_model_transform_linearize_host(const plp_transform_optimize_args* a, const uint8_t* active, double* out_sums, double* out_chi2) {
    if (plp_status s = tf_check(a, false)) return -(int32_t)s;
    if (a->P > 0 && !out_sums) return -(int32_t)set_error(PLP_ERR_INVALID_ARG, "out_sums is required");
    const TfArgs A = tf_args(a);
    for (int p = 0; p < A.P; ++p) {
        TfEdges E;
        tf_model_edges(A, p, E);
        for (size_t k = 0; k < E.slot.size(); ++k) E.level[k] = active && !active[(size_t)p * A.n_cap + E.slot[k]];
        TfWork W{};
        tf_est_from_input(A.rot_12 + (size_t)9 * p, A.trans_12 + (size_t)3 * p, A.scale_12[p], W.est);
        tf_model_linearize(A, W);
        tf_model_pass(A, p, W, E, true, out_sums + (size_t)kTfTerms * p);
        if (out_chi2)
            for (size_t k = 0; k < E.slot.size(); ++k)
                if (!E.level[k]) {
                    out_chi2[2 * ((size_t)p * A.n_cap + E.slot[k])] = E.chi2[2 * k];
                    out_chi2[2 * ((size_t)p * A.n_cap + E.slot[k]) + 1] = E.chi2[2 * k + 1];
                }
    }
    return A.P;
}

int32_t plp_model_sim3_exp_host(const double* update, const double* est, int32_t fix_scale, int32_t n, double* out) {
    if (n < 0 || (n > 0 && (!update || !est || !out))) return -1;
    for (int32_t i = 0; i < n; ++i) tf_oplus(update + 7 * (size_t)i, fix_scale != 0, est + 8 * (size_t)i, out + 8 * (size_t)i);
    return n;
}

int32_t plp_model_chol7_host(const double* H, const double* b, const double* lambda, int32_t n, double* out_x, int32_t* out_ok) {
    if (n < 0 || (n > 0 && (!H || !b || !lambda || !out_x || !out_ok))) return -1;
    for (int32_t i = 0; i < n; ++i) {
        double Lf[49] = {0}, y[7] = {0};
        out_ok[i] = tf_chol7(H + 28 * (size_t)i, b + 7 * (size_t)i, lambda[i], Lf, y, out_x + 7 * (size_t)i) ? 1 : 0;
    }
    return n;
}

int32_t plp_model_pose_exp_host(const double* x, int32_t n, double* out) {
    if (n < 0 || (n > 0 && (!x || !out))) return -1;
    for (int32_t i = 0; i < n; ++i) out[i] = pose_exp(x[i]);
    return n;
}

// ---- local bundle adjustment: optimize::local_bundle_adjuster (include/plp_front.h: plp_local_ba_*; local_ba_kernels.hip, local_ba.hpp)
namespace {
// host: the arrays are host memory, so the observation list and the number of free key frames are checked as well
plp_status la_check(const plp_local_ba_args* a, bool outputs, bool host) {
    if (!a) return set_error(PLP_ERR_INVALID_ARG, "NULL argument");
    if (a->camera.model != PLP_CAMERA_PERSPECTIVE && a->camera.model != PLP_CAMERA_FISHEYE && a->camera.model != PLP_CAMERA_EQUIRECTANGULAR)
        return set_error(PLP_ERR_INVALID_ARG, "unknown camera model");
    if (a->setup_type < 0 || a->setup_type > 2) return set_error(PLP_ERR_INVALID_ARG, "setup_type must be 0, 1 or 2");
    if (a->G < 0 || a->F < 0 || a->L < 0 || a->T < 0 || a->kp_stride < 0) return set_error(PLP_ERR_INVALID_ARG, "G, F, L, T and kp_stride must not be negative");
    if (a->num_first_iter < 1 || a->num_second_iter < 1) return set_error(PLP_ERR_INVALID_ARG, "num_first_iter and num_second_iter must be positive");
    if (a->pose_stride < 12) return set_error(PLP_ERR_INVALID_ARG, "pose_stride must be at least 12");
    if (a->num_levels < 1 || a->num_levels > 16 || !a->inv_level_sigma_sq) return set_error(PLP_ERR_INVALID_ARG, "num_levels must be 1 .. 16, inv_level_sigma_sq is required");
    if (a->camera.model == PLP_CAMERA_EQUIRECTANGULAR) return set_error(PLP_ERR_UNSUPPORTED, "the equirectangular reprojection edge is not implemented (DESIGN.md D17)");
    if (!std::isfinite(a->camera.fx) || !std::isfinite(a->camera.fy) || !std::isfinite(a->camera.cx) || !std::isfinite(a->camera.cy) || a->camera.fx == 0 || a->camera.fy == 0)
        return set_error(PLP_ERR_INVALID_ARG, "fx, fy, cx, cy must be finite, fx and fy non-zero");
    if (a->F > kLaMaxKf) return set_error(PLP_ERR_UNSUPPORTED, "more than 1024 key frames in the table");
    if (a->L > kLaMaxObs || a->T > kLaMaxObs) return set_error(PLP_ERR_UNSUPPORTED, "more than 2^18 landmarks or observations");
    if (a->G > kLaMaxProblems || (long long)a->G * a->T > kLaMaxWork || (long long)a->G * a->L > kLaMaxWork)
        return set_error(PLP_ERR_UNSUPPORTED, "more than 256 problems, or G * T or G * L above 2^22");
    if (a->G == 0) return PLP_OK;
    if (!a->obs_offsets) return set_error(PLP_ERR_INVALID_ARG, "obs_offsets is required");
    if (a->F > 0 && (!a->kf_local || !a->pose || (a->kp_stride > 0 && !a->undist))) return set_error(PLP_ERR_INVALID_ARG, "kf_local, pose and undist are required");
    if (a->L > 0 && !a->pos_w) return set_error(PLP_ERR_INVALID_ARG, "pos_w is required");
    if (a->T > 0 && (!a->obs_kf || !a->obs_idx)) return set_error(PLP_ERR_INVALID_ARG, "obs_kf and obs_idx are required");
    if (outputs) {
        if (!a->out_status || (a->F > 0 && (!a->out_kf_role || !a->out_pose)) || (a->L > 0 && (!a->out_lm_role || !a->out_pos_w)) || (a->T > 0 && !a->out_outlier))
            return set_error(PLP_ERR_INVALID_ARG, "out_status, out_kf_role, out_lm_role, out_pose, out_pos_w, out_outlier are required");
    }
    if (host) {
        if (a->obs_offsets[0] != 0 || a->obs_offsets[a->L] != a->T) return set_error(PLP_ERR_INVALID_ARG, "obs_offsets must rise from 0 to T");
        for (int l = 0; l < a->L; ++l)
            if (a->obs_offsets[l + 1] < a->obs_offsets[l]) return set_error(PLP_ERR_INVALID_ARG, "obs_offsets must rise from 0 to T");
        for (int g = 0; g < a->G; ++g) {
            int n = 0;
            for (int f = 0; f < a->F; ++f)
                n += a->kf_local[(size_t)g * a->F + f] && !(a->kf_erased && a->kf_erased[f]) && !(a->kf_is_origin && a->kf_is_origin[f]);
            if (n > kLaMaxFree) return set_error(PLP_ERR_UNSUPPORTED, "more than 64 free key frames in a problem");
        }
    }
    return PLP_OK;
}

LaArgs la_args(const plp_local_ba_args* a) {
    LaArgs A{};
    A.G = a->G; A.F = a->F; A.L = a->L; A.T = a->T; A.kp_stride = a->kp_stride; A.pose_stride = a->pose_stride; A.num_levels = a->num_levels;
    A.mono_setup = a->setup_type == 0; A.it1 = a->num_first_iter; A.it2 = a->num_second_iter;
    A.cam = pose_cam(a->camera.fx, a->camera.fy, a->camera.cx, a->camera.cy, a->camera.focal_x_baseline);
    A.delta_2d = (double)std::sqrt(kPoseChiSq2D); A.delta_3d = (double)std::sqrt(kPoseChiSq3D);
    for (int l = 0; l < 16; ++l) A.inv_sigma_sq[l] = l < A.num_levels ? a->inv_level_sigma_sq[l] : 0.0f;
    A.pose = a->pose; A.kf_erased = a->kf_erased; A.kf_is_origin = a->kf_is_origin; A.undist = a->undist; A.x_right = a->x_right; A.counts = a->counts;
    A.pos_w = a->pos_w; A.lm_erased = a->lm_erased; A.obs_offsets = a->obs_offsets; A.obs_kf = a->obs_kf; A.obs_idx = a->obs_idx; A.kf_local = a->kf_local;
    A.out_status = a->out_status; A.out_kf_role = a->out_kf_role; A.out_lm_role = a->out_lm_role; A.out_pose = a->out_pose; A.out_pos_w = a->out_pos_w;
    A.out_outlier = a->out_outlier; A.out_round_info = a->out_round_info; A.out_round_chi2 = a->out_round_chi2;
    return A;
}

// the state of the host builds: one problem's worth
struct LaHostCtx {
    std::vector<double> d; std::vector<int32_t> i; std::vector<uint8_t> b;
    void bind(LaArgs& A) {
        d.assign(la_doubles(A.F, A.L, A.T), 0.0); i.assign(la_ints(A.T), 0); b.assign(la_bytes(A.F, A.L, A.T) + 1, 0);
        A.ctx_d = d.data(); A.ctx_i = i.data(); A.ctx_b = b.data();
    }
};
// problem g of A with a context that holds one problem: the tables are shared, the per-problem arrays shifted
LaArgs la_one(const LaArgs& A, int g) {
    LaArgs B = A;
    B.G = 1;
    B.kf_local = A.kf_local ? A.kf_local + (size_t)g * A.F : nullptr;
    B.out_status = A.out_status ? A.out_status + g : nullptr;
    B.out_kf_role = A.out_kf_role ? A.out_kf_role + (size_t)g * A.F : nullptr;
    B.out_lm_role = A.out_lm_role ? A.out_lm_role + (size_t)g * A.L : nullptr;
    B.out_pose = A.out_pose ? A.out_pose + (size_t)g * A.F * 15 : nullptr;
    B.out_pos_w = A.out_pos_w ? A.out_pos_w + (size_t)g * A.L * 3 : nullptr;
    B.out_outlier = A.out_outlier ? A.out_outlier + (size_t)g * A.T : nullptr;
    B.out_round_info = A.out_round_info ? A.out_round_info + (size_t)g * 8 : nullptr;
    B.out_round_chi2 = A.out_round_chi2 ? A.out_round_chi2 + (size_t)g * 4 : nullptr;
    return B;
}
}  // namespace

plp_status plp_local_ba_device(plp_matcher* c, const plp_local_ba_args* a, void* hip_stream) {
    if (!c) return set_error(PLP_ERR_INVALID_ARG, "ctx is NULL");
    if (plp_status s = la_check(a, true, false)) return s;
    if (a->G == 0) return PLP_OK;
    std::lock_guard<std::mutex> lk(c->mu);
    PLP_HIP(hipSetDevice(c->device));
    LaArgs A = la_args(a);
    const size_t G = (size_t)a->G;
    PLP_HIP(c->la_d.reserve(G * la_doubles(A.F, A.L, A.T) * sizeof(double)));
    PLP_HIP(c->la_i.reserve(G * la_ints(A.T) * sizeof(int32_t)));
    PLP_HIP(c->la_b.reserve(G * la_bytes(A.F, A.L, A.T) + 16));
    A.ctx_d = (double*)c->la_d.p; A.ctx_i = (int32_t*)c->la_i.p; A.ctx_b = (uint8_t*)c->la_b.p;
    PLP_HIP(launch_local_ba((hipStream_t)hip_stream, A));
    return PLP_OK;
}

plp_status plp_local_ba_host(plp_matcher* c, const plp_local_ba_args* a) {
    if (!c) return set_error(PLP_ERR_INVALID_ARG, "ctx is NULL");
    if (plp_status s = la_check(a, true, true)) return s;
    if (a->G == 0) return PLP_OK;
    LaArgs A = la_args(a);
    const size_t G = (size_t)a->G, F = (size_t)a->F, L = (size_t)a->L, T = (size_t)a->T, K = (size_t)a->kp_stride;
    std::lock_guard<std::mutex> lk(c->mu);
    PLP_HIP(hipSetDevice(c->device));
    Stage s(c->stage, c->stream);
    s.in(A.pose, F * a->pose_stride); s.in(A.kf_erased, F); s.in(A.kf_is_origin, F); s.in(A.undist, F * K); s.in(A.x_right, F * K); s.in(A.counts, F);
    s.in(A.pos_w, L * 3); s.in(A.lm_erased, L); s.in(A.obs_offsets, L + 1); s.in(A.obs_kf, T); s.in(A.obs_idx, T); s.in(A.kf_local, G * F);
    s.out(A.out_status, G); s.out(A.out_kf_role, G * F); s.out(A.out_lm_role, G * L); s.out(A.out_pose, G * F * 15); s.out(A.out_pos_w, G * L * 3);
    s.out(A.out_outlier, G * T); s.out(A.out_round_info, G * 8); s.out(A.out_round_chi2, G * 4);
    s.room(A.ctx_d, G * la_doubles(A.F, A.L, A.T)); s.room(A.ctx_i, G * la_ints(A.T)); s.room(A.ctx_b, G * la_bytes(A.F, A.L, A.T) + 16);
    PLP_TRY(s.upload());
    PLP_HIP(launch_local_ba(c->stream, A));
    return s.finish();
}

// the host builds of local_ba.hpp (no HIP call)
int32_t plp_model_local_ba_host(const plp_local_ba_args* a) {
    if (plp_status s = la_check(a, true, true)) return -(int32_t)s;
    const LaArgs A = la_args(a);
    for (int g = 0; g < A.G; ++g) {
        LaArgs B = la_one(A, g);
        LaHostCtx ctx;
        ctx.bind(B);
        LaShared sh{};
        LaTeamHost par;
        la_prepare(B, 0, sh, par);
        la_solve(B, 0, sh, par);
        la_finish(B, 0, par);
    }
    return A.G;
}

int32_t plp_model_local_ba_linearize_host(const plp_local_ba_args* a, int32_t robust, int32_t* out_free_kf, double* out_hpp, double* out_hll, double* out_w,
                                          double* out_chi2, double* out_edge_chi2) {
    if (plp_status s = la_check(a, false, true)) return -(int32_t)s;
    if (a->G != 1) return -(int32_t)set_error(PLP_ERR_INVALID_ARG, "G must be 1");
    LaArgs B = la_args(a);
    LaHostCtx ctx;
    ctx.bind(B);
    LaShared sh{};
    LaTeamHost par;
    la_prepare(B, 0, sh, par);
    LaOff O;
    la_offsets(B, 0, O);
    const LaView V = la_view(B, O);
    if (out_free_kf) for (int i = 0; i < kLaMaxFree; ++i) out_free_kf[i] = -1;
    if (V.hdr()[kLaHStatus] != PLP_LOCAL_BA_OK) { if (out_chi2) out_chi2[0] = 0.0; return 0; }
    sh.cam = B.cam; sh.delta = B.mono_setup ? B.delta_2d : B.delta_3d;
    la_round_setup(B, V, sh, par);
    la_edge_pass(B, V, sh, par, true, robust != 0);
    la_sums(B, V, sh, par, true);
    sh.acc = 0.0;
    la_chain(B, V, sh, par, 0, kLaLmPart);
    if (out_chi2) out_chi2[0] = sh.acc;
    for (int i = 0; i < sh.nfa; ++i) {
        if (out_free_kf) out_free_kf[i] = sh.akf[i];
        if (out_hpp) for (int t = 0; t < 27; ++t) out_hpp[27 * i + t] = la_p(V, i, t);
    }
    for (int l = 0; l < B.L; ++l)
        if (out_hll && V.lm_act()[l]) for (int t = 0; t < 9; ++t) out_hll[(size_t)9 * l + t] = la_l(V, l, kLaLmH + t);
    for (int t = 0; t < B.T; ++t) {
        if (V.e_kf()[t] < 0) continue;
        if (out_edge_chi2) out_edge_chi2[t] = la_e(V, t, kLaRowChi);
        if (out_w && sh.kf2ai[V.e_kf()[t]] >= 0) for (int k = 0; k < 18; ++k) out_w[(size_t)18 * t + k] = la_e(V, t, kLaRowW + k);
    }
    return sh.nfa;
}

int32_t plp_model_local_ba_solve_host(int32_t P, int32_t M, int32_t E, const double* hpp, const double* hll, const int32_t* e_pose, const int32_t* e_lm,
                                      const double* w, double lambda, double* out_xp, double* out_xl) {
    if (P < 0 || P > kLaMaxFree || M < 0 || M > kLaMaxObs || E < 0 || E > kLaMaxObs || (P > 0 && (!hpp || !out_xp)) || (M > 0 && (!hll || !out_xl)) ||
        (E > 0 && (!e_pose || !e_lm || !w))) return -1;
    for (int e = 0; e < E; ++e)
        if (e_pose[e] < -1 || e_pose[e] >= P || e_lm[e] < 0 || e_lm[e] >= M || (e > 0 && e_lm[e] < e_lm[e - 1])) return -1;
    // the blocks as a problem of P + 1 key frames (row P: the constant pose), M landmarks and E observations
    LaArgs B{};
    B.G = 1; B.F = P + 1; B.L = M; B.T = E;
    std::vector<int32_t> off(M + 1, 0);
    for (int e = 0; e < E; ++e) off[e_lm[e] + 1] += 1;
    for (int l = 0; l < M; ++l) off[l + 1] += off[l];
    B.obs_offsets = off.data();
    LaHostCtx ctx;
    ctx.bind(B);
    LaShared sh{};
    LaTeamHost par;
    LaOff O;
    la_offsets(B, 0, O);
    const LaView V = la_view(B, O);
    V.hdr()[kLaHNf] = P;
    for (int i = 0; i < P; ++i) V.hdr()[kLaHFl + i] = i;
    for (int l = 0; l < M; ++l) V.lm_role()[l] = 1;
    for (int e = 0; e < E; ++e) { V.e_kf()[e] = e_pose[e] < 0 ? P : e_pose[e]; V.e_l()[e] = e_lm[e]; V.lvl()[e] = 0; }
    la_round_setup(B, V, sh, par);
    for (int i = 0; i < sh.nfa; ++i) for (int t = 0; t < 27; ++t) la_p(V, i, t) = hpp[27 * sh.akf[i] + t];
    for (int l = 0; l < M; ++l) for (int t = 0; t < 9; ++t) la_l(V, l, kLaLmH + t) = hll[(size_t)9 * l + t];
    for (int e = 0; e < E; ++e) for (int k = 0; k < 18; ++k) la_e(V, e, kLaRowW + k) = w[(size_t)18 * e + k];
    sh.lambda = lambda;
    la_solve_system(B, V, sh, par);
    for (int i = 0; i < 6 * P; ++i) out_xp[i] = 0.0;
    for (int i = 0; i < sh.nfa; ++i) for (int k = 0; k < 6; ++k) out_xp[6 * sh.akf[i] + k] = sh.x[6 * i + k];
    for (int l = 0; l < M; ++l) for (int k = 0; k < 3; ++k) out_xl[(size_t)3 * l + k] = V.lm_act()[l] ? la_l(V, l, kLaLmX + k) : 0.0;
    return sh.ok ? 1 : 0;
}

int32_t plp_model_inv3_host(const double* a, int32_t n, double* out, int32_t* out_ok) {
    if (n < 0 || (n > 0 && (!a || !out || !out_ok))) return -1;
    for (int32_t i = 0; i < n; ++i) out_ok[i] = la_inv3(a + 6 * (size_t)i, out + 6 * (size_t)i) ? 1 : 0;
    return n;
}

// ---- the local map: module::local_map_updater (include/plp_front.h: plp_local_map_*; local_map_kernels.hip, local_map.hpp)
namespace {
// host: the arrays are host memory, so the two offset tables are checked as well
plp_status lm_check(const plp_local_map_args* a, bool host) {
    if (!a) return set_error(PLP_ERR_INVALID_ARG, "NULL argument");
    if (a->B < 0 || a->F < 0 || a->C < 0 || a->L < 0 || a->LL < 0 || a->T < 0 || a->cap < 0 || a->lcap < 0 || a->fcap < 0 || a->flcap < 0)
        return set_error(PLP_ERR_INVALID_ARG, "B, F, C, L, LL, T, cap, lcap, fcap and flcap must not be negative");
    if (a->frm_stride < 0 || a->frm_stride_lines < 0 || (a->frm_stride && a->frm_stride < a->fcap) || (a->frm_stride_lines && a->frm_stride_lines < a->flcap))
        return set_error(PLP_ERR_INVALID_ARG, "frm_stride and frm_stride_lines must be 0 or at least fcap and flcap");
    if (a->max_num_local_keyfrms < 0 || a->workspace_bytes < 0) return set_error(PLP_ERR_INVALID_ARG, "max_num_local_keyfrms and workspace_bytes must not be negative");
    if (a->k_cap < 0 || a->m_cap < 0 || a->ml_cap < 0) return set_error(PLP_ERR_INVALID_ARG, "k_cap, m_cap and ml_cap must not be negative");
    if (a->F > kLmMaxKf) return set_error(PLP_ERR_UNSUPPORTED, "more than 8192 key frames: the weights of a frame are an LDS table");
    if (a->cap > kLmMaxSlots || a->lcap > kLmMaxSlots || a->fcap > kLmMaxSlots || a->flcap > kLmMaxSlots)
        return set_error(PLP_ERR_UNSUPPORTED, "more than 8192 slots per row");
    if (a->B > kLmMaxFrames) return set_error(PLP_ERR_UNSUPPORTED, "more than 65535 frames");
    if ((long long)a->k_cap * std::max(a->cap, a->lcap) >= (1ll << 31)) return set_error(PLP_ERR_UNSUPPORTED, "k_cap * max(cap, lcap) must stay below 2^31");
    if (a->B == 0) return PLP_OK;
    const bool lines = a->kf_lm_lines != nullptr;
    if (!a->kf_covis && a->F > 0) return set_error(PLP_ERR_INVALID_ARG, "kf_covis is required");
    if (!a->kf_parent && a->F > 0) return set_error(PLP_ERR_INVALID_ARG, "kf_parent is required");
    if (!a->kf_children_offsets || (a->C > 0 && !a->kf_children)) return set_error(PLP_ERR_INVALID_ARG, "kf_children_offsets and kf_children are required");
    if (a->F > 0 && a->cap > 0 && !a->kf_lm) return set_error(PLP_ERR_INVALID_ARG, "kf_lm is required");
    if (!a->obs_offsets || (a->T > 0 && !a->obs_kf)) return set_error(PLP_ERR_INVALID_ARG, "obs_offsets and obs_kf are required");
    if (a->fcap > 0 && !a->frm_lm) return set_error(PLP_ERR_INVALID_ARG, "frm_lm is required");
    if (!a->out_status || !a->out_num_first || !a->out_num_kf || !a->out_nearest_kf || !a->out_num_lm || (a->k_cap > 0 && !a->out_local_kf) ||
        (a->m_cap > 0 && (!a->out_local_lm || !a->out_held)))
        return set_error(PLP_ERR_INVALID_ARG, "out_status, out_num_first, out_num_kf, out_local_kf, out_nearest_kf, out_num_lm, out_local_lm, out_held are required");
    if (lines && (!a->out_num_lines || (a->ml_cap > 0 && (!a->out_local_lines || !a->out_held_lines))))
        return set_error(PLP_ERR_INVALID_ARG, "out_num_lines, out_local_lines, out_held_lines are required with kf_lm_lines");
    if (host) {
        if (a->obs_offsets[0] != 0 || a->obs_offsets[a->L] != a->T) return set_error(PLP_ERR_INVALID_ARG, "obs_offsets must rise from 0 to T");
        for (int l = 0; l < a->L; ++l)
            if (a->obs_offsets[l + 1] < a->obs_offsets[l]) return set_error(PLP_ERR_INVALID_ARG, "obs_offsets must rise from 0 to T");
        if (a->kf_children_offsets[0] != 0 || a->kf_children_offsets[a->F] != a->C) return set_error(PLP_ERR_INVALID_ARG, "kf_children_offsets must rise from 0 to C");
        for (int f = 0; f < a->F; ++f)
            if (a->kf_children_offsets[f + 1] < a->kf_children_offsets[f]) return set_error(PLP_ERR_INVALID_ARG, "kf_children_offsets must rise from 0 to C");
    }
    return PLP_OK;
}

LmArgs lm_args(const plp_local_map_args* a) {
    LmArgs A{};
    A.lines = a->kf_lm_lines != nullptr;
    A.B = a->B; A.F = a->F; A.C = a->C; A.L = a->L; A.LL = A.lines ? a->LL : 0; A.T = a->T; A.cap = a->cap; A.lcap = a->lcap; A.fcap = a->fcap; A.flcap = a->flcap;
    A.frm_stride = a->frm_stride ? a->frm_stride : a->fcap; A.frm_stride_lines = a->frm_stride_lines ? a->frm_stride_lines : a->flcap;
    A.max_kf = a->max_num_local_keyfrms; A.k_cap = a->k_cap; A.m_cap = a->m_cap; A.ml_cap = a->ml_cap;
    A.kf_erased = a->kf_erased; A.kf_covis = a->kf_covis; A.kf_parent = a->kf_parent; A.kf_children_offsets = a->kf_children_offsets; A.kf_children = a->kf_children;
    A.kf_lm = a->kf_lm; A.kf_counts = a->kf_counts; A.kf_lm_lines = a->kf_lm_lines; A.kf_kl_counts = a->kf_kl_counts;
    A.obs_offsets = a->obs_offsets; A.obs_kf = a->obs_kf; A.lm_erased = a->lm_erased; A.lm_erased_lines = a->lm_erased_lines;
    A.frm_lm = a->frm_lm; A.frm_counts = a->frm_counts; A.frm_lm_lines = a->frm_lm_lines; A.frm_kl_counts = a->frm_kl_counts;
    A.out_status = a->out_status; A.out_num_first = a->out_num_first; A.out_num_kf = a->out_num_kf; A.out_local_kf = a->out_local_kf;
    A.out_first_weight = a->out_first_weight; A.out_nearest_kf = a->out_nearest_kf; A.out_num_lm = a->out_num_lm; A.out_local_lm = a->out_local_lm;
    A.out_held = a->out_held; A.out_num_lines = a->out_num_lines; A.out_local_lines = a->out_local_lines; A.out_held_lines = a->out_held_lines;
    A.ws_rows = lm_ws_rows(A.L, A.LL); A.ws_words = lm_ws_words(A.L, A.LL);
    return A;
}

// frames per chunk: as many mark-table rows as fit workspace_bytes, at least one
int lm_chunk(const plp_local_map_args* a, const LmArgs& A) {
    const size_t per = lm_ws_frame_bytes(A.L, A.LL);
    const size_t room = a->workspace_bytes ? (size_t)a->workspace_bytes : (size_t)kLmDefaultWorkspace;
    const size_t n = per ? std::max<size_t>(room / per, 1) : (size_t)A.B;
    return (int)std::min<size_t>(n, (size_t)A.B);
}

// every launch of a call; A.ws holds nc frames
plp_status lm_run_device(hipStream_t st, LmArgs A, int nc) {
    PLP_HIP(launch_local_map_keyframes(st, A));
    for (int b0 = 0; b0 < A.B; b0 += nc) {
        A.b0 = b0; A.nb = std::min(nc, A.B - b0);
        PLP_HIP(launch_local_map_lists(st, A, false));
        if (A.lines) PLP_HIP(launch_local_map_lists(st, A, true));
    }
    return PLP_OK;
}
}  // namespace

plp_status plp_local_map_device(plp_matcher* c, const plp_local_map_args* a, void* hip_stream) {
    if (!c) return set_error(PLP_ERR_INVALID_ARG, "ctx is NULL");
    if (plp_status s = lm_check(a, false)) return s;
    if (a->B == 0) return PLP_OK;
    std::lock_guard<std::mutex> lk(c->mu);
    PLP_HIP(hipSetDevice(c->device));
    LmArgs A = lm_args(a);
    const int nc = lm_chunk(a, A);
    PLP_HIP(c->lm_ws.reserve((size_t)nc * lm_ws_frame_bytes(A.L, A.LL)));
    A.ws = (uint32_t*)c->lm_ws.p;
    return lm_run_device((hipStream_t)hip_stream, A, nc);
}

plp_status plp_local_map_host(plp_matcher* c, const plp_local_map_args* a) {
    if (!c) return set_error(PLP_ERR_INVALID_ARG, "ctx is NULL");
    if (plp_status s = lm_check(a, true)) return s;
    if (a->B == 0) return PLP_OK;
    LmArgs A = lm_args(a);
    const int nc = lm_chunk(a, A);
    const size_t B = (size_t)A.B, F = (size_t)A.F;
    std::lock_guard<std::mutex> lk(c->mu);
    PLP_HIP(hipSetDevice(c->device));
    Stage s(c->stage, c->stream);
    s.in(A.kf_erased, F); s.in(A.kf_covis, F * kLmCovis); s.in(A.kf_parent, F); s.in(A.kf_children_offsets, F + 1); s.in(A.kf_children, (size_t)A.C);
    s.in(A.kf_lm, F * A.cap); s.in(A.kf_counts, F); s.in(A.kf_lm_lines, F * A.lcap); s.in(A.kf_kl_counts, F);
    s.in(A.obs_offsets, (size_t)A.L + 1); s.in(A.obs_kf, (size_t)A.T); s.in(A.lm_erased, (size_t)A.L); s.in(A.lm_erased_lines, (size_t)A.LL);
    s.in(A.frm_lm, B * A.frm_stride); s.in(A.frm_counts, B); s.in(A.frm_lm_lines, B * A.frm_stride_lines); s.in(A.frm_kl_counts, B);
    s.out(A.out_status, B); s.out(A.out_num_first, B); s.out(A.out_num_kf, B); s.out(A.out_local_kf, B * A.k_cap); s.out(A.out_first_weight, B * A.k_cap);
    s.out(A.out_nearest_kf, B); s.out(A.out_num_lm, B); s.out(A.out_local_lm, B * A.m_cap); s.out(A.out_held, B * A.m_cap);
    if (A.lines) { s.out(A.out_num_lines, B); s.out(A.out_local_lines, B * A.ml_cap); s.out(A.out_held_lines, B * A.ml_cap); }
    s.room(A.ws, (size_t)nc * lm_ws_frame_bytes(A.L, A.LL) / 4);
    PLP_TRY(s.upload());
    PLP_TRY(lm_run_device(c->stream, A, nc));
    return s.finish();
}

// the host build of local_map.hpp (no HIP call): one frame's mark table at a time
int32_t plp_model_local_map_host(const plp_local_map_args* a) {
    if (plp_status s = lm_check(a, true)) return -(int32_t)s;
    LmArgs A = lm_args(a);
    std::vector<uint32_t> ws((size_t)A.ws_rows + A.ws_words + 1);
    std::vector<LmShared> shared(1);
    A.ws = ws.data(); A.nb = 1;
    LmTeamHost par;
    const int kb = lm_mark_blocks(A.k_cap, A.F);
    for (int b = 0; b < A.B; ++b) {
        A.b0 = b;
        lm_keyframes(A, b, shared[0], par);
        for (int side = 0; side < (A.lines ? 2 : 1); ++side) {
            std::fill(ws.begin(), ws.begin() + A.ws_rows, 0xFFFFFFFFu);
            std::fill(ws.begin() + A.ws_rows, ws.end(), 0u);
            LmSharedCompact sc{};
            for (int k = 0; k <= kb; ++k) {
                if (side) lm_mark<true>(A, 0, k, par); else lm_mark<false>(A, 0, k, par);
            }
            if (side) lm_compact<true>(A, 0, sc, par); else lm_compact<false>(A, 0, sc, par);
        }
    }
    return A.B;
}

plp_status plp_convert_to_grayscale_device(plp_matcher* c, const uint8_t* d_src, int32_t rows, int32_t cols, size_t src_step,
                                           size_t src_frame_stride, int32_t channels, int32_t color_order, int32_t B, uint8_t* d_gray,
                                           size_t gray_step, size_t gray_frame_stride, void* hip_stream) {
    if (!c || !d_src || !d_gray) return set_error(PLP_ERR_INVALID_ARG, "NULL argument");
    if (rows <= 0 || cols <= 0 || B <= 0 || (channels != 3 && channels != 4) || (color_order != 0 && color_order != 1) ||
        src_step < (size_t)cols * channels || gray_step < (size_t)cols) return set_error(PLP_ERR_INVALID_ARG, "bad geometry");
    std::lock_guard<std::mutex> lk(c->mu);
    PLP_HIP(hipSetDevice(c->device));
    launch_to_gray((hipStream_t)hip_stream, d_src, rows, cols, src_step, src_frame_stride, channels, color_order, B, d_gray,
                   gray_step, gray_frame_stride);
    PLP_HIP(hipGetLastError());
    return PLP_OK;
}

plp_status plp_convert_to_true_depth_device(plp_matcher* c, const void* d_src, int32_t src_is_u16, int32_t rows, int32_t cols, size_t src_step,
                                            size_t src_frame_stride, double depthmap_factor, int32_t B, float* d_dst, size_t dst_step,
                                            size_t dst_frame_stride, void* hip_stream) {
    if (!c || !d_src || !d_dst) return set_error(PLP_ERR_INVALID_ARG, "NULL argument");
    if (rows <= 0 || cols <= 0 || B <= 0 || src_step < (size_t)cols * (src_is_u16 ? 2 : 4) || dst_step < (size_t)cols * 4)
        return set_error(PLP_ERR_INVALID_ARG, "bad geometry");
    std::lock_guard<std::mutex> lk(c->mu);
    PLP_HIP(hipSetDevice(c->device));
    launch_to_depth((hipStream_t)hip_stream, d_src, src_is_u16 != 0, rows, cols, src_step, src_frame_stride,
                    (float)(1.0 / depthmap_factor), B, d_dst, dst_step, dst_frame_stride);
    PLP_HIP(hipGetLastError());
    return PLP_OK;
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
    std::lock_guard<std::mutex> lk(c->mu);
    PLP_HIP(hipSetDevice(c->device));
    launch_rectify_map((hipStream_t)hip_stream, A, fisheye);
    PLP_HIP(hipGetLastError());
    return PLP_OK;
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
    std::lock_guard<std::mutex> lk(c->mu);
    PLP_HIP(hipSetDevice(c->device));
    launch_remap_linear((hipStream_t)hip_stream, d_src, rows, cols, src_step, src_frame_stride, d_map_x, d_map_y, map_step, dst_rows, dst_cols, B, d_dst,
                        dst_step, dst_frame_stride);
    PLP_HIP(hipGetLastError());
    return PLP_OK;
}

plp_status plp_color_vote_device(plp_matcher* c, const uint8_t* d_mask, int32_t rows, int32_t cols, size_t mask_step,
                                 size_t mask_frame_stride, const plp_keypoint* d_undist, const uint8_t* d_valid, const int32_t* d_counts,
                                 int32_t cap, int32_t B, int32_t check_3x3_window, int32_t* d_labels, void* hip_stream) {
    if (!c || !d_mask || !d_undist || !d_labels) return set_error(PLP_ERR_INVALID_ARG, "NULL argument");
    if (rows <= 0 || cols <= 0 || cap <= 0 || B <= 0 || mask_step < (size_t)cols * 3) return set_error(PLP_ERR_INVALID_ARG, "bad geometry");
    std::lock_guard<std::mutex> lk(c->mu);
    PLP_HIP(hipSetDevice(c->device));
    launch_color_vote((hipStream_t)hip_stream, d_mask, rows, cols, mask_step, mask_frame_stride, d_undist, d_valid, d_counts, cap, B,
                      check_3x3_window != 0, d_labels);
    PLP_HIP(hipGetLastError());
    return PLP_OK;
}

plp_status plp_landmark_descriptor_device(plp_matcher* c, const uint8_t* d_descs, const int32_t* d_offsets, int32_t L, int32_t* d_best_idx,
                                          void* hip_stream) {
    if (!c || !d_offsets || !d_best_idx || L < 0) return set_error(PLP_ERR_INVALID_ARG, "bad argument");
    if (L == 0) return PLP_OK;
    std::lock_guard<std::mutex> lk(c->mu);
    PLP_HIP(hipSetDevice(c->device));
    launch_landmark_descriptor((hipStream_t)hip_stream, d_descs, d_offsets, L, d_best_idx);
    PLP_HIP(hipGetLastError());
    return PLP_OK;
}

plp_status plp_landmark_descriptor_host(plp_matcher* c, const uint8_t* descs, const int32_t* offsets, int32_t L, int32_t* best_idx) {
    if (!c || !offsets || !best_idx || L < 0) return set_error(PLP_ERR_INVALID_ARG, "bad argument");
    if (L == 0) return PLP_OK;
    const int64_t total = offsets[L];
    if (total < 0 || (total > 0 && !descs)) return set_error(PLP_ERR_INVALID_ARG, "bad offsets / descs");
    for (int l = 0; l < L; ++l)
        if (offsets[l + 1] < offsets[l] || offsets[l + 1] - offsets[l] > 1024) return set_error(PLP_ERR_UNSUPPORTED, "offsets must ascend, at most 1024 rows per landmark");
    std::lock_guard<std::mutex> lk(c->mu);
    PLP_HIP(hipSetDevice(c->device));
    const uint8_t* d_descs = descs;   // device addresses after upload()
    const int32_t* d_offsets = offsets;
    int32_t* d_best_idx = best_idx;
    Stage s(c->stage, c->stream);   // no row at all: the kernel reads no descriptor
    s.in(d_descs, (size_t)total * 32); s.in(d_offsets, (size_t)L + 1); s.out(d_best_idx, L, false);
    PLP_TRY(s.upload());
    launch_landmark_descriptor(c->stream, d_descs, d_offsets, L, d_best_idx);
    PLP_HIP(hipGetLastError());
    return s.finish();
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
    std::lock_guard<std::mutex> lk(c->mu);
    PLP_HIP(hipSetDevice(c->device));
    const uint8_t *d_q = q, *d_t = t;   // device addresses after upload()
    uint16_t* d_dist = dist;
    Stage s(c->stage, c->stream);
    s.in(d_q, (size_t)nq * 32); s.in(d_t, (size_t)nt * 32); s.out(d_dist, (size_t)nq * nt, false);
    PLP_TRY(s.upload());
    launch_hamming_matrix(c->stream, d_q, nq, d_t, nt, d_dist);
    PLP_HIP(hipGetLastError());
    return s.finish();
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
