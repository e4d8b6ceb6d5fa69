// Per-frame pose optimisation: optimize::pose_optimizer and pose_optimizer_extended_line (plp_pose_optimize_*, include/plp_front.h; DESIGN.md
// section 5, D15).  The arithmetic is pose_opt.hpp's, which the host model runs too.  One workgroup of 256 lanes per frame, two launches:
//
// k_pose_prepare:
//      the observations of a frame in slot order (valid and an octave inside the table), ballot + wave prefix: rank -> slot for points and, when
//      there are at least five point observations, for lines; clears the outlier flags the reference clears (:146 / :184).
// k_pose_optimize<lines>:
//      the whole trial loop (:162-222 / :208-298) in one launch.  Edge k of a frame belongs to lane k mod 256 in every pass, so the chi2 of its
//      last evaluation comes back to the lane that stored it.  A pass walks the edges in tiles of 256, points before lines: every lane forms the
//      terms of its edge at the estimate in LDS (28 for a linearisation, the robust chi2 alone for an evaluation; +0.0 for an edge at level 1,
//      which leaves a sum's bits alone) into a tile of LDS rows, and lane t adds row t in edge order to its accumulator -- D15's one chain per
//      sum.  Lane 0 owns the estimate: the 6 x 6 Cholesky, exp, accept / reject, lambda; the other lanes read its decision from LDS after a barrier.
//      The twelve estimates of the line edge's numeric Jacobian are formed once per linearisation by twelve lanes.
//
// The launches hand the ranks and the per-edge chi2 on through buffers the context owns: the calls of one context must be ordered on the device.
#include <hip/hip_runtime.h>

#include "plp_barrier.hpp"
#include "pose_opt.hpp"

namespace plp {
namespace {

constexpr int kPoseTile = 256;           // edges per pass tile: one per lane (tests/test_gpu_pose_optimizer.py restates it)
constexpr int kPoseRow = kPoseTile + 1;  // doubles between two term rows: the 28 adding lanes read 28 different banks

// One step of an ordered compaction over the workgroup (as pnp_kernels.hip): the rank of this lane's item among the flagged ones; ends with a barrier
__device__ __forceinline__ int pose_compact_step(bool v, int& n, int (&s_wave_n)[4]) {
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const unsigned long long m = __ballot(v);
    if (lane == 0) s_wave_n[w] = (int)__popcll(m);
    wg_barrier();
    int off = n, tot = 0;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        if (u < w) off += s_wave_n[u];
        tot += s_wave_n[u];
    }
    n += tot;
    wg_barrier();
    return off + (int)__popcll(m & ((1ull << lane) - 1ull));
}

__global__ __launch_bounds__(256) void k_pose_prepare(PoseArgs A) {
    __shared__ int s_wave_n[4];
    const int b = blockIdx.x, tid = threadIdx.x;
    const size_t row = (size_t)b * A.n_cap, lrow = (size_t)b * A.l_cap;
    const int count = pose_count(A, b);
    int n = 0;
    for (int base = 0; base < count; base += 256) {
        const int slot = base + tid;
        bool v = slot < count && A.valid[row + slot] != 0;
        if (v) v = (unsigned)A.undist[row + slot].octave < (unsigned)A.num_levels;
        const int pos = pose_compact_step(v, n, s_wave_n);
        if (v) {
            A.ctx_slot[row + pos] = (uint16_t)slot;
            A.out_outlier[row + slot] = 0;
        }
    }
    int nl = 0;
    if (A.l_cap > 0 && n >= kPoseMinObs) {
        const int lcount = pose_line_count(A, b);
        for (int base = 0; base < lcount; base += 256) {
            const int slot = base + tid;
            bool v = slot < lcount && A.line_valid[lrow + slot] != 0;
            if (v) v = (unsigned)A.keylines[lrow + slot].octave < (unsigned)A.num_levels_lsd;
            const int pos = pose_compact_step(v, nl, s_wave_n);
            if (v) {
                A.ctx_slot_lines[lrow + pos] = (uint16_t)slot;
                A.out_outlier_lines[lrow + slot] = 0;
            }
        }
    }
    if (tid == 0) { A.ctx_n[2 * b] = n; A.ctx_n[2 * b + 1] = nl; }
}

// One pass over the active edges at W.est.  lin: the 28 sums, lane t < 28 returns sum t; otherwise the robust chi2 alone, lane 0 returns it.
// (One body for both, chosen at run time: two inlined copies of the edges cost scalar registers.)
// Stores every active edge's chi2.  Uniform over the workgroup; ends with a barrier.
// what every lane reads of the arguments' numbers, in LDS: scalar registers are left to the pointers
struct PoseConst {
    PoseCam cam;
    double delta_pt, delta_2d;
    float sig[16], sig_l[16];
};

template <bool LINES>
__device__ __forceinline__ double pose_pass(const PoseArgs& A, PoseWork& W, const PoseConst& K, double* s_terms, int b, int n, int nl, bool robust, bool lin) {
    const int tid = threadIdx.x;
    const size_t row = (size_t)b * A.n_cap, lrow = (size_t)b * A.l_cap;
    double* chi2_pt = A.ctx_chi2 + (size_t)b * (A.n_cap + A.l_cap);
    double* chi2_ln = chi2_pt + A.n_cap;
    const double delta_pt = K.delta_pt;
    const int first = lin ? 0 : 27, rows = lin ? 28 : 1;
    double acc = 0.0;
    const int total = LINES ? 2 : 1;
    for (int part = 0; part < total; ++part) {
        const int m = part == 0 ? n : nl;
        for (int base = 0; base < m; base += kPoseTile) {
            const int k = base + tid;
            double* T = s_terms + tid;
            bool active = false;
            if (k < m) {
                if (part == 0) {
                    const int slot = A.ctx_slot[row + k];
                    active = A.out_outlier[row + slot] == 0;
                    if (active) {
                        const plp_keypoint* kp = A.undist + row + slot;
                        const float xr = A.x_right ? A.x_right[row + slot] : -1.0f;
                        const double w = (double)K.sig[kp->octave];
                        const double* pw = A.pos_w + 3 * (row + slot);
                        const double p[3] = {pw[0], pw[1], pw[2]};
                        if (lin) {
                            chi2_pt[k] = pose_point_terms(W.est, K.cam, p, (double)kp->x, (double)kp->y, (double)xr, xr < 0.0f, w, robust, delta_pt, T, kPoseRow);
                        } else {
                            double x, y, z, e0, e1, e2;
                            const double chi2 = pose_point_error(W.est, K.cam, p, (double)kp->x, (double)kp->y, (double)xr, xr < 0.0f, w, x, y, z, e0, e1, e2);
                            double rho0 = chi2, rho1 = 1.0;
                            if (robust) pose_huber(chi2, delta_pt, rho0, rho1);
                            T[27 * kPoseRow] = rho0;
                            chi2_pt[k] = chi2;
                        }
                    }
                } else if (LINES) {
                    const int slot = A.ctx_slot_lines[lrow + k];
                    active = A.out_outlier_lines[lrow + slot] == 0;
                    if (active) {
                        const plp_keyline* kl = A.keylines + lrow + slot;
                        const double w = (double)K.sig_l[kl->octave];
                        const double* pl = A.pos_w_lines + 6 * (lrow + slot);
                        const double L[6] = {pl[0], pl[1], pl[2], pl[3], pl[4], pl[5]};
                        const double xs = (double)kl->startPointX, ys = (double)kl->startPointY, xe = (double)kl->endPointX, ye = (double)kl->endPointY;
                        if (lin) {
                            chi2_ln[k] = pose_line_terms(W.est, W.pert, K.cam, L, xs, ys, xe, ye, w, robust, K.delta_2d, T, kPoseRow);
                        } else {
                            double e0, e1;
                            const double chi2 = pose_line_error(W.est, K.cam, L, xs, ys, xe, ye, w, e0, e1);
                            double rho0 = chi2, rho1 = 1.0;
                            if (robust) pose_huber(chi2, K.delta_2d, rho0, rho1);
                            T[27 * kPoseRow] = rho0;
                            chi2_ln[k] = chi2;
                        }
                    }
                }
            }
            if (!active) {
                for (int t = first; t < 28; ++t) T[t * kPoseRow] = 0.0;
            }
            wg_barrier();
            if (tid < rows) {
                const int cnt = m - base < kPoseTile ? m - base : kPoseTile;
                const double* r = s_terms + (first + tid) * kPoseRow;
                for (int i = 0; i < cnt; ++i) acc = acc + r[i];
            }
            wg_barrier();
        }
    }
    return acc;
}

template <bool LINES>
__global__ __launch_bounds__(256) void k_pose_optimize(PoseArgs A) {
    __shared__ PoseWork W;
    __shared__ double s_terms[kPoseTerms * kPoseRow];
    __shared__ PoseConst K;
    __shared__ int s_bad;
    const int b = blockIdx.x, tid = threadIdx.x;
    const size_t row = (size_t)b * A.n_cap, lrow = (size_t)b * A.l_cap;
    const int n = A.ctx_n[2 * b], nl = LINES ? A.ctx_n[2 * b + 1] : 0;
    const int T = A.num_trials;
    if (tid < 16) { K.sig[tid] = A.inv_sigma_sq[tid]; K.sig_l[tid] = A.inv_sigma_sq_lsd[tid]; }
    if (tid == 0) { K.cam = A.cam; K.delta_pt = A.mono_setup ? A.delta_2d : A.delta_3d; K.delta_2d = A.delta_2d; }
    for (int i = tid; i < 4 * T; i += 256)
        if (A.out_trial_info) A.out_trial_info[(size_t)4 * T * b + i] = 0;
    for (int i = tid; i < 2 * T; i += 256)
        if (A.out_trial_chi2) A.out_trial_chi2[(size_t)2 * T * b + i] = 0.0;
    if (n < kPoseMinObs) {                                   // :153 / :162
        if (tid == 0) {
            const double* in = A.pose_in + (size_t)b * A.pose_stride;
            double* out = A.out_pose + (size_t)15 * b;
            for (int i = 0; i < 12; ++i) out[i] = in[i];
            for (int i = 0; i < 3; ++i) out[12 + i] = ((-in[i]) * in[9] + (-in[3 + i]) * in[10]) + (-in[6 + i]) * in[11];
            A.out_status[b] = PLP_POSE_OPT_TOO_FEW_OBS;
            A.out_num_init_obs[b] = n;
            A.out_num_valid[b] = 0;
        }
        return;
    }
    if (tid == 0) {
        const double* in = A.pose_in + (size_t)b * A.pose_stride;
        double p12[12];
#pragma unroll
        for (int i = 0; i < 12; ++i) p12[i] = in[i];
        pose_est_from_pose(p12, W.est);
        W.lambda = 0.0; W.ni = 2.0; W.current_chi = 0.0;
    }
    wg_barrier_after_global_stores();                        // the trial rows zeroed above are rewritten by lane 0 below
    const double* chi2_pt = A.ctx_chi2 + (size_t)b * (A.n_cap + A.l_cap);
    const double* chi2_ln = chi2_pt + A.n_cap;
    int num_bad = 0;
    for (int trial = 0; trial < T; ++trial) {
        const bool robust = pose_trial_robust(trial, T);
        if (tid == 0) { W.iterations = 0; W.rejected = 0; W.end = 0; s_bad = 0; }
        wg_barrier();
        // optimize(num_each_iter): a linearisation, then evaluations of tried estimates until one is kept or the tries are used up
        int it = 0;
        bool lin = true;
        for (;;) {
            if (LINES && lin) {
                if (tid < 12 && nl > 0) pose_perturb(W.est, tid, W.pert + 7 * tid);
                wg_barrier();
            }
            const double acc = pose_pass<LINES>(A, W, K, s_terms, b, n, nl, robust, lin);
            if (lin) {
                if (tid < kPoseTerms) W.sum[tid] = acc;
                wg_barrier();
                if (tid == 0) { lev_begin<6>(W, it); pose_lm_try(W); }
                wg_barrier();
                lin = false;
                continue;
            }
            if (tid == 0) {
                lev_decide_vertex<6, 7>(W, acc);
                if (W.go_on) pose_lm_try(W);
                else { W.iterations += 1; W.end = lev_end(W); }
            }
            wg_barrier();
            if (W.go_on) continue;
            ++it;
            if (W.end || it >= A.num_each_iter) break;
            lin = true;
        }
        // the flags of the point edges (:172-216 / :218-262): a flagged edge is evaluated at the estimate, an active one keeps its last error
        int bad = 0;
        for (int base = 0; base < n; base += 256) {
            const int k = base + tid;
            bool is_bad = false;
            if (k < n) {
                const int slot = A.ctx_slot[row + k];
                const float xr = A.x_right ? A.x_right[row + slot] : -1.0f;
                double chi2;
                if (A.out_outlier[row + slot]) {
                    const plp_keypoint* kp = A.undist + row + slot;
                    const double* pw = A.pos_w + 3 * (row + slot);
                    const double p[3] = {pw[0], pw[1], pw[2]};
                    double x, y, z, e0, e1, e2;
                    chi2 = pose_point_error(W.est, K.cam, p, (double)kp->x, (double)kp->y, (double)xr, xr < 0.0f, (double)K.sig[kp->octave], x, y, z, e0, e1, e2);
                } else {
                    chi2 = chi2_pt[k];
                }
                is_bad = (double)(xr < 0.0f ? kPoseChiSq2D : kPoseChiSq3D) < chi2;
                A.out_outlier[row + slot] = is_bad ? 1 : 0;
            }
            bad += (int)__popcll(__ballot(is_bad));
        }
        if ((tid & 63) == 0) atomicAdd(&s_bad, bad);
        wg_barrier_after_global_stores();
        num_bad = s_bad;
        const bool stop = n - num_bad < kPoseMinObs;             // :218 / :264, before the line loop
        if (LINES && !stop) {
            for (int k = tid; k < nl; k += 256) {
                const int slot = A.ctx_slot_lines[lrow + k];
                double chi2;
                if (A.out_outlier_lines[lrow + slot]) {
                    const plp_keyline* kl = A.keylines + lrow + slot;
                    const double* pl = A.pos_w_lines + 6 * (lrow + slot);
                    const double L[6] = {pl[0], pl[1], pl[2], pl[3], pl[4], pl[5]};
                    double e0, e1;
                    chi2 = pose_line_error(W.est, K.cam, L, (double)kl->startPointX, (double)kl->startPointY, (double)kl->endPointX, (double)kl->endPointY,
                                           (double)K.sig_l[kl->octave], e0, e1);
                } else {
                    chi2 = chi2_ln[k];
                }
                A.out_outlier_lines[lrow + slot] = (double)kPoseChiSq2D < chi2 ? 1 : 0;
            }
        }
        if (tid == 0) {
            if (A.out_trial_info) {
                int32_t* ti = A.out_trial_info + ((size_t)T * b + trial) * 4;
                ti[0] = W.iterations; ti[1] = W.rejected; ti[2] = num_bad; ti[3] = W.end ? W.end : kLevEndIterations;
            }
            if (A.out_trial_chi2) {
                double* tc = A.out_trial_chi2 + ((size_t)T * b + trial) * 2;
                tc[0] = W.current_chi; tc[1] = W.lambda;
            }
        }
        wg_barrier_after_global_stores();                    // s_bad is reset and the flags are read by the next trial
        if (stop) break;
    }
    if (tid == 0) {
        pose_pose_from_est(W.est, A.out_pose + (size_t)15 * b);
        A.out_status[b] = PLP_POSE_OPT_OK;
        A.out_num_init_obs[b] = n;
        A.out_num_valid[b] = n - num_bad;
    }
}

}  // namespace

hipError_t launch_pose_optimize(hipStream_t st, const PoseArgs& A) {
    hipLaunchKernelGGL(k_pose_prepare, dim3(A.B), dim3(256), 0, st, A);
    if (A.l_cap > 0) hipLaunchKernelGGL(k_pose_optimize<true>, dim3(A.B), dim3(256), 0, st, A);
    else hipLaunchKernelGGL(k_pose_optimize<false>, dim3(A.B), dim3(256), 0, st, A);
    return hipGetLastError();
}

}  // namespace plp
