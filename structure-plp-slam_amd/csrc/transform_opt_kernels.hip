// Sim3 refinement of loop candidates: optimize::transform_optimizer (plp_transform_optimize_*, include/plp_front.h).
// The arithmetic is transform_opt.hpp's, which the host model runs too.  One workgroup of 256 lanes per problem, three launches:
//
// k_transform_prepare:
//      the observations of a problem in slot order (valid and both octaves inside the table), ballot + wave prefix: rank -> slot; sets out_kept
//      of every observation slot (the match is still set) and leaves, per edge, what does not depend on the estimate: the landmark in the
//      camera of its key frame, the observation and the weight.
// k_transform_optimize:
//      both rounds (:129-196) in one launch.  A pass walks the matches in tiles of 128, which is 256 edges: lane 2 i + d owns direction d
//      (0 forward, 1 backward) of match i of the tile, so the rows of a tile are in D16's edge order.  Every lane forms the terms of its edge
//      in LDS (36 for a linearisation, the robust chi2 alone for an evaluation; +0.0 for a dropped match, which leaves a sum's bits alone), and
//      lane t adds row t in edge order to its accumulator -- one chain per sum.  The fourteen perturbed estimates of the numeric Jacobian, the
//      estimate and the fifteen inverses are formed once per linearisation by fifteen lanes.  Lane 0 owns the estimate: the 7 x 7 Cholesky,
//      exp, accept / reject, lambda; the other lanes read its decision from LDS after a barrier.
// k_transform_finish:
//      clears out_kept of the dropped matches and writes the Sim3 outputs, the counts and the status from what the second kernel left in
//      the context's buffers.
//
// The launches hand the ranks and the per-edge chi2 on through buffers the context owns: the calls of one context must be ordered on the device.
#include <hip/hip_runtime.h>

#include "plp_barrier.hpp"
#include "transform_opt.hpp"

namespace plp {
namespace {

constexpr int kTfTile = 128;                 // matches per pass tile, two edges each: one edge per lane (tests/test_gpu_transform_optimizer.py restates it)
constexpr int kTfEdgeRec = 6;                // doubles an edge keeps between the launches: x y z in the camera, the observation, the weight
constexpr int kTfRow = 2 * kTfTile + 1;      // doubles between two term rows: the 36 adding lanes read 36 different banks

__global__ __launch_bounds__(256) void k_transform_prepare(TfArgs A) {
    __shared__ int s_wave_n[4];
    __shared__ float s_sig[2][16];                           // [0] key frame 1's table (forward edges), [1] key frame 2's
    const int p = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const size_t row = (size_t)p * A.n_cap;
    const int count = tf_count(A, p);
    if (tid < 16) { s_sig[0][tid] = A.inv_sigma_sq_1[tid]; s_sig[1][tid] = A.inv_sigma_sq_2[tid]; }
    wg_barrier();
    int n = 0;
    for (int base = 0; base < count; base += 256) {
        const int slot = base + tid;
        const bool v = slot < count && tf_observation(A, row + slot);
        const unsigned long long m = __ballot(v);
        if (lane == 0) s_wave_n[w] = (int)__popcll(m);
        wg_barrier();
        int off = n;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (u < w) off += s_wave_n[u];
            n += s_wave_n[u];
        }
        wg_barrier();
        if (v) {
            const int k = off + (int)__popcll(m & ((1ull << lane) - 1ull));
            A.ctx_slot[row + k] = (uint16_t)slot;
            A.ctx_level[row + k] = 0;
            A.out_kept[row + slot] = 1;
            // what the two edges of the match read in every pass, none of which depends on the estimate: the landmark in the other key frame's
            // camera (forward: key frame 2's landmark, observed by key frame 1), the observation and its weight
#pragma unroll
            for (int dir = 0; dir < 2; ++dir) {
                const plp_keypoint* kp = (dir ? A.undist_2 : A.undist_1) + row + slot;
                const double* pw = (dir ? A.pos_w_1 : A.pos_w_2) + 3 * (row + slot);
                const double q[3] = {pw[0], pw[1], pw[2]};
                double* e = A.ctx_edge + kTfEdgeRec * (2 * (row + k) + dir);
                tf_to_camera((dir ? A.pose_1 : A.pose_2) + (size_t)15 * p, q, e[0], e[1], e[2]);
                e[3] = (double)kp->x; e[4] = (double)kp->y; e[5] = (double)s_sig[dir][kp->octave];
            }
        }
    }
    if (tid == 0) A.ctx_n[kTfCtxInts * p] = n;
}

// what every lane reads of the arguments' numbers, in LDS: scalar registers are left to the pointers
struct TfConst {
    PoseCam cam;
    double delta;
};

// One pass over the kept matches.  lin: the 36 sums at the linearisation W.sims / W.invs, lane t < 36 returns sum t; otherwise the robust chi2
// alone at entry 14 (the tried estimate), lane 0 returns it.  Stores every evaluated edge's chi2.  Uniform over the workgroup; ends with a barrier.
__device__ __forceinline__ double tf_pass(const TfArgs& A, const TfWork& W, const TfConst& K, double* s_terms, int p, int n, bool lin) {
    const int tid = threadIdx.x, dir = tid & 1;
    const size_t row = (size_t)p * A.n_cap;
    double* chi2 = A.ctx_chi2 + 2 * row;
    const int first = lin ? 0 : 35, rows = lin ? kTfTerms : 1;
    static_assert(offsetof(TfWork, invs) == offsetof(TfWork, sims) + 8 * kTfSims * sizeof(double), "invs follows sims");
    const double* sims = W.sims + (dir ? 8 * kTfSims : 0);   // one LDS base: the inverses for a backward edge
    const double* edge = A.ctx_edge + kTfEdgeRec * 2 * row;
    const uint8_t* level = A.ctx_level + row;
    double acc = 0.0;
    for (int base = 0; base < n; base += kTfTile) {
        const int k = base + (tid >> 1);
        double* T = s_terms + tid;
        bool active = false;
        if (k < n) {
            active = level[k] == 0;
            if (active) {
                const double* e = edge + kTfEdgeRec * (2 * k + dir);
                const double x = e[0], y = e[1], z = e[2], ox = e[3], oy = e[4], w = e[5];
                if (lin) {
                    chi2[2 * k + dir] = tf_edge_terms(sims, K.cam, x, y, z, ox, oy, w, K.delta, T, kTfRow);
                } else {
                    double e0, e1, rho0, rho1;
                    const double c = tf_edge_error(sims + 8 * 14, K.cam, x, y, z, ox, oy, w, e0, e1);
                    pose_huber(c, K.delta, rho0, rho1);
                    T[35 * kTfRow] = rho0;
                    chi2[2 * k + dir] = c;
                }
            }
        }
        if (!active) {
            for (int t = first; t < kTfTerms; ++t) T[t * kTfRow] = 0.0;
        }
        wg_barrier();
        if (tid < rows) {
            const int cnt = 2 * (n - base < kTfTile ? n - base : kTfTile);
            const double* r = s_terms + (first + tid) * kTfRow;
            for (int i = 0; i < cnt; ++i) acc = acc + r[i];
        }
        wg_barrier();
    }
    return acc;
}

// what k_transform_finish needs of a problem: the estimate behind the chi2 rows (the rounds' chi2 and lambda follow it), the outcome beside
// the count (the rounds' counters follow it)
__device__ __forceinline__ void tf_hand_over(const TfArgs& A, int p, const double* est, bool early, int inliers) {
    double* e = A.ctx_chi2 + 2 * (size_t)A.P * A.n_cap + kTfCtxDoubles * (size_t)p;
    for (int i = 0; i < 8; ++i) e[i] = est[i];
    A.ctx_n[kTfCtxInts * p + 1] = early ? 1 : 0;
    A.ctx_n[kTfCtxInts * p + 2] = inliers;
}

__global__ __launch_bounds__(256) void k_transform_optimize(TfArgs A) {
    __shared__ TfWork W;
    __shared__ double s_terms[kTfTerms * kTfRow];
    __shared__ TfConst K;
    __shared__ int s_drop;
    const int p = blockIdx.x, tid = threadIdx.x;
    const size_t row = (size_t)p * A.n_cap;
    const int n = A.ctx_n[kTfCtxInts * p];
    if (tid == 0) { K.cam = A.cam; K.delta = A.delta; }
    if (tid == 0) {
        tf_est_from_input(A.rot_12 + (size_t)9 * p, A.trans_12 + (size_t)3 * p, A.scale_12[p], W.est);
        W.lambda = 0.0; W.ni = 2.0; W.current_chi = 0.0;
    }
    wg_barrier();
    if (n == 0) {                                            // an empty graph: optimize() returns at once, :156 returns 0
        if (tid == 0) tf_hand_over(A, p, W.est, true, 0);
        return;
    }
    const double* chi2 = A.ctx_chi2 + 2 * row;
    const bool fix = A.fix_scale != 0;
    int left = n;                                            // matches at level 0
    for (int round = 0; round < 2; ++round) {
        const int iters = tf_round_iters(round, A.num_iter);
        if (tid == 0) { W.iterations = 0; W.rejected = 0; W.end = 0; s_drop = 0; }
        wg_barrier();
        // optimize(iters): a linearisation, then evaluations of tried estimates until one is kept or the tries are used up
        int it = 0;
        bool lin = true;
        for (;;) {
            // the similarities of this pass and their inverses, by one copy of Sim3(update) * est: the fifteen of a linearisation (a lane
            // each), or the tried estimate alone (lane 0, from the step it solved for)
            if (tid < (lin ? kTfSims : 1)) {
                const int which = lin ? tid : 2 * kTfDim;
                double* out = W.sims + 8 * which;
                if (lin && which == 2 * kTfDim) {
                    for (int i = 0; i < 8; ++i) out[i] = W.est[i];
                } else {
                    double u[kTfDim];
#pragma unroll
                    for (int i = 0; i < kTfDim; ++i)
                        u[i] = !lin ? W.x[i] : i != (which >> 1) ? 0.0 : (which & 1) ? -kPoseNumericDelta : kPoseNumericDelta;
                    tf_oplus(u, fix, lin ? W.est : W.bak, out);
                }
                tf_inverse(out, W.invs + 8 * which);
                if (!lin) {
                    for (int i = 0; i < 8; ++i) W.est[i] = out[i];
                }
            }
            wg_barrier();
            const double acc = tf_pass(A, W, K, s_terms, p, n, lin);
            if (lin) {
                if (tid < kTfTerms) W.sum[tid] = acc;
                wg_barrier();
            }
            if (tid == 0) {
                if (lin) { lev_begin<kTfDim>(W, it); W.go_on = 1; }
                else lev_decide_vertex<kTfDim, 8>(W, acc);
                if (W.go_on) tf_lm_solve(W);
                else { W.iterations += 1; W.end = lev_end(W); }
            }
            wg_barrier();
            lin = false;
            if (W.go_on) continue;
            ++it;
            if (W.end || it >= iters) break;
            lin = true;
        }
        wg_barrier_after_global_stores();                    // the chi2 of an edge is read by another lane than the one that stored it
        int drop = 0;
        for (int base = 0; base < n; base += 256) {
            const int k = base + tid;
            bool d = false;
            if (k < n && A.ctx_level[row + k] == 0) {
                d = tf_drop(round, A.chi_sq, chi2[2 * k], chi2[2 * k + 1]);
                if (d) A.ctx_level[row + k] = 1;
            }
            drop += (int)__popcll(__ballot(d));
        }
        if ((tid & 63) == 0) atomicAdd(&s_drop, drop);
        wg_barrier_after_global_stores();                    // the flags are read by the next round's passes
        const int drops = s_drop;
        left -= drops;
        if (tid == 0) {
            int32_t* ri = A.ctx_n + kTfCtxInts * p + 3 + 4 * round;
            ri[0] = W.iterations; ri[1] = W.rejected; ri[2] = drops; ri[3] = W.end ? W.end : kLevEndIterations;
            double* rc = A.ctx_chi2 + 2 * (size_t)A.P * A.n_cap + kTfCtxDoubles * (size_t)p + 8 + 2 * round;
            rc[0] = W.current_chi; rc[1] = W.lambda;
        }
        wg_barrier();                                        // s_drop is reset by the next round
        if (round == 0 && left < kTfMinInliers) {            // :156: the Sim3 is not written back
            if (tid == 0) {
                tf_hand_over(A, p, W.est, true, 0);
            }
            return;
        }
    }
    if (tid == 0) tf_hand_over(A, p, W.est, false, left);
}

// The outputs of a problem: the flags of the dropped matches, and lane 0 the Sim3, the counts and the status.  Kept apart so that
// k_transform_optimize holds neither the slot table nor ten output pointers across its loops.
__global__ __launch_bounds__(64) void k_transform_finish(TfArgs A) {
    const int p = blockIdx.x, tid = threadIdx.x;
    const size_t row = (size_t)p * A.n_cap;
    const int n = A.ctx_n[kTfCtxInts * p];
    for (int k = tid; k < n; k += 64)
        if (A.ctx_level[row + k]) A.out_kept[row + A.ctx_slot[row + k]] = 0;
    if (tid != 0) return;
    const double* e = A.ctx_chi2 + 2 * (size_t)A.P * A.n_cap + kTfCtxDoubles * (size_t)p;
    double est[8];
    const bool early = A.ctx_n[kTfCtxInts * p + 1] != 0;
    if (early) {                                             // :156: the Sim3 is not written back
        tf_est_from_input(A.rot_12 + (size_t)9 * p, A.trans_12 + (size_t)3 * p, A.scale_12[p], est);
    } else {
#pragma unroll
        for (int i = 0; i < 8; ++i) est[i] = e[i];
    }
    tf_write_result(A, p, est, early, n, A.ctx_n[kTfCtxInts * p + 2]);
    const int rounds = n == 0 ? 0 : early ? 1 : 2;           // a round that was not run: zeros
    for (int i = 0; i < 8; ++i)
        if (A.out_round_info) A.out_round_info[(size_t)8 * p + i] = i < 4 * rounds ? A.ctx_n[kTfCtxInts * p + 3 + i] : 0;
    for (int i = 0; i < 4; ++i)
        if (A.out_round_chi2) A.out_round_chi2[(size_t)4 * p + i] = i < 2 * rounds ? e[8 + i] : 0.0;
}

}  // namespace

hipError_t launch_transform_optimize(hipStream_t st, const TfArgs& A) {
    hipLaunchKernelGGL(k_transform_prepare, dim3(A.P), dim3(256), 0, st, A);
    hipLaunchKernelGGL(k_transform_optimize, dim3(A.P), dim3(256), 0, st, A);
    hipLaunchKernelGGL(k_transform_finish, dim3(A.P), dim3(64), 0, st, A);
    return hipGetLastError();
}

}  // namespace plp
