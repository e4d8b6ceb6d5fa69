// Relocalisation: solve::pnp_solver's constructor and find_via_ransac (plp_pnp_ransac_*, include/plp_front.h).
// The arithmetic is pnp.hpp's, which the host model runs too.
//
// Five launches, one workgroup of four waves per problem in each.  No result depends on the lane mapping: every hypothesis is a pure function
// of the problem's inputs, the rotations of one round of the Jacobi schedule touch disjoint columns, counts are integer sums, the winner is
// the maximum of a key that is unique per iteration, and every sum over correspondences is one accumulator in match order.
// k_pnp_prepare:
//   1. the valid slots are compacted in slot order, 256 at a time (64-bit ballot within the wave, the waves' totals through LDS), into the
//      context: slot[rank], the rank being what a sample index means.
// k_pnp_hypotheses:
//   2. a hypothesis goes to a group of 16 lanes (one DPP row), kPnpPass = 16 per workgroup pass.  Lane 0 of the group gathers the four
//      samples and runs compute_pose up to M^T M in the group's PnpWork in LDS; lanes 0 .. 11 then own one column of G and of V each (24
//      doubles, every index a compile-time constant) and run the 12 x 12 Jacobi, a round = one cross-lane fetch of the partner's two
//      columns, both lanes of a pair forming the three dot products in the same order; the four null vectors go back to LDS and lane 0
//      finishes compute_pose (L_6x10, betas, Gauss-Newton, the three R, t) there.  (R, t) goes to the call's context buffer.
// k_pnp_count:
//   3. 256 hypotheses at a time, one per lane with its 12 doubles; the matches go through LDS in tiles of kPnpTile (world point, bearing,
//      float threshold), every lane reading the same address.  The best hypothesis is the workgroup maximum of (count << 32 | ~iter).
// k_pnp_refit:
//   4. recompute (:136-152): the inliers of the best hypothesis are compacted in match order into the context's correspondence buffer; the
//      sums over them are chains of pnp.hpp, one per lane (3 centroid, 9 PW0tPW0, 78 of M^T M, 6 + 9 of estimate_R_and_t, 1 reprojection
//      error over terms formed by all lanes); what is independent per correspondence (alphas, pcs, the error terms) runs on all lanes; the
//      12 x 12 Jacobi is the same device function as in 2, run by wave 0; the scalar rest runs on lane 0.
// k_pnp_finish:
//   5. lane 0 writes the outputs and one pass over the slots writes out_inliers.
// The launches hand their results on through buffers the context owns: the calls of one context must be ordered on the device.
#include <hip/hip_runtime.h>

#include "plp_barrier.hpp"
#include "pnp.hpp"
#include "ransac_device.hpp"

namespace plp {
namespace {

constexpr int kPnpTile = 256;    // matches per LDS tile: one per lane
constexpr int kPnpPass = 16;     // hypotheses per workgroup pass: one per group of 16 lanes

__device__ __forceinline__ double* pnp_hyp_field(const PnpArgs& A, int p, int field) { return A.ctx_hyp + ((size_t)p * kPnpHypDoubles + field) * A.iters; }

__global__ __launch_bounds__(256) void k_pnp_prepare(PnpArgs A) {
    __shared__ int s_wave_n[4];
    const int p = blockIdx.x, tid = threadIdx.x;
    const size_t row = (size_t)p * A.n_cap;
    const int count = clamp_count(A.counts, p, A.n_cap);
    int n = 0;
    for (int base = 0; base < count; base += 256) {
        const int slot = base + tid;
        const bool v = slot < count && A.valid[row + slot] != 0;
        const int pos = wg_compact_step(v, n, s_wave_n);
        if (v) A.ctx_slot[row + pos] = (uint16_t)slot;
    }
    if (tid == 0) A.ctx[(size_t)kPnpCtxInts * p] = n;
}

// Use 2 of D14 by the 16-lane group of the calling lane: W.null from W.mtm.  j = the lane within its group; lanes 12 .. 15 take part in the
// cross-lane reads only.  The whole wave must call it; write: whether this group stores its result.  Returns the sweeps that rotated.
__device__ __forceinline__ int jacobi12_group(PnpWork& W, int j, bool write) {
    const int lane = threadIdx.x & 63;
    const int jj = j < 12 ? j : 0;
    double g[12], v[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) {
        g[i] = W.mtm[12 * i + jj];
        v[i] = i == jj ? 1.0 : 0.0;
    }
    int sweeps = 0;
    bool done = false;
    while (__ballot(!done) != 0ull) {                               // uniform over the wave; a group that is done rotates nothing
        bool rotated = false;
        for (int r = 0; r < 11; ++r) {
            const int q = j < 12 ? jacobi_partner(j, r, 12) : j;
            const bool lo = j < q;
            double pg[12], pv[12];
#pragma unroll
            for (int i = 0; i < 12; ++i) {
                pg[i] = __shfl(g[i], q, 16);
                pv[i] = __shfl(v[i], q, 16);
            }
            double alpha = 0.0, beta = 0.0, gamma = 0.0;
#pragma unroll
            for (int i = 0; i < 12; ++i) {
                const double a = lo ? g[i] : pg[i], b = lo ? pg[i] : g[i];   // the pair's lower column first, in both lanes
                alpha = alpha + a * a;
                beta = beta + b * b;
                gamma = gamma + a * b;
            }
            double c = 1.0, s = 0.0;
            const bool rot = hestenes_cs(alpha, beta, gamma, c, s) && !done && j < 12;
            if (rot) {
#pragma unroll
                for (int i = 0; i < 12; ++i) {
                    g[i] = lo ? c * g[i] - s * pg[i] : s * pg[i] + c * g[i];
                    v[i] = lo ? c * v[i] - s * pv[i] : s * pv[i] + c * v[i];
                }
            }
            rotated |= rot;
        }
        const unsigned long long bal = __ballot(rotated);
        const bool any = ((bal >> (lane & 48)) & 0xFFFFull) != 0ull;
        if (!done) {
            if (!any) done = true;
            else if (++sweeps >= kJacobiSweepLimit) done = true;
        }
    }
    double n2 = 0.0;
#pragma unroll
    for (int i = 0; i < 12; ++i) n2 = n2 + g[i] * g[i];
    const double key = jacobi_key(n2);
    int rank = 0;
#pragma unroll
    for (int k = 0; k < 12; ++k) rank += jacobi_before(__shfl(key, k, 16), k, key, j) ? 1 : 0;
    if (write && j < 12 && rank >= 8) {
#pragma unroll
        for (int i = 0; i < 12; ++i) W.null[12 * (11 - rank) + i] = v[i];
    }
    return sweeps;
}

__global__ __launch_bounds__(256) void k_pnp_hypotheses(PnpArgs A) {
    __shared__ PnpWork s_w[kPnpPass];
    __shared__ double s_corr[kPnpPass][4 * kPnpCorrDoubles];
    const int p = blockIdx.x, tid = threadIdx.x, grp = tid >> 4, j = tid & 15;
    const size_t row = (size_t)p * A.n_cap;
    const int n = A.ctx[(size_t)kPnpCtxInts * p];
    const bool enough = !(n < 4 || n < A.min_num_inliers);          // :76
    PnpWork& W = s_w[grp];
    double* corr = s_corr[grp];
    for (int base = 0; base < A.iters; base += kPnpPass) {          // uniform over the workgroup
        const int it = base + grp;
        const bool live = it < A.iters;
        int nc = 0, sign0 = 0;
        if (j == 0) {
            int idx[4];
            if (live && enough && ransac_sample<4>(A, p, it, n, idx)) {
#pragma unroll
                for (int k = 0; k < 4; ++k) {                       // :103-108, in the order given
                    const size_t s = row + A.ctx_slot[row + idx[k]];
                    int sg;
                    if (pnp_add_correspondence(A.pos_w + 3 * s, A.bearing + 3 * s, corr + nc * kPnpCorrDoubles, corr + nc * kPnpCorrDoubles + 3, sg)) {
                        if (nc == 0) sign0 = sg;
                        ++nc;
                    }
                }
            }
            if (nc > 0) {
                pnp_pose_front(W, corr, corr + 3, corr + 5, kPnpCorrDoubles, nc);
            } else {
                for (int i = 0; i < 144; ++i) W.mtm[i] = 0.0;
            }
        }
        __builtin_amdgcn_wave_barrier();
        const int sw = jacobi12_group(W, j, true);
        __builtin_amdgcn_wave_barrier();
        if (j == 0 && live) {
            if (nc > 0) {
                W.sweeps[1] = sw;
                const int N = pnp_pose_back(W, corr, corr + 3, corr + 5, corr + 9, kPnpCorrDoubles, nc, sign0);
                for (int i = 0; i < 9; ++i) pnp_hyp_field(A, p, i)[it] = W.Rs[9 * N + i];
                for (int i = 0; i < 3; ++i) pnp_hyp_field(A, p, 9 + i)[it] = W.ts[3 * N + i];
            }
            pnp_hyp_field(A, p, 12)[it] = nc > 0 ? 1.0 : 0.0;
        }
        __builtin_amdgcn_wave_barrier();
    }
}

__global__ __launch_bounds__(256) void k_pnp_count(PnpArgs A) {
    __shared__ double s_pt[6][kPnpTile];        // pos_w (3), bearing (3)
    __shared__ float s_thr[kPnpTile];
    __shared__ uint8_t s_never[kPnpTile];
    __shared__ float s_tab[16];
    __shared__ unsigned long long s_part[4];
    const int p = blockIdx.x, tid = threadIdx.x;
    const size_t row = (size_t)p * A.n_cap;
    if (tid < 16) s_tab[tid] = A.thr[tid];
    wg_barrier();
    const int n = A.ctx[(size_t)kPnpCtxInts * p];
    const bool enough = !(n < 4 || n < A.min_num_inliers);          // :76

    unsigned long long key = 0;
    for (int chunk = 0; chunk < A.iters; chunk += 256) {
        const int it = chunk + tid;
        const bool live = it < A.iters;
        const bool hyp = live && enough && pnp_hyp_field(A, p, 12)[it] != 0.0;
        double R[9], t[3];
#pragma unroll
        for (int i = 0; i < 9; ++i) R[i] = hyp ? pnp_hyp_field(A, p, i)[it] : 0.0;
#pragma unroll
        for (int i = 0; i < 3; ++i) t[i] = hyp ? pnp_hyp_field(A, p, 9 + i)[it] : 0.0;
        int num = 0;
        if (enough) {   // uniform over the workgroup
            for (int tile = 0; tile < n; tile += kPnpTile) {
                const int k = tile + tid;
                if (k < n) {
                    const size_t s = row + A.ctx_slot[row + k];
#pragma unroll
                    for (int r = 0; r < 3; ++r) { s_pt[r][tid] = A.pos_w[3 * s + r]; s_pt[3 + r][tid] = A.bearing[3 * s + r]; }
                    const int o = A.octave[s];
                    const bool lv = (unsigned)o < (unsigned)A.num_levels;
                    s_thr[tid] = lv ? s_tab[o] : 0.0f;
                    s_never[tid] = lv ? 0 : 1;
                }
                wg_barrier();
                const int m = n - tile < kPnpTile ? n - tile : kPnpTile;
                if (hyp) {
                    for (int q = 0; q < m; ++q) {
                        const double w[3] = {s_pt[0][q], s_pt[1][q], s_pt[2][q]}, b[3] = {s_pt[3][q], s_pt[4][q], s_pt[5][q]};
                        num += pnp_inlier(R, t, w, b, s_thr[q], s_never[q] != 0) ? 1 : 0;
                    }
                }
                wg_barrier();   // the next tile, or the next chunk, rewrites the arrays
            }
        }
        if (live) {
            if (A.out_hyp_inliers) A.out_hyp_inliers[(size_t)p * A.iters + it] = num;
            const unsigned long long mine = ransac_key((unsigned)num, it);
            key = mine > key ? mine : key;
        }
    }
    key = wg_max_u64(key, s_part);
    if (tid == 0) {
        const int best_count = (int)(key >> 32);
        int32_t* c = A.ctx + (size_t)kPnpCtxInts * p;
        c[1] = best_count;
        c[2] = best_count > 0 ? ransac_key_iter(key) : -1;
        c[3] = 0;
    }
}

__global__ __launch_bounds__(256) void k_pnp_refit(PnpArgs A) {
    __shared__ PnpWork s_w;
    __shared__ double s_pose[12];
    __shared__ float s_tab[16];
    __shared__ int s_wave_n[4];
    const int p = blockIdx.x, tid = threadIdx.x;
    const size_t row = (size_t)p * A.n_cap;
    int32_t* ctx = A.ctx + (size_t)kPnpCtxInts * p;
    const int n = ctx[0], best_count = ctx[1], best_iter = ctx[2];
    const bool enough = !(n < 4 || n < A.min_num_inliers);          // :76
    const bool ok = enough && best_count > A.min_num_inliers;       // :126
    if (!(ok && A.recompute != 0 && best_iter >= 0 && best_iter < A.iters)) return;   // :131, uniform over the workgroup
    if (tid < 12) s_pose[tid] = pnp_hyp_field(A, p, tid)[best_iter];
    if (tid < 16) s_tab[tid] = A.thr[tid];
    wg_barrier();

    // :138-150: the inliers in match order; add_correspondence skips bearing(2) == 0
    constexpr int S = kPnpCorrDoubles;
    double* pws = A.ctx_corr + row * S;
    double* us = pws + 3;
    double* alphas = pws + 5;
    double* pcs = pws + 9;
    int nc = 0;
    for (int base = 0; base < n; base += 256) {
        const int k = base + tid;
        bool in = false;
        size_t s = 0;
        if (k < n) {
            s = row + A.ctx_slot[row + k];
            const int o = A.octave[s];
            const bool lv = (unsigned)o < (unsigned)A.num_levels;
            in = pnp_inlier(s_pose, s_pose + 9, A.pos_w + 3 * s, A.bearing + 3 * s, lv ? s_tab[o] : 0.0f, !lv) && A.bearing[3 * s + 2] != 0;
        }
        const int pos = wg_compact_step(in, nc, s_wave_n);
        if (in) {
            int sg;
            pnp_add_correspondence(A.pos_w + 3 * s, A.bearing + 3 * s, pws + (size_t)pos * S, us + (size_t)pos * S, sg);
            if (pos == 0) A.ctx_sign[p] = sg;
        }
    }
    if (nc == 0) return;                                            // D14: the best hypothesis' pose stays (uniform)
    wg_barrier_after_global_stores();
    const int sign0 = A.ctx_sign[p];
    PnpWork& W = s_w;

    if (tid < 3) W.cws[tid] = pnp_sum_chain(pws + tid, S, nc);     // choose_control_points (:292-333)
    wg_barrier();
    if (tid == 0) pnp_centroid(W, nc);
    wg_barrier();
    if (tid < 9) { const int a = tid / 3, b = tid - 3 * a; W.s3[tid] = pnp_pw0tpw0_chain(pws, S, nc, W.cws, a < b ? a : b, a < b ? b : a); }
    wg_barrier();
    if (tid == 0) pnp_control_points(W, nc);
    wg_barrier();
    for (int i = tid; i < nc; i += 256) pnp_alphas(W, pws + (size_t)i * S, alphas + (size_t)i * S);   // :349-360
    wg_barrier_after_global_stores();
    if (tid < 78) {                                                 // :237-242
        int a, b;
        pnp_mtm_pair(tid, a, b);
        const double v = pnp_mtm_chain(alphas, us, S, nc, a, b);
        W.mtm[12 * a + b] = v;
        W.mtm[12 * b + a] = v;
    }
    wg_barrier();
    if (tid < 64) {                                                 // :243-244, wave 0; its four groups compute the same, the first stores
        const int sw = jacobi12_group(W, tid & 15, tid < 16);
        if (tid == 0) W.sweeps[1] = sw;
    }
    wg_barrier();
    if (tid == 0) pnp_betas(W, nc);                                     // :246-263
    wg_barrier();
    for (int a = 0; a < 3; ++a) {                                   // compute_R_and_t (:543-553)
        if (tid == 0) pnp_ccs(W, a);
        wg_barrier();
        for (int i = tid; i < nc; i += 256) pnp_pcs(W, alphas + (size_t)i * S, pcs + (size_t)i * S);
        wg_barrier_after_global_stores();
        const bool flip = pnp_sign_flips(pcs[2], sign0);            // :524, uniform
        wg_barrier();                                               // every lane has read pcs[2]
        if (flip) {
            for (int i = tid; i < nc; i += 256)
                for (int c = 0; c < 3; ++c) pcs[(size_t)i * S + c] = -pcs[(size_t)i * S + c];
            if (tid < 12) W.ccs[tid] = -W.ccs[tid];
        }
        wg_barrier_after_global_stores();
        if (tid < 3) W.pc0[tid] = pnp_sum_chain(pcs + tid, S, nc);  // :447-457
        else if (tid < 6) W.pw0[tid - 3] = pnp_sum_chain(pws + (tid - 3), S, nc);
        wg_barrier();
        if (tid == 0) pnp_centroids(W, nc);
        wg_barrier();
        if (tid < 9) { const int r = tid / 3, c = tid - 3 * r; W.abt[tid] = pnp_abt_chain(pcs, pws, S, nc, W.pc0, W.pw0, r, c); }
        wg_barrier();
        if (tid == 0) pnp_R_and_t(W, a);
        wg_barrier();
        for (int i = tid; i < nc; i += 256)                         // the terms of reprojection_error; pcs of this approximation is dead
            pcs[(size_t)i * S] = pnp_reproj_term(pws + (size_t)i * S, us[(size_t)i * S], us[(size_t)i * S + 1], W.Rs + 9 * a, W.ts + 3 * a);
        wg_barrier_after_global_stores();
        if (tid == 0) {
            double sum2 = 0.0;
            for (int i = 0; i < nc; ++i) sum2 += pcs[(size_t)i * S];
            W.err[a] = sum2 / (double)(unsigned)nc;
        }
        wg_barrier();
    }
    if (tid == 0) {
        const int N = pnp_choose(W);
        for (int i = 0; i < 9; ++i) A.ctx_pose[(size_t)12 * p + i] = W.Rs[9 * N + i];
        for (int i = 0; i < 3; ++i) A.ctx_pose[(size_t)12 * p + 9 + i] = W.ts[3 * N + i];
        ctx[3] = nc;
    }
}

__global__ __launch_bounds__(256) void k_pnp_finish(PnpArgs A) {
    __shared__ double s_pose[12];
    __shared__ float s_tab[16];
    const int p = blockIdx.x, tid = threadIdx.x;
    const size_t row = (size_t)p * A.n_cap;
    const int count = clamp_count(A.counts, p, A.n_cap);
    const int32_t* ctx = A.ctx + (size_t)kPnpCtxInts * p;
    const int n = ctx[0], best_count = ctx[1], best_iter = ctx[2], refit = ctx[3];
    const bool enough = !(n < 4 || n < A.min_num_inliers);          // :76
    const bool ok = enough && best_count > A.min_num_inliers;       // :126
    const bool have = ok && best_iter >= 0 && best_iter < A.iters;
    if (tid < 12) {
        const double h = have ? pnp_hyp_field(A, p, tid)[best_iter] : 0.0;   // check_inliers' pose: the best hypothesis
        s_pose[tid] = h;
        const double v = have && refit > 0 ? A.ctx_pose[(size_t)12 * p + tid] : h;
        if (tid < 9) A.out_rot_cw[(size_t)9 * p + tid] = v;
        else A.out_trans_cw[(size_t)3 * p + tid - 9] = v;
    }
    if (tid < 16) s_tab[tid] = A.thr[tid];
    wg_barrier();
    if (tid == 0) {
        A.out_status[p] = !enough ? PLP_PNP_TOO_FEW_MATCHES : ok ? PLP_PNP_OK : PLP_PNP_TOO_FEW_INLIERS;
        A.out_num_matches[p] = n;
        A.out_num_inliers[p] = enough ? best_count : 0;
        A.out_best_iter[p] = ok ? best_iter : -1;
    }
    if (A.out_inliers) {
        for (int slot = tid; slot < count; slot += 256) {
            bool in = false;
            const size_t s = row + slot;
            if (have && A.valid[s] != 0) {
                const int o = A.octave[s];
                const bool lv = (unsigned)o < (unsigned)A.num_levels;
                in = pnp_inlier(s_pose, s_pose + 9, A.pos_w + 3 * s, A.bearing + 3 * s, lv ? s_tab[o] : 0.0f, !lv);
            }
            A.out_inliers[s] = in ? 1 : 0;
        }
    }
}

}  // namespace

hipError_t launch_pnp_ransac(hipStream_t st, const PnpArgs& A) {
    hipLaunchKernelGGL(k_pnp_prepare, dim3(A.P), dim3(256), 0, st, A);
    hipLaunchKernelGGL(k_pnp_hypotheses, dim3(A.P), dim3(256), 0, st, A);
    hipLaunchKernelGGL(k_pnp_count, dim3(A.P), dim3(256), 0, st, A);
    hipLaunchKernelGGL(k_pnp_refit, dim3(A.P), dim3(256), 0, st, A);
    hipLaunchKernelGGL(k_pnp_finish, dim3(A.P), dim3(256), 0, st, A);
    return hipGetLastError();
}

}  // namespace plp
