// Map initialisation and the tracker's robust match: solve::essential_solver's find_via_ransac (plp_essential_ransac_*, include/plp_front.h;
// DESIGN.md section 5, D24).  The arithmetic is essential.hpp's, which the host model runs too.
//
// Five launches of workgroups of four waves: one per problem in k_ess_prepare, k_ess_refit and k_ess_finish, one per problem and 16 iterations in
// k_ess_hypotheses, one per problem and 32 hypotheses in k_ess_count.  No result depends on the lane mapping or on the order of the workgroups: every hypothesis is a pure function
// of the problem's inputs, the rotations of one round of the Jacobi schedule touch disjoint columns, the score of a hypothesis is one float
// accumulator over the matches in match order, the winner is the maximum of a key that is unique per iteration, and every sum over bearing
// pairs is one accumulator in match order.
// k_ess_prepare:
//   1. the matched slots are compacted in slot order, 256 at a time (64-bit ballot within the wave, the waves' totals through LDS), into the
//      context: slot[k], k being what a sample index means.
// k_ess_hypotheses:
//   2. a hypothesis goes to a group of 16 lanes (one DPP row), kEssPass = 16 per workgroup, a workgroup per problem and pass of 16
//      iterations (the passes share nothing, so they run side by side on other compute units).  Lane 0 of the group gathers the eight
//      sampled bearing pairs into the group's EssWork in LDS; lanes 0 .. 8 then form one column of A^T A each, straight into the registers
//      that hold their column of G (18 doubles with V, every index a compile-time constant), and run the 9 x 9 Jacobi, a round = one
//      cross-lane fetch of the partner's two columns, both lanes of a pair forming the three dot products in the same order; the null vector
//      goes back to LDS and lane 0 runs the sign rule and the 3 x 3 step there.  E_21 goes to the call's context buffer.
// k_ess_count:
//   3. a workgroup per problem and chunk of kEssChunk = 32 hypotheses, their matrices in LDS; the matches' bearing pairs go through LDS in
//      tiles of T matches, T * H <= kEssItems for the H hypotheses of the chunk.  The residuals of a tile -- the divisions and square roots, independent per (match, hypothesis) -- are
//      formed by all 256 lanes into LDS; then lane h adds up hypothesis h's in match order: the float score of a lane is the reference's
//      accumulator, and only its two additions per match are serial.  The best hypothesis is the maximum of
//      (score bits << 32 | ~iter) over the scores that are > 0 (non-negative floats order as their bits; a NaN is not > 0): over the
//      workgroup by shuffles and LDS, over the problem's workgroups by one 64-bit atomic maximum each on a word k_ess_prepare zeroed.
// k_ess_refit:
//   4. the matches' codes under the best hypothesis, its inliers compacted in match order into the context's pair buffer; with recompute and
//      at least eight of them (:96-118) the 45 distinct entries of A^T A are chains of essential.hpp, one per lane, the Jacobi is the device
//      function of 2 run by wave 0, lane 0 finishes the matrix, and the second check_inliers forms the residuals on all lanes, tile by tile,
//      with lane 0 adding them up in match order.
// k_ess_finish:
//   5. lane 0 writes the outputs and two passes write out_inliers: the slots without a match, then the matches.
// The launches hand their results on through buffers the context owns: the calls of one context must be ordered on the device.
#include <hip/hip_runtime.h>

#include "essential.hpp"
#include "plp_barrier.hpp"
#include "ransac_device.hpp"

namespace plp {
namespace {

constexpr int kEssTile = 256;    // matches per LDS tile at most: one per lane
constexpr int kEssPass = 16;     // hypotheses per workgroup of k_ess_hypotheses: one per group of 16 lanes
constexpr int kEssChunk = 32;    // hypotheses per workgroup of k_ess_count
constexpr int kEssItems = 4096;  // (match, hypothesis) residual pairs per LDS round of k_ess_count

struct EssWork {
    double pairs[kEssMinSet * kEssPairDoubles];   // the sampled bearing pairs, in sample order
    double null9[9];
    double g3[9], v3[9], key3[3];
    double E[9];
};

// the winner of k_ess_count's key (score bits << 32 | ~iter; 0 = no hypothesis scored above 0)
__device__ __forceinline__ int ess_best_iter(unsigned long long key) { return key != 0ull ? ransac_key_iter(key) : -1; }

__device__ __forceinline__ double* ess_hyp_field(const EssArgs& A, int p, int field) { return A.ctx_hyp + ((size_t)p * kEssHypDoubles + field) * A.iters; }

__global__ __launch_bounds__(256) void k_ess_prepare(EssArgs A) {
    __shared__ int s_wave_n[4];
    const int p = blockIdx.x, tid = threadIdx.x;
    const size_t row = (size_t)p * A.n_cap;
    const int count_1 = clamp_count(A.counts_1, p, A.n_cap), count_2 = clamp_count(A.counts_2, p, A.m_cap);
    int n = 0;
    for (int base = 0; base < count_1; base += 256) {
        const int slot = base + tid;
        const bool v = slot < count_1 && ess_matched(A, p, slot, count_2);
        const int pos = wg_compact_step(v, n, s_wave_n);
        if (v) A.ctx_slot[row + pos] = (uint16_t)slot;
    }
    if (tid == 0) {
        int32_t* c = A.ctx + (size_t)kEssCtxInts * p;
        c[0] = n; c[1] = 0; c[2] = 0; c[3] = 0; c[4] = 0;
        A.ctx_key[p] = 0ull;                                        // the maximum k_ess_count's workgroups form
    }
}

// D24 item b, first half, by the 16-lane group of the calling lane: the null vector of the 9 x 9 matrix whose column jj this lane holds in
// g.  j = the lane within its group; lanes 9 .. 15 take part in the cross-lane reads only (lane 9 is the schedule's dummy column).  The
// whole wave must call it; write: whether this group stores its result.  Returns the sweeps that rotated.
__device__ __forceinline__ int jacobi9_group(double (&g)[9], double* null9, int j, bool write) {
    const int lane = threadIdx.x & 63;
    double v[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) v[i] = i == j ? 1.0 : 0.0;
    int sweeps = 0;
    bool done = false;
    while (__ballot(!done) != 0ull) {                               // uniform over the wave; a group that is done rotates nothing
        bool rotated = false;
        for (int r = 0; r < 9; ++r) {
            const int q = j < 9 ? jacobi_partner(j, r, 10) : j;
            const bool lo = j < q;
            double pg[9], pv[9];
#pragma unroll
            for (int i = 0; i < 9; ++i) {
                pg[i] = __shfl(g[i], q, 16);
                pv[i] = __shfl(v[i], q, 16);
            }
            double alpha = 0.0, beta = 0.0, gamma = 0.0;
#pragma unroll
            for (int i = 0; i < 9; ++i) {
                const double a = lo ? g[i] : pg[i], b = lo ? pg[i] : g[i];   // the pair's lower column first, in both lanes
                alpha = alpha + a * a;
                beta = beta + b * b;
                gamma = gamma + a * b;
            }
            double c = 1.0, s = 0.0;
            const bool rot = hestenes_cs(alpha, beta, gamma, c, s) && !done && j < 9 && q < 9;
            if (rot) {
#pragma unroll
                for (int i = 0; i < 9; ++i) {
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
    for (int i = 0; i < 9; ++i) n2 = n2 + g[i] * g[i];
    const double key = jacobi_key(n2);
    int rank = 0;
#pragma unroll
    for (int k = 0; k < 9; ++k) rank += jacobi_before(__shfl(key, k, 16), k, key, j) ? 1 : 0;
    if (write && j < 9 && rank == 8) {
#pragma unroll
        for (int i = 0; i < 9; ++i) null9[i] = v[i];
    }
    return sweeps;
}

__global__ __launch_bounds__(256) void k_ess_hypotheses(EssArgs A) {
    __shared__ EssWork s_w[kEssPass];
    const int p = blockIdx.x, tid = threadIdx.x, grp = tid >> 4, j = tid & 15;
    const size_t row = (size_t)p * A.n_cap;
    const int n = A.ctx[(size_t)kEssCtxInts * p];
    const bool enough = n >= kEssMinSet;                            // :45
    EssWork& W = s_w[grp];
    const int jj = j < 9 ? j : 0;
    {                                                               // blockIdx.y: the pass of kEssPass hypotheses
        const int it = (int)blockIdx.y * kEssPass + grp;
        const bool live = it < A.iters;
        bool have = false;
        if (j == 0) {
            int idx[8];
            have = live && enough && ransac_sample<kEssMinSet>(A, p, it, n, idx);
#pragma unroll
            for (int k = 0; k < 8; ++k) {                           // :73-78, in the order given
                if (have) {
                    const int s1 = A.ctx_slot[row + idx[k]];
                    const double* b1 = A.bearing_1 + 3 * (row + s1);
                    const double* b2 = A.bearing_2 + 3 * ((size_t)p * A.m_cap + A.match[row + s1]);
                    for (int c = 0; c < 3; ++c) { W.pairs[kEssPairDoubles * k + c] = b1[c]; W.pairs[kEssPairDoubles * k + 3 + c] = b2[c]; }
                } else {
                    for (int c = 0; c < kEssPairDoubles; ++c) W.pairs[kEssPairDoubles * k + c] = 0.0;
                }
            }
        }
        __builtin_amdgcn_wave_barrier();
        double g[9];
#pragma unroll
        for (int i = 0; i < 9; ++i) g[i] = ess_ata_chain(W.pairs, kEssPairDoubles, kEssMinSet, i, jj);
        jacobi9_group(g, W.null9, j, true);
        __builtin_amdgcn_wave_barrier();
        if (j == 0 && live) {
            if (have) {
                ess_from_null(W.null9, W.g3, W.v3, W.key3, W.E);
                for (int i = 0; i < 9; ++i) ess_hyp_field(A, p, i)[it] = W.E[i];
            }
            ess_hyp_field(A, p, 9)[it] = have ? 1.0 : 0.0;
        }
    }
}

__global__ __launch_bounds__(256) void k_ess_count(EssArgs A) {
    __shared__ double s_E[9][kEssChunk];            // the chunk's hypotheses, one per column
    __shared__ uint8_t s_has[kEssChunk];
    __shared__ double s_b[kEssPairDoubles][kEssTile];
    __shared__ float s_r2[kEssItems], s_r1[kEssItems];
    __shared__ uint8_t s_code[kEssItems];
    __shared__ unsigned long long s_part[4];
    const int p = blockIdx.x, tid = threadIdx.x;
    const size_t row = (size_t)p * A.n_cap;
    const int n = A.ctx[(size_t)kEssCtxInts * p];
    const bool enough = n >= kEssMinSet;                            // :45

    unsigned long long key = 0;
    {
        const int chunk = (int)blockIdx.y * kEssChunk;                  // blockIdx.y: the chunk of kEssChunk hypotheses
        const int it = chunk + tid;
        const int H = A.iters - chunk < kEssChunk ? A.iters - chunk : kEssChunk;   // lane h < H owns the score of hypothesis chunk + h
        const bool live = tid < H;
        const bool hyp = live && enough && ess_hyp_field(A, p, 9)[it] != 0.0;
        if (tid < kEssChunk) {
#pragma unroll
            for (int i = 0; i < 9; ++i) s_E[i][tid] = hyp ? ess_hyp_field(A, p, i)[it] : 0.0;
            s_has[tid] = hyp ? 1 : 0;
        }
        float score = 0;
        if (enough) {   // uniform over the workgroup
            const int T = kEssItems / H < kEssTile ? kEssItems / H : kEssTile;   // matches per tile: T * H residual pairs fit the arrays
            for (int tile = 0; tile < n; tile += T) {
                const int m = n - tile < T ? n - tile : T;
                if (tid < m) {                                      // the readers of the previous tile's bearings are behind its second barrier
                    const int s1 = A.ctx_slot[row + tile + tid];
                    const double* b1 = A.bearing_1 + 3 * (row + s1);
                    const double* b2 = A.bearing_2 + 3 * ((size_t)p * A.m_cap + A.match[row + s1]);
#pragma unroll
                    for (int r = 0; r < 3; ++r) { s_b[r][tid] = b1[r]; s_b[3 + r][tid] = b2[r]; }
                }
                wg_barrier();                                       // ... and the previous tile's sums have read its residuals
                for (int w = tid; w < m * H; w += 256) {            // the residuals of (match q, hypothesis h), all lanes
                    const int q = w / H, h = w - q * H;
                    if (s_has[h]) {
                        const double E[9] = {s_E[0][h], s_E[1][h], s_E[2][h], s_E[3][h], s_E[4][h], s_E[5][h], s_E[6][h], s_E[7][h], s_E[8][h]};
                        const double b1[3] = {s_b[0][q], s_b[1][q], s_b[2][q]}, b2[3] = {s_b[3][q], s_b[4][q], s_b[5][q]};
                        float r2, r1;
                        s_code[w] = (uint8_t)ess_residuals(E, b1, b2, r2, r1);
                        s_r2[w] = r2; s_r1[w] = r1;
                    }
                }
                wg_barrier();
                if (hyp)
                    for (int q = 0; q < m; ++q) score = ess_score_add(score, s_code[q * H + tid], s_r2[q * H + tid], s_r1[q * H + tid]);   // in match order
            }
        }
        if (live) {
            if (A.out_hyp_score) A.out_hyp_score[(size_t)p * A.iters + it] = score;
            if (score > 0.0f) {                                     // :87 against best_score_ = 0.0 (:52); false for a NaN
                const unsigned long long mine = ransac_key(__float_as_uint(score), it);
                key = mine > key ? mine : key;
            }
        }
    }
    key = wg_max_u64(key, s_part);
    if (tid == 0 && key != 0ull) atomicMax(A.ctx_key + p, key);       // a maximum: the order of the workgroups does not matter
}

__global__ __launch_bounds__(256) void k_ess_refit(EssArgs A) {
    __shared__ double s_E[9];
    __shared__ double s_M[81];
    __shared__ EssWork s_w;
    __shared__ float s_r2[kEssTile], s_r1[kEssTile];
    __shared__ int s_code[kEssTile];
    __shared__ int s_wave_n[4];
    const int p = blockIdx.x, tid = threadIdx.x;
    const size_t row = (size_t)p * A.n_cap;
    int32_t* ctx = A.ctx + (size_t)kEssCtxInts * p;
    const int n = ctx[0], best_iter = ess_best_iter(A.ctx_key[p]);
    if (!(n >= kEssMinSet && best_iter >= 0 && best_iter < A.iters)) return;   // uniform over the workgroup
    if (tid < 9) s_E[tid] = ess_hyp_field(A, p, tid)[best_iter];
    wg_barrier();

    // is_inlier_match_ of the best hypothesis (:91) and, for :109-116, its inliers in match order
    double* pairs = A.ctx_pairs + row * kEssPairDoubles;
    int nc = 0;
    for (int base = 0; base < n; base += 256) {
        const int k = base + tid;
        bool in = false;
        double b1[3] = {0, 0, 0}, b2[3] = {0, 0, 0};
        if (k < n) {
            const int s1 = A.ctx_slot[row + k];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                b1[c] = A.bearing_1[3 * (row + s1) + c];
                b2[c] = A.bearing_2[3 * ((size_t)p * A.m_cap + A.match[row + s1]) + c];
            }
            float r2, r1;
            const int code = ess_residuals(s_E, b1, b2, r2, r1);
            A.ctx_code[row + k] = (uint8_t)code;
            in = code == 3;
        }
        const int pos = wg_compact_step(in, nc, s_wave_n);
        if (in) {
#pragma unroll
            for (int c = 0; c < 3; ++c) { pairs[(size_t)pos * kEssPairDoubles + c] = b1[c]; pairs[(size_t)pos * kEssPairDoubles + 3 + c] = b2[c]; }
        }
    }
    if (!(A.recompute != 0 && nc >= kEssMinSet)) {                  // :96-101 (the score of the best hypothesis is > 0); uniform
        if (tid == 0) ctx[3] = nc;
        return;
    }
    wg_barrier_after_global_stores();

    if (tid < 45) {                                                 // :117, compute_E_21 over the inliers (:128-135)
        int a, b;
        ess_ata_pair(tid, a, b);
        const double v = ess_ata_chain(pairs, kEssPairDoubles, nc, a, b);
        s_M[9 * a + b] = v;
        s_M[9 * b + a] = v;
    }
    wg_barrier();
    if (tid < 64) {                                                 // :137-139, wave 0; its four groups compute the same, the first stores
        const int j = tid & 15, jj = j < 9 ? j : 0;
        double g[9];
#pragma unroll
        for (int i = 0; i < 9; ++i) g[i] = s_M[9 * i + jj];
        jacobi9_group(g, s_w.null9, j, tid < 16);
    }
    wg_barrier();
    if (tid == 0) {                                                 // :141-151
        ess_from_null(s_w.null9, s_w.g3, s_w.v3, s_w.key3, s_w.E);
        for (int i = 0; i < 9; ++i) { s_E[i] = s_w.E[i]; A.ctx_E[(size_t)9 * p + i] = s_w.E[i]; }
    }
    wg_barrier();

    float score = 0;                                                // :118, the second check_inliers; lane 0's accumulator
    int num = 0;
    for (int tile = 0; tile < n; tile += kEssTile) {
        const int k = tile + tid;
        if (k < n) {
            const int s1 = A.ctx_slot[row + k];
            double b1[3], b2[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                b1[c] = A.bearing_1[3 * (row + s1) + c];
                b2[c] = A.bearing_2[3 * ((size_t)p * A.m_cap + A.match[row + s1]) + c];
            }
            float r2, r1;
            const int code = ess_residuals(s_E, b1, b2, r2, r1);
            A.ctx_code[row + k] = (uint8_t)code;
            s_r2[tid] = r2; s_r1[tid] = r1; s_code[tid] = code;
        }
        wg_barrier();
        if (tid == 0) {
            const int m = n - tile < kEssTile ? n - tile : kEssTile;
            for (int q = 0; q < m; ++q) {
                score = ess_score_add(score, s_code[q], s_r2[q], s_r1[q]);
                num += s_code[q] == 3 ? 1 : 0;
            }
        }
        wg_barrier();   // the next tile rewrites the arrays
    }
    if (tid == 0) {
        ctx[2] = (int32_t)__float_as_uint(score);
        ctx[3] = num;
        ctx[4] = 1;
    }
}

__global__ __launch_bounds__(256) void k_ess_finish(EssArgs A) {
    const int p = blockIdx.x, tid = threadIdx.x;
    const size_t row = (size_t)p * A.n_cap;
    const int count_1 = clamp_count(A.counts_1, p, A.n_cap), count_2 = clamp_count(A.counts_2, p, A.m_cap);
    const int32_t* ctx = A.ctx + (size_t)kEssCtxInts * p;
    const unsigned long long key = A.ctx_key[p];
    const int n = ctx[0], best_iter = ess_best_iter(key), num = ctx[3], refit = ctx[4];
    const bool enough = n >= kEssMinSet;                            // :45
    const bool ok = enough && best_iter >= 0 && best_iter < A.iters && num >= kEssMinSet;   // :96; with the refit, its count may be lower (D24 item e)
    const bool valid = ok || (enough && refit != 0);
    if (tid < 9) A.out_E_21[(size_t)9 * p + tid] = !valid ? 0.0 : refit != 0 ? A.ctx_E[(size_t)9 * p + tid] : ess_hyp_field(A, p, tid)[best_iter];
    if (tid == 0) {
        A.out_status[p] = !enough ? PLP_ESSENTIAL_TOO_FEW_MATCHES : valid ? PLP_ESSENTIAL_OK : PLP_ESSENTIAL_INVALID;
        A.out_num_matches[p] = n;
        A.out_score[p] = valid ? __uint_as_float(refit != 0 ? (unsigned)ctx[2] : (unsigned)(key >> 32)) : 0.0f;
        A.out_num_inliers[p] = valid ? num : 0;
        A.out_best_iter[p] = valid ? best_iter : -1;
    }
    if (A.out_inliers) {
        for (int slot = tid; slot < count_1; slot += 256)
            if (!ess_matched(A, p, slot, count_2)) A.out_inliers[row + slot] = 0;
        for (int k = tid; k < n; k += 256) A.out_inliers[row + A.ctx_slot[row + k]] = valid && A.ctx_code[row + k] == 3 ? 1 : 0;
    }
}

}  // namespace

hipError_t launch_essential_ransac(hipStream_t st, const EssArgs& A) {
    hipLaunchKernelGGL(k_ess_prepare, dim3(A.P), dim3(256), 0, st, A);
    hipLaunchKernelGGL(k_ess_hypotheses, dim3(A.P, (A.iters + kEssPass - 1) / kEssPass), dim3(256), 0, st, A);
    hipLaunchKernelGGL(k_ess_count, dim3(A.P, (A.iters + kEssChunk - 1) / kEssChunk), dim3(256), 0, st, A);
    hipLaunchKernelGGL(k_ess_refit, dim3(A.P), dim3(256), 0, st, A);
    hipLaunchKernelGGL(k_ess_finish, dim3(A.P), dim3(256), 0, st, A);
    return hipGetLastError();
}

}  // namespace plp
