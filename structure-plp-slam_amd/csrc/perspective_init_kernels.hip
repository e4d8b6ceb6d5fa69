// Map initialisation of the perspective and fisheye cameras: the homography and the fundamental RANSAC of initialize::perspective::initialize and the
// choice between them (plp_perspective_ransac_*, include/plp_front.h).  The arithmetic is perspective_init.hpp's, which the
// host model runs too.
//
// The layout is essential_kernels.hip's with the solver (0 = H, 1 = F) as one more grid dimension: five launches of workgroups of four waves, one per
// problem in k_persp_prepare and k_persp_finish, one per problem, solver and 16 iterations in k_persp_hypotheses, one per problem, solver and 32
// hypotheses in k_persp_count, one per problem and solver in k_persp_refit.  No result depends on the lane mapping or on the order of the workgroups:
// every hypothesis is a pure function of the problem's inputs, a float sum is one accumulator in one lane over its items in their order, and the winner
// of a solver is the maximum of a key that is unique per iteration.
// k_persp_prepare:
//   1. the matched slots are compacted in slot order, 256 at a time, into the context.
//   2. solve::normalize of both frames over ALL their key points: the key points go through LDS in tiles of 256, staged by all lanes; lanes 0 .. 3
//      each own one of the four coordinate chains (x and y of frame 1, of frame 2) and add a tile up in key-point order, first the means, then, in a
//      second sweep, the mean absolute deviations.  Lane 0 forms the three 3 x 3 matrices the hypotheses de-normalise with.
// k_persp_hypotheses:
//   3. a hypothesis per group of 16 lanes.  Lane 0 of the group gathers the eight sampled point pairs, normalised, into the group's LDS record; lanes
//      0 .. 8 form one column of A^T A each and run the 9 x 9 Jacobi (essential_kernels.hip's, one column per lane); lane 0 runs the sign rule, F's
//      rank-two step, the de-normalisation and H's inverse.  The matrices go to the context.
// k_persp_count:
//   4. the chunk's matrices in LDS, the matched point pairs tiled through LDS, the residuals of (match, hypothesis) formed by all lanes, lane h adding
//      up hypothesis h's in match order; the packed-key maximum per solver by one 64-bit atomic maximum per workgroup.
// k_persp_refit:
//   5. per solver: the codes of the best hypothesis, its inliers' normalised pairs compacted in match order; with recompute and eight of them the 45
//      chains of A^T A one per lane, the Jacobi by wave 0, lane 0 finishing the matrix, and the second check with lane 0 adding in match order.  A
//      given homography skips to that check.
// k_persp_finish:
//   6. the statuses, the H/F choice and the outputs; the masks in two passes: the slots without a match, then the matches.
#include <hip/hip_runtime.h>

#include "perspective_init.hpp"
#include "plp_barrier.hpp"
#include "ransac_device.hpp"

namespace plp {
namespace {

constexpr int kPerspTile = 256;    // key points or matches per LDS tile: one per lane
constexpr int kPerspPass = 16;     // hypotheses per workgroup of k_persp_hypotheses: one per group of 16 lanes
constexpr int kPerspChunk = 32;    // hypotheses per workgroup of k_persp_count
constexpr int kPerspItems = 4096;  // (match, hypothesis) residual pairs per LDS round of k_persp_count

struct PerspWork {
    double pairs[kPerspMinSet * kPerspPairDoubles];   // the sampled point pairs, normalised, in sample order
    double null9[9];
    double g3[9], v3[9], key3[3], tmp[9];
    double out[18];
};

__device__ __forceinline__ int persp_best_iter(unsigned long long key) { return key != 0ull ? ransac_key_iter(key) : -1; }
__device__ __forceinline__ double* persp_hyp_field(const PerspArgs& A, int p, int solver, int field) {
    return A.ctx_hyp + (((size_t)p * 2 + solver) * kPerspHypDoubles + field) * A.iters;
}
__device__ __forceinline__ int32_t* persp_ctx(const PerspArgs& A, int p) { return A.ctx + (size_t)kPerspCtxInts * p; }

// the four coordinates of match k of problem p, as the key points hold them
__device__ __forceinline__ void persp_match_points(const PerspArgs& A, int p, int k, float& x1, float& y1, float& x2, float& y2) {
    const size_t row = (size_t)p * A.n_cap;
    const int s1 = A.ctx_slot[row + k];
    const plp_keypoint* k1 = A.undist_1 + row + s1;
    const plp_keypoint* k2 = A.undist_2 + (size_t)p * A.m_cap + A.match[row + s1];
    x1 = k1->x; y1 = k1->y; x2 = k2->x; y2 = k2->y;
}
// ... normalised (common.cc:52, :67) and widened, as compute_H_21 / compute_F_21 read them
__device__ __forceinline__ void persp_normalized_pair(const float* nrm, float x1, float y1, float x2, float y2, double* q) {
    q[0] = (double)persp_normalized(x1, nrm[0], nrm[2]);
    q[1] = (double)persp_normalized(y1, nrm[1], nrm[3]);
    q[2] = (double)persp_normalized(x2, nrm[4], nrm[6]);
    q[3] = (double)persp_normalized(y2, nrm[5], nrm[7]);
}

__global__ __launch_bounds__(256) void k_persp_prepare(PerspArgs A) {
    __shared__ int s_wave_n[4];
    __shared__ float s_v[4][kPerspTile];            // chain c: x and y of frame 1, x and y of frame 2
    __shared__ float s_mean[4], s_inv[4];           // by chain
    __shared__ float s_nrm[kPerspNormFloats];
    __shared__ double s_T[kPerspTDoubles], s_T2[9];
    const int p = blockIdx.x, tid = threadIdx.x;
    const size_t row = (size_t)p * A.n_cap, row2 = (size_t)p * A.m_cap;
    const int count_1 = clamp_count(A.counts_1, p, A.n_cap), count_2 = clamp_count(A.counts_2, p, A.m_cap);
    int n = 0;
    for (int base = 0; base < count_1; base += 256) {
        const int slot = base + tid;
        const bool v = slot < count_1 && persp_matched(A, p, slot, count_2);
        const int pos = wg_compact_step(v, n, s_wave_n);
        if (v) A.ctx_slot[row + pos] = (uint16_t)slot;
    }
    if (tid == 0) {
        int32_t* c = persp_ctx(A, p);
        c[0] = n;
        for (int i = 1; i < kPerspCtxInts; ++i) c[i] = 0;
        A.ctx_key[2 * (size_t)p] = 0ull;                            // the maxima k_persp_count's workgroups form
        A.ctx_key[2 * (size_t)p + 1] = 0ull;
    }

    // solve::normalize of both frames: chain tid < 4 is coordinate tid & 1 of frame tid >> 1
    const int cmax = count_1 > count_2 ? count_1 : count_2;
    const int mine = tid < 2 ? count_1 : count_2;
    for (int sweep = 0; sweep < 2; ++sweep) {
        const float mean = sweep != 0 && tid < 4 ? s_mean[tid] : 0.0f;   // behind the barrier that ended sweep 0
        float acc = 0;
        for (int base = 0; base < cmax; base += kPerspTile) {
            const int k = base + tid;
            if (k < count_1) { s_v[0][tid] = A.undist_1[row + k].x; s_v[1][tid] = A.undist_1[row + k].y; }
            if (k < count_2) { s_v[2][tid] = A.undist_2[row2 + k].x; s_v[3][tid] = A.undist_2[row2 + k].y; }
            wg_barrier();
            if (tid < 4) {
                const int m = mine - base < kPerspTile ? mine - base : kPerspTile;
                if (sweep == 0)
                    for (int q = 0; q < m; ++q) acc += s_v[tid][q];                          // common.cc:41-42
                else
                    for (int q = 0; q < m; ++q) acc += persp_dev_term(s_v[tid][q], mean);     // :52-56
            }
            wg_barrier();   // the next tile rewrites the arrays
        }
        if (tid < 4) {
            const float avg = persp_mean(acc, mine);                                          // :44-45, :59-60
            if (sweep == 0) s_mean[tid] = avg;
            else s_inv[tid] = persp_inv_dev(avg);                                             // :62-63
        }
        wg_barrier();
    }
    if (tid == 0) {                                                 // :71-75 and what find_via_ransac makes of transform_2 (:72; fundamental_solver.cc:62)
        for (int f = 0; f < 2; ++f) {
            s_nrm[4 * f] = s_mean[2 * f]; s_nrm[4 * f + 1] = s_mean[2 * f + 1];
            s_nrm[4 * f + 2] = s_inv[2 * f]; s_nrm[4 * f + 3] = s_inv[2 * f + 1];
        }
        persp_transform(s_nrm, s_T);
        persp_transform(s_nrm + 4, s_T2);
        persp_inv3(s_T2, s_T + 9);
        persp_transpose3(s_T2, s_T + 18);
        for (int i = 0; i < kPerspNormFloats; ++i) A.ctx_norm[(size_t)kPerspNormFloats * p + i] = s_nrm[i];
        for (int i = 0; i < kPerspTDoubles; ++i) A.ctx_T[(size_t)kPerspTDoubles * p + i] = s_T[i];
    }
}

// D24 item b, first half, by the 16-lane group of the calling lane, as in essential_kernels.hip: the null vector of the 9 x 9 matrix whose column
// jj this lane holds in g.  j = the lane within its group; lanes 9 .. 15 take part in the cross-lane reads only (lane 9 is the schedule's dummy
// column).  The whole wave must call it; write: whether this group stores its result.
__device__ __forceinline__ int persp_jacobi9_group(double (&g)[9], double* null9, int j, bool write) {
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

__global__ __launch_bounds__(256) void k_persp_hypotheses(PerspArgs A) {
    __shared__ PerspWork s_w[kPerspPass];
    __shared__ double s_T[kPerspTDoubles];
    __shared__ float s_nrm[kPerspNormFloats];
    const int p = blockIdx.x, solver = blockIdx.z, tid = threadIdx.x, grp = tid >> 4, j = tid & 15;
    const int n = persp_ctx(A, p)[0];
    const bool enough = n >= kPerspMinSet && !(solver == kPerspH && persp_given(A, p));   // homography_solver.cc:78; a given homography has no hypotheses
    if (tid < kPerspTDoubles) s_T[tid] = A.ctx_T[(size_t)kPerspTDoubles * p + tid];
    if (tid < kPerspNormFloats) s_nrm[tid] = A.ctx_norm[(size_t)kPerspNormFloats * p + tid];
    wg_barrier();
    PerspWork& W = s_w[grp];
    const int jj = j < 9 ? j : 0;
    const int it = (int)blockIdx.y * kPerspPass + grp;              // blockIdx.y: the pass of kPerspPass hypotheses
    const bool live = it < A.iters;
    bool have = false;
    if (j == 0) {
        int idx[8];
        have = live && enough && persp_sample(A, solver, p, it, n, idx);
#pragma unroll
        for (int k = 0; k < 8; ++k) {                               // :107-112, in the order given
            if (have) {
                float x1, y1, x2, y2;
                persp_match_points(A, p, idx[k], x1, y1, x2, y2);
                persp_normalized_pair(s_nrm, x1, y1, x2, y2, W.pairs + kPerspPairDoubles * k);
            } else {
                for (int c = 0; c < kPerspPairDoubles; ++c) W.pairs[kPerspPairDoubles * k + c] = 0.0;
            }
        }
    }
    __builtin_amdgcn_wave_barrier();
    double g[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) g[i] = persp_ata_chain(W.pairs, kPerspPairDoubles, kPerspMinSet, solver, i, jj);
    persp_jacobi9_group(g, W.null9, j, true);
    __builtin_amdgcn_wave_barrier();
    if (j == 0 && live) {
        if (have) {
            persp_from_null(solver, W.null9, s_T, W.g3, W.v3, W.key3, W.tmp, W.out);
            for (int i = 0; i < 18; ++i) persp_hyp_field(A, p, solver, i)[it] = W.out[i];
        }
        persp_hyp_field(A, p, solver, 18)[it] = have ? 1.0 : 0.0;
    }
}

__global__ __launch_bounds__(256) void k_persp_count(PerspArgs A) {
    __shared__ double s_M[18][kPerspChunk];         // the chunk's hypotheses, one per column
    __shared__ uint8_t s_has[kPerspChunk];
    __shared__ float s_pt[4][kPerspTile];
    __shared__ float s_ra[kPerspItems], s_rb[kPerspItems];
    __shared__ uint8_t s_code[kPerspItems];
    __shared__ unsigned long long s_part[4];
    const int p = blockIdx.x, solver = blockIdx.z, tid = threadIdx.x;
    const int n = persp_ctx(A, p)[0];
    const bool enough = n >= kPerspMinSet;
    float* out_hyp = solver == kPerspH ? A.out_hyp_score_h : A.out_hyp_score_f;

    unsigned long long key = 0;
    {
        const int chunk = (int)blockIdx.y * kPerspChunk;            // blockIdx.y: the chunk of kPerspChunk hypotheses
        const int it = chunk + tid;
        const int H = A.iters - chunk < kPerspChunk ? A.iters - chunk : kPerspChunk;   // lane h < H owns the score of hypothesis chunk + h
        const bool live = tid < H;
        const bool hyp = live && enough && persp_hyp_field(A, p, solver, 18)[it] != 0.0;
        if (tid < kPerspChunk) {
#pragma unroll
            for (int i = 0; i < 18; ++i) s_M[i][tid] = hyp ? persp_hyp_field(A, p, solver, i)[it] : 0.0;
            s_has[tid] = hyp ? 1 : 0;
        }
        float score = 0;
        if (enough) {   // uniform over the workgroup
            const int T = kPerspItems / H < kPerspTile ? kPerspItems / H : kPerspTile;   // matches per tile: T * H residual pairs fit the arrays
            for (int tile = 0; tile < n; tile += T) {
                const int m = n - tile < T ? n - tile : T;
                if (tid < m) {                                      // the readers of the previous tile's points are behind its second barrier
                    float x1, y1, x2, y2;
                    persp_match_points(A, p, tile + tid, x1, y1, x2, y2);
                    s_pt[0][tid] = x1; s_pt[1][tid] = y1; s_pt[2][tid] = x2; s_pt[3][tid] = y2;
                }
                wg_barrier();                                       // ... and the previous tile's sums have read its residuals
                for (int w = tid; w < m * H; w += 256) {            // the residuals of (match q, hypothesis h), all lanes
                    const int q = w / H, h = w - q * H;
                    if (s_has[h]) {
                        float ca, cb;
                        if (solver == kPerspH) {                    // uniform over the workgroup: H reads its matrix and the inverse, F its matrix alone
                            const double M[18] = {s_M[0][h], s_M[1][h], s_M[2][h], s_M[3][h], s_M[4][h], s_M[5][h], s_M[6][h], s_M[7][h], s_M[8][h],
                                                  s_M[9][h], s_M[10][h], s_M[11][h], s_M[12][h], s_M[13][h], s_M[14][h], s_M[15][h], s_M[16][h], s_M[17][h]};
                            s_code[w] = (uint8_t)hom_residuals(M, s_pt[0][q], s_pt[1][q], s_pt[2][q], s_pt[3][q], ca, cb);
                        } else {
                            const double M[9] = {s_M[0][h], s_M[1][h], s_M[2][h], s_M[3][h], s_M[4][h], s_M[5][h], s_M[6][h], s_M[7][h], s_M[8][h]};
                            s_code[w] = (uint8_t)fund_residuals(M, s_pt[0][q], s_pt[1][q], s_pt[2][q], s_pt[3][q], ca, cb);
                        }
                        s_ra[w] = ca; s_rb[w] = cb;
                    }
                }
                wg_barrier();
                if (hyp)
                    for (int q = 0; q < m; ++q) score = persp_score_add(score, s_code[q * H + tid], s_ra[q * H + tid], s_rb[q * H + tid]);   // in match order
            }
        }
        if (live) {
            if (out_hyp) out_hyp[(size_t)p * A.iters + it] = persp_out(score);
            if (score > 0.0f) {                                     // :122 against best_score_ = 0.0 (:85); false for a NaN
                const unsigned long long mine = ransac_key(__float_as_uint(score), it);
                key = mine > key ? mine : key;
            }
        }
    }
    key = wg_max_u64(key, s_part);
    if (tid == 0 && key != 0ull) atomicMax(A.ctx_key + 2 * (size_t)p + solver, key);   // a maximum: the order of the workgroups does not matter
}

__global__ __launch_bounds__(256) void k_persp_refit(PerspArgs A) {
    __shared__ double s_M[18];
    __shared__ double s_A[81];
    __shared__ double s_T[kPerspTDoubles];
    __shared__ float s_nrm[kPerspNormFloats];
    __shared__ PerspWork s_w;
    __shared__ float s_ra[kPerspTile], s_rb[kPerspTile];
    __shared__ int s_code[kPerspTile];
    __shared__ int s_wave_n[4];
    const int p = blockIdx.x, solver = blockIdx.y, tid = threadIdx.x;
    const size_t srow = ((size_t)p * 2 + solver) * A.n_cap;
    int32_t* ctx = persp_ctx(A, p) + 2 + 3 * solver;
    const int n = persp_ctx(A, p)[0];
    if (n < kPerspMinSet) return;                                   // uniform over the workgroup
    const bool given = solver == kPerspH && persp_given(A, p);
    double* ctx_M = A.ctx_M + ((size_t)p * 2 + solver) * 18;
    uint8_t* code_of = A.ctx_code + srow;
    if (tid < kPerspTDoubles) s_T[tid] = A.ctx_T[(size_t)kPerspTDoubles * p + tid];
    if (tid < kPerspNormFloats) s_nrm[tid] = A.ctx_norm[(size_t)kPerspNormFloats * p + tid];

    if (given) {                                                    // homography_solver.cc:398: the caller's matrix, checked below
        if (tid < 9) s_M[tid] = A.given_H_21[(size_t)9 * p + tid];
        wg_barrier();
        if (tid == 0) {
            persp_inv3(s_M, s_M + 9);
            for (int i = 0; i < 18; ++i) ctx_M[i] = s_M[i];
        }
        wg_barrier();
    } else {
        const int best_iter = persp_best_iter(A.ctx_key[2 * (size_t)p + solver]);
        if (!(best_iter >= 0 && best_iter < A.iters)) return;       // uniform
        if (tid < 18) s_M[tid] = persp_hyp_field(A, p, solver, tid)[best_iter];
        wg_barrier();

        // is_inlier_match_ of the best hypothesis (:126) and, for :144-151, its inliers' normalised points in match order
        double* pairs = A.ctx_pairs + srow * kPerspPairDoubles;
        int nc = 0;
        for (int base = 0; base < n; base += 256) {
            const int k = base + tid;
            bool in = false;
            float x1 = 0, y1 = 0, x2 = 0, y2 = 0;
            if (k < n) {
                persp_match_points(A, p, k, x1, y1, x2, y2);
                float ca, cb;
                const int code = persp_residuals(solver, s_M, x1, y1, x2, y2, ca, cb);
                code_of[k] = (uint8_t)code;
                in = code == 3;
            }
            const int pos = wg_compact_step(in, nc, s_wave_n);
            if (in) persp_normalized_pair(s_nrm, x1, y1, x2, y2, pairs + (size_t)pos * kPerspPairDoubles);
        }
        if (!(A.recompute != 0 && nc >= kPerspMinSet)) {            // :130-136 (the score of the best hypothesis is > 0); uniform
            if (tid == 0) ctx[1] = nc;
            return;
        }
        wg_barrier_after_global_stores();

        if (tid < 45) {                                             // :152, compute_H_21 / compute_F_21 over the inliers
            int a, b;
            ess_ata_pair(tid, a, b);
            const double v = persp_ata_chain(pairs, kPerspPairDoubles, nc, solver, a, b);
            s_A[9 * a + b] = v;
            s_A[9 * b + a] = v;
        }
        wg_barrier();
        if (tid < 64) {                                             // wave 0; its four groups compute the same, the first stores
            const int j = tid & 15, jj = j < 9 ? j : 0;
            double g[9];
#pragma unroll
            for (int i = 0; i < 9; ++i) g[i] = s_A[9 * i + jj];
            persp_jacobi9_group(g, s_w.null9, j, tid < 16);
        }
        wg_barrier();
        if (tid == 0) {                                             // :153
            persp_from_null(solver, s_w.null9, s_T, s_w.g3, s_w.v3, s_w.key3, s_w.tmp, s_w.out);
            for (int i = 0; i < 18; ++i) { s_M[i] = s_w.out[i]; ctx_M[i] = s_w.out[i]; }
        }
        wg_barrier();
    }

    float score = 0;                                                // :154 / :398, check_inliers of the matrix that is returned; lane 0's accumulator
    int num = 0;
    for (int tile = 0; tile < n; tile += kPerspTile) {
        const int k = tile + tid;
        if (k < n) {
            float x1, y1, x2, y2, ca, cb;
            persp_match_points(A, p, k, x1, y1, x2, y2);
            const int code = persp_residuals(solver, s_M, x1, y1, x2, y2, ca, cb);
            code_of[k] = (uint8_t)code;
            s_ra[tid] = ca; s_rb[tid] = cb; s_code[tid] = code;
        }
        wg_barrier();
        if (tid == 0) {
            const int m = n - tile < kPerspTile ? n - tile : kPerspTile;
            for (int q = 0; q < m; ++q) {
                score = persp_score_add(score, s_code[q], s_ra[q], s_rb[q]);
                num += s_code[q] == 3 ? 1 : 0;
            }
        }
        wg_barrier();   // the next tile rewrites the arrays
    }
    if (tid == 0) {
        ctx[0] = (int32_t)__float_as_uint(score);
        ctx[1] = num;
        ctx[2] = 1;
    }
}

__global__ __launch_bounds__(256) void k_persp_finish(PerspArgs A) {
    const int p = blockIdx.x, tid = threadIdx.x;
    const size_t row = (size_t)p * A.n_cap;
    const int count_1 = clamp_count(A.counts_1, p, A.n_cap), count_2 = clamp_count(A.counts_2, p, A.m_cap);
    const int32_t* ctx = persp_ctx(A, p);
    const int n = ctx[0];
    const bool enough = n >= kPerspMinSet;
    bool valid[2];
    float score[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const int32_t* c = ctx + 2 + 3 * s;
        const unsigned long long key = A.ctx_key[2 * (size_t)p + s];
        const int best_iter = persp_best_iter(key), num = c[1], second = c[2];
        const bool given = s == kPerspH && persp_given(A, p);
        const float sc = !enough ? 0.0f : second != 0 ? __uint_as_float((unsigned)c[0]) : given ? 0.0f : __uint_as_float((unsigned)(key >> 32));
        const bool ok = given ? enough && sc > 0.0f && A.given_H_num_inliers[p] >= kPerspMinSet                           // homography_solver.cc:401-402
                              : (enough && best_iter >= 0 && best_iter < A.iters && num >= kPerspMinSet) || (enough && second != 0);   // :131; the refit's count may be lower
        valid[s] = ok; score[s] = sc;
        const bool from_ctx = given || second != 0;
        double* out_M = s == kPerspH ? A.out_H_21 : A.out_F_21;
        if (tid < 9)
            out_M[(size_t)9 * p + tid] = !ok ? 0.0 : persp_out(from_ctx ? A.ctx_M[((size_t)p * 2 + s) * 18 + tid] : persp_hyp_field(A, p, s, tid)[best_iter]);
        if (tid == 0) {
            (s == kPerspH ? A.out_status_h : A.out_status_f)[p] = !enough ? PLP_PERSPECTIVE_TOO_FEW_MATCHES : ok ? PLP_PERSPECTIVE_OK : PLP_PERSPECTIVE_INVALID;
            (s == kPerspH ? A.out_score_h : A.out_score_f)[p] = persp_out(sc);
            (s == kPerspH ? A.out_num_inliers_h : A.out_num_inliers_f)[p] = ok ? num : 0;
            (s == kPerspH ? A.out_best_iter_h : A.out_best_iter_f)[p] = ok && !given ? best_iter : -1;
        }
    }
    float rel;
    const int choice = persp_choice(score[0], score[1], valid[0], valid[1], rel);
    if (tid == 0) {
        A.out_num_matches[p] = n;
        A.out_rel_score_h[p] = persp_out(rel);
        A.out_choice[p] = (uint8_t)choice;
    }
    for (int o = 0; o < 3; ++o) {                                   // the chosen mask, H's, F's
        uint8_t* out = o == 0 ? A.out_inliers : o == 1 ? A.out_inliers_h : A.out_inliers_f;
        if (!out) continue;
        const int s = o == 0 ? (choice == PLP_PERSPECTIVE_CHOICE_F ? kPerspF : kPerspH) : o - 1;
        const bool on = o == 0 ? choice != PLP_PERSPECTIVE_CHOICE_NONE : o == 1 ? valid[0] : valid[1];
        const uint8_t* code_of = A.ctx_code + ((size_t)p * 2 + s) * A.n_cap;
        for (int slot = tid; slot < count_1; slot += 256)
            if (!persp_matched(A, p, slot, count_2)) out[row + slot] = 0;
        for (int k = tid; k < n; k += 256) out[row + A.ctx_slot[row + k]] = on ? (code_of[k] == 3 ? 1 : 0) : 0;
    }
}

}  // namespace

hipError_t launch_perspective_ransac(hipStream_t st, const PerspArgs& A) {
    hipLaunchKernelGGL(k_persp_prepare, dim3(A.P), dim3(256), 0, st, A);
    hipLaunchKernelGGL(k_persp_hypotheses, dim3(A.P, (A.iters + kPerspPass - 1) / kPerspPass, 2), dim3(256), 0, st, A);
    hipLaunchKernelGGL(k_persp_count, dim3(A.P, (A.iters + kPerspChunk - 1) / kPerspChunk, 2), dim3(256), 0, st, A);
    hipLaunchKernelGGL(k_persp_refit, dim3(A.P, 2), dim3(256), 0, st, A);
    hipLaunchKernelGGL(k_persp_finish, dim3(A.P), dim3(256), 0, st, A);
    return hipGetLastError();
}

}  // namespace plp
