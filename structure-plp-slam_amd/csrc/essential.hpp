// solve::essential_solver (solve/essential_solver.cc:33-253), one definition of the arithmetic for host and device (plp_essential_ransac_* /
// plp_model_essential_ransac_host, plp_model_essential_fit_host, plp_model_essential_check_host, plp_model_essential_draw_host,
// include/plp_front.h): compute_E_21 and the loop body of check_inliers; the samples are ransac.hpp's at K = 8 (D24 item d).  f64 with IEEE
// + - * / sqrt only, every sum left to right, floats where the reference holds floats; translation units that include this file are compiled
// with -ffp-contract=off.  The two Eigen::JacobiSVD uses of compute_E_21 are the one-sided Jacobi of jacobi.hpp (D14), hestenes().
//
// Everything here works on memory the caller names: on the device that is LDS or a context buffer, reached with run-time indices, so that no
// kernel keeps an indexed array in registers; on the host it is the stack.  The sums over bearing pairs are `chain` functions, one accumulator
// each: the host runs them one after the other, the kernels one per lane.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/plp_front.h"
#include "jacobi.hpp"
#include "ransac.hpp"

namespace plp {

constexpr int kEssMaxSlots = 8192;                    // n_cap limit of the entries (a rank fits 16 bits)
constexpr int kEssMaxIters = 65536;                   // iters limit of the entries (a workgroup of k_ess_hypotheses per 16 of them)
constexpr int kEssMinSet = 8;                         // min_set_size (:44)
constexpr int kEssCtxInts = 5;                        // per problem: num_matches, (free), the refit's score bits, num_inliers, whether the refit ran
constexpr int kEssHypDoubles = 10;                    // per hypothesis: E_21 (9, row-major), whether it exists
constexpr int kEssPairDoubles = 6;                    // per bearing pair of a fit: bearing_1 (3), bearing_2 (3)
constexpr float kEssResidualCosThr = 0.01745240643f;  // residual_cos_thr (:207)

// entry `col` of the row of A that a bearing pair gives (:130-135): A(i, 3 r + c) = bearing_2(r) * bearing_1(c)
__host__ __device__ __forceinline__ double ess_a(const double* b1, const double* b2, int col) {
    const int r = col / 3, c = col - 3 * r;
    return b2[r] * b1[c];
}
// entry (a, b) of A^T A over nc bearing pairs held `stride` doubles apart (bearing_1 at pairs, bearing_2 at pairs + 3), in their order
__host__ __device__ __forceinline__ double ess_ata_chain(const double* pairs, int stride, int nc, int a, int b) {
    double acc = 0.0;
    for (int i = 0; i < nc; ++i) {
        const double* q = pairs + (size_t)i * stride;
        acc = acc + ess_a(q, q + 3, a) * ess_a(q, q + 3, b);
    }
    return acc;
}
// entry (a, b), a <= b, of the upper triangle of the 9 x 9 matrix as the index of its chain, 0 .. 44, and back
__host__ __device__ __forceinline__ void ess_ata_pair(int e, int& a, int& b) {
    a = 0;
    while (e >= 9 - a) { e -= 9 - a; ++a; }
    b = a + e;
}

// D24 item b, first half, on the host: the column of V of rank 8 of hestenes() on M = A^T A (row-major, both triangles).  G, V: 81 doubles
// of scratch each.  Returns the sweeps that rotated.
__host__ __device__ __forceinline__ int ess_null_vector(const double* M, double* G, double* V, double* null9) {
    for (int j = 0; j < 9; ++j)
        for (int i = 0; i < 9; ++i) G[9 * j + i] = M[9 * i + j];
    set_identity(V, 9);
    const int sweeps = hestenes(G, V, 9, 9);
    double key[9];
    for (int j = 0; j < 9; ++j) {
        double n2 = 0.0;
        for (int i = 0; i < 9; ++i) n2 = n2 + G[9 * j + i] * G[9 * j + i];
        key[j] = jacobi_key(n2);
    }
    for (int j = 0; j < 9; ++j) {
        int rank = 0;
        for (int k = 0; k < 9; ++k) rank += jacobi_before(key[k], k, key[j], j) ? 1 : 0;
        if (rank == 8)
            for (int i = 0; i < 9; ++i) null9[i] = V[9 * j + i];
    }
    return sweeps;
}

// D24 items b (second half) and c: the sign rule on the null vector (the component of largest magnitude is made non-negative, the first of
// equals), the 3 x 3 matrix it fills row by row (:141), hestenes() on that as a general matrix, and E_21 = g_r0 v_r0^T + g_r1 v_r1^T over the
// columns of rank 0 and 1: U diag(lambda_0, lambda_1, 0) V^T (:149-151) without a division.  G, V: 9 doubles of scratch each, key: 3.
__host__ __device__ __forceinline__ int ess_from_null(double* null9, double* G, double* V, double* key, double* E) {
    int big = 0;
    for (int i = 1; i < 9; ++i)
        if (__builtin_fabs(null9[i]) > __builtin_fabs(null9[big])) big = i;
    if (null9[big] < 0)
        for (int i = 0; i < 9; ++i) null9[i] = -null9[i];
    for (int j = 0; j < 3; ++j)
        for (int i = 0; i < 3; ++i) G[3 * j + i] = null9[3 * i + j];
    set_identity(V, 3);
    const int sweeps = hestenes(G, V, 3, 3);
    for (int j = 0; j < 3; ++j) {
        double n2 = 0.0;
        for (int i = 0; i < 3; ++i) n2 = n2 + G[3 * j + i] * G[3 * j + i];
        key[j] = jacobi_key(n2);
    }
    int r0 = 0, r1 = 0;
    for (int j = 0; j < 3; ++j) {
        int rank = 0;
        for (int k = 0; k < 3; ++k) rank += jacobi_before(key[k], k, key[j], j) ? 1 : 0;
        if (rank == 0) r0 = j;
        if (rank == 1) r1 = j;
    }
    for (int i = 0; i < 3; ++i)
        for (int k = 0; k < 3; ++k) E[3 * i + k] = G[3 * r0 + i] * V[3 * r0 + k] + G[3 * r1 + i] * V[3 * r1 + k];
    return sweeps;
}

// compute_E_21 (:121-154) for nc bearing pairs held `stride` apart, one after the other.  M: 81, G, V: 81 each, null9: 9, key: 3.
__host__ __device__ __forceinline__ void ess_fit(const double* pairs, int stride, int nc, double* M, double* G, double* V, double* null9, double* key, double* E,
                                                 int* sweeps) {
    for (int a = 0; a < 9; ++a)
        for (int b = a; b < 9; ++b) M[9 * a + b] = M[9 * b + a] = ess_ata_chain(pairs, stride, nc, a, b);
    const int s0 = ess_null_vector(M, G, V, null9);
    const int s1 = ess_from_null(null9, G, V, key, E);
    if (sweeps) { sweeps[0] = s0; sweeps[1] = s1; }
}

// The loop body of check_inliers (:211-249) for one match: the two float residuals, and what the match does to the score and the flag.
// Bit 0: residual_in_2 is added to the score (:221-230); bit 1: residual_in_1 is added too and the match is an inlier (:240-249).  A NaN
// residual passes its comparison, as the reference's does.
__host__ __device__ __forceinline__ int ess_residuals(const double* E, const double* b1, const double* b2, float& res_in_2, float& res_in_1) {
    const double p0 = (E[0] * b1[0] + E[1] * b1[1]) + E[2] * b1[2];   // epiplane_in_2 = E_21 * bearing_1 (:217)
    const double p1 = (E[3] * b1[0] + E[4] * b1[1]) + E[5] * b1[2];
    const double p2 = (E[6] * b1[0] + E[7] * b1[1]) + E[8] * b1[2];
    res_in_2 = (float)__builtin_fabs(((p0 * b2[0] + p1 * b2[1]) + p2 * b2[2]) / __builtin_sqrt((p0 * p0 + p1 * p1) + p2 * p2));
    const double q0 = (E[0] * b2[0] + E[3] * b2[1]) + E[6] * b2[2];   // epiplane_in_1 = E_12 * bearing_2 (:235)
    const double q1 = (E[1] * b2[0] + E[4] * b2[1]) + E[7] * b2[2];
    const double q2 = (E[2] * b2[0] + E[5] * b2[1]) + E[8] * b2[2];
    res_in_1 = (float)__builtin_fabs(((q0 * b1[0] + q1 * b1[1]) + q2 * b1[2]) / __builtin_sqrt((q0 * q0 + q1 * q1) + q2 * q2));
    if (kEssResidualCosThr < res_in_2) return 0;
    if (kEssResidualCosThr < res_in_1) return 1;
    return 3;
}
__host__ __device__ __forceinline__ float ess_score_add(float score, int code, float res_in_2, float res_in_1) {
    if (code & 1) score += res_in_2;
    if (code & 2) score += res_in_1;
    return score;
}

struct EssArgs {
    int P, n_cap, m_cap, iters, recompute;
    unsigned long long seed;
    const double* bearing_1; const double* bearing_2; const int32_t* match; const int32_t* counts_1; const int32_t* counts_2; const int32_t* samples;
    uint8_t* out_status; int32_t* out_num_matches; double* out_E_21; float* out_score; int32_t* out_num_inliers; int32_t* out_best_iter;
    uint8_t* out_inliers; float* out_hyp_score;
    int32_t* ctx;            // DEVICE, P x kEssCtxInts
    uint16_t* ctx_slot;      // DEVICE, P x n_cap: slot of match k
    double* ctx_hyp;         // DEVICE, P x kEssHypDoubles x iters
    double* ctx_pairs;       // DEVICE, P x n_cap x kEssPairDoubles: the bearing pairs of the refit
    double* ctx_E;           // DEVICE, P x 9: the refit's matrix
    unsigned long long* ctx_key;   // DEVICE, P: the best hypothesis, score bits << 32 | ~iter, 0 = none
    uint8_t* ctx_code;       // DEVICE, P x n_cap: ess_residuals' code of match k under the matrix that is returned
};
hipError_t launch_essential_ransac(hipStream_t st, const EssArgs& A);   // essential_kernels.hip: five launches, the first error

// whether slot `slot` < counts_1[p] of problem p holds a match: an index in frame 2 below counts_2[p] (D24 item e)
__host__ __device__ __forceinline__ bool ess_matched(const EssArgs& A, int p, int slot, int count_2) {
    const int m = A.match[(size_t)p * A.n_cap + slot];
    return m >= 0 && m < count_2;
}

}  // namespace plp
