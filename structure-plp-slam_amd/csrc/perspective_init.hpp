// initialize::perspective's two solvers (initialize/perspective.cc:84-120): solve::homography_solver (solve/homography_solver.cc:60-155, :388-402,
// :405-436, :556-631), solve::fundamental_solver (solve/fundamental_solver.cc:50-144, :299-332, :349-426) and solve::normalize (solve/common.cc:31-76),
// one definition of the arithmetic for host and device (plp_perspective_ransac_* / plp_model_perspective_ransac_host and the plp_model_* pieces,
// include/plp_front.h).  f64 where the reference holds Mat33_t / Vec3_t, float where it holds float / cv::Point2f, IEEE
// + - * / only, every sum left to right; translation units that include this file are compiled with -ffp-contract=off.  The Eigen::JacobiSVD uses are
// the one-sided Jacobi of jacobi.hpp (D14) through essential.hpp's ess_null_vector and ess_from_null; the samples are ransac.hpp's at K = 8.
//
// As in essential.hpp everything works on memory the caller names (LDS or a context buffer on the device, the stack on the host), and the sums over
// point pairs are `chain` functions of one accumulator each.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/plp_front.h"
#include "essential.hpp"
#include "two_view.hpp"

namespace plp {

constexpr int kPerspMaxSlots = kEssMaxSlots;          // n_cap limit of the entries (a rank fits 16 bits)
constexpr int kPerspMaxIters = kEssMaxIters;
constexpr int kPerspMinSet = 8;                       // min_set_size of both solvers (homography_solver.cc:77, fundamental_solver.cc:67)
constexpr int kPerspH = 0, kPerspF = 1;               // the solver of a hypothesis, a key, a score
constexpr int kPerspCtxInts = 8;                      // per problem: num_matches, (free), then per solver: the final score bits, num_inliers, whether a second check ran
constexpr int kPerspHypDoubles = 19;                  // per hypothesis: the matrix (9, row-major), for H its inverse (9), whether it exists
constexpr int kPerspPairDoubles = 4;                  // per point pair of a fit: the normalised key point of frame 1 (x, y), of frame 2 (x, y)
constexpr int kPerspNormFloats = 8;                   // per problem: mean_x, mean_y, 1 / dev_x, 1 / dev_y of frame 1, of frame 2
constexpr int kPerspTDoubles = 27;                    // per problem: transform_1, transform_2.inverse(), transform_2.transpose()
constexpr int kPerspStreamOfF = 65536;                // the F hypotheses of problem p draw from ransac.hpp's streams of problem p + 65536 (D27 item f)
constexpr float kPerspChiSq2 = 5.991f;                // chi_sq_thr of H, score_thr of F
constexpr float kPerspChiSq1 = 3.841f;                // chi_sq_thr of F

// a float quotient: the f64 quotient of two floats narrowed once is the correctly rounded float quotient
__host__ __device__ __forceinline__ float persp_fdiv(float a, float b) { return (float)((double)a / (double)b); }

// D27 item g: a NaN that is written to an output is the canonical quiet NaN (sign 0, payload 0), whatever the operation that made it left
__host__ __device__ __forceinline__ float persp_out(float v) { return v == v ? v : __builtin_nanf(""); }
__host__ __device__ __forceinline__ double persp_out(double v) { return v == v ? v : __builtin_nan(""); }

// ---- solve::normalize (common.cc:31-76), D27 item a.  The four sums are chains over ALL key points of the frame in their order; n: their number.
__host__ __device__ __forceinline__ float persp_dev_term(float v, float mean) { return __builtin_fabsf(v - mean); }                     // :52-56
__host__ __device__ __forceinline__ float persp_mean(float sum, int n) { return persp_fdiv(sum, (float)n); }                            // :44, :59: 0 / 0 for an empty frame
__host__ __device__ __forceinline__ float persp_inv_dev(float dev) { return persp_fdiv(1.0f, dev); }                                    // :62: +inf for a zero deviation
__host__ __device__ __forceinline__ float persp_normalized(float v, float mean, float inv) { return (v - mean) * inv; }                 // :52, :67
// transform (:71-75), row-major; nrm: mean_x, mean_y, inv_x, inv_y
__host__ __device__ __forceinline__ void persp_transform(const float* nrm, double* T) {
    T[0] = (double)nrm[2]; T[1] = 0.0; T[2] = (double)(-nrm[0] * nrm[2]);
    T[3] = 0.0; T[4] = (double)nrm[3]; T[5] = (double)(-nrm[1] * nrm[3]);
    T[6] = 0.0; T[7] = 0.0; T[8] = 1.0;
}

// ---- 3 x 3 helpers, row-major
__host__ __device__ __forceinline__ void persp_mul3(const double* A, const double* B, double* C) {
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) C[3 * i + j] = (A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j]) + A[3 * i + 2] * B[6 + j];
}
__host__ __device__ __forceinline__ void persp_transpose3(const double* A, double* At) {
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) At[3 * i + j] = A[3 * j + i];
}
// D27 item c: the one inverse (transform_2.inverse(), homography_solver.cc:72; H_21.inverse(), :565): every cofactor divided by the determinant
// expanded along the first row.  A zero determinant gives entries that are +-inf or NaN, nothing is tested.
__host__ __device__ __forceinline__ void persp_inv3(const double* a, double* o) {
    const double c00 = a[4] * a[8] - a[5] * a[7], c01 = a[3] * a[8] - a[5] * a[6], c02 = a[3] * a[7] - a[4] * a[6];
    const double det = (a[0] * c00 - a[1] * c01) + a[2] * c02;
    o[0] = c00 / det;
    o[1] = (a[2] * a[7] - a[1] * a[8]) / det;
    o[2] = (a[1] * a[5] - a[2] * a[4]) / det;
    o[3] = (a[5] * a[6] - a[3] * a[8]) / det;
    o[4] = (a[0] * a[8] - a[2] * a[6]) / det;
    o[5] = (a[2] * a[3] - a[0] * a[5]) / det;
    o[6] = c02 / det;
    o[7] = (a[1] * a[6] - a[0] * a[7]) / det;
    o[8] = (a[0] * a[4] - a[1] * a[3]) / det;
}

// ---- the coefficient rows.  A pair is 4 doubles: the normalised (u1, v1) and (u2, v2), floats widened.
// to_homogeneous(keypt_1)(c)
__host__ __device__ __forceinline__ double persp_hom(const double* q, int c) { return c == 0 ? q[0] : c == 1 ? q[1] : 1.0; }
// entry `col` of row 2 i + par of compute_H_21's A (homography_solver.cc:418-423)
__host__ __device__ __forceinline__ double hom_a(const double* q, int par, int col) {
    const int g = col / 3;
    const double h = persp_hom(q, col - 3 * g);
    if (par == 0) return g == 0 ? 0.0 : g == 1 ? -h : q[3] * h;
    return g == 0 ? h : g == 1 ? 0.0 : (-q[2]) * h;
}
// entry `col` of row i of compute_F_21's A (fundamental_solver.cc:310-312)
__host__ __device__ __forceinline__ double fund_a(const double* q, int col) {
    const int g = col / 3;
    const double h = persp_hom(q, col - 3 * g);
    return g == 0 ? q[2] * h : g == 1 ? q[3] * h : h;
}
// entry (a, b) of A^T A over nc pairs held `stride` doubles apart, the rows in their order (H: two per pair)
__host__ __device__ __forceinline__ double persp_ata_chain(const double* pairs, int stride, int nc, int solver, int a, int b) {
    double acc = 0.0;
    for (int i = 0; i < nc; ++i) {
        const double* q = pairs + (size_t)i * stride;
        if (solver == kPerspH) {
            acc = acc + hom_a(q, 0, a) * hom_a(q, 0, b);
            acc = acc + hom_a(q, 1, a) * hom_a(q, 1, b);
        } else {
            acc = acc + fund_a(q, a) * fund_a(q, b);
        }
    }
    return acc;
}

// D24's sign rule on a null vector: the component of largest magnitude is made non-negative, the first of equals
__host__ __device__ __forceinline__ void persp_sign_rule(double* null9) {
    int big = 0;
    for (int i = 1; i < 9; ++i)
        if (__builtin_fabs(null9[i]) > __builtin_fabs(null9[big])) big = i;
    if (null9[big] < 0)
        for (int i = 0; i < 9; ++i) null9[i] = -null9[i];
}

// From the null vector to the matrix a hypothesis is checked with, D27 items b to d.  T: the problem's kPerspTDoubles.  g3, v3, tmp: 9 doubles of
// scratch each, key3: 3.  out: 18 doubles -- H: H_21 = (T2^-1 * Hn) * T1 (:116) and H_12 = H_21.inverse() (:565); F: F_21 = (T2^T * Fn) * T1 (:105), the
// second nine unused.
__host__ __device__ __forceinline__ void persp_from_null(int solver, double* null9, const double* T, double* g3, double* v3, double* key3, double* tmp, double* out) {
    if (solver == kPerspH) {
        persp_sign_rule(null9);                                     // Hn fills its rows from the vector (:433)
        persp_mul3(T + 9, null9, tmp);
        persp_mul3(tmp, T, out);
        persp_inv3(out, out + 9);
    } else {
        ess_from_null(null9, g3, v3, key3, tmp);                    // the sign rule, then U diag(l0, l1, 0) V^T (:319-329)
        persp_mul3(T + 18, tmp, g3);
        persp_mul3(g3, T, out);
        for (int i = 0; i < 9; ++i) out[9 + i] = 0.0;
    }
}

struct PerspScratch { double M[81], G[81], V[81], null9[9], g3[9], v3[9], key3[3], tmp[9]; };
// compute_H_21 / compute_F_21 and the de-normalisation for nc pairs, one after the other (the host's order of the kernels' steps)
__host__ __device__ __forceinline__ void persp_fit(int solver, const double* pairs, int nc, const double* T, PerspScratch& S, double* out, int* sweeps) {
    for (int a = 0; a < 9; ++a)
        for (int b = a; b < 9; ++b) S.M[9 * a + b] = S.M[9 * b + a] = persp_ata_chain(pairs, kPerspPairDoubles, nc, solver, a, b);
    const int s0 = ess_null_vector(S.M, S.G, S.V, S.null9);
    if (sweeps) *sweeps = s0;
    persp_from_null(solver, S.null9, T, S.g3, S.v3, S.key3, S.tmp, out);
}

// ---- the loop bodies of the two check_inliers for one match (sigma = 1: inv_sigma_sq is 1.0f and its products are left out).  chi_a: the side tested
// first, chi_b: the second.  Code bit 0: score_thr - chi_a is added; bit 1: score_thr - chi_b too and the match is an inlier.  A NaN passes.
// homography_solver.cc:571-628.  M: H_21 (9), H_12 (9).
__host__ __device__ __forceinline__ int hom_residuals(const double* M, float x1, float y1, float x2, float y2, float& chi_a, float& chi_b) {
    const double u1 = (double)x1, v1 = (double)y1, u2 = (double)x2, v2 = (double)y2;
    {
        const double t0 = (M[0] * u1 + M[1] * v1) + M[2], t1 = (M[3] * u1 + M[4] * v1) + M[5], t2 = (M[6] * u1 + M[7] * v1) + M[8];
        const double dx = u2 - t0 / t2, dy = v2 - t1 / t2, dz = 1.0 - t2 / t2;
        chi_a = (float)((dx * dx + dy * dy) + dz * dz);
    }
    {
        const double* N = M + 9;
        const double t0 = (N[0] * u2 + N[1] * v2) + N[2], t1 = (N[3] * u2 + N[4] * v2) + N[5], t2 = (N[6] * u2 + N[7] * v2) + N[8];
        const double dx = u1 - t0 / t2, dy = v1 - t1 / t2, dz = 1.0 - t2 / t2;
        chi_b = (float)((dx * dx + dy * dy) + dz * dz);
    }
    if (kPerspChiSq2 < chi_a) return 0;
    if (kPerspChiSq2 < chi_b) return 1;
    return 3;
}
// fundamental_solver.cc:366-423.  M: F_21 (9).
__host__ __device__ __forceinline__ int fund_residuals(const double* M, float x1, float y1, float x2, float y2, float& chi_a, float& chi_b) {
    const double u1 = (double)x1, v1 = (double)y1, u2 = (double)x2, v2 = (double)y2;
    {
        const double l0 = (M[0] * u1 + M[1] * v1) + M[2], l1 = (M[3] * u1 + M[4] * v1) + M[5], l2 = (M[6] * u1 + M[7] * v1) + M[8];
        const float r = (float)((l0 * u2 + l1 * v2) + l2);
        chi_a = (float)((double)(r * r) / (l0 * l0 + l1 * l1));
    }
    {
        const double l0 = (M[0] * u2 + M[3] * v2) + M[6], l1 = (M[1] * u2 + M[4] * v2) + M[7], l2 = (M[2] * u2 + M[5] * v2) + M[8];
        const float r = (float)((l0 * u1 + l1 * v1) + l2);
        chi_b = (float)((double)(r * r) / (l0 * l0 + l1 * l1));
    }
    if (kPerspChiSq1 < chi_a) return 0;
    if (kPerspChiSq1 < chi_b) return 1;
    return 3;
}
__host__ __device__ __forceinline__ int persp_residuals(int solver, const double* M, float x1, float y1, float x2, float y2, float& chi_a, float& chi_b) {
    return solver == kPerspH ? hom_residuals(M, x1, y1, x2, y2, chi_a, chi_b) : fund_residuals(M, x1, y1, x2, y2, chi_a, chi_b);
}
__host__ __device__ __forceinline__ float persp_score_add(float score, int code, float chi_a, float chi_b) {
    if (code & 1) score += kPerspChiSq2 - chi_a;
    if (code & 2) score += kPerspChiSq2 - chi_b;
    return score;
}

// ---- the choice (perspective.cc:99-120).  0 none, 1 H, 2 F.
__host__ __device__ __forceinline__ int persp_choice(float score_h, float score_f, bool valid_h, bool valid_f, float& rel_score_h) {
    rel_score_h = persp_fdiv(score_h, score_h + score_f);            // 0 / 0 = NaN, which is not above 0.40
    if (0.40 < (double)rel_score_h && valid_h) return PLP_PERSPECTIVE_CHOICE_H;
    if (valid_f) return PLP_PERSPECTIVE_CHOICE_F;
    return PLP_PERSPECTIVE_CHOICE_NONE;
}

struct PerspArgs {
    int P, n_cap, m_cap, iters, recompute;
    unsigned long long seed;
    const plp_keypoint* undist_1; const plp_keypoint* undist_2; const int32_t* match; const int32_t* counts_1; const int32_t* counts_2;
    const int32_t* samples_h; const int32_t* samples_f; const double* given_H_21; const int32_t* given_H_num_inliers;
    uint8_t* out_status_h; uint8_t* out_status_f; int32_t* out_num_matches; double* out_H_21; double* out_F_21; float* out_score_h; float* out_score_f;
    int32_t* out_best_iter_h; int32_t* out_best_iter_f; int32_t* out_num_inliers_h; int32_t* out_num_inliers_f; float* out_rel_score_h; uint8_t* out_choice;
    uint8_t* out_inliers; uint8_t* out_inliers_h; uint8_t* out_inliers_f; float* out_hyp_score_h; float* out_hyp_score_f;
    int32_t* ctx;            // DEVICE, P x kPerspCtxInts
    float* ctx_norm;         // DEVICE, P x kPerspNormFloats
    double* ctx_T;           // DEVICE, P x kPerspTDoubles
    uint16_t* ctx_slot;      // DEVICE, P x n_cap: slot of match k
    double* ctx_hyp;         // DEVICE, P x 2 x kPerspHypDoubles x iters
    double* ctx_pairs;       // DEVICE, P x 2 x n_cap x kPerspPairDoubles: the normalised point pairs of the refits
    double* ctx_M;           // DEVICE, P x 2 x 18: the matrix that is returned where it is no hypothesis (the refit's, the given one)
    unsigned long long* ctx_key;   // DEVICE, P x 2: the best hypothesis, score bits << 32 | ~iter, 0 = none
    uint8_t* ctx_code;       // DEVICE, P x 2 x n_cap: the code of match k under the matrix that is returned
};
hipError_t launch_perspective_ransac(hipStream_t st, const PerspArgs& A);   // perspective_init_kernels.hip: five launches, the first error

// whether slot `slot` < counts_1[p] of problem p holds a match: an index in frame 2 below counts_2[p]
__host__ __device__ __forceinline__ bool persp_matched(const PerspArgs& A, int p, int slot, int count_2) {
    const int m = A.match[(size_t)p * A.n_cap + slot];
    return m >= 0 && m < count_2;
}
// whether problem p takes its homography from the caller (the graph-cut path, homography_solver.cc:388-402)
__host__ __device__ __forceinline__ bool persp_given(const PerspArgs& A, int p) { return A.given_H_21 && A.given_H_num_inliers && A.given_H_num_inliers[p] >= 0; }
// the samples of hypothesis `it` of a solver: the caller's, or ransac.hpp's draw from the solver's stream
__host__ __device__ __forceinline__ bool persp_sample(const PerspArgs& A, int solver, int p, int it, int n, int idx[8]) {
    const int32_t* s = solver == kPerspH ? A.samples_h : A.samples_f;
    struct { const int32_t* samples; int iters; unsigned long long seed; } v = {s ? s + (size_t)p * A.iters * 8 : nullptr, A.iters, A.seed};
    return ransac_sample<kPerspMinSet>(v, s ? 0 : p + solver * kPerspStreamOfF, it, n, idx);
}

// ---------------------------------------------------------------------------------------------------------------- from the matrix to the pose
// initialize::perspective::reconstruct_with_H / reconstruct_with_F (perspective.cc:123-174): homography_solver::decompose
// (homography_solver.cc:438-554), fundamental_solver::decompose (fundamental_solver.cc:334-340) and find_most_plausible_pose(..., true) over the
// eight or four hypotheses, with two_view.hpp's tv_check (plp_perspective_pose_*; D27 items e and h).
constexpr int kPerspMaxHyp = 8;

struct PerspPoseArgs {
    TvArgs tv;               // the camera, the bounds, the thresholds and the tables tv_check<MODEL> reads; depth_is_positive is 1; E_21 and in_status unused
    const uint8_t* in_choice; const double* H_21; const double* F_21;
    double* ctx_pts;         // DEVICE, P x 8 x n_cap x 3: the points of the hypotheses
    uint8_t* ctx_flag;       // DEVICE, P x 8 x n_cap: their flags
};
hipError_t launch_perspective_pose(hipStream_t st, const PerspPoseArgs& A);   // perspective_pose_kernels.hip: one launch, the first error

// scratch of hom_decompose and fund_decompose
struct PerspPoseWs { double K[9], Kinv[9], T[9], A[9], G[9], V[9], key[3], sg[3], U[9], W[9], SU[9], RA[9], aux[9], tv[kTvDecomposeDoubles], rots[18], trans[3]; };

__host__ __device__ __forceinline__ void persp_cam_matrix(const TvArgs& A, double* K) {   // get_camera_matrix (perspective.cc:176-199): eigen_cam_matrix_
    K[0] = A.fx; K[1] = 0.0; K[2] = A.cx; K[3] = 0.0; K[4] = A.fy; K[5] = A.cy; K[6] = 0.0; K[7] = 0.0; K[8] = 1.0;
}
__host__ __device__ __forceinline__ float persp_fsqrt(float v) { return (float)__builtin_sqrt((double)v); }   // the correctly rounded float root
__host__ __device__ __forceinline__ double persp_det3(const double* R) {
    return R[0] * R[4] * R[8] + R[1] * R[5] * R[6] + R[2] * R[3] * R[7] - R[2] * R[4] * R[6] - R[1] * R[3] * R[8] - R[0] * R[5] * R[7];
}

// D27 item e: homography_solver::decompose.  poses: 8 x 12 (rot row-major, trans) in the reference's order.  false: the rank test of :462.
// The SVD of A = K^-1 H K is hestenes() on A as a general matrix; the pairs (u_a, v_a) come in the order of descending singular value, each with the
// sign that makes the component of largest magnitude of v_a non-negative (the first of equals); a singular value that is 0 or not finite leaves no
// u_a: the first two are then zero vectors, the third is u_0 x u_1.
__host__ __device__ __forceinline__ bool hom_decompose(const double* H, PerspPoseWs& w, double* poses) {
    persp_inv3(w.K, w.Kinv);
    persp_mul3(w.Kinv, H, w.T);
    persp_mul3(w.T, w.K, w.A);                                      // :448
    for (int j = 0; j < 3; ++j)
        for (int i = 0; i < 3; ++i) w.G[3 * j + i] = w.A[3 * i + j];
    set_identity(w.V, 3);
    hestenes(w.G, w.V, 3, 3);
    for (int j = 0; j < 3; ++j) {
        double n2 = 0.0;
        for (int i = 0; i < 3; ++i) n2 = n2 + w.G[3 * j + i] * w.G[3 * j + i];
        w.key[j] = jacobi_key(n2);
    }
    for (int j = 0; j < 3; ++j) {
        int rank = 0;
        for (int k = 0; k < 3; ++k) rank += jacobi_before(w.key[k], k, w.key[j], j) ? 1 : 0;
        const double sg = __builtin_sqrt(w.key[j]);
        const bool have = sg > 0.0 && sg < __builtin_inf();
        w.sg[rank] = sg;
        for (int i = 0; i < 3; ++i) { w.U[3 * rank + i] = have ? w.G[3 * j + i] / sg : 0.0; w.W[3 * rank + i] = w.V[3 * j + i]; }
    }
    for (int a = 0; a < 3; ++a) {
        if (a == 2 && !(w.sg[2] > 0.0 && w.sg[2] < __builtin_inf()))
            for (int i = 0; i < 3; ++i) {
                const int i1 = (i + 1) % 3, i2 = (i + 2) % 3;
                w.U[6 + i] = w.U[i1] * w.U[3 + i2] - w.U[i2] * w.U[3 + i1];
            }
        int big = 0;
        for (int i = 1; i < 3; ++i)
            if (__builtin_fabs(w.W[3 * a + i]) > __builtin_fabs(w.W[3 * a + big])) big = i;
        if (w.W[3 * a + big] < 0)
            for (int i = 0; i < 3; ++i) { w.U[3 * a + i] = -w.U[3 * a + i]; w.W[3 * a + i] = -w.W[3 * a + i]; }
    }
    const float d1 = (float)w.sg[0], d2 = (float)w.sg[1], d3 = (float)w.sg[2];               // :457-459
    if ((double)persp_fdiv(d1, d2) < 1.0001 || (double)persp_fdiv(d2, d3) < 1.0001) return false;   // :462
    const float s = (float)(persp_det3(w.U) * persp_det3(w.W));                              // :468; w.U holds U^T, w.W holds V^T
    const float p12 = d1 * d1 - d2 * d2, p23 = d2 * d2 - d3 * d3, p13 = d1 * d1 - d3 * d3;
    const float aux_1 = persp_fsqrt(persp_fdiv(p12, p13)), aux_3 = persp_fsqrt(persp_fdiv(p23, p13));   // :471-472
    const float root = persp_fsqrt(p12 * p23);
    const float sin_theta = persp_fdiv(root, (d1 + d3) * d2), cos_theta = persp_fdiv(d2 * d2 + d1 * d3, (d1 + d3) * d2);   // :479-480
    const float sin_phi = persp_fdiv(root, (d1 - d3) * d2), cos_phi = persp_fdiv(d1 * d3 - d2 * d2, (d1 - d3) * d2);       // :516-517
    for (int i = 0; i < 3; ++i)
        for (int a = 0; a < 3; ++a) w.SU[3 * i + a] = (double)s * w.U[3 * a + i];            // s * U
    for (int h = 0; h < 8; ++h) {
        const int i = h & 3;
        const float x1 = i < 2 ? aux_1 : -aux_1, x3 = (i & 1) ? -aux_3 : aux_3;               // :473-474
        const bool plus = i == 0 || i == 3;                                                  // :481, :518: {+, -, -, +}
        for (int e = 0; e < 9; ++e) w.aux[e] = 0.0;
        double at0, at2;
        if (h < 4) {                                                                         // d' > 0, :483-511
            const float sn = plus ? sin_theta : -sin_theta;
            w.aux[0] = (double)cos_theta; w.aux[2] = (double)(-sn); w.aux[4] = 1.0; w.aux[6] = (double)sn; w.aux[8] = (double)cos_theta;
            at0 = (double)x1 * (double)(d1 - d3); at2 = (double)(-x3) * (double)(d1 - d3);
        } else {                                                                             // d' < 0, :520-551
            const float sn = plus ? sin_phi : -sin_phi;
            w.aux[0] = (double)cos_phi; w.aux[2] = (double)sn; w.aux[4] = -1.0; w.aux[6] = (double)sn; w.aux[8] = (double)(-cos_phi);
            at0 = (double)x1 * (double)(d1 + d3); at2 = (double)x3 * (double)(d1 + d3);
        }
        const double at1 = 0.0 * (double)(h < 4 ? d1 - d3 : d1 + d3);
        persp_mul3(w.SU, w.aux, w.RA);
        double* pose = poses + 12 * h;
        persp_mul3(w.RA, w.W, pose);                                                         // ... * Vt (:492, :530)
        double t[3];
        for (int r = 0; r < 3; ++r) t[r] = (w.U[r] * at0 + w.U[3 + r] * at1) + w.U[6 + r] * at2;   // U * aux_trans (:499, :540)
        const double nrm = __builtin_sqrt((t[0] * t[0] + t[1] * t[1]) + t[2] * t[2]);
        for (int r = 0; r < 3; ++r) pose[9 + r] = t[r] / nrm;
    }
    return true;
}
// fundamental_solver::decompose: E_21 = (K^T * F_21) * K (:337), then D24 item c's decompose: four poses
__host__ __device__ __forceinline__ void fund_decompose(const double* F, PerspPoseWs& w, double* poses) {
    persp_transpose3(w.K, w.Kinv);
    persp_mul3(w.Kinv, F, w.T);
    persp_mul3(w.T, w.K, w.A);
    tv_decompose(w.A, w.tv, w.rots, w.trans);
    for (int h = 0; h < 4; ++h) tv_hypothesis(w.rots, w.trans, h, poses + 12 * h);
}
// tv_select (two_view.hpp) over nh hypotheses (base.cc:83-120).  A copy and not a defaulted parameter of tv_select: k_two_view_pose is held instruction for
// instruction to what it was, and its loops over four hypotheses stay literal there.  A change to one of the two belongs in the other as well.
__host__ __device__ __forceinline__ int persp_select(const int* num_valid, const float* parallax_deg, int nh, int min_num_triangulated, float parallax_deg_thr, int& chosen) {
    int best = 0;
    for (int h = 1; h < nh; ++h)
        if (num_valid[h] > num_valid[best]) best = h;               // std::max_element: the first of equal maxima
    chosen = -1;
    if (num_valid[best] < min_num_triangulated) return PLP_TWO_VIEW_TOO_FEW_TRIANGULATED;
    int similars = 0;
    for (int h = 0; h < nh; ++h) similars += 0.8 * (double)(unsigned)num_valid[best] < (double)(unsigned)num_valid[h] ? 1 : 0;
    if (1 < similars) return PLP_TWO_VIEW_AMBIGUOUS;
    if (parallax_deg[best] < parallax_deg_thr) return PLP_TWO_VIEW_SMALL_PARALLAX;
    chosen = best;
    return PLP_TWO_VIEW_OK;
}

}  // namespace plp
