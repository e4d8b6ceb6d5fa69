// The second half of initialize::bearing_vector::initialize, one definition of the arithmetic for host and device (plp_two_view_pose_* /
// plp_model_two_view_pose_host, plp_model_essential_decompose_host, plp_model_check_pose_host, include/plp_front.h; DESIGN.md section 5, D24
// items c, f and g): essential_solver::decompose (solve/essential_solver.cc:156-186), the loop body of initialize::base::check_pose
// (initialize/base.cc:146-228) with solve::triangulator::triangulate (solve/triangulator.h:86-103), its order statistic and
// find_most_plausible_pose (:62-121).  f64 with IEEE + - * / sqrt only, every sum left to right, floats where the reference holds floats;
// acos is D22's pose_acos; translation units that include this file are compiled with -ffp-contract=off.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/plp_front.h"
#include "essential.hpp"
#include "jacobi.hpp"
#include "pose_graph.hpp"
#include "ransac.hpp"
#include "reproject.hpp"

namespace plp {

constexpr float kTvCosParallaxThr = 0.99996192306f;   // cos_parallax_thr (base.cc:129)
constexpr int kTvDecomposeDoubles = 39;               // scratch of tv_decompose: G (9), V (9), key (3), U (9), W (9)
constexpr int kTvSortRank = 50;                       // the index of base.cc:234

// what a match does in the loop of check_pose: where it leaves the iteration, or how it ends it
enum {
    kTvNotFinite = 1,      // :158-161
    kTvDepthRef = 2,       // :175-178
    kTvDepthCur = 3,       // :180-183
    kTvInvalidRef = 4,     // :194-197
    kTvErrRef = 5,         // :200-203
    kTvInvalidCur = 6,     // :210-213
    kTvErrCur = 7,         // :215-218
    kTvValidSmall = 8,     // :221-222, the parallax is small: counted, no point (:223)
    kTvValid = 9           // :221-227
};

// the camera fields reproject<MODEL> reads (set_camera, matcher_context.hpp) and what every problem of a call shares
struct TvArgs {
    int model;
    double fx, fy, cx, cy, fxb, cols_d, rows_d;
    float bounds[4];
    int P, n_cap, m_cap, min_num_triangulated, depth_is_positive;
    float parallax_deg_thr, reproj_err_thr;
    const double* E_21; const uint8_t* inliers; const int32_t* match; const int32_t* counts_1; const int32_t* counts_2; const double* bearing_1;
    const double* bearing_2; const plp_keypoint* undist_1; const plp_keypoint* undist_2; const uint8_t* in_status;
    uint8_t* out_status; double* out_rot; double* out_trans; int32_t* out_hypothesis; int32_t* out_num_valid; float* out_parallax_deg;
    double* out_pts; uint8_t* out_is_triangulated; uint8_t* out_hyp_is_triangulated;
    double* ctx_pts;         // DEVICE, P x 4 x n_cap x 3: the points of the four hypotheses
    uint8_t* ctx_flag;       // DEVICE, P x 4 x n_cap: their flags
};
hipError_t launch_two_view_pose(hipStream_t st, const TvArgs& A);   // two_view_kernels.hip: one launch, the first error

// D24 item c: essential_solver::decompose.  rots: rot_1 then rot_2 (9 each, row-major), trans: 3.  ws: kTvDecomposeDoubles of scratch.  The
// four hypotheses are (rot_1, trans), (rot_1, -trans), (rot_2, trans), (rot_2, -trans) (:182-183).
__host__ __device__ __forceinline__ int tv_decompose(const double* E, double* ws, double* rots, double* trans) {
    double* G = ws; double* V = ws + 9; double* key = ws + 18; double* U = ws + 21; double* W = ws + 30;
    for (int j = 0; j < 3; ++j)
        for (int i = 0; i < 3; ++i) G[3 * j + i] = E[3 * i + j];
    set_identity(V, 3);
    const int sweeps = hestenes(G, V, 3, 3);
    for (int j = 0; j < 3; ++j) {
        double n2 = 0.0;
        for (int i = 0; i < 3; ++i) n2 = n2 + G[3 * j + i] * G[3 * j + i];
        key[j] = jacobi_key(n2);
    }
    int r[2] = {0, 0};
    for (int j = 0; j < 3; ++j) {
        int rank = 0;
        for (int k = 0; k < 3; ++k) rank += jacobi_before(key[k], k, key[j], j) ? 1 : 0;
        if (rank == 0) r[0] = j;
        if (rank == 1) r[1] = j;
    }
    for (int a = 0; a < 2; ++a) {                                   // the pairs (u_a, v_a) of rank 0 and 1, and their sign rule
        const int j = a == 0 ? r[0] : r[1];
        const double sg = __builtin_sqrt(key[j]);
        const bool have = sg > 0.0 && sg < __builtin_inf();
        for (int i = 0; i < 3; ++i) { U[3 * a + i] = have ? G[3 * j + i] / sg : 0.0; W[3 * a + i] = V[3 * j + i]; }
        int big = 0;
        for (int i = 1; i < 3; ++i)
            if (__builtin_fabs(W[3 * a + i]) > __builtin_fabs(W[3 * a + big])) big = i;
        if (W[3 * a + big] < 0)
            for (int i = 0; i < 3; ++i) { U[3 * a + i] = -U[3 * a + i]; W[3 * a + i] = -W[3 * a + i]; }
    }
    for (int i = 0; i < 3; ++i) {                                   // u_2 = u_0 x u_1, v_2 = v_0 x v_1
        const int i1 = (i + 1) % 3, i2 = (i + 2) % 3;
        U[6 + i] = U[i1] * U[3 + i2] - U[i2] * U[3 + i1];
        W[6 + i] = W[i1] * W[3 + i2] - W[i2] * W[3 + i1];
    }
    const double nrm = __builtin_sqrt((U[6] * U[6] + U[7] * U[7]) + U[8] * U[8]);   // trans.normalize() (:162-163)
    for (int i = 0; i < 3; ++i) trans[i] = U[6 + i] / nrm;
    for (int i = 0; i < 3; ++i)
        for (int k = 0; k < 3; ++k) {
            rots[3 * i + k] = (U[3 + i] * W[k] + (-U[i]) * W[3 + k]) + U[6 + i] * W[6 + k];         // U * W * V^T (:170)
            rots[9 + 3 * i + k] = ((-U[3 + i]) * W[k] + U[i] * W[3 + k]) + U[6 + i] * W[6 + k];   // U * W^T * V^T (:176)
        }
    for (int a = 0; a < 2; ++a) {
        double* R = rots + 9 * a;
        const double det = R[0] * R[4] * R[8] + R[1] * R[5] * R[6] + R[2] * R[3] * R[7] - R[2] * R[4] * R[6] - R[1] * R[3] * R[8] - R[0] * R[5] * R[7];
        if (det < 0)                                                // :171-174, :177-180
            for (int i = 0; i < 9; ++i) R[i] = R[i] * -1.0;
    }
    return sweeps;
}
// hypothesis h = 0 .. 3 as the 12 doubles reproject<MODEL> takes (rot row-major, trans) from tv_decompose's output
__host__ __device__ __forceinline__ void tv_hypothesis(const double* rots, const double* trans, int h, double* pose12) {
    for (int i = 0; i < 9; ++i) pose12[i] = rots[9 * (h >> 1) + i];
    for (int i = 0; i < 3; ++i) pose12[9 + i] = (h & 1) ? -trans[i] : trans[i];
}
// -rot^T * trans (base.cc:141, triangulator.h:88): each coefficient the left-to-right sum of the negated column times trans
__host__ __device__ __forceinline__ void tv_center(const double* pose12, double* c) {
    for (int i = 0; i < 3; ++i) c[i] = ((-pose12[i]) * pose12[9] + (-pose12[3 + i]) * pose12[10]) + (-pose12[6 + i]) * pose12[11];
}

__host__ __device__ __forceinline__ double tv_dot(const double* a, const double* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }
__host__ __device__ __forceinline__ bool tv_finite(double v) { return v - v == 0.0; }

// The loop body of check_pose (:153-227) for one inlier match.  pose12: (R, t) of the hypothesis; c: tv_center of it (cur_cam_center and
// trans_12 are the same expression).  Returns a kTv* code; pos and cos_parallax are set from kTvDepthRef on.
template <int MODEL>
__host__ __device__ __forceinline__ int tv_check(const TvArgs& A, const double* pose12, const double* c, const double* b1, const double* b2, float x1, float y1,
                                                 float x2, float y2, double* pos, float& cos_parallax) {
    // solve::triangulator::triangulate (triangulator.h:86-103); A.inverse() is the adjugate times 1 / det
    double q[3];
    for (int i = 0; i < 3; ++i) q[i] = (pose12[i] * b2[0] + pose12[3 + i] * b2[1]) + pose12[6 + i] * b2[2];   // rot_21^T * bearing_2
    const double a00 = tv_dot(b1, b1), a10 = tv_dot(b1, q), a01 = -a10, a11 = -tv_dot(q, q);
    const double r0 = tv_dot(b1, c), r1 = tv_dot(q, c);
    const double inv_det = 1.0 / (a00 * a11 - a01 * a10);
    const double i00 = a11 * inv_det, i01 = (-a01) * inv_det, i10 = (-a10) * inv_det, i11 = a00 * inv_det;
    const double l0 = i00 * r0 + i01 * r1, l1 = i10 * r0 + i11 * r1;
    for (int i = 0; i < 3; ++i) pos[i] = (l0 * b1[i] + (l1 * q[i] + c[i])) / 2.0;
    if (!tv_finite(pos[0]) || !tv_finite(pos[1]) || !tv_finite(pos[2])) return kTvNotFinite;
    const double cn[3] = {pos[0] - c[0], pos[1] - c[1], pos[2] - c[2]};
    const float ref_norm = (float)__builtin_sqrt(tv_dot(pos, pos));
    const float cur_norm = (float)__builtin_sqrt(tv_dot(cn, cn));
    cos_parallax = (float)(tv_dot(pos, cn) / (double)(ref_norm * cur_norm));
    const bool small = kTvCosParallaxThr < cos_parallax;
    if (A.depth_is_positive) {
        if (!small && pos[2] <= 0) return kTvDepthRef;
        const double zc = ((pose12[6] * pos[0] + pose12[7] * pos[1]) + pose12[8] * pos[2]) + pose12[11];
        if (!small && zc <= 0) return kTvDepthCur;
    }
    const float thr_sq = A.reproj_err_thr * A.reproj_err_thr;
    const double ident[12] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0};
    const Reproj ra = reproject<MODEL>(A, ident, pos[0], pos[1], pos[2]);
    if (!small && !ra.in) return kTvInvalidRef;
    const double dxa = ra.u - (double)x1, dya = ra.v - (double)y1;   // where the camera wrote nothing the reference's Vec2_t is uninitialised: (0, 0) here
    if (thr_sq < (float)(dxa * dxa + dya * dya)) return kTvErrRef;
    const Reproj rb = reproject<MODEL>(A, pose12, pos[0], pos[1], pos[2]);
    if (!small && !rb.in) return kTvInvalidCur;
    const double dxb = rb.u - (double)x2, dyb = rb.v - (double)y2;
    if (thr_sq < (float)(dxb * dxb + dyb * dyb)) return kTvErrCur;
    return small ? kTvValidSmall : kTvValid;
}

// the order of the float cos_parallaxes as unsigned keys (ascending float = ascending key; a NaN, which std::sort does not define, by its bits)
__host__ __device__ __forceinline__ uint32_t tv_key(float v) {
    uint32_t u;
    __builtin_memcpy(&u, &v, 4);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__host__ __device__ __forceinline__ float tv_unkey(uint32_t k) {
    const uint32_t u = (k & 0x80000000u) ? (k ^ 0x80000000u) : ~k;
    float v;
    __builtin_memcpy(&v, &u, 4);
    return v;
}
// parallax_deg from the order statistic (:230-240); coef: pg_coef_init's table
__host__ __device__ __forceinline__ float tv_parallax_deg(float cos_at_rank, const double* coef) {
    return (float)(pose_acos((double)cos_at_rank, coef) * 180.0 / 3.14159265358979323846);
}

// find_most_plausible_pose behind its four check_pose calls (:83-120): the status and the chosen hypothesis (-1 unless OK)
__host__ __device__ __forceinline__ int tv_select(const int* num_valid, const float* parallax_deg, int min_num_triangulated, float parallax_deg_thr, int& chosen) {
    int best = 0;
    for (int h = 1; h < 4; ++h)
        if (num_valid[h] > num_valid[best]) best = h;               // std::max_element: the first of equal maxima
    chosen = -1;
    if (num_valid[best] < min_num_triangulated) return PLP_TWO_VIEW_TOO_FEW_TRIANGULATED;   // :92
    int similars = 0;
    for (int h = 0; h < 4; ++h) similars += 0.8 * (double)(unsigned)num_valid[best] < (double)(unsigned)num_valid[h] ? 1 : 0;
    if (1 < similars) return PLP_TWO_VIEW_AMBIGUOUS;                 // :103
    if (parallax_deg[best] < parallax_deg_thr) return PLP_TWO_VIEW_SMALL_PARALLAX;   // :109
    chosen = best;
    return PLP_TWO_VIEW_OK;
}

}  // namespace plp
