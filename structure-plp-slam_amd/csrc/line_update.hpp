// The line map update every optimiser of the reference ends with, one definition of the arithmetic for host and device (plp_trim_line_endpoints_*,
// plp_correct_landmark_lines_*, plp_loop_ba_propagate_lines_* and their plp_model_*_host builds, include/plp_front.h):
//   endpoint_trimming           optimize/graph_optimizer.cc:424-532 = module/loop_bundle_adjuster.cc:269- = optimize/global_bundle_adjuster.cc:362-,
//                               and optimize/local_bundle_adjuster_extended_line.cc:676-787 with its own acceptance test
//   the pose graph's line cloud optimize/graph_optimizer.cc:352-403
//   the loop adjuster's         module/loop_bundle_adjuster.cc:184-244
// f64 with IEEE + - * / sqrt only.  Every Eigen expression is written out in index order with all of its terms, the zero blocks of the 6 x 6
// matrices included (D7's rule; translation units that include this file are compiled with -ffp-contract=off), so that a non-finite value reaches
// every sum the reference lets it reach.  One item per line, no state shared between items.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/plp_front.h"
#include "line3d.hpp"
#include "pose_opt.hpp"   // pose_rot_from_quat: Eigen's toRotationMatrix, the formula of the pose rows

namespace plp {

constexpr int kLineUpdateMaxKfPg = 1024;    // plp_correct_landmark_lines_*: the table of plp_pose_graph_optimize_*
constexpr int kLineUpdateMaxKfBa = 4096;    // plp_loop_ba_propagate_lines_*: the table of plp_global_ba_*

// ---- the 6 x 6 line transformation [s R, skew(t) R; 0, R], held as its three non-zero 3 x 3 blocks (row-major): A = s R, B = skew(t) R, R
struct LineT6 { double A[9], B[9], R[9]; };

// scaled: block(0,0) = scale * rot (graph_optimizer.cc:388, :398); else block(0,0) = rot (the rigid transformation_line_cw / _wc)
__host__ __device__ __forceinline__ void line_transform6(const double* R, const double* t, double s, bool scaled, LineT6& T) {
    const double tx = t[0], ty = t[1], tz = t[2];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double r0 = R[c], r1 = R[3 + c], r2 = R[6 + c];
        T.R[c] = r0; T.R[3 + c] = r1; T.R[6 + c] = r2;
        T.A[c] = scaled ? s * r0 : r0; T.A[3 + c] = scaled ? s * r1 : r1; T.A[6 + c] = scaled ? s * r2 : r2;
        // skew(t) * rot, skew = (0, -tz, ty; tz, 0, -tx; -ty, tx, 0), three terms per coefficient
        T.B[c] = (0.0 * r0 + (-tz) * r1) + ty * r2;
        T.B[3 + c] = (tz * r0 + 0.0 * r1) + (-tx) * r2;
        T.B[6 + c] = ((-ty) * r0 + tx * r1) + 0.0 * r2;
    }
}
// coefficient (i, k) of the 6 x 6 matrix; i and k are compile-time values after unrolling, so the zero block costs no register
__host__ __device__ __forceinline__ double line_t6_at(const LineT6& T, int i, int k) {
    return i < 3 ? (k < 3 ? T.A[3 * i + k] : T.B[3 * i + (k - 3)]) : (k < 3 ? 0.0 : T.R[3 * (i - 3) + (k - 3)]);
}
// o = T * v: o(i) = the sum over k = 0 .. 5 of T(i,k) v(k), left to right
__host__ __device__ __forceinline__ void line_t6_apply(const LineT6& T, const double (&v)[6], double (&o)[6]) {
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        double s = line_t6_at(T, i, 0) * v[0];
#pragma unroll
        for (int k = 1; k < 6; ++k) s = s + line_t6_at(T, i, k) * v[k];
        o[i] = s;
    }
}
// o = (X * Y) * v: the product of the two matrices first, C(i,j) = the sum over k of X(i,k) Y(k,j), then o(i) = the sum over j of C(i,j) v(j);
// a row of C lives only until its dot product is taken
__host__ __device__ __forceinline__ void line_t6_product_apply(const LineT6& X, const LineT6& Y, const double (&v)[6], double (&o)[6]) {
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        double s = 0.0;
#pragma unroll
        for (int j = 0; j < 6; ++j) {
            double c = line_t6_at(X, i, 0) * line_t6_at(Y, 0, j);
#pragma unroll
            for (int k = 1; k < 6; ++k) c = c + line_t6_at(X, i, k) * line_t6_at(Y, k, j);
            s = j == 0 ? c * v[0] : s + c * v[j];
        }
        o[i] = s;
    }
}

// ---- endpoint_trimming and what its call sites do with the result
struct LineTrimArgs {
    int L, F, cap, pose_stride, mode;
    double fx, fy, cx, cy, max_change;
    const double* pluecker; const int32_t* ref_kf; const uint8_t* skip; const int32_t* obs_offsets; const int32_t* obs_kf; const int32_t* obs_idx;
    const double* pose; const uint8_t* kf_erased; const plp_keyline* kl; const int32_t* counts; const double* pos_w_old; const float* median;
    double* out_pos_w; uint8_t* out_status; uint8_t* out_erase;
};

// The status of line l; sp / ep = the trimmed end points where the arithmetic was reached (OK and REJECTED).
__host__ __device__ __forceinline__ int trim_to_ref(const LineTrimArgs& A, int l, double (&sp)[3], double (&ep)[3]) {
    if (A.skip && A.skip[l]) return PLP_TRIM_SKIPPED;
    const int r = A.ref_kf[l];
    if ((unsigned)r >= (unsigned)A.F || (A.kf_erased && A.kf_erased[r])) return PLP_TRIM_NO_REF;
    // get_index_in_keyframe(ref_kf): the observation of the reference key frame, the first in list order
    int idx = -1;
    const int beg = A.obs_offsets[l], end = A.obs_offsets[l + 1];
    for (int o = beg; o < end; ++o)
        if (A.obs_kf[o] == r) { idx = A.obs_idx[o]; break; }
    if (idx == -1) return PLP_TRIM_NOT_OBSERVED;
    int cnt = A.cap;
    if (A.counts) { cnt = A.counts[r]; cnt = cnt < 0 ? 0 : cnt > A.cap ? A.cap : cnt; }
    if ((unsigned)idx >= (unsigned)cnt) return PLP_TRIM_INDEX_RANGE;
    const plp_keyline& kl = A.kl[(size_t)r * A.cap + idx];
    const double* P = A.pose + (size_t)r * A.pose_stride;
    double Lw[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) Lw[i] = A.pluecker[(size_t)6 * l + i];
    // [2] reproj_line_function = _K * (transformation_line_cw * plucker_coord).block<3,1>(0,0)
    LineT6 T;
    line_transform6(P, P + 9, 1.0, false, T);
    double v[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        double s = line_t6_at(T, i, 0) * Lw[0];
#pragma unroll
        for (int k = 1; k < 6; ++k) s = s + line_t6_at(T, i, k) * Lw[k];
        v[i] = s;
    }
    const double K[9] = {A.fy, 0.0, 0.0, 0.0, A.fx, 0.0, -A.fy * A.cx, -A.fx * A.cy, A.fx * A.fy};
    const double l1 = (K[0] * v[0] + K[1] * v[1]) + K[2] * v[2];
    const double l2 = (K[3] * v[0] + K[4] * v[1]) + K[5] * v[2];
    const double l3 = (K[6] * v[0] + K[7] * v[1]) + K[8] * v[2];
    const double den = l1 * l1 + l2 * l2;
    // [5] P = eigen_cam_matrix_ * [rot_cw | trans_cw], three terms per coefficient, the zero entries of the camera matrix included
    double Pm[12];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const double a0 = c < 3 ? P[c] : P[9], a1 = c < 3 ? P[3 + c] : P[10], a2 = c < 3 ? P[6 + c] : P[11];
        Pm[c] = (A.fx * a0 + 0.0 * a1) + A.cx * a2;
        Pm[4 + c] = (0.0 * a0 + A.fy * a1) + A.cy * a2;
        Pm[8 + c] = (0.0 * a0 + 0.0 * a1) + 1.0 * a2;
    }
    // [6] the Pluecker matrix: skew(m) | d over -d^T | 0
    const double M[16] = {0.0, -Lw[2], Lw[1], Lw[3],
                          Lw[2], 0.0, -Lw[0], Lw[4],
                          -Lw[1], Lw[0], 0.0, Lw[5],
                          -Lw[3], -Lw[4], -Lw[5], 0.0};
    // [3] [4] [6] per end point; the reference tests no value on the way, a non-finite one reaches the acceptance test
    line3d_trim(Pm, M, l1, l2, l3, den, kl.startPointX, kl.startPointY, sp);
    line3d_trim(Pm, M, l1, l2, l3, den, kl.endPointX, kl.endPointY, ep);
    if (A.mode == PLP_TRIM_MAX_CHANGE) {
        // (updated.head<3>() - old.head<3>()).norm() / compute_median_depth(true) > 0.1, either end point (:773-784)
        const double* old = A.pos_w_old + (size_t)6 * l;
        const double med = (double)A.median[r];
        const double sx = sp[0] - old[0], sy = sp[1] - old[1], sz = sp[2] - old[2];
        const double ex = ep[0] - old[3], ey = ep[1] - old[4], ez = ep[2] - old[5];
        const double ds = __builtin_sqrt((sx * sx + sy * sy) + sz * sz) / med;
        const double de = __builtin_sqrt((ex * ex + ey * ey) + ez * ez) / med;
        return (ds > A.max_change || de > A.max_change) ? PLP_TRIM_REJECTED : PLP_TRIM_OK;
    }
    // pos_c = rotation_translation_combined * (pos_w, 1): the third row, four terms; 0 < pos_c_sp(2) && 0 < pos_c_ep(2)
    const double zs = ((P[6] * sp[0] + P[7] * sp[1]) + P[8] * sp[2]) + P[11] * 1.0;
    const double ze = ((P[6] * ep[0] + P[7] * ep[1]) + P[8] * ep[2]) + P[11] * 1.0;
    return (0.0 < zs && 0.0 < ze) ? PLP_TRIM_OK : PLP_TRIM_REJECTED;
}

__host__ __device__ __forceinline__ void line_trim_item(const LineTrimArgs& A, int l) {
    double sp[3], ep[3];
    const int st = trim_to_ref(A, l, sp, ep);
    A.out_status[l] = (uint8_t)st;
    A.out_erase[l] = (st == PLP_TRIM_NOT_OBSERVED || st == PLP_TRIM_REJECTED) ? 1 : 0;
    if (st != PLP_TRIM_OK) return;
    double* o = A.out_pos_w + (size_t)6 * l;
#pragma unroll
    for (int i = 0; i < 3; ++i) { o[i] = sp[i]; o[3 + i] = ep[i]; }
}

// ---- the pose graph's line cloud
struct LineCorrectArgs {
    int L, F;
    const double* pluecker; const uint8_t* lm_erased; const int32_t* ref_kf; const int32_t* corr_kf; const uint8_t* kf_erased; const double* sim3_cw;
    const double* corrected_wc; double* out_pluecker; uint8_t* out_status;
};
// a Sim3 row {qx, qy, qz, qw, tx, ty, tz, s} as its 6 x 6 matrix
__host__ __device__ __forceinline__ void line_sim3_transform6(const double* sim3, LineT6& T) {
    double q[8], R[9];
#pragma unroll
    for (int i = 0; i < 8; ++i) q[i] = sim3[i];
    pose_rot_from_quat(q, R);
    line_transform6(R, q + 4, q[7], true, T);
}
__host__ __device__ __forceinline__ void line_correct_item(const LineCorrectArgs& A, int l) {
    if (A.lm_erased && A.lm_erased[l]) { A.out_status[l] = PLP_CORRECT_LINE_ERASED; return; }
    const int r = A.ref_kf[l];
    if ((unsigned)r >= (unsigned)A.F || (A.kf_erased && A.kf_erased[r])) { A.out_status[l] = PLP_CORRECT_LINE_NO_REF; return; }
    const int c = A.corr_kf ? A.corr_kf[l] : r;
    if ((unsigned)c >= (unsigned)A.F || (A.kf_erased && A.kf_erased[c])) { A.out_status[l] = PLP_CORRECT_LINE_NO_VERTEX; return; }
    LineT6 X, Y;
    line_sim3_transform6(A.corrected_wc + (size_t)8 * c, X);
    line_sim3_transform6(A.sim3_cw + (size_t)8 * c, Y);
    double v[6], o[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) v[i] = A.pluecker[(size_t)6 * l + i];
    line_t6_product_apply(X, Y, v, o);   // corrected_Sim3_wc_pluecker * Sim3_cw_pluecker * pos_w (:403)
#pragma unroll
    for (int i = 0; i < 6; ++i) A.out_pluecker[(size_t)6 * l + i] = o[i];
    A.out_status[l] = PLP_CORRECT_LINE_OK;
}

// ---- the loop adjuster's line cloud
struct LinePropagateArgs {
    int L, F;
    const double* pose_after; const double* pose_before; const uint8_t* kf_status; const double* pluecker; const uint8_t* lm_erased; const int32_t* ref_kf;
    const uint8_t* line_optimized; const double* pluecker_after; double* out_pluecker; uint8_t* out_status;
};
__host__ __device__ __forceinline__ void line_propagate_item(const LinePropagateArgs& A, int l) {
    if (A.lm_erased && A.lm_erased[l]) { A.out_status[l] = PLP_LOOP_BA_LM_ERASED; return; }
    double* out = A.out_pluecker + (size_t)6 * l;
    if (A.line_optimized && A.line_optimized[l]) {
        double v[6];
#pragma unroll
        for (int i = 0; i < 6; ++i) v[i] = A.pluecker_after[(size_t)6 * l + i];
#pragma unroll
        for (int i = 0; i < 6; ++i) out[i] = v[i];
        A.out_status[l] = PLP_LOOP_BA_LM_OPTIMIZED;
        return;
    }
    const int r = A.ref_kf[l];
    int st = PLP_LOOP_BA_KF_NOT_REACHED;
    if ((unsigned)r < (unsigned)A.F) st = A.kf_status[r];
    if (st != PLP_LOOP_BA_KF_OPTIMIZED && st != PLP_LOOP_BA_KF_PROPAGATED) { A.out_status[l] = PLP_LOOP_BA_LM_NO_REF; return; }
    const double* b = A.pose_before + (size_t)12 * r;
    const double* a = A.pose_after + (size_t)15 * r;
    double v[6], c[6], o[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) v[i] = A.pluecker[(size_t)6 * l + i];
    LineT6 T;
    line_transform6(b, b + 9, 1.0, false, T);
    line_t6_apply(T, v, c);              // pos_c_pluecker = transformation_line_cw * get_PlueckerCoord() (:231)
    // get_cam_pose_inv(): rot_cw transposed, cam_center (entries 12-14 of the row)
    double Rwc[9];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) Rwc[3 * i + j] = a[3 * j + i];
    line_transform6(Rwc, a + 12, 1.0, false, T);
    line_t6_apply(T, c, o);              // pos_w_pluecker = transformation_line_wc * pos_c_pluecker (:242)
#pragma unroll
    for (int i = 0; i < 6; ++i) out[i] = o[i];
    A.out_status[l] = PLP_LOOP_BA_LM_MOVED;
}

// the launches (line_update_kernels.hip)
hipError_t launch_trim_line_endpoints(hipStream_t st, const LineTrimArgs& A);
hipError_t launch_correct_landmark_lines(hipStream_t st, const LineCorrectArgs& A);
hipError_t launch_loop_ba_propagate_lines(hipStream_t st, const LinePropagateArgs& A);

}  // namespace plp
