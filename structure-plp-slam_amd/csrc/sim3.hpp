// solve::sim3_solver (solve/sim3_solver.cc), one definition of the arithmetic for host and device (plp_sim3_ransac_* / plp_model_sim3_ransac_host,
// plp_model_horn_sim3_host, plp_model_sym_eig4_max_host, include/plp_front.h): the eigenvector of Horn's 4 x 4 matrix by a
// written-down cyclic Jacobi, compute_Sim3 (:193-288), the per-point constants of the constructor (:96-118) and the inlier
// test of count_inliers (:290-325); the samples are ransac.hpp's at K = 3.  f64 with IEEE + - * / sqrt only (the equirectangular reprojection's asin / atan2 aside, D5 item 2), every sum
// left to right, floats where the reference holds floats; translation units that include this file are compiled with -ffp-contract=off.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/plp_front.h"
#include "ransac.hpp"
#include "reproject.hpp"

namespace plp {

constexpr int kSim3MaxSlots = 8192;                   // n_cap limit of the entries (a rank fits 16 bits)
constexpr int kSim3CtxInts = 4;                       // per problem: num_common, best count, best iteration
constexpr int kSim3HypDoubles = 38;                   // per hypothesis: m21 (12), m12 (12), rot_12 (9), trans_12 (3), scale_12, whether it exists
constexpr int kEig4SweepLimit = 30;                   // sweeps that rotate; scene matrices need at most 5 (tests/test_sim3_solver_cpu.py)
constexpr double kEig4SkipTol = 0x1p-106;             // a pair is left alone unless a_pq^2 > 2^-106 (a_pp^2 + a_qq^2)

// entry (i, j) of the symmetric matrix kept as its upper triangle in 10 doubles
__host__ __device__ constexpr int eig4_at(int i, int j) { return i <= j ? (i * (7 - i)) / 2 + j : (j * (7 - j)) / 2 + i; }

// One pair (P, Q), P < Q, of the sweep: the two-sided rotation that makes a_PQ zero (Rutishauser's formulas), applied to S and to the
// accumulated V (row-major, columns are the eigenvectors).  Returns whether it rotated.
template <int P, int Q>
__host__ __device__ __forceinline__ bool eig4_rotate(double (&S)[10], double (&V)[16]) {
    const double apq = S[eig4_at(P, Q)], app = S[eig4_at(P, P)], aqq = S[eig4_at(Q, Q)];
    if (!(apq * apq > kEig4SkipTol * (app * app + aqq * aqq))) return false;   // the fixed skip test; a NaN or an overflowing square skips too
    const double theta = (aqq - app) / (2.0 * apq);
    const double root = __builtin_sqrt(1.0 + theta * theta);
    const double t = theta >= 0.0 ? 1.0 / (theta + root) : -1.0 / (root - theta);
    const double c = 1.0 / __builtin_sqrt(1.0 + t * t);
    const double s = c * t;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (k == P || k == Q) continue;
        const double akp = S[eig4_at(k, P)], akq = S[eig4_at(k, Q)];
        S[eig4_at(k, P)] = c * akp - s * akq;
        S[eig4_at(k, Q)] = s * akp + c * akq;
    }
    S[eig4_at(P, P)] = app - t * apq;
    S[eig4_at(Q, Q)] = aqq + t * apq;
    S[eig4_at(P, Q)] = 0.0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const double vp = V[4 * r + P], vq = V[4 * r + Q];
        V[4 * r + P] = c * vp - s * vq;
        V[4 * r + Q] = s * vp + c * vq;
    }
    return true;
}

// N row-major, symmetric: only its upper triangle is read.  v = the column of V that belongs to the largest diagonal entry after the sweeps
// (ties and NaN: the lowest index), unit length up to rounding, sign unspecified.  Returns the number of sweeps that rotated;
// kEig4SweepLimit = the limit was reached.
__host__ __device__ __forceinline__ int sym_eig4_max(const double N[16], double v[4]) {
    double S[10], V[16];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = i; j < 4; ++j) S[eig4_at(i, j)] = N[4 * i + j];
#pragma unroll
    for (int i = 0; i < 16; ++i) V[i] = (i % 5 == 0) ? 1.0 : 0.0;
    int n = 0;
    while (n < kEig4SweepLimit) {
        bool any = eig4_rotate<0, 1>(S, V);            // the pairs in a fixed order
        any |= eig4_rotate<0, 2>(S, V);
        any |= eig4_rotate<0, 3>(S, V);
        any |= eig4_rotate<1, 2>(S, V);
        any |= eig4_rotate<1, 3>(S, V);
        any |= eig4_rotate<2, 3>(S, V);
        if (!any) break;
        ++n;
    }
    int best = 0;
    double lb = S[eig4_at(0, 0)];
    if (S[eig4_at(1, 1)] > lb) { best = 1; lb = S[eig4_at(1, 1)]; }
    if (S[eig4_at(2, 2)] > lb) { best = 2; lb = S[eig4_at(2, 2)]; }
    if (S[eig4_at(3, 3)] > lb) { best = 3; lb = S[eig4_at(3, 3)]; }
#pragma unroll
    for (int r = 0; r < 4; ++r) v[r] = best == 0 ? V[4 * r] : best == 1 ? V[4 * r + 1] : best == 2 ? V[4 * r + 2] : V[4 * r + 3];
    return n;
}

// One hypothesis as count_inliers uses it: m21 = ((double)scale_21 * rot_21 row-major, trans_21), m12 likewise -- the first 12 entries of a
// pose row, which reproject<MODEL> reads -- beside what find_via_ransac keeps of it.
struct Sim3Hyp {
    double rot_12[9], trans_12[3];
    double rot_21[9], trans_21[3];
    float scale_12, scale_21;
    int sweeps;
};

// sim3_solver::compute_Sim3 (:193-288).  pts_1 / pts_2 row-major 3 x 3, column c = sample c (:150-154).
__host__ __device__ __forceinline__ void horn_sim3(const double pts_1[9], const double pts_2[9], bool fix_scale, Sim3Hyp& H) {
    double c1[3], c2[3], a1[9], a2[9];
#pragma unroll
    for (int r = 0; r < 3; ++r) {                                   // rowwise().mean(): the sum left to right, divided by 3 (:201-202)
        c1[r] = ((pts_1[3 * r] + pts_1[3 * r + 1]) + pts_1[3 * r + 2]) / 3.0;
        c2[r] = ((pts_2[3 * r] + pts_2[3 * r + 1]) + pts_2[3 * r + 2]) / 3.0;
#pragma unroll
        for (int c = 0; c < 3; ++c) {                               // :205-208
            a1[3 * r + c] = pts_1[3 * r + c] - c1[r];
            a2[3 * r + c] = pts_2[3 * r + c] - c2[r];
        }
    }
    double M[9];                                                    // M = ave_pts_1 * ave_pts_2^T (:213)
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) M[3 * i + j] = (a1[3 * i] * a2[3 * j] + a1[3 * i + 1] * a2[3 * j + 1]) + a1[3 * i + 2] * a2[3 * j + 2];
    const double Sxx = M[0], Syx = M[3], Szx = M[6], Sxy = M[1], Syy = M[4], Szy = M[7], Sxz = M[2], Syz = M[5], Szz = M[8];   // :216-224
    const double N[16] = {(Sxx + Syy) + Szz, Syz - Szy, Szx - Sxz, Sxy - Syx,                                                 // :226-229
                          Syz - Szy, (Sxx - Syy) - Szz, Sxy + Syx, Szx + Sxz,
                          Szx - Sxz, Sxy + Syx, (-Sxx + Syy) - Szz, Syz + Szy,
                          Sxy - Syx, Szx + Sxz, Syz + Szy, (-Sxx - Syy) + Szz};
    double e[4];
    H.sweeps = sym_eig4_max(N, e);                                  // D13, in place of Eigen::EigenSolver (:234-252)
    const double e2 = ((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]) + e[3] * e[3];   // eigenvector.normalize() (:253): nothing for a zero vector
    if (e2 > 0.0) {
        const double en = __builtin_sqrt(e2);
        e[0] = e[0] / en; e[1] = e[1] / en; e[2] = e[2] / en; e[3] = e[3] / en;
    }
    const double qn = __builtin_sqrt(((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]) + e[3] * e[3]);   // q_rot_21.normalized() (:259): coeffs / norm
    const double w = e[0] / qn, x = e[1] / qn, y = e[2] / qn, z = e[3] / qn;                        // Quaterniond(w, x, y, z) (:256)
    double* R = H.rot_21;                                           // toRotationMatrix(), Eigen/src/Geometry/Quaternion.h
    {
        const double tx = 2.0 * x, ty = 2.0 * y, tz = 2.0 * z;
        const double twx = tx * w, twy = ty * w, twz = tz * w, txx = tx * x, txy = ty * x, txz = tz * x, tyy = ty * y, tyz = tz * y, tzz = tz * z;
        R[0] = 1.0 - (tyy + tzz); R[1] = txy - twz; R[2] = txz + twy;
        R[3] = txy + twz; R[4] = 1.0 - (txx + tzz); R[5] = tyz - twx;
        R[6] = txz - twy; R[7] = tyz + twx; R[8] = 1.0 - (txx + tyy);
    }
    if (fix_scale) {
        H.scale_21 = 1.0f;                                          // :265
    } else {
        double denom = 0.0, numer = 0.0;                            // :270-277; both sums run over the matrix in storage (column-major) order
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                const double in2 = (R[3 * r] * a1[c] + R[3 * r + 1] * a1[3 + c]) + R[3 * r + 2] * a1[6 + c];   // (rot_21 * ave_pts_1)(r, c)
                const double d = a1[3 * r + c] * a1[3 * r + c], m = a2[3 * r + c] * in2;
                denom = denom + d;
                numer = numer + m;
            }
        H.scale_21 = (float)(numer / denom);
    }
    {   // trans_21 = centroid_2 - scale_21 * rot_21 * centroid_1 (:282): (float * Mat33) * Vec3
        const double s = (double)H.scale_21;
#pragma unroll
        for (int r = 0; r < 3; ++r) H.trans_21[r] = c2[r] - (((s * R[3 * r]) * c1[0] + (s * R[3 * r + 1]) * c1[1]) + (s * R[3 * r + 2]) * c1[2]);
    }
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) H.rot_12[3 * r + c] = R[3 * c + r];   // :285
    H.scale_12 = (float)(1.0 / (double)H.scale_21);                 // :286
    {   // trans_12 = -scale_12 * rot_12 * trans_21 (:287)
        const double s = (double)(-H.scale_12);
#pragma unroll
        for (int r = 0; r < 3; ++r)
            H.trans_12[r] = ((s * H.rot_12[3 * r]) * H.trans_21[0] + (s * H.rot_12[3 * r + 1]) * H.trans_21[1]) + (s * H.rot_12[3 * r + 2]) * H.trans_21[2];
    }
}

// scale * rot and trans as the 12 entries reproject<MODEL> reads (reproject_to_other_image, :338: `scale_21 * rot_21` is float * Mat33)
__host__ __device__ __forceinline__ void sim3_pose_row(const double rot[9], const double trans[3], float scale, double m[12]) {
    const double s = (double)scale;
#pragma unroll
    for (int i = 0; i < 9; ++i) m[i] = s * rot[i];
    m[9] = trans[0]; m[10] = trans[1]; m[11] = trans[2];
}

// the camera fields reproject<MODEL> reads (set_camera, matcher_context.hpp) and what every problem of a call shares
struct Sim3Args {
    int model;
    double fx, fy, cx, cy, fxb, cols_d, rows_d;
    float bounds[4];                                                // not read by anything the solver uses (reproject's `in`)
    int P, n_cap, iters, fix_scale, min_num_inliers, num_levels;
    unsigned long long seed;
    float level_sigma_sq_1[16], level_sigma_sq_2[16];
    const uint8_t* valid; const double* pos_w_1; const double* pos_w_2; const int32_t* octave_1; const int32_t* octave_2; const int32_t* counts;
    const double* pose_1; const double* pose_2; const int32_t* samples;
    uint8_t* out_status; int32_t* out_num_common; double* out_rot_12; double* out_trans_12; float* out_scale_12; int32_t* out_num_inliers;
    int32_t* out_best_iter; uint8_t* out_inliers; int32_t* out_hyp_inliers;
    int32_t* ctx;                                                   // DEVICE, P x kSim3CtxInts: num_common, the best count, its iteration
    double* ctx_hyp;                                                // DEVICE, P x kSim3HypDoubles x iters: the hypotheses
};
hipError_t launch_sim3_ransac(hipStream_t st, const Sim3Args& A);   // sim3_kernels.hip: three launches, the first error

// What the constructor keeps of one common point (:96-118): the two camera-frame points, their reprojections into their own images and the
// two float thresholds.  never: a point behind its own camera (perspective, fisheye), whose reprojected_1_ / reprojected_2_ entry the
// reference leaves uninitialised (:352-356) -- not an inlier of any hypothesis (D13) -- or an octave outside the sigma tables (.at() throws).
struct Sim3Point {
    double x1[3], x2[3], u1, v1, u2, v2;
    float thr_1, thr_2;
    bool never;
};

// P1 / P2: the problem's two pose rows, sigma_1 / sigma_2: the two tables of A (the kernels read all four from copies in LDS: a lane's
// octave is no uniform index, and the pointers need not stay in scalar registers)
template <int MODEL>
__host__ __device__ __forceinline__ Sim3Point sim3_point(const Sim3Args& A, const double* P1, const double* P2, const float* sigma_1, const float* sigma_2,
                                                         int p, int slot) {
    const size_t s = (size_t)p * A.n_cap + slot;
    const double* w1 = A.pos_w_1 + 3 * s;
    const double* w2 = A.pos_w_2 + 3 * s;
    Sim3Point pt;
#pragma unroll
    for (int r = 0; r < 3; ++r) {                                   // rot_1w * pos_w_1 + trans_1w (:109, :112)
        pt.x1[r] = ((P1[3 * r] * w1[0] + P1[3 * r + 1] * w1[1]) + P1[3 * r + 2] * w1[2]) + P1[9 + r];
        pt.x2[r] = ((P2[3 * r] * w2[0] + P2[3 * r + 1] * w2[1]) + P2[3 * r + 2] * w2[2]) + P2[9 + r];
    }
    const double I[12] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0};   // reproject_to_same_image (:354)
    const Reproj r1 = reproject<MODEL>(A, I, pt.x1[0], pt.x1[1], pt.x1[2]);
    const Reproj r2 = reproject<MODEL>(A, I, pt.x2[0], pt.x2[1], pt.x2[2]);
    pt.u1 = r1.u; pt.v1 = r1.v; pt.u2 = r2.u; pt.v2 = r2.v;
    const int o1 = A.octave_1[s], o2 = A.octave_2[s];
    const bool lv = (unsigned)o1 < (unsigned)A.num_levels && (unsigned)o2 < (unsigned)A.num_levels;
    pt.thr_1 = lv ? 9.21034f * sigma_1[o1] : 0.0f;       // chi_sq_2D * sigma_sq_1, a float product (:67, :102-103)
    pt.thr_2 = lv ? 9.21034f * sigma_2[o2] : 0.0f;
    pt.never = !r1.wrote || !r2.wrote || !lv;
    return pt;
}

// the loop body of count_inliers (:306-322) for one common point; a reprojection the camera did not write (:336-340) is no inlier (D13)
template <int MODEL>
__host__ __device__ __forceinline__ bool sim3_inlier(const Sim3Args& A, const double m21[12], const double m12[12], const double x1[3], const double x2[3],
                                                     double u1, double v1, double u2, double v2, float thr_1, float thr_2, bool never) {
    const Reproj a = reproject<MODEL>(A, m21, x1[0], x1[1], x1[2]);   // point of key frame 1 in image 2
    const Reproj b = reproject<MODEL>(A, m12, x2[0], x2[1], x2[2]);   // point of key frame 2 in image 1
    const double d2u = a.u - u2, d2v = a.v - v2, d1u = b.u - u1, d1v = b.v - v1;
    const double error_in_2 = d2u * d2u + d2v * d2v, error_in_1 = d1u * d1u + d1v * d1v;
    return !never && a.wrote && b.wrote && error_in_2 < (double)thr_2 && error_in_1 < (double)thr_1;
}

// the hypothesis of three common points given by their slots: their camera-frame points are formed as the constructor forms them
__host__ __device__ __forceinline__ void sim3_hypothesis(const Sim3Args& A, const double* P1, const double* P2, int p, const int slot[3], Sim3Hyp& H) {
    double pts_1[9], pts_2[9];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const size_t s = (size_t)p * A.n_cap + slot[c];
        const double* w1 = A.pos_w_1 + 3 * s;
        const double* w2 = A.pos_w_2 + 3 * s;
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            pts_1[3 * r + c] = ((P1[3 * r] * w1[0] + P1[3 * r + 1] * w1[1]) + P1[3 * r + 2] * w1[2]) + P1[9 + r];
            pts_2[3 * r + c] = ((P2[3 * r] * w2[0] + P2[3 * r + 1] * w2[1]) + P2[3 * r + 2] * w2[2]) + P2[9 + r];
        }
    }
    horn_sim3(pts_1, pts_2, A.fix_scale != 0, H);
}

}  // namespace plp
