// optimize::pose_optimizer / pose_optimizer_extended_line (optimize/pose_optimizer.cc:53-229, pose_optimizer_extended_line.cc:62-305), one
// definition of the arithmetic for host and device (plp_pose_optimize_* / plp_model_pose_*_host, include/plp_front.h):
// the vertex (g2o::SE3Quat as shot_vertex holds it), the three edges, the Huber kernel, the 28 per-edge terms of the quadratic form; the 6 x 6
// Cholesky and the Levenberg-Marquardt bookkeeping are levenberg.hpp's.  f64 with IEEE + - * / sqrt only, in the order written, floats where the reference holds
// floats; translation units that include this file are compiled with -ffp-contract=off.  sin / cos are pose_sincos() below, not a library's.
//
// Everything works on memory the caller names (PoseWork, the term rows): on the device that is LDS, reached with run-time indices, so that no
// kernel keeps an indexed array in registers; on the host it is the stack.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/plp_front.h"
#include "levenberg.hpp"

namespace plp {

constexpr int kPoseMaxSlots = 8192;      // n_cap / l_cap limit of the entries (a rank fits 16 bits)
constexpr int kPoseTerms = 28;           // per edge: H upper triangle row-major (21), b (6), robust chi2 (1)
constexpr int kPoseMinObs = 5;           // :153 / :162, :218 / :264
constexpr float kPoseChiSq2D = 5.99146f;
constexpr float kPoseChiSq3D = 7.81473f;
constexpr double kPoseNumericDelta = 1e-9;   // g2o's numeric Jacobian of a unary edge

// ---- sin and cos (D15 item 1): k = floor(x 2/pi + 1/2), r = (x - k P1) - k P2 (P1 = the first 33 bits of pi/2, so k P1 is exact for |k| < 2^20),
// fdlibm's kernel polynomials on |r| <= pi/4 evaluated by Horner without fma, quadrant from k mod 4.  |x| > 2^20 or not finite: both NaN.
__host__ __device__ __forceinline__ void pose_sincos(double x, double& s, double& c) {
    if (!(x >= -1048576.0 && x <= 1048576.0)) { s = c = __builtin_nan(""); return; }
    const double k = __builtin_floor(x * 6.36619772367581382433e-01 + 0.5);
    const double r = (x - k * 1.57079632673412561417e+00) - k * 6.07710050650619224932e-11;
    const double z = r * r;
    const double ps = -1.66666666666666324348e-01 + z * (8.33333333332248946124e-03 + z * (-1.98412698298579493134e-04 + z * (2.75573137070700676789e-06 +
                      z * (-2.50507602534068634195e-08 + z * 1.58969099521155010221e-10))));
    const double pc = 4.16666666666666019037e-02 + z * (-1.38888888888741095749e-03 + z * (2.48015872894767294178e-05 + z * (-2.75573143513906633035e-07 +
                      z * (2.08757232129817482790e-09 + z * -1.13596475577881948265e-11))));
    const double sr = r + (r * z) * ps;
    const double cr = 1.0 - (0.5 * z - (z * z) * pc);
    const int q = (int)k & 3;
    s = q == 0 ? sr : q == 1 ? cr : q == 2 ? -sr : -cr;
    c = q == 0 ? cr : q == 1 ? -sr : q == 2 ? -cr : sr;
}

// ---- the vertex: est = {qx, qy, qz, qw, tx, ty, tz}
// Eigen::Quaterniond(R), R row-major
__host__ __device__ __forceinline__ void pose_quat_from_rot(const double* R, double* q) {
    double t = (R[0] + R[4]) + R[8];
    if (t > 0.0) {
        t = __builtin_sqrt(t + 1.0);
        q[3] = 0.5 * t;
        t = 0.5 / t;
        q[0] = (R[7] - R[5]) * t;
        q[1] = (R[2] - R[6]) * t;
        q[2] = (R[3] - R[1]) * t;
    } else if (!(R[4] > R[0]) && !(R[8] > R[0])) {      // i = 0: the largest diagonal element, the first among equals
        t = __builtin_sqrt(((R[0] - R[4]) - R[8]) + 1.0);
        q[0] = 0.5 * t;
        t = 0.5 / t;
        q[3] = (R[7] - R[5]) * t;
        q[1] = (R[3] + R[1]) * t;
        q[2] = (R[6] + R[2]) * t;
    } else if (R[4] > R[0] && !(R[8] > R[4])) {         // i = 1
        t = __builtin_sqrt(((R[4] - R[8]) - R[0]) + 1.0);
        q[1] = 0.5 * t;
        t = 0.5 / t;
        q[3] = (R[2] - R[6]) * t;
        q[2] = (R[7] + R[5]) * t;
        q[0] = (R[1] + R[3]) * t;
    } else {                                             // i = 2
        t = __builtin_sqrt(((R[8] - R[0]) - R[4]) + 1.0);
        q[2] = 0.5 * t;
        t = 0.5 / t;
        q[3] = (R[3] - R[1]) * t;
        q[0] = (R[2] + R[6]) * t;
        q[1] = (R[5] + R[7]) * t;
    }
}
// SE3Quat::normalizeRotation: w < 0 negates, then Eigen's normalize()
__host__ __device__ __forceinline__ void pose_quat_normalize(double* q) {
    if (q[3] < 0.0) { q[0] = -q[0]; q[1] = -q[1]; q[2] = -q[2]; q[3] = -q[3]; }
    const double n2 = ((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3];
    if (n2 > 0.0) {
        const double n = __builtin_sqrt(n2);
        q[0] = q[0] / n; q[1] = q[1] / n; q[2] = q[2] / n; q[3] = q[3] / n;
    }
}
// Eigen's toRotationMatrix, R row-major
__host__ __device__ __forceinline__ void pose_rot_from_quat(const double* q, double* R) {
    const double tx = 2.0 * q[0], ty = 2.0 * q[1], tz = 2.0 * q[2];
    const double twx = tx * q[3], twy = ty * q[3], twz = tz * q[3];
    const double txx = tx * q[0], txy = ty * q[0], txz = tz * q[0];
    const double tyy = ty * q[1], tyz = tz * q[1], tzz = tz * q[2];
    R[0] = 1.0 - (tyy + tzz); R[1] = txy - twz; R[2] = txz + twy;
    R[3] = txy + twz; R[4] = 1.0 - (txx + tzz); R[5] = tyz - twx;
    R[6] = txz - twy; R[7] = tyz + twx; R[8] = 1.0 - (txx + tyy);
}
// Eigen's quaternion times vector: uv = 2 (q.vec x v); v + w uv + q.vec x uv
__host__ __device__ __forceinline__ void pose_quat_rotate(const double* q, double vx, double vy, double vz, double& ox, double& oy, double& oz) {
    double ux = q[1] * vz - q[2] * vy, uy = q[2] * vx - q[0] * vz, uz = q[0] * vy - q[1] * vx;
    ux = ux + ux; uy = uy + uy; uz = uz + uz;
    ox = (vx + q[3] * ux) + (q[1] * uz - q[2] * uy);
    oy = (vy + q[3] * uy) + (q[2] * ux - q[0] * uz);
    oz = (vz + q[3] * uz) + (q[0] * uy - q[1] * ux);
}
// SE3Quat::map: r p + t
__host__ __device__ __forceinline__ void pose_map(const double* est, const double* p, double& x, double& y, double& z) {
    pose_quat_rotate(est, p[0], p[1], p[2], x, y, z);
    x = x + est[4]; y = y + est[5]; z = z + est[6];
}
// util::converter::to_g2o_SE3: SE3Quat(rot, trans)
__host__ __device__ __forceinline__ void pose_est_from_pose(const double* pose12, double* est) {
    pose_quat_from_rot(pose12, est);
    pose_quat_normalize(est);
    est[4] = pose12[9]; est[5] = pose12[10]; est[6] = pose12[11];
}
// set_cam_pose + update_pose_params: rot_cw, trans_cw, cam_center = -rot_cw^T trans_cw as plp.frame_pose forms it
__host__ __device__ __forceinline__ void pose_pose_from_est(const double* est, double* pose15) {
    pose_rot_from_quat(est, pose15);
    pose15[9] = est[4]; pose15[10] = est[5]; pose15[11] = est[6];
    for (int i = 0; i < 3; ++i)
        pose15[12 + i] = ((-pose15[i]) * pose15[9] + (-pose15[3 + i]) * pose15[10]) + (-pose15[6 + i]) * pose15[11];
}
// SE3Quat::exp(u) * est (shot_vertex::oplusImpl), u = (omega, upsilon).  out may not alias est.
__host__ __device__ __forceinline__ void pose_oplus(const double* u, const double* est, double* out) {
    const double a = u[0], b = u[1], c = u[2];
    const double theta = __builtin_sqrt((a * a + b * b) + c * c);
    // Omega = skew(omega), Omega2 = Omega Omega
    const double O2[9] = {-(b * b + c * c), a * b, a * c, a * b, -(a * a + c * c), b * c, a * c, b * c, -(a * a + b * b)};
    const double O[9] = {0.0, -c, b, c, 0.0, -a, -b, a, 0.0};
    double k1, k2, v1, v2;
    if (theta < 0.00001) {
        k1 = 1.0; k2 = 0.5; v1 = 0.5; v2 = 1.0 / 6.0;
    } else {
        double s, co;
        pose_sincos(theta, s, co);
        const double th2 = theta * theta;
        k1 = s / theta; k2 = (1.0 - co) / th2; v1 = k2; v2 = (theta - s) / (th2 * theta);
    }
    double R[9], V[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        const double id = (i == 0 || i == 4 || i == 8) ? 1.0 : 0.0;
        R[i] = (id + k1 * O[i]) + k2 * O2[i];
        V[i] = (id + v1 * O[i]) + v2 * O2[i];
    }
    double e[4];
    pose_quat_from_rot(R, e);
    pose_quat_normalize(e);
    const double et0 = (V[0] * u[3] + V[1] * u[4]) + V[2] * u[5];
    const double et1 = (V[3] * u[3] + V[4] * u[4]) + V[5] * u[5];
    const double et2 = (V[6] * u[3] + V[7] * u[4]) + V[8] * u[5];
    // SE3Quat::operator*: r = e r_est (Eigen's product), t = e_t + e t_est, normalizeRotation
    const double* p = est;
    out[3] = ((e[3] * p[3] - e[0] * p[0]) - e[1] * p[1]) - e[2] * p[2];
    out[0] = ((e[3] * p[0] + e[0] * p[3]) + e[1] * p[2]) - e[2] * p[1];
    out[1] = ((e[3] * p[1] + e[1] * p[3]) + e[2] * p[0]) - e[0] * p[2];
    out[2] = ((e[3] * p[2] + e[2] * p[3]) + e[0] * p[1]) - e[1] * p[0];
    double rx, ry, rz;
    pose_quat_rotate(e, p[4], p[5], p[6], rx, ry, rz);
    out[4] = et0 + rx; out[5] = et1 + ry; out[6] = et2 + rz;
    pose_quat_normalize(out);
}

// ---- the camera of the edges
struct PoseCam {
    double fx, fy, cx, cy, fxb;
    double k20, k21, k22;        // the line edge's _K, last row: -fy cx, -fx cy, fx fy (pose_opt_edge_wrapper.h:275-277)
};
__host__ __device__ __forceinline__ PoseCam pose_cam(double fx, double fy, double cx, double cy, double fxb) {
    PoseCam C;
    C.fx = fx; C.fy = fy; C.cx = cx; C.cy = cy; C.fxb = fxb;
    C.k20 = (-fy) * cx; C.k21 = (-fx) * cy; C.k22 = fx * fy;
    return C;
}

// ---- point edges (perspective_pose_opt_edge.h:54-59, :90-95): the error at est, two- or three-dimensional (e2 = 0 for mono); returns chi2
__host__ __device__ __forceinline__ double pose_point_error(const double* est, const PoseCam& C, const double* pos_w, double ox, double oy, double orr,
                                                            bool mono, double w, double& pcx, double& pcy, double& pcz, double& e0, double& e1, double& e2) {
    pose_map(est, pos_w, pcx, pcy, pcz);
    const double rx = (C.fx * pcx) / pcz + C.cx;
    e0 = ox - rx;
    e1 = oy - ((C.fy * pcy) / pcz + C.cy);
    if (mono) { e2 = 0.0; return e0 * (w * e0) + e1 * (w * e1); }
    e2 = orr - (rx - C.fxb / pcz);
    return (e0 * (w * e0) + e1 * (w * e1)) + e2 * (w * e2);
}

// RobustKernelHuber::robustify
__host__ __device__ __forceinline__ void pose_huber(double e2, double delta, double& rho0, double& rho1) {
    const double dsqr = delta * delta;
    if (e2 <= dsqr) { rho0 = e2; rho1 = 1.0; return; }
    const double sqrte = __builtin_sqrt(e2);
    rho0 = (2.0 * sqrte) * delta - dsqr;
    rho1 = delta / sqrte;
}

// The 28 terms of one edge from its Jacobian rows J (rows x 6, row-major at J[6 r + c]), its error and weight: T[t * stride].
// weightedOmega = rho1 w I, omega_r = -(w e) rho1 (BaseUnaryEdge::constructQuadraticForm); kernel off: rho1 = 1, rho0 = chi2.
__host__ __device__ __forceinline__ void pose_terms(const double* J, int rows, double e0, double e1, double e2, double w, double rho0, double rho1,
                                                    double* T, int stride) {
    const double wr = rho1 * w;
    const double o0 = (-(w * e0)) * rho1, o1 = (-(w * e1)) * rho1, o2 = (-(w * e2)) * rho1;
    int t = 0;
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = i; j < 6; ++j) {
            double v = J[i] * (wr * J[j]) + J[6 + i] * (wr * J[6 + j]);
            if (rows == 3) v = v + J[12 + i] * (wr * J[12 + j]);
            T[(t++) * stride] = v;
        }
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        double v = J[i] * o0 + J[6 + i] * o1;
        if (rows == 3) v = v + J[12 + i] * o2;
        T[(21 + i) * stride] = v;
    }
    T[27 * stride] = rho0;
}

// One point edge at est: its chi2 (returned) and its 28 terms (linearizeOplus, perspective_pose_opt_edge.cc:76-101, :142-173).
// robust: the Huber kernel with delta is on.
__host__ __device__ __forceinline__ double pose_point_terms(const double* est, const PoseCam& C, const double* pos_w, double ox, double oy, double orr,
                                                            bool mono, double w, bool robust, double delta, double* T, int stride) {
    double x, y, z, e0, e1, e2;
    const double chi2 = pose_point_error(est, C, pos_w, ox, oy, orr, mono, w, x, y, z, e0, e1, e2);
    const double z_sq = z * z;
    double J[18];
    J[0] = ((x * y) / z_sq) * C.fx;
    J[1] = (-(1.0 + (x * x) / z_sq)) * C.fx;
    J[2] = (y / z) * C.fx;
    J[3] = (-1.0 / z) * C.fx;
    J[4] = 0.0;
    J[5] = (x / z_sq) * C.fx;
    J[6] = (1.0 + (y * y) / z_sq) * C.fy;
    J[7] = (((-x) * y) / z_sq) * C.fy;
    J[8] = ((-x) / z) * C.fy;
    J[9] = 0.0;
    J[10] = (-1.0 / z) * C.fy;
    J[11] = (y / z_sq) * C.fy;
    J[12] = J[0] - (C.fxb * y) / z_sq;
    J[13] = J[1] + (C.fxb * x) / z_sq;
    J[14] = J[2];
    J[15] = J[3];
    J[16] = 0.0;
    J[17] = J[5] - C.fxb / z_sq;
    double rho0 = chi2, rho1 = 1.0;
    if (robust) pose_huber(chi2, delta, rho0, rho1);
    pose_terms(J, mono ? 2 : 3, e0, e1, e2, w, rho0, rho1, T, stride);
    return chi2;
}

// ---- the line edge (pose_opt_edge_line3d_orthonormal.h:62-87): error at est; returns chi2
__host__ __device__ __forceinline__ double pose_line_error(const double* est, const PoseCam& C, const double* L, double xs, double ys, double xe, double ye,
                                                           double w, double& e0, double& e1) {
    double R[9];
    pose_rot_from_quat(est, R);
    const double tx = est[4], ty = est[5], tz = est[6];
    double top[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        // row i of skew(t) R
        double m0, m1, m2;
        if (i == 0) { m0 = (-tz) * R[3] + ty * R[6]; m1 = (-tz) * R[4] + ty * R[7]; m2 = (-tz) * R[5] + ty * R[8]; }
        else if (i == 1) { m0 = tz * R[0] + (-tx) * R[6]; m1 = tz * R[1] + (-tx) * R[7]; m2 = tz * R[2] + (-tx) * R[8]; }
        else { m0 = (-ty) * R[0] + tx * R[3]; m1 = (-ty) * R[1] + tx * R[4]; m2 = (-ty) * R[2] + tx * R[5]; }
        top[i] = ((((R[3 * i] * L[0] + R[3 * i + 1] * L[1]) + R[3 * i + 2] * L[2]) + m0 * L[3]) + m1 * L[4]) + m2 * L[5];
    }
    const double p0 = C.fy * top[0], p1 = C.fx * top[1], p2 = (C.k20 * top[0] + C.k21 * top[1]) + C.k22 * top[2];
    const double den = __builtin_sqrt(p0 * p0 + p1 * p1);
    e0 = ((xs * p0 + ys * p1) + p2) / den;
    e1 = ((xe * p0 + ye * p1) + p2) / den;
    return e0 * (w * e0) + e1 * (w * e1);
}

// The twelve estimates of g2o's numeric Jacobian: pert[7 (2 d)] = exp(+delta e_d) est, pert[7 (2 d + 1)] = exp(-delta e_d) est
__host__ __device__ __forceinline__ void pose_perturb(const double* est, int which, double* out) {
    double u[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    const int d = which >> 1;
    const double v = (which & 1) ? -kPoseNumericDelta : kPoseNumericDelta;
#pragma unroll
    for (int i = 0; i < 6; ++i) u[i] = i == d ? v : 0.0;
    pose_oplus(u, est, out);
}

// One line edge at est with the twelve perturbed estimates: chi2 (returned) and the 28 terms
__host__ __device__ __forceinline__ double pose_line_terms(const double* est, const double* pert, const PoseCam& C, const double* L, double xs, double ys,
                                                           double xe, double ye, double w, bool robust, double delta, double* T, int stride) {
    const double scalar = 1.0 / (2.0 * kPoseNumericDelta);
    // the columns wait in the first twelve term rows, so that the loop over d stays a loop on the device
#pragma unroll 1
    for (int d = 0; d < 6; ++d) {
        double p0, p1, m0, m1;
        pose_line_error(pert + 7 * (2 * d), C, L, xs, ys, xe, ye, w, p0, p1);
        pose_line_error(pert + 7 * (2 * d + 1), C, L, xs, ys, xe, ye, w, m0, m1);
        T[d * stride] = scalar * (p0 - m0);
        T[(6 + d) * stride] = scalar * (p1 - m1);
    }
    double J[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) J[i] = T[i * stride];
    double e0, e1;
    const double chi2 = pose_line_error(est, C, L, xs, ys, xe, ye, w, e0, e1);
    double rho0 = chi2, rho1 = 1.0;
    if (robust) pose_huber(chi2, delta, rho0, rho1);
    pose_terms(J, 2, e0, e1, 0.0, w, rho0, rho1, T, stride);
    return chi2;
}

// ---- the Levenberg-Marquardt state of one frame (levenberg.hpp at N = 6)
struct PoseWork {
    double est[7], bak[7];
    double pert[84];
    double sum[kPoseTerms];      // the sums of the last linearisation: H (21), b (6), robust chi2
    double Lf[36];               // the Cholesky factor, row-major lower
    double x[6], y[6];
    double lambda, ni, current_chi, rho, temp_sum;
    int32_t ok2, qmax, iterations, rejected, go_on, end;
};

// push, solve, update: W.est becomes the tried estimate
__host__ __device__ __forceinline__ void pose_lm_try(PoseWork& W) {
    for (int i = 0; i < 7; ++i) W.bak[i] = W.est[i];
    W.ok2 = lev_chol<6>(W.sum, W.sum + 21, W.lambda, W.Lf, W.y, W.x) ? 1 : 0;
    pose_oplus(W.x, W.bak, W.est);
}
// whether trial `trial` of num_trials runs with the Huber kernels: they are removed after trial num_trials - 2 (unsigned: never for num_trials < 2)
__host__ __device__ __forceinline__ bool pose_trial_robust(int trial, int num_trials) { return num_trials < 2 || trial <= num_trials - 2; }

// ---- the arguments of the launches and of the host build
struct PoseArgs {
    int B, n_cap, l_cap, num_trials, num_each_iter, mono_setup, pose_stride, num_levels, num_levels_lsd;
    PoseCam cam;
    double delta_2d, delta_3d;   // (double)std::sqrt(chi_sq_2D), (double)std::sqrt(chi_sq_3D), floats formed on the host
    float inv_sigma_sq[16], inv_sigma_sq_lsd[16];
    const double* pose_in;
    const int32_t* counts; const int32_t* line_counts;
    const uint8_t* valid; const plp_keypoint* undist; const float* x_right; const double* pos_w;
    const uint8_t* line_valid; const plp_keyline* keylines; const double* pos_w_lines;
    uint8_t* out_status; double* out_pose; int32_t* out_num_init_obs; int32_t* out_num_valid; uint8_t* out_outlier; uint8_t* out_outlier_lines;
    int32_t* out_trial_info; double* out_trial_chi2;
    // buffers of the context (device entries): ranks -> slots, the chi2 of every edge's last evaluation, the edge counts
    uint16_t* ctx_slot; uint16_t* ctx_slot_lines; double* ctx_chi2; int32_t* ctx_n;
};
__host__ __device__ __forceinline__ int pose_count(const PoseArgs& A, int b) {
    const int c = A.counts ? A.counts[b] : A.n_cap;
    return c < 0 ? 0 : c > A.n_cap ? A.n_cap : c;
}
__host__ __device__ __forceinline__ int pose_line_count(const PoseArgs& A, int b) {
    const int c = A.line_counts ? A.line_counts[b] : A.l_cap;
    return c < 0 ? 0 : c > A.l_cap ? A.l_cap : c;
}

hipError_t launch_pose_optimize(hipStream_t st, const PoseArgs& A);

}  // namespace plp
