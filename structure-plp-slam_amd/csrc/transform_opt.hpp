// optimize::transform_optimizer::optimize (optimize/transform_optimizer.cc:47-197), one definition of the arithmetic for host and device
// (plp_transform_optimize_* / plp_model_transform_*_host, include/plp_front.h): the vertex (g2o::Sim3 as
// transform_vertex holds it), the forward and backward reprojection edges with g2o's numeric Jacobian, the 36 per-edge terms of the quadratic
// form and exp.  Everything D15 fixes is pose_opt.hpp's and is used from there: the quaternion arithmetic, pose_sincos, Huber, the order of
// the operations.  The 7 x 7 Cholesky and the Levenberg-Marquardt bookkeeping are levenberg.hpp's at N = 7.  Translation units that include
// this file are compiled with -ffp-contract=off.
//
// As in pose_opt.hpp everything works on memory the caller names (TfWork, the term rows): LDS on the device, the stack on the host.
#pragma once
#include "pose_opt.hpp"

namespace plp {

constexpr int kTfMaxSlots = 8192;        // n_cap limit of the entries (a rank fits 16 bits)
constexpr int kTfDim = 7;                // omega, upsilon, sigma
constexpr int kTfTerms = 36;             // per edge: H upper triangle row-major (28), b (7), robust chi2 (1)
constexpr int kTfFirstIters = 5;         // :131 optimize(5)
constexpr int kTfMinInliers = 10;        // :156
constexpr int kTfCtxInts = 11;           // per problem between the launches: count, early return, inliers, two rounds of four counters
constexpr int kTfCtxDoubles = 12;        // ... and the estimate (8), two rounds of chi2 and lambda
constexpr int kTfSims = 15;              // the fourteen perturbed estimates of a linearisation and the estimate itself

// ---- exp (D16): k = floor(x / ln2 + 1/2), r = (x - k ln2_hi) - k ln2_lo (k ln2_hi is exact for |k| <= 1010: ln2_hi has 32 significant bits, its last 21 mantissa bits are zero), fdlibm's
// polynomial for exp(r) on |r| <= ln2 / 2 by Horner without fma, times 2^k built from its bits (exact: the result is a normal number on the
// whole domain).  |x| > 700 or not finite: NaN.
__host__ __device__ __forceinline__ double pose_exp(double x) {
    if (!(x >= -700.0 && x <= 700.0)) return __builtin_nan("");
    const double k = __builtin_floor(x * 1.44269504088896338700e+00 + 0.5);
    const double hi = x - k * 6.93147180369123816490e-01;
    const double lo = k * 1.90821492927058770002e-10;
    const double r = hi - lo;
    const double t = r * r;
    const double c = r - t * (1.66666666666666019037e-01 + t * (-2.77777777770155933842e-03 + t * (6.61375632143793436117e-05 +
                     t * (-1.65339022054652515390e-06 + t * 4.13813679705723846039e-08))));
    const double y = 1.0 - ((lo - (r * c) / (2.0 - c)) - hi);
    const uint64_t bits = (uint64_t)((int64_t)k + 1023) << 52;
    double p;
    __builtin_memcpy(&p, &bits, 8);
    return y * p;
}

// ---- the vertex: est = {qx, qy, qz, qw, tx, ty, tz, s}.  No constructor and no product normalises the quaternion (D16).
// g2o::Sim3(rot_12, trans_12, (double)scale_12)
__host__ __device__ __forceinline__ void tf_est_from_input(const double* rot9, const double* trans3, float scale, double* est) {
    pose_quat_from_rot(rot9, est);
    est[4] = trans3[0]; est[5] = trans3[1]; est[6] = trans3[2];
    est[7] = (double)scale;
}
// Sim3::map: s (r p) + t
__host__ __device__ __forceinline__ void tf_map(const double* est, double px, double py, double pz, double& x, double& y, double& z) {
    pose_quat_rotate(est, px, py, pz, x, y, z);
    x = est[7] * x + est[4]; y = est[7] * y + est[5]; z = est[7] * z + est[6];
}
// Sim3::inverse: (r*, r* ((-1 / s) t), 1 / s).  out may not alias est.
__host__ __device__ __forceinline__ void tf_inverse(const double* est, double* out) {
    out[0] = -est[0]; out[1] = -est[1]; out[2] = -est[2]; out[3] = est[3];
    const double c = -1.0 / est[7];
    double x, y, z;
    pose_quat_rotate(out, c * est[4], c * est[5], c * est[6], x, y, z);
    out[4] = x; out[5] = y; out[6] = z;
    out[7] = 1.0 / est[7];
}
// Sim3::operator*: r = a.r b.r (Eigen's product), t = a.s (a.r b.t) + a.t, s = a.s b.s.  out may alias neither.
__host__ __device__ __forceinline__ void tf_mul(const double* a, const double* b, double* out) {
    out[3] = ((a[3] * b[3] - a[0] * b[0]) - a[1] * b[1]) - a[2] * b[2];
    out[0] = ((a[3] * b[0] + a[0] * b[3]) + a[1] * b[2]) - a[2] * b[1];
    out[1] = ((a[3] * b[1] + a[1] * b[3]) + a[2] * b[0]) - a[0] * b[2];
    out[2] = ((a[3] * b[2] + a[2] * b[3]) + a[0] * b[1]) - a[1] * b[0];
    double x, y, z;
    pose_quat_rotate(a, b[4], b[5], b[6], x, y, z);
    out[4] = a[7] * x + a[4]; out[5] = a[7] * y + a[5]; out[6] = a[7] * z + a[6];
    out[7] = a[7] * b[7];
}
// where tf_oplus takes exp, sin and cos from: D16's functions with their coefficients as literals (pose_graph.hpp reads the same coefficients from its shared state)
struct TfMathLit {
    __host__ __device__ __forceinline__ double exp(double x) const { return pose_exp(x); }
    __host__ __device__ __forceinline__ void sincos(double x, double& s, double& c) const { pose_sincos(x, s, c); }
};
// Sim3(update) * est (transform_vertex::oplusImpl), update = (omega, upsilon, sigma); fix_scale: sigma is taken as 0.  out may not alias est.
template <class M = TfMathLit>
__host__ __device__ __forceinline__ void tf_oplus(const double* u, bool fix_scale, const double* est, double* out, const M& math = M()) {
    const double a = u[0], b = u[1], c = u[2];
    const double sigma = fix_scale ? 0.0 : u[6];
    const double theta = __builtin_sqrt((a * a + b * b) + c * c);
    const double s = math.exp(sigma);
    const double O2[9] = {-(b * b + c * c), a * b, a * c, a * b, -(a * a + c * c), b * c, a * c, b * c, -(a * a + b * b)};
    const double O[9] = {0.0, -c, b, c, 0.0, -a, -b, a, 0.0};
    const double eps = 0.00001;
    double A, B, C, k1 = 1.0, k2 = 1.0;      // R = I + k1 Omega + k2 Omega2; theta < eps: I + Omega + Omega2
    double si = 0.0, co = 1.0;
    if (!(theta < eps)) {
        math.sincos(theta, si, co);
        k1 = si / theta;
        k2 = (1.0 - co) / (theta * theta);
    }
    if (__builtin_fabs(sigma) < eps) {
        C = 1.0;
        if (theta < eps) {
            A = 0.5; B = 1.0 / 6.0;
        } else {
            const double th2 = theta * theta;
            A = (1.0 - co) / th2;
            B = (theta - si) / (th2 * theta);
        }
    } else {
        C = (s - 1.0) / sigma;
        const double sg2 = sigma * sigma;
        if (theta < eps) {
            A = ((sigma - 1.0) * s + 1.0) / sg2;
            B = (((0.5 * sg2 - sigma) + 1.0) * s) / (sg2 * sigma);
        } else {
            const double sa = s * si, sb = s * co;
            const double th2 = theta * theta;
            const double cc = th2 + sg2;
            A = (sa * sigma + (1.0 - sb) * theta) / (theta * cc);
            B = (C - ((sb - 1.0) * sigma + sa * theta) / cc) / th2;
        }
    }
    double R[9], W[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        const double id = (i == 0 || i == 4 || i == 8) ? 1.0 : 0.0;
        R[i] = (id + k1 * O[i]) + k2 * O2[i];
        W[i] = (A * O[i] + B * O2[i]) + C * id;
    }
    double e[8];
    pose_quat_from_rot(R, e);
    e[4] = (W[0] * u[3] + W[1] * u[4]) + W[2] * u[5];
    e[5] = (W[3] * u[3] + W[4] * u[4]) + W[5] * u[5];
    e[6] = (W[6] * u[3] + W[7] * u[4]) + W[8] * u[5];
    e[7] = s;
    tf_mul(e, est, out);
}
// estimate `which` of a linearisation: 2 d = Sim3(+delta e_d) est, 2 d + 1 = Sim3(-delta e_d) est, 14 = est itself
// (the host build's; k_transform_optimize forms the same update vector itself and sends it, like the tried step of tf_lm_update, through its ONE inlined
// tf_oplus -- two call sites cost 40 VGPRs there: profiles/r16_transform_optimizer.md section 1)
__host__ __device__ __forceinline__ void tf_perturb(const double* est, int which, bool fix_scale, double* out) {
    if (which >= 2 * kTfDim) {
#pragma unroll
        for (int i = 0; i < 8; ++i) out[i] = est[i];
        return;
    }
    double u[kTfDim];
    const int d = which >> 1;
    const double v = (which & 1) ? -kPoseNumericDelta : kPoseNumericDelta;
#pragma unroll
    for (int i = 0; i < kTfDim; ++i) u[i] = i == d ? v : 0.0;
    tf_oplus(u, fix_scale, est, out);
}

// ---- the edges.  A forward edge (forward_reproj_edge.h:52-68) maps the candidate's landmark with Sim3_12 into key frame 1, a backward edge
// (backward_reproj_edge.h:52-69) the current key frame's landmark with Sim3_12.inverse() into key frame 2: one function, given the similarity.
// rot_cw pos_w + trans_cw of the edge's key frame (pose row: rot row-major, trans)
__host__ __device__ __forceinline__ void tf_to_camera(const double* pose, const double* pw, double& x, double& y, double& z) {
    x = ((pose[0] * pw[0] + pose[1] * pw[1]) + pose[2] * pw[2]) + pose[9];
    y = ((pose[3] * pw[0] + pose[4] * pw[1]) + pose[5] * pw[2]) + pose[10];
    z = ((pose[6] * pw[0] + pose[7] * pw[1]) + pose[8] * pw[2]) + pose[11];
}
// the error at the similarity `sim` of the point pc (in the other key frame's camera); returns chi2
__host__ __device__ __forceinline__ double tf_edge_error(const double* sim, const PoseCam& C, double pcx, double pcy, double pcz, double ox, double oy,
                                                         double w, double& e0, double& e1) {
    double x, y, z;
    tf_map(sim, pcx, pcy, pcz, x, y, z);
    e0 = ox - ((C.fx * x) / z + C.cx);
    e1 = oy - ((C.fy * y) / z + C.cy);
    return e0 * (w * e0) + e1 * (w * e1);
}
// The 36 terms of one edge from its Jacobian rows J (2 x 7, row-major), its error and weight: T[t * stride] (constructQuadraticForm as pose_terms)
__host__ __device__ __forceinline__ void tf_terms(const double* J, double e0, double e1, double w, double rho0, double rho1, double* T, int stride) {
    const double wr = rho1 * w;
    const double o0 = (-(w * e0)) * rho1, o1 = (-(w * e1)) * rho1;
    int t = 0;
#pragma unroll
    for (int i = 0; i < kTfDim; ++i)
#pragma unroll
        for (int j = i; j < kTfDim; ++j) T[(t++) * stride] = J[i] * (wr * J[j]) + J[kTfDim + i] * (wr * J[kTfDim + j]);
#pragma unroll
    for (int i = 0; i < kTfDim; ++i) T[(28 + i) * stride] = J[i] * o0 + J[kTfDim + i] * o1;
    T[35 * stride] = rho0;
}
// One edge at a linearisation: sims = the fifteen similarities of its direction (8 doubles each; the inverses for a backward edge).
// chi2 at the estimate (returned) and the 36 terms; the Huber kernel is always on.
__host__ __device__ __forceinline__ double tf_edge_terms(const double* sims, const PoseCam& C, double pcx, double pcy, double pcz, double ox, double oy,
                                                         double w, double delta, double* T, int stride) {
    const double scalar = 1.0 / (2.0 * kPoseNumericDelta);
    // the columns wait in the first fourteen term rows, so that the loop over d stays a loop on the device
#pragma unroll 1
    for (int d = 0; d < kTfDim; ++d) {
        double p0, p1, m0, m1;
        tf_edge_error(sims + 8 * (2 * d), C, pcx, pcy, pcz, ox, oy, w, p0, p1);
        tf_edge_error(sims + 8 * (2 * d + 1), C, pcx, pcy, pcz, ox, oy, w, m0, m1);
        T[d * stride] = scalar * (p0 - m0);
        T[(kTfDim + d) * stride] = scalar * (p1 - m1);
    }
    double J[2 * kTfDim];
#pragma unroll
    for (int i = 0; i < 2 * kTfDim; ++i) J[i] = T[i * stride];
    double e0, e1;
    const double chi2 = tf_edge_error(sims + 8 * (2 * kTfDim), C, pcx, pcy, pcz, ox, oy, w, e0, e1);
    double rho0, rho1;
    pose_huber(chi2, delta, rho0, rho1);
    tf_terms(J, e0, e1, w, rho0, rho1, T, stride);
    return chi2;
}

// ---- the Levenberg-Marquardt state of one problem (levenberg.hpp at N = 7)
struct TfWork {
    double est[8], bak[8];
    double sims[8 * kTfSims], invs[8 * kTfSims];   // of the last linearisation; entry 14 of both follows every tried estimate
    double sum[kTfTerms];        // the sums of the last linearisation: H (28), b (7), robust chi2
    double Lf[49];               // the Cholesky factor, row-major lower
    double x[kTfDim], y[kTfDim];
    double lambda, ni, current_chi, rho;
    int32_t ok2, qmax, iterations, rejected, go_on, end;
};

// push and solve: W.x is the step to try from W.bak
__host__ __device__ __forceinline__ void tf_lm_solve(TfWork& W) {
    for (int i = 0; i < 8; ++i) W.bak[i] = W.est[i];
    W.ok2 = lev_chol<kTfDim>(W.sum, W.sum + 28, W.lambda, W.Lf, W.y, W.x) ? 1 : 0;
}
// update: W.est becomes the tried estimate, entry 14 of sims / invs the tried estimate and its inverse
// (the host build's: see tf_perturb)
__host__ __device__ __forceinline__ void tf_lm_update(TfWork& W, bool fix_scale) {
    tf_oplus(W.x, fix_scale, W.bak, W.sims + 8 * 14);
    tf_inverse(W.sims + 8 * 14, W.invs + 8 * 14);
    for (int i = 0; i < 8; ++i) W.est[i] = W.sims[8 * 14 + i];
}
// iterations of round `round` (0, 1)
__host__ __device__ __forceinline__ int tf_round_iters(int round, int num_iter) { return round == 0 ? kTfFirstIters : num_iter; }
// round 1 (:139-153): the match stays iff both chi2 are below chi_sq (a NaN drops it); round 2 (:176-183): it is dropped iff chi_sq is below one
__host__ __device__ __forceinline__ bool tf_drop(int round, double chi_sq, double c12, double c21) {
    return round == 0 ? !(c12 < chi_sq && c21 < chi_sq) : (chi_sq < c12 || chi_sq < c21);
}

// the Sim3 outputs: rot (toRotationMatrix), trans, scale of est; world_to_1 (13) = est * Sim3(rot_2w, trans_2w, 1.0) (loop_detector.cc:404)
__host__ __device__ __forceinline__ void tf_world_to_1(const double* est, const double* pose_2, double* out13) {
    double b[8], m[8];
    pose_quat_from_rot(pose_2, b);
    b[4] = pose_2[9]; b[5] = pose_2[10]; b[6] = pose_2[11]; b[7] = 1.0;
    tf_mul(est, b, m);
    pose_rot_from_quat(m, out13);
    out13[9] = m[4]; out13[10] = m[5]; out13[11] = m[6]; out13[12] = m[7];
}

// ---- the arguments of the launches and of the host build
struct TfArgs {
    int P, n_cap, num_iter, fix_scale, num_levels;
    PoseCam cam;
    double chi_sq, delta;        // (double)chi_sq, (double)std::sqrt(chi_sq), the float root formed on the host
    float inv_sigma_sq_1[16], inv_sigma_sq_2[16];
    const int32_t* counts; const uint8_t* valid;
    const double* pos_w_1; const double* pos_w_2; const plp_keypoint* undist_1; const plp_keypoint* undist_2;
    const double* pose_1; const double* pose_2;          // rows of 15
    const double* rot_12; const double* trans_12; const float* scale_12;
    uint8_t* out_status; int32_t* out_num_valid; int32_t* out_num_inliers; double* out_rot_12; double* out_trans_12; double* out_scale_12;
    double* out_world_to_1; uint8_t* out_kept; int32_t* out_round_info; double* out_round_chi2;
    // buffers of the context (device entries): ranks -> slots; the chi2 of every edge's last evaluation ([2 k] forward, [2 k + 1] backward), then
    // per problem kTfCtxDoubles; per problem kTfCtxInts
    // ... and per rank the level of the match (1 = dropped) and two edge records of six doubles
    uint16_t* ctx_slot; double* ctx_chi2; int32_t* ctx_n; uint8_t* ctx_level; double* ctx_edge;
};
__host__ __device__ __forceinline__ int tf_count(const TfArgs& A, int p) {
    int c = A.n_cap;
    if (A.counts) c = A.counts[p] < c ? A.counts[p] : c;
    return c < 0 ? 0 : c;
}
__host__ __device__ __forceinline__ bool tf_observation(const TfArgs& A, size_t s) {
    return A.valid[s] != 0 && (unsigned)A.undist_1[s].octave < (unsigned)A.num_levels && (unsigned)A.undist_2[s].octave < (unsigned)A.num_levels;
}
// what a problem returns: the Sim3 est (the input's on the early return, where rot / trans are copied as given)
__host__ __device__ __forceinline__ void tf_write_result(const TfArgs& A, int p, const double* est, bool early, int n, int inliers) {
    double* r = A.out_rot_12 + (size_t)9 * p;
    double* t = A.out_trans_12 + (size_t)3 * p;
    if (early) {
        for (int i = 0; i < 9; ++i) r[i] = A.rot_12[(size_t)9 * p + i];
        for (int i = 0; i < 3; ++i) t[i] = A.trans_12[(size_t)3 * p + i];
        A.out_scale_12[p] = (double)A.scale_12[p];
    } else {
        pose_rot_from_quat(est, r);
        t[0] = est[4]; t[1] = est[5]; t[2] = est[6];
        A.out_scale_12[p] = est[7];
    }
    if (A.out_world_to_1) tf_world_to_1(est, A.pose_2 + (size_t)15 * p, A.out_world_to_1 + (size_t)13 * p);
    A.out_status[p] = early ? PLP_TRANSFORM_OPT_TOO_FEW_INLIERS : PLP_TRANSFORM_OPT_OK;
    A.out_num_valid[p] = n;
    A.out_num_inliers[p] = inliers;
}

hipError_t launch_transform_optimize(hipStream_t st, const TfArgs& A);

}  // namespace plp
