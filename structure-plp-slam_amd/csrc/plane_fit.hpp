// Planar_Mapping_module (planar_mapping_module.cc): estimate_plane_SVD (:735-771), the two RANSAC loops around it
// (estimate_plane_sequential_RANSAC :412-591 behind the gate of create_new_plane :359, update_plane_via_RANSAC :593-733) and refine_points
// (:954-1004), one definition of the arithmetic for host and device (plp_plane_ransac_* / plp_model_plane_ransac_host, plp_model_plane_fit_host,
// plp_model_plane_draw_host, plp_plane_refine_points_*, include/plp_front.h).  f64 with IEEE + - * / sqrt only;
// translation units that include this file are compiled with -ffp-contract=off.  estimate_plane_sequential_Graph_cut_RANSAC (:1006-) needs a
// third-party library and is not part of this.
//
// A sum over a list x_0 .. x_{m-1} has one shape everywhere (D19 item 4): 64 partial chains, chain j over the k = j, j + 64, j + 128, ... in
// ascending order from 0.0, then one chain over j = 0 .. 63 from 0.0.  A `Team` runs it: the host's team of one forms the 64 partials one after
// the other, a wave forms partial j in lane j (plane_kernels.hip).  Nothing else of a fit depends on who runs it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/plp_front.h"
#include "jacobi.hpp"
#include "ransac.hpp"

namespace plp {

constexpr int kPlaneMaxSlots = 8192;                  // n_cap limit of the entries (a rank fits 16 bits)
constexpr int kPlaneMaxIters = 1024;
constexpr int kPlaneHypDoubles = 12;                  // per hypothesis: sample equation (4), residual, refit equation (4), error, inliers, ok
constexpr int kPlaneWorkDoubles = 42;                 // plane_normal's work: A, G, V (9 each), key, vals (3 each), Ut (9)
constexpr double kPlaneMax = 1.7976931348623157e308;  // std::numeric_limits<double>::max() (:439)

// who may be sampled (:452, :623-628) and who is scanned for inliers (:480, :656)
__host__ __device__ __forceinline__ bool plane_live(uint8_t f) { return (f & PLP_PLANE_LM_ERASED) == 0; }
__host__ __device__ __forceinline__ bool plane_eligible(int mode, uint8_t f) {
    return plane_live(f) && (mode == PLP_PLANE_CREATE || (f & PLP_PLANE_LM_OWNED) != 0);
}

// the number of samples of a hypothesis: POINTS_PER_RANSAC (:449), or the smallest m with !((double)m < (double)n * 0.8) (:620)
__host__ __device__ __forceinline__ int plane_sample_size(int mode, int n, int points_per_ransac) {
    if (mode == PLP_PLANE_CREATE) return points_per_ransac;
    const double lim = (double)n * 0.8;
    int m = (int)lim;                                 // n <= 8192: exact, at most one below the answer
    while ((double)m < lim) ++m;
    return m;
}

// Plane::set_equation's _abs_n (landmark_plane.cc:106) and Plane::calculate_distance (:118-123)
__host__ __device__ __forceinline__ double plane_abs_n(const double eq[4]) { return __builtin_sqrt((eq[0] * eq[0] + eq[1] * eq[1]) + eq[2] * eq[2]); }
__host__ __device__ __forceinline__ double plane_dot(const double eq[4], const double x[3]) { return (eq[0] * x[0] + eq[1] * x[1]) + eq[2] * x[2]; }
__host__ __device__ __forceinline__ double plane_distance(const double eq[4], double abs_n, const double x[3]) {
    return __builtin_fabs((plane_dot(eq, x) + eq[3]) / abs_n);
}

// The unit normal of the scatter matrix C = (c00, c01, c02, c11, c12, c22): the eigenvector of the smallest eigenvalue by sym_jacobi (jacobi.hpp)
// at n = 3, Ut row 2, divided by its norm when that is > 0 (normalized()), the component of largest magnitude made positive (ties: the lowest
// index).  W: kPlaneWorkDoubles of memory reached with run-time indices (LDS on the device).  Returns the sweeps that rotated.
__host__ __device__ __forceinline__ int plane_normal(const double C[6], double* W, double nrm[3]) {
    double* A = W;
    A[0] = C[0]; A[1] = C[1]; A[2] = C[2];
    A[3] = C[1]; A[4] = C[3]; A[5] = C[4];
    A[6] = C[2]; A[7] = C[4]; A[8] = C[5];
    const int sweeps = sym_jacobi(A, 3, W + 9, W + 18, W + 27, W + 30, W + 33);
    double v0 = W[33 + 6], v1 = W[33 + 7], v2 = W[33 + 8];
    const double n2 = (v0 * v0 + v1 * v1) + v2 * v2;
    if (n2 > 0.0) {
        const double nn = __builtin_sqrt(n2);
        v0 = v0 / nn; v1 = v1 / nn; v2 = v2 / nn;
    }
    double big = v0, mag = __builtin_fabs(v0);
    if (__builtin_fabs(v1) > mag) { big = v1; mag = __builtin_fabs(v1); }
    if (__builtin_fabs(v2) > mag) { big = v2; mag = __builtin_fabs(v2); }
    if (big < 0.0) { v0 = -v0; v1 = -v1; v2 = -v2; }
    nrm[0] = v0; nrm[1] = v1; nrm[2] = v2;
    return sweeps;
}

// The host's team: the 64 partials one after the other, then their chain.
struct PlaneHostTeam {
    double work[kPlaneWorkDoubles];
    // f(j, part): adds chain j's terms to part[0 .. N-1], which start at 0.0
    template <int N, class F> void sum64(F f, double (&tot)[N]) {
        for (int i = 0; i < N; ++i) tot[i] = 0.0;
        for (int j = 0; j < 64; ++j) {
            double part[N];
            for (int i = 0; i < N; ++i) part[i] = 0.0;
            f(j, part);
            for (int i = 0; i < N; ++i) tot[i] = tot[i] + part[i];
        }
    }
    bool leader() const { return true; }
    double* jacobi_work() { return work; }
    double share(double v) const { return v; }
    int share(int v) const { return v; }
};

// estimate_plane_SVD (:735-771) over the list get(k, x), k = 0 .. m-1 (get returns false for an entry that names no point: the fit is then
// void, residual DBL_MAX and equation 0).  D19 item 3: centroid = sum / m; scatter of the centred coordinates; normal; d = -(n . centroid);
// residual = fabs(sqrt(sum ((n . x_k) + d)^2) / m).
template <class Team, class Get>
__host__ __device__ __forceinline__ void plane_fit(Team& T, Get get, int m, double eq[4], double& residual, int& sweeps) {
    double s[4];                                      // x, y, z and the number of void entries
    T.template sum64<4>([&](int j, double (&part)[4]) {
        for (int k = j; k < m; k += 64) {
            double x[3];
            if (get(k, x)) { part[0] = part[0] + x[0]; part[1] = part[1] + x[1]; part[2] = part[2] + x[2]; }
            else part[3] = part[3] + 1.0;
        }
    }, s);
    if (s[3] != 0.0) {
        eq[0] = 0.0; eq[1] = 0.0; eq[2] = 0.0; eq[3] = 0.0;
        residual = kPlaneMax;
        sweeps = 0;
        return;
    }
    const double md = (double)m;
    const double c[3] = {s[0] / md, s[1] / md, s[2] / md};
    double C[6];
    T.template sum64<6>([&](int j, double (&part)[6]) {
        for (int k = j; k < m; k += 64) {
            double x[3];
            get(k, x);
            const double a = x[0] - c[0], b = x[1] - c[1], g = x[2] - c[2];
            part[0] = part[0] + a * a; part[1] = part[1] + a * b; part[2] = part[2] + a * g;
            part[3] = part[3] + b * b; part[4] = part[4] + b * g; part[5] = part[5] + g * g;
        }
    }, C);
    double nrm[3] = {0.0, 0.0, 0.0};
    int sw = 0;
    if (T.leader()) sw = plane_normal(C, T.jacobi_work(), nrm);
    nrm[0] = T.share(nrm[0]); nrm[1] = T.share(nrm[1]); nrm[2] = T.share(nrm[2]);
    sweeps = T.share(sw);
    eq[0] = nrm[0]; eq[1] = nrm[1]; eq[2] = nrm[2];
    eq[3] = -((nrm[0] * c[0] + nrm[1] * c[1]) + nrm[2] * c[2]);
    double r[1];
    T.template sum64<1>([&](int j, double (&part)[1]) {
        for (int k = j; k < m; k += 64) {
            double x[3];
            get(k, x);
            const double e = plane_dot(eq, x) + eq[3];
            part[0] = part[0] + e * e;
        }
    }, r);
    residual = __builtin_fabs(__builtin_sqrt(r[0]) / md);
}

// what every problem of a call shares
struct PlaneArgs {
    int mode, P, n_cap, iters, points_per_ransac, min_points_before_ransac, m_cap;
    double inliers_ratio_thr;
    unsigned long long seed;
    const int32_t* counts; const double* pos_w; const uint8_t* flags; const double* dist_thresh; const double* error_thresh;
    const double* best_error_in; const double* equation_in; const int32_t* samples;
    uint8_t* out_status; uint8_t* out_flags; double* out_equation; double* out_best_error; int32_t* out_best_iter; int32_t* out_last_iter;
    int32_t* out_num_inliers; uint8_t* out_inliers; double* out_hyp_residual; int32_t* out_hyp_inliers; double* out_hyp_error;
    double* ctx_hyp;                                  // DEVICE, P x iters x kPlaneHypDoubles: the hypotheses
};
hipError_t launch_plane_ransac(hipStream_t st, const PlaneArgs& A);   // plane_kernels.hip: two launches, the first error

// Where the function returns before its loop (:359, :423-436, :597-606; no eligible slot: D19 item 2), else PLP_PLANE_OK.  n = lms.size().
__host__ __device__ __forceinline__ int plane_early_status(const PlaneArgs& A, int n, int n_eligible, int& flags) {
    flags = 0;
    if (A.mode == PLP_PLANE_CREATE && n < A.min_points_before_ransac) { flags = PLP_PLANE_FLAG_GATED; return PLP_PLANE_TOO_FEW_POINTS; }
    if (n == 0) return PLP_PLANE_TOO_FEW_POINTS;
    if (n < A.points_per_ransac) { flags = A.mode == PLP_PLANE_UPDATE ? PLP_PLANE_FLAG_INVALID : 0; return PLP_PLANE_TOO_FEW_POINTS; }
    if (n_eligible == 0) return PLP_PLANE_NO_ELIGIBLE;
    return PLP_PLANE_OK;
}

// the gate of step [3] (:498-499, :670)
__host__ __device__ __forceinline__ bool plane_refit_gate(const PlaneArgs& A, int n, int num_inliers) {
    if (A.mode == PLP_PLANE_UPDATE) return num_inliers >= A.points_per_ransac;
    const double inlier_ratio = (double)num_inliers / (double)n;
    return inlier_ratio > A.inliers_ratio_thr && num_inliers >= A.points_per_ransac;
}

// The reference's loop over the hypotheses' records: the running minimum, the acceptances and CREATE's break.
// residual(i), tried(i), error(i) read record i.
struct PlaneReplay {
    double best_error, plane_error;                   // the local best_error; Plane::_best_error as the loop leaves it
    int best_iter, last_iter;                         // the owner of best_inliers_list (-1: !best_found); the last iteration that ran
    bool last_refit;                                  // the plane's equation is the last iteration's refit, not its sample fit
};
template <class FR, class FT, class FE>
__host__ __device__ __forceinline__ PlaneReplay plane_replay(int mode, int iters, double best_error_in, double error_thresh, FR residual, FT tried, FE error) {
    PlaneReplay R;
    R.best_error = mode == PLP_PLANE_CREATE ? kPlaneMax : best_error_in;   // :439, :609
    R.plane_error = R.best_error; R.best_iter = -1; R.last_iter = -1; R.last_refit = false;
    for (int i = 0; i < iters; ++i) {
        const double res = residual(i);
        if (res < R.best_error) R.best_error = res;   // :465, :641
        R.plane_error = res; R.last_iter = i; R.last_refit = false;   // :469-474, :645-650
        if (!tried(i)) continue;
        const double err = error(i);
        if (err < R.best_error) {                     // :505, :675
            R.best_error = err;
            R.plane_error = err; R.last_refit = true; R.best_iter = i;
            if (mode == PLP_PLANE_CREATE && err < error_thresh) break;   // :526
        }
    }
    return R;
}

// what follows the loop up to step [4] (:545-562, :698-702)
__host__ __device__ __forceinline__ int plane_late_status(int mode, const PlaneReplay& R, double error_thresh, int& flags) {
    flags = 0;
    if (R.best_iter < 0) { flags = mode == PLP_PLANE_UPDATE ? PLP_PLANE_FLAG_NEED_REFINEMENT : 0; return PLP_PLANE_NOT_FOUND; }
    if (R.best_error > error_thresh) { flags = mode == PLP_PLANE_UPDATE ? PLP_PLANE_FLAG_NEED_REFINEMENT : 0; return PLP_PLANE_ERROR_ABOVE_THRESHOLD; }
    return PLP_PLANE_OK;
}

// refine_points (:968-991) for one landmark of an active plane: whether x moved
__host__ __device__ __forceinline__ bool plane_refine_point(const double eq[4], double dist_thresh, double x[3]) {
    const double n2 = (eq[0] * eq[0] + eq[1] * eq[1]) + eq[2] * eq[2];
    const double abs_n = __builtin_sqrt(n2);
    const double dist_old = plane_distance(eq, abs_n, x);                                   // :976
    if (!(__builtin_fabs(dist_old) > 0.0)) return false;                                    // :977
    double nn[3] = {eq[0], eq[1], eq[2]};                                                   // get_normal().normalized() (:982)
    if (n2 > 0.0) { nn[0] = eq[0] / abs_n; nn[1] = eq[1] / abs_n; nn[2] = eq[2] / abs_n; }
    const double y[3] = {x[0] - nn[0] * dist_old, x[1] - nn[1] * dist_old, x[2] - nn[2] * dist_old};   // :983
    const double dist_new = plane_distance(eq, abs_n, y);                                   // :984
    if (!(dist_new < dist_thresh && dist_new < dist_old)) return false;                     // :985-986
    x[0] = y[0]; x[1] = y[1]; x[2] = y[2];
    return true;
}

struct PlaneRefineArgs {
    int M, NP;
    double* pos_w; const int32_t* lm_plane; const uint8_t* flags; const double* equation; const uint8_t* active; const double* dist_thresh;
    uint8_t* out_changed;
};
hipError_t launch_plane_refine_points(hipStream_t st, const PlaneRefineArgs& A);   // plane_kernels.hip

// landmark i of the list: the skips of :960-973, then the point
__host__ __device__ __forceinline__ void plane_refine_landmark(const PlaneRefineArgs& A, int i) {
    const int pl = A.lm_plane[i];
    bool changed = false;
    if (pl >= 0 && pl < A.NP && A.active[pl] != 0 && plane_live(A.flags[i]) && (A.flags[i] & PLP_PLANE_LM_OWNED) != 0) {
        const double eq[4] = {A.equation[4 * (size_t)pl], A.equation[4 * (size_t)pl + 1], A.equation[4 * (size_t)pl + 2], A.equation[4 * (size_t)pl + 3]};
        double x[3] = {A.pos_w[3 * (size_t)i], A.pos_w[3 * (size_t)i + 1], A.pos_w[3 * (size_t)i + 2]};
        changed = plane_refine_point(eq, A.dist_thresh[0], x);
        if (changed) { A.pos_w[3 * (size_t)i] = x[0]; A.pos_w[3 * (size_t)i + 1] = x[1]; A.pos_w[3 * (size_t)i + 2] = x[2]; }
    }
    A.out_changed[i] = changed ? 1 : 0;
}

}  // namespace plp
