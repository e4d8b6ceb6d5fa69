// g2o's Levenberg-Marquardt step (OptimizationAlgorithmLevenberg::solve) and the dense (H + lambda I) x = b solve, one definition for
// pose_opt.hpp (N = 6), transform_opt.hpp (N = 7) and local_ba.hpp (its accept / reject step and end rule).
// f64 with IEEE + - * / sqrt only, in the order written; translation units that include this file are compiled with -ffp-contract=off.
//
// The functions are templates over the solver's own state (PoseWork, TfWork, LaShared) and read its fields by name: lambda, ni, current_chi,
// rho, qmax, rejected, go_on; the dense ones also sum (H upper triangle row-major, b, robust chi2), x, ok2, est, bak.
#pragma once
#include <hip/hip_runtime.h>

namespace plp {

constexpr int kLevMaxTries = 10;         // g2o's maxTrialsAfterFailure
constexpr double kLevDblMax = 1.7976931348623157e308;

// why an optimize() ended (out_trial_info[..][3], out_round_info[..][3]); 0 = it was not run
enum { kLevEndIterations = 1, kLevEndTries = 2, kLevEndRhoZero = 3 };

// (i, j), i <= j, of an N x N upper triangle held row-major
template <int N> __host__ __device__ __forceinline__ int lev_h_index(int i, int j) { return i * N - (i * (i - 1)) / 2 + (j - i); }

// (H + lambda I) x = b by Cholesky (Lf: the factor, row-major lower); false = a pivot that is not positive and finite (x is then zero)
template <int N> __host__ __device__ __forceinline__ bool lev_chol(const double* H, const double* b, double lambda, double* Lf, double* y, double* x) {
    for (int i = 0; i < N; ++i) x[i] = 0.0;
    for (int j = 0; j < N; ++j) {
        double s = H[lev_h_index<N>(j, j)] + lambda;
        for (int k = 0; k < j; ++k) s = s - Lf[N * j + k] * Lf[N * j + k];
        if (!(s > 0.0) || s > kLevDblMax) return false;
        const double d = __builtin_sqrt(s);
        Lf[N * j + j] = d;
        for (int i = j + 1; i < N; ++i) {
            double v = H[lev_h_index<N>(j, i)];
            for (int k = 0; k < j; ++k) v = v - Lf[N * i + k] * Lf[N * j + k];
            Lf[N * i + j] = v / d;
        }
    }
    for (int i = 0; i < N; ++i) {
        double v = b[i];
        for (int k = 0; k < i; ++k) v = v - Lf[N * i + k] * y[k];
        y[i] = v / Lf[N * i + i];
    }
    for (int i = N - 1; i >= 0; --i) {
        double v = y[i];
        for (int k = i + 1; k < N; ++k) v = v - Lf[N * k + i] * x[k];
        x[i] = v / Lf[N * i + i];
    }
    return true;
}

// solve() after buildSystem of one N-dimensional vertex: w.sum holds the linearisation at w.est
template <int N, class W> __host__ __device__ __forceinline__ void lev_begin(W& w, int iteration) {
    w.current_chi = w.sum[N * (N + 1) / 2 + N];
    if (iteration == 0) {                       // computeLambdaInit: tau max |H_jj|
        double m = 0.0;
        for (int j = 0; j < N; ++j) {
            const double d = __builtin_fabs(w.sum[lev_h_index<N>(j, j)]);
            m = d > m ? d : m;
        }
        w.lambda = 1e-5 * m;
        w.ni = 2.0;
    }
    w.qmax = 0;
    w.rho = 0.0;
}

// The decision after the errors at the tried estimate were summed to temp_sum: ok = the solve succeeded, scale = computeScale's sum
// x . (lambda x + b).  Sets go_on (the do-while repeats).  kept() runs when the step is kept, undo() restores what a rejection has to.
template <class W, class Kept, class Undo>
__host__ __device__ __forceinline__ void lev_decide(W& w, bool ok, double temp_sum, double scale, Kept kept, Undo undo) {
    const double temp_chi = ok ? temp_sum : kLevDblMax;
    scale = scale + 1e-3;
    w.rho = (w.current_chi - temp_chi) / scale;
    const bool finite = temp_chi >= -kLevDblMax && temp_chi <= kLevDblMax;
    if (w.rho > 0.0 && finite) {
        const double v = 2.0 * w.rho - 1.0;
        double alpha = 1.0 - (v * v) * v;
        alpha = alpha < 2.0 / 3.0 ? alpha : 2.0 / 3.0;
        const double f = alpha > 1.0 / 3.0 ? alpha : 1.0 / 3.0;
        w.lambda = w.lambda * f;
        w.ni = 2.0;
        w.current_chi = temp_chi;
        kept();
    } else {
        w.lambda = w.lambda * w.ni;
        w.ni = w.ni * 2.0;
        undo();
        w.rejected += 1;
    }
    w.qmax += 1;
    w.go_on = (w.rho < 0.0 && w.qmax < kLevMaxTries) ? 1 : 0;
}
// ... of one N-dimensional vertex whose estimate is E doubles: the scale from w.x and w.sum; a rejection puts w.bak back
template <int N, int E, class W> __host__ __device__ __forceinline__ void lev_decide_vertex(W& w, double temp_sum) {
    double scale = 0.0;
    for (int j = 0; j < N; ++j) scale = scale + w.x[j] * (w.lambda * w.x[j] + w.sum[N * (N + 1) / 2 + j]);
    lev_decide(w, w.ok2 != 0, temp_sum, scale, [] {}, [&w] { for (int i = 0; i < E; ++i) w.est[i] = w.bak[i]; });
}

// after the do-while: whether the iteration returns Terminate
template <class W> __host__ __device__ __forceinline__ int lev_end(const W& w) {
    return w.qmax == kLevMaxTries ? kLevEndTries : w.rho == 0.0 ? kLevEndRhoZero : 0;
}

}  // namespace plp
