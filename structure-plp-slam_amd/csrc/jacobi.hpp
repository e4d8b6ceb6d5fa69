// The one-sided (Hestenes) Jacobi that stands for every Eigen::JacobiSVD use of the solvers, one definition for host and device (pnp.hpp,
// essential.hpp, two_view.hpp, plane_fit.hpp).  f64 with IEEE + - * / sqrt only, every sum left to right
// from 0.0; translation units that include this file are compiled with -ffp-contract=off.
#pragma once
#include <hip/hip_runtime.h>

namespace plp {

constexpr int kJacobiSweepLimit = 60;                 // sweeps that rotate; scene matrices need far fewer (tests/test_pnp_solver_cpu.py)
constexpr double kJacobiSkipTol = 0x1p-100;           // a column pair is left alone unless (g_p . g_q)^2 > 2^-100 |g_p|^2 |g_q|^2: |cos| <= 4 eps

// The round-robin ("circle") schedule over N columns, N even: in round r = 0 .. N-2 column N-1 meets column r and every other column j meets
// (2r - j) mod (N-1).  The pairs of a round are disjoint, so their rotations commute exactly.
__host__ __device__ __forceinline__ int jacobi_partner(int j, int r, int N) {
    if (j == N - 1) return r;
    if (j == r) return N - 1;
    int q = (2 * r - j) % (N - 1);
    if (q < 0) q += N - 1;
    return q;
}

// c, s of the rotation that makes columns p < q orthogonal, from alpha = |g_p|^2, beta = |g_q|^2, gamma = g_p . g_q; false = the pair is left alone
// (the fixed skip test; a NaN skips too)
__host__ __device__ __forceinline__ bool hestenes_cs(double alpha, double beta, double gamma, double& c, double& s) {
    if (!(gamma * gamma > kJacobiSkipTol * (alpha * beta))) return false;
    const double zeta = (beta - alpha) / (2.0 * gamma);
    const double root = __builtin_sqrt(1.0 + zeta * zeta);
    const double t = zeta >= 0.0 ? 1.0 / (zeta + root) : -1.0 / (root - zeta);
    c = 1.0 / __builtin_sqrt(1.0 + t * t);
    s = c * t;
    return true;
}

// G: m x n, V: n x n, both column-major (column j at G + j * m, V + j * n); V must hold the identity.  Sweeps of the schedule above (an odd n
// gets a dummy last column whose pairs are skipped) until one rotates nothing.  Returns the number of sweeps that rotated; kJacobiSweepLimit =
// the limit was reached.  Afterwards A V = G with orthogonal columns: sigma_j = |g_j|, right vectors = columns of V, left = g_j / sigma_j.
__host__ __device__ __forceinline__ int hestenes(double* G, double* V, int m, int n) {
    const int N = n + (n & 1);
    int sweeps = 0;
    while (sweeps < kJacobiSweepLimit) {
        bool any = false;
        for (int r = 0; r < N - 1; ++r)
            for (int p = 0; p < n; ++p) {
                const int q = jacobi_partner(p, r, N);
                if (q >= n || q < p) continue;           // the dummy, or the pair is taken from its lower column
                double* gp = G + p * m; double* gq = G + q * m;
                double alpha = 0.0, beta = 0.0, gamma = 0.0;
                for (int i = 0; i < m; ++i) { alpha = alpha + gp[i] * gp[i]; beta = beta + gq[i] * gq[i]; gamma = gamma + gp[i] * gq[i]; }
                double c, s;
                if (!hestenes_cs(alpha, beta, gamma, c, s)) continue;
                any = true;
                for (int i = 0; i < m; ++i) {
                    const double a = gp[i], b = gq[i];
                    gp[i] = c * a - s * b;
                    gq[i] = s * a + c * b;
                }
                double* vp = V + p * n; double* vq = V + q * n;
                for (int i = 0; i < n; ++i) {
                    const double a = vp[i], b = vq[i];
                    vp[i] = c * a - s * b;
                    vq[i] = s * a + c * b;
                }
            }
        if (!any) break;
        ++sweeps;
    }
    return sweeps;
}

// the ordering key of a column: |g_j|^2, a NaN counts as +inf; rank j = the number of columns that come before j when the keys are sorted
// descending, equal keys by ascending column
__host__ __device__ __forceinline__ double jacobi_key(double n2) { return n2 == n2 ? n2 : __builtin_inf(); }
__host__ __device__ __forceinline__ bool jacobi_before(double key_k, int k, double key_j, int j) { return key_k > key_j || (key_k == key_j && k < j); }

__host__ __device__ __forceinline__ void set_identity(double* V, int n) {
    for (int i = 0; i < n * n; ++i) V[i] = 0.0;
    for (int i = 0; i < n; ++i) V[i * n + i] = 1.0;
}

// Uses 1 and 2 of D14: A n x n row-major, symmetric positive semi-definite.  vals[r] = the r-th largest singular value |g_j|, Ut row r
// (row-major n x n) = the column of V that belongs to it.  G, V: n * n doubles of scratch each, key: n.
__host__ __device__ __forceinline__ int sym_jacobi(const double* A, int n, double* G, double* V, double* key, double* vals, double* Ut) {
    for (int j = 0; j < n; ++j)
        for (int i = 0; i < n; ++i) G[j * n + i] = A[i * n + j];
    set_identity(V, n);
    const int sweeps = hestenes(G, V, n, n);
    for (int j = 0; j < n; ++j) {
        double n2 = 0.0;
        for (int i = 0; i < n; ++i) n2 = n2 + G[j * n + i] * G[j * n + i];
        key[j] = jacobi_key(n2);
    }
    for (int j = 0; j < n; ++j) {
        int rank = 0;
        for (int k = 0; k < n; ++k) rank += jacobi_before(key[k], k, key[j], j) ? 1 : 0;
        vals[rank] = __builtin_sqrt(key[j]);
        for (int i = 0; i < n; ++i) Ut[rank * n + i] = V[j * n + i];
    }
    return sweeps;
}

}  // namespace plp
