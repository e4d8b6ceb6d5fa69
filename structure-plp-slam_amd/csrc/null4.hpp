// The null vector of a 4 x 4 matrix, one definition for host and device: what solve::triangulator::triangulate
// (solve/triangulator.h:105-119) takes from Eigen's JacobiSVD as the last column of V.  A cyclic one-sided (Hestenes) Jacobi in f64 on the
// columns of U = A, V = I, with IEEE + - * / sqrt only, every sum left to right, no libm call; translation units that include this file are
// compiled with -ffp-contract=off.  All 32 coefficients are named by compile-time constants, so that on the device they stay in registers.
#pragma once
#include <hip/hip_runtime.h>

namespace plp {

constexpr int kNull4SweepLimit = 30;                  // sweeps that rotate; scene matrices need at most 6 (tests/test_keypoint_pairs_cpu.py)
constexpr double kNull4SkipTol = 0x1p-100;            // a pair is left alone unless gamma^2 > (2^-100 alpha) beta, i.e. |cos| > 2^-50

// One pair (P, Q), P < Q, of the sweep: alpha = |u_P|^2, beta = |u_Q|^2, gamma = u_P . u_Q; the rotation that makes the two columns
// orthogonal is applied to U and V.  Returns whether it rotated.
template <int P, int Q>
__host__ __device__ __forceinline__ bool null4_rotate(double (&U)[16], double (&V)[16]) {
    const double alpha = ((U[P] * U[P] + U[4 + P] * U[4 + P]) + U[8 + P] * U[8 + P]) + U[12 + P] * U[12 + P];
    const double beta = ((U[Q] * U[Q] + U[4 + Q] * U[4 + Q]) + U[8 + Q] * U[8 + Q]) + U[12 + Q] * U[12 + Q];
    const double gamma = ((U[P] * U[Q] + U[4 + P] * U[4 + Q]) + U[8 + P] * U[8 + Q]) + U[12 + P] * U[12 + Q];
    if (!(gamma * gamma > (kNull4SkipTol * alpha) * beta)) return false;   // the fixed skip test; a NaN or an infinite norm skips too
    const double zeta = (beta - alpha) / (2.0 * gamma);
    const double root = __builtin_sqrt(1.0 + zeta * zeta);
    const double t = zeta >= 0.0 ? 1.0 / (zeta + root) : -1.0 / (root - zeta);
    const double c = 1.0 / __builtin_sqrt(1.0 + t * t);
    const double s = c * t;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const double up = U[4 * r + P], uq = U[4 * r + Q];
        U[4 * r + P] = c * up - s * uq;
        U[4 * r + Q] = s * up + c * uq;
        const double vp = V[4 * r + P], vq = V[4 * r + Q];
        V[4 * r + P] = c * vp - s * vq;
        V[4 * r + Q] = s * vp + c * vq;
    }
    return true;
}

// A row-major.  v = the column of V whose column of A V has the smallest squared norm (ties: the lowest index), unit length up to rounding,
// sign unspecified.  *sweeps = the number of sweeps that rotated; kNull4SweepLimit = the limit was reached.
__host__ __device__ __forceinline__ void null_vector4(const double A[16], double v[4], int* sweeps) {
    double U[16], V[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        U[i] = A[i];
        V[i] = (i % 5 == 0) ? 1.0 : 0.0;
    }
    int n = 0;
    while (n < kNull4SweepLimit) {
        bool any = null4_rotate<0, 1>(U, V);           // the column pairs in a fixed order
        any |= null4_rotate<0, 2>(U, V);
        any |= null4_rotate<0, 3>(U, V);
        any |= null4_rotate<1, 2>(U, V);
        any |= null4_rotate<1, 3>(U, V);
        any |= null4_rotate<2, 3>(U, V);
        if (!any) break;
        ++n;
    }
    const double n0 = ((U[0] * U[0] + U[4] * U[4]) + U[8] * U[8]) + U[12] * U[12];
    const double n1 = ((U[1] * U[1] + U[5] * U[5]) + U[9] * U[9]) + U[13] * U[13];
    const double n2 = ((U[2] * U[2] + U[6] * U[6]) + U[10] * U[10]) + U[14] * U[14];
    const double n3 = ((U[3] * U[3] + U[7] * U[7]) + U[11] * U[11]) + U[15] * U[15];
    int best = 0;
    double nb = n0;
    if (n1 < nb) { best = 1; nb = n1; }
    if (n2 < nb) { best = 2; nb = n2; }
    if (n3 < nb) { best = 3; nb = n3; }
#pragma unroll
    for (int r = 0; r < 4; ++r) v[r] = best == 0 ? V[4 * r] : best == 1 ? V[4 * r + 1] : best == 2 ? V[4 * r + 2] : V[4 * r + 3];
    *sweeps = n;
}

}  // namespace plp
