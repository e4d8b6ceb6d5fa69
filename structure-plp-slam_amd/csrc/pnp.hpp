// solve::pnp_solver (solve/pnp_solver.cc:36-866), one definition of the arithmetic for host and device (plp_pnp_ransac_* / plp_model_pnp_ransac_host,
// plp_model_epnp_host, plp_model_sym_jacobi_host, plp_model_lstsq6_host, plp_model_rot_from_abt_host, include/plp_front.h; DESIGN.md section 5,
// D14): EPnP's compute_pose, the inlier test of check_inliers and the threshold table of the constructor; the samples are ransac.hpp's at K = 4.  f64 with
// IEEE + - * / sqrt only, every sum left to right from 0.0, floats where the reference holds floats; translation units that include this file are
// compiled with -ffp-contract=off.  The four Eigen::JacobiSVD uses are one written-down one-sided (Hestenes) Jacobi, jacobi.hpp's hestenes().
//
// Everything here works on memory the caller names (PnpWork and the correspondence arrays): on the device that is LDS or a context buffer, reached
// with run-time indices, so that no kernel keeps an indexed array in registers; on the host it is the stack.  The sums over correspondences are
// `chain` functions, one accumulator each: the host runs them one after the other, the refit kernel one per lane.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/plp_front.h"
#include "jacobi.hpp"
#include "ransac.hpp"

namespace plp {

constexpr int kPnpMaxSlots = 8192;                    // n_cap limit of the entries (a rank fits 16 bits)
constexpr int kPnpCtxInts = 4;                        // per problem: num_matches, best count, best iteration, correspondences of the refit
constexpr int kPnpHypDoubles = 13;                    // per hypothesis: rot_cw (9), trans_cw (3), whether it exists
constexpr int kPnpCorrDoubles = 12;                   // per correspondence of the refit: pws (3), us (2), alphas (4), pcs (3)

// util::cos (util/trigonometric.h:42-73), float throughout; cvFloor is (int)v - ((int)v > v)
__host__ __device__ __forceinline__ float pnp_poly_cos(float v) {
    const float v2 = v * v;
    return 0.99940307f + v2 * (-0.49558072f + 0.03679168f * v2);
}
__host__ __device__ __forceinline__ float pnp_ref_cos(float v) {
    const float PI = 3.14159265358979f, PI_2 = PI / 2.0f, TWO_PI = 2.0f * PI, INV_TWO_PI = 1.0f / TWO_PI, THREE_PI_2 = 3.0f * PI_2;
    const float q = v * INV_TWO_PI;
    int fl = (int)q;
    fl -= (fl > q);
    v = v - (float)fl * TWO_PI;
    v = (0.0f < v) ? v : -v;
    if (v < PI_2) return pnp_poly_cos(v);
    if (v < PI) return -pnp_poly_cos(PI - v);
    if (v < THREE_PI_2) return -pnp_poly_cos(v - PI);
    return pnp_poly_cos(TWO_PI - v);
}
// max_cos_errors_ of a key point of level l (:47-51): util::cos((float)(scale_factors[l] * (1.0 * M_PI / 180.0)))
__host__ __device__ __forceinline__ float pnp_level_threshold(float scale_factor) {
    const double max_rad_error = 1.0 * 3.14159265358979323846 / 180.0;
    return pnp_ref_cos((float)((double)scale_factor * max_rad_error));
}

// ---- the small uses of the one-sided Jacobi (jacobi.hpp) that are EPnP's own
// Use 3 of D14: the minimum-norm least-squares solution of the 6 x k system whose columns are G's (column-major, destroyed), k = 3, 4, 5:
// x = sum over the columns j in ascending order with sigma_j > (k * 2^-52) * sigma_max of v_j * ((g_j . b) / |g_j|^2).  V: k * k, key: k.
__host__ __device__ __forceinline__ int lstsq6(double* G, const double* b, int k, double* V, double* key, double* x) {
    set_identity(V, k);
    const int sweeps = hestenes(G, V, 6, k);
    double smax = 0.0;
    for (int j = 0; j < k; ++j) {
        double n2 = 0.0;
        for (int i = 0; i < 6; ++i) n2 = n2 + G[j * 6 + i] * G[j * 6 + i];
        key[j] = n2;
        const double sg = __builtin_sqrt(n2);
        if (sg > smax) smax = sg;
    }
    const double thr = ((double)k * 0x1p-52) * smax;
    for (int i = 0; i < k; ++i) x[i] = 0.0;
    for (int j = 0; j < k; ++j) {
        if (!(__builtin_sqrt(key[j]) > thr)) continue;
        double gb = 0.0;
        for (int i = 0; i < 6; ++i) gb = gb + G[j * 6 + i] * b[i];
        const double coef = gb / key[j];
        for (int i = 0; i < k; ++i) x[i] = x[i] + V[j * k + i] * coef;
    }
    return sweeps;
}

// Use 4 of D14: R = U V^T of the 3 x 3 matrix Abt (row-major), with V's column of the smallest singular value negated when det(U V^T) < 0
// (:487-514).  u_j = g_j / sigma_j; where sigma_j is not > 0 the column of the smallest singular value is the cross product of the other two
// (in column order) and any other is zero.  G, V: 9 doubles of scratch each, key: 3, U: 9 (column-major).
__host__ __device__ __forceinline__ int rot_from_abt(const double* Abt, double* G, double* V, double* key, double* U, double* R) {
    for (int j = 0; j < 3; ++j)
        for (int i = 0; i < 3; ++i) G[j * 3 + i] = Abt[i * 3 + j];
    set_identity(V, 3);
    const int sweeps = hestenes(G, V, 3, 3);
    int jmin = 0;
    for (int j = 0; j < 3; ++j) {
        double n2 = 0.0;
        for (int i = 0; i < 3; ++i) n2 = n2 + G[j * 3 + i] * G[j * 3 + i];
        key[j] = jacobi_key(n2);
    }
    for (int j = 0; j < 3; ++j) {
        int rank = 0;
        for (int k = 0; k < 3; ++k) rank += jacobi_before(key[k], k, key[j], j) ? 1 : 0;
        if (rank == 2) jmin = j;
    }
    for (int j = 0; j < 3; ++j) {
        const double sg = __builtin_sqrt(key[j]);
        const bool have = sg > 0.0 && sg < __builtin_inf();
        for (int i = 0; i < 3; ++i) U[j * 3 + i] = have ? G[j * 3 + i] / sg : 0.0;
    }
    {
        const double sg = __builtin_sqrt(key[jmin]);
        if (!(sg > 0.0 && sg < __builtin_inf())) {
            const int a = jmin == 0 ? 1 : 0, b = jmin == 2 ? 1 : 2;
            const double* ua = U + a * 3; const double* ub = U + b * 3;
            U[jmin * 3 + 0] = ua[1] * ub[2] - ua[2] * ub[1];
            U[jmin * 3 + 1] = ua[2] * ub[0] - ua[0] * ub[2];
            U[jmin * 3 + 2] = ua[0] * ub[1] - ua[1] * ub[0];
        }
    }
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) R[3 * i + j] = (U[i] * V[j] + U[3 + i] * V[3 + j]) + U[6 + i] * V[6 + j];   // Abt_u.row(i) * Abt_v.row(j)^T (:495)
    const double det = R[0] * R[4] * R[8] + R[1] * R[5] * R[6] + R[2] * R[3] * R[7] - R[2] * R[4] * R[6] - R[1] * R[3] * R[8] - R[0] * R[5] * R[7];   // :499
    if (det < 0) {                                                  // :503-514
        for (int i = 0; i < 3; ++i) V[jmin * 3 + i] = -V[jmin * 3 + i];
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) R[3 * i + j] = (U[i] * V[j] + U[3 + i] * V[3 + j]) + U[6 + i] * V[6 + j];
    }
    return sweeps;
}

// ---- EPnP
// The scratch of one compute_pose (:230-290).  jac: the scratch of the small Jacobi uses; the 12 x 12 matrix is dead by the time the least
// squares and the rotation need it and not yet built when the control points do.
struct PnpWork {
    double cws[12];        // control points, world (:292-333)
    double s3[9];          // PW0tPW0 (:320)
    double ccinv[9];       // CC.inverse() (:347)
    double mtm[144];       // M^T M, row-major, both triangles (:242)
    double null[48];       // row i = row 11 - i of Ut (:244): the eigenvectors of the four smallest eigenvalues, smallest first
    double L[60];          // L_6x10 (:667-702)
    double rho[6];         // :704-712
    double betas[12];      // Betas[1..3] (:252)
    double ccs[12];        // control points, camera (:377-394)
    double gnA[24], gnB[6], gnX[4], gnA1[4], gnA2[4];   // gauss_newton / qr_solve (:728-866)
    double pc0[3], pw0[3], abt[9];   // estimate_R_and_t (:440-485)
    double Rs[27], ts[9], err[3];    // Rs[1..3], ts[1..3], rep_errors[1..3] (:252-265)
    double vals[3], ut3[9], u3[9];
    int sweeps[8];         // PW0tPW0, MtM, the three least-squares systems, the three Abt
};
__host__ __device__ __forceinline__ double* pnp_jac_G(PnpWork& W) { return W.mtm; }
__host__ __device__ __forceinline__ double* pnp_jac_V(PnpWork& W) { return W.mtm + 36; }
__host__ __device__ __forceinline__ double* pnp_jac_key(PnpWork& W) { return W.mtm + 72; }

// add_correspondence (:204-228): false = skipped (bearing(2) == 0)
__host__ __device__ __forceinline__ bool pnp_add_correspondence(const double* pos_w, const double* bearing, double* pw, double* us, int& sign) {
    if (bearing[2] == 0) return false;
    pw[0] = pos_w[0]; pw[1] = pos_w[1]; pw[2] = pos_w[2];
    us[0] = bearing[0] / bearing[2];
    us[1] = bearing[1] / bearing[2];
    sign = 0.0 < bearing[2] ? 1 : -1;
    return true;
}

__host__ __device__ __forceinline__ double pnp_dot3(const double* a, const double* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }   // :415
__host__ __device__ __forceinline__ double pnp_dist2(const double* a, const double* b) {                                                   // :410
    return (a[0] - b[0]) * (a[0] - b[0]) + (a[1] - b[1]) * (a[1] - b[1]) + (a[2] - b[2]) * (a[2] - b[2]);
}

// the chains: sums over the nc correspondences in their order, one accumulator each.  stride: doubles between two correspondences.
__host__ __device__ __forceinline__ double pnp_sum_chain(const double* x, int stride, int nc) {          // :296-302, :447-457
    double acc = 0;
    for (int i = 0; i < nc; ++i) acc += x[(size_t)i * stride];
    return acc;
}
__host__ __device__ __forceinline__ double pnp_pw0tpw0_chain(const double* pws, int stride, int nc, const double* c, int a, int b) {   // :312-320
    double acc = 0.0;
    for (int i = 0; i < nc; ++i) acc = acc + (pws[(size_t)i * stride + a] - c[a]) * (pws[(size_t)i * stride + b] - c[b]);
    return acc;
}
// entry (row parity, col) of the two rows fill_M writes for a correspondence (:363-375), fx_ = fy_ = 1.0f, cx_ = cy_ = 0.0f (pnp_solver.h:166)
__host__ __device__ __forceinline__ double pnp_m(const double* as, double u, double v, int parity, int col) {
    const float fx = 1.0f, fy = 1.0f, cx = 0.0f, cy = 0.0f;
    const int i = col / 3, k = col - 3 * i;
    if (parity == 0) return k == 0 ? as[i] * fx : k == 1 ? 0.0 : as[i] * (cx - u);
    return k == 0 ? 0.0 : k == 1 ? as[i] * fy : as[i] * (cy - v);
}
__host__ __device__ __forceinline__ double pnp_mtm_chain(const double* alphas, const double* us, int stride, int nc, int a, int b) {   // :237-242
    double acc = 0.0;
    for (int i = 0; i < nc; ++i) {
        const double* as = alphas + (size_t)i * stride;
        const double u = us[(size_t)i * stride], v = us[(size_t)i * stride + 1];
        acc = acc + pnp_m(as, u, v, 0, a) * pnp_m(as, u, v, 0, b);
        acc = acc + pnp_m(as, u, v, 1, a) * pnp_m(as, u, v, 1, b);
    }
    return acc;
}
__host__ __device__ __forceinline__ double pnp_abt_chain(const double* pcs, const double* pws, int stride, int nc, const double* pc0, const double* pw0, int j,
                                                         int k) {   // :474-485
    double acc = 0.0;
    for (int i = 0; i < nc; ++i) acc += (pcs[(size_t)i * stride + j] - pc0[j]) * (pws[(size_t)i * stride + k] - pw0[k]);
    return acc;
}
// one term of reprojection_error (:426-434)
__host__ __device__ __forceinline__ double pnp_reproj_term(const double* pw, double u, double v, const double* R, const double* t) {
    const float fx = 1.0f, fy = 1.0f, cx = 0.0f, cy = 0.0f;
    const double Xc = pnp_dot3(R, pw) + t[0];
    const double Yc = pnp_dot3(R + 3, pw) + t[1];
    const double inv_Zc = 1.0 / (pnp_dot3(R + 6, pw) + t[2]);
    const double ue = cx + fx * Xc * inv_Zc;
    const double ve = cy + fy * Yc * inv_Zc;
    return __builtin_sqrt((u - ue) * (u - ue) + (v - ve) * (v - ve));
}
__host__ __device__ __forceinline__ double pnp_reproj_chain(const double* pws, const double* us, int stride, int nc, const double* R, const double* t) {   // :420-438
    double sum2 = 0.0;
    for (int i = 0; i < nc; ++i) sum2 += pnp_reproj_term(pws + (size_t)i * stride, us[(size_t)i * stride], us[(size_t)i * stride + 1], R, t);
    return sum2 / (double)(unsigned)nc;
}

// choose_control_points behind its sums (:304-332): W.cws[0..2] holds the sum of the points, W.s3 is filled by the caller after pnp_centroid
__host__ __device__ __forceinline__ void pnp_centroid(PnpWork& W, int nc) {
    for (int j = 0; j < 3; ++j) W.cws[j] /= (double)(unsigned)nc;
}
__host__ __device__ __forceinline__ void pnp_control_points(PnpWork& W, int nc) {
    W.sweeps[0] = sym_jacobi(W.s3, 3, pnp_jac_G(W), pnp_jac_V(W), pnp_jac_key(W), W.vals, W.ut3);
    for (int r = 0; r < 3; ++r) {                                   // D14 item 2a: the sign of a singular vector is the routine's own affair; the component of
        double* v = W.ut3 + 3 * r;                                  // largest magnitude (the first of equals) is made non-negative
        int big = 0;
        for (int i = 1; i < 3; ++i)
            if (__builtin_fabs(v[i]) > __builtin_fabs(v[big])) big = i;
        if (v[big] < 0)
            for (int i = 0; i < 3; ++i) v[i] = -v[i];
    }
    for (int i = 1; i < 4; ++i) {
        const double k = __builtin_sqrt(W.vals[i - 1] / (double)(unsigned)nc);
        for (int j = 0; j < 3; ++j) W.cws[3 * i + j] = W.cws[j] + k * W.ut3[3 * (i - 1) + j];
    }
    // compute_barycentric_coordinates (:337-347).  CC.inverse(): the cofactors in cyclic form, times 1 / det, det along the first column
    double* CC = W.u3;
    for (int i = 0; i < 3; ++i)
        for (int j = 1; j < 4; ++j) CC[3 * i + (j - 1)] = W.cws[3 * j + i] - W.cws[i];
    double* cof = W.ut3;
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) {
            const int r1 = (r + 1) % 3, r2 = (r + 2) % 3, c1 = (c + 1) % 3, c2 = (c + 2) % 3;
            cof[3 * r + c] = CC[3 * r1 + c1] * CC[3 * r2 + c2] - CC[3 * r1 + c2] * CC[3 * r2 + c1];
        }
    const double det = (cof[0] * CC[0] + cof[3] * CC[3]) + cof[6] * CC[6];
    const double invdet = 1.0 / det;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) W.ccinv[3 * i + j] = cof[3 * j + i] * invdet;
}
// the loop body of compute_barycentric_coordinates (:349-360)
__host__ __device__ __forceinline__ void pnp_alphas(const PnpWork& W, const double* pi, double* a) {
    for (int j = 0; j < 3; ++j)
        a[1 + j] = W.ccinv[3 * j] * (pi[0] - W.cws[0]) + W.ccinv[3 * j + 1] * (pi[1] - W.cws[1]) + W.ccinv[3 * j + 2] * (pi[2] - W.cws[2]);
    a[0] = 1.0f - a[1] - a[2] - a[3];
}

// entry (a, b), a <= b, of the upper triangle of M^T M as the index of its chain, 0 .. 77, and back
__host__ __device__ __forceinline__ void pnp_mtm_pair(int e, int& a, int& b) {
    a = 0;
    while (e >= 12 - a) { e -= 12 - a; ++a; }
    b = a + e;
}

// qr_solve (:748-866), A row-major 6 x 4 (destroyed), b destroyed; X keeps its values on the early return
__host__ __device__ __forceinline__ void pnp_qr_solve(double* pA, double* pb, double* pX, double* A1, double* A2) {
    const int nr = 6, nc = 4;
    double* ppAkk = pA;
    for (int k = 0; k < nc; ++k) {
        double* ppAik = ppAkk;
        double eta = __builtin_fabs(*ppAik);
        for (int i = k + 1; i < nr; ++i) {
            const double elt = __builtin_fabs(*ppAik);
            if (eta < elt) eta = elt;
            ppAik += nc;
        }
        if (eta == 0) {
            A1[k] = A2[k] = 0.0;
            return;
        }
        ppAik = ppAkk;
        double sum = 0.0;
        const double inv_eta = 1.0 / eta;
        for (int i = k; i < nr; ++i) {
            *ppAik *= inv_eta;
            sum += *ppAik * *ppAik;
            ppAik += nc;
        }
        double sigma = __builtin_sqrt(sum);
        if (*ppAkk < 0) sigma = -sigma;
        *ppAkk += sigma;
        A1[k] = sigma * *ppAkk;
        A2[k] = -eta * sigma;
        for (int j = k + 1; j < nc; ++j) {
            double* q = ppAkk;
            double sum2 = 0.0;
            for (int i = k; i < nr; i++) {
                sum2 += *q * q[j - k];
                q += nc;
            }
            const double tau = sum2 / A1[k];
            q = ppAkk;
            for (int i = k; i < nr; ++i) {
                q[j - k] -= tau * *q;
                q += nc;
            }
        }
        ppAkk += nc + 1;
    }
    double* ppAjj = pA;                                             // b <- Qt b
    for (int j = 0; j < nc; ++j) {
        double* ppAij = ppAjj;
        double tau = 0;
        for (int i = j; i < nr; i++) {
            tau += *ppAij * pb[i];
            ppAij += nc;
        }
        tau /= A1[j];
        ppAij = ppAjj;
        for (int i = j; i < nr; ++i) {
            pb[i] -= tau * *ppAij;
            ppAij += nc;
        }
        ppAjj += nc + 1;
    }
    pX[nc - 1] = pb[nc - 1] / A2[nc - 1];                           // X = R-1 b
    for (int i = nc - 2; i >= 0; --i) {
        double* ppAij = pA + i * nc + (i + 1);
        double sum = 0;
        for (int j = i + 1; j < nc; ++j) {
            sum += *ppAij * pX[j];
            ppAij++;
        }
        pX[i] = (pb[i] - sum) / A2[i];
    }
}

// gauss_newton (:728-746) with compute_A_and_b_gauss_newton (:714-726); X is zero before the first iteration (D14)
__host__ __device__ __forceinline__ void pnp_gauss_newton(PnpWork& W, double* betas) {
    const double* L = W.L;
    for (int i = 0; i < 4; ++i) W.gnX[i] = 0.0;
    for (int k = 0; k < 5; ++k) {
        for (int i = 0; i < 6; ++i) {
            const double* l = L + 10 * i;
            double* A = W.gnA + 4 * i;
            A[0] = 2 * l[0] * betas[0] + l[1] * betas[1] + l[3] * betas[2] + l[6] * betas[3];
            A[1] = l[1] * betas[0] + 2 * l[2] * betas[1] + l[4] * betas[2] + l[7] * betas[3];
            A[2] = l[3] * betas[0] + l[4] * betas[1] + 2 * l[5] * betas[2] + l[8] * betas[3];
            A[3] = l[6] * betas[0] + l[7] * betas[1] + l[8] * betas[2] + 2 * l[9] * betas[3];
            W.gnB[i] = W.rho[i] - (l[0] * betas[0] * betas[0] + l[1] * betas[0] * betas[1] + l[2] * betas[1] * betas[1] + l[3] * betas[0] * betas[2] +
                                   l[4] * betas[1] * betas[2] + l[5] * betas[2] * betas[2] + l[6] * betas[0] * betas[3] + l[7] * betas[1] * betas[3] +
                                   l[8] * betas[2] * betas[3] + l[9] * betas[3] * betas[3]);
        }
        pnp_qr_solve(W.gnA, W.gnB, W.gnX, W.gnA1, W.gnA2);
        for (int i = 0; i < 4; ++i) betas[i] += W.gnX[i];
    }
}

// dv[i][j][k] of compute_L_6x10 (:669-687): pair j of the control points (0,1) (0,2) (0,3) (1,2) (1,3) (2,3)
__host__ __device__ __forceinline__ double pnp_dv(const PnpWork& W, int i, int j, int k) {
    const int a = j < 3 ? 0 : j < 5 ? 1 : 2, b = j < 3 ? j + 1 : j < 5 ? j - 1 : 3;
    return W.null[12 * i + 3 * a + k] - W.null[12 * i + 3 * b + k];
}
__host__ __device__ __forceinline__ double pnp_dv_dot(const PnpWork& W, int i1, int i2, int j) {
    return pnp_dv(W, i1, j, 0) * pnp_dv(W, i2, j, 0) + pnp_dv(W, i1, j, 1) * pnp_dv(W, i2, j, 1) + pnp_dv(W, i1, j, 2) * pnp_dv(W, i2, j, 2);
}

// compute_L_6x10, compute_rho, the three find_betas_approx_* and gauss_newton (:249-263 without compute_R_and_t; :558-712) from W.null and W.cws
// D14 item 2a: with at most four correspondences M has at most eight rows, the four vectors of W.null span nothing but null space, and which
// basis of it a routine returns is its own affair.  The basis used is made a function of the span alone: column c of the projector
// sum_k n_k n_k^T, c = 0 .. 3, orthogonalised against the earlier ones (modified Gram-Schmidt) and scaled to unit length.  tmp: 48 doubles.
__host__ __device__ __forceinline__ void pnp_canonical_null(PnpWork& W, double* tmp) {
    for (int c = 0; c < 4; ++c) {
        double* w = tmp + 12 * c;
        for (int i = 0; i < 12; ++i) {
            double acc = 0.0;
            for (int k = 0; k < 4; ++k) acc = acc + W.null[12 * k + i] * W.null[12 * k + c];
            w[i] = acc;
        }
        for (int p = 0; p < c; ++p) {
            const double* b = tmp + 12 * p;
            double d = 0.0;
            for (int i = 0; i < 12; ++i) d = d + b[i] * w[i];
            for (int i = 0; i < 12; ++i) w[i] = w[i] - d * b[i];
        }
        double n2 = 0.0;
        for (int i = 0; i < 12; ++i) n2 = n2 + w[i] * w[i];
        const double nrm = __builtin_sqrt(n2);
        for (int i = 0; i < 12; ++i) w[i] = w[i] / nrm;
    }
    for (int i = 0; i < 48; ++i) W.null[i] = tmp[i];
}

__host__ __device__ __forceinline__ void pnp_betas(PnpWork& W, int nc) {
    if (nc <= 4) pnp_canonical_null(W, W.L);                        // W.L is not yet built
    for (int i = 0; i < 6; ++i) {
        double* l = W.L + 10 * i;
        l[0] = pnp_dv_dot(W, 0, 0, i);
        l[1] = 2.0f * pnp_dv_dot(W, 0, 1, i);
        l[2] = pnp_dv_dot(W, 1, 1, i);
        l[3] = 2.0f * pnp_dv_dot(W, 0, 2, i);
        l[4] = 2.0f * pnp_dv_dot(W, 1, 2, i);
        l[5] = pnp_dv_dot(W, 2, 2, i);
        l[6] = 2.0f * pnp_dv_dot(W, 0, 3, i);
        l[7] = 2.0f * pnp_dv_dot(W, 1, 3, i);
        l[8] = 2.0f * pnp_dv_dot(W, 2, 3, i);
        l[9] = pnp_dv_dot(W, 3, 3, i);
    }
    W.rho[0] = pnp_dist2(W.cws, W.cws + 3);
    W.rho[1] = pnp_dist2(W.cws, W.cws + 6);
    W.rho[2] = pnp_dist2(W.cws, W.cws + 9);
    W.rho[3] = pnp_dist2(W.cws + 3, W.cws + 6);
    W.rho[4] = pnp_dist2(W.cws + 3, W.cws + 9);
    W.rho[5] = pnp_dist2(W.cws + 6, W.cws + 9);
    double* G = pnp_jac_G(W);
    double* V = pnp_jac_V(W);
    double* key = pnp_jac_key(W);
    double* x = W.gnB;                                              // b4 / b3 / b5: free until gauss_newton
    {   // find_betas_approx_1 (:558-588): columns 0, 1, 3, 6
        double* betas = W.betas;
        for (int i = 0; i < 6; ++i) { G[i] = W.L[10 * i]; G[6 + i] = W.L[10 * i + 1]; G[12 + i] = W.L[10 * i + 3]; G[18 + i] = W.L[10 * i + 6]; }
        W.sweeps[2] = lstsq6(G, W.rho, 4, V, key, x);
        if (x[0] < 0) {
            betas[0] = __builtin_sqrt(-x[0]);
            betas[1] = -x[1] / betas[0];
            betas[2] = -x[2] / betas[0];
            betas[3] = -x[3] / betas[0];
        } else {
            betas[0] = __builtin_sqrt(x[0]);
            betas[1] = x[1] / betas[0];
            betas[2] = x[2] / betas[0];
            betas[3] = x[3] / betas[0];
        }
    }
    {   // find_betas_approx_2 (:593-626): columns 0, 1, 2
        double* betas = W.betas + 4;
        for (int i = 0; i < 6; ++i) { G[i] = W.L[10 * i]; G[6 + i] = W.L[10 * i + 1]; G[12 + i] = W.L[10 * i + 2]; }
        W.sweeps[3] = lstsq6(G, W.rho, 3, V, key, x);
        if (x[0] < 0) {
            betas[0] = __builtin_sqrt(-x[0]);
            betas[1] = (x[2] < 0) ? __builtin_sqrt(-x[2]) : 0.0;
        } else {
            betas[0] = __builtin_sqrt(x[0]);
            betas[1] = (x[2] > 0) ? __builtin_sqrt(x[2]) : 0.0;
        }
        if (x[1] < 0) betas[0] = -betas[0];
        betas[2] = 0.0;
        betas[3] = 0.0;
    }
    {   // find_betas_approx_3 (:631-665): columns 0 .. 4
        double* betas = W.betas + 8;
        for (int i = 0; i < 6; ++i)
            for (int j = 0; j < 5; ++j) G[6 * j + i] = W.L[10 * i + j];
        W.sweeps[4] = lstsq6(G, W.rho, 5, V, key, x);
        if (x[0] < 0) {
            betas[0] = __builtin_sqrt(-x[0]);
            betas[1] = (x[2] < 0) ? __builtin_sqrt(-x[2]) : 0.0;
        } else {
            betas[0] = __builtin_sqrt(x[0]);
            betas[1] = (x[2] > 0) ? __builtin_sqrt(x[2]) : 0.0;
        }
        if (x[1] < 0) betas[0] = -betas[0];
        betas[2] = x[3] / betas[0];
        betas[3] = 0.0;
    }
    for (int a = 0; a < 3; ++a) pnp_gauss_newton(W, W.betas + 4 * a);
}

// compute_ccs (:377-394) for approximation a = 0, 1, 2 (Betas[a + 1])
__host__ __device__ __forceinline__ void pnp_ccs(PnpWork& W, int a) {
    const double* betas = W.betas + 4 * a;
    for (int i = 0; i < 12; ++i) W.ccs[i] = 0.0;
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j)
            for (int k = 0; k < 3; ++k) W.ccs[3 * j + k] += betas[i] * W.null[12 * i + 3 * j + k];
}
// the loop body of compute_pcs (:400-406)
__host__ __device__ __forceinline__ void pnp_pcs(const PnpWork& W, const double* a, double* pc) {
    for (int j = 0; j < 3; ++j) pc[j] = a[0] * W.ccs[j] + a[1] * W.ccs[3 + j] + a[2] * W.ccs[6 + j] + a[3] * W.ccs[9 + j];
}
// the test of solve_for_sign (:524) on pcs_[2] and signs_[0] of the first correspondence
__host__ __device__ __forceinline__ bool pnp_sign_flips(double pcs2, int sign0) { return (pcs2 < 0.0 && sign0 > 0) || (pcs2 > 0.0 && sign0 < 0); }
// estimate_R_and_t behind its sums (:458-462, :487-518) and the slot of approximation a: W.pc0 / W.pw0 hold the sums, W.abt is filled by the
// caller after pnp_centroids
__host__ __device__ __forceinline__ void pnp_centroids(PnpWork& W, int nc) {
    for (int j = 0; j < 3; ++j) {
        W.pc0[j] /= (double)(unsigned)nc;
        W.pw0[j] /= (double)(unsigned)nc;
    }
}
__host__ __device__ __forceinline__ void pnp_R_and_t(PnpWork& W, int a) {
    double* R = W.Rs + 9 * a;
    double* t = W.ts + 3 * a;
    W.sweeps[5 + a] = rot_from_abt(W.abt, pnp_jac_G(W), pnp_jac_V(W), pnp_jac_key(W), W.u3, R);
    t[0] = W.pc0[0] - pnp_dot3(R, W.pw0);
    t[1] = W.pc0[1] - pnp_dot3(R + 3, W.pw0);
    t[2] = W.pc0[2] - pnp_dot3(R + 6, W.pw0);
}
// the choice of N (:267-275), as an index 0 .. 2 into Rs / ts / err
__host__ __device__ __forceinline__ int pnp_choose(const PnpWork& W) {
    int N = 0;
    if (W.err[1] < W.err[0]) N = 1;
    if (W.err[2] < W.err[N]) N = 2;
    return N;
}

// compute_pose up to M^T M (:232-242) for nc >= 1 correspondences held with `stride` doubles between them, one after the other
__host__ __device__ __forceinline__ void pnp_pose_front(PnpWork& W, const double* pws, const double* us, double* alphas, int stride, int nc) {
    for (int j = 0; j < 3; ++j) W.cws[j] = pnp_sum_chain(pws + j, stride, nc);
    pnp_centroid(W, nc);
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) W.s3[3 * a + b] = pnp_pw0tpw0_chain(pws, stride, nc, W.cws, a < b ? a : b, a < b ? b : a);
    pnp_control_points(W, nc);
    for (int i = 0; i < nc; ++i) pnp_alphas(W, pws + (size_t)i * stride, alphas + (size_t)i * stride);
    for (int a = 0; a < 12; ++a)
        for (int b = a; b < 12; ++b) W.mtm[12 * a + b] = W.mtm[12 * b + a] = pnp_mtm_chain(alphas, us, stride, nc, a, b);
}
// use 2 of D14 on the host: W.null from W.mtm
__host__ __device__ __forceinline__ void pnp_null_space(PnpWork& W, double* G, double* V) {
    for (int j = 0; j < 12; ++j)
        for (int i = 0; i < 12; ++i) G[12 * j + i] = W.mtm[12 * i + j];
    set_identity(V, 12);
    W.sweeps[1] = hestenes(G, V, 12, 12);
    double key[12];
    for (int j = 0; j < 12; ++j) {
        double n2 = 0.0;
        for (int i = 0; i < 12; ++i) n2 = n2 + G[12 * j + i] * G[12 * j + i];
        key[j] = jacobi_key(n2);
    }
    for (int j = 0; j < 12; ++j) {
        int rank = 0;
        for (int k = 0; k < 12; ++k) rank += jacobi_before(key[k], k, key[j], j) ? 1 : 0;
        if (rank >= 8)
            for (int i = 0; i < 12; ++i) W.null[12 * (11 - rank) + i] = V[12 * j + i];
    }
}
// compute_pose from Ut on (:246-289); returns the index of the chosen approximation
__host__ __device__ __forceinline__ int pnp_pose_back(PnpWork& W, const double* pws, const double* us, const double* alphas, double* pcs, int stride, int nc,
                                                      int sign0) {
    pnp_betas(W, nc);
    for (int a = 0; a < 3; ++a) {                                   // compute_R_and_t (:543-553)
        pnp_ccs(W, a);
        for (int i = 0; i < nc; ++i) pnp_pcs(W, alphas + (size_t)i * stride, pcs + (size_t)i * stride);
        if (pnp_sign_flips(pcs[2], sign0)) {                        // :526-539
            for (int i = 0; i < 12; ++i) W.ccs[i] = -W.ccs[i];
            for (int i = 0; i < nc; ++i)
                for (int j = 0; j < 3; ++j) pcs[(size_t)i * stride + j] = -pcs[(size_t)i * stride + j];
        }
        for (int j = 0; j < 3; ++j) {
            W.pc0[j] = pnp_sum_chain(pcs + j, stride, nc);
            W.pw0[j] = pnp_sum_chain(pws + j, stride, nc);
        }
        pnp_centroids(W, nc);
        for (int j = 0; j < 3; ++j)
            for (int k = 0; k < 3; ++k) W.abt[3 * j + k] = pnp_abt_chain(pcs, pws, stride, nc, W.pc0, W.pw0, j, k);
        pnp_R_and_t(W, a);
        W.err[a] = pnp_reproj_chain(pws, us, stride, nc, W.Rs + 9 * a, W.ts + 3 * a);
    }
    return pnp_choose(W);
}

// the loop body of check_inliers (:162-177): the float threshold widened to double
__host__ __device__ __forceinline__ bool pnp_inlier(const double* R, const double* t, const double* pos_w, const double* bearing, float thr, bool never) {
    const double x = ((R[0] * pos_w[0] + R[1] * pos_w[1]) + R[2] * pos_w[2]) + t[0];
    const double y = ((R[3] * pos_w[0] + R[4] * pos_w[1]) + R[5] * pos_w[2]) + t[1];
    const double z = ((R[6] * pos_w[0] + R[7] * pos_w[1]) + R[8] * pos_w[2]) + t[2];
    const double cos = ((x * bearing[0] + y * bearing[1]) + z * bearing[2]) / __builtin_sqrt((x * x + y * y) + z * z);
    return !never && (double)thr < cos;
}

struct PnpArgs {
    int P, n_cap, iters, min_num_inliers, recompute, num_levels;
    unsigned long long seed;
    float thr[16];                                                  // max_cos_errors_ per level
    const uint8_t* valid; const double* bearing; const double* pos_w; const int32_t* octave; const int32_t* counts; const int32_t* samples;
    uint8_t* out_status; int32_t* out_num_matches; double* out_rot_cw; double* out_trans_cw; int32_t* out_num_inliers; int32_t* out_best_iter;
    uint8_t* out_inliers; int32_t* out_hyp_inliers;
    int32_t* ctx;            // DEVICE, P x kPnpCtxInts
    uint16_t* ctx_slot;      // DEVICE, P x n_cap: slot of rank k
    double* ctx_hyp;         // DEVICE, P x kPnpHypDoubles x iters
    double* ctx_corr;        // DEVICE, P x n_cap x kPnpCorrDoubles: the correspondences of the refit
    double* ctx_pose;        // DEVICE, P x 12: the refit's pose
    int32_t* ctx_sign;       // DEVICE, P: signs_[0] of the refit
};
hipError_t launch_pnp_ransac(hipStream_t st, const PnpArgs& A);     // pnp_kernels.hip: five launches, the first error

}  // namespace plp
