// optimize::local_bundle_adjuster_extended_line::optimize (optimize/local_bundle_adjuster_extended_line.cc:70-674), one definition for host and
// device (plp_local_ba_lines_* / plp_model_local_ba_lines*_host, include/plp_front.h) on top of local_ba.hpp (D17): the
// 4-DoF line vertex in orthonormal representation (g2o/line3d.h), the binary line edge with both numeric Jacobian blocks
// (g2o/se3/reproj_edge_line3d_orthonormal.h), the 4 x 4 marginalised blocks beside the 3 x 3 ones and the line half of the outlier schedule.
// The point half of every step is local_ba.hpp's own function, called as it is, so that a problem without a line edge takes exactly D17's
// arithmetic; only the damped solve is restated here (ll_solve_system), because the lines' subtractions stand in its middle.  f64 with IEEE
// + - * / sqrt only, in the order written; translation units that include this file are compiled with -ffp-contract=off.
//
// As local_ba.hpp the steps are written once over a team `P` of lanes; every coefficient is owned by one lane that adds its terms in the defined
// order, and all state between the steps lives in the context's buffers.
#pragma once
#include "line3d.hpp"
#include "local_ba.hpp"

namespace plp {

// rows of the line-edge table: D15's 28 terms of the pose block, the line block H_ll (upper triangle row-major) and b_l, W = Jp^T Omega Jl (6 x 4),
// Y = W Hll^-1; during a linearisation rows W .. W + 39 first hold the 20 perturbed errors
enum { kLlRowRho = 27, kLlRowLn = 28, kLlRowW = 42, kLlRowY = 66, kLlRowChi = 90, kLlRowObs = 91, kLlEdgeRows = 96 };
// rows of the line table: both estimate buffers, the eight perturbed copies of the kept estimate, the sums, the inverse, the update
enum { kLlLnEst = 0, kLlLnPert = 12, kLlLnH = 60, kLlLnB = 70, kLlLnInv = 74, kLlLnX = 84, kLlLnPart = 88, kLlLnRows = 89 };
constexpr int kLlPoseDoubles = 84 * kLaMaxFree;      // the twelve perturbed poses of every active free key frame

struct LlArgs {
    LaArgs p;
    int LL, TL, kl_stride, num_levels_lsd;
    float inv_sigma_sq_lsd[16];
    const plp_keyline* keylines; const int32_t* kl_counts; const double* pluecker; const uint8_t* line_erased;
    const int32_t* obs_offsets_lines; const int32_t* obs_kf_lines; const int32_t* obs_idx_lines;
    uint8_t* out_line_role; double* out_pluecker; uint8_t* out_outlier_lines;
};                                                      // the lines' state lies behind the G problems' state of local_ba.hpp in p's three buffers

__host__ __device__ __forceinline__ size_t ll_doubles(int LL, int TL) { return (size_t)kLlEdgeRows * TL + (size_t)kLlLnRows * LL + kLlPoseDoubles; }
__host__ __device__ __forceinline__ size_t ll_ints(int TL) { return (size_t)3 * TL; }
__host__ __device__ __forceinline__ size_t ll_bytes(int LL, int TL) { return (size_t)TL + (size_t)2 * LL; }

struct LlOff { size_t et, ln, pp, e_l, e_kf, byp, lvl, role, act; };
struct LlView {
    double* d; int32_t* i; uint8_t* b; const LlOff* o;
    __host__ __device__ __forceinline__ double* et() const { return d + o->et; }
    __host__ __device__ __forceinline__ double* ln() const { return d + o->ln; }
    __host__ __device__ __forceinline__ double* pp() const { return d + o->pp; }
    __host__ __device__ __forceinline__ int32_t* e_l() const { return i + o->e_l; }
    __host__ __device__ __forceinline__ int32_t* e_kf() const { return i + o->e_kf; }
    __host__ __device__ __forceinline__ int32_t* byp() const { return i + o->byp; }
    __host__ __device__ __forceinline__ uint8_t* lvl() const { return b + o->lvl; }
    __host__ __device__ __forceinline__ uint8_t* role() const { return b + o->role; }
    __host__ __device__ __forceinline__ uint8_t* act() const { return b + o->act; }
};
__host__ __device__ __forceinline__ void ll_offsets(const LlArgs& A, int g, LlOff& O) {
    O.et = la_doubles(A.p.F, A.p.L, A.p.T) * A.p.G + ll_doubles(A.LL, A.TL) * g;
    O.ln = O.et + (size_t)kLlEdgeRows * A.TL;
    O.pp = O.ln + (size_t)kLlLnRows * A.LL;
    O.e_l = la_ints(A.p.T) * A.p.G + ll_ints(A.TL) * g;
    O.e_kf = O.e_l + A.TL;
    O.byp = O.e_kf + A.TL;
    O.lvl = la_bytes(A.p.F, A.p.L, A.p.T) * A.p.G + ll_bytes(A.LL, A.TL) * g;
    O.role = O.lvl + A.TL;
    O.act = O.role + A.LL;
}
__host__ __device__ __forceinline__ LlView ll_view(const LlArgs& A, const LlOff& O) {
    LlView W;
    W.d = A.p.ctx_d; W.i = A.p.ctx_i; W.b = A.p.ctx_b; W.o = &O;
    return W;
}
__host__ __device__ __forceinline__ double& ll_e(const LlView& W, int t, int row) { return W.et()[(size_t)t * kLlEdgeRows + row]; }
__host__ __device__ __forceinline__ double& ll_l(const LlView& W, int l, int row) { return W.ln()[(size_t)l * kLlLnRows + row]; }

// the lines' dimensions under the names la_run reads: L lines, T entries of their observation list
struct LlDims { int L, T; const int32_t* obs_offsets; };
struct LlDimsView { const int& L; const int& T; const int32_t* obs_offsets; };

struct LlShared {
    LaShared s;
    LlOff O; int LL, TL;
    int32_t cntl[kLaMaxFree], aoffl[kLaMaxFree], acntl[kLaMaxFree];
    int32_t nlna, anyl, iters;
    double delta_lines;         // the line edges' Huber delta, sqrt(chi_sq_2D) whatever the set-up (:403)
};

// (i, j), i <= j, of the 4 x 4 upper triangle; the inverse is read through it in both orders
__host__ __device__ __forceinline__ int ll_h4(int i, int j) { return i <= j ? lev_h_index<4>(i, j) : lev_h_index<4>(j, i); }

// ---- the line vertex: Line3D::oplus (g2o/line3d.h:171-186), L = (m, d), v = (the rotation's quaternion vector, the angle of W).  out may not alias L.
__host__ __device__ __forceinline__ void ll_oplus(const double* L, const double* v, double* out) {
    // toOrthonormal (:137-157)
    const double m0 = L[0], m1 = L[1], m2 = L[2], d0 = L[3], d1 = L[4], d2 = L[5];
    const double dnorm = __builtin_sqrt((d0 * d0 + d1 * d1) + d2 * d2), mnorm = __builtin_sqrt((m0 * m0 + m1 * m1) + m2 * m2);
    const double wn = 1.0 / __builtin_sqrt(dnorm * dnorm + mnorm * mnorm);
    const double W00 = mnorm * wn, W01 = (-dnorm) * wn, W10 = dnorm * wn, W11 = mnorm * wn;
    const double mn = 1.0 / mnorm, dn = 1.0 / dnorm;
    const double c0 = m1 * d2 - m2 * d1, c1 = m2 * d0 - m0 * d2, c2 = m0 * d1 - m1 * d0;
    const double cn = 1.0 / __builtin_sqrt((c0 * c0 + c1 * c1) + c2 * c2);
    const double U[9] = {m0 * mn, d0 * dn, c0 * cn, m1 * mn, d1 * dn, c1 * cn, m2 * mn, d2 * dn, c2 * cn};
    // the update: W from the angle, U from the quaternion (sqrt(1 - |v|^2), v) normalised; a negative radicand is NaN
    double sn, cs;
    pose_sincos(v[3], sn, cs);
    double q[4] = {v[0], v[1], v[2], __builtin_sqrt(1.0 - ((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]))};
    const double n2 = ((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3];
    if (n2 > 0.0) {
        const double n = __builtin_sqrt(n2);
        q[0] = q[0] / n; q[1] = q[1] / n; q[2] = q[2] / n; q[3] = q[3] / n;
    }
    double Ru[9];
    pose_rot_from_quat(q, Ru);
    // the two products; of U Ru only the two columns fromOrthonormal reads, of W Wu only its first column
    double u0[3], u1[3];
    _Pragma("unroll") for (int i = 0; i < 3; ++i) {
        u0[i] = (U[3 * i] * Ru[0] + U[3 * i + 1] * Ru[3]) + U[3 * i + 2] * Ru[6];
        u1[i] = (U[3 * i] * Ru[1] + U[3 * i + 1] * Ru[4]) + U[3 * i + 2] * Ru[7];
    }
    const double w0 = W00 * cs + W01 * sn, w1 = W10 * cs + W11 * sn;
    // fromOrthonormal with its normalize(), and oplus's own
    _Pragma("unroll") for (int i = 0; i < 3; ++i) { out[i] = u0[i] * w0; out[3 + i] = u1[i] * w1; }
    _Pragma("unroll 1") for (int pass = 0; pass < 2; ++pass) {
        const double n = 1.0 / __builtin_sqrt((out[3] * out[3] + out[4] * out[4]) + out[5] * out[5]);
        _Pragma("unroll") for (int i = 0; i < 6; ++i) out[i] = out[i] * n;
    }
}

// ---- the line edge's depth test: depth_is_positive_via_endpoints_trimming (reproj_edge_line3d_orthonormal.h:97-177) at (est, L)
__host__ __device__ __forceinline__ bool ll_depth_ok(const double* est, const PoseCam& C, const double* L, double xs, double ys, double xe, double ye) {
    double R[9];
    pose_rot_from_quat(est, R);
    const double tx = est[4], ty = est[5], tz = est[6];
    // cam_project as pose_line_error forms it (D15 item 2)
    double top[3];
    _Pragma("unroll") for (int i = 0; i < 3; ++i) {
        double m0, m1, m2;
        if (i == 0) { m0 = (-tz) * R[3] + ty * R[6]; m1 = (-tz) * R[4] + ty * R[7]; m2 = (-tz) * R[5] + ty * R[8]; }
        else if (i == 1) { m0 = tz * R[0] + (-tx) * R[6]; m1 = tz * R[1] + (-tx) * R[7]; m2 = tz * R[2] + (-tx) * R[8]; }
        else { m0 = (-ty) * R[0] + tx * R[3]; m1 = (-ty) * R[1] + tx * R[4]; m2 = (-ty) * R[2] + tx * R[5]; }
        top[i] = ((((R[3 * i] * L[0] + R[3 * i + 1] * L[1]) + R[3 * i + 2] * L[2]) + m0 * L[3]) + m1 * L[4]) + m2 * L[5];
    }
    const double l1 = C.fy * top[0], l2 = C.fx * top[1], l3 = (C.k20 * top[0] + C.k21 * top[1]) + C.k22 * top[2];
    const double den = l1 * l1 + l2 * l2;
    // P = _cam_matrix [rot_cw | trans_cw], three terms per coefficient, the zero entries of the camera matrix included (D25)
    double Pm[12];
    _Pragma("unroll") for (int c = 0; c < 4; ++c) {
        const double a0 = c < 3 ? R[c] : tx, a1 = c < 3 ? R[3 + c] : ty, a2 = c < 3 ? R[6 + c] : tz;
        Pm[c] = (C.fx * a0 + 0.0 * a1) + C.cx * a2;
        Pm[4 + c] = (0.0 * a0 + C.fy * a1) + C.cy * a2;
        Pm[8 + c] = (0.0 * a0 + 0.0 * a1) + 1.0 * a2;
    }
    const double M[16] = {0.0, -L[2], L[1], L[3],
                          L[2], 0.0, -L[0], L[4],
                          -L[1], L[0], 0.0, L[5],
                          -L[3], -L[4], -L[5], 0.0};
    double sp[3], ep[3];
    line3d_trim(Pm, M, l1, l2, l3, den, (float)xs, (float)ys, sp);     // the measurements are the key line's floats
    line3d_trim(Pm, M, l1, l2, l3, den, (float)xe, (float)ye, ep);
    const double zs = ((R[6] * sp[0] + R[7] * sp[1]) + R[8] * sp[2]) + tz * 1.0;
    const double ze = ((R[6] * ep[0] + R[7] * ep[1]) + R[8] * ep[2]) + tz * 1.0;
    return 0.0 < zs && 0.0 < ze;
}

// the verdict of :498 and :568 on line edge t: chi_sq_2D below the chi2 of its last evaluation, or the depth test fails (NaN fails)
__host__ __device__ __forceinline__ bool ll_edge_bad(const LaView& V, const LlView& W, const PoseCam& C, int t, int kc, int lc) {
    const int kf = W.e_kf()[t], l = W.e_l()[t];
    double est[7], L[6];
    _Pragma("unroll") for (int i = 0; i < 7; ++i) est[i] = la_k(V, kf, kc + i);
    _Pragma("unroll") for (int i = 0; i < 6; ++i) L[i] = ll_l(W, l, lc + i);
    const bool deep = ll_depth_ok(est, C, L, ll_e(W, t, kLlRowObs), ll_e(W, t, kLlRowObs + 1), ll_e(W, t, kLlRowObs + 2), ll_e(W, t, kLlRowObs + 3));
    return (double)kPoseChiSq2D < ll_e(W, t, kLlRowChi) || !deep;
}
// D17's verdict on point edge t (local_ba.hpp's la_solve and la_finish hold the same lines)
__host__ __device__ __forceinline__ bool ll_point_bad(const LaView& V, int t, int kc, int lc) {
    const int kf = V.e_kf()[t], l = V.e_l()[t];
    double est[7], p[3], x, y, z;
    _Pragma("unroll") for (int i = 0; i < 7; ++i) est[i] = la_k(V, kf, kc + i);
    _Pragma("unroll") for (int i = 0; i < 3; ++i) p[i] = la_l(V, l, lc + i);
    pose_map(est, p, x, y, z);
    const double thr = (double)(la_e(V, t, kLaRowObs + 2) < 0.0 ? kPoseChiSq2D : kPoseChiSq3D);
    return thr < la_e(V, t, kLaRowChi) || !(0.0 < z);
}

// ---- step 1: D17's sets, then the lines': local lines, the key frames fixed through a line, the line edges (:204-224, :365-415)
template <class P> __host__ __device__ __forceinline__ void ll_prepare(const LlArgs& A, int g, LlShared& sh, P& par) {
    la_prepare(A.p, g, sh.s, par);
    par.barrier_g();
    LaOff O;
    la_offsets(A.p, g, O);
    const LaView V = la_view(A.p, O);
    LlOff Q;
    ll_offsets(A, g, Q);
    const LlView W = ll_view(A, Q);
    const LlDims E{A.LL, A.TL, A.obs_offsets_lines};
    const int tid = par.tid(), F = A.p.F, LL = A.LL, TL = A.TL, kls = A.kl_stride;
    for (int f = tid; f < F; f += P::NT) sh.s.fixed[f] = 0;
    for (int t = tid; t < TL; t += P::NT) { W.e_kf()[t] = -1; W.e_l()[t] = 0; W.lvl()[t] = 0; }
    if (tid == 0) sh.anyl = 0;
    par.barrier_g();
    for (int l = tid; l < LL; l += P::NT) {
        int lo, hi;
        la_run(E, l, lo, hi);
        bool local = false;
        if (!(A.line_erased && A.line_erased[l]))
            for (int t = lo; t < hi && !local; ++t) {
                const int kf = A.obs_kf_lines[t];
                local = (unsigned)kf < (unsigned)F && (sh.s.role[kf] == PLP_LOCAL_BA_KF_FREE || sh.s.role[kf] == PLP_LOCAL_BA_KF_ORIGIN);
            }
        W.role()[l] = local ? 1 : 0;
        W.act()[l] = 0;
        if (!local) continue;
        _Pragma("unroll") for (int i = 0; i < 6; ++i) ll_l(W, l, kLlLnEst + i) = A.pluecker[(size_t)6 * l + i];
        for (int t = lo; t < hi; ++t) {
            const int kf = A.obs_kf_lines[t];
            if ((unsigned)kf >= (unsigned)F || (A.p.kf_erased && A.p.kf_erased[kf])) continue;
            if (sh.s.role[kf] == PLP_LOCAL_BA_KF_NONE) sh.s.fixed[kf] = 1;
            int cnt = kls;
            if (A.kl_counts) { cnt = A.kl_counts[kf]; cnt = cnt < 0 ? 0 : cnt > kls ? kls : cnt; }
            const int idx = A.obs_idx_lines[t];
            if ((unsigned)idx >= (unsigned)cnt) continue;
            const plp_keyline* kl = A.keylines + ((size_t)kf * kls + idx);
            if ((unsigned)kl->octave >= (unsigned)A.num_levels_lsd) continue;
            W.e_kf()[t] = kf; W.e_l()[t] = l;
            ll_e(W, t, kLlRowObs + 0) = (double)kl->startPointX;
            ll_e(W, t, kLlRowObs + 1) = (double)kl->startPointY;
            ll_e(W, t, kLlRowObs + 2) = (double)kl->endPointX;
            ll_e(W, t, kLlRowObs + 3) = (double)kl->endPointY;
            ll_e(W, t, kLlRowObs + 4) = (double)A.inv_sigma_sq_lsd[kl->octave];
            ll_e(W, t, kLlRowChi) = 0.0;
            sh.anyl = 1;
        }
    }
    par.barrier_g();
    for (int f = tid; f < F; f += P::NT) {
        if (!(sh.s.role[f] == PLP_LOCAL_BA_KF_NONE && sh.s.fixed[f])) continue;
        V.kf_role()[f] = PLP_LOCAL_BA_KF_FIXED;
        const double* in = A.p.pose + (size_t)f * A.p.pose_stride;
        double p12[12], est[7];
        _Pragma("unroll") for (int i = 0; i < 12; ++i) p12[i] = in[i];
        pose_est_from_pose(p12, est);
        _Pragma("unroll") for (int i = 0; i < 7; ++i) la_k(V, f, kLaKfEst + i) = est[i];
    }
    if (tid == 0 && sh.anyl && V.hdr()[kLaHStatus] == PLP_LOCAL_BA_NO_EDGES) V.hdr()[kLaHStatus] = PLP_LOCAL_BA_OK;
}

// ---- the active sets of a round: la_round_setup with the line edges counted into a pose's activity, the line-edge list of every active pose
// behind its point-edge list, and the active lines
template <class P, class AA, class BB>
__host__ __device__ __forceinline__ void ll_round_setup(const AA& A, const BB& E, const LaView& V, const LlView& W, LlShared& sh, P& par) {
    LaShared& s = sh.s;
    const int tid = par.tid(), F = A.F, L = A.L, T = A.T, LL = E.L, TL = E.T, nf = V.hdr()[kLaHNf];
    for (int q = par.wave(); q < nf; q += P::NW) {
        const int kf = V.hdr()[kLaHFl + q];
        int c = 0, cl = 0;
        for (int base = 0; base < T; base += P::WS) {
            const int t = base + par.lane();
            const bool v = t < T && V.e_kf()[t] == kf && V.lvl()[t] == 0;
            c += (int)__builtin_popcountll(par.ballot(v));
        }
        for (int base = 0; base < TL; base += P::WS) {
            const int t = base + par.lane();
            const bool v = t < TL && W.e_kf()[t] == kf && W.lvl()[t] == 0;
            cl += (int)__builtin_popcountll(par.ballot(v));
        }
        if (par.lane() == 0) { s.cnt[q] = c; sh.cntl[q] = cl; }
    }
    for (int f = tid; f < F; f += P::NT) s.kf2ai[f] = -1;
    if (tid == 0) { s.nla = 0; sh.nlna = 0; }
    par.barrier();
    if (tid == 0) {
        int a = 0, o = 0, ol = 0;
        for (int q = 0; q < nf; ++q)
            if (s.cnt[q] + sh.cntl[q] > 0) {
                const int kf = V.hdr()[kLaHFl + q];
                s.kf2ai[kf] = (int16_t)a; s.akf[a] = kf; s.aoff[a] = o; s.acnt[a] = s.cnt[q]; sh.aoffl[a] = ol; sh.acntl[a] = sh.cntl[q];
                o += s.cnt[q]; ol += sh.cntl[q]; ++a;
            }
        s.nfa = a;
    }
    par.barrier();
    for (int a = par.wave(); a < s.nfa; a += P::NW) {
        const int kf = s.akf[a];
        int pos = s.aoff[a];
        for (int base = 0; base < T; base += P::WS) {
            const int t = base + par.lane();
            const bool v = t < T && V.e_kf()[t] == kf && V.lvl()[t] == 0;
            const unsigned long long m = par.ballot(v);
            if (v) V.byp()[pos + (int)__builtin_popcountll(m & ((1ull << par.lane()) - 1ull))] = t;
            pos += (int)__builtin_popcountll(m);
        }
        pos = sh.aoffl[a];
        for (int base = 0; base < TL; base += P::WS) {
            const int t = base + par.lane();
            const bool v = t < TL && W.e_kf()[t] == kf && W.lvl()[t] == 0;
            const unsigned long long m = par.ballot(v);
            if (v) W.byp()[pos + (int)__builtin_popcountll(m & ((1ull << par.lane()) - 1ull))] = t;
            pos += (int)__builtin_popcountll(m);
        }
    }
    for (int l = tid; l < L; l += P::NT) {
        bool act = false;
        if (V.lm_role()[l]) {
            int lo, hi;
            la_run(A, l, lo, hi);
            for (int t = lo; t < hi && !act; ++t) act = V.e_kf()[t] >= 0 && V.lvl()[t] == 0;
        }
        V.lm_act()[l] = act ? 1 : 0;
        if (act) s.nla = 1;
    }
    for (int l = tid; l < LL; l += P::NT) {
        bool act = false;
        if (W.role()[l]) {
            int lo, hi;
            la_run(E, l, lo, hi);
            for (int t = lo; t < hi && !act; ++t) act = W.e_kf()[t] >= 0 && W.lvl()[t] == 0;
        }
        W.act()[l] = act ? 1 : 0;
        if (act) sh.nlna = 1;
    }
    par.barrier_g();
}

// ---- the perturbed sets of a linearisation, once per vertex: exp(+-1e-9 e_d) est of every active free pose, oplus(+-1e-9 e_d) of every active line
template <class P, class BB> __host__ __device__ __forceinline__ void ll_perturb(const BB& E, const LaView& V, const LlView& W, LlShared& sh, P& par) {
    const int LL = E.L, cur = sh.s.cur;
    for (int it = par.tid(); it < 12 * sh.s.nfa; it += P::NT) {
        const int a = it / 12, which = it % 12, kf = sh.s.akf[a];
        double est[7], out[7];
        _Pragma("unroll") for (int i = 0; i < 7; ++i) est[i] = la_k(V, kf, 7 * cur + i);
        pose_perturb(est, which, out);
        _Pragma("unroll") for (int i = 0; i < 7; ++i) W.pp()[84 * a + 7 * which + i] = out[i];
    }
    for (int it = par.tid(); it < 8 * LL; it += P::NT) {
        const int l = it >> 3, which = it & 7, d = which >> 1;
        if (!W.act()[l]) continue;
        const double dv = (which & 1) ? -kPoseNumericDelta : kPoseNumericDelta;
        double Lc[6], v[4], out[6];
        _Pragma("unroll") for (int i = 0; i < 6; ++i) Lc[i] = ll_l(W, l, 6 * cur + i);
        _Pragma("unroll") for (int i = 0; i < 4; ++i) v[i] = i == d ? dv : 0.0;
        ll_oplus(Lc, v, out);
        _Pragma("unroll") for (int i = 0; i < 6; ++i) ll_l(W, l, kLlLnPert + 6 * which + i) = out[i];
    }
    par.barrier_g();
}

// ---- one pass over the level-0 line edges: chi2 and the robust chi2, and when lin both numeric Jacobian blocks (BaseBinaryEdge::linearizeOplus)
// and the quadratic form; the pose block and W only for a free pose.  The 21 errors of an edge are one loop over the tables.
template <class P, class BB>
__host__ __device__ __forceinline__ void ll_edge_pass(const BB& E, const LaView& V, const LlView& W, LlShared& sh, P& par, bool lin, bool robust, const double delta) {
    const int TL = E.T, buf = lin ? sh.s.cur : 1 - sh.s.cur;
    const double scalar = 1.0 / (2.0 * kPoseNumericDelta);
    for (int t = par.tid(); t < TL; t += P::NT) {
        const int kf = W.e_kf()[t];
        if (kf < 0 || W.lvl()[t]) continue;
        const int l = W.e_l()[t], a = sh.s.kf2ai[kf];
        double* R = W.et() + (size_t)t * kLlEdgeRows;
        const double xs = R[kLlRowObs], ys = R[kLlRowObs + 1], xe = R[kLlRowObs + 2], ye = R[kLlRowObs + 3], w = R[kLlRowObs + 4];
        const double* pe = V.kf() + ((size_t)kf * kLaKfRows + 7 * buf);
        const double* le = W.ln() + ((size_t)l * kLlLnRows + 6 * buf);
        double e0, e1;
        const double chi2 = pose_line_error(pe, sh.s.cam, le, xs, ys, xe, ye, w, e0, e1);
        double rho0 = chi2, rho1 = 1.0;
        if (robust) pose_huber(chi2, delta, rho0, rho1);
        R[kLlRowChi] = chi2;
        R[kLlRowRho] = rho0;
        if (!lin) continue;
        const bool free_pose = a >= 0;
        _Pragma("unroll 1") for (int k = free_pose ? 0 : 12; k < 20; ++k) {
            const double* pk = k < 12 ? W.pp() + (84 * a + 7 * k) : pe;
            const double* lk = k < 12 ? le : W.ln() + ((size_t)l * kLlLnRows + kLlLnPert + 6 * (k - 12));
            double q0, q1;
            pose_line_error(pk, sh.s.cam, lk, xs, ys, xe, ye, w, q0, q1);
            R[kLlRowW + 2 * k] = q0; R[kLlRowW + 2 * k + 1] = q1;
        }
        double Jp[12], Jl[8];
        _Pragma("unroll") for (int d = 0; d < 6; ++d) {
            Jp[d] = free_pose ? scalar * (R[kLlRowW + 4 * d] - R[kLlRowW + 4 * d + 2]) : 0.0;
            Jp[6 + d] = free_pose ? scalar * (R[kLlRowW + 4 * d + 1] - R[kLlRowW + 4 * d + 3]) : 0.0;
        }
        _Pragma("unroll") for (int d = 0; d < 4; ++d) {
            Jl[d] = scalar * (R[kLlRowW + 24 + 4 * d] - R[kLlRowW + 24 + 4 * d + 2]);
            Jl[4 + d] = scalar * (R[kLlRowW + 24 + 4 * d + 1] - R[kLlRowW + 24 + 4 * d + 3]);
        }
        if (free_pose) pose_terms(Jp, 2, e0, e1, 0.0, w, rho0, rho1, R, 1);
        const double wr = rho1 * w;
        const double o0 = (-(w * e0)) * rho1, o1 = (-(w * e1)) * rho1;
        int k = 0;
        _Pragma("unroll") for (int i = 0; i < 4; ++i)
            _Pragma("unroll") for (int j = i; j < 4; ++j) R[kLlRowLn + (k++)] = Jl[i] * (wr * Jl[j]) + Jl[4 + i] * (wr * Jl[4 + j]);
        _Pragma("unroll") for (int i = 0; i < 4; ++i) R[kLlRowLn + 10 + i] = Jl[i] * o0 + Jl[4 + i] * o1;
        if (free_pose)
            _Pragma("unroll") for (int i = 0; i < 6; ++i)
                _Pragma("unroll") for (int j = 0; j < 4; ++j) R[kLlRowW + 4 * i + j] = Jp[i] * (wr * Jl[j]) + Jp[6 + i] * (wr * Jl[4 + j]);
    }
    par.barrier_g();
}

// ---- the lines' sums of a pass, after la_sums: every active line's robust chi2 (and its block when lin) over its level-0 edges in list order;
// every active pose's 27 sums go on over its line edges in edge order
template <class P, class BB> __host__ __device__ __forceinline__ void ll_sums(const BB& E, const LaView& V, const LlView& W, LlShared& sh, P& par, bool lin) {
    const int LL = E.L;
    for (int l = par.tid(); l < LL; l += P::NT) {
        if (!W.act()[l]) continue;
        int lo, hi;
        la_run(E, l, lo, hi);
        double part = 0.0;
        if (lin)
            _Pragma("unroll") for (int i = 0; i < 14; ++i) ll_l(W, l, kLlLnH + i) = 0.0;
        for (int t = lo; t < hi; ++t) {
            if (W.e_kf()[t] < 0 || W.lvl()[t]) continue;
            part = part + ll_e(W, t, kLlRowRho);
            if (lin)
                _Pragma("unroll") for (int i = 0; i < 14; ++i) ll_l(W, l, kLlLnH + i) = ll_l(W, l, kLlLnH + i) + ll_e(W, t, kLlRowLn + i);
        }
        ll_l(W, l, kLlLnPart) = part;
    }
    if (lin)
        for (int it = par.tid(); it < 27 * sh.s.nfa; it += P::NT) {
            const int a = it / 27, term = it % 27;
            const int32_t* list = W.byp() + sh.aoffl[a];
            double acc = la_p(V, a, term);
            for (int k = 0; k < sh.acntl[a]; ++k) acc = acc + ll_e(W, list[k], term);
            la_p(V, a, term) = acc;
        }
    par.barrier_g();
}

// la_chain over the active lines in table order, going on from sh.s.acc: mode 0 adds row `row`, mode 1 takes the largest |diagonal| of the blocks
template <class P, class BB> __host__ __device__ __forceinline__ void ll_chain(const BB& E, const LlView& W, LlShared& sh, P& par, int mode, int row) {
    const int LL = E.L, tid = par.tid();
    for (int base = 0; base < LL; base += P::NT) {
        const int l = base + tid;
        double v = 0.0;
        if (l < LL && W.act()[l]) {
            if (mode == 0) v = ll_l(W, l, row);
            else
                _Pragma("unroll") for (int i = 0; i < 4; ++i) {
                    const double d = __builtin_fabs(ll_l(W, l, kLlLnH + (i == 0 ? 0 : i == 1 ? 4 : i == 2 ? 7 : 9)));
                    v = d > v ? d : v;
                }
        }
        sh.s.tile[tid] = v;
        par.barrier();
        if (tid == 0) {
            const int cnt = LL - base < P::NT ? LL - base : P::NT;
            double acc = sh.s.acc;
            if (mode == 0) for (int i = 0; i < cnt; ++i) acc = acc + sh.s.tile[i];
            else for (int i = 0; i < cnt; ++i) acc = sh.s.tile[i] > acc ? sh.s.tile[i] : acc;
            sh.s.acc = acc;
        }
        par.barrier();
    }
}

// ---- one damped solve over both kinds of marginalised vertex: la_solve_system restated with the lines' inverse (lev_chol at N = 4 against the
// four unit vectors), their Y and their subtractions behind the landmarks', and x_line = Hinv (b_l - sum W^T x_p) in list order
template <class P, class AA, class BB>
__host__ __device__ __forceinline__ void ll_solve_system(const AA& A, const BB& E, const LaView& V, const LlView& W, LlShared& shl, P& par) {
    LaShared& sh = shl.s;
    const int L = A.L, T = A.T, LL = E.L, TL = E.T, tid = par.tid(), nfa = sh.nfa, n = 6 * nfa;
    const double lambda = sh.lambda;
    if (tid == 0) sh.ok = 1;
    par.barrier();
    for (int l = tid; l < L; l += P::NT) {
        if (!V.lm_act()[l]) continue;
        double a[6], o[6];
        _Pragma("unroll") for (int i = 0; i < 6; ++i) a[i] = la_l(V, l, kLaLmH + i);
        a[0] = a[0] + lambda; a[3] = a[3] + lambda; a[5] = a[5] + lambda;
        if (!la_inv3(a, o)) sh.ok = 0;
        _Pragma("unroll") for (int i = 0; i < 6; ++i) la_l(V, l, kLaLmInv + i) = o[i];
    }
    for (int l = tid; l < LL; l += P::NT) {
        if (!W.act()[l]) continue;
        double H[10], Lf[16], y[4], x[4], u[4];
        _Pragma("unroll") for (int i = 0; i < 10; ++i) H[i] = ll_l(W, l, kLlLnH + i);
        _Pragma("unroll 1") for (int k = 0; k < 4; ++k) {
            _Pragma("unroll") for (int i = 0; i < 4; ++i) u[i] = i == k ? 1.0 : 0.0;
            if (!lev_chol<4>(H, u, lambda, Lf, y, x)) sh.ok = 0;
            _Pragma("unroll") for (int i = 0; i < 4; ++i)
                if (i <= k) ll_l(W, l, kLlLnInv + lev_h_index<4>(i, k)) = x[i];
        }
    }
    for (int it = tid; it < n * n; it += P::NT) {
        const int p = it / n, q = it % n;
        double v = 0.0;
        if (q >= p && q / 6 == p / 6) {
            v = la_p(V, p / 6, lev_h_index<6>(p % 6, q % 6));
            if (p == q) v = v + lambda;
        }
        V.S()[(size_t)p * kLaN + q] = v;
    }
    for (int p = tid; p < n; p += P::NT) V.pv()[kLaPvB + p] = la_p(V, p / 6, 21 + p % 6);
    par.barrier_g();
    for (int t = tid; t < T; t += P::NT) {
        const int kf = V.e_kf()[t];
        if (kf < 0 || V.lvl()[t] || sh.kf2ai[kf] < 0) continue;
        const int l = V.e_l()[t];
        double h[6];
        _Pragma("unroll") for (int i = 0; i < 6; ++i) h[i] = la_l(V, l, kLaLmInv + i);
        _Pragma("unroll") for (int r = 0; r < 6; ++r) {
            const double w0 = la_e(V, t, kLaRowW + 3 * r), w1 = la_e(V, t, kLaRowW + 3 * r + 1), w2 = la_e(V, t, kLaRowW + 3 * r + 2);
            la_e(V, t, kLaRowY + 3 * r) = (w0 * h[0] + w1 * h[1]) + w2 * h[2];
            la_e(V, t, kLaRowY + 3 * r + 1) = (w0 * h[1] + w1 * h[3]) + w2 * h[4];
            la_e(V, t, kLaRowY + 3 * r + 2) = (w0 * h[2] + w1 * h[4]) + w2 * h[5];
        }
    }
    for (int t = tid; t < TL; t += P::NT) {
        const int kf = W.e_kf()[t];
        if (kf < 0 || W.lvl()[t] || sh.kf2ai[kf] < 0) continue;
        const int l = W.e_l()[t];
        _Pragma("unroll 1") for (int r = 0; r < 6; ++r) {
            const double w0 = ll_e(W, t, kLlRowW + 4 * r), w1 = ll_e(W, t, kLlRowW + 4 * r + 1), w2 = ll_e(W, t, kLlRowW + 4 * r + 2), w3 = ll_e(W, t, kLlRowW + 4 * r + 3);
            _Pragma("unroll") for (int k = 0; k < 4; ++k)
                ll_e(W, t, kLlRowY + 4 * r + k) = ((w0 * ll_l(W, l, kLlLnInv + ll_h4(0, k)) + w1 * ll_l(W, l, kLlLnInv + ll_h4(1, k))) + w2 * ll_l(W, l, kLlLnInv + ll_h4(2, k))) +
                                                  w3 * ll_l(W, l, kLlLnInv + ll_h4(3, k));
        }
    }
    par.barrier_g();
    // the Schur complement: item (i, r, c) first walks pose i's point edges as D17, then its line edges in edge order and for each the level-0
    // edges of its line in list order
    for (int it = tid; it < 42 * nfa; it += P::NT) {
        const int i = it / 42, r = (it % 42) / 7, c = it % 7;
        const int32_t* list = V.byp() + sh.aoff[i];
        for (int k = 0; k < sh.acnt[i]; ++k) {
            const int ta = list[k], l = V.e_l()[ta];
            const double y0 = la_e(V, ta, kLaRowY + 3 * r), y1 = la_e(V, ta, kLaRowY + 3 * r + 1), y2 = la_e(V, ta, kLaRowY + 3 * r + 2);
            if (c == 6) {
                double* b = V.pv() + kLaPvB + 6 * i + r;
                *b = *b - ((y0 * la_l(V, l, kLaLmB + 0) + y1 * la_l(V, l, kLaLmB + 1)) + y2 * la_l(V, l, kLaLmB + 2));
                continue;
            }
            int lo, hi;
            la_run(A, l, lo, hi);
            for (int tb = lo; tb < hi; ++tb) {
                const int kfb = V.e_kf()[tb];
                if (kfb < 0 || V.lvl()[tb]) continue;
                const int j = sh.kf2ai[kfb];
                if (j < i || (j == i && c < r)) continue;
                double* s = V.S() + (size_t)(6 * i + r) * kLaN + 6 * j + c;
                *s = *s - ((y0 * la_e(V, tb, kLaRowW + 3 * c) + y1 * la_e(V, tb, kLaRowW + 3 * c + 1)) + y2 * la_e(V, tb, kLaRowW + 3 * c + 2));
            }
        }
        list = W.byp() + shl.aoffl[i];
        for (int k = 0; k < shl.acntl[i]; ++k) {
            const int ta = list[k], l = W.e_l()[ta];
            const double y0 = ll_e(W, ta, kLlRowY + 4 * r), y1 = ll_e(W, ta, kLlRowY + 4 * r + 1), y2 = ll_e(W, ta, kLlRowY + 4 * r + 2), y3 = ll_e(W, ta, kLlRowY + 4 * r + 3);
            if (c == 6) {
                double* b = V.pv() + kLaPvB + 6 * i + r;
                *b = *b - (((y0 * ll_l(W, l, kLlLnB + 0) + y1 * ll_l(W, l, kLlLnB + 1)) + y2 * ll_l(W, l, kLlLnB + 2)) + y3 * ll_l(W, l, kLlLnB + 3));
                continue;
            }
            int lo, hi;
            la_run(E, l, lo, hi);
            for (int tb = lo; tb < hi; ++tb) {
                const int kfb = W.e_kf()[tb];
                if (kfb < 0 || W.lvl()[tb]) continue;
                const int j = sh.kf2ai[kfb];
                if (j < i || (j == i && c < r)) continue;
                double* s = V.S() + (size_t)(6 * i + r) * kLaN + 6 * j + c;
                *s = *s - (((y0 * ll_e(W, tb, kLlRowW + 4 * c) + y1 * ll_e(W, tb, kLlRowW + 4 * c + 1)) + y2 * ll_e(W, tb, kLlRowW + 4 * c + 2)) + y3 * ll_e(W, tb, kLlRowW + 4 * c + 3));
            }
        }
    }
    par.barrier_g();
    for (int j = 0; j < n; ++j) {
        for (int p = j + tid; p < n; p += P::NT) {
            double s = V.S()[(size_t)j * kLaN + j], v = V.S()[(size_t)j * kLaN + p];
            for (int k = 0; k < j; ++k) {
                const double ljk = V.S()[(size_t)k * kLaN + j];
                s = s - ljk * ljk;
                if (p > j) v = v - V.S()[(size_t)k * kLaN + p] * ljk;
            }
            if (!(s > 0.0) || s > kLevDblMax) { sh.ok = 0; continue; }
            const double d = __builtin_sqrt(s);
            if (p == j) sh.dl[j] = d;
            else V.S()[(size_t)j * kLaN + p] = v / d;
        }
        par.barrier_g();
    }
    if (sh.ok) {
        for (int p = tid; p < n; p += P::NT) sh.v[p] = V.pv()[kLaPvB + p];
        par.barrier();
        for (int j = 0; j < n; ++j) {
            if (tid == 0) sh.y[j] = sh.v[j] / sh.dl[j];
            par.barrier();
            for (int p = j + 1 + tid; p < n; p += P::NT) sh.v[p] = sh.v[p] - V.S()[(size_t)j * kLaN + p] * sh.y[j];
            par.barrier();
        }
        for (int p = tid; p < n; p += P::NT) sh.v[p] = sh.y[p];
        par.barrier();
        for (int j = n - 1; j >= 0; --j) {
            if (tid == 0) sh.x[j] = sh.v[j] / sh.dl[j];
            par.barrier();
            for (int p = tid; p < j; p += P::NT) sh.v[p] = sh.v[p] - V.S()[(size_t)p * kLaN + j] * sh.x[j];
            par.barrier();
        }
    }
    par.barrier();
    const bool ok = sh.ok != 0;
    if (!ok)
        for (int p = tid; p < n; p += P::NT) sh.x[p] = 0.0;
    par.barrier();
    for (int l = tid; l < L; l += P::NT) {
        if (!V.lm_act()[l]) continue;
        double t3[3] = {0.0, 0.0, 0.0};
        if (ok) {
            int lo, hi;
            la_run(A, l, lo, hi);
            _Pragma("unroll") for (int i = 0; i < 3; ++i) t3[i] = la_l(V, l, kLaLmB + i);
            for (int t = lo; t < hi; ++t) {
                const int kf = V.e_kf()[t];
                if (kf < 0 || V.lvl()[t]) continue;
                const int j = sh.kf2ai[kf];
                if (j < 0) continue;
                _Pragma("unroll") for (int i = 0; i < 3; ++i) {
                    double d = la_e(V, t, kLaRowW + i) * sh.x[6 * j];
                    _Pragma("unroll") for (int r = 1; r < 6; ++r) d = d + la_e(V, t, kLaRowW + 3 * r + i) * sh.x[6 * j + r];
                    t3[i] = t3[i] - d;
                }
            }
            double h[6];
            _Pragma("unroll") for (int i = 0; i < 6; ++i) h[i] = la_l(V, l, kLaLmInv + i);
            const double x0 = (h[0] * t3[0] + h[1] * t3[1]) + h[2] * t3[2], x1 = (h[1] * t3[0] + h[3] * t3[1]) + h[4] * t3[2], x2 = (h[2] * t3[0] + h[4] * t3[1]) + h[5] * t3[2];
            t3[0] = x0; t3[1] = x1; t3[2] = x2;
        }
        _Pragma("unroll") for (int i = 0; i < 3; ++i) la_l(V, l, kLaLmX + i) = t3[i];
    }
    for (int l = tid; l < LL; l += P::NT) {
        if (!W.act()[l]) continue;
        double t4[4] = {0.0, 0.0, 0.0, 0.0};
        if (ok) {
            int lo, hi;
            la_run(E, l, lo, hi);
            _Pragma("unroll") for (int i = 0; i < 4; ++i) t4[i] = ll_l(W, l, kLlLnB + i);
            for (int t = lo; t < hi; ++t) {
                const int kf = W.e_kf()[t];
                if (kf < 0 || W.lvl()[t]) continue;
                const int j = sh.kf2ai[kf];
                if (j < 0) continue;
                _Pragma("unroll") for (int i = 0; i < 4; ++i) {
                    double d = ll_e(W, t, kLlRowW + i) * sh.x[6 * j];
                    _Pragma("unroll") for (int r = 1; r < 6; ++r) d = d + ll_e(W, t, kLlRowW + 4 * r + i) * sh.x[6 * j + r];
                    t4[i] = t4[i] - d;
                }
            }
            double x4[4];
            _Pragma("unroll") for (int i = 0; i < 4; ++i)
                x4[i] = ((ll_l(W, l, kLlLnInv + ll_h4(i, 0)) * t4[0] + ll_l(W, l, kLlLnInv + ll_h4(i, 1)) * t4[1]) + ll_l(W, l, kLlLnInv + ll_h4(i, 2)) * t4[2]) +
                        ll_l(W, l, kLlLnInv + ll_h4(i, 3)) * t4[3];
            _Pragma("unroll") for (int i = 0; i < 4; ++i) t4[i] = x4[i];
        }
        _Pragma("unroll") for (int i = 0; i < 4; ++i) ll_l(W, l, kLlLnX + i) = t4[i];
    }
    par.barrier_g();
}

// the tried estimate of every local line: oplus(x) of the kept one for an active line, a copy for the others
template <class P, class BB> __host__ __device__ __forceinline__ void ll_update(const BB& E, const LlView& W, LlShared& sh, P& par) {
    const int LL = E.L, lc = 6 * sh.s.cur, lt = 6 - lc;
    for (int l = par.tid(); l < LL; l += P::NT) {
        if (!W.role()[l]) continue;
        double Lc[6], v[4], out[6];
        _Pragma("unroll") for (int i = 0; i < 6; ++i) Lc[i] = ll_l(W, l, lc + i);
        if (W.act()[l]) {
            _Pragma("unroll") for (int i = 0; i < 4; ++i) v[i] = ll_l(W, l, kLlLnX + i);
            ll_oplus(Lc, v, out);
            _Pragma("unroll") for (int i = 0; i < 6; ++i) ll_l(W, l, lt + i) = out[i];
        } else {
            _Pragma("unroll") for (int i = 0; i < 6; ++i) ll_l(W, l, lt + i) = Lc[i];
        }
    }
    par.barrier_g();
}

// computeScale's partial of every active line, x . (lambda x + b_l), where ll_chain adds it behind the landmarks'
template <class P, class BB> __host__ __device__ __forceinline__ void ll_scale_parts(const BB& E, const LlView& W, LlShared& sh, P& par) {
    const int LL = E.L;
    const double lambda = sh.s.lambda;
    for (int l = par.tid(); l < LL; l += P::NT) {
        if (!W.act()[l]) continue;
        double part = 0.0;
        _Pragma("unroll") for (int i = 0; i < 4; ++i) {
            const double x = ll_l(W, l, kLlLnX + i);
            part = part + x * (lambda * x + ll_l(W, l, kLlLnB + i));
        }
        ll_l(W, l, kLlLnPart) = part;
    }
}

// ---- one round of one problem (:434-510): la_solve's loop with the lines' half of every step behind the points'.  The two rounds are two
// instances, so that the kernels can run them as two launches; what round 1 hands to round 2 lies in the problem's header (the kept buffer, the
// robust chi2 and lambda of its end) and in the edge levels.  ROUND 0 runs with the Huber kernels and ends with the edges that go to level 1.
template <int ROUND, class P> __host__ __device__ __forceinline__ void ll_solve_round(const LlArgs& A, int g, LlShared& shl, P& par) {
    LaShared& sh = shl.s;
    const int tid = par.tid();
    if (tid == 0) { la_offsets(A.p, g, sh.O); sh.D.F = A.p.F; sh.D.L = A.p.L; sh.D.T = A.p.T; ll_offsets(A, g, shl.O); shl.LL = A.LL; shl.TL = A.TL; }
    par.barrier();
    const LaView V = la_view(A.p, sh.O);
    const LlView W = ll_view(A, shl.O);
    const LaDimsView D{sh.D.F, sh.D.L, sh.D.T, A.p.obs_offsets};
    const LlDimsView E{shl.LL, shl.TL, A.obs_offsets_lines};
    if (V.hdr()[kLaHStatus] != PLP_LOCAL_BA_OK) return;
    for (int f = tid; f < D.F; f += P::NT) sh.role[f] = V.kf_role()[f];
    if (tid == 0) {
        shl.iters = ROUND == 0 ? A.p.it1 : A.p.it2; shl.delta_lines = A.p.delta_2d;
        sh.cam.fx = A.p.cam.fx; sh.cam.fy = A.p.cam.fy; sh.cam.cx = A.p.cam.cx; sh.cam.cy = A.p.cam.cy; sh.cam.fxb = A.p.cam.fxb;
        sh.cam.k20 = A.p.cam.k20; sh.cam.k21 = A.p.cam.k21; sh.cam.k22 = A.p.cam.k22;
        sh.delta = A.p.mono_setup ? A.p.delta_2d : A.p.delta_3d; sh.ni = 2.0;
        if (ROUND == 0) { sh.lambda = 0.0; sh.current_chi = 0.0; sh.cur = 0; }
        else { sh.current_chi = V.hd()[0]; sh.lambda = V.hd()[1]; sh.cur = V.hdr()[kLaHCur]; }
    }
    par.barrier();
    constexpr bool robust = ROUND == 0;
    ll_round_setup(D, E, V, W, shl, par);
    if (tid == 0) { sh.iterations = 0; sh.rejected = 0; sh.end = 0; sh.drops = 0; }
    par.barrier();
    int it = 0;
    bool lin = true;
    while (sh.nla || shl.nlna) {
        if (!lin) {
            ll_solve_system(D, E, V, W, shl, par);
            la_update(D, V, sh, par);
            ll_update(E, W, shl, par);
        } else {
            ll_perturb(E, V, W, shl, par);
        }
        la_edge_pass(D, V, sh, par, lin, robust);
        ll_edge_pass(E, V, W, shl, par, lin, robust, shl.delta_lines);
        la_sums(D, V, sh, par, lin);
        ll_sums(E, V, W, shl, par, lin);
        if (tid == 0) sh.acc = 0.0;
        par.barrier();
        la_chain(D, V, sh, par, 0, kLaLmPart);
        ll_chain(E, W, shl, par, 0, kLlLnPart);
        if (lin) {
            if (tid == 0) {
                sh.current_chi = sh.acc;
                double m = 0.0;                              // computeLambdaInit over every active vertex, at iteration 0
                for (int a = 0; a < sh.nfa; ++a)
                    _Pragma("unroll") for (int j = 0; j < 6; ++j) {
                        const double d = __builtin_fabs(la_p(V, a, lev_h_index<6>(j, j)));
                        m = d > m ? d : m;
                    }
                sh.acc = m;
            }
            par.barrier();
            if (it == 0) {
                la_chain(D, V, sh, par, 1, 0);
                ll_chain(E, W, shl, par, 1, 0);
                if (tid == 0) { sh.lambda = 1e-5 * sh.acc; sh.ni = 2.0; }
            }
            if (tid == 0) { sh.qmax = 0; sh.rho = 0.0; }
            par.barrier();
            lin = false;
            continue;
        }
        const double temp_sum = sh.acc;
        par.barrier();
        ll_scale_parts(E, W, shl, par);
        la_scale(D, V, sh, par);
        ll_chain(E, W, shl, par, 0, kLlLnPart);
        if (tid == 0) {
            lev_decide(sh, sh.ok != 0, temp_sum, sh.acc, [&sh] { sh.cur = 1 - sh.cur; }, [] {});   // kept: the tried estimates become the kept ones
            if (!sh.go_on) {
                sh.iterations += 1;
                sh.end = lev_end(sh);
            }
        }
        par.barrier();
        if (sh.go_on) continue;
        ++it;
        if (sh.end || it >= shl.iters) break;
        lin = true;
    }
    if (ROUND == 0) {                                        // :456-505: the edges that go to level 1, points and lines counted together
        const int T = D.T, TL = E.T, kc = 7 * sh.cur;
        int drops = 0;
        for (int t = tid; t < T; t += P::NT) {
            if (V.e_kf()[t] < 0) continue;
            const bool bad = ll_point_bad(V, t, kc, 3 * sh.cur);
            V.lvl()[t] = bad ? 1 : 0;
            drops += bad ? 1 : 0;
        }
        for (int t = tid; t < TL; t += P::NT) {
            if (W.e_kf()[t] < 0) continue;
            const bool bad = ll_edge_bad(V, W, sh.cam, t, kc, 6 * sh.cur);
            W.lvl()[t] = bad ? 1 : 0;
            drops += bad ? 1 : 0;
        }
        if (drops) par.add(sh.drops, drops);
    }
    par.barrier_g();
    if (tid == 0) {
        int32_t* ri = V.hdr() + kLaHInfo + 4 * ROUND;
        ri[0] = sh.iterations; ri[1] = sh.rejected; ri[2] = sh.drops; ri[3] = sh.end ? sh.end : sh.iterations ? kLevEndIterations : 0;
        V.hd()[2 * ROUND] = sh.current_chi; V.hd()[2 * ROUND + 1] = sh.lambda;
        V.hdr()[kLaHCur] = sh.cur;
    }
}
// both rounds in turn: the host build
template <class P> __host__ __device__ __forceinline__ void ll_solve(const LlArgs& A, int g, LlShared& shl, P& par) {
    ll_solve_round<0>(A, g, shl, par);
    par.barrier_g();
    ll_solve_round<1>(A, g, shl, par);
}

// ---- the outputs: la_finish, then the lines' roles, estimates and step [7]'s verdict of every line edge (:555-573)
template <class P> __host__ __device__ __forceinline__ void ll_finish(const LlArgs& A, int g, P& par) {
    la_finish(A.p, g, par);
    LaOff O;
    la_offsets(A.p, g, O);
    const LaView V = la_view(A.p, O);
    LlOff Q;
    ll_offsets(A, g, Q);
    const LlView W = ll_view(A, Q);
    const int tid = par.tid(), LL = A.LL, TL = A.TL;
    const int status = V.hdr()[kLaHStatus], kc = 7 * V.hdr()[kLaHCur], lc = 6 * V.hdr()[kLaHCur];
    if (status == PLP_LOCAL_BA_TOO_MANY_FREE) return;
    for (int l = tid; l < LL; l += P::NT) {
        A.out_line_role[(size_t)g * LL + l] = W.role()[l];
        if (!W.role()[l]) continue;
        _Pragma("unroll") for (int i = 0; i < 6; ++i) A.out_pluecker[((size_t)g * LL + l) * 6 + i] = ll_l(W, l, lc + i);
    }
    for (int t = tid; t < TL; t += P::NT) {
        if (W.e_kf()[t] < 0) continue;
        A.out_outlier_lines[(size_t)g * TL + t] = ll_edge_bad(V, W, A.p.cam, t, kc, lc) ? 1 : 0;
    }
}

hipError_t launch_local_ba_lines(hipStream_t st, const LlArgs& A);

}  // namespace plp
