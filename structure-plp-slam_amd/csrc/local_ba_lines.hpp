// optimize::local_bundle_adjuster_extended_line::optimize (optimize/local_bundle_adjuster_extended_line.cc:70-674), one definition for host and
// device (plp_local_ba_lines_* / plp_model_local_ba_lines*_host, include/plp_front.h) on top of local_ba.hpp (D17): the
// 4-DoF line vertex in orthonormal representation (g2o/line3d.h), the binary line edge with both numeric Jacobian blocks
// (g2o/se3/reproj_edge_line3d_orthonormal.h), the 4 x 4 marginalised blocks beside the 3 x 3 ones and the line half of the outlier schedule.
// The active sets, the damped solve and the round are local_ba.hpp's own (la_round_setup, la_solve_system, la_round), and so is the point half of
// every other step, so that a problem without a line edge takes exactly D17's arithmetic.  What is here is the lines' half: the layout of their
// tables, the vertex and the edge, the line part of step 1 and of the outputs, and LlLines, the extension those shared steps call for the lines'
// counts and lists, their inverse, Y, Schur subtractions and x, their passes, sums, chains, scale parts, update and level-1 verdicts -- always
// behind the landmarks'.  f64 with IEEE + - * / sqrt only, in the order written; translation units that include this file are compiled with
// -ffp-contract=off.
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

// the lines' dimensions under the names la_run reads: L lines, T entries of their observation list, where the caller keeps them (the shared
// state in a round)
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
    const LlDimsView E{A.LL, A.TL, A.obs_offsets_lines};
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

// ---- the lines' half of a round: the extension that la_round_setup, la_solve_system and la_round (local_ba.hpp) call, each member behind the
// landmarks' half of its step
struct LlLines {
    LlDimsView E; LlView W; LlShared& sh;

    __host__ __device__ __forceinline__ bool any_active() const { return sh.nlna != 0; }

    // the active sets: every free key frame's level-0 line edges counted into its activity (count, cnt), the line-edge list of every active
    // pose behind its point-edge list (rank, place), and the active lines
    template <class P> __host__ __device__ __forceinline__ void count(const LaView& V, P& par) const {
        const int TL = E.T, nf = V.hdr()[kLaHNf];
        for (int q = par.wave(); q < nf; q += P::NW) {
            const int kf = V.hdr()[kLaHFl + q];
            int c = 0;
            for (int base = 0; base < TL; base += P::WS) {
                const int t = base + par.lane();
                const bool v = t < TL && W.e_kf()[t] == kf && W.lvl()[t] == 0;
                c += (int)__builtin_popcountll(par.ballot(v));
            }
            if (par.lane() == 0) sh.cntl[q] = c;
        }
        if (par.tid() == 0) sh.nlna = 0;
    }
    __host__ __device__ __forceinline__ int cnt(int q) const { return sh.cntl[q]; }
    __host__ __device__ __forceinline__ void rank(int a, int q) const {
        sh.aoffl[a] = a ? sh.aoffl[a - 1] + sh.acntl[a - 1] : 0;
        sh.acntl[a] = sh.cntl[q];
    }
    template <class P> __host__ __device__ __forceinline__ void place(P& par) const {
        const int TL = E.T;
        for (int a = par.wave(); a < sh.s.nfa; a += P::NW) {
            const int kf = sh.s.akf[a];
            int pos = sh.aoffl[a];
            for (int base = 0; base < TL; base += P::WS) {
                const int t = base + par.lane();
                const bool v = t < TL && W.e_kf()[t] == kf && W.lvl()[t] == 0;
                const unsigned long long m = par.ballot(v);
                if (v) W.byp()[pos + (int)__builtin_popcountll(m & ((1ull << par.lane()) - 1ull))] = t;
                pos += (int)__builtin_popcountll(m);
            }
        }
    }
    template <class P> __host__ __device__ __forceinline__ void active(P& par) const {
        const int LL = E.L;
        for (int l = par.tid(); l < LL; l += P::NT) {
            bool act = false;
            if (W.role()[l]) {
                int lo, hi;
                la_run(E, l, lo, hi);
                for (int t = lo; t < hi && !act; ++t) act = W.e_kf()[t] >= 0 && W.lvl()[t] == 0;
            }
            W.act()[l] = act ? 1 : 0;
            if (act) sh.nlna = 1;
        }
    }

    // the perturbed sets of a linearisation, once per vertex: exp(+-1e-9 e_d) est of every active free pose, oplus(+-1e-9 e_d) of every active line
    template <class P> __host__ __device__ __forceinline__ void perturb(const LaView& V, P& par) const {
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

    // one pass over the level-0 line edges: chi2 and the robust chi2, and when lin both numeric Jacobian blocks (BaseBinaryEdge::linearizeOplus)
    // and the quadratic form; the pose block and W only for a free pose.  The 21 errors of an edge are one loop over the tables.
    template <class P> __host__ __device__ __forceinline__ void edge_pass(const LaView& V, P& par, bool lin, bool robust) const {
        const int TL = E.T, buf = lin ? sh.s.cur : 1 - sh.s.cur;
        const double scalar = 1.0 / (2.0 * kPoseNumericDelta), delta = sh.delta_lines;
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

    // the sums of a pass, after la_sums: every active line's robust chi2 (and its block when lin) over its level-0 edges in list order; every
    // active pose's 27 sums go on over its line edges in edge order
    template <class P> __host__ __device__ __forceinline__ void sums(const LaView& V, P& par, bool lin) const {
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

    // la_chain over the active lines in table order, going on from sh.s.acc: mode 0 adds the lines' partials (row Part), mode 1 takes the
    // largest |diagonal| of the blocks
    template <class P> __host__ __device__ __forceinline__ void chain(P& par, int mode) const {
        const LlView& Wl = W;
        la_chain_over(E.L, sh.s, par, mode, [&Wl, mode](int l) {
            double v = 0.0;
            if (Wl.act()[l]) {
                if (mode == 0) v = ll_l(Wl, l, kLlLnPart);
                else
                    _Pragma("unroll") for (int i = 0; i < 4; ++i) {
                        const double d = __builtin_fabs(ll_l(Wl, l, kLlLnH + (i == 0 ? 0 : i == 1 ? 4 : i == 2 ? 7 : 9)));
                        v = d > v ? d : v;
                    }
            }
            return v;
        });
    }

    // the damped solve: the lines' inverse (lev_chol at N = 4 against the four unit vectors) ...
    template <class P> __host__ __device__ __forceinline__ void inverse(P& par) const {
        const int LL = E.L;
        const double lambda = sh.s.lambda;
        for (int l = par.tid(); l < LL; l += P::NT) {
            if (!W.act()[l]) continue;
            double H[10], Lf[16], y[4], x[4], u[4];
            _Pragma("unroll") for (int i = 0; i < 10; ++i) H[i] = ll_l(W, l, kLlLnH + i);
            _Pragma("unroll 1") for (int k = 0; k < 4; ++k) {
                _Pragma("unroll") for (int i = 0; i < 4; ++i) u[i] = i == k ? 1.0 : 0.0;
                if (!lev_chol<4>(H, u, lambda, Lf, y, x)) sh.s.ok = 0;
                _Pragma("unroll") for (int i = 0; i < 4; ++i)
                    if (i <= k) ll_l(W, l, kLlLnInv + lev_h_index<4>(i, k)) = x[i];
            }
        }
    }
    // ... Y = W Hinv of every level-0 line edge of an active pose ...
    template <class P> __host__ __device__ __forceinline__ void y(P& par) const {
        const int TL = E.T;
        for (int t = par.tid(); t < TL; t += P::NT) {
            const int kf = W.e_kf()[t];
            if (kf < 0 || W.lvl()[t] || sh.s.kf2ai[kf] < 0) continue;
            const int l = W.e_l()[t];
            _Pragma("unroll 1") for (int r = 0; r < 6; ++r) {
                const double w0 = ll_e(W, t, kLlRowW + 4 * r), w1 = ll_e(W, t, kLlRowW + 4 * r + 1), w2 = ll_e(W, t, kLlRowW + 4 * r + 2), w3 = ll_e(W, t, kLlRowW + 4 * r + 3);
                _Pragma("unroll") for (int k = 0; k < 4; ++k)
                    ll_e(W, t, kLlRowY + 4 * r + k) = ((w0 * ll_l(W, l, kLlLnInv + ll_h4(0, k)) + w1 * ll_l(W, l, kLlLnInv + ll_h4(1, k))) + w2 * ll_l(W, l, kLlLnInv + ll_h4(2, k))) +
                                                      w3 * ll_l(W, l, kLlLnInv + ll_h4(3, k));
            }
        }
    }
    // ... item (i, r, c) of the Schur complement goes on over pose i's line edges in edge order and for each over the level-0 edges of its line
    // in list order ...
    __host__ __device__ __forceinline__ void schur(const LaView& V, int i, int r, int c) const {
        const int32_t* list = W.byp() + sh.aoffl[i];
        for (int k = 0; k < sh.acntl[i]; ++k) {
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
                const int j = sh.s.kf2ai[kfb];
                if (j < i || (j == i && c < r)) continue;
                double* s = V.S() + (size_t)(6 * i + r) * kLaN + 6 * j + c;
                *s = *s - (((y0 * ll_e(W, tb, kLlRowW + 4 * c) + y1 * ll_e(W, tb, kLlRowW + 4 * c + 1)) + y2 * ll_e(W, tb, kLlRowW + 4 * c + 2)) + y3 * ll_e(W, tb, kLlRowW + 4 * c + 3));
            }
        }
    }
    // ... and x_line = Hinv (b_l - sum W^T x_p) in list order
    template <class P> __host__ __device__ __forceinline__ void x(P& par, bool ok) const {
        const int LL = E.L;
        for (int l = par.tid(); l < LL; l += P::NT) {
            if (!W.act()[l]) continue;
            double t4[4] = {0.0, 0.0, 0.0, 0.0};
            if (ok) {
                int lo, hi;
                la_run(E, l, lo, hi);
                _Pragma("unroll") for (int i = 0; i < 4; ++i) t4[i] = ll_l(W, l, kLlLnB + i);
                for (int t = lo; t < hi; ++t) {
                    const int kf = W.e_kf()[t];
                    if (kf < 0 || W.lvl()[t]) continue;
                    const int j = sh.s.kf2ai[kf];
                    if (j < 0) continue;
                    _Pragma("unroll") for (int i = 0; i < 4; ++i) {
                        double d = ll_e(W, t, kLlRowW + i) * sh.s.x[6 * j];
                        _Pragma("unroll") for (int r = 1; r < 6; ++r) d = d + ll_e(W, t, kLlRowW + 4 * r + i) * sh.s.x[6 * j + r];
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
    }

    // the tried estimate of every local line: oplus(x) of the kept one for an active line, a copy for the others
    template <class P> __host__ __device__ __forceinline__ void update(P& par) const {
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

    // computeScale's partial of every active line, x . (lambda x + b_l), where chain adds it behind the landmarks'
    template <class P> __host__ __device__ __forceinline__ void scale_parts(P& par) const {
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

    // :456-505: the line edges that go to level 1 after round 0; how many this lane sent there
    template <class P> __host__ __device__ __forceinline__ int level1(const LaView& V, P& par, int kc) const {
        const int TL = E.T;
        int drops = 0;
        for (int t = par.tid(); t < TL; t += P::NT) {
            if (W.e_kf()[t] < 0) continue;
            const bool bad = ll_edge_bad(V, W, sh.s.cam, t, kc, 6 * sh.s.cur);
            W.lvl()[t] = bad ? 1 : 0;
            drops += bad ? 1 : 0;
        }
        return drops;
    }
};

// ---- one round of one problem (:434-510): la_round over points and lines.  The two rounds are two instances, so that the kernels can run them as
// two launches; what round 1 hands to round 2 lies in the problem's header (the kept buffer, the robust chi2 and lambda of its end) and in the
// edge levels.
template <int ROUND, class P> __host__ __device__ __forceinline__ void ll_solve_round(const LlArgs& A, int g, LlShared& shl, P& par) {
    LaShared& sh = shl.s;
    const int tid = par.tid();
    if (tid == 0) { la_offsets(A.p, g, sh.O); sh.D.F = A.p.F; sh.D.L = A.p.L; sh.D.T = A.p.T; ll_offsets(A, g, shl.O); shl.LL = A.LL; shl.TL = A.TL; }
    par.barrier();
    const LaView V = la_view(A.p, sh.O);
    const LaDimsView D{sh.D.F, sh.D.L, sh.D.T, A.p.obs_offsets};
    LlLines lines{{shl.LL, shl.TL, A.obs_offsets_lines}, ll_view(A, shl.O), shl};
    if (V.hdr()[kLaHStatus] != PLP_LOCAL_BA_OK) return;
    for (int f = tid; f < D.F; f += P::NT) sh.role[f] = V.kf_role()[f];
    if (tid == 0) {
        shl.iters = ROUND == 0 ? A.p.it1 : A.p.it2; shl.delta_lines = A.p.delta_2d;
        la_round_consts(A.p, sh);
        if (ROUND == 0) { sh.lambda = 0.0; sh.current_chi = 0.0; sh.cur = 0; }
        else { sh.current_chi = V.hd()[0]; sh.lambda = V.hd()[1]; sh.cur = V.hdr()[kLaHCur]; }
    }
    par.barrier();
    la_round(D, V, sh, par, lines, ROUND, shl.iters);
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
