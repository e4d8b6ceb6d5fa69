// optimize::local_bundle_adjuster::optimize (optimize/local_bundle_adjuster.cc:62-410), one definition for host and device (plp_local_ba_* /
// plp_model_local_ba*_host, include/plp_front.h) on top of pose_opt.hpp (D15): the sets and roles from the map tables,
// the binary reprojection edge with both Jacobian blocks, the ordered sums of the blocks, the Schur complement on the landmarks, the Cholesky of
// the reduced system and the two rounds; g2o's Levenberg-Marquardt accept / reject step and end rule are levenberg.hpp's.  f64 with IEEE
// + - * / sqrt only, in the order written; translation units that include this file are compiled with -ffp-contract=off.
//
// The active sets, the damped solve and the round (la_round_setup, la_solve_system, la_round) are the only ones of both local adjusters: they
// take an extension `X` for a second kind of marginalised vertex and call it at the places where its half of a step stands, always behind the
// landmarks' half.  LaNoLines, the extension of this adjuster, is empty; local_ba_lines.hpp's LlLines (D28) holds the line vertices.
//
// The steps are written once over a team `P` of lanes (P::NT lanes in waves of P::WS): the kernels run them with a workgroup of 512, the host
// build with a team of one, for which every barrier is empty and every strided loop is the plain loop.  No sum depends on the team's size: each
// coefficient is owned by one lane that adds its terms in the defined order.  All state between the steps lives in memory the caller names (a
// context's buffers on the device), reached with run-time indices.
#pragma once
#include "pose_opt.hpp"

namespace plp {

constexpr int kLaMaxFree = 64;            // free key frames of a problem: the reduced system has at most 384 rows
constexpr int kLaMaxKf = 1024;            // F
constexpr int kLaMaxObs = 1 << 18;        // T, and L
constexpr int kLaMaxProblems = 256;       // G
constexpr long long kLaMaxWork = 1ll << 22;   // G * T and G * L: the state of a call is G (78 T + 25 L + 14 F + 384^2) doubles, at most 3.8 GB; it fits L2 for a few problems of mapping size only
constexpr int kLaN = 6 * kLaMaxFree;
constexpr int kLaThreads = 512;           // the workgroup of the kernels (tests/test_gpu_local_ba.py restates it)

// rows of the per-edge table: D15's 28 terms of the pose block, then the landmark block, W = Jp^T Omega Jl, Y = W Hll^-1
enum { kLaRowRho = 27, kLaRowLm = 28, kLaRowW = 37, kLaRowY = 55, kLaRowChi = 73, kLaRowObs = 74, kLaEdgeRows = 78 };
// rows of the landmark table and of the key-frame table; the estimates are kept twice: buffer `cur` is the kept one, the other the tried one
enum { kLaLmEst = 0, kLaLmEst1 = 3, kLaLmH = 6, kLaLmB = 12, kLaLmInv = 15, kLaLmX = 21, kLaLmPart = 24, kLaLmRows = 25 };
enum { kLaKfEst = 0, kLaKfEst1 = 7, kLaKfRows = 14 };
// the pose sums [64][27], the reduced right-hand side [384]
enum { kLaPvB = 27 * kLaMaxFree, kLaPvDoubles = 27 * kLaMaxFree + kLaN, kLaHeadDoubles = 8 };
// the header ints of a problem
enum { kLaHStatus = 0, kLaHNf = 1, kLaHCur = 2, kLaHInfo = 4, kLaHFl = 16, kLaHdrInts = 16 + kLaMaxFree };

struct LaArgs {
    int G, F, L, T, kp_stride, pose_stride, num_levels, mono_setup, it1, it2;
    PoseCam cam;
    double delta_2d, delta_3d;
    float inv_sigma_sq[16];
    const double* pose; const uint8_t* kf_erased; const uint8_t* kf_is_origin; const plp_keypoint* undist; const float* x_right; const int32_t* counts;
    const double* pos_w; const uint8_t* lm_erased; const int32_t* obs_offsets; const int32_t* obs_kf; const int32_t* obs_idx; const uint8_t* kf_local;
    uint8_t* out_status; uint8_t* out_kf_role; uint8_t* out_lm_role; double* out_pose; double* out_pos_w; uint8_t* out_outlier;
    int32_t* out_round_info; double* out_round_chi2;
    double* ctx_d; int32_t* ctx_i; uint8_t* ctx_b;      // what the steps hand to one another
};
__host__ __device__ __forceinline__ size_t la_doubles(int F, int L, int T) {
    return (size_t)kLaEdgeRows * T + (size_t)kLaLmRows * L + (size_t)kLaKfRows * F + kLaPvDoubles + (size_t)kLaN * kLaN + kLaHeadDoubles;
}
__host__ __device__ __forceinline__ size_t la_ints(int T) { return (size_t)3 * T + kLaHdrInts; }
__host__ __device__ __forceinline__ size_t la_bytes(int F, int L, int T) { return (size_t)T + (size_t)2 * L + F; }

// where a problem's tables lie in the three buffers (elements); the view reaches them through the buffers' own pointers, so that the offsets
// can wait in the shared state while every access stays an access to global memory
struct LaOff { size_t et, lm, kf, pv, S, hd, e_l, e_kf, byp, hdr, lvl, lm_role, lm_act, kf_role; };
struct LaView {
    double* d; int32_t* i; uint8_t* b; const LaOff* o;
    __host__ __device__ __forceinline__ double* et() const { return d + o->et; }
    __host__ __device__ __forceinline__ double* lm() const { return d + o->lm; }
    __host__ __device__ __forceinline__ double* kf() const { return d + o->kf; }
    __host__ __device__ __forceinline__ double* pv() const { return d + o->pv; }
    __host__ __device__ __forceinline__ double* S() const { return d + o->S; }
    __host__ __device__ __forceinline__ double* hd() const { return d + o->hd; }
    __host__ __device__ __forceinline__ int32_t* e_l() const { return i + o->e_l; }
    __host__ __device__ __forceinline__ int32_t* e_kf() const { return i + o->e_kf; }
    __host__ __device__ __forceinline__ int32_t* byp() const { return i + o->byp; }
    __host__ __device__ __forceinline__ int32_t* hdr() const { return i + o->hdr; }
    __host__ __device__ __forceinline__ uint8_t* lvl() const { return b + o->lvl; }
    __host__ __device__ __forceinline__ uint8_t* lm_role() const { return b + o->lm_role; }
    __host__ __device__ __forceinline__ uint8_t* lm_act() const { return b + o->lm_act; }
    __host__ __device__ __forceinline__ uint8_t* kf_role() const { return b + o->kf_role; }
};
__host__ __device__ __forceinline__ void la_offsets(const LaArgs& A, int g, LaOff& O) {
    O.et = la_doubles(A.F, A.L, A.T) * g;
    O.lm = O.et + (size_t)kLaEdgeRows * A.T;
    O.kf = O.lm + (size_t)kLaLmRows * A.L;
    O.pv = O.kf + (size_t)kLaKfRows * A.F;
    O.S = O.pv + kLaPvDoubles;
    O.hd = O.S + (size_t)kLaN * kLaN;
    O.e_l = la_ints(A.T) * g;
    O.e_kf = O.e_l + A.T;
    O.byp = O.e_kf + A.T;
    O.hdr = O.byp + A.T;
    O.lvl = la_bytes(A.F, A.L, A.T) * g;
    O.lm_role = O.lvl + A.T;
    O.lm_act = O.lm_role + A.L;
    O.kf_role = O.lm_act + A.L;
}
__host__ __device__ __forceinline__ LaView la_view(const LaArgs& A, const LaOff& O) {
    LaView V;
    V.d = A.ctx_d; V.i = A.ctx_i; V.b = A.ctx_b; V.o = &O;
    return V;
}

// record-major tables: one edge's 78 doubles, one landmark's 25, one key frame's 14 lie together, so that a row is a constant offset
__host__ __device__ __forceinline__ double& la_e(const LaView& V, int t, int row) { return V.et()[(size_t)t * kLaEdgeRows + row]; }
__host__ __device__ __forceinline__ double& la_l(const LaView& V, int l, int row) { return V.lm()[(size_t)l * kLaLmRows + row]; }
__host__ __device__ __forceinline__ double& la_k(const LaView& V, int f, int row) { return V.kf()[(size_t)f * kLaKfRows + row]; }
__host__ __device__ __forceinline__ double& la_p(const LaView& V, int a, int term) { return V.pv()[a * 27 + term]; }

// what the steps of a round read of the arguments: in the shared state, so that on the device scalar registers are left to the loops
struct LaDims { int F, L, T; };
struct LaDimsView { const int& F; const int& L; const int& T; const int32_t* obs_offsets; };   // the observation list stays a kernel argument
// the team's shared state: LDS on the device, the stack on the host
struct LaShared {
    LaOff O; LaDims D;
    double tile[kLaThreads];
    double dl[kLaN], y[kLaN], x[kLaN], v[kLaN];
    double lambda, ni, current_chi, rho, acc, delta;
    PoseCam cam;
    int32_t ok, qmax, iterations, rejected, go_on, end, nfa, nla, any, drops, cur;
    int32_t wave_n[kLaThreads / 64], cnt[kLaMaxFree], aoff[kLaMaxFree], acnt[kLaMaxFree], akf[kLaMaxFree];
    int16_t kf2ai[kLaMaxKf];
    uint8_t role[kLaMaxKf], fixed[kLaMaxKf];
};

// the team of one of the host build
struct LaTeamHost {
    static constexpr int NT = 1, WS = 1, NW = 1;
    __host__ __device__ int tid() const { return 0; }
    __host__ __device__ int lane() const { return 0; }
    __host__ __device__ int wave() const { return 0; }
    __host__ __device__ void barrier() const {}
    __host__ __device__ void barrier_g() const {}
    __host__ __device__ unsigned long long ballot(bool v) const { return v ? 1ull : 0ull; }
    __host__ __device__ void add(int32_t& t, int v) const { t += v; }
};

// the closed inverse of a symmetric 3 x 3 matrix by cofactors (a = 00 01 02 11 12 22); false: a coefficient of the inverse is not finite
__host__ __device__ __forceinline__ bool la_inv3(const double* a, double* o) {
    const double c00 = a[3] * a[5] - a[4] * a[4], c01 = a[2] * a[4] - a[1] * a[5], c02 = a[1] * a[4] - a[2] * a[3];
    const double c11 = a[0] * a[5] - a[2] * a[2], c12 = a[1] * a[2] - a[0] * a[4], c22 = a[0] * a[3] - a[1] * a[1];
    const double det = (a[0] * c00 + a[1] * c01) + a[2] * c02;
    const double id = 1.0 / det;
    o[0] = c00 * id; o[1] = c01 * id; o[2] = c02 * id; o[3] = c11 * id; o[4] = c12 * id; o[5] = c22 * id;
    bool ok = true;
    _Pragma("unroll") for (int i = 0; i < 6; ++i) ok = ok && o[i] >= -kLevDblMax && o[i] <= kLevDblMax;
    return ok;
}

// the verdict of :305-331 and of step [7] on point edge t at the estimates of buffer (kc, lc): its chi-square bound below the chi2 of its last
// evaluation, or a depth that is not positive (NaN fails)
__host__ __device__ __forceinline__ bool la_point_bad(const LaView& V, int t, int kc, int lc) {
    const int kf = V.e_kf()[t], l = V.e_l()[t];
    double est[7], p[3], x, y, z;
    _Pragma("unroll") for (int i = 0; i < 7; ++i) est[i] = la_k(V, kf, kc + i);
    _Pragma("unroll") for (int i = 0; i < 3; ++i) p[i] = la_l(V, l, lc + i);
    pose_map(est, p, x, y, z);
    const double thr = (double)(la_e(V, t, kLaRowObs + 2) < 0.0 ? kPoseChiSq2D : kPoseChiSq3D);
    return thr < la_e(V, t, kLaRowChi) || !(0.0 < z);
}

// the extension of an adjuster without a second kind of marginalised vertex: every half of a step is empty.  The members are the places where
// la_round_setup, la_solve_system and la_round call an extension (LlLines of local_ba_lines.hpp says what each one does).
struct LaNoLines {
    __host__ __device__ __forceinline__ bool any_active() const { return false; }
    __host__ __device__ __forceinline__ int cnt(int) const { return 0; }
    __host__ __device__ __forceinline__ void rank(int, int) const {}
    template <class P> __host__ __device__ __forceinline__ void count(const LaView&, P&) const {}
    template <class P> __host__ __device__ __forceinline__ void place(P&) const {}
    template <class P> __host__ __device__ __forceinline__ void active(P&) const {}
    template <class P> __host__ __device__ __forceinline__ void inverse(P&) const {}
    template <class P> __host__ __device__ __forceinline__ void y(P&) const {}
    __host__ __device__ __forceinline__ void schur(const LaView&, int, int, int) const {}
    template <class P> __host__ __device__ __forceinline__ void x(P&, bool) const {}
    template <class P> __host__ __device__ __forceinline__ void perturb(const LaView&, P&) const {}
    template <class P> __host__ __device__ __forceinline__ void edge_pass(const LaView&, P&, bool, bool) const {}
    template <class P> __host__ __device__ __forceinline__ void sums(const LaView&, P&, bool) const {}
    template <class P> __host__ __device__ __forceinline__ void chain(P&, int) const {}
    template <class P> __host__ __device__ __forceinline__ void scale_parts(P&) const {}
    template <class P> __host__ __device__ __forceinline__ void update(P&) const {}
    template <class P> __host__ __device__ __forceinline__ int level1(const LaView&, P&, int) const { return 0; }
};

// the observations of landmark l: [lo, hi) of the observation list, cut to the list
template <class AA> __host__ __device__ __forceinline__ void la_run(const AA& A, int l, int& lo, int& hi) {
    lo = A.obs_offsets[l]; hi = A.obs_offsets[l + 1];
    lo = lo < 0 ? 0 : lo > A.T ? A.T : lo;
    hi = hi < lo ? lo : hi > A.T ? A.T : hi;
}

// an ordered compaction step over the team: the rank of this lane's item among the flagged ones, n moves on; two barriers
template <class P> __host__ __device__ __forceinline__ int la_rank(P& par, LaShared& sh, bool v, int& n) {
    const unsigned long long m = par.ballot(v);
    if (par.lane() == 0) sh.wave_n[par.wave()] = (int)__builtin_popcountll(m);
    par.barrier();
    int off = n, tot = 0;
    for (int u = 0; u < P::NW; ++u) {
        if (u < par.wave()) off += sh.wave_n[u];
        tot += sh.wave_n[u];
    }
    n += tot;
    par.barrier();
    return off + (int)__builtin_popcountll(m & ((1ull << par.lane()) - 1ull));
}

// ---- step 1: the sets, the roles, the edges and the vertices from the tables (:72-272)
template <class P> __host__ __device__ __forceinline__ void la_prepare(const LaArgs& A, int g, LaShared& sh, P& par) {
    LaOff O;
    la_offsets(A, g, O);
    const LaView V = la_view(A, O);
    const int tid = par.tid(), F = A.F, L = A.L, T = A.T, kps = A.kp_stride;
    const uint8_t* loc = A.kf_local + (size_t)g * F;
    for (int f = tid; f < F; f += P::NT) {
        const bool er = A.kf_erased && A.kf_erased[f];
        sh.role[f] = (loc[f] && !er) ? ((A.kf_is_origin && A.kf_is_origin[f]) ? PLP_LOCAL_BA_KF_ORIGIN : PLP_LOCAL_BA_KF_FREE) : PLP_LOCAL_BA_KF_NONE;
        sh.fixed[f] = 0;
    }
    for (int t = tid; t < T; t += P::NT) { V.e_kf()[t] = -1; V.e_l()[t] = 0; V.lvl()[t] = 0; }
    if (tid == 0) sh.any = 0;
    par.barrier_g();
    for (int l = tid; l < L; l += P::NT) {
        int lo, hi;
        la_run(A, l, lo, hi);
        bool local = false;
        if (!(A.lm_erased && A.lm_erased[l]))
            for (int t = lo; t < hi && !local; ++t) {
                const int kf = A.obs_kf[t];
                local = (unsigned)kf < (unsigned)F && (sh.role[kf] == PLP_LOCAL_BA_KF_FREE || sh.role[kf] == PLP_LOCAL_BA_KF_ORIGIN);
            }
        V.lm_role()[l] = local ? 1 : 0;
        V.lm_act()[l] = 0;
        if (!local) continue;
        _Pragma("unroll") for (int i = 0; i < 3; ++i) la_l(V, l, kLaLmEst + i) = A.pos_w[(size_t)3 * l + i];
        for (int t = lo; t < hi; ++t) {
            const int kf = A.obs_kf[t];
            if ((unsigned)kf >= (unsigned)F || (A.kf_erased && A.kf_erased[kf])) continue;
            if (sh.role[kf] == PLP_LOCAL_BA_KF_NONE) sh.fixed[kf] = 1;
            int cnt = kps;
            if (A.counts) { cnt = A.counts[kf]; cnt = cnt < 0 ? 0 : cnt > kps ? kps : cnt; }
            const int idx = A.obs_idx[t];
            if ((unsigned)idx >= (unsigned)cnt) continue;
            const size_t s = (size_t)kf * kps + idx;
            const plp_keypoint* kp = A.undist + s;
            if ((unsigned)kp->octave >= (unsigned)A.num_levels) continue;
            V.e_kf()[t] = kf; V.e_l()[t] = l;
            la_e(V, t, kLaRowObs + 0) = (double)kp->x;
            la_e(V, t, kLaRowObs + 1) = (double)kp->y;
            la_e(V, t, kLaRowObs + 2) = (double)(A.x_right ? A.x_right[s] : -1.0f);
            la_e(V, t, kLaRowObs + 3) = (double)A.inv_sigma_sq[kp->octave];
            la_e(V, t, kLaRowChi) = 0.0;
            sh.any = 1;
        }
    }
    par.barrier_g();
    for (int f = tid; f < F; f += P::NT) {
        if (sh.role[f] == PLP_LOCAL_BA_KF_NONE && sh.fixed[f]) sh.role[f] = PLP_LOCAL_BA_KF_FIXED;
        V.kf_role()[f] = sh.role[f];
        if (sh.role[f] == PLP_LOCAL_BA_KF_NONE) continue;
        const double* in = A.pose + (size_t)f * A.pose_stride;
        double p12[12], est[7];
        _Pragma("unroll") for (int i = 0; i < 12; ++i) p12[i] = in[i];
        pose_est_from_pose(p12, est);
        _Pragma("unroll") for (int i = 0; i < 7; ++i) la_k(V, f, kLaKfEst + i) = est[i];
    }
    par.barrier();
    int n = 0;
    for (int base = 0; base < F; base += P::NT) {
        const int f = base + tid;
        const bool v = f < F && sh.role[f] == PLP_LOCAL_BA_KF_FREE;
        const int pos = la_rank(par, sh, v, n);
        if (v && pos < kLaMaxFree) V.hdr()[kLaHFl + pos] = f;
    }
    if (tid == 0) {
        V.hdr()[kLaHNf] = n;
        V.hdr()[kLaHStatus] = n > kLaMaxFree ? PLP_LOCAL_BA_TOO_MANY_FREE : sh.any ? PLP_LOCAL_BA_OK : PLP_LOCAL_BA_NO_EDGES;
        V.hdr()[kLaHCur] = 0;
        for (int i = 0; i < 8; ++i) V.hdr()[kLaHInfo + i] = 0;
        for (int i = 0; i < 4; ++i) V.hd()[i] = 0.0;
    }
}

// ---- the active sets of a round (initializeOptimization at level 0): the free key frames and landmarks with a level-0 edge, the list of every
// active pose's edges in edge order.  The extension's edges count into a pose's activity; its lists and its active vertices are its own.
template <class P, class AA, class X> __host__ __device__ __forceinline__ void la_round_setup(const AA& A, const LaView& V, LaShared& sh, P& par, X& ext) {
    const int tid = par.tid(), F = A.F, L = A.L, T = A.T, nf = V.hdr()[kLaHNf];
    for (int q = par.wave(); q < nf; q += P::NW) {
        const int kf = V.hdr()[kLaHFl + q];
        int c = 0;
        for (int base = 0; base < T; base += P::WS) {
            const int t = base + par.lane();
            const bool v = t < T && V.e_kf()[t] == kf && V.lvl()[t] == 0;
            c += (int)__builtin_popcountll(par.ballot(v));
        }
        if (par.lane() == 0) sh.cnt[q] = c;
    }
    ext.count(V, par);
    for (int f = tid; f < F; f += P::NT) sh.kf2ai[f] = -1;
    if (tid == 0) sh.nla = 0;
    par.barrier();
    if (tid == 0) {
        int a = 0, o = 0;
        for (int q = 0; q < nf; ++q)
            if (sh.cnt[q] + ext.cnt(q) > 0) {
                const int kf = V.hdr()[kLaHFl + q];
                sh.kf2ai[kf] = (int16_t)a; sh.akf[a] = kf; sh.aoff[a] = o; sh.acnt[a] = sh.cnt[q];
                ext.rank(a, q);
                o += sh.cnt[q]; ++a;
            }
        sh.nfa = a;
    }
    par.barrier();
    for (int a = par.wave(); a < sh.nfa; a += P::NW) {
        const int kf = sh.akf[a];
        int pos = sh.aoff[a];
        for (int base = 0; base < T; base += P::WS) {
            const int t = base + par.lane();
            const bool v = t < T && V.e_kf()[t] == kf && V.lvl()[t] == 0;
            const unsigned long long m = par.ballot(v);
            if (v) V.byp()[pos + (int)__builtin_popcountll(m & ((1ull << par.lane()) - 1ull))] = t;
            pos += (int)__builtin_popcountll(m);
        }
    }
    ext.place(par);
    for (int l = tid; l < L; l += P::NT) {
        bool act = false;
        if (V.lm_role()[l]) {
            int lo, hi;
            la_run(A, l, lo, hi);
            for (int t = lo; t < hi && !act; ++t) act = V.e_kf()[t] >= 0 && V.lvl()[t] == 0;
        }
        V.lm_act()[l] = act ? 1 : 0;
        if (act) sh.nla = 1;
    }
    ext.active(par);
    par.barrier_g();
}

// ---- one edge at the estimates (est, p): chi2 and the robust chi2 into its record E, and when lin its blocks (linearizeOplus,
// perspective_reproj_edge.cc:78-125, :166-214; BaseBinaryEdge::constructQuadraticForm); the pose block and W only for a free pose.  The local
// and the global adjuster (global_ba.hpp) both call this.
// is_free() is asked once, after the errors: whether the edge's pose is a free one.
template <class Free> __host__ __device__ __forceinline__ void la_edge_terms(double* E, const double* est, const double* p, const PoseCam& C, const double& delta, bool lin,
                                                                             bool robust, Free is_free) {
    const double ox = E[kLaRowObs + 0], oy = E[kLaRowObs + 1], orr = E[kLaRowObs + 2], w = E[kLaRowObs + 3];
    const bool mono = orr < 0.0;
    double x, y, z, e0, e1, e2;
    const double chi2 = pose_point_error(est, C, p, ox, oy, orr, mono, w, x, y, z, e0, e1, e2);
    double rho0 = chi2, rho1 = 1.0;
    if (robust) pose_huber(chi2, delta, rho0, rho1);
    E[kLaRowChi] = chi2;
    E[kLaRowRho] = rho0;
    if (!lin) return;
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
    const bool free_pose = is_free();
    if (free_pose) pose_terms(J, mono ? 2 : 3, e0, e1, e2, w, rho0, rho1, E, 1);
    double R[9], Jl[9];
    pose_rot_from_quat(est, R);
    _Pragma("unroll") for (int c = 0; c < 3; ++c) {
        Jl[c] = ((-C.fx) * R[c]) / z + ((C.fx * x) * R[6 + c]) / z_sq;
        Jl[3 + c] = ((-C.fy) * R[3 + c]) / z + ((C.fy * y) * R[6 + c]) / z_sq;
        Jl[6 + c] = Jl[c] - (C.fxb * R[6 + c]) / z_sq;
    }
    const double wr = rho1 * w;
    const double o0 = (-(w * e0)) * rho1, o1 = (-(w * e1)) * rho1, o2 = (-(w * e2)) * rho1;
    int k = 0;
    _Pragma("unroll") for (int i = 0; i < 3; ++i)
        _Pragma("unroll") for (int j = i; j < 3; ++j) {
            double v = Jl[i] * (wr * Jl[j]) + Jl[3 + i] * (wr * Jl[3 + j]);
            if (!mono) v = v + Jl[6 + i] * (wr * Jl[6 + j]);
            E[kLaRowLm + (k++)] = v;
        }
    _Pragma("unroll") for (int i = 0; i < 3; ++i) {
        double v = Jl[i] * o0 + Jl[3 + i] * o1;
        if (!mono) v = v + Jl[6 + i] * o2;
        E[kLaRowLm + 6 + i] = v;
    }
    if (free_pose)
        _Pragma("unroll") for (int i = 0; i < 6; ++i)
            _Pragma("unroll") for (int j = 0; j < 3; ++j) {
                double v = J[i] * (wr * Jl[j]) + J[6 + i] * (wr * Jl[3 + j]);
                if (!mono) v = v + J[12 + i] * (wr * Jl[6 + j]);
                E[kLaRowW + 3 * i + j] = v;
            }
}

// the sums of one landmark over the live edges [lo, hi) of its run in list order: the robust chi2, and when lin the nine terms of its block
template <class Live> __host__ __device__ __forceinline__ void la_lm_sums(const double* et, int lo, int hi, bool lin, Live live, double& part, double* s) {
    for (int t = lo; t < hi; ++t) {
        if (!live(t)) continue;
        part = part + et[(size_t)t * kLaEdgeRows + kLaRowRho];
        if (lin)
            _Pragma("unroll") for (int i = 0; i < 9; ++i) s[i] = s[i] + et[(size_t)t * kLaEdgeRows + kLaRowLm + i];
    }
}
// one of the 27 sums of a pose over its edge list in edge order
__host__ __device__ __forceinline__ double la_pose_sum(const double* et, const int32_t* list, int cnt, int term) {
    double acc = 0.0;
    for (int k = 0; k < cnt; ++k) acc = acc + et[(size_t)list[k] * kLaEdgeRows + term];
    return acc;
}

// ---- one pass over the level-0 edges at the estimates: la_edge_terms for every edge
template <class P, class AA> __host__ __device__ __forceinline__ void la_edge_pass(const AA& A, const LaView& V, LaShared& sh, P& par, bool lin, bool robust) {
    const int T = A.T, buf = lin ? sh.cur : 1 - sh.cur;     // a linearisation is at the kept estimates, an evaluation at the tried ones
    for (int t = par.tid(); t < T; t += P::NT) {
        const int kf = V.e_kf()[t];
        if (kf < 0 || V.lvl()[t]) continue;
        const int l = V.e_l()[t];
        double est[7], p[3];
        _Pragma("unroll") for (int i = 0; i < 7; ++i) est[i] = la_k(V, kf, 7 * buf + i);
        _Pragma("unroll") for (int i = 0; i < 3; ++i) p[i] = la_l(V, l, 3 * buf + i);
        la_edge_terms(V.et() + (size_t)t * kLaEdgeRows, est, p, sh.cam, sh.delta, lin, robust, [&sh, kf] { return sh.kf2ai[kf] >= 0; });
    }
    par.barrier_g();
}

// ---- the sums of a pass: every active landmark's robust chi2 (and its block when lin) over its level-0 edges in list order, every active
// pose's 27 sums over its edges in edge order
template <class P, class AA> __host__ __device__ __forceinline__ void la_sums(const AA& A, const LaView& V, LaShared& sh, P& par, bool lin) {
    const int L = A.L;
    for (int l = par.tid(); l < L; l += P::NT) {
        if (!V.lm_act()[l]) continue;
        int lo, hi;
        la_run(A, l, lo, hi);
        double part = 0.0, s[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        la_lm_sums(V.et(), lo, hi, lin, [&V](int t) { return !(V.e_kf()[t] < 0 || V.lvl()[t]); }, part, s);
        la_l(V, l, kLaLmPart) = part;
        if (lin)
            _Pragma("unroll") for (int i = 0; i < 9; ++i) la_l(V, l, kLaLmH + i) = s[i];
    }
    if (lin)
        for (int it = par.tid(); it < 27 * sh.nfa; it += P::NT) {
            const int a = it / 27, term = it % 27;
            la_p(V, a, term) = la_pose_sum(V.et(), V.byp() + sh.aoff[a], sh.acnt[a], term);
        }
    par.barrier_g();
}

// one chain over the n vertices of a table in table order, going on from sh.acc: every lane puts val(l) of its vertex (0 for one that is not
// active) into the tile, lane 0 adds the tile in order (mode 0) or takes its largest value (mode 1).  The result is in sh.acc after the closing
// barrier.
template <class P, class Val> __host__ __device__ __forceinline__ void la_chain_over(int n, LaShared& sh, P& par, int mode, Val val) {
    const int tid = par.tid();
    for (int base = 0; base < n; base += P::NT) {
        const int l = base + tid;
        sh.tile[tid] = l < n ? val(l) : 0.0;
        par.barrier();
        if (tid == 0) {
            const int cnt = n - base < P::NT ? n - base : P::NT;
            double acc = sh.acc;
            if (mode == 0) for (int i = 0; i < cnt; ++i) acc = acc + sh.tile[i];
            else for (int i = 0; i < cnt; ++i) acc = sh.tile[i] > acc ? sh.tile[i] : acc;
            sh.acc = acc;
        }
        par.barrier();
    }
}
// the chain over the active landmarks: mode 0 adds row `row` of the landmark table, mode 1 takes the largest |diagonal| of the landmark blocks
template <class P, class AA> __host__ __device__ __forceinline__ void la_chain(const AA& A, const LaView& V, LaShared& sh, P& par, int mode, int row) {
    la_chain_over(A.L, sh, par, mode, [&V, mode, row](int l) {
        double v = 0.0;
        if (V.lm_act()[l]) {
            if (mode == 0) v = la_l(V, l, row);
            else
                _Pragma("unroll") for (int i = 0; i < 3; ++i) {
                    const double d = __builtin_fabs(la_l(V, l, kLaLmH + (i == 0 ? 0 : i == 1 ? 3 : 5)));
                    v = d > v ? d : v;
                }
        }
        return v;
    });
}

// ---- one damped solve (BlockSolver<6,3>::solve): lambda on every diagonal, Hll^-1 closed, the Schur complement in the defined order, the
// Cholesky of the reduced system column by column, x_l = Hll^-1 (b_l - W^T x_p).  sh.ok = 0: a pivot or an inverse failed, every x is then zero.
// The extension's inverse, its Y, its subtractions and its x stand behind the landmarks'.
template <class P, class AA, class X> __host__ __device__ __forceinline__ void la_solve_system(const AA& A, const LaView& V, LaShared& sh, P& par, X& ext) {
    const int L = A.L, T = A.T, tid = par.tid(), nfa = sh.nfa, n = 6 * nfa;
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
    ext.inverse(par);
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
    ext.y(par);
    par.barrier_g();
    // the Schur complement: coefficient (r, c) of every block (i, j >= i) belongs to item (i, r, c), which walks pose i's edges in edge order and
    // for each the level-0 edges of its landmark in list order, then the extension's edges of pose i likewise; item (i, r, 6) owns the right-hand side
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
        ext.schur(V, i, r, c);
    }
    par.barrier_g();
    // Cholesky, one column and one barrier per step: row p of the factor is lane p's; L(p, k) takes the place of S(k, p).  After a failed pivot
    // the remaining columns are still walked (their values are not used: every x is zero then)
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
        par.barrier_g();                                     // no early exit on a failed pivot: a lane a column ahead may be the one that reports it
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
    ext.x(par, ok);
    par.barrier_g();
}

// the tried estimates (buffer 1 - cur) of every vertex of the problem from the kept ones: exp(x_p) * est and est + x_l for the active vertices,
// a copy for the others.  Accepting a step swaps the buffers; rejecting it needs nothing.
template <class P, class AA> __host__ __device__ __forceinline__ void la_update(const AA& A, const LaView& V, LaShared& sh, P& par) {
    const int F = A.F, L = A.L, kc = 7 * sh.cur, kt = 7 - kc, lc = 3 * sh.cur, lt = 3 - lc;
    for (int f = par.tid(); f < F; f += P::NT) {
        if (sh.role[f] == PLP_LOCAL_BA_KF_NONE) continue;
        const int a = sh.kf2ai[f];
        if (a < 0) {
            _Pragma("unroll") for (int i = 0; i < 7; ++i) la_k(V, f, kt + i) = la_k(V, f, kc + i);
            continue;
        }
        double bak[7], u[6], out[7];
        _Pragma("unroll") for (int i = 0; i < 7; ++i) bak[i] = la_k(V, f, kc + i);
        _Pragma("unroll") for (int i = 0; i < 6; ++i) u[i] = sh.x[6 * a + i];
        pose_oplus(u, bak, out);
        _Pragma("unroll") for (int i = 0; i < 7; ++i) la_k(V, f, kt + i) = out[i];
    }
    for (int l = par.tid(); l < L; l += P::NT) {
        if (!V.lm_role()[l]) continue;
        _Pragma("unroll") for (int i = 0; i < 3; ++i) {
            const double e = la_l(V, l, lc + i);
            la_l(V, l, lt + i) = V.lm_act()[l] ? e + la_l(V, l, kLaLmX + i) : e;
        }
    }
    par.barrier_g();
}

// computeScale over the 6 P + 3 M entries: one partial per vertex, the vertices in order (poses, then landmarks) on one accumulator
template <class P, class AA> __host__ __device__ __forceinline__ void la_scale(const AA& A, const LaView& V, LaShared& sh, P& par) {
    const int L = A.L;
    const double lambda = sh.lambda;
    for (int l = par.tid(); l < L; l += P::NT) {
        if (!V.lm_act()[l]) continue;
        double part = 0.0;
        _Pragma("unroll") for (int i = 0; i < 3; ++i) {
            const double x = la_l(V, l, kLaLmX + i);
            part = part + x * (lambda * x + la_l(V, l, kLaLmB + i));
        }
        la_l(V, l, kLaLmPart) = part;
    }
    if (par.tid() == 0) {
        double acc = 0.0;
        for (int a = 0; a < sh.nfa; ++a) {
            double part = 0.0;
            _Pragma("unroll") for (int i = 0; i < 6; ++i) part = part + sh.x[6 * a + i] * (lambda * sh.x[6 * a + i] + la_p(V, a, 21 + i));
            acc = acc + part;
        }
        sh.acc = acc;
    }
    par.barrier_g();
    la_chain(A, V, sh, par, 0, kLaLmPart);
}

// ---- one round of one problem (:286-335; with lines, local_bundle_adjuster_extended_line.cc:434-510): the active sets, the Levenberg-Marquardt
// loop and the round's record in the problem's header.  One body serves the linearisation and the evaluation of a tried step, chosen at run
// time.  Round 0 runs with the Huber kernels and ends with the edges that go to level 1; `round` is a literal or a loop counter of the caller.
template <class P, class AA, class X>
__host__ __device__ __forceinline__ void la_round(const AA& D, const LaView& V, LaShared& sh, P& par, X& ext, int round, const int& iters) {
    const int tid = par.tid();
    const bool robust = round == 0;
    la_round_setup(D, V, sh, par, ext);
    if (tid == 0) { sh.iterations = 0; sh.rejected = 0; sh.end = 0; sh.drops = 0; }
    par.barrier();
    int it = 0;
    bool lin = true;
    while (sh.nla || ext.any_active()) {
        if (!lin) {
            la_solve_system(D, V, sh, par, ext);
            la_update(D, V, sh, par);
            ext.update(par);
        } else {
            ext.perturb(V, par);
        }
        la_edge_pass(D, V, sh, par, lin, robust);
        ext.edge_pass(V, par, lin, robust);
        la_sums(D, V, sh, par, lin);
        ext.sums(V, par, lin);
        if (tid == 0) sh.acc = 0.0;
        par.barrier();
        la_chain(D, V, sh, par, 0, kLaLmPart);
        ext.chain(par, 0);
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
                ext.chain(par, 1);
                if (tid == 0) { sh.lambda = 1e-5 * sh.acc; sh.ni = 2.0; }
            }
            if (tid == 0) { sh.qmax = 0; sh.rho = 0.0; }
            par.barrier();
            lin = false;
            continue;
        }
        const double temp_sum = sh.acc;
        par.barrier();
        ext.scale_parts(par);
        la_scale(D, V, sh, par);
        ext.chain(par, 0);
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
        if (sh.end || it >= iters) break;
        lin = true;
    }
    if (round == 0) {                                        // :305-331: the edges that go to level 1, both kinds counted together
        const int T = D.T, kc = 7 * sh.cur, lc = 3 * sh.cur;
        int drops = 0;
        for (int t = tid; t < T; t += P::NT) {
            if (V.e_kf()[t] < 0) continue;
            const bool bad = la_point_bad(V, t, kc, lc);
            V.lvl()[t] = bad ? 1 : 0;
            drops += bad ? 1 : 0;
        }
        drops += ext.level1(V, par, kc);
        if (drops) par.add(sh.drops, drops);
    }
    par.barrier_g();
    if (tid == 0) {
        int32_t* ri = V.hdr() + kLaHInfo + 4 * round;
        ri[0] = sh.iterations; ri[1] = sh.rejected; ri[2] = sh.drops; ri[3] = sh.end ? sh.end : sh.iterations ? kLevEndIterations : 0;
        V.hd()[2 * round] = sh.current_chi; V.hd()[2 * round + 1] = sh.lambda;
        V.hdr()[kLaHCur] = sh.cur;
    }
}

// what a round reads of the camera and the Huber delta, into the shared state (lane 0)
__host__ __device__ __forceinline__ void la_round_consts(const LaArgs& A, LaShared& sh) {
    sh.cam.fx = A.cam.fx; sh.cam.fy = A.cam.fy; sh.cam.cx = A.cam.cx; sh.cam.cy = A.cam.cy; sh.cam.fxb = A.cam.fxb;   // field by field: a struct copy went through the stack
    sh.cam.k20 = A.cam.k20; sh.cam.k21 = A.cam.k21; sh.cam.k22 = A.cam.k22;
    sh.delta = A.mono_setup ? A.delta_2d : A.delta_3d; sh.ni = 2.0;
}

// ---- both rounds of one problem in one launch
template <class P> __host__ __device__ __forceinline__ void la_solve(const LaArgs& A, int g, LaShared& sh, P& par) {
    const int tid = par.tid();
    if (tid == 0) { la_offsets(A, g, sh.O); sh.D.F = A.F; sh.D.L = A.L; sh.D.T = A.T; }
    par.barrier();
    const LaView V = la_view(A, sh.O);
    const LaDimsView D{sh.D.F, sh.D.L, sh.D.T, A.obs_offsets};
    if (V.hdr()[kLaHStatus] != PLP_LOCAL_BA_OK) return;
    const int it1 = A.it1, it2 = A.it2;
    for (int f = tid; f < D.F; f += P::NT) sh.role[f] = V.kf_role()[f];
    if (tid == 0) { la_round_consts(A, sh); sh.lambda = 0.0; sh.current_chi = 0.0; sh.cur = 0; }
    par.barrier();
    LaNoLines none;
    for (int round = 0; round < 2; ++round) {
        const int iters = round == 0 ? it1 : it2;
        la_round(D, V, sh, par, none, round, iters);
        par.barrier();
    }
}

// ---- the outputs (:345-408): step [7]'s classification of every edge with the chi2 of its last evaluation and the depth at the final estimates
template <class P> __host__ __device__ __forceinline__ void la_finish(const LaArgs& A, int g, P& par) {
    LaOff O;
    la_offsets(A, g, O);
    const LaView V = la_view(A, O);
    const int tid = par.tid(), F = A.F, L = A.L, T = A.T;
    const int status = V.hdr()[kLaHStatus], kc = 7 * V.hdr()[kLaHCur], lc = 3 * V.hdr()[kLaHCur];
    if (tid == 0) A.out_status[g] = (uint8_t)status;
    if (status == PLP_LOCAL_BA_TOO_MANY_FREE) return;
    for (int f = tid; f < F; f += P::NT) {
        A.out_kf_role[(size_t)g * F + f] = V.kf_role()[f];
        if (V.kf_role()[f] != PLP_LOCAL_BA_KF_FREE) continue;
        double* out = A.out_pose + ((size_t)g * F + f) * 15;
        if (status == PLP_LOCAL_BA_NO_EDGES) {
            const double* in = A.pose + (size_t)f * A.pose_stride;
            _Pragma("unroll") for (int i = 0; i < 12; ++i) out[i] = in[i];
            _Pragma("unroll") for (int i = 0; i < 3; ++i) out[12 + i] = ((-in[i]) * in[9] + (-in[3 + i]) * in[10]) + (-in[6 + i]) * in[11];
            continue;
        }
        double est[7], p15[15];
        _Pragma("unroll") for (int i = 0; i < 7; ++i) est[i] = la_k(V, f, kc + i);
        pose_pose_from_est(est, p15);
        for (int i = 0; i < 15; ++i) out[i] = p15[i];
    }
    for (int l = tid; l < L; l += P::NT) {
        A.out_lm_role[(size_t)g * L + l] = V.lm_role()[l];
        if (!V.lm_role()[l]) continue;
        _Pragma("unroll") for (int i = 0; i < 3; ++i) A.out_pos_w[((size_t)g * L + l) * 3 + i] = la_l(V, l, lc + i);
    }
    for (int t = tid; t < T; t += P::NT) {
        if (V.e_kf()[t] < 0) continue;
        A.out_outlier[(size_t)g * T + t] = la_point_bad(V, t, kc, lc) ? 1 : 0;
    }
    if (tid == 0) {
        if (A.out_round_info) for (int i = 0; i < 8; ++i) A.out_round_info[(size_t)8 * g + i] = V.hdr()[kLaHInfo + i];
        if (A.out_round_chi2) for (int i = 0; i < 4; ++i) A.out_round_chi2[(size_t)4 * g + i] = V.hd()[i];
    }
}

hipError_t launch_local_ba(hipStream_t st, const LaArgs& A);

}  // namespace plp
