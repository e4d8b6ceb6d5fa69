// optimize::global_bundle_adjuster::optimize (optimize/global_bundle_adjuster.cc:64-311) and the array half of module::loop_bundle_adjuster's map
// update (module/loop_bundle_adjuster.cc:109-181), one definition for host and device (plp_global_ba_* / plp_loop_ba_propagate_* / plp_model_*_host,
// include/plp_front.h) on top of local_ba.hpp (D17): the edge arithmetic, the sums, the 3 x 3 inverse and the tables' rows are
// D17's own functions; levenberg.hpp decides a step.  f64 with IEEE + - * / sqrt only, in the order written; -ffp-contract=off.
//
// One problem uses the whole device, so the steps are written per ITEM (one key frame, landmark, edge, pose sum, Schur coefficient): a kernel gives
// every item a lane of its grid, the host build walks the items in a loop.  No sum depends on how the items are spread: every coefficient is owned
// by one item that adds its terms in the defined order.  The few serial steps (the chains, the step decision) are written over a team of lanes as
// local_ba.hpp's are and run in one workgroup.  The dense Cholesky and the substitutions have a plain host form here and a panel form in
// global_ba_kernels.hip; both subtract every coefficient's terms from one accumulator with k ascending (descending in the back substitution).
#pragma once
#include <vector>

#include "local_ba.hpp"

namespace plp {

constexpr int kGbMaxKf = PLP_GLOBAL_BA_MAX_KF;         // F
constexpr int kGbMaxLm = 1 << 20;                      // L
constexpr int kGbMaxObs = 1 << 22;                     // T
constexpr int kGbPanel = PLP_GLOBAL_BA_PANEL;          // columns of a Cholesky panel
constexpr int kGbRows = PLP_GLOBAL_BA_ROWS;            // rows of a workgroup of the rows-below launch
constexpr int kGbThreads = 256;                        // the workgroup of every kernel

// the Levenberg record of the run: device memory that every kernel reads; the entry reads it back after the prepare launches and after every try
struct GbRec {
    double lambda, ni, current_chi, rho, init_chi, temp_sum, scale;
    int32_t status, P, any, cur, ok, qmax, iterations, rejected, go_on, end, factorisations, pad;
};

struct GbArgs {
    int F, L, T, kp_stride, pose_stride, num_levels, robust, n;
    PoseCam cam;
    double delta;
    float inv_sigma_sq[16];
    const double* pose; const uint8_t* kf_erased; const uint8_t* kf_is_origin; const plp_keypoint* undist; const float* x_right; const int32_t* counts;
    const double* pos_w; const uint8_t* lm_erased; const int32_t* obs_offsets; const int32_t* obs_kf; const int32_t* obs_idx;
    uint8_t* out_status; uint8_t* out_kf_optimized; uint8_t* out_lm_optimized; double* out_pose; double* out_pos_w; int32_t* out_info; double* out_chi2;
    // what the steps hand to one another: D17's edge [T][78], landmark [L][25] and key-frame [F][14] tables, the pose sums [F][27], x_p [6 F] (the
    // reduced right-hand side before the substitutions), S [n][n] row-major, its upper triangle; L(p, k) takes the place of S(k, p)
    double* et; double* lm; double* kf; double* pv; double* x; double* S;
    int32_t* e_l; int32_t* e_kf; int32_t* byp; int32_t* cnt; int32_t* aoff; int32_t* akf; int32_t* kf2ai;
    uint8_t* lm_act; uint8_t* role;
    GbRec* rec;
};
__host__ __device__ __forceinline__ size_t gb_doubles(int F, int L, int T) { return (size_t)kLaEdgeRows * T + (size_t)kLaLmRows * L + (size_t)(kLaKfRows + 27 + 6) * F + 8; }
__host__ __device__ __forceinline__ size_t gb_ints(int F, int T) { return (size_t)3 * T + (size_t)4 * F + 8; }
__host__ __device__ __forceinline__ size_t gb_bytes(int F, int L) { return (size_t)L + F + 8; }
inline void gb_bind(GbArgs& A, double* d, int32_t* i, uint8_t* b) {
    A.et = d; A.lm = A.et + (size_t)kLaEdgeRows * A.T; A.kf = A.lm + (size_t)kLaLmRows * A.L; A.pv = A.kf + (size_t)kLaKfRows * A.F; A.x = A.pv + (size_t)27 * A.F;
    A.e_l = i; A.e_kf = A.e_l + A.T; A.byp = A.e_kf + A.T; A.cnt = A.byp + A.T; A.aoff = A.cnt + A.F; A.akf = A.aoff + A.F + 1; A.kf2ai = A.akf + A.F;
    A.lm_act = b; A.role = A.lm_act + A.L;
}

__host__ __device__ __forceinline__ double& gb_e(const GbArgs& A, int t, int row) { return A.et[(size_t)t * kLaEdgeRows + row]; }
__host__ __device__ __forceinline__ double& gb_l(const GbArgs& A, int l, int row) { return A.lm[(size_t)l * kLaLmRows + row]; }
__host__ __device__ __forceinline__ double& gb_k(const GbArgs& A, int f, int row) { return A.kf[(size_t)f * kLaKfRows + row]; }

// the integer adds of the prepare step: plain on the host, atomic on the device (a count does not depend on the order)
struct GbAddHost { __host__ __device__ void operator()(int32_t* p) const { *p += 1; } };

__host__ __device__ __forceinline__ void gb_rec_init(const GbArgs& A) {
    GbRec& R = *A.rec;
    R.lambda = 0.0; R.ni = 2.0; R.current_chi = 0.0; R.rho = 0.0; R.init_chi = 0.0; R.temp_sum = 0.0; R.scale = 0.0;
    R.status = PLP_GLOBAL_BA_OK; R.P = 0; R.any = 0; R.cur = 0; R.ok = 1; R.qmax = 0; R.iterations = 0; R.rejected = 0; R.go_on = 0; R.end = 0; R.factorisations = 0; R.pad = 0;
}

// ---- the sets (:91-184).  Item f: the role of key frame f (every key frame that is not erased is a vertex, the origin a constant one), its estimate
// in both buffers
__host__ __device__ __forceinline__ void gb_kf_item(const GbArgs& A, int f) {
    const bool er = A.kf_erased && A.kf_erased[f];
    const int role = er ? PLP_LOCAL_BA_KF_NONE : (A.kf_is_origin && A.kf_is_origin[f]) ? PLP_LOCAL_BA_KF_ORIGIN : PLP_LOCAL_BA_KF_FREE;
    A.role[f] = (uint8_t)role;
    A.cnt[f] = 0; A.kf2ai[f] = -1;
    if (er) return;
    const double* in = A.pose + (size_t)f * A.pose_stride;
    double p12[12], est[7];
    _Pragma("unroll") for (int i = 0; i < 12; ++i) p12[i] = in[i];
    pose_est_from_pose(p12, est);
    _Pragma("unroll") for (int i = 0; i < 7; ++i) { gb_k(A, f, kLaKfEst + i) = est[i]; gb_k(A, f, kLaKfEst1 + i) = est[i]; }
}
__host__ __device__ __forceinline__ void gb_edge_clear(const GbArgs& A, int t) { A.e_kf[t] = -1; A.e_l[t] = 0; }

// Item l: the edges of landmark l's run with their measurements (D17 item 7's rules), its estimate; the edge count of every key frame
template <class Add> __host__ __device__ __forceinline__ void gb_lm_item(const GbArgs& A, int l, Add add) {
    int lo, hi;
    la_run(A, l, lo, hi);
    bool act = false;
    if (!(A.lm_erased && A.lm_erased[l]))
        for (int t = lo; t < hi; ++t) {
            const int kf = A.obs_kf[t];
            if ((unsigned)kf >= (unsigned)A.F || (A.kf_erased && A.kf_erased[kf])) continue;
            int cnt = A.kp_stride;
            if (A.counts) { cnt = A.counts[kf]; cnt = cnt < 0 ? 0 : cnt > A.kp_stride ? A.kp_stride : cnt; }
            const int idx = A.obs_idx[t];
            if ((unsigned)idx >= (unsigned)cnt) continue;
            const size_t s = (size_t)kf * A.kp_stride + idx;
            const plp_keypoint* kp = A.undist + s;
            if ((unsigned)kp->octave >= (unsigned)A.num_levels) continue;
            A.e_kf[t] = kf; A.e_l[t] = l;
            gb_e(A, t, kLaRowObs + 0) = (double)kp->x;
            gb_e(A, t, kLaRowObs + 1) = (double)kp->y;
            gb_e(A, t, kLaRowObs + 2) = (double)(A.x_right ? A.x_right[s] : -1.0f);
            gb_e(A, t, kLaRowObs + 3) = (double)A.inv_sigma_sq[kp->octave];
            gb_e(A, t, kLaRowChi) = 0.0;
            add(A.cnt + kf);
            act = true;
        }
    A.lm_act[l] = act ? 1 : 0;
    if (!act) return;
    A.rec->any = 1;
    _Pragma("unroll") for (int i = 0; i < 3; ++i) { gb_l(A, l, kLaLmEst + i) = A.pos_w[(size_t)3 * l + i]; gb_l(A, l, kLaLmEst1 + i) = A.pos_w[(size_t)3 * l + i]; }
}

// One lane: the free key frames with an edge ranked in table order (the rows of the reduced system), where each one's edge list begins
__host__ __device__ __forceinline__ void gb_rank(const GbArgs& A) {
    int a = 0, o = 0;
    for (int f = 0; f < A.F; ++f) {
        if (A.role[f] != PLP_LOCAL_BA_KF_FREE || A.cnt[f] <= 0) continue;
        A.kf2ai[f] = a; A.akf[a] = f; A.aoff[a] = o;
        o += A.cnt[f]; ++a;
    }
    A.aoff[a] = o;
    A.rec->P = a;
    A.rec->status = A.rec->any ? PLP_GLOBAL_BA_OK : PLP_GLOBAL_BA_NO_EDGES;
}
// the edge list of pose a in edge order (the host form; the kernel scans the edge table with a wave's ballots)
inline void gb_fill_host(const GbArgs& A, int a) {
    int pos = A.aoff[a];
    for (int t = 0; t < A.T; ++t)
        if (A.e_kf[t] == A.akf[a]) A.byp[pos++] = t;
}

// ---- a pass.  Item t: edge t at the kept (lin) or the tried estimates
__host__ __device__ __forceinline__ void gb_edge_item(const GbArgs& A, int t, bool lin) {
    const int kf = A.e_kf[t];
    if (kf < 0) return;
    const int l = A.e_l[t], buf = lin ? A.rec->cur : 1 - A.rec->cur;
    double est[7], p[3];
    _Pragma("unroll") for (int i = 0; i < 7; ++i) est[i] = gb_k(A, kf, 7 * buf + i);
    _Pragma("unroll") for (int i = 0; i < 3; ++i) p[i] = gb_l(A, l, 3 * buf + i);
    la_edge_terms(A.et + (size_t)t * kLaEdgeRows, est, p, A.cam, A.delta, lin, A.robust != 0, [&A, kf] { return A.kf2ai[kf] >= 0; });
}
// Item l: landmark l's sums over its run
__host__ __device__ __forceinline__ void gb_lm_sum_item(const GbArgs& A, int l, bool lin) {
    if (!A.lm_act[l]) return;
    int lo, hi;
    la_run(A, l, lo, hi);
    double part = 0.0, s[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    la_lm_sums(A.et, lo, hi, lin, [&A](int t) { return A.e_kf[t] >= 0; }, part, s);
    gb_l(A, l, kLaLmPart) = part;
    if (lin)
        _Pragma("unroll") for (int i = 0; i < 9; ++i) gb_l(A, l, kLaLmH + i) = s[i];
}
// Item (a, term): one of pose a's 27 sums over its edge list
__host__ __device__ __forceinline__ void gb_pose_sum_item(const GbArgs& A, int it) {
    const int a = it / 27, term = it % 27;
    A.pv[(size_t)a * 27 + term] = la_pose_sum(A.et, A.byp + A.aoff[a], A.aoff[a + 1] - A.aoff[a], term);
}

// ---- the damped solve.  Item l: Hll + lambda I inverted
__host__ __device__ __forceinline__ void gb_inv_item(const GbArgs& A, int l) {
    if (!A.lm_act[l]) return;
    const double lambda = A.rec->lambda;
    double a[6], o[6];
    _Pragma("unroll") for (int i = 0; i < 6; ++i) a[i] = gb_l(A, l, kLaLmH + i);
    a[0] = a[0] + lambda; a[3] = a[3] + lambda; a[5] = a[5] + lambda;
    if (!la_inv3(a, o)) A.rec->ok = 0;
    _Pragma("unroll") for (int i = 0; i < 6; ++i) gb_l(A, l, kLaLmInv + i) = o[i];
}
// Item t: Y = W Hll^-1 of an edge with a free pose
__host__ __device__ __forceinline__ void gb_y_item(const GbArgs& A, int t) {
    const int kf = A.e_kf[t];
    if (kf < 0 || A.kf2ai[kf] < 0) return;
    const int l = A.e_l[t];
    double h[6];
    _Pragma("unroll") for (int i = 0; i < 6; ++i) h[i] = gb_l(A, l, kLaLmInv + i);
    _Pragma("unroll") for (int r = 0; r < 6; ++r) {
        const double w0 = gb_e(A, t, kLaRowW + 3 * r), w1 = gb_e(A, t, kLaRowW + 3 * r + 1), w2 = gb_e(A, t, kLaRowW + 3 * r + 2);
        gb_e(A, t, kLaRowY + 3 * r) = (w0 * h[0] + w1 * h[1]) + w2 * h[2];
        gb_e(A, t, kLaRowY + 3 * r + 1) = (w0 * h[1] + w1 * h[3]) + w2 * h[4];
        gb_e(A, t, kLaRowY + 3 * r + 2) = (w0 * h[2] + w1 * h[4]) + w2 * h[5];
    }
}
// Item (i, r, c): coefficient (r, c) of every block (i, j >= i) of S -- from H_pp + lambda I, then D17's walk over pose i's edges in edge order and
// for each the edges of its landmark in list order; c == 6 owns b_red(6 i + r), which starts as b_p.  Nothing else writes these coefficients.
__host__ __device__ __forceinline__ void gb_schur_item(const GbArgs& A, int i, int r, int c) {
    const int P = A.rec->P, n = 6 * P;
    const double lambda = A.rec->lambda;
    const int32_t* list = A.byp + A.aoff[i];
    const int cnt = A.aoff[i + 1] - A.aoff[i];
    if (c == 6) {
        double b = A.pv[(size_t)i * 27 + 21 + r];
        for (int k = 0; k < cnt; ++k) {
            const int ta = list[k], l = A.e_l[ta];
            const double y0 = gb_e(A, ta, kLaRowY + 3 * r), y1 = gb_e(A, ta, kLaRowY + 3 * r + 1), y2 = gb_e(A, ta, kLaRowY + 3 * r + 2);
            b = b - ((y0 * gb_l(A, l, kLaLmB + 0) + y1 * gb_l(A, l, kLaLmB + 1)) + y2 * gb_l(A, l, kLaLmB + 2));
        }
        A.x[6 * i + r] = b;
        return;
    }
    double* row = A.S + (size_t)(6 * i + r) * n;
    for (int j = i; j < P; ++j) {
        double v = 0.0;
        if (j == i && c >= r) {
            v = A.pv[(size_t)i * 27 + lev_h_index<6>(r, c)];
            if (r == c) v = v + lambda;
        }
        row[6 * j + c] = v;
    }
    for (int k = 0; k < cnt; ++k) {
        const int ta = list[k], l = A.e_l[ta];
        const double y0 = gb_e(A, ta, kLaRowY + 3 * r), y1 = gb_e(A, ta, kLaRowY + 3 * r + 1), y2 = gb_e(A, ta, kLaRowY + 3 * r + 2);
        int lo, hi;
        la_run(A, l, lo, hi);
        for (int tb = lo; tb < hi; ++tb) {
            const int kfb = A.e_kf[tb];
            if (kfb < 0) continue;
            const int j = A.kf2ai[kfb];
            if (j < i || (j == i && c < r)) continue;
            double* s = row + 6 * j + c;
            *s = *s - ((y0 * gb_e(A, tb, kLaRowW + 3 * c) + y1 * gb_e(A, tb, kLaRowW + 3 * c + 1)) + y2 * gb_e(A, tb, kLaRowW + 3 * c + 2));
        }
    }
}

// The dense Cholesky in natural order, the host form: row j of the factor from the rows above it, k ascending for every coefficient
// (L_jj = sqrt(A_jj - sum_k L_jk^2), L_pj = (A_pj - sum_k L_pk L_jk) / L_jj; the accumulator of (p, j) is S(j, p) itself).  false: a pivot failed.
inline bool gb_chol_host(double* S, int n) {
    for (int j = 0; j < n; ++j) {
        double* rj = S + (size_t)j * n;
        for (int k = 0; k < j; ++k) {
            const double* rk = S + (size_t)k * n;
            const double ljk = rk[j];
            for (int p = j; p < n; ++p) rj[p] = rj[p] - rk[p] * ljk;
        }
        const double s = rj[j];
        if (!(s > 0.0) || s > kLevDblMax) return false;
        const double d = __builtin_sqrt(s);
        rj[j] = d;
        for (int p = j + 1; p < n; ++p) rj[p] = rj[p] / d;
    }
    return true;
}
// forward substitution with k ascending, back substitution with k descending, in place on v
inline void gb_subst_host(const double* S, int n, double* v) {
    for (int j = 0; j < n; ++j) {
        v[j] = v[j] / S[(size_t)j * n + j];
        for (int p = j + 1; p < n; ++p) v[p] = v[p] - S[(size_t)j * n + p] * v[j];
    }
    for (int j = n - 1; j >= 0; --j) {
        v[j] = v[j] / S[(size_t)j * n + j];
        for (int p = 0; p < j; ++p) v[p] = v[p] - S[(size_t)p * n + j] * v[j];
    }
}

// Item l: x_l = Hll^-1 (b_l - W^T x_p); zero after a failed solve
__host__ __device__ __forceinline__ void gb_xl_item(const GbArgs& A, int l) {
    if (!A.lm_act[l]) return;
    double t3[3] = {0.0, 0.0, 0.0};
    if (A.rec->ok) {
        int lo, hi;
        la_run(A, l, lo, hi);
        _Pragma("unroll") for (int i = 0; i < 3; ++i) t3[i] = gb_l(A, l, kLaLmB + i);
        for (int t = lo; t < hi; ++t) {
            const int kf = A.e_kf[t];
            if (kf < 0) continue;
            const int j = A.kf2ai[kf];
            if (j < 0) continue;
            _Pragma("unroll") for (int i = 0; i < 3; ++i) {
                double d = gb_e(A, t, kLaRowW + i) * A.x[6 * j];
                _Pragma("unroll") for (int r = 1; r < 6; ++r) d = d + gb_e(A, t, kLaRowW + 3 * r + i) * A.x[6 * j + r];
                t3[i] = t3[i] - d;
            }
        }
        double h[6];
        _Pragma("unroll") for (int i = 0; i < 6; ++i) h[i] = gb_l(A, l, kLaLmInv + i);
        const double x0 = (h[0] * t3[0] + h[1] * t3[1]) + h[2] * t3[2], x1 = (h[1] * t3[0] + h[3] * t3[1]) + h[4] * t3[2], x2 = (h[2] * t3[0] + h[4] * t3[1]) + h[5] * t3[2];
        t3[0] = x0; t3[1] = x1; t3[2] = x2;
    }
    const int lc = 3 * A.rec->cur, lt = 3 - lc;
    _Pragma("unroll") for (int i = 0; i < 3; ++i) {
        gb_l(A, l, kLaLmX + i) = t3[i];
        gb_l(A, l, lt + i) = gb_l(A, l, lc + i) + t3[i];       // the tried estimate
    }
}
// Item a: the tried estimate of free pose a, exp(x_p) * est
__host__ __device__ __forceinline__ void gb_update_item(const GbArgs& A, int a) {
    const int f = A.akf[a], kc = 7 * A.rec->cur, kt = 7 - kc;
    double bak[7], u[6], out[7];
    _Pragma("unroll") for (int i = 0; i < 7; ++i) bak[i] = gb_k(A, f, kc + i);
    _Pragma("unroll") for (int i = 0; i < 6; ++i) u[i] = A.x[6 * a + i];
    pose_oplus(u, bak, out);
    _Pragma("unroll") for (int i = 0; i < 7; ++i) gb_k(A, f, kt + i) = out[i];
}

// ---- the serial steps, over a team of lanes (one workgroup; the host build's team is LaTeamHost).  An ordered chain: count terms fn(i) added
// to acc in index order by lane 0 (the value is lane 0's)
template <class P, class Fn> __host__ __device__ __forceinline__ double gb_chain(P& par, double* tile, int count, double acc, Fn fn) {
    const int tid = par.tid();
    for (int base = 0; base < count; base += P::NT) {
        const int i = base + tid;
        tile[tid] = i < count ? fn(i) : 0.0;
        par.barrier();
        if (tid == 0) {
            const int cnt = count - base < P::NT ? count - base : P::NT;
            for (int k = 0; k < cnt; ++k) acc = acc + tile[k];
        }
        par.barrier();
    }
    return acc;
}
// the largest fn(i) with NaN dropped (no order: a maximum over values that are not NaN does not depend on it); lane 0's value
template <class P, class Fn> __host__ __device__ __forceinline__ double gb_max(P& par, double* tile, int count, double m, Fn fn) {
    const int tid = par.tid();
    double v = 0.0;
    for (int i = tid; i < count; i += P::NT) { const double d = fn(i); v = d > v ? d : v; }
    tile[tid] = v;
    par.barrier();
    if (tid == 0)
        for (int k = 0; k < P::NT; ++k) m = tile[k] > m ? tile[k] : m;
    par.barrier();
    return m;
}
// after a linearisation: currentChi, and at iteration 0 computeLambdaInit over every active vertex
template <class P> __host__ __device__ __forceinline__ void gb_begin(const GbArgs& A, P& par, double* tile, int iteration) {
    GbRec& R = *A.rec;
    const double chi = gb_chain(par, tile, A.L, 0.0, [&A](int l) { return A.lm_act[l] ? gb_l(A, l, kLaLmPart) : 0.0; });
    double m = 0.0;
    if (iteration == 0) {
        m = gb_max(par, tile, 6 * R.P, 0.0, [&A](int i) { return __builtin_fabs(A.pv[(size_t)(i / 6) * 27 + lev_h_index<6>(i % 6, i % 6)]); });
        m = gb_max(par, tile, 3 * A.L, m, [&A](int i) { const int l = i / 3, k = i % 3; return A.lm_act[l] ? __builtin_fabs(gb_l(A, l, kLaLmH + (k == 0 ? 0 : k == 1 ? 3 : 5))) : 0.0; });
    }
    if (par.tid() == 0) {
        R.current_chi = chi;
        if (iteration == 0) { R.lambda = 1e-5 * m; R.ni = 2.0; R.init_chi = chi; }
        R.qmax = 0; R.rho = 0.0; R.ok = 1;
    }
}
// after the evaluation of a tried step: its chi2, computeScale, g2o's decision; the next try starts with ok = 1
template <class P> __host__ __device__ __forceinline__ void gb_decide(const GbArgs& A, P& par, double* tile) {
    GbRec& R = *A.rec;
    const double lambda = R.lambda;
    const double temp_sum = gb_chain(par, tile, A.L, 0.0, [&A](int l) { return A.lm_act[l] ? gb_l(A, l, kLaLmPart) : 0.0; });
    double scale = gb_chain(par, tile, R.P, 0.0, [&A, lambda](int a) {
        double part = 0.0;
        _Pragma("unroll") for (int i = 0; i < 6; ++i) part = part + A.x[6 * a + i] * (lambda * A.x[6 * a + i] + A.pv[(size_t)a * 27 + 21 + i]);
        return part;
    });
    scale = gb_chain(par, tile, A.L, scale, [&A, lambda](int l) {
        double part = 0.0;
        if (A.lm_act[l])
            _Pragma("unroll") for (int i = 0; i < 3; ++i) {
                const double x = gb_l(A, l, kLaLmX + i);
                part = part + x * (lambda * x + gb_l(A, l, kLaLmB + i));
            }
        return part;
    });
    if (par.tid() == 0) {
        R.temp_sum = temp_sum; R.scale = scale;
        R.factorisations += 1;
        lev_decide(R, R.ok != 0, temp_sum, scale, [&R] { R.cur = 1 - R.cur; }, [] {});
        if (!R.go_on) {
            R.iterations += 1;
            R.end = lev_end(R);
        }
        R.ok = 1;
    }
}

// ---- the outputs (:262-311).  Item f: out_pose of every key frame that is not erased; item l: out_pos_w of the optimised landmarks
__host__ __device__ __forceinline__ void gb_out_kf_item(const GbArgs& A, int f) {
    const bool vertex = A.role[f] != PLP_LOCAL_BA_KF_NONE;
    A.out_kf_optimized[f] = vertex ? 1 : 0;
    if (!vertex) return;
    double* out = A.out_pose + (size_t)f * 15;
    if (A.rec->status == PLP_GLOBAL_BA_NO_EDGES) {
        const double* in = A.pose + (size_t)f * A.pose_stride;
        _Pragma("unroll") for (int i = 0; i < 12; ++i) out[i] = in[i];
        _Pragma("unroll") for (int i = 0; i < 3; ++i) out[12 + i] = ((-in[i]) * in[9] + (-in[3 + i]) * in[10]) + (-in[6 + i]) * in[11];
        return;
    }
    const int kc = A.kf2ai[f] >= 0 ? 7 * A.rec->cur : 0;          // a vertex without an edge and the origin keep the converted input
    double est[7], p15[15];
    _Pragma("unroll") for (int i = 0; i < 7; ++i) est[i] = gb_k(A, f, kc + i);
    pose_pose_from_est(est, p15);
    for (int i = 0; i < 15; ++i) out[i] = p15[i];
}
__host__ __device__ __forceinline__ void gb_out_lm_item(const GbArgs& A, int l) {
    A.out_lm_optimized[l] = A.lm_act[l];
    if (!A.lm_act[l]) return;
    const int lc = 3 * A.rec->cur;
    _Pragma("unroll") for (int i = 0; i < 3; ++i) A.out_pos_w[(size_t)3 * l + i] = gb_l(A, l, lc + i);
}
__host__ __device__ __forceinline__ void gb_out_rec(const GbArgs& A, bool stopped) {
    const GbRec& R = *A.rec;
    if (stopped) { A.out_status[0] = PLP_GLOBAL_BA_STOPPED; return; }
    A.out_status[0] = (uint8_t)R.status;
    if (A.out_info) {
        A.out_info[0] = R.iterations; A.out_info[1] = R.rejected; A.out_info[2] = R.factorisations;
        A.out_info[3] = R.end ? R.end : R.iterations ? kLevEndIterations : 0;
    }
    if (A.out_chi2) { A.out_chi2[0] = R.init_chi; A.out_chi2[1] = R.current_chi; A.out_chi2[2] = R.lambda; }
}

// what the entry does between the launches: the loop of OptimizationAlgorithmLevenberg::solve inside SparseOptimizer::optimize, as la_solve walks
// it for one round.  D is the driver: D.lin(it) runs a linearisation (edge pass, sums, gb_begin), D.try_step() one damped solve, the update, the
// evaluation and gb_decide and returns the record; `stop` is read before every iteration and before every try.
template <class D> void gb_loop(D& drv, int iters, const volatile int32_t* stop) {
    for (int it = 0; it < iters; ++it) {
        if (stop && *stop) return;
        drv.lin(it);
        for (;;) {
            if (stop && *stop) return;
            const GbRec r = drv.try_step();
            if (!r.go_on) { if (r.end) return; break; }
        }
    }
}

// the host build: the same items in loops, a team of one lane for the serial steps
struct GbHostDriver {
    GbArgs& A; int P; double tile[1];
    void pass(bool lin) {
        for (int t = 0; t < A.T; ++t) gb_edge_item(A, t, lin);
        for (int l = 0; l < A.L; ++l) gb_lm_sum_item(A, l, lin);
    }
    void lin(int it) {
        pass(true);
        for (int k = 0; k < 27 * P; ++k) gb_pose_sum_item(A, k);
        LaTeamHost par;
        gb_begin(A, par, tile, it);
    }
    GbRec try_step() {
        for (int l = 0; l < A.L; ++l) gb_inv_item(A, l);
        if (P > 0) {
            for (int t = 0; t < A.T; ++t) gb_y_item(A, t);
            for (int k = 0; k < 42 * P; ++k) gb_schur_item(A, k / 42, (k % 42) / 7, k % 7);
            if (A.rec->ok && !gb_chol_host(A.S, A.n)) A.rec->ok = 0;
            if (A.rec->ok) gb_subst_host(A.S, A.n, A.x);
            else for (int p = 0; p < A.n; ++p) A.x[p] = 0.0;
        }
        for (int l = 0; l < A.L; ++l) gb_xl_item(A, l);
        for (int a = 0; a < P; ++a) gb_update_item(A, a);
        pass(false);
        LaTeamHost par;
        gb_decide(A, par, tile);
        return *A.rec;
    }
};

inline void gb_run_host(GbArgs& A, int iters, const volatile int32_t* stop) {
    std::vector<double> d(gb_doubles(A.F, A.L, A.T), 0.0), S;
    std::vector<int32_t> i(gb_ints(A.F, A.T), 0);
    std::vector<uint8_t> b(gb_bytes(A.F, A.L), 0);
    GbRec rec{};
    gb_bind(A, d.data(), i.data(), b.data());
    A.rec = &rec;
    const bool stopped = stop && *stop;                  // the host builds take the flag as a constant
    gb_rec_init(A);
    for (int f = 0; f < A.F; ++f) gb_kf_item(A, f);
    for (int t = 0; t < A.T; ++t) gb_edge_clear(A, t);
    for (int l = 0; l < A.L; ++l) gb_lm_item(A, l, GbAddHost());
    gb_rank(A);
    if (rec.status == PLP_GLOBAL_BA_OK && !stopped) {
        A.n = 6 * rec.P;
        S.assign((size_t)A.n * A.n, 0.0);
        A.S = S.data();
        for (int a = 0; a < rec.P; ++a) gb_fill_host(A, a);
        GbHostDriver drv{A, rec.P};
        gb_loop(drv, iters, nullptr);
    }
    if (!stopped) {
        for (int f = 0; f < A.F; ++f) gb_out_kf_item(A, f);
        for (int l = 0; l < A.L; ++l) gb_out_lm_item(A, l);
    }
    gb_out_rec(A, stopped);
}

// ---- the loop adjuster's map update (module/loop_bundle_adjuster.cc:109-181), its array half
struct LpArgs {
    int F, L, pose_stride;
    const double* pose; const uint8_t* kf_erased; const uint8_t* kf_is_origin; const int32_t* kf_parent; const uint8_t* kf_optimized; const double* pose_after;
    const double* pos_w; const uint8_t* lm_erased; const int32_t* ref_kf; const uint8_t* lm_optimized; const double* pos_after;
    double* out_pose; double* out_pose_before; uint8_t* out_kf_status; double* out_pos_w; uint8_t* out_lm_status;
};
// c = a * b of affine 3 x 4 maps (rotation row-major, then the translation): rotation entries three-term sums left to right, translation (R_a t_b) + t_a
__host__ __device__ __forceinline__ void lp_mul(const double* a, const double* b, double* c) {
    _Pragma("unroll") for (int i = 0; i < 3; ++i) {
        _Pragma("unroll") for (int j = 0; j < 3; ++j) c[3 * i + j] = (a[3 * i] * b[j] + a[3 * i + 1] * b[3 + j]) + a[3 * i + 2] * b[6 + j];
        c[9 + i] = ((a[3 * i] * b[9] + a[3 * i + 1] * b[10]) + a[3 * i + 2] * b[11]) + a[9 + i];
    }
}
// pose_inv as set_cam_pose stores it: rot^T, -rot^T t
__host__ __device__ __forceinline__ void lp_inv(const double* p, double* o) {
    _Pragma("unroll") for (int i = 0; i < 3; ++i) {
        _Pragma("unroll") for (int j = 0; j < 3; ++j) o[3 * i + j] = p[3 * j + i];
        o[9 + i] = ((-p[i]) * p[9] + (-p[3 + i]) * p[10]) + (-p[6 + i]) * p[11];
    }
}
// Item f: the corrected pose of key frame f.  The walk goes up over kf_parent to the origin (at most F steps: a chain that leaves the table, meets
// an erased key frame or runs in a cycle is "not reached") and notes the first key frame on its way that the adjuster optimised, then comes down
// again from that one applying
// after(c) = (pose(c) * pose_inv(p)) * after(p) one step at a time -- the products the queue walk of :110-143 makes, in its order.  The way down
// is walked by counting: step d from the top is found by walking up (depth - d) parents, so that no list has to be kept.
__host__ __device__ __forceinline__ int lp_kf_item(const LpArgs& A, int f, double* after) {
    if (A.kf_erased && A.kf_erased[f]) return PLP_LOOP_BA_KF_ERASED;
    int top = -1, depth = 0, cur = f;
    bool reached = false;
    for (int step = 0; step <= A.F; ++step) {
        if (A.kf_erased && A.kf_erased[cur]) break;
        if (top < 0 && A.kf_optimized[cur]) top = cur;
        if (A.kf_is_origin && A.kf_is_origin[cur]) { reached = true; break; }
        const int p = A.kf_parent[cur];
        if ((unsigned)p >= (unsigned)A.F) break;
        if (top < 0) ++depth;
        cur = p;
    }
    if (!reached || top < 0) return PLP_LOOP_BA_KF_NOT_REACHED;
    _Pragma("unroll") for (int i = 0; i < 12; ++i) after[i] = A.pose_after[(size_t)top * 15 + i];
    for (int d = depth - 1; d >= 0; --d) {
        int c = f;
        for (int s = 0; s < d; ++s) c = A.kf_parent[c];
        const int p = A.kf_parent[c];
        double pc[12], pp[12], inv[12], rel[12], nx[12];
        _Pragma("unroll") for (int i = 0; i < 12; ++i) { pc[i] = A.pose[(size_t)c * A.pose_stride + i]; pp[i] = A.pose[(size_t)p * A.pose_stride + i]; }
        lp_inv(pp, inv);
        lp_mul(pc, inv, rel);
        lp_mul(rel, after, nx);
        _Pragma("unroll") for (int i = 0; i < 12; ++i) after[i] = nx[i];
    }
    return depth ? PLP_LOOP_BA_KF_PROPAGATED : PLP_LOOP_BA_KF_OPTIMIZED;
}
__host__ __device__ __forceinline__ void lp_kf_out(const LpArgs& A, int f) {
    double after[12];
    const int st = lp_kf_item(A, f, after);
    A.out_kf_status[f] = (uint8_t)st;
    if (st != PLP_LOOP_BA_KF_OPTIMIZED && st != PLP_LOOP_BA_KF_PROPAGATED) return;
    double* o = A.out_pose + (size_t)f * 15;
    _Pragma("unroll") for (int i = 0; i < 12; ++i) { o[i] = after[i]; A.out_pose_before[(size_t)f * 12 + i] = A.pose[(size_t)f * A.pose_stride + i]; }
    _Pragma("unroll") for (int i = 0; i < 3; ++i) o[12 + i] = ((-after[i]) * after[9] + (-after[3 + i]) * after[10]) + (-after[6 + i]) * after[11];
}
// Item l: an optimised landmark takes pos_after; any other one goes through its reference key frame: rot_wc_after (rot_before pos + t_before) + t_wc_after
__host__ __device__ __forceinline__ void lp_lm_item(const LpArgs& A, int l) {
    if (A.lm_erased && A.lm_erased[l]) { A.out_lm_status[l] = PLP_LOOP_BA_LM_ERASED; return; }
    double* o = A.out_pos_w + (size_t)3 * l;
    if (A.lm_optimized[l]) {
        _Pragma("unroll") for (int i = 0; i < 3; ++i) o[i] = A.pos_after[(size_t)3 * l + i];
        A.out_lm_status[l] = PLP_LOOP_BA_LM_OPTIMIZED;
        return;
    }
    const int r = A.ref_kf[l];
    double after[12];
    int st = PLP_LOOP_BA_KF_NOT_REACHED;
    if ((unsigned)r < (unsigned)A.F) st = lp_kf_item(A, r, after);
    if (st != PLP_LOOP_BA_KF_OPTIMIZED && st != PLP_LOOP_BA_KF_PROPAGATED) { A.out_lm_status[l] = PLP_LOOP_BA_LM_NO_REF; return; }
    const double* b = A.pose + (size_t)r * A.pose_stride;
    const double* p = A.pos_w + (size_t)3 * l;
    double pc[3], wc[12];
    _Pragma("unroll") for (int i = 0; i < 3; ++i) pc[i] = ((b[3 * i] * p[0] + b[3 * i + 1] * p[1]) + b[3 * i + 2] * p[2]) + b[9 + i];
    lp_inv(after, wc);
    _Pragma("unroll") for (int i = 0; i < 3; ++i) o[i] = ((wc[3 * i] * pc[0] + wc[3 * i + 1] * pc[1]) + wc[3 * i + 2] * pc[2]) + wc[9 + i];
    A.out_lm_status[l] = PLP_LOOP_BA_LM_MOVED;
}

// the launches (global_ba_kernels.hip)
hipError_t gb_launch_prepare(hipStream_t st, const GbArgs& A);
hipError_t gb_launch_fill(hipStream_t st, const GbArgs& A, int P);
hipError_t gb_launch_lin(hipStream_t st, const GbArgs& A, int P, int iteration);
hipError_t gb_launch_try(hipStream_t st, const GbArgs& A, int P);
hipError_t gb_launch_finish(hipStream_t st, const GbArgs& A, bool stopped);
hipError_t gb_launch_chol(hipStream_t st, double* S, double* v, int n, GbRec* rec);
hipError_t lp_launch(hipStream_t st, const LpArgs& A);

}  // namespace plp
