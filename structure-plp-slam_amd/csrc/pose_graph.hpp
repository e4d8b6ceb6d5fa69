// optimize::graph_optimizer::optimize (optimize/graph_optimizer.cc:53-350), one definition for host and device (plp_pose_graph_optimize_* /
// plp_correct_landmarks_* / plp_model_pose_graph_*_host, include/plp_front.h) on top of transform_opt.hpp (D16): the
// vertices and the four kinds of edges from the key-frame and graph tables, g2o's Sim3::log, the Sim3 edge with its central-difference Jacobian
// blocks, the ordered sums of the 7 x 7 blocks into a block skyline, its Cholesky in vertex order, the Levenberg-Marquardt loop (levenberg.hpp)
// and the outputs.  f64 with IEEE + - * / sqrt only, in the order written; translation units that include this file are compiled with
// -ffp-contract=off.  log and acos are pose_log() / pose_acos() below, not a library's.
//
// As in local_ba.hpp the steps are written once over a team `P` of lanes: the kernels run them with a workgroup of 512, the host build with a
// team of one.  No result depends on the team's size: every coefficient is owned by one lane that adds its terms in the defined order.  All
// state between the steps lives in memory the caller names (a context's buffers on the device); the offsets into it wait in the shared state.
#pragma once
#include "transform_opt.hpp"

namespace plp {

constexpr int kPgMaxKf = 1024;            // F
constexpr int kPgMaxEdges = 1 << 14;      // edge_cap: edges of a problem
constexpr int kPgMaxEnv = 1 << 16;        // env_cap: 7 x 7 blocks of a problem's skyline
constexpr int kPgMaxProblems = 16;        // G: the state of a call is G (122 edge_cap + 98 env_cap + 60 F) doubles, at most 1.1 GB
constexpr int kPgMaxList = 1 << 16;       // entries of kf_loop and of the per-problem lists, row width of the graph tables
constexpr int kPgThreads = 512;           // the workgroup of the kernels (tests/test_gpu_pose_graph.py restates it)
constexpr int kPgMinWeight = 100;         // :83

// rows of the per-edge table: both Jacobian blocks (error row major), the error, chi2, the measurement Sim3_21
enum { kPgEJ0 = 0, kPgEJ1 = 49, kPgEErr = 98, kPgEChi = 105, kPgEMeas = 106, kPgEdgeRows = 114 };
// rows of the vertex table: Sim3s_cw, the Sim3 the relative poses of [3.2] use, the kept / tried estimates (two buffers that swap)
enum { kPgVInit = 0, kPgVRel = 8, kPgVEst = 16, kPgVRows = 32 };
// the header ints of a problem
enum { kPgHStatus = 0, kPgHEdges = 1, kPgHN = 2, kPgHEnv = 3, kPgHCur = 4, kPgHIter = 5, kPgHRej = 6, kPgHEnd = 7, kPgHdrInts = 8 };

struct PgArgs {
    int G, F, pose_stride, conn_cap, covis_cap, edge_cap, env_cap, max_iter, ctx_base, edges_only;   // ctx_base: the problem whose state lies first (0 on the device); edges_only: stop after the edge list (a host build's)
    const double* pose; const uint8_t* kf_erased; const int32_t* kf_id; const int32_t* kf_parent;
    const int32_t* kf_conn; const int32_t* kf_conn_w; const int32_t* kf_n_conn; const int32_t* kf_covis; const int32_t* kf_covis_w; const int32_t* kf_n_covis;
    const int32_t* kf_loop_offsets; const int32_t* kf_loop;
    const int32_t* loop_kf; const int32_t* curr_kf; const uint8_t* fix_scale;
    const int32_t* pre_offsets; const int32_t* pre_row; const double* pre_sim3;
    const int32_t* non_offsets; const int32_t* non_row; const double* non_sim3;
    const int32_t* lc_offsets; const int32_t* lc_owner; const int32_t* lc_target;
    uint8_t* out_status; int32_t* out_num_edges; int32_t* out_edges; double* out_sim3_cw; double* out_corrected_wc; double* out_pose;
    int32_t* out_info; double* out_chi2;
    double* ctx_d; int32_t* ctx_i;           // what the steps hand to one another
};
__host__ __device__ __forceinline__ size_t pg_doubles(int F, int E, int V) {
    return (size_t)kPgEdgeRows * E + (size_t)98 * V + (size_t)(kPgVRows + 28) * F + 8;
}
__host__ __device__ __forceinline__ size_t pg_ints(int F, int E, int V) { return (size_t)5 * E + V + (size_t)5 * F + 2 + kPgHdrInts; }

// where a problem's tables lie in the two buffers (elements)
struct PgOff { size_t et, H, Lf, vt, b, x, v, dl, hd, e_a, e_b, e_t, inc, blk, v2s, s2v, first, eoff, ioff, hdr; };
__host__ __device__ __forceinline__ void pg_offsets(const PgArgs& A, int g, PgOff& O) {
    const size_t E = A.edge_cap, V = A.env_cap, F = A.F;
    O.et = pg_doubles(A.F, A.edge_cap, A.env_cap) * (g - A.ctx_base);
    O.H = O.et + kPgEdgeRows * E;
    O.Lf = O.H + 49 * V;
    O.vt = O.Lf + 49 * V;
    O.b = O.vt + kPgVRows * F;
    O.x = O.b + 7 * F;
    O.v = O.x + 7 * F;
    O.dl = O.v + 7 * F;
    O.hd = O.dl + 7 * F;
    O.e_a = pg_ints(A.F, A.edge_cap, A.env_cap) * (g - A.ctx_base);
    O.e_b = O.e_a + E;
    O.e_t = O.e_b + E;
    O.inc = O.e_t + E;
    O.blk = O.inc + 2 * E;
    O.v2s = O.blk + V;
    O.s2v = O.v2s + F;
    O.first = O.s2v + F;
    O.eoff = O.first + F;
    O.ioff = O.eoff + F + 1;
    O.hdr = O.ioff + F + 1;
}
struct PgView {
    double* d; int32_t* i; const PgOff* o;
    __host__ __device__ __forceinline__ double* et() const { return d + o->et; }
    __host__ __device__ __forceinline__ double* H() const { return d + o->H; }
    __host__ __device__ __forceinline__ double* Lf() const { return d + o->Lf; }
    __host__ __device__ __forceinline__ double* vt() const { return d + o->vt; }
    __host__ __device__ __forceinline__ double* b() const { return d + o->b; }
    __host__ __device__ __forceinline__ double* x() const { return d + o->x; }
    __host__ __device__ __forceinline__ double* v() const { return d + o->v; }
    __host__ __device__ __forceinline__ double* dl() const { return d + o->dl; }
    __host__ __device__ __forceinline__ double* hd() const { return d + o->hd; }
    __host__ __device__ __forceinline__ int32_t* e_a() const { return i + o->e_a; }
    __host__ __device__ __forceinline__ int32_t* e_b() const { return i + o->e_b; }
    __host__ __device__ __forceinline__ int32_t* e_t() const { return i + o->e_t; }
    __host__ __device__ __forceinline__ int32_t* inc() const { return i + o->inc; }
    __host__ __device__ __forceinline__ int32_t* blk() const { return i + o->blk; }
    __host__ __device__ __forceinline__ int32_t* v2s() const { return i + o->v2s; }
    __host__ __device__ __forceinline__ int32_t* s2v() const { return i + o->s2v; }
    __host__ __device__ __forceinline__ int32_t* first() const { return i + o->first; }
    __host__ __device__ __forceinline__ int32_t* eoff() const { return i + o->eoff; }
    __host__ __device__ __forceinline__ int32_t* ioff() const { return i + o->ioff; }
    __host__ __device__ __forceinline__ int32_t* hdr() const { return i + o->hdr; }
};
__host__ __device__ __forceinline__ double& pg_e(const PgView& V, int e, int row) { return V.et()[(size_t)e * kPgEdgeRows + row]; }
__host__ __device__ __forceinline__ double& pg_v(const PgView& V, int f, int row) { return V.vt()[(size_t)f * kPgVRows + row]; }

// where the coefficients of pose_log and pose_acos lie in the shared state
enum { kPgCLg = 0, kPgCLn2Hi = 7, kPgCLn2Lo = 8, kPgCpS = 9, kPgCqS = 15, kPgCPio2Hi = 19, kPgCPio2Lo = 20, kPgCPi = 21, kPgCSin = 22, kPgCCos = 28, kPgCTwoOPi = 34, kPgCP1 = 35, kPgCP2 = 36, kPgCExp = 37,
       kPgCInvLn2 = 42, kPgCoefs = 43 };

// the team's shared state: LDS on the device, the stack on the host
struct PgShared {
    PgOff O;
    double tile[kPgThreads];
    double coef[kPgCoefs];
    double lambda, ni, current_chi, rho, acc;
    int32_t ok, qmax, iterations, rejected, go_on, end, cur, n, N, nenv, E, F, fix_scale, status;
    int32_t wave_n[kPgThreads / 64];
    int32_t eoff[kPgMaxKf + 1], ioff[kPgMaxKf + 1], cnt[kPgMaxKf + 1];
    int16_t v2s[kPgMaxKf], s2v[kPgMaxKf], first[kPgMaxKf];
    uint8_t touched[kPgMaxKf];
};

// the team of one of the host build
struct PgTeamHost {
    static constexpr int NT = 1, NW = 1;
    __host__ __device__ int tid() const { return 0; }
    __host__ __device__ int lane() const { return 0; }
    __host__ __device__ int wave() const { return 0; }
    __host__ __device__ void barrier() const {}
    __host__ __device__ void barrier_g() const {}
    __host__ __device__ unsigned long long ballot(bool v) const { return v ? 1ull : 0ull; }
};

// ---- the coefficients of log and acos.  They wait in the shared state (LDS on the device) and are read where they are used: as literals they would
// all be hoisted into scalar registers for the whole of k_pg_solve, which does not have that many.
__host__ __device__ __forceinline__ void pg_coef_init(double* c) {
    c[0] = 6.666666666666735130e-01; c[1] = 3.999999999940941908e-01; c[2] = 2.857142874366239149e-01; c[3] = 2.222219843214978396e-01;
    c[4] = 1.818357216161805012e-01; c[5] = 1.531383769920937332e-01; c[6] = 1.479819860511658591e-01;
    c[7] = 6.93147180369123816490e-01; c[8] = 1.90821492927058770002e-10;
    c[9] = 1.66666666666666657415e-01; c[10] = -3.25565818622400915405e-01; c[11] = 2.01212532134862925881e-01; c[12] = -4.00555345006794114027e-02;
    c[13] = 7.91534994289814532176e-04; c[14] = 3.47933107596021167570e-05;
    c[15] = -2.40339491173441421878e+00; c[16] = 2.02094576023350569471e+00; c[17] = -6.88283971605453293030e-01; c[18] = 7.70381505559019352791e-02;
    c[19] = 1.57079632679489655800e+00; c[20] = 6.12323399573676603587e-17; c[21] = 3.14159265358979311600e+00;
    // pose_sincos's (D15) and pose_exp's (D16)
    c[22] = -1.66666666666666324348e-01; c[23] = 8.33333333332248946124e-03; c[24] = -1.98412698298579493134e-04; c[25] = 2.75573137070700676789e-06;
    c[26] = -2.50507602534068634195e-08; c[27] = 1.58969099521155010221e-10;
    c[28] = 4.16666666666666019037e-02; c[29] = -1.38888888888741095749e-03; c[30] = 2.48015872894767294178e-05; c[31] = -2.75573143513906633035e-07;
    c[32] = 2.08757232129817482790e-09; c[33] = -1.13596475577881948265e-11;
    c[34] = 6.36619772367581382433e-01; c[35] = 1.57079632673412561417e+00; c[36] = 6.07710050650619224932e-11;
    c[37] = 1.66666666666666019037e-01; c[38] = -2.77777777770155933842e-03; c[39] = 6.61375632143793436117e-05; c[40] = -1.65339022054652515390e-06;
    c[41] = 4.13813679705723846039e-08; c[42] = 1.44269504088896338700e+00;
}
// pose_exp and pose_sincos with the coefficients read from the table: the same operations in the same order (tests/test_pose_graph_cpu.py holds them equal)
struct PgMath {
    const double* c;
    __host__ __device__ __forceinline__ double exp(double x) const {
        if (!(x >= -700.0 && x <= 700.0)) return __builtin_nan("");
        const double k = __builtin_floor(x * c[kPgCInvLn2] + 0.5);
        const double hi = x - k * c[kPgCLn2Hi];
        const double lo = k * c[kPgCLn2Lo];
        const double r = hi - lo;
        const double t = r * r;
        const double cc = r - t * (c[kPgCExp] + t * (c[kPgCExp + 1] + t * (c[kPgCExp + 2] + t * (c[kPgCExp + 3] + t * c[kPgCExp + 4]))));
        const double y = 1.0 - ((lo - (r * cc) / (2.0 - cc)) - hi);
        const uint64_t bits = (uint64_t)((int64_t)k + 1023) << 52;
        double p;
        __builtin_memcpy(&p, &bits, 8);
        return y * p;
    }
    __host__ __device__ __forceinline__ void sincos(double x, double& s, double& co) const {
        if (!(x >= -1048576.0 && x <= 1048576.0)) { s = co = __builtin_nan(""); return; }
        const double k = __builtin_floor(x * c[kPgCTwoOPi] + 0.5);
        const double r = (x - k * c[kPgCP1]) - k * c[kPgCP2];
        const double z = r * r;
        const double ps = c[kPgCSin] + z * (c[kPgCSin + 1] + z * (c[kPgCSin + 2] + z * (c[kPgCSin + 3] + z * (c[kPgCSin + 4] + z * c[kPgCSin + 5]))));
        const double pc = c[kPgCCos] + z * (c[kPgCCos + 1] + z * (c[kPgCCos + 2] + z * (c[kPgCCos + 3] + z * (c[kPgCCos + 4] + z * c[kPgCCos + 5]))));
        const double sr = r + (r * z) * ps;
        const double cr = 1.0 - (0.5 * z - (z * z) * pc);
        const int q = (int)k & 3;
        s = q == 0 ? sr : q == 1 ? cr : q == 2 ? -sr : -cr;
        co = q == 0 ? cr : q == 1 ? -sr : q == 2 ? -cr : sr;
    }
};

// ---- log (D22): fdlibm's e_log.c.  x = 2^k (1 + f) with sqrt(2) / 2 < 1 + f < sqrt(2) from the bits, s = f / (2 + f), R(s^2) by Horner without fma,
// k ln2_hi - ((f^2 / 2 - (s (f^2 / 2 + R) + k ln2_lo)) - f).  Domain: 1e-300 <= x <= 1e300 (normal numbers); anything else: NaN.
__host__ __device__ __forceinline__ double pose_log(double x, const double* c) {
    if (!(x >= 1e-300 && x <= 1e300)) return __builtin_nan("");
    uint64_t bits;
    __builtin_memcpy(&bits, &x, 8);
    uint32_t hx = (uint32_t)(bits >> 32);
    int k = (int)(hx >> 20) - 1023;
    hx &= 0x000fffffu;
    const uint32_t i = (hx + 0x95f64u) & 0x100000u;
    hx |= i ^ 0x3ff00000u;
    k += (int)(i >> 20);
    bits = ((uint64_t)hx << 32) | (bits & 0xffffffffull);
    double m;
    __builtin_memcpy(&m, &bits, 8);
    const double f = m - 1.0;
    const double s = f / (2.0 + f);
    const double dk = (double)k;
    const double z = s * s;
    const double R = z * (c[kPgCLg] + z * (c[kPgCLg + 1] + z * (c[kPgCLg + 2] + z * (c[kPgCLg + 3] + z * (c[kPgCLg + 4] + z * (c[kPgCLg + 5] + z * c[kPgCLg + 6]))))));
    const double hfsq = (0.5 * f) * f;
    return dk * c[kPgCLn2Hi] - ((hfsq - (s * (hfsq + R) + dk * c[kPgCLn2Lo])) - f);
}

// ---- acos (D22): fdlibm's e_acos.c, its rational P / Q by Horner without fma.  Domain: -1 <= x <= 1; anything else: NaN.
__host__ __device__ __forceinline__ double pose_acos_r(double z, const double* c) {
    const double p = z * (c[kPgCpS] + z * (c[kPgCpS + 1] + z * (c[kPgCpS + 2] + z * (c[kPgCpS + 3] + z * (c[kPgCpS + 4] + z * c[kPgCpS + 5])))));
    const double q = 1.0 + z * (c[kPgCqS] + z * (c[kPgCqS + 1] + z * (c[kPgCqS + 2] + z * c[kPgCqS + 3])));
    return p / q;
}
__host__ __device__ __forceinline__ double pose_acos(double x, const double* c) {
    const double pio2_hi = c[kPgCPio2Hi], pio2_lo = c[kPgCPio2Lo], pi = c[kPgCPi];
    if (!(x >= -1.0 && x <= 1.0)) return __builtin_nan("");
    if (x == 1.0) return 0.0;
    if (x == -1.0) return pi + 2.0 * pio2_lo;
    const double ax = __builtin_fabs(x);
    if (ax < 0.5) {
        if (ax < 6.938893903907228e-18) return pio2_hi + pio2_lo;       // 2^-57
        const double r = pose_acos_r(x * x, c);
        return pio2_hi - (x - (pio2_lo - x * r));
    }
    if (x < 0.0) {
        const double z = (1.0 + x) * 0.5;
        const double s = __builtin_sqrt(z);
        const double w = pose_acos_r(z, c) * s - pio2_lo;
        return pi - 2.0 * (s + w);
    }
    const double z = (1.0 - x) * 0.5;
    const double s = __builtin_sqrt(z);
    uint64_t bits;
    __builtin_memcpy(&bits, &s, 8);
    bits &= 0xffffffff00000000ull;
    double df;
    __builtin_memcpy(&df, &bits, 8);
    const double cc = (z - df * df) / (s + df);
    const double w = pose_acos_r(z, c) * s + cc;
    return 2.0 * (df + w);
}

// ---- g2o's Sim3::log: out = (omega, upsilon, sigma).  upsilon = W^-1 t by a 3 x 3 LU with partial pivoting (the largest |a|, the first among equals),
// unit lower factor, forward then backward substitution, every chain in ascending column order.
__host__ __device__ __forceinline__ void sim3_log(const double* est, double* out, const double* cf) {
    const double s = est[7];
    const double sigma = pose_log(s, cf);
    double R[9];
    pose_rot_from_quat(est, R);
    const double d = 0.5 * (((R[0] + R[4]) + R[8]) - 1.0);
    const double eps = 0.00001;
    const double dx = R[7] - R[5], dy = R[2] - R[6], dz = R[3] - R[1];      // deltaR
    double A, B, C, k;
    if (__builtin_fabs(sigma) < eps) {
        C = 1.0;
        if (d > 1.0 - eps) {
            k = 0.5; A = 0.5; B = 1.0 / 6.0;
        } else {
            const double theta = pose_acos(d, cf), th2 = theta * theta;
            double si, co;
            PgMath{cf}.sincos(theta, si, co);
            k = theta / (2.0 * __builtin_sqrt(1.0 - d * d));
            A = (1.0 - co) / th2;
            B = (theta - si) / (th2 * theta);
        }
    } else {
        C = (s - 1.0) / sigma;
        const double sg2 = sigma * sigma;
        if (d > 1.0 - eps) {
            k = 0.5;
            A = ((sigma - 1.0) * s + 1.0) / sg2;
            B = (((0.5 * sg2 - sigma) + 1.0) * s) / (sg2 * sigma);
        } else {
            const double theta = pose_acos(d, cf), th2 = theta * theta;
            double si, co;
            PgMath{cf}.sincos(theta, si, co);
            k = theta / (2.0 * __builtin_sqrt(1.0 - d * d));
            const double sa = s * si, sb = s * co, cc = th2 + sg2;
            A = (sa * sigma + (1.0 - sb) * theta) / (theta * cc);
            B = (C - ((sb - 1.0) * sigma + sa * theta) / cc) * 1.0 / th2;
        }
    }
    const double a = k * dx, b = k * dy, c = k * dz;
    out[0] = a; out[1] = b; out[2] = c; out[6] = sigma;
    // W = A Omega + B Omega Omega + C I, rows with the right-hand side behind them
    double r0[4] = {(A * 0.0 + B * (-(b * b + c * c))) + C, A * (-c) + B * (a * b), A * b + B * (a * c), est[4]};
    double r1[4] = {A * c + B * (a * b), (A * 0.0 + B * (-(a * a + c * c))) + C, A * (-a) + B * (b * c), est[5]};
    double r2[4] = {A * (-b) + B * (a * c), A * a + B * (b * c), (A * 0.0 + B * (-(a * a + b * b))) + C, est[6]};
    {
        const bool p1 = __builtin_fabs(r1[0]) > __builtin_fabs(r0[0]);
        const bool p2 = __builtin_fabs(r2[0]) > (p1 ? __builtin_fabs(r1[0]) : __builtin_fabs(r0[0]));
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const double t0 = r0[j], t1 = r1[j], t2 = r2[j];
            r0[j] = p2 ? t2 : p1 ? t1 : t0;
            r1[j] = (p1 && !p2) ? t0 : t1;
            r2[j] = p2 ? t0 : t2;
        }
    }
    const double l10 = r1[0] / r0[0], l20 = r2[0] / r0[0];
#pragma unroll
    for (int j = 1; j < 4; ++j) { r1[j] = r1[j] - l10 * r0[j]; r2[j] = r2[j] - l20 * r0[j]; }
    if (__builtin_fabs(r2[1]) > __builtin_fabs(r1[1])) {
#pragma unroll
        for (int j = 1; j < 4; ++j) { const double t = r1[j]; r1[j] = r2[j]; r2[j] = t; }
    }
    const double l21 = r2[1] / r1[1];
    r2[2] = r2[2] - l21 * r1[2]; r2[3] = r2[3] - l21 * r1[3];
    const double x2 = r2[3] / r2[2];
    const double x1 = (r1[3] - r1[2] * x2) / r1[1];
    const double x0 = ((r0[3] - r0[1] * x1) - r0[2] * x2) / r0[0];
    out[3] = x0; out[4] = x1; out[5] = x2;
}

// the error of a Sim3 edge (graph_opt_edge::computeError): (C v1 v2^-1).log()
__host__ __device__ __forceinline__ void pg_error(const double* C, const double* v1, const double* v2, double* err, const double* cf) {
    double inv[8], m1[8], m2[8];
    tf_inverse(v2, inv);
    tf_mul(C, v1, m1);
    tf_mul(m1, inv, m2);
    sim3_log(m2, err, cf);
}
// g2o::Sim3(rot_cw, trans_cw, 1.0) of a pose row
__host__ __device__ __forceinline__ void pg_sim3_from_pose(const double* pose, double* est) {
    pose_quat_from_rot(pose, est);
    est[4] = pose[9]; est[5] = pose[10]; est[6] = pose[11]; est[7] = 1.0;
}
// set_cam_pose of a corrected Sim3 (:319-325): rot of the quaternion as it is, trans / (double)(float)scale, the camera centre as plp.frame_pose forms it
__host__ __device__ __forceinline__ void pg_pose_from_sim3(const double* est, double* pose15) {
    const double s = (double)(float)est[7];
    pose_rot_from_quat(est, pose15);
    pose15[9] = est[4] / s; pose15[10] = est[5] / s; pose15[11] = est[6] / s;
    for (int i = 0; i < 3; ++i)
        pose15[12 + i] = ((-pose15[i]) * pose15[9] + (-pose15[3 + i]) * pose15[10]) + (-pose15[6 + i]) * pose15[11];
}

// an ordered compaction step over the team (la_rank of local_ba.hpp on this state)
template <class P> __host__ __device__ __forceinline__ int pg_rank(P& par, PgShared& sh, bool v, int& n) {
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

// one chain over items 0 .. count - 1 in order, from sh.acc: fn(i) is item i's value; mode 0 adds, mode 1 takes the largest.  The result is in
// sh.acc after the closing barrier.
template <class P, class Fn> __host__ __device__ __forceinline__ void pg_chain(PgShared& sh, P& par, int count, int mode, Fn fn) {
    const int tid = par.tid();
    for (int base = 0; base < count; base += P::NT) {
        const int i = base + tid;
        sh.tile[tid] = i < count ? fn(i) : 0.0;
        par.barrier();
        if (tid == 0) {
            const int cnt = count - base < P::NT ? count - base : P::NT;
            double acc = sh.acc;
            if (mode == 0) for (int j = 0; j < cnt; ++j) acc = acc + sh.tile[j];
            else for (int j = 0; j < cnt; ++j) acc = sh.tile[j] > acc ? sh.tile[j] : acc;
            sh.acc = acc;
        }
        par.barrier();
    }
}

// a row is a vertex: inside the table and not erased
__host__ __device__ __forceinline__ bool pg_is_vertex(const PgArgs& A, int r) { return (unsigned)r < (unsigned)A.F && !(A.kf_erased && A.kf_erased[r]); }
// graph_node::get_weight: 0 when not connected
__host__ __device__ __forceinline__ int pg_weight(const PgArgs& A, int k, int c) {
    int n = A.kf_n_conn[k];
    n = n < 0 ? 0 : n > A.conn_cap ? A.conn_cap : n;
    for (int i = 0; i < n; ++i)
        if (A.kf_conn[(size_t)k * A.conn_cap + i] == c) return A.kf_conn_w[(size_t)k * A.conn_cap + i];
    return 0;
}
// the entry of a per-problem Sim3 list that names row r (the first one), -1: none
__host__ __device__ __forceinline__ int pg_listed(const int32_t* offsets, const int32_t* rows, int g, int r) {
    if (!offsets) return -1;
    for (int i = offsets[g]; i < offsets[g + 1]; ++i)
        if (rows[i] == r) return i;
    return -1;
}

// the edges of [3.2] that key frame k adds, in insertion order: emit(type, other row).  n31: the edges of [3.1], which the list holds already.
template <class Emit> __host__ __device__ __forceinline__ void pg_row_edges(const PgArgs& A, const PgView& V, int k, int n31, Emit emit) {
    if (!pg_is_vertex(A, k)) return;
    const int id1 = A.kf_id[k], p = A.kf_parent[k];
    const bool has_parent = (unsigned)p < (unsigned)A.F;
    if (has_parent) {
        if (id1 <= A.kf_id[p]) return;                        // :202-205: this `continue` leaves the key frame, not only its parent edge
        if (pg_is_vertex(A, p)) emit(PLP_POSE_GRAPH_EDGE_PARENT, p);
    }
    int lo = A.kf_loop_offsets ? A.kf_loop_offsets[k] : 0, hi = A.kf_loop_offsets ? A.kf_loop_offsets[k + 1] : 0;
    hi = hi < lo ? lo : hi;
    for (int t = lo; t < hi; ++t) {
        const int c = A.kf_loop[t];
        if (!pg_is_vertex(A, c) || id1 <= A.kf_id[c]) continue;
        emit(PLP_POSE_GRAPH_EDGE_LOOP, c);
    }
    // get_covisibilities_over_weight(100): the prefix that reaches the weight, and the empty list when every entry does
    int n = A.kf_n_covis[k];
    n = n < 0 ? 0 : n > A.covis_cap ? A.covis_cap : n;
    const int32_t* cv = A.kf_covis + (size_t)k * A.covis_cap;
    const int32_t* cw = A.kf_covis_w + (size_t)k * A.covis_cap;
    int num = 0;
    while (num < n && cw[num] >= kPgMinWeight) ++num;
    if (num == n || !has_parent) return;
    for (int q = 0; q < num; ++q) {
        const int c = cv[q];
        if ((unsigned)c >= (unsigned)A.F) continue;
        if (A.kf_id[c] == A.kf_id[p] || A.kf_parent[c] == k) continue;
        bool is_loop = false;
        for (int t = lo; t < hi && !is_loop; ++t) is_loop = A.kf_loop[t] == c;
        if (is_loop || (A.kf_erased && A.kf_erased[c])) continue;
        const int id2 = A.kf_id[c];
        if (id1 <= id2) continue;
        bool seen = false;                                    // inserted_edge_pairs: with unique ids only an edge of [3.1] can hold the pair
        for (int e = 0; e < n31 && !seen; ++e) {
            const int ia = A.kf_id[V.e_a()[e]], ib = A.kf_id[V.e_b()[e]];
            seen = (ia == id1 && ib == id2) || (ia == id2 && ib == id1);
        }
        if (!seen) emit(PLP_POSE_GRAPH_EDGE_COVIS, c);
    }
}

// element (p, c) of a skyline (H or the factor): row block i holds the column blocks first(i) .. i, seven scalar rows of 7 (i - first(i) + 1)
__host__ __device__ __forceinline__ long long pg_at(const PgShared& sh, int p, int c) {
    const int i = p / 7, f = sh.first[i];
    return (long long)49 * sh.eoff[i] + (long long)(p - 7 * i) * (7 * (i - f + 1)) + (c - 7 * f);
}

// the tables of the system from the edge list: the vertices of the system in row order, first(i), the envelope's offsets, every vertex's edges
// in insertion order.  sh.status != OK: the envelope does not fit.
template <class P> __host__ __device__ __forceinline__ void pg_structure(const PgView& V, PgShared& sh, P& par, int fixed_row, int env_cap) {
    const int tid = par.tid(), F = sh.F, E = sh.E;
    for (int f = tid; f < F; f += P::NT) sh.touched[f] = 0;
    par.barrier();
    for (int e = tid; e < E; e += P::NT) { sh.touched[V.e_a()[e]] = 1; sh.touched[V.e_b()[e]] = 1; }
    par.barrier();
    int n = 0;
    for (int base = 0; base < F; base += P::NT) {
        const int f = base + tid;
        const bool v = f < F && sh.touched[f] && f != fixed_row;
        const int pos = pg_rank(par, sh, v, n);
        if (f < F) sh.v2s[f] = v ? (int16_t)pos : (int16_t)-1;
        if (v) sh.s2v[pos] = (int16_t)f;
    }
    par.barrier();
    // every vertex's edges in insertion order, and first(i): the lowest vertex of the system one of them reaches
    for (int i = tid; i < n; i += P::NT) {
        int c = 0, lo = i;
        for (int e = 0; e < E; ++e) {
            const int a = sh.v2s[V.e_a()[e]], b = sh.v2s[V.e_b()[e]];
            if (a != i && b != i) continue;
            ++c;
            const int o = a == i ? b : a;
            if (o >= 0 && o < lo) lo = o;
        }
        sh.cnt[i] = c;
        sh.first[i] = (int16_t)lo;
    }
    par.barrier();
    if (tid == 0) {
        int o = 0, q = 0;
        for (int i = 0; i < n; ++i) { sh.ioff[i] = o; o += sh.cnt[i]; sh.eoff[i] = q; q += i - sh.first[i] + 1; }
        sh.ioff[n] = o; sh.eoff[n] = q;
        sh.n = n; sh.N = 7 * n; sh.nenv = q;
        if (q > env_cap) sh.status = PLP_POSE_GRAPH_ENVELOPE_TOO_LARGE;
    }
    par.barrier();
    if (sh.status != PLP_POSE_GRAPH_OK) return;
    for (int i = tid; i < n; i += P::NT) {
        int o = sh.ioff[i];
        for (int e = 0; e < E; ++e)
            if (sh.v2s[V.e_a()[e]] == i || sh.v2s[V.e_b()[e]] == i) V.inc()[o++] = e;
        for (int q = sh.eoff[i]; q < sh.eoff[i + 1]; ++q) V.blk()[q] = i;
    }
    par.barrier_g();
}

// ---- step 1: the vertices (:85-129), the edges (:131-298), the structure of the system
template <class P> __host__ __device__ __forceinline__ void pg_prepare(const PgArgs& A, int g, PgShared& sh, P& par) {
    const int tid = par.tid(), F = A.F;
    if (tid == 0) { pg_offsets(A, g, sh.O); sh.F = F; sh.E = 0; sh.status = PLP_POSE_GRAPH_OK; sh.n = 0; sh.N = 0; sh.nenv = 0; }
    par.barrier();
    const PgView V{A.ctx_d, A.ctx_i, &sh.O};
    const int loop_kf = A.loop_kf[g], curr_kf = A.curr_kf[g];
    if (!pg_is_vertex(A, loop_kf)) {
        if (tid == 0) {
            for (int i = 0; i < kPgHdrInts; ++i) V.hdr()[i] = 0;
            V.hdr()[kPgHStatus] = PLP_POSE_GRAPH_BAD_LOOP_KF;
        }
        return;
    }
    for (int f = tid; f < F; f += P::NT) {
        if (!pg_is_vertex(A, f)) continue;
        double init[8];
        const int pi = pg_listed(A.pre_offsets, A.pre_row, g, f);
        if (pi >= 0) for (int i = 0; i < 8; ++i) init[i] = A.pre_sim3[(size_t)8 * pi + i];
        else pg_sim3_from_pose(A.pose + (size_t)f * A.pose_stride, init);
        const int ni = pg_listed(A.non_offsets, A.non_row, g, f);
        for (int i = 0; i < 8; ++i) {
            pg_v(V, f, kPgVInit + i) = init[i];
            pg_v(V, f, kPgVRel + i) = ni >= 0 ? A.non_sim3[(size_t)8 * ni + i] : init[i];
            pg_v(V, f, kPgVEst + i) = init[i];
            pg_v(V, f, kPgVEst + 8 + i) = init[i];
        }
    }
    par.barrier_g();
    // [3.1] the loop connections in list order (:154-181)
    const int l0 = A.lc_offsets ? A.lc_offsets[g] : 0, l1 = A.lc_offsets ? A.lc_offsets[g + 1] : 0;
    const int cap = A.edge_cap;
    int n31 = 0;
    for (int base = l0; base < l1; base += P::NT) {
        const int t = base + tid;
        bool v = false;
        int a = -1, b = -1;
        if (t < l1) {
            a = A.lc_owner[t]; b = A.lc_target[t];
            v = a != b && pg_is_vertex(A, a) && pg_is_vertex(A, b);
            if (v) {
                const bool exempt = pg_is_vertex(A, curr_kf) && A.kf_id[a] == A.kf_id[curr_kf] && A.kf_id[b] == A.kf_id[loop_kf];
                v = exempt || !(pg_weight(A, a, b) < kPgMinWeight);
            }
        }
        const int pos = pg_rank(par, sh, v, n31);
        if (v && pos < cap) {
            V.e_a()[pos] = a; V.e_b()[pos] = b; V.e_t()[pos] = PLP_POSE_GRAPH_EDGE_LOOP_CONNECTION;
            double w1[8], i1[8], w2[8], m[8];
            for (int i = 0; i < 8; ++i) { w1[i] = pg_v(V, a, kPgVInit + i); w2[i] = pg_v(V, b, kPgVInit + i); }
            tf_inverse(w1, i1);
            tf_mul(w2, i1, m);
            for (int i = 0; i < 8; ++i) pg_e(V, pos, kPgEMeas + i) = m[i];
        }
    }
    par.barrier_g();
    const int n31c = n31 < cap ? n31 : cap;
    // [3.2] (:184-298): every key frame counts its edges, then writes them behind those of the rows before it
    for (int k = tid; k < F; k += P::NT) {
        int c = 0;
        pg_row_edges(A, V, k, n31c, [&c](int, int) { ++c; });
        sh.cnt[k] = c;
    }
    par.barrier();
    if (tid == 0) {
        long long o = n31;
        for (int k = 0; k < F; ++k) { const int c = sh.cnt[k]; sh.cnt[k] = (int)(o < cap ? o : cap); o += c; }
        sh.cnt[F] = (int)(o < cap ? o : cap);
        sh.E = o > cap ? 0 : (int)o;
        if (o > cap) sh.status = PLP_POSE_GRAPH_TOO_MANY_EDGES;
        else if (o == 0) sh.status = PLP_POSE_GRAPH_NO_EDGES;
        V.hdr()[kPgHEdges] = (int)(o > 0x7fffffff ? 0x7fffffff : o);
    }
    par.barrier();
    if (sh.status != PLP_POSE_GRAPH_TOO_MANY_EDGES)
        for (int k = tid; k < F; k += P::NT) {
            int pos = sh.cnt[k];
            pg_row_edges(A, V, k, n31c, [&](int type, int c) {
                V.e_a()[pos] = k; V.e_b()[pos] = c; V.e_t()[pos] = type;
                double w1[8], i1[8], w2[8], m[8];
                for (int i = 0; i < 8; ++i) { w1[i] = pg_v(V, k, kPgVRel + i); w2[i] = pg_v(V, c, kPgVRel + i); }
                tf_inverse(w1, i1);
                tf_mul(w2, i1, m);
                for (int i = 0; i < 8; ++i) pg_e(V, pos, kPgEMeas + i) = m[i];
                ++pos;
            });
        }
    par.barrier_g();
    if (sh.status == PLP_POSE_GRAPH_OK && !A.edges_only) pg_structure(V, sh, par, loop_kf, A.env_cap);
    par.barrier();
    if (sh.status == PLP_POSE_GRAPH_OK) {
        const int n = sh.n;
        for (int f = tid; f < F; f += P::NT) V.v2s()[f] = sh.v2s[f];
        for (int i = tid; i < n; i += P::NT) { V.s2v()[i] = sh.s2v[i]; V.first()[i] = sh.first[i]; }
        for (int i = tid; i <= n; i += P::NT) { V.eoff()[i] = sh.eoff[i]; V.ioff()[i] = sh.ioff[i]; }
    }
    if (tid == 0) {
        V.hdr()[kPgHStatus] = sh.status; V.hdr()[kPgHN] = sh.n; V.hdr()[kPgHEnv] = sh.nenv; V.hdr()[kPgHCur] = 0;
        V.hdr()[kPgHIter] = 0; V.hdr()[kPgHRej] = 0; V.hdr()[kPgHEnd] = 0;
        V.hd()[0] = 0.0; V.hd()[1] = 0.0;
    }
}

// ---- one pass over the edges: the error and chi2 of every edge at the kept (lin) or tried estimates, and when lin the Jacobian block of every
// end that is in the system by central differences (g2o's BaseBinaryEdge::linearizeOplus; the update is tf_oplus, which honours fix_scale)
template <class P> __host__ __device__ __forceinline__ void pg_edge_pass(const PgView& V, PgShared& sh, P& par, bool lin) {
    const int E = sh.E, buf = kPgVEst + 8 * (lin ? sh.cur : 1 - sh.cur);
    const bool fs = sh.fix_scale != 0;
    const double scalar = 1.0 / (2.0 * kPoseNumericDelta);
    for (int e = par.tid(); e < E; e += P::NT) {
        const int ra = V.e_a()[e], rb = V.e_b()[e];
        double va[8], vb[8], C[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) { va[i] = pg_v(V, ra, buf + i); vb[i] = pg_v(V, rb, buf + i); C[i] = pg_e(V, e, kPgEMeas + i); }
        double* T = V.et() + (size_t)e * kPgEdgeRows;
        const bool in_a = sh.v2s[ra] >= 0, in_b = sh.v2s[rb] >= 0;
#pragma unroll 1
        for (int w = lin ? 0 : 28; w < 29; ++w) {
            const bool second = w >= 14 && w < 28, own = w == 28;
            if (!own && !(second ? in_b : in_a)) continue;
            double pa[8], pb[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) { pa[i] = va[i]; pb[i] = vb[i]; }
            const int d = (second ? w - 14 : w) >> 1;
            if (!own) {
                double u[kTfDim], base[8], out[8];
                const double dv = (w & 1) ? -kPoseNumericDelta : kPoseNumericDelta;
#pragma unroll
                for (int i = 0; i < kTfDim; ++i) u[i] = i == d ? dv : 0.0;
#pragma unroll
                for (int i = 0; i < 8; ++i) base[i] = second ? vb[i] : va[i];
                tf_oplus(u, fs, base, out, PgMath{sh.coef});
#pragma unroll
                for (int i = 0; i < 8; ++i) { pa[i] = second ? va[i] : out[i]; pb[i] = second ? out[i] : vb[i]; }
            }
            double err[7];
            pg_error(C, pa, pb, err, sh.coef);
            if (own) {
                double chi = 0.0;
#pragma unroll
                for (int m = 0; m < 7; ++m) { T[kPgEErr + m] = err[m]; chi = chi + err[m] * err[m]; }
                T[kPgEChi] = chi;
            } else {
                double* J = T + (second ? kPgEJ1 : kPgEJ0) + d;          // column d: the plus side waits there for the minus side
                if (!(w & 1)) {
#pragma unroll
                    for (int m = 0; m < 7; ++m) J[7 * m] = err[m];
                } else {
#pragma unroll
                    for (int m = 0; m < 7; ++m) J[7 * m] = scalar * (J[7 * m] - err[m]);
                }
            }
        }
    }
    par.barrier_g();
}

// ---- the sums of a linearisation: coefficient (r, c) of block (i, k) of the skyline belongs to one lane, which walks vertex i's edges in
// insertion order (information = identity: the term of an edge is the dot product of two Jacobian columns, rows ascending); b likewise
template <class P> __host__ __device__ __forceinline__ void pg_sums(const PgView& V, PgShared& sh, P& par) {
    const int nH = 49 * sh.nenv, total = nH + sh.N;
    for (int it = par.tid(); it < total; it += P::NT) {
        int i, k, r, c;
        if (it < nH) {
            const int q = it / 49, rc = it - 49 * q;
            r = rc / 7; c = rc - 7 * r;
            i = V.blk()[q]; k = sh.first[i] + (q - sh.eoff[i]);
            if (k == i && c > r) continue;
        } else {
            i = (it - nH) / 7; r = (it - nH) - 7 * i; k = -1; c = 0;
        }
        double acc = 0.0;
        for (int t = sh.ioff[i]; t < sh.ioff[i + 1]; ++t) {
            const int e = V.inc()[t];
            const bool first_end = sh.v2s[V.e_a()[e]] == i;
            const double* T = V.et() + (size_t)e * kPgEdgeRows;
            const double* own = T + (first_end ? kPgEJ0 : kPgEJ1) + r;
            const double* oth;
            if (k < 0) oth = nullptr;
            else if (k == i) oth = T + (first_end ? kPgEJ0 : kPgEJ1) + c;
            else {
                if (sh.v2s[first_end ? V.e_b()[e] : V.e_a()[e]] != k) continue;
                oth = T + (first_end ? kPgEJ1 : kPgEJ0) + c;
            }
            double term = 0.0;
            if (k < 0) {
#pragma unroll
                for (int m = 0; m < 7; ++m) { const double v = own[7 * m] * (-T[kPgEErr + m]); term = m == 0 ? v : term + v; }
            } else {
#pragma unroll
                for (int m = 0; m < 7; ++m) { const double v = own[7 * m] * oth[7 * m]; term = m == 0 ? v : term + v; }
            }
            acc = acc + term;
        }
        if (k < 0) V.b()[7 * i + r] = acc;
        else V.H()[pg_at(sh, 7 * i + r, 7 * k + c)] = acc;
    }
    par.barrier_g();
}

// ---- (H + lambda I) x = b by the Cholesky of the skyline in vertex order, one column and one barrier per step: row p of the factor is lane p's,
// every subtraction chain runs over ascending k inside the envelope.  sh.ok = 0: a pivot is not positive and finite, x is then zero.
template <class P> __host__ __device__ __forceinline__ void pg_solve_system(const PgView& V, PgShared& sh, P& par) {
    const int tid = par.tid(), N = sh.N;
    const double lambda = sh.lambda;
    const double* H = V.H();
    double* Lf = V.Lf();
    if (tid == 0) sh.ok = 1;
    par.barrier();
    for (int j = 0; j < N; ++j) {
        const int jb = j / 7, fj = 7 * sh.first[jb];
        for (int p = j + tid; p < N; p += P::NT) {
            const int fp = 7 * sh.first[p / 7];
            if (fp > j) continue;
            const long long rj = pg_at(sh, j, 0), rp = pg_at(sh, p, 0);       // may lie before the row: only columns inside it are reached
            double s = H[rj + j] + lambda, v = H[rp + j];
            for (int k = fj; k < j; ++k) {
                const double ljk = Lf[rj + k];
                s = s - ljk * ljk;
                if (p > j && k >= fp) v = v - Lf[rp + k] * ljk;
            }
            if (!(s > 0.0) || s > kLevDblMax) { sh.ok = 0; continue; }
            const double d = __builtin_sqrt(s);
            if (p == j) V.dl()[j] = d;
            else Lf[rp + j] = v / d;
        }
        par.barrier_g();
    }
    if (sh.ok) {
        for (int p = tid; p < N; p += P::NT) V.v()[p] = V.b()[p];
        par.barrier_g();
        for (int j = 0; j < N; ++j) {                         // L y = b: y ends in x
            const double yj = V.v()[j] / V.dl()[j];
            for (int p = j + tid; p < N; p += P::NT) {
                if (p == j) { V.x()[j] = yj; continue; }
                if (7 * sh.first[p / 7] > j) continue;
                V.v()[p] = V.v()[p] - Lf[pg_at(sh, p, 0) + j] * yj;
            }
            par.barrier_g();
        }
        for (int p = tid; p < N; p += P::NT) V.v()[p] = V.x()[p];
        par.barrier_g();
        for (int j = N - 1; j >= 0; --j) {                    // L^T x = y
            const double xj = V.v()[j] / V.dl()[j];
            const long long rj = pg_at(sh, j, 0);
            for (int p = 7 * sh.first[j / 7] + tid; p <= j; p += P::NT) {
                if (p == j) { V.x()[j] = xj; continue; }
                V.v()[p] = V.v()[p] - Lf[rj + p] * xj;
            }
            par.barrier_g();
        }
    } else {
        for (int p = tid; p < N; p += P::NT) V.x()[p] = 0.0;
        par.barrier_g();
    }
}

// ---- the Levenberg-Marquardt loop of one problem (:302-303; OptimizationAlgorithmLevenberg::solve as local_ba.hpp walks it)
template <class P> __host__ __device__ __forceinline__ void pg_solve(const PgArgs& A, int g, PgShared& sh, P& par) {
    const int tid = par.tid();
    if (tid == 0) pg_offsets(A, g, sh.O);
    par.barrier();
    const PgView V{A.ctx_d, A.ctx_i, &sh.O};
    if (V.hdr()[kPgHStatus] != PLP_POSE_GRAPH_OK) return;
    if (tid == 0) {
        sh.F = A.F; sh.E = V.hdr()[kPgHEdges]; sh.n = V.hdr()[kPgHN]; sh.N = 7 * sh.n; sh.nenv = V.hdr()[kPgHEnv];
        sh.fix_scale = A.fix_scale && A.fix_scale[g] ? 1 : 0;
        pg_coef_init(sh.coef);
        sh.lambda = 0.0; sh.ni = 2.0; sh.current_chi = 0.0; sh.cur = 0; sh.iterations = 0; sh.rejected = 0; sh.end = 0; sh.rho = 0.0; sh.qmax = 0;
    }
    par.barrier();
    const int n = sh.n, iters = A.max_iter;
    for (int f = tid; f < sh.F; f += P::NT) sh.v2s[f] = (int16_t)V.v2s()[f];
    for (int i = tid; i < n; i += P::NT) { sh.s2v[i] = (int16_t)V.s2v()[i]; sh.first[i] = (int16_t)V.first()[i]; }
    for (int i = tid; i <= n; i += P::NT) { sh.eoff[i] = V.eoff()[i]; sh.ioff[i] = V.ioff()[i]; }
    par.barrier();
    int it = 0;
    bool lin = true;
    while (n > 0 && iters > 0) {
        if (!lin) {
            pg_solve_system(V, sh, par);
            const int kc = kPgVEst + 8 * sh.cur, kt = kPgVEst + 8 * (1 - sh.cur);
            const bool fs = sh.fix_scale != 0;
            for (int i = tid; i < n; i += P::NT) {           // the tried estimates: Sim3(x_i) * est_i
                const int f = sh.s2v[i];
                double u[kTfDim], bak[8], out[8];
                for (int k = 0; k < kTfDim; ++k) u[k] = V.x()[7 * i + k];
                for (int k = 0; k < 8; ++k) bak[k] = pg_v(V, f, kc + k);
                tf_oplus(u, fs, bak, out, PgMath{sh.coef});
                for (int k = 0; k < 8; ++k) pg_v(V, f, kt + k) = out[k];
            }
            par.barrier_g();
        }
        pg_edge_pass(V, sh, par, lin);
        if (lin) pg_sums(V, sh, par);
        if (tid == 0) sh.acc = 0.0;
        par.barrier();
        pg_chain(sh, par, sh.E, 0, [&V](int e) { return pg_e(V, e, kPgEChi); });
        if (lin) {
            if (tid == 0) sh.current_chi = sh.acc;
            par.barrier();
            if (it == 0) {                                    // computeLambdaInit over every diagonal
                if (tid == 0) sh.acc = 0.0;
                par.barrier();
                pg_chain(sh, par, sh.N, 1, [&V, &sh](int p) { return __builtin_fabs(V.H()[pg_at(sh, p, p)]); });
                if (tid == 0) { sh.lambda = 1e-5 * sh.acc; sh.ni = 2.0; }
            }
            if (tid == 0) { sh.qmax = 0; sh.rho = 0.0; }
            par.barrier();
            lin = false;
            continue;
        }
        const double temp_sum = sh.acc;
        par.barrier();
        if (tid == 0) sh.acc = 0.0;
        par.barrier();
        {                                                     // computeScale: one partial per vertex, the vertices in order on one accumulator
            const double lambda = sh.lambda;
            pg_chain(sh, par, n, 0, [&V, lambda](int i) {
                double part = 0.0;
                for (int k = 0; k < 7; ++k) { const double x = V.x()[7 * i + k]; part = part + x * (lambda * x + V.b()[7 * i + k]); }
                return part;
            });
        }
        if (tid == 0) {
            lev_decide(sh, sh.ok != 0, temp_sum, sh.acc, [&sh] { sh.cur = 1 - sh.cur; }, [] {});
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
    par.barrier();
    if (tid == 0) {
        V.hdr()[kPgHCur] = sh.cur; V.hdr()[kPgHIter] = sh.iterations; V.hdr()[kPgHRej] = sh.rejected;
        V.hdr()[kPgHEnd] = sh.end ? sh.end : sh.iterations ? kLevEndIterations : 0;
        V.hd()[0] = sh.current_chi; V.hd()[1] = sh.lambda;
    }
}

// ---- the outputs (:307-328)
template <class P> __host__ __device__ __forceinline__ void pg_finish(const PgArgs& A, int g, P& par) {
    PgOff O;
    pg_offsets(A, g, O);
    const PgView V{A.ctx_d, A.ctx_i, &O};
    const int tid = par.tid(), F = A.F, status = V.hdr()[kPgHStatus];
    if (tid == 0) {
        A.out_status[g] = (uint8_t)status;
        if (A.out_num_edges) A.out_num_edges[g] = V.hdr()[kPgHEdges];
    }
    if (status != PLP_POSE_GRAPH_OK && status != PLP_POSE_GRAPH_NO_EDGES) return;
    const int E = V.hdr()[kPgHEdges], kc = kPgVEst + 8 * V.hdr()[kPgHCur];
    if (A.out_edges)
        for (int e = tid; e < E; e += P::NT) {
            int32_t* o = A.out_edges + ((size_t)g * A.edge_cap + e) * 3;
            o[0] = V.e_a()[e]; o[1] = V.e_b()[e]; o[2] = V.e_t()[e];
        }
    for (int f = tid; f < F; f += P::NT) {
        if (!pg_is_vertex(A, f)) continue;
        double est[8], inv[8], p15[15];
        for (int i = 0; i < 8; ++i) est[i] = pg_v(V, f, kc + i);
        if (A.out_sim3_cw) for (int i = 0; i < 8; ++i) A.out_sim3_cw[((size_t)g * F + f) * 8 + i] = pg_v(V, f, kPgVInit + i);
        if (A.out_corrected_wc) {
            tf_inverse(est, inv);
            for (int i = 0; i < 8; ++i) A.out_corrected_wc[((size_t)g * F + f) * 8 + i] = inv[i];
        }
        if (A.out_pose) {
            pg_pose_from_sim3(est, p15);
            for (int i = 0; i < 15; ++i) A.out_pose[((size_t)g * F + f) * 15 + i] = p15[i];
        }
    }
    if (tid == 0) {
        if (A.out_info) {
            int32_t* o = A.out_info + (size_t)4 * g;
            o[0] = V.hdr()[kPgHIter]; o[1] = V.hdr()[kPgHRej]; o[2] = V.hdr()[kPgHEnd]; o[3] = V.hdr()[kPgHN];
        }
        if (A.out_chi2) { A.out_chi2[(size_t)2 * g] = V.hd()[0]; A.out_chi2[(size_t)2 * g + 1] = V.hd()[1]; }
    }
}

// ---- the landmark half (:331-350): corrected_Sim3_wc[ref].map(Sim3_cw[ref].map(pos_w)), one lane per landmark
struct PgLmArgs {
    int L, F;
    const double* pos_w; const uint8_t* lm_erased; const int32_t* ref_kf; const uint8_t* kf_erased; const double* sim3_cw; const double* corrected_wc;
    double* out_pos_w; uint8_t* out_status;
};
__host__ __device__ __forceinline__ void pg_correct_landmark(const PgLmArgs& A, int l) {
    if (A.lm_erased && A.lm_erased[l]) { A.out_status[l] = PLP_CORRECT_LM_ERASED; return; }
    const int r = A.ref_kf[l];
    if ((unsigned)r >= (unsigned)A.F || (A.kf_erased && A.kf_erased[r])) { A.out_status[l] = PLP_CORRECT_LM_NO_VERTEX; return; }
    double a[8], b[8], x, y, z, ox, oy, oz;
    for (int i = 0; i < 8; ++i) { a[i] = A.sim3_cw[(size_t)8 * r + i]; b[i] = A.corrected_wc[(size_t)8 * r + i]; }
    tf_map(a, A.pos_w[(size_t)3 * l], A.pos_w[(size_t)3 * l + 1], A.pos_w[(size_t)3 * l + 2], x, y, z);
    tf_map(b, x, y, z, ox, oy, oz);
    A.out_pos_w[(size_t)3 * l] = ox; A.out_pos_w[(size_t)3 * l + 1] = oy; A.out_pos_w[(size_t)3 * l + 2] = oz;
    A.out_status[l] = PLP_CORRECT_LM_OK;
}

hipError_t launch_pose_graph(hipStream_t st, const PgArgs& A);
hipError_t launch_correct_landmarks(hipStream_t st, const PgLmArgs& A);

}  // namespace plp
