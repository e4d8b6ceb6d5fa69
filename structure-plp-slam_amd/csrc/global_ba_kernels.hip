// Global bundle adjustment: optimize::global_bundle_adjuster (plp_global_ba_*, plp_loop_ba_propagate_*, include/plp_front.h; DESIGN.md section 5,
// D23).  One problem on the whole device: every step of global_ba.hpp is a launch of its own on the caller's stream, an item per lane, and a phase
// boundary is a launch boundary -- no grid-wide barrier, no cooperative launch, no workgroup ever waits for another.
//
// k_gb_kf / k_gb_lm / k_gb_rank / k_gb_fill: the sets, the edges of every landmark run, the rows of the reduced system, every free pose's edge
//      list in edge order (a wave per pose scans the edge table with ballots), once per call.
// k_gb_edge / k_gb_lm_sum / k_gb_pose_sum: a pass; k_gb_begin (one workgroup): the chi2 chain and computeLambdaInit.
// k_gb_inv / k_gb_y / k_gb_schur (a wave per free pose, 42 lanes own the coefficients of its block row) : the reduced system.
// k_gb_chol_diag / k_gb_chol_rows: the dense Cholesky panel by panel (kGbPanel columns).  Per panel one launch of one workgroup for the diagonal
//      block and one launch over all workgroups for the rows below, kGbRows rows each.  Every coefficient's accumulator is a register from its
//      A(p, j) to its L(p, j); k runs ascending over all earlier panels -- both operand rows staged through LDS tiles of kGbPanel columns of k --
//      and then inside the panel.  The result does not depend on the panel width, the tiling or the number of workgroups.
// k_gb_subst (one workgroup): both substitutions, blocked by kGbPanel: a wave solves the triangle of a block, then every remaining row subtracts
//      the block's terms in the defined order.
// k_gb_xl / k_gb_update, the evaluation pass, k_gb_decide (one workgroup): the tried step and g2o's decision.
// k_gb_out_*: the outputs.  k_lp_kf / k_lp_lm: the loop adjuster's map update.
#include <hip/hip_runtime.h>

#include "plp_barrier.hpp"
#include "global_ba.hpp"

namespace plp {
namespace {

struct GbTeamWg {
    static constexpr int NT = kGbThreads;
    __device__ __forceinline__ int tid() const { return threadIdx.x; }
    __device__ __forceinline__ void barrier() const { wg_barrier_after_global_stores(); }
};
struct GbAddDev { __device__ __forceinline__ void operator()(int32_t* p) const { atomicAdd(p, 1); } };

__device__ __forceinline__ int gb_gid() { return blockIdx.x * kGbThreads + threadIdx.x; }

__global__ __launch_bounds__(kGbThreads) void k_gb_kf(GbArgs A) {
    const int i = gb_gid();
    if (i == 0) gb_rec_init(A);
    if (i < A.F) gb_kf_item(A, i);
    if (i < A.T) gb_edge_clear(A, i);
}
__global__ __launch_bounds__(kGbThreads) void k_gb_lm(GbArgs A) {
    const int l = gb_gid();
    if (l < A.L) gb_lm_item(A, l, GbAddDev());
}
__global__ __launch_bounds__(64) void k_gb_rank(GbArgs A) {
    if (threadIdx.x == 0) gb_rank(A);
}
__global__ __launch_bounds__(64) void k_gb_fill(GbArgs A) {
    const int a = blockIdx.x, lane = threadIdx.x, kf = A.akf[a], T = A.T;
    int pos = A.aoff[a];
    for (int base = 0; base < T; base += 64) {
        const int t = base + lane;
        const bool v = t < T && A.e_kf[t] == kf;
        const unsigned long long m = __ballot(v);
        if (v) A.byp[pos + (int)__builtin_popcountll(m & ((1ull << lane) - 1ull))] = t;
        pos += (int)__builtin_popcountll(m);
    }
}
__global__ __launch_bounds__(kGbThreads) void k_gb_edge(GbArgs A, int lin) {
    const int t = gb_gid();
    if (t < A.T) gb_edge_item(A, t, lin != 0);
}
__global__ __launch_bounds__(kGbThreads) void k_gb_lm_sum(GbArgs A, int lin) {
    const int l = gb_gid();
    if (l < A.L) gb_lm_sum_item(A, l, lin != 0);
}
__global__ __launch_bounds__(kGbThreads) void k_gb_pose_sum(GbArgs A, int P) {
    const int it = gb_gid();
    if (it < 27 * P) gb_pose_sum_item(A, it);
}
__global__ __launch_bounds__(kGbThreads) void k_gb_begin(GbArgs A, int iteration) {
    __shared__ double tile[kGbThreads];
    GbTeamWg par;
    gb_begin(A, par, tile, iteration);
}
__global__ __launch_bounds__(kGbThreads) void k_gb_inv(GbArgs A) {
    const int l = gb_gid();
    if (l < A.L) gb_inv_item(A, l);
}
__global__ __launch_bounds__(kGbThreads) void k_gb_y(GbArgs A) {
    const int t = gb_gid();
    if (t < A.T) gb_y_item(A, t);
}
__global__ __launch_bounds__(64) void k_gb_schur(GbArgs A) {
    const int it = threadIdx.x;
    if (it < 42) gb_schur_item(A, blockIdx.x, it / 7, it % 7);
}
__global__ __launch_bounds__(kGbThreads) void k_gb_xl(GbArgs A) {
    const int l = gb_gid();
    if (l < A.L) gb_xl_item(A, l);
}
__global__ __launch_bounds__(kGbThreads) void k_gb_update(GbArgs A, int P) {
    const int a = gb_gid();
    if (a < P) gb_update_item(A, a);
}
__global__ __launch_bounds__(kGbThreads) void k_gb_decide(GbArgs A) {
    __shared__ double tile[kGbThreads];
    GbTeamWg par;
    gb_decide(A, par, tile);
}
__global__ __launch_bounds__(kGbThreads) void k_gb_out_kf(GbArgs A) {
    const int f = gb_gid();
    if (f < A.F) gb_out_kf_item(A, f);
}
__global__ __launch_bounds__(kGbThreads) void k_gb_out_lm(GbArgs A) {
    const int l = gb_gid();
    if (l < A.L) gb_out_lm_item(A, l);
}
__global__ __launch_bounds__(64) void k_gb_out_rec(GbArgs A, int stopped) {
    if (threadIdx.x == 0) gb_out_rec(A, stopped != 0);
}

// ---- the dense Cholesky.  S is n x n row-major; A(p, j) = S(j, p) for p >= j, and L(p, j) takes its place.  NB = kGbPanel columns j0 .. j0 + NB - 1
// form a panel.  A workgroup of 256 lanes is 8 rows of 32: lane (ty, tx) owns column j0 + tx of the rows r0 + ty + 8 m.
constexpr int NB = kGbPanel;
static_assert(NB == 32 && kGbRows == 64 && kGbThreads == 256, "the lane layout of the panel kernels");

// acc[m] -= sum over k < j0, ascending, of L(r0 + ty + 8 m, k) L(j0 + tx, k): both operand rows through LDS, NB columns of k at a time
template <int M> __device__ __forceinline__ void gb_panel_gemm(const double* S, int n, int j0, int r0, double (&acc)[M], double (*ta)[8 * M + 1], double (*tb)[NB + 1]) {
    const int tid = threadIdx.x, tx = tid & 31, ty = tid >> 5;
    for (int k0 = 0; k0 < j0; k0 += NB) {
        for (int e = tid; e < NB * 8 * M; e += kGbThreads) {
            const int kk = e / (8 * M), c = e % (8 * M);
            ta[kk][c] = r0 + c < n ? S[(size_t)(k0 + kk) * n + r0 + c] : 0.0;
        }
        for (int e = tid; e < NB * NB; e += kGbThreads) {
            const int kk = e / NB, c = e % NB;
            tb[kk][c] = j0 + c < n ? S[(size_t)(k0 + kk) * n + j0 + c] : 0.0;
        }
        wg_barrier();
        for (int kk = 0; kk < NB; ++kk) {
            const double b = tb[kk][tx];
            _Pragma("unroll") for (int m = 0; m < M; ++m) acc[m] = acc[m] - ta[kk][ty + 8 * m] * b;
        }
        wg_barrier();
    }
}

// the diagonal block of panel j0: one workgroup
__global__ __launch_bounds__(kGbThreads) void k_gb_chol_diag(double* S, int n, int j0, GbRec* rec) {
    __shared__ double ta[NB][NB + 1], tb[NB][NB + 1], lp[NB][NB + 1];
    __shared__ double dsh;
    __shared__ int ok;
    if (!rec->ok) return;
    const int tid = threadIdx.x, tx = tid & 31, ty = tid >> 5, j = j0 + tx, w = n - j0 < NB ? n - j0 : NB;
    double acc[4];
    _Pragma("unroll") for (int m = 0; m < 4; ++m) {
        const int p = j0 + ty + 8 * m;
        acc[m] = (j < n && p < n && p >= j) ? S[(size_t)j * n + p] : 0.0;
        lp[ty + 8 * m][tx] = 0.0;
    }
    if (tid == 0) ok = 1;
    gb_panel_gemm<4>(S, n, j0, j0, acc, ta, tb);
    wg_barrier();
    for (int kk = 0; kk < w; ++kk) {
        if (tx == kk) {
            _Pragma("unroll") for (int m = 0; m < 4; ++m)
                if (ty + 8 * m == kk) {
                    const double s = acc[m];
                    if (!(s > 0.0) || s > kLevDblMax) { ok = 0; rec->ok = 0; }
                    const double d = __builtin_sqrt(s);
                    dsh = d;
                    S[(size_t)j * n + j] = d;
                }
        }
        wg_barrier();
        if (!ok) return;
        if (tx == kk) {
            const double d = dsh;
            _Pragma("unroll") for (int m = 0; m < 4; ++m) {
                const int q = ty + 8 * m;
                if (q > kk && q < w) {
                    const double v = acc[m] / d;
                    lp[q][kk] = v;
                    S[(size_t)j * n + j0 + q] = v;
                }
            }
        }
        wg_barrier();
        if (tx > kk) {
            const double b = lp[tx][kk];
            _Pragma("unroll") for (int m = 0; m < 4; ++m)
                if (ty + 8 * m >= tx) acc[m] = acc[m] - lp[ty + 8 * m][kk] * b;
        }
    }
}

// the rows below the diagonal block of panel j0: workgroup b owns rows j0 + NB + kGbRows b ..
__global__ __launch_bounds__(kGbThreads) void k_gb_chol_rows(double* S, int n, int j0, const GbRec* rec) {
    __shared__ double ta[NB][kGbRows + 1], tb[NB][NB + 1], lp[kGbRows][NB + 1];
    if (!rec->ok) return;
    const int tid = threadIdx.x, tx = tid & 31, ty = tid >> 5, r0 = j0 + NB + kGbRows * blockIdx.x;
    double acc[8];
    _Pragma("unroll") for (int m = 0; m < 8; ++m) {
        const int p = r0 + ty + 8 * m;
        acc[m] = p < n ? S[(size_t)(j0 + tx) * n + p] : 0.0;
    }
    gb_panel_gemm<8>(S, n, j0, r0, acc, ta, tb);
    // the panel's own columns: tb = the finished diagonal block, tb[kk][c] = L(j0 + c, j0 + kk) for c >= kk
    for (int e = tid; e < NB * NB; e += kGbThreads) {
        const int kk = e / NB, c = e % NB;
        tb[kk][c] = S[(size_t)(j0 + kk) * n + j0 + c];
    }
    wg_barrier();
    for (int kk = 0; kk < NB; ++kk) {
        if (tx == kk) {
            const double d = tb[kk][kk];
            _Pragma("unroll") for (int m = 0; m < 8; ++m) lp[ty + 8 * m][kk] = acc[m] / d;
        }
        wg_barrier();
        if (tx > kk) {
            const double b = tb[kk][tx];
            _Pragma("unroll") for (int m = 0; m < 8; ++m) acc[m] = acc[m] - lp[ty + 8 * m][kk] * b;
        }
    }
    wg_barrier();
    for (int e = tid; e < NB * kGbRows; e += kGbThreads) {
        const int kk = e / kGbRows, c = e % kGbRows;
        if (r0 + c < n) S[(size_t)(j0 + kk) * n + r0 + c] = lp[c][kk];
    }
}

// both substitutions in place on v, one workgroup; a failed solve leaves v zero
__global__ __launch_bounds__(kGbThreads) void k_gb_subst(const double* S, double* v, int n, const GbRec* rec) {
    __shared__ double blk[NB][NB + 1], ys[NB];
    const int tid = threadIdx.x;
    if (!rec->ok) {
        for (int p = tid; p < n; p += kGbThreads) v[p] = 0.0;
        return;
    }
    for (int jb = 0; jb < n; jb += NB) {
        const int w = n - jb < NB ? n - jb : NB;
        for (int e = tid; e < NB * NB; e += kGbThreads) {
            const int kk = e / NB, c = e % NB;
            blk[kk][c] = (kk < w && c < w) ? S[(size_t)(jb + kk) * n + jb + c] : 1.0;
        }
        wg_barrier_after_global_stores();
        if (tid < 64) {
            const int lane = tid;
            const bool in = lane < w;
            double x = in ? v[jb + lane] : 0.0;
            const double d = in ? blk[lane][lane] : 1.0;
            for (int kk = 0; kk < w; ++kk) {
                const double y = __shfl(x / d, kk);
                if (lane == kk) x = y;
                else if (lane > kk && in) x = x - blk[kk][lane] * y;
            }
            if (in) { ys[lane] = x; v[jb + lane] = x; }
        }
        wg_barrier_after_global_stores();
        for (int p = jb + NB + tid; p < n; p += kGbThreads) {
            double acc = v[p];
            for (int kk = 0; kk < NB; ++kk) acc = acc - S[(size_t)(jb + kk) * n + p] * ys[kk];
            v[p] = acc;
        }
        wg_barrier_after_global_stores();
    }
    for (int jb = ((n - 1) / NB) * NB; jb >= 0; jb -= NB) {
        const int w = n - jb < NB ? n - jb : NB;
        for (int e = tid; e < NB * NB; e += kGbThreads) {
            const int kk = e / NB, c = e % NB;
            blk[kk][c] = (kk < w && c < w) ? S[(size_t)(jb + kk) * n + jb + c] : 1.0;
        }
        wg_barrier_after_global_stores();
        if (tid < 64) {
            const int lane = tid;
            const bool in = lane < w;
            double x = in ? v[jb + lane] : 0.0;
            const double d = in ? blk[lane][lane] : 1.0;
            for (int kk = w - 1; kk >= 0; --kk) {
                const double y = __shfl(x / d, kk);
                if (lane == kk) x = y;
                else if (lane < kk) x = x - blk[lane][kk] * y;
            }
            if (in) { ys[lane] = x; v[jb + lane] = x; }
        }
        wg_barrier_after_global_stores();
        for (int p = tid; p < jb; p += kGbThreads) {
            double acc = v[p];
            for (int kk = w - 1; kk >= 0; --kk) acc = acc - S[(size_t)p * n + jb + kk] * ys[kk];
            v[p] = acc;
        }
        wg_barrier_after_global_stores();
    }
}

__global__ __launch_bounds__(kGbThreads) void k_lp_kf(LpArgs A) {
    const int f = gb_gid();
    if (f < A.F) lp_kf_out(A, f);
}
__global__ __launch_bounds__(kGbThreads) void k_lp_lm(LpArgs A) {
    const int l = gb_gid();
    if (l < A.L) lp_lm_item(A, l);
}

inline dim3 gb_grid(long long items) { return dim3((unsigned)((items + kGbThreads - 1) / kGbThreads)); }

}  // namespace

hipError_t gb_launch_prepare(hipStream_t st, const GbArgs& A) {
    const int m = A.F > A.T ? A.F : A.T;
    hipLaunchKernelGGL(k_gb_kf, gb_grid(m > 1 ? m : 1), dim3(kGbThreads), 0, st, A);
    if (A.L > 0) hipLaunchKernelGGL(k_gb_lm, gb_grid(A.L), dim3(kGbThreads), 0, st, A);
    hipLaunchKernelGGL(k_gb_rank, dim3(1), dim3(64), 0, st, A);
    return hipGetLastError();
}
hipError_t gb_launch_fill(hipStream_t st, const GbArgs& A, int P) {
    if (P > 0) hipLaunchKernelGGL(k_gb_fill, dim3(P), dim3(64), 0, st, A);
    return hipGetLastError();
}
hipError_t gb_launch_lin(hipStream_t st, const GbArgs& A, int P, int iteration) {
    hipLaunchKernelGGL(k_gb_edge, gb_grid(A.T), dim3(kGbThreads), 0, st, A, 1);
    hipLaunchKernelGGL(k_gb_lm_sum, gb_grid(A.L), dim3(kGbThreads), 0, st, A, 1);
    if (P > 0) hipLaunchKernelGGL(k_gb_pose_sum, gb_grid(27ll * P), dim3(kGbThreads), 0, st, A, P);
    hipLaunchKernelGGL(k_gb_begin, dim3(1), dim3(kGbThreads), 0, st, A, iteration);
    return hipGetLastError();
}
hipError_t gb_launch_chol(hipStream_t st, double* S, double* v, int n, GbRec* rec) {
    for (int j0 = 0; j0 < n; j0 += NB) {
        hipLaunchKernelGGL(k_gb_chol_diag, dim3(1), dim3(kGbThreads), 0, st, S, n, j0, rec);
        const int below = n - (j0 + NB);
        if (below > 0) hipLaunchKernelGGL(k_gb_chol_rows, dim3((below + kGbRows - 1) / kGbRows), dim3(kGbThreads), 0, st, S, n, j0, rec);
    }
    hipLaunchKernelGGL(k_gb_subst, dim3(1), dim3(kGbThreads), 0, st, S, v, n, rec);
    return hipGetLastError();
}
hipError_t gb_launch_try(hipStream_t st, const GbArgs& A, int P) {
    hipLaunchKernelGGL(k_gb_inv, gb_grid(A.L), dim3(kGbThreads), 0, st, A);
    if (P > 0) {
        hipLaunchKernelGGL(k_gb_y, gb_grid(A.T), dim3(kGbThreads), 0, st, A);
        hipLaunchKernelGGL(k_gb_schur, dim3(P), dim3(64), 0, st, A);
        const hipError_t e = gb_launch_chol(st, A.S, A.x, 6 * P, A.rec);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(k_gb_xl, gb_grid(A.L), dim3(kGbThreads), 0, st, A);
    if (P > 0) hipLaunchKernelGGL(k_gb_update, gb_grid(P), dim3(kGbThreads), 0, st, A, P);
    hipLaunchKernelGGL(k_gb_edge, gb_grid(A.T), dim3(kGbThreads), 0, st, A, 0);
    hipLaunchKernelGGL(k_gb_lm_sum, gb_grid(A.L), dim3(kGbThreads), 0, st, A, 0);
    hipLaunchKernelGGL(k_gb_decide, dim3(1), dim3(kGbThreads), 0, st, A);
    return hipGetLastError();
}
hipError_t gb_launch_finish(hipStream_t st, const GbArgs& A, bool stopped) {
    if (!stopped) {
        if (A.F > 0) hipLaunchKernelGGL(k_gb_out_kf, gb_grid(A.F), dim3(kGbThreads), 0, st, A);
        if (A.L > 0) hipLaunchKernelGGL(k_gb_out_lm, gb_grid(A.L), dim3(kGbThreads), 0, st, A);
    }
    hipLaunchKernelGGL(k_gb_out_rec, dim3(1), dim3(64), 0, st, A, stopped ? 1 : 0);
    return hipGetLastError();
}
hipError_t lp_launch(hipStream_t st, const LpArgs& A) {
    if (A.F > 0) hipLaunchKernelGGL(k_lp_kf, gb_grid(A.F), dim3(kGbThreads), 0, st, A);
    if (A.L > 0) hipLaunchKernelGGL(k_lp_lm, gb_grid(A.L), dim3(kGbThreads), 0, st, A);
    return hipGetLastError();
}

}  // namespace plp
