// Plane fitting: Planar_Mapping_module's RANSAC loops and refine_points (plp_plane_ransac_*, plp_plane_refine_points_*, include/plp_front.h;
// DESIGN.md section 5, D19; the reformulation: DESIGN.md section 4).  The arithmetic is plane_fit.hpp's, which the host model runs too.
//
// Two launches for the RANSAC, one workgroup of four waves per plane in each.  No result depends on the launch shape: a hypothesis is
// computed from the problem's inputs alone, every floating-point sum has D19's shape (lane j of a wave owns partial chain j; the 64 partials
// are chained in lane order by reading the lanes one after the other), counts are integer sums, and nothing is accumulated with atomics in
// floating point.
// k_plane_hypotheses:
//   1. the eligible and the non-erased slots are compacted in slot order, 256 slots at a time (64-bit ballot within the wave, the waves'
//      totals through LDS): s_elig[rank] = slot is what a sample rank means, s_live is the list step [2] scans;
//   2. hypotheses are dealt to the waves, wave w takes w, w + 4, ...  The wave fits its samples (three passes: centroid, scatter,
//      residual; the points come from L2, the 3 x 3 Jacobi runs in lane 0 on work arrays in LDS), scans the non-erased slots 64 at a time
//      and appends the inliers to its own list in LDS by ballot and prefix, fits that list when the gate holds, and lane 0 writes the
//      record -- both equations, residual, error, the inlier count, whether the refit was tried -- to the call's context buffer.
//      The waves do not meet again after step 1.
// k_plane_finish:
//   3. the records' residuals, errors and gates go to LDS and every lane replays the reference's loop over them (the running minimum, the
//      acceptances, CREATE's break): the last iteration that ran and the owner of best_inliers_list;
//   4. one pass over the slots writes step [4]'s membership, lane 0 the rest of the outputs.
// k_plane_refine_points: one landmark per lane.
#include <hip/hip_runtime.h>

#include "plane_fit.hpp"
#include "plane_team.hpp"
#include "plp_barrier.hpp"

namespace plp {
namespace {

constexpr int kPlaneWaves = 4;

__device__ __forceinline__ double* hyp_record(const PlaneArgs& A, int p, int it) { return A.ctx_hyp + ((size_t)p * A.iters + it) * kPlaneHypDoubles; }

__global__ __launch_bounds__(256) void k_plane_hypotheses(PlaneArgs A) {
    __shared__ uint16_t s_elig[kPlaneMaxSlots];
    __shared__ uint16_t s_live[kPlaneMaxSlots];
    __shared__ uint16_t s_list[kPlaneWaves][kPlaneMaxSlots];
    __shared__ double s_work[kPlaneWaves][kPlaneWorkDoubles];
    __shared__ int s_wave_n[2][kPlaneWaves];

    const int p = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int n = clamp_count(A.counts, p, A.n_cap);
    const size_t row = (size_t)p * A.n_cap;
    const double* pos = A.pos_w + 3 * row;
    const unsigned long long below = (1ull << lane) - 1ull;

    int n_elig = 0, n_live = 0;
    for (int base = 0; base < n; base += 256) {
        const int slot = base + tid;
        const uint8_t f = slot < n ? A.flags[row + slot] : (uint8_t)PLP_PLANE_LM_ERASED;
        const bool e = slot < n && plane_eligible(A.mode, f), l = slot < n && plane_live(f);
        const unsigned long long me = __ballot(e), ml = __ballot(l);
        if (lane == 0) { s_wave_n[0][w] = (int)__popcll(me); s_wave_n[1][w] = (int)__popcll(ml); }
        wg_barrier();
        int off_e = n_elig, off_l = n_live, tot_e = 0, tot_l = 0;
#pragma unroll
        for (int u = 0; u < kPlaneWaves; ++u) {
            if (u < w) { off_e += s_wave_n[0][u]; off_l += s_wave_n[1][u]; }
            tot_e += s_wave_n[0][u]; tot_l += s_wave_n[1][u];
        }
        if (e) s_elig[off_e + (int)__popcll(me & below)] = (uint16_t)slot;
        if (l) s_live[off_l + (int)__popcll(ml & below)] = (uint16_t)slot;
        n_elig += tot_e; n_live += tot_l;
        wg_barrier();   // s_wave_n is rewritten by the next round; the last one publishes the two lists
    }
    int early_flags;
    if (plane_early_status(A, n, n_elig, early_flags) != PLP_PLANE_OK) return;   // uniform; k_plane_finish writes the outputs

    const int m = plane_sample_size(A.mode, n, A.points_per_ransac);
    const double thr = A.dist_thresh[p];
    PlaneWaveTeam T{lane, s_work[w]};
    uint16_t* list = s_list[w];
    for (int it = w; it < A.iters; it += kPlaneWaves) {
        double eq_s[4], res;
        int sweeps;
        const int32_t* smp = A.samples ? A.samples + ((size_t)p * A.iters + it) * A.m_cap : nullptr;
        plane_fit(T, [&](int k, double x[3]) {
            const int rank = smp ? smp[k] : ransac_draw_one(A.seed, p, it, k, n_elig);
            if ((unsigned)rank >= (unsigned)n_elig) return false;
            const double* q = pos + 3 * (size_t)s_elig[rank];
            x[0] = q[0]; x[1] = q[1]; x[2] = q[2];
            return true;
        }, m, eq_s, res, sweeps);
        const double abs_n = plane_abs_n(eq_s);
        int cnt = 0;
        for (int base = 0; base < n_live; base += 64) {   // step [2]: the inliers in slot order
            const int r = base + lane;
            bool in = false;
            int slot = 0;
            if (r < n_live) {
                slot = s_live[r];
                const double* q = pos + 3 * (size_t)slot;
                const double x[3] = {q[0], q[1], q[2]};
                in = plane_distance(eq_s, abs_n, x) < thr;
            }
            const unsigned long long mk = __ballot(in);
            if (in) list[cnt + (int)__popcll(mk & below)] = (uint16_t)slot;
            cnt += (int)__popcll(mk);
        }
        __builtin_amdgcn_wave_barrier();                  // the list is read by other lanes of this wave: LDS keeps a wave's order
        const bool tried = plane_refit_gate(A, n, cnt);
        double eq_r[4] = {0.0, 0.0, 0.0, 0.0}, err = kPlaneMax;
        if (tried)                                        // uniform over the wave
            plane_fit(T, [&](int k, double x[3]) {
                const double* q = pos + 3 * (size_t)list[k];
                x[0] = q[0]; x[1] = q[1]; x[2] = q[2];
                return true;
            }, cnt, eq_r, err, sweeps);
        __builtin_amdgcn_wave_barrier();                  // the next iteration rewrites the list
        if (lane == 0) {
            double* rec = hyp_record(A, p, it);
#pragma unroll
            for (int i = 0; i < 4; ++i) { rec[i] = eq_s[i]; rec[5 + i] = eq_r[i]; }
            rec[4] = res; rec[9] = err; rec[10] = (double)cnt; rec[11] = tried ? 1.0 : 0.0;
        }
    }
}

// The second launch: what the first left per hypothesis in the context buffer becomes the outputs.
__global__ __launch_bounds__(256) void k_plane_finish(PlaneArgs A) {
    __shared__ double s_res[kPlaneMaxIters];
    __shared__ double s_err[kPlaneMaxIters];
    __shared__ uint8_t s_tried[kPlaneMaxIters];
    __shared__ int s_n[2];                                // eligible slots; members of step [4]

    const int p = blockIdx.x, tid = threadIdx.x, lane = tid & 63, I = A.iters;
    const int n = clamp_count(A.counts, p, A.n_cap);
    const size_t row = (size_t)p * A.n_cap;
    const double* pos = A.pos_w + 3 * row;
    if (tid < 2) s_n[tid] = 0;
    wg_barrier();
    for (int base = 0; base < n; base += 256) {
        const int slot = base + tid;
        const bool e = slot < n && plane_eligible(A.mode, A.flags[row + slot]);
        const unsigned long long me = __ballot(e);
        if (lane == 0 && me) atomicAdd(&s_n[0], (int)__popcll(me));
    }
    wg_barrier();
    const int n_elig = s_n[0];
    int flags;
    const int early = plane_early_status(A, n, n_elig, flags);
    if (early != PLP_PLANE_OK) {                          // uniform
        if (tid == 0) {
            A.out_status[p] = (uint8_t)early; A.out_flags[p] = (uint8_t)flags;
            if (A.mode == PLP_PLANE_UPDATE) {
#pragma unroll
                for (int i = 0; i < 4; ++i) A.out_equation[4 * (size_t)p + i] = A.equation_in[4 * (size_t)p + i];
                A.out_best_error[p] = A.best_error_in[p];
            }
            A.out_best_iter[p] = -1; A.out_last_iter[p] = -1; A.out_num_inliers[p] = 0;
        }
        for (int s = tid; s < n; s += 256) A.out_inliers[row + s] = 0;
        for (int it = tid; it < I; it += 256) {
            if (A.out_hyp_residual) A.out_hyp_residual[(size_t)p * I + it] = 0.0;
            if (A.out_hyp_inliers) A.out_hyp_inliers[(size_t)p * I + it] = 0;
            if (A.out_hyp_error) A.out_hyp_error[(size_t)p * I + it] = kPlaneMax;
        }
        return;
    }
    for (int it = tid; it < I; it += 256) {
        const double* rec = hyp_record(A, p, it);
        const double res = rec[4], err = rec[9];
        s_res[it] = res; s_err[it] = err; s_tried[it] = rec[11] != 0.0 ? 1 : 0;
        if (A.out_hyp_residual) A.out_hyp_residual[(size_t)p * I + it] = res;
        if (A.out_hyp_inliers) A.out_hyp_inliers[(size_t)p * I + it] = (int)rec[10];
        if (A.out_hyp_error) A.out_hyp_error[(size_t)p * I + it] = err;
    }
    wg_barrier();
    const double error_thresh = A.error_thresh[p], thr = A.dist_thresh[p];
    const PlaneReplay R = plane_replay(A.mode, I, A.mode == PLP_PLANE_UPDATE ? A.best_error_in[p] : 0.0, error_thresh,
                                       [&](int i) { return s_res[i]; }, [&](int i) { return s_tried[i] != 0; }, [&](int i) { return s_err[i]; });
    int status = plane_late_status(A.mode, R, error_thresh, flags);
    const double* rec_l = hyp_record(A, p, R.last_iter) + (R.last_refit ? 5 : 0);
    const double* rec_b = hyp_record(A, p, R.best_iter < 0 ? R.last_iter : R.best_iter);
    const double eq[4] = {rec_l[0], rec_l[1], rec_l[2], rec_l[3]}, eq_b[4] = {rec_b[0], rec_b[1], rec_b[2], rec_b[3]};
    const double abs_n = plane_abs_n(eq), abs_b = plane_abs_n(eq_b);
    for (int base = 0; base < n; base += 256) {           // step [4] (:564-579, :704-720)
        const int s = base + tid;
        bool in = false;
        if (s < n) {
            if (status == PLP_PLANE_OK && plane_live(A.flags[row + s])) {
                const double* q = pos + 3 * (size_t)s;
                const double x[3] = {q[0], q[1], q[2]};
                in = plane_distance(eq_b, abs_b, x) < thr && plane_distance(eq, abs_n, x) < thr;
            }
            A.out_inliers[row + s] = in ? 1 : 0;
        }
        const unsigned long long mk = __ballot(in);
        if (lane == 0 && mk) atomicAdd(&s_n[1], (int)__popcll(mk));
    }
    wg_barrier();
    if (tid == 0) {
        const int num = s_n[1];
        if (status == PLP_PLANE_OK && A.mode == PLP_PLANE_UPDATE && num < A.points_per_ransac) { status = PLP_PLANE_TOO_FEW_LEFT; flags = PLP_PLANE_FLAG_INVALID; }   // :722
        A.out_status[p] = (uint8_t)status; A.out_flags[p] = (uint8_t)flags;
#pragma unroll
        for (int i = 0; i < 4; ++i) A.out_equation[4 * (size_t)p + i] = eq[i];
        A.out_best_error[p] = R.plane_error;
        A.out_best_iter[p] = R.best_iter; A.out_last_iter[p] = R.last_iter; A.out_num_inliers[p] = num;
    }
}

__global__ __launch_bounds__(256) void k_plane_refine_points(PlaneRefineArgs A) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < A.M) plane_refine_landmark(A, i);
}

}  // namespace

hipError_t launch_plane_ransac(hipStream_t st, const PlaneArgs& A) {
    hipLaunchKernelGGL(k_plane_hypotheses, dim3(A.P), dim3(256), 0, st, A);
    hipLaunchKernelGGL(k_plane_finish, dim3(A.P), dim3(256), 0, st, A);
    return hipGetLastError();
}

hipError_t launch_plane_refine_points(hipStream_t st, const PlaneRefineArgs& A) {
    hipLaunchKernelGGL(k_plane_refine_points, dim3((A.M + 255) / 256), dim3(256), 0, st, A);
    return hipGetLastError();
}

}  // namespace plp
