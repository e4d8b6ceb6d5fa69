// Loop candidates: solve::sim3_solver's constructor and find_via_ransac (plp_sim3_ransac_*, include/plp_front.h).
// The arithmetic is sim3.hpp's, which the host model runs too.
//
// Three launches, one workgroup of four waves per problem in each.  The lane-to-work mapping is fixed and no result depends on it: every
// hypothesis and every point is computed by exactly one lane from the problem's inputs alone, counts are integer sums, and the winner is
// the maximum of a key that is unique per iteration.
// k_sim3_hypotheses:
//   1. the valid slots are compacted in slot order, 256 slots at a time (64-bit ballot within the wave, the waves' totals through LDS):
//      s_slot[rank] = slot, the rank being what a sample index means;
//   2. hypotheses go one to a lane, 256 at a time: the lane takes its three samples, gathers their world points, runs horn_sim3 in
//      registers and writes (scale * rot, trans) of both directions, rot_12, trans_12 and scale_12 to the call's context buffer.
// k_sim3_count<MODEL>:
//   3. the compaction again, then 256 hypotheses at a time, each lane with the 24 doubles of its own.  The common points go through LDS
//      in tiles of kSim3Tile: a lane forms the constants of one point of the tile (camera-frame points, own reprojections, the two float
//      thresholds, the "never an inlier" bit), then every lane tests the whole tile against its hypothesis -- all lanes read the same LDS
//      address, a broadcast.  The tile is rebuilt for every chunk of 256 hypotheses (one point per lane: small beside the chunk's
//      256 x tile inlier tests); the slot limit does not depend on the LDS size;
//   4. the best hypothesis is the workgroup maximum of (count << 32 | ~iter): more inliers win, among equal counts the lowest iteration.
// k_sim3_finish<MODEL>:
//   5. lane 0 writes the outputs from the context buffers and one pass over the slots writes out_inliers.
// Horn's fit and the counting are separate kernels for their registers: in one kernel the Jacobi, the two sets of (R, t, s) and the
// equirectangular camera's asin / atan2 (whose coefficients the compiler keeps in scalar registers across the loops) spilled 24 - 31
// scalar registers, above what tests/test_kernel_resources.py allows.
#include <hip/hip_runtime.h>

#include "plp_barrier.hpp"
#include "ransac_device.hpp"
#include "sim3.hpp"

namespace plp {
namespace {

constexpr int kSim3Tile = 256;   // common points per LDS tile: one per lane

// step 1 of both kernels below: the valid slots of problem p in slot order, s_slot[rank] = slot; returns their number.  Uniform over the
// workgroup; ends with a barrier.
__device__ __forceinline__ int compact_slots(const Sim3Args& A, int p, int count, uint16_t (&s_slot)[kSim3MaxSlots], int (&s_wave_n)[4]) {
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const size_t row = (size_t)p * A.n_cap;
    int n = 0;
    for (int base = 0; base < count; base += 256) {
        const int slot = base + tid;
        const bool v = slot < count && A.valid[row + slot] != 0;
        const unsigned long long m = __ballot(v);
        if (lane == 0) s_wave_n[w] = (int)__popcll(m);
        wg_barrier();
        int off = n, tot = 0;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (u < w) off += s_wave_n[u];
            tot += s_wave_n[u];
        }
        if (v) s_slot[off + (int)__popcll(m & ((1ull << lane) - 1ull))] = (uint16_t)slot;
        n += tot;
        wg_barrier();   // s_wave_n is rewritten by the next round; the last one publishes s_slot
    }
    return n;
}

// hypothesis `it` of problem p in the context buffer: kSim3HypDoubles fields, each a row of `iters` doubles (lanes of a wave write and
// read neighbouring addresses)
__device__ __forceinline__ double* hyp_field(const Sim3Args& A, int p, int field) { return A.ctx_hyp + ((size_t)p * kSim3HypDoubles + field) * A.iters; }

__global__ __launch_bounds__(256) void k_sim3_hypotheses(Sim3Args A) {
    __shared__ uint16_t s_slot[kSim3MaxSlots];
    __shared__ double s_pose[2][12];
    __shared__ int s_wave_n[4];
    const int p = blockIdx.x, tid = threadIdx.x;
    if (tid < 12) { s_pose[0][tid] = A.pose_1[(size_t)15 * p + tid]; s_pose[1][tid] = A.pose_2[(size_t)15 * p + tid]; }
    const int n = compact_slots(A, p, clamp_count(A.counts, p, A.n_cap), s_slot, s_wave_n);   // its barriers publish s_pose too (count == 0: nothing reads it)
    const bool enough = !(n < 3 || n < A.min_num_inliers);   // :130
    if (tid == 0) A.ctx[(size_t)kSim3CtxInts * p] = n;
    for (int it = tid; it < A.iters; it += 256) {
        int idx[3];
        const bool hyp = enough && ransac_sample<3>(A, p, it, n, idx);
        hyp_field(A, p, 37)[it] = hyp ? 1.0 : 0.0;
        if (!hyp) continue;
        const int slot[3] = {s_slot[idx[0]], s_slot[idx[1]], s_slot[idx[2]]};
        Sim3Hyp H;
        sim3_hypothesis(A, s_pose[0], s_pose[1], p, slot, H);
        double m21[12], m12[12];
        sim3_pose_row(H.rot_21, H.trans_21, H.scale_21, m21);
        sim3_pose_row(H.rot_12, H.trans_12, H.scale_12, m12);
#pragma unroll
        for (int i = 0; i < 12; ++i) { hyp_field(A, p, i)[it] = m21[i]; hyp_field(A, p, 12 + i)[it] = m12[i]; }
#pragma unroll
        for (int i = 0; i < 9; ++i) hyp_field(A, p, 24 + i)[it] = H.rot_12[i];
#pragma unroll
        for (int i = 0; i < 3; ++i) hyp_field(A, p, 33 + i)[it] = H.trans_12[i];
        hyp_field(A, p, 36)[it] = (double)H.scale_12;
    }
}

template <int MODEL>
__global__ __launch_bounds__(256) void k_sim3_count(Sim3Args A) {
    __shared__ uint16_t s_slot[kSim3MaxSlots];
    __shared__ double s_pt[10][kSim3Tile];      // x1 (3), x2 (3), u1, v1, u2, v2
    __shared__ float s_thr[2][kSim3Tile];
    __shared__ uint8_t s_never[kSim3Tile];
    __shared__ float s_sigma[2][16];
    __shared__ double s_pose[2][12];
    __shared__ int s_wave_n[4];
    __shared__ unsigned long long s_part[4];

    const int p = blockIdx.x, tid = threadIdx.x;
    if (tid < 16) { s_sigma[0][tid] = A.level_sigma_sq_1[tid]; s_sigma[1][tid] = A.level_sigma_sq_2[tid]; }
    if (tid < 12) { s_pose[0][tid] = A.pose_1[(size_t)15 * p + tid]; s_pose[1][tid] = A.pose_2[(size_t)15 * p + tid]; }
    const int n = compact_slots(A, p, clamp_count(A.counts, p, A.n_cap), s_slot, s_wave_n);   // its barriers publish s_sigma and s_pose too
    const bool enough = !(n < 3 || n < A.min_num_inliers);   // :130

    unsigned long long key = 0;
    for (int chunk = 0; chunk < A.iters; chunk += 256) {
        const int it = chunk + tid;
        const bool live = it < A.iters;
        const bool hyp = live && enough && hyp_field(A, p, 37)[it] != 0.0;
        double m21[12], m12[12];
#pragma unroll
        for (int i = 0; i < 12; ++i) {
            m21[i] = hyp ? hyp_field(A, p, i)[it] : 0.0;
            m12[i] = hyp ? hyp_field(A, p, 12 + i)[it] : 0.0;
        }
        int num = 0;
        if (enough) {   // uniform over the workgroup
            for (int tile = 0; tile < n; tile += kSim3Tile) {
                const int k = tile + tid;
                if (k < n) {
                    const Sim3Point q = sim3_point<MODEL>(A, s_pose[0], s_pose[1], s_sigma[0], s_sigma[1], p, s_slot[k]);
#pragma unroll
                    for (int r = 0; r < 3; ++r) { s_pt[r][tid] = q.x1[r]; s_pt[3 + r][tid] = q.x2[r]; }
                    s_pt[6][tid] = q.u1; s_pt[7][tid] = q.v1; s_pt[8][tid] = q.u2; s_pt[9][tid] = q.v2;
                    s_thr[0][tid] = q.thr_1; s_thr[1][tid] = q.thr_2;
                    s_never[tid] = q.never ? 1 : 0;
                }
                wg_barrier();
                const int m = n - tile < kSim3Tile ? n - tile : kSim3Tile;
                if (hyp) {
                    for (int j = 0; j < m; ++j) {
                        const double x1[3] = {s_pt[0][j], s_pt[1][j], s_pt[2][j]}, x2[3] = {s_pt[3][j], s_pt[4][j], s_pt[5][j]};
                        num += sim3_inlier<MODEL>(A, m21, m12, x1, x2, s_pt[6][j], s_pt[7][j], s_pt[8][j], s_pt[9][j], s_thr[0][j], s_thr[1][j],
                                                  s_never[j] != 0) ? 1 : 0;
                    }
                }
                wg_barrier();   // the next tile, or the next chunk, rewrites the arrays
            }
        }
        if (live) {
            if (A.out_hyp_inliers) A.out_hyp_inliers[(size_t)p * A.iters + it] = num;
            const unsigned long long mine = ransac_key((unsigned)num, it);
            key = mine > key ? mine : key;
        }
    }
    key = wg_max_u64(key, s_part);
    if (tid == 0) {
        const int best_count = (int)(key >> 32);
        int32_t* c = A.ctx + (size_t)kSim3CtxInts * p;
        c[1] = best_count;
        c[2] = best_count > 0 ? ransac_key_iter(key) : -1;
    }
}

// The third launch: what the first two left per problem in the context buffers -- num_common, the best count, its iteration, the
// hypotheses -- becomes the outputs; one pass over the slots writes out_inliers.
template <int MODEL>
__global__ __launch_bounds__(256) void k_sim3_finish(Sim3Args A) {
    __shared__ float s_sigma[2][16];
    __shared__ double s_pose[2][12];
    const int p = blockIdx.x, tid = threadIdx.x;
    const size_t row = (size_t)p * A.n_cap;
    const int count = clamp_count(A.counts, p, A.n_cap);
    if (tid < 16) { s_sigma[0][tid] = A.level_sigma_sq_1[tid]; s_sigma[1][tid] = A.level_sigma_sq_2[tid]; }
    if (tid < 12) { s_pose[0][tid] = A.pose_1[(size_t)15 * p + tid]; s_pose[1][tid] = A.pose_2[(size_t)15 * p + tid]; }
    wg_barrier();
    const int32_t* c = A.ctx + (size_t)kSim3CtxInts * p;
    const int n = c[0], best_count = c[1], best_iter = c[2];
    const bool enough = !(n < 3 || n < A.min_num_inliers);         // :130
    const bool ok = enough && !(best_count < A.min_num_inliers);   // :177
    const bool have = ok && best_iter >= 0 && best_iter < A.iters;
    double m21[12], m12[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) {
        m21[i] = have ? hyp_field(A, p, i)[best_iter] : 0.0;
        m12[i] = have ? hyp_field(A, p, 12 + i)[best_iter] : 0.0;
    }
    if (tid == 0) {
        A.out_status[p] = !enough ? PLP_SIM3_TOO_FEW_POINTS : ok ? PLP_SIM3_OK : PLP_SIM3_TOO_FEW_INLIERS;
        A.out_num_common[p] = n;
        A.out_num_inliers[p] = best_count;
        A.out_best_iter[p] = ok ? best_iter : -1;
        A.out_scale_12[p] = have ? (float)hyp_field(A, p, 36)[best_iter] : 0.0f;
#pragma unroll
        for (int i = 0; i < 9; ++i) A.out_rot_12[(size_t)9 * p + i] = have ? hyp_field(A, p, 24 + i)[best_iter] : 0.0;
#pragma unroll
        for (int i = 0; i < 3; ++i) A.out_trans_12[(size_t)3 * p + i] = have ? hyp_field(A, p, 33 + i)[best_iter] : 0.0;
    }
    if (A.out_inliers) {
        for (int slot = tid; slot < count; slot += 256) {
            bool in = false;
            if (have && A.valid[row + slot] != 0) {
                const Sim3Point q = sim3_point<MODEL>(A, s_pose[0], s_pose[1], s_sigma[0], s_sigma[1], p, slot);
                in = sim3_inlier<MODEL>(A, m21, m12, q.x1, q.x2, q.u1, q.v1, q.u2, q.v2, q.thr_1, q.thr_2, q.never);
            }
            A.out_inliers[row + slot] = in ? 1 : 0;
        }
    }
}

template <int MODEL> hipError_t launch_model(hipStream_t st, const Sim3Args& A) {
    hipLaunchKernelGGL(k_sim3_hypotheses, dim3(A.P), dim3(256), 0, st, A);
    hipLaunchKernelGGL(k_sim3_count<MODEL>, dim3(A.P), dim3(256), 0, st, A);
    hipLaunchKernelGGL(k_sim3_finish<MODEL>, dim3(A.P), dim3(256), 0, st, A);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_sim3_ransac(hipStream_t st, const Sim3Args& A) {
    if (A.model == PLP_CAMERA_PERSPECTIVE) return launch_model<PLP_CAMERA_PERSPECTIVE>(st, A);
    if (A.model == PLP_CAMERA_FISHEYE) return launch_model<PLP_CAMERA_FISHEYE>(st, A);
    return launch_model<PLP_CAMERA_EQUIRECTANGULAR>(st, A);
}

}  // namespace plp
