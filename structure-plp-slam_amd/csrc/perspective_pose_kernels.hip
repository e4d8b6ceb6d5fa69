// Map initialisation of the perspective and fisheye cameras, from the chosen matrix to the pose: perspective::reconstruct_with_H / reconstruct_with_F
// (plp_perspective_pose_*, include/plp_front.h; DESIGN.md section 5, D27 items e and h).  The arithmetic is perspective_init.hpp's and two_view.hpp's,
// which the host model runs too.
//
// One launch, one workgroup of four waves per problem, the layout of k_two_view_pose over eight or four hypotheses.  No result depends on the lane
// mapping: a match's triangulation and tests are a pure function of the problem's inputs, the counts are integer sums, and the parallax is an order
// statistic of a multiset.
// k_persp_pose<MODEL>:
//   1. lane 0 decomposes the chosen matrix in LDS: homography_solver::decompose into eight poses, or fundamental_solver::decompose into four.
//   2. per hypothesis, the slots 256 at a time, one lane per slot: an inlier match is triangulated and tested (tv_check<MODEL>, depth_is_positive
//      true); its point and flag go to the call's context buffers by slot, its cos_parallax as an ordered 32-bit key to a list in LDS at a
//      position taken with an LDS atomic (the list's order does not matter).
//   3. the key of rank min(50, n - 1) by the radix selection in LDS, eight bits a pass; lane 0 forms parallax_deg with D22's acos.
//   4. lane 0 chooses (base.cc:83-120 over the hypotheses that exist) and writes the per-problem outputs; every lane copies its slots' points and
//      flags of the chosen hypothesis.
// The points and flags of the hypotheses lie in buffers the context owns: the calls of one context must be ordered on the device.
#include <hip/hip_runtime.h>

#include "perspective_init.hpp"
#include "plp_barrier.hpp"

namespace plp {
namespace {

template <int MODEL>
__global__ __launch_bounds__(256) void k_persp_pose(PerspPoseArgs B) {
    __shared__ PerspPoseWs s_w;
    __shared__ double s_poses[kPerspMaxHyp * 12], s_c[3];
    __shared__ double s_coef[kPgCoefs];
    __shared__ uint32_t s_keys[kEssMaxSlots];
    __shared__ int s_hist[256];
    __shared__ int s_num, s_rank, s_nh;
    __shared__ uint32_t s_prefix;
    __shared__ int s_num_valid[kPerspMaxHyp], s_chosen;
    __shared__ float s_parallax[kPerspMaxHyp];
    const TvArgs& A = B.tv;
    const int p = blockIdx.x, tid = threadIdx.x;
    const size_t row = (size_t)p * A.n_cap;
    const int count_1 = clamp_count(A.counts_1, p, A.n_cap), count_2 = clamp_count(A.counts_2, p, A.m_cap);
    const int choice = B.in_choice[p];                              // uniform over the workgroup
    if (tid == 0) {
        int nh = 0;
        persp_cam_matrix(A, s_w.K);
        if (choice == PLP_PERSPECTIVE_CHOICE_H) nh = hom_decompose(B.H_21 + (size_t)9 * p, s_w, s_poses) ? 8 : 0;
        else if (choice == PLP_PERSPECTIVE_CHOICE_F) { fund_decompose(B.F_21 + (size_t)9 * p, s_w, s_poses); nh = 4; }
        s_nh = nh;
        pg_coef_init(s_coef);
    }
    if (tid < kPerspMaxHyp) { s_num_valid[tid] = 0; s_parallax[tid] = 0.0f; }
    wg_barrier();
    const int nh = s_nh;

    for (int h = 0; h < nh; ++h) {
        const double* pose = s_poses + 12 * h;
        if (tid == 0) {
            tv_center(pose, s_c);
            s_num = 0;
        }
        wg_barrier();
        double* pts = B.ctx_pts + ((size_t)p * kPerspMaxHyp + h) * A.n_cap * 3;
        uint8_t* flag = B.ctx_flag + ((size_t)p * kPerspMaxHyp + h) * A.n_cap;
        for (int base = 0; base < count_1; base += 256) {
            const int slot = base + tid;
            if (slot >= count_1) continue;
            double pos[3] = {0.0, 0.0, 0.0};
            int code = 0;
            if (A.inliers[row + slot] != 0) {
                const int m = A.match[row + slot];
                if (m >= 0 && m < count_2) {
                    const size_t s2 = (size_t)p * A.m_cap + m;
                    const double b1[3] = {A.bearing_1[3 * (row + slot)], A.bearing_1[3 * (row + slot) + 1], A.bearing_1[3 * (row + slot) + 2]};
                    const double b2[3] = {A.bearing_2[3 * s2], A.bearing_2[3 * s2 + 1], A.bearing_2[3 * s2 + 2]};
                    float cosp = 0.0f;
                    code = tv_check<MODEL>(A, pose, s_c, b1, b2, A.undist_1[row + slot].x, A.undist_1[row + slot].y, A.undist_2[s2].x, A.undist_2[s2].y, pos, cosp);
                    if (code >= kTvValidSmall) s_keys[atomicAdd(&s_num, 1)] = tv_key(cosp);   // at most one per slot: below kEssMaxSlots
                }
            }
            const bool tri = code == kTvValid;
            flag[slot] = tri ? 1 : 0;
#pragma unroll
            for (int i = 0; i < 3; ++i) pts[3 * (size_t)slot + i] = tri ? pos[i] : 0.0;
        }
        wg_barrier();
        const int num = s_num;
        if (num > 0) {                                              // uniform; the key of rank min(50, num - 1)
            if (tid == 0) { s_rank = num - 1 < kTvSortRank ? num - 1 : kTvSortRank; s_prefix = 0u; }
            for (int pass = 0; pass < 4; ++pass) {
                const int shift = 24 - 8 * pass;
                s_hist[tid] = 0;
                wg_barrier();
                const uint32_t prefix = s_prefix;
                for (int k = tid; k < num; k += 256) {
                    const uint32_t key = s_keys[k];
                    if (pass == 0 || (key >> (shift + 8)) == (prefix >> (shift + 8))) atomicAdd(&s_hist[(key >> shift) & 255u], 1);
                }
                wg_barrier();
                if (tid == 0) {
                    int rank = s_rank, b = 0;
                    while (b < 255 && rank >= s_hist[b]) { rank -= s_hist[b]; ++b; }
                    s_rank = rank;
                    s_prefix = prefix | ((uint32_t)b << shift);
                }
                wg_barrier();
            }
        }
        if (tid == 0) {
            s_num_valid[h] = num;
            s_parallax[h] = num > 0 ? tv_parallax_deg(tv_unkey(s_prefix), s_coef) : 0.0f;
        }
        wg_barrier();
    }

    if (tid == 0) {
        int chosen = -1;
        const int status = choice != PLP_PERSPECTIVE_CHOICE_H && choice != PLP_PERSPECTIVE_CHOICE_F ? (int)PLP_TWO_VIEW_NO_SOLUTION
                           : nh == 0 ? (int)PLP_PERSPECTIVE_POSE_NO_DECOMPOSITION
                                     : persp_select(s_num_valid, s_parallax, nh, A.min_num_triangulated, A.parallax_deg_thr, chosen);
        s_chosen = chosen;
        A.out_status[p] = (uint8_t)status;
        A.out_hypothesis[p] = chosen;
        const double* pose = s_poses + 12 * (chosen >= 0 ? chosen : 0);
        for (int i = 0; i < 9; ++i) A.out_rot[(size_t)9 * p + i] = chosen >= 0 ? persp_out(pose[i]) : 0.0;
        for (int i = 0; i < 3; ++i) A.out_trans[(size_t)3 * p + i] = chosen >= 0 ? persp_out(pose[9 + i]) : 0.0;
        for (int h = 0; h < kPerspMaxHyp; ++h) {
            A.out_num_valid[(size_t)kPerspMaxHyp * p + h] = s_num_valid[h];
            A.out_parallax_deg[(size_t)kPerspMaxHyp * p + h] = s_parallax[h];
        }
    }
    wg_barrier();
    const int chosen = s_chosen;
    const int hc = chosen >= 0 ? chosen : 0;
    const double* cpts = B.ctx_pts + ((size_t)p * kPerspMaxHyp + hc) * A.n_cap * 3;    // written by this lane for these slots
    const uint8_t* cflag = B.ctx_flag + ((size_t)p * kPerspMaxHyp + hc) * A.n_cap;
    for (int slot = tid; slot < count_1; slot += 256) {
        const bool tri = chosen >= 0 && cflag[slot] != 0;
        A.out_is_triangulated[row + slot] = tri ? 1 : 0;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const double v = chosen >= 0 ? cpts[3 * (size_t)slot + i] : 0.0;
            A.out_pts[3 * (row + slot) + i] = tri ? v : 0.0;
        }
        if (A.out_hyp_is_triangulated)
            for (int h = 0; h < kPerspMaxHyp; ++h)
                A.out_hyp_is_triangulated[((size_t)p * kPerspMaxHyp + h) * A.n_cap + slot] =
                    h < nh && B.ctx_flag[((size_t)p * kPerspMaxHyp + h) * A.n_cap + slot] != 0 ? 1 : 0;
    }
}

}  // namespace

hipError_t launch_perspective_pose(hipStream_t st, const PerspPoseArgs& A) {
    if (A.tv.model == PLP_CAMERA_PERSPECTIVE) hipLaunchKernelGGL(k_persp_pose<PLP_CAMERA_PERSPECTIVE>, dim3(A.tv.P), dim3(256), 0, st, A);
    else hipLaunchKernelGGL(k_persp_pose<PLP_CAMERA_FISHEYE>, dim3(A.tv.P), dim3(256), 0, st, A);
    return hipGetLastError();
}

}  // namespace plp
