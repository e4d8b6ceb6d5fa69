// Key-frame pair point triangulation (plp_keyframe_pair_geometry_* / plp_triangulate_keypoint_pairs_*, include/plp_front.h).
//
// k_keyframe_pair_geometry: what mapping_module::create_new_landmarks (mapping_module.cc:386-402) and triangulate_with_two_keyframes (:429)
// compute per neighbour in front of robust::match_for_triangulation: the baseline gate, E_12 = create_E_21 (solve/essential_solver.cc:188-194)
// and the epipole bearing (match/robust.cc:50-55, camera::*::reproject_to_bearing).  One lane per pair.
//
// k_triangulate_keypoint_pairs<MODEL>: module::two_view_triangulator::triangulate (module/two_view_triangulator.cc:45-122, .h:114-137) for
// every matched key point of key frame 2, one lane per key point t, the pair along y: the pose rows, the camera and the level tables are
// uniform over a wave.  A workgroup first finishes its unmatched slots, then packs the matched ones into its first lanes (a ballot per
// wave, 1 KB of LDS, two barriers) and triangulates those.  The two-camera branch takes the null vector of null4.hpp; its sweep count
// differs from lane to lane, finished lanes wait.  Numeric contract: DESIGN.md section 5, D10 (the file is compiled with -ffp-contract=off).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "match_device.hpp"
#include "null4.hpp"
#include "plp_barrier.hpp"
#include "reproject.hpp"

namespace plp {
namespace {

enum : uint8_t {
    kCreated = PLP_KPP_CREATED, kPairSkipped = PLP_KPP_PAIR_SKIPPED, kNoMatch = PLP_KPP_NO_MATCH, kNoParallax = PLP_KPP_NO_PARALLAX,
    kDepth = PLP_KPP_DEPTH, kReproj1 = PLP_KPP_REPROJ_1, kReproj2 = PLP_KPP_REPROJ_2, kScale = PLP_KPP_SCALE, kNonFinite = PLP_KPP_NON_FINITE,
    kIndexRange = PLP_KPP_INDEX_RANGE
};

__device__ __forceinline__ int clamp_count(const int32_t* counts, int f, int cap) { return counts ? min(max(counts[f], 0), cap) : cap; }

// ---------------------------------------------------------------------------------------------------------------- pair geometry
__global__ __launch_bounds__(256) void k_keyframe_pair_geometry(PairGeometryArgs A) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= A.P) return;
    const int f1 = A.pairs[2 * p], f2 = A.pairs[2 * p + 1];
    if ((unsigned)f1 >= (unsigned)A.F || (unsigned)f2 >= (unsigned)A.F) return;   // outside the table: nothing read, nothing written
    const double* P1 = A.pose + (size_t)15 * f1;   // cur
    const double* P2 = A.pose + (size_t)15 * f2;   // ngh
    // baseline_vec = ngh_cam_center - cur_cam_center (:382-383)
    const double dist = norm3(P2[12] - P1[12], P2[13] - P1[13], P2[14] - P1[14]);
    bool skip;
    if (A.setup_type == 0) skip = dist < 0.02 * (double)A.median[f2];   // 0.02 * (float) median_depth_in_ngh (:389)
    else skip = dist < A.true_baseline;                                 // :397
    A.out_skip[p] = skip ? 1 : 0;
    A.out_baseline[p] = dist;
    // create_E_21(rot_1w = ngh's, trans_1w = ngh's, rot_2w = cur's, trans_2w = cur's): rot_21 = rot_2w * rot_1w^T
    double R[9], tr[3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int k = 0; k < 3; ++k) R[3 * i + k] = (P1[3 * i] * P2[3 * k] + P1[3 * i + 1] * P2[3 * k + 1]) + P1[3 * i + 2] * P2[3 * k + 2];
    // trans_21 = -rot_21 * trans_1w + trans_2w
#pragma unroll
    for (int i = 0; i < 3; ++i) tr[i] = (((-R[3 * i]) * P2[9] + (-R[3 * i + 1]) * P2[10]) + (-R[3 * i + 2]) * P2[11]) + P1[9 + i];
    // to_skew_symmetric_mat(trans_21) * rot_21, the zero entries included
    const double S[9] = {0.0, -tr[2], tr[1], tr[2], 0.0, -tr[0], -tr[1], tr[0], 0.0};
    double* out = A.out_epipolar + (size_t)12 * p;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int k = 0; k < 3; ++k) out[3 * i + k] = (S[3 * i] * R[k] + S[3 * i + 1] * R[3 + k]) + S[3 * i + 2] * R[6 + k];
    // reproject_to_bearing(rot_2w, trans_2w, cam_center_1) in key frame 2; its return value is ignored (robust.cc:55)
    const double x = P1[12], y = P1[13], z = P1[14];
    double bx = ((P2[0] * x + P2[1] * y) + P2[2] * z) + P2[9];
    double by = ((P2[3] * x + P2[4] * y) + P2[5] * z) + P2[10];
    double bz = ((P2[6] * x + P2[7] * y) + P2[8] * z) + P2[11];
    // perspective.cc:217-220, fisheye.cc:258-261: z <= 0 returns before normalize(), the vector stays as it is
    if (A.model == PLP_CAMERA_EQUIRECTANGULAR || !(bz <= 0.0)) {
        const double sq = (bx * bx + by * by) + bz * bz;   // Eigen 3.3 normalize(): v /= sqrt(squaredNorm) when it is positive
        if (sq > 0.0) {
            const double s = sqrt(sq);
            bx = bx / s; by = by / s; bz = bz / s;
        }
    }
    out[9] = bx; out[10] = by; out[11] = bz;
}

// ---------------------------------------------------------------------------------------------------------------- triangulation
// row i of rot_w? = rot_?w^T is column i of the pose row's rot_cw
__device__ __forceinline__ void turn_to_world(const double* P, const double* c, double (&w)[3]) {
#pragma unroll
    for (int i = 0; i < 3; ++i) w[i] = (P[i] * c[0] + P[3 + i] * c[1]) + P[6 + i] * c[2];
}

// keyframe::triangulate_stereo (data/keyframe.cc:589-640), perspective and fisheye: the same lines
__device__ __forceinline__ void triangulate_stereo(const KeypointPairArgs& A, const double* P, const plp_keypoint& kp, float depth, double (&pos)[3]) {
    if (0.0 < (double)depth) {
        const float ux = (float)((((double)kp.x - A.cx) * (double)depth) * A.fx_inv);
        const float uy = (float)((((double)kp.y - A.cy) * (double)depth) * A.fy_inv);
        const double c[3] = {(double)ux, (double)uy, (double)depth};
#pragma unroll
        for (int i = 0; i < 3; ++i) pos[i] = ((P[i] * c[0] + P[3 + i] * c[1]) + P[6 + i] * c[2]) + P[12 + i];   // rot_wc * pos_c + cam_center
    } else {
        pos[0] = 0.0; pos[1] = 0.0; pos[2] = 0.0;
    }
}

// check_reprojection_error (.cc:124-158) -> 0 passed, 1 rejected, 2 non-finite
template <int MODEL>
__device__ __forceinline__ int reprojection_check(const KeypointPairArgs& A, const double* P, const double (&pos)[3], const plp_keypoint& kp,
                                                  float x_right, float sigma_sq, bool is_stereo) {
    const Reproj r = reproject<MODEL>(A, P, pos[0], pos[1], pos[2]);
    if (!r.wrote) return 1;                        // z <= 0: not reachable behind check_depth_is_positive, which formed the same sum
    const double ex = r.u - (double)kp.x, ey = r.v - (double)kp.y;   // Vec2_t - cv::Point2f: the key point widened to f64
    const double sq = ex * ex + ey * ey;
    if (is_stereo) {
        const float exr = (float)r.xr - x_right;   // float x_right_in_cur - float x_right
        const double total = sq + (double)(exr * exr);
        if (!isfinite(total)) return 2;
        return (double)(7.81473f * sigma_sq) < total ? 1 : 0;
    }
    if (!isfinite(sq)) return 2;
    return (double)(5.99146f * sigma_sq) < sq ? 1 : 0;
}

template <int MODEL>
__device__ uint8_t triangulate_keypoints(const KeypointPairArgs& A, int f1, int f2, int j, int t, double (&pos)[3]) {
    const size_t o1 = (size_t)f1 * A.cap + j, o2 = (size_t)f2 * A.cap + t;
    const plp_keypoint& k1 = A.kps[o1];
    const plp_keypoint& k2 = A.kps[o2];
    const double* P1 = A.pose + (size_t)15 * f1;
    const double* P2 = A.pose + (size_t)15 * f2;
    // a monocular setup holds -1 in every stereo_x_right_: the arrays are not read
    const bool stereo_setup = MODEL != PLP_CAMERA_EQUIRECTANGULAR && A.setup_type != 0;
    const float xr1 = stereo_setup ? A.x_right[o1] : -1.0f, xr2 = stereo_setup ? A.x_right[o2] : -1.0f;
    const bool s1 = 0.0f <= xr1, s2 = 0.0f <= xr2;
    const double* b1 = A.bearings + 3 * o1;
    const double* b2 = A.bearings + 3 * o2;
    const double c1v[3] = {b1[0], b1[1], b1[2]}, c2v[3] = {b2[0], b2[1], b2[2]};
    double w1[3], w2[3];
    turn_to_world(P1, c1v, w1);
    turn_to_world(P2, c2v, w2);
    const double cr = (w1[0] * w2[0] + w1[1] * w2[1]) + w1[2] * w2[2];
    float d1 = 0.0f, d2 = 0.0f;
    double cs1 = 2.0, cs2 = 2.0;
    if (s1) { d1 = A.depths[o1]; cs1 = cos(2.0 * atan2(A.half_baseline, (double)d1)); }
    if (s2) { d2 = A.depths[o2]; cs2 = cos(2.0 * atan2(A.half_baseline, (double)d2)); }
    const double cs = cs2 < cs1 ? cs2 : cs1;   // std::min
    const bool two = ((!s1 && !s2) && 0.0 < cr && cr < (double)A.cos_thr) || ((s1 || s2) && 0.0 < cr && cr < cs);
    if (two) {
        // solve::triangulator::triangulate: rows of A from the bearings and cam_pose_cw = (rot_cw | trans_cw)
        double M[16], v[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const double a0 = c < 3 ? P1[c] : P1[9], a1 = c < 3 ? P1[3 + c] : P1[10], a2 = c < 3 ? P1[6 + c] : P1[11];
            const double e0 = c < 3 ? P2[c] : P2[9], e1 = c < 3 ? P2[3 + c] : P2[10], e2 = c < 3 ? P2[6 + c] : P2[11];
            M[c] = c1v[0] * a2 - c1v[2] * a0;
            M[4 + c] = c1v[1] * a2 - c1v[2] * a1;
            M[8 + c] = c2v[0] * e2 - c2v[2] * e0;
            M[12 + c] = c2v[1] * e2 - c2v[2] * e1;
        }
        int sweeps;
        null_vector4(M, v, &sweeps);
        if (v[3] == 0.0) return kNonFinite;
        pos[0] = v[0] / v[3]; pos[1] = v[1] / v[3]; pos[2] = v[2] / v[3];
    } else if (s1 && cs1 < cs2) {
        triangulate_stereo(A, P1, k1, d1, pos);
    } else if (s2 && cs2 < cs1) {
        triangulate_stereo(A, P2, k2, d2, pos);
    } else {
        return kNoParallax;
    }
    if (!isfinite(pos[0]) || !isfinite(pos[1]) || !isfinite(pos[2])) return kNonFinite;
    if constexpr (MODEL != PLP_CAMERA_EQUIRECTANGULAR) {   // check_depth_is_positive (.h:114-118)
        if (!(0 < ((P1[6] * pos[0] + P1[7] * pos[1]) + P1[8] * pos[2]) + P1[11])) return kDepth;
        if (!(0 < ((P2[6] * pos[0] + P2[7] * pos[1]) + P2[8] * pos[2]) + P2[11])) return kDepth;
    }
    const int oc1 = min(max(k1.octave, 0), A.num_levels - 1), oc2 = min(max(k2.octave, 0), A.num_levels - 1);
    const int e1 = reprojection_check<MODEL>(A, P1, pos, k1, xr1, A.level_sigma_sq[oc1], s1);
    if (e1) return e1 == 2 ? kNonFinite : kReproj1;
    const int e2 = reprojection_check<MODEL>(A, P2, pos, k2, xr2, A.level_sigma_sq[oc2], s2);
    if (e2) return e2 == 2 ? kNonFinite : kReproj2;
    // check_scale_factors (.h:120-137)
    const double l1 = norm3(pos[0] - P1[12], pos[1] - P1[13], pos[2] - P1[14]);
    const double l2 = norm3(pos[0] - P2[12], pos[1] - P2[13], pos[2] - P2[14]);
    if (l1 == 0 || l2 == 0) return kScale;
    const double ratio_dists = l2 / l1;
    const float ratio_octave = A.scale_factors[oc1] / A.scale_factors[oc2];
    if (!((double)ratio_octave / ratio_dists < (double)A.ratio_factor && ratio_dists / (double)ratio_octave < (double)A.ratio_factor)) return kScale;
    return kCreated;
}

template <int MODEL>
__global__ __launch_bounds__(256) void k_triangulate_keypoint_pairs(KeypointPairArgs A) {
    __shared__ uint32_t s_work[256];                // the workgroup's matched slots, packed to the front: slot in the workgroup | idx_1 << 8
    __shared__ int s_wave[4];
    const int p = A.p0 + blockIdx.y, tid = threadIdx.x, t0 = blockIdx.x * 256, t = t0 + tid;
    // uniform over the workgroup: the pair, its two key frames, the neighbour's count, the skip flag
    const int f1 = A.pairs[2 * p], f2 = A.pairs[2 * p + 1];
    if ((unsigned)f1 >= (unsigned)A.F || (unsigned)f2 >= (unsigned)A.F) return;   // outside the table: nothing read, nothing written
    const int n2 = clamp_count(A.counts, f2, A.cap);
    if (t0 >= n2) return;
    const size_t row = (size_t)p * A.cap;
    if (A.pair_skip && A.pair_skip[p]) {            // the `continue` of create_new_landmarks: one status, nothing else
        if (t < n2) A.out_status[row + t] = kPairSkipped;
        return;
    }
    // every slot without a triangulation is finished here
    bool work = false;
    int j = -1;
    if (t < n2) {
        const int q = A.match_q[row + t];
        uint8_t st = kNoMatch;
        if (q >= 0 && q < A.m_cap) {
            j = A.q_feature ? A.q_feature[(size_t)p * A.m_cap + q] : q;
            st = kIndexRange;                       // undist_keypts_.at(idx_1) throws
            work = j >= 0 && j < clamp_count(A.counts, f1, A.cap);
        }
        if (!work) {
            A.out_status[row + t] = st;
            A.out_idx_1[row + t] = j;
            double* out = A.out_pos_w + 3 * (row + t);
            out[0] = 0.0; out[1] = 0.0; out[2] = 0.0;
        }
    }
    // Matches are a fraction of the key points and a triangulation is a few thousand f64 operations: the matched slots are packed into the
    // workgroup's first lanes, so that whole waves leave instead of idling beside a few busy lanes (profiles/r10_keypoint_pairs.md).
    const unsigned long long m = __ballot(work);
    const int lane = tid & 63, w = tid >> 6;
    if (lane == 0) s_wave[w] = (int)__popcll(m);
    wg_barrier();
    int before = 0, total = 0;
#pragma unroll
    for (int v = 0; v < 4; ++v) {
        if (v < w) before += s_wave[v];
        total += s_wave[v];
    }
    if (work) s_work[before + (int)__popcll(m & ((1ull << lane) - 1ull))] = (uint32_t)tid | ((uint32_t)j << 8);
    wg_barrier();
    if (tid >= total) return;
    const uint32_t e = s_work[tid];
    const int tt = t0 + (int)(e & 255u), jj = (int)(e >> 8);
    double pos[3] = {0.0, 0.0, 0.0};
    const uint8_t st = triangulate_keypoints<MODEL>(A, f1, f2, jj, tt, pos);
    const bool made = st == kCreated;
    const size_t o = row + tt;
    A.out_status[o] = st;
    A.out_idx_1[o] = jj;
    double* out = A.out_pos_w + 3 * o;
    out[0] = made ? pos[0] : 0.0;
    out[1] = made ? pos[1] : 0.0;
    out[2] = made ? pos[2] : 0.0;
    if (made) {                                     // keyframe::add_landmark on both key frames (mapping_module.cc:464-465)
        if (A.occ1) A.occ1[row + jj] = 1;
        if (A.occ2) A.occ2[o] = 1;
    }
}

}  // namespace

hipError_t launch_pair_geometry(hipStream_t st, const PairGeometryArgs& A) {
    hipLaunchKernelGGL(k_keyframe_pair_geometry, dim3((A.P + 255) / 256), dim3(256), 0, st, A);
    return hipGetLastError();
}

hipError_t launch_keypoint_pairs(hipStream_t st, const KeypointPairArgs& A0) {
    KeypointPairArgs A = A0;
    for (int p0 = 0; p0 < A0.P; p0 += 65535) {      // the pair index runs along y
        A.p0 = p0;
        const dim3 grid((A.cap + 255) / 256, min(A0.P - p0, 65535));
        if (A.model == PLP_CAMERA_PERSPECTIVE) hipLaunchKernelGGL(k_triangulate_keypoint_pairs<PLP_CAMERA_PERSPECTIVE>, grid, dim3(256), 0, st, A);
        else if (A.model == PLP_CAMERA_FISHEYE) hipLaunchKernelGGL(k_triangulate_keypoint_pairs<PLP_CAMERA_FISHEYE>, grid, dim3(256), 0, st, A);
        else hipLaunchKernelGGL(k_triangulate_keypoint_pairs<PLP_CAMERA_EQUIRECTANGULAR>, grid, dim3(256), 0, st, A);
        if (hipError_t e = hipGetLastError()) return e;
    }
    return hipSuccess;
}

}  // namespace plp
