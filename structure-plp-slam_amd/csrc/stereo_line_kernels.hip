// Stereo key-line association and 3-D key lines (plp_stereo_keylines_* / plp_keylines_3d_*, include/plp_front.h).
//
// Association: the filter the stereo frame constructors run on BinaryDescriptorMatcher::match's left -> right result (data/frame.cc:389-427,
// again at :494-533): distance < 30, both end points within 200 px of the partner's, |abs(angle1) - abs(angle2)| * 180 / 3.14 < 5 degrees.
// One lane per left key line, grid = (ceil(cap_left / 256), B); the partner's record is gathered by its index.  No LDS, no barrier.
//
// 3-D key lines: frame::triangulate_stereo_for_line (data/frame.cc:953-1123; keyframe.cc:647-820 is the same code) for every key line of
// B frames: RGB-D unprojects both end points with their depth, stereo intersects the two back-projected planes (line3d.hpp).  One lane per
// key line in f64, grid = (ceil(cap / 256), B).  No LDS, no barrier.
// Numeric contract: DESIGN.md section 5, D7 (the file is compiled with -ffp-contract=off).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "line3d.hpp"
#include "match_device.hpp"

namespace plp {
namespace {

__device__ __forceinline__ int clamp_count(const int32_t* counts, int b, int cap) { return counts ? min(max(counts[b], 0), cap) : cap; }

// sqrt(p.dot(p)) of cv::Point2f: the float dot x*x + y*y (Point_::dot), its square root rounded to float (the f64 root of a float rounds to
// the same float as the correctly rounded f32 root)
__device__ __forceinline__ float point_distance(float x, float y) { return (float)sqrt((double)(x * x + y * y)); }

__global__ __launch_bounds__(256) void k_stereo_keylines(StereoKeylineArgs A) {
    const int b = blockIdx.y, j = blockIdx.x * 256 + threadIdx.x;
    if (j >= clamp_count(A.counts_l, b, A.cap_l)) return;
    const int nr = A.cap_r > 0 ? clamp_count(A.counts_r, b, A.cap_r) : 0;
    const size_t o = (size_t)b * A.cap_l + j;
    int good = -1;
    if (nr > 0) {   // an empty right side: the 1-NN has nothing, every slot -1
        const int t = A.train_idx[o];
        // DMatch.distance (float) < 30; the 1-NN's "nothing within 128" (-1, 256) and any index outside the right side are never kept
        if ((float)A.dist[o] < 30.f && t >= 0 && t < nr) {
            const plp_keyline& l1 = A.kl_l[o];
            const plp_keyline& l2 = A.kl_r[(size_t)b * A.cap_r + t];
            // getStartPoint() / getEndPoint() differences as cv::Point2f (float), their lengths compared with 200 strictly
            const float ds = point_distance(l1.startPointX - l2.startPointX, l1.startPointY - l2.startPointY);
            const float de = point_distance(l1.endPointX - l2.endPointX, l1.endPointY - l2.endPointY);
            // abs((abs(a1) - abs(a2))) * 180 / 3.14 with the float abs (D7): float product, divided in f64, rounded to float, compared with 5
            const float angle = (float)((double)(fabsf(fabsf(l1.angle) - fabsf(l2.angle)) * 180.f) / 3.14);
            if (ds < 200.f && de < 200.f && angle < 5.f) good = t;
        }
    }
    A.good[o] = good;
    const float v = good >= 0 ? 1.f : -1.f;   // (1.0, 1.0) marks a kept match, (-1, -1) the constructor's initial value
    A.depths[2 * o] = v; A.depths[2 * o + 1] = v;
    A.x_right[2 * o] = v; A.x_right[2 * o + 1] = v;
}

// rot_wc_ * p + cam_center_ with rot_wc_ = rot_cw_^T: row i of rot_wc_ is column i of the pose row's rot_cw (D5 item 1's order)
__device__ __forceinline__ void to_world(const double* P, const double (&p)[3], double (&w)[3]) {
#pragma unroll
    for (int i = 0; i < 3; ++i) w[i] = ((P[i] * p[0] + P[3 + i] * p[1]) + P[6 + i] * p[2]) + P[12 + i];
}

__global__ __launch_bounds__(256) void k_keylines_3d(Keylines3dArgs A) {
    const int b = blockIdx.y, j = blockIdx.x * 256 + threadIdx.x;
    if (j >= clamp_count(A.counts, b, A.cap)) return;
    const size_t o = (size_t)b * A.cap + j;
    const double* P = A.pose + (size_t)15 * b;
    const plp_keyline& kl = A.kl[o];
    double w_sp[3] = {0.0, 0.0, 0.0}, w_ep[3] = {0.0, 0.0, 0.0};
    bool ok = false;
    if (A.setup_type == 2) {   // RGB-D, frame.cc:960-991
        const float depth_sp = A.kl_depths[2 * o], depth_ep = A.kl_depths[2 * o + 1];
        if (0.0f < depth_sp && 0.0f < depth_ep) {
            // (x - cx_) * depth * fx_inv_ in f64 (float x and depth promoted), stored as float
            const float ux_sp = (float)((((double)kl.startPointX - A.cx) * (double)depth_sp) * A.fx_inv);
            const float uy_sp = (float)((((double)kl.startPointY - A.cy) * (double)depth_sp) * A.fy_inv);
            const float ux_ep = (float)((((double)kl.endPointX - A.cx) * (double)depth_ep) * A.fx_inv);
            const float uy_ep = (float)((((double)kl.endPointY - A.cy) * (double)depth_ep) * A.fy_inv);
            const double c_sp[3] = {(double)ux_sp, (double)uy_sp, (double)depth_sp}, c_ep[3] = {(double)ux_ep, (double)uy_ep, (double)depth_ep};
            to_world(P, c_sp, w_sp);
            to_world(P, c_ep, w_ep);
            ok = true;
        }
    } else {   // stereo, frame.cc:995-1118
        const int nr = A.cap_r > 0 ? clamp_count(A.counts_r, b, A.cap_r) : 0;
        const int t = A.good_match[o];
        if (t >= 0 && t < nr) {   // _good_matches_stereo.count(idx)
            const plp_keyline& kr = A.kl_r[(size_t)b * A.cap_r + t];
            // P1 = K [I | 0], P2 = K [I | -focal_x_baseline_ / fx e_x] as the reference writes them; transformation_line_cw = identity blocks;
            // _K = (fy, 0, 0; 0, fx, 0; -fy cx, -fx cy, fx fy)
            const double P1[12] = {A.fx, 0.0, A.cx, 0.0, 0.0, A.fy, A.cy, 0.0, 0.0, 0.0, 1.0, 0.0};
            const double P2[12] = {A.fx, 0.0, A.cx, -A.fxb, 0.0, A.fy, A.cy, 0.0, 0.0, 0.0, 1.0, 0.0};
            const double T[18] = {1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0};
            const double K[9] = {A.fy, 0.0, 0.0, 0.0, A.fx, 0.0, -A.fy * A.cx, -A.fx * A.cy, A.fx * A.fy};
            double c_sp[3], c_ep[3];
            ok = line3d_triangulate_pair(P1, P2, T, K, kl.startPointX, kl.startPointY, kl.endPointX, kl.endPointY, kr.startPointX, kr.startPointY,
                                         kr.endPointX, kr.endPointY, c_sp, c_ep);
            to_world(P, c_sp, w_sp);
            to_world(P, c_ep, w_ep);
            ok = ok && 0 < w_sp[2] && 0 < w_ep[2];   // the world z, as the reference checks it (:1109)
        }
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) ok = ok && isfinite(w_sp[i]) && isfinite(w_ep[i]);   // D7: a non-finite value gives Vec6_t::Zero()
    double* out = A.pos_w + 6 * o;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        out[i] = ok ? w_sp[i] : 0.0;
        out[3 + i] = ok ? w_ep[i] : 0.0;
    }
    if (A.valid) A.valid[o] = ok ? 1 : 0;
}

}  // namespace

hipError_t launch_stereo_keylines(hipStream_t st, const StereoKeylineArgs& A, int B) {
    hipLaunchKernelGGL(k_stereo_keylines, dim3((A.cap_l + 255) / 256, B), dim3(256), 0, st, A);
    return hipGetLastError();
}

hipError_t launch_keylines_3d(hipStream_t st, const Keylines3dArgs& A, int B) {
    hipLaunchKernelGGL(k_keylines_3d, dim3((A.cap + 255) / 256, B), dim3(256), 0, st, A);
    return hipGetLastError();
}

}  // namespace plp
