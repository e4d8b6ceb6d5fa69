// Local-landmark visibility (plp_observe_landmarks_* / plp_observe_landmark_lines_*): the loops of tracking_module::search_local_landmarks
// and search_local_landmarks_line (src/PLPSLAM/tracking_module.cc:908-1064) over local_landmarks_, i.e. data::frame::can_observe
// (data/frame.cc:797-824) and can_observe_line (:827-878) with camera::*::reproject_to_image of the three models.
// Numeric contract: DESIGN.md section 5, D5.  f64 in the reference's order (the file is compiled with -ffp-contract=off); the only
// non-IEEE operations are ocml's f64 asin / atan2 of the equirectangular model (D4) and its f64 log behind predict_scale_level's logf (D5).
//
// Points: one lane per landmark, grid = (ceil(m_cap / 256), B), no LDS.
// Lines: the reference's reproj_sp / reproj_ep temporaries are declared once before the loop and reproject_to_image leaves them alone for a
// point behind the camera, so an end point can carry the value of an EARLIER landmark (D5 item 5).  One workgroup of four waves per problem
// walks the landmarks in chunks of 256: the geometry of a chunk in parallel, then "the nearest writer at or below me" from a 64-bit ballot
// within the wave, the waves' last writers through LDS, and the value carried from the previous chunks (carry_chunk).
//
// Last-frame queries (plp_project_last_frame[_lines]_*): the loops of projection::match_current_and_last_frames (match/projection.cc:214-358)
// and match_current_and_last_frames_line (:361-527) in front of their searches, with the same reproject<MODEL> and the same layouts:
// points one lane per key point of the last frame, lines one workgroup per problem with the end points (and their x_right) carried by
// carry_chunk as D6 defines it, and the problem's assume_forward / assume_backward as one value per problem.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include "match_device.hpp"
#include "plp_barrier.hpp"
#include "plp_common.hpp"
#include "reproject.hpp"

namespace plp {
namespace {

// Reproj, reproject<MODEL>, predict_level, norm3 and carry_chunk: reproject.hpp (shared with project_kernels.hip)

template <int MODEL>
__global__ __launch_bounds__(256) void k_observe_points(ObserveArgs A) {
    const int b = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    const int n = A.counts ? min(max(A.counts[b], 0), A.m_cap) : A.m_cap;
    bool ok = false;
    if (i < n) {
        const size_t o = (size_t)b * A.m_cap + i;
        if (!(A.skip && A.skip[o])) {   // frame::can_observe (frame.cc:797-824)
            const double* P = A.pose + (size_t)15 * b;
            const double x = A.pos_w[3 * o], y = A.pos_w[3 * o + 1], z = A.pos_w[3 * o + 2];
            const Reproj r = reproject<MODEL>(A, P, x, y, z);
            ok = r.in;
            if (ok && A.normal) {
                const double dx = x - P[12], dy = y - P[13], dz = z - P[14];
                const double dist = norm3(dx, dy, dz);
                const float fd = (float)dist;                                // is_inside_in_orb_scale(const float)
                const float max_d = (float)(1.3 * (double)A.max_dist[o]);    // get_max_valid_distance (landmark.cc:303-307)
                const float min_d = (float)(0.7 * (double)A.min_dist[o]);    // get_min_valid_distance (:297-301)
                ok = min_d <= fd && fd <= max_d;
                if (ok) {
                    const double* nm = A.normal + 3 * o;
                    const double ray_cos = ((dx * nm[0] + dy * nm[1]) + dz * nm[2]) / dist;
                    ok = !(ray_cos < (double)A.ray_cos_thr);
                }
                if (ok) A.level[o] = predict_level(A.max_dist[o], fd, A.log_sf, A.num_levels);
            }
            if (ok) {
                A.reproj[2 * o] = (float)r.u; A.reproj[2 * o + 1] = (float)r.v;
                if (A.x_right) A.x_right[o] = (float)r.xr;
            }
        }
        A.valid[o] = ok ? 1 : 0;
    }
    if (A.num_valid) {   // zeroed by the launcher
        const unsigned long long m = __ballot(ok);
        if ((threadIdx.x & 63) == 0 && m) atomicAdd(A.num_valid + b, (int)__popcll(m));
    }
}

template <int MODEL>
__global__ __launch_bounds__(256) void k_observe_lines(ObserveArgs A) {
    const int b = blockIdx.x, t = threadIdx.x;
    const int n = A.counts ? min(max(A.counts[b], 0), A.m_cap) : A.m_cap;
    const double* P = A.pose + (size_t)15 * b;
    float cs[2] = {0.f, 0.f}, ce[2] = {0.f, 0.f};   // the temporaries before the first write: (0, 0) (D5 item 5)
    int total = 0;
    for (int base = 0; base < n; base += 256) {   // uniform over the workgroup
        const int i = base + t;
        const size_t o = (size_t)b * A.m_cap + i;
        bool ws = false, we = false, ok = false;
        float s[2] = {0.f, 0.f}, e[2] = {0.f, 0.f};
        int level = 0;
        if (i < n && !(A.skip && A.skip[o])) {   // frame::can_observe_line (frame.cc:827-878)
            const double* p = A.pos_w + 6 * o;
            const double x0 = p[0], y0 = p[1], z0 = p[2], x1 = p[3], y1 = p[4], z1 = p[5];
            const Reproj rs = reproject<MODEL>(A, P, x0, y0, z0);
            const Reproj re = reproject<MODEL>(A, P, x1, y1, z1);
            ws = rs.wrote; we = re.wrote;
            s[0] = (float)rs.u; s[1] = (float)rs.v; e[0] = (float)re.u; e[1] = (float)re.v;
            const double mx = 0.5 * (x0 + x1), my = 0.5 * (y0 + y1), mz = 0.5 * (z0 + z1);
            ok = rs.in || re.in;
            if (ok && !(rs.in && re.in)) ok = reproject<MODEL>(A, P, mx, my, mz).in;   // partial occlusion: the midpoint decides
            if (ok) {
                const float fd = (float)norm3(mx - P[12], my - P[13], mz - P[14]);     // is_inside_in_feature_scale(const float)
                const float max_d = (float)(1.2 * (double)A.max_dist[o]);           // Line::get_max_valid_distance (landmark_line.cc:360-364)
                const float min_d = (float)(0.8 * (double)A.min_dist[o]);           // Line::get_min_valid_distance (:354-358)
                ok = min_d <= fd && fd <= max_d;
                if (ok) level = predict_level(A.max_dist[o], fd, A.log_sf, A.num_levels);
            }
        }
        total += carry_chunk<2>(ws, we, ok, s, e, cs, ce);
        if (i < n) {
            A.reproj[2 * o] = s[0]; A.reproj[2 * o + 1] = s[1];
            A.reproj2[2 * o] = e[0]; A.reproj2[2 * o + 1] = e[1];
            A.valid[o] = ok ? 1 : 0;
            if (ok) A.level[o] = level;
        }
    }
    if (t == 0 && A.num_valid) A.num_valid[b] = total;
}

// assume_forward / assume_backward of projection.cc:219-236 (:366-383 for lines): trans_lc = rot_lw * trans_wc + trans_lw, where trans_wc =
// -rot_cw^T trans_cw is the current frame's cam_center_ (the pose row's 12-14, formed in frame::update_pose_params' order); only its z is read.
// 0 neither, 1 forward, 2 backward; a monocular setup is always 0.
__device__ __forceinline__ void write_direction(const ObserveArgs& A, int b) {
    const double* P = A.pose + (size_t)15 * b;
    const double* L = A.pose_last + (size_t)15 * b;
    const double z = ((L[6] * P[12] + L[7] * P[13]) + L[8] * P[14]) + L[11];
    int d = 0;
    if (A.setup_type != 0) d = (z > A.true_baseline) ? 1 : (-z > A.true_baseline) ? 2 : 0;
    A.direction[b] = d;
}

// projection::match_current_and_last_frames up to its search: a slot is valid when it is not skipped (!lm || outlier) and its landmark
// reprojects into the current image; valid slots get the reprojection, x_right, the last frame's key point octave and angle.
template <int MODEL>
__global__ __launch_bounds__(256) void k_last_frame_points(ObserveArgs A) {
    const int b = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    if (i == 0) write_direction(A, b);
    const int n = A.counts ? min(max(A.counts[b], 0), A.m_cap) : A.m_cap;
    bool ok = false;
    if (i < n) {
        const size_t o = (size_t)b * A.m_cap + i;
        if (!(A.skip && A.skip[o])) {
            const double* P = A.pose + (size_t)15 * b;
            const Reproj r = reproject<MODEL>(A, P, A.pos_w[3 * o], A.pos_w[3 * o + 1], A.pos_w[3 * o + 2]);
            ok = r.in;
            if (ok) {
                A.reproj[2 * o] = (float)r.u; A.reproj[2 * o + 1] = (float)r.v;
                if (A.x_right) A.x_right[o] = (float)r.xr;
                A.level[o] = A.kps[o].octave;                  // last_frm.keypts_.at(idx_last).octave (= undist_keypts_' octave)
                if (A.angle) A.angle[o] = A.kps[o].angle;     // last_frm.undist_keypts_.at(idx_last).angle
            }
        }
        A.valid[o] = ok ? 1 : 0;
    }
    if (A.num_valid) {   // zeroed by the launcher
        const unsigned long long m = __ballot(ok);
        if ((threadIdx.x & 63) == 0 && m) atomicAdd(A.num_valid + b, (int)__popcll(m));
    }
}

// projection::match_current_and_last_frames_line up to its search: both end points reprojected, the line kept when one is in the image
// and, if the other is not, the midpoint is (:415-440); the level is the last frame's key line octave.  reproj_sp / reproj_ep and
// x_right_sp / x_right_ep are declared INSIDE the reference's loop, so an end point behind the camera of a kept line reads uninitialised
// values; D6 defines them as carried from the most recent earlier non-skipped slot whose matching end point was written, (0, 0) / 0 before.
template <int MODEL>
__global__ __launch_bounds__(256) void k_last_frame_lines(ObserveArgs A) {
    const int b = blockIdx.x, t = threadIdx.x;
    if (t == 0) write_direction(A, b);
    const int n = A.counts ? min(max(A.counts[b], 0), A.m_cap) : A.m_cap;
    const double* P = A.pose + (size_t)15 * b;
    float cs[3] = {0.f, 0.f, 0.f}, ce[3] = {0.f, 0.f, 0.f};   // (u, v, x_right) before the first write (D6)
    int total = 0;
    for (int base = 0; base < n; base += 256) {   // uniform over the workgroup
        const int i = base + t;
        const size_t o = (size_t)b * A.m_cap + i;
        bool ws = false, we = false, ok = false;
        float s[3] = {0.f, 0.f, 0.f}, e[3] = {0.f, 0.f, 0.f};
        if (i < n && !(A.skip && A.skip[o])) {
            const double* p = A.pos_w + 6 * o;
            const double x0 = p[0], y0 = p[1], z0 = p[2], x1 = p[3], y1 = p[4], z1 = p[5];
            const Reproj rs = reproject<MODEL>(A, P, x0, y0, z0);
            const Reproj re = reproject<MODEL>(A, P, x1, y1, z1);
            ws = rs.wrote; we = re.wrote;
            s[0] = (float)rs.u; s[1] = (float)rs.v; s[2] = (float)rs.xr;
            e[0] = (float)re.u; e[1] = (float)re.v; e[2] = (float)re.xr;
            ok = rs.in || re.in;
            if (ok && !(rs.in && re.in)) ok = reproject<MODEL>(A, P, 0.5 * (x0 + x1), 0.5 * (y0 + y1), 0.5 * (z0 + z1)).in;
        }
        total += carry_chunk<3>(ws, we, ok, s, e, cs, ce);
        if (i < n) {
            A.reproj[2 * o] = s[0]; A.reproj[2 * o + 1] = s[1];
            A.reproj2[2 * o] = e[0]; A.reproj2[2 * o + 1] = e[1];
            if (A.x_right) A.x_right[o] = s[2];
            if (A.x_right2) A.x_right2[o] = e[2];
            A.valid[o] = ok ? 1 : 0;
            if (ok) A.level[o] = A.kl[o].octave;   // last_frm._keylsd.at(idx_last).octave
        }
    }
    if (t == 0 && A.num_valid) A.num_valid[b] = total;
}

}  // namespace

hipError_t launch_observe_points(hipStream_t st, const ObserveArgs& A, int B) {
    if (A.num_valid) {   // the kernel adds each wave's count to it
        const hipError_t e = hipMemsetAsync(A.num_valid, 0, (size_t)B * sizeof(int32_t), st);
        if (e != hipSuccess) return e;
    }
    const dim3 grid((A.m_cap + 255) / 256, B);
    if (A.model == PLP_CAMERA_FISHEYE) hipLaunchKernelGGL(k_observe_points<PLP_CAMERA_FISHEYE>, grid, dim3(256), 0, st, A);
    else if (A.model == PLP_CAMERA_EQUIRECTANGULAR) hipLaunchKernelGGL(k_observe_points<PLP_CAMERA_EQUIRECTANGULAR>, grid, dim3(256), 0, st, A);
    else hipLaunchKernelGGL(k_observe_points<PLP_CAMERA_PERSPECTIVE>, grid, dim3(256), 0, st, A);
    return hipGetLastError();
}

hipError_t launch_observe_lines(hipStream_t st, const ObserveArgs& A, int B) {
    if (A.model == PLP_CAMERA_FISHEYE) hipLaunchKernelGGL(k_observe_lines<PLP_CAMERA_FISHEYE>, dim3(B), dim3(256), 0, st, A);
    else if (A.model == PLP_CAMERA_EQUIRECTANGULAR) hipLaunchKernelGGL(k_observe_lines<PLP_CAMERA_EQUIRECTANGULAR>, dim3(B), dim3(256), 0, st, A);
    else hipLaunchKernelGGL(k_observe_lines<PLP_CAMERA_PERSPECTIVE>, dim3(B), dim3(256), 0, st, A);
    return hipGetLastError();
}

hipError_t launch_last_frame_points(hipStream_t st, const ObserveArgs& A, int B) {
    if (A.num_valid) {
        const hipError_t e = hipMemsetAsync(A.num_valid, 0, (size_t)B * sizeof(int32_t), st);
        if (e != hipSuccess) return e;
    }
    const dim3 grid(A.m_cap > 0 ? (A.m_cap + 255) / 256 : 1, B);   // m_cap == 0: one workgroup per problem still writes its direction
    if (A.model == PLP_CAMERA_FISHEYE) hipLaunchKernelGGL(k_last_frame_points<PLP_CAMERA_FISHEYE>, grid, dim3(256), 0, st, A);
    else if (A.model == PLP_CAMERA_EQUIRECTANGULAR) hipLaunchKernelGGL(k_last_frame_points<PLP_CAMERA_EQUIRECTANGULAR>, grid, dim3(256), 0, st, A);
    else hipLaunchKernelGGL(k_last_frame_points<PLP_CAMERA_PERSPECTIVE>, grid, dim3(256), 0, st, A);
    return hipGetLastError();
}

hipError_t launch_last_frame_lines(hipStream_t st, const ObserveArgs& A, int B) {
    if (A.model == PLP_CAMERA_FISHEYE) hipLaunchKernelGGL(k_last_frame_lines<PLP_CAMERA_FISHEYE>, dim3(B), dim3(256), 0, st, A);
    else if (A.model == PLP_CAMERA_EQUIRECTANGULAR) hipLaunchKernelGGL(k_last_frame_lines<PLP_CAMERA_EQUIRECTANGULAR>, dim3(B), dim3(256), 0, st, A);
    else hipLaunchKernelGGL(k_last_frame_lines<PLP_CAMERA_PERSPECTIVE>, dim3(B), dim3(256), 0, st, A);
    return hipGetLastError();
}

}  // namespace plp
