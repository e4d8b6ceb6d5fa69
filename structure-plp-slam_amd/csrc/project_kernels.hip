// Fuse, Sim3 and relocalisation queries (plp_project_landmarks_* / plp_project_landmark_lines_*): what seven matcher loops of the reference
// do per landmark in front of their search --
//   fuse::replace_duplication (match/fuse.cc:169-236), replace_duplication_line (:335-420), detect_duplication (:40-111),
//   projection::match_by_Sim3_transform (match/projection.cc:781-848), match_keyframes_mutually (:894-993, :1029-1087),
//   match_frame_and_keyframe (:529-593), match_frame_and_keyframe_line (:648-743)
// -- transform, reproject, image test, distance range, viewing angle, predict_scale_level, with reproject<MODEL>, predict_level, norm3 and
// carry_chunk of reproject.hpp.  Numeric contract: DESIGN.md section 5, D9 (f64 in the reference's order, the file is compiled with
// -ffp-contract=off).  Two expressions differ from frame::can_observe (observe_kernels.hip) and are written out here, not shared:
//   the distance range is an f64 comparison of the f64 distance with the float bounds widened: dist < min || max < dist
//   the viewing angle is dot < 0.5 * dist, without a division
// Points: one lane per slot, grid = (ceil(m_cap / 256), B), no LDS.  Lines: one workgroup of four waves per problem walks its slots in chunks
// of 256; reproj_sp / reproj_ep and their x_right of a slot whose end point is behind the camera are the carried ones of D6 (carry_chunk).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "match_device.hpp"
#include "plp_barrier.hpp"
#include "plp_common.hpp"
#include "reproject.hpp"

namespace plp {
namespace {

template <int MODEL>
__global__ __launch_bounds__(256) void k_project_points(ProjectArgs A) {
    const int b = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    const int n = A.counts ? min(max(A.counts[b], 0), A.m_cap) : A.m_cap;
    bool ok = false;
    if (i < n) {
        const size_t o = (size_t)b * A.m_cap + i;
        const size_t l = A.shared ? (size_t)i : o;   // the landmark's row: shared tables have m_cap rows in all
        int st = PLP_PROJECT_SKIPPED;
        if (!(A.skip && A.skip[o])) {
            const double* P = A.pose + (size_t)15 * b;
            const double x = A.pos_w[3 * l], y = A.pos_w[3 * l + 1], z = A.pos_w[3 * l + 2];
            const Reproj r = reproject<MODEL>(A, P, x, y, z);
            st = PLP_PROJECT_NOT_IN_IMAGE;
            if (r.in) {
                double dx, dy, dz;
                if (A.dist_mode == PLP_PROJECT_DIST_CAMERA) {   // pos_2 = s_rot_21w * pos_w + trans_21w (projection.cc:962, 1056)
                    dx = ((P[0] * x + P[1] * y) + P[2] * z) + P[9];
                    dy = ((P[3] * x + P[4] * y) + P[5] * z) + P[10];
                    dz = ((P[6] * x + P[7] * y) + P[8] * z) + P[11];
                } else {                                        // cam_to_lm_vec = pos_w - cam_center
                    dx = x - P[12]; dy = y - P[13]; dz = z - P[14];
                }
                const double dist = norm3(dx, dy, dz);
                const float max_d = (float)(1.3 * (double)A.max_dist[l]);    // get_max_valid_distance (landmark.cc:303-307)
                const float min_d = (float)(0.7 * (double)A.min_dist[l]);    // get_min_valid_distance (:297-301)
                st = PLP_PROJECT_DISTANCE;
                if (!(dist < (double)min_d || (double)max_d < dist)) {       // the reference's own f64 comparison (fuse.cc:89)
                    bool away = false;
                    if (A.ray_test) {
                        const double* nm = A.normal + 3 * l;
                        away = ((dx * nm[0] + dy * nm[1]) + dz * nm[2]) < 0.5 * dist;   // fuse.cc:98
                    }
                    st = PLP_PROJECT_RAY;
                    if (!away) {
                        st = PLP_PROJECT_KEPT;
                        ok = true;
                        if (A.reproj_d) { A.reproj_d[2 * o] = r.u; A.reproj_d[2 * o + 1] = r.v; }
                        if (A.reproj) { A.reproj[2 * o] = (float)r.u; A.reproj[2 * o + 1] = (float)r.v; }
                        if (A.x_right) A.x_right[o] = (float)r.xr;
                        if (A.level) A.level[o] = predict_level(A.max_dist[l], (float)dist, A.log_sf, A.num_levels);
                    }
                }
            }
        }
        A.valid[o] = ok ? 1 : 0;
        if (A.status) A.status[o] = (uint8_t)st;
    }
    if (A.num_valid) {   // zeroed by the launcher
        const unsigned long long m = __ballot(ok);
        if ((threadIdx.x & 63) == 0 && m) atomicAdd(A.num_valid + b, (int)__popcll(m));
    }
}

// A kernel-argument pointer held in vector registers.  The empty asm statement hides where the value comes from, and with it the address
// space the compiler infers for argument pointers; the global address space is therefore part of the type (no FLAT access).
template <class T> using global_ptr = __attribute__((address_space(1))) T*;
template <class T>
__device__ __forceinline__ global_ptr<T> in_vector_regs(T* p) {
    global_ptr<T> g = (global_ptr<T>)p;
    asm volatile("" : "+v"(g));
    return g;
}

template <int MODEL>
__global__ __launch_bounds__(256) void k_project_lines(ProjectArgs A) {
    const int b = blockIdx.x, t = threadIdx.x;
    const int n = A.counts ? min(max(A.counts[b], 0), A.m_cap) : A.m_cap;
    // Scalar registers: the f64 coefficients of the equirectangular model's asin / atan2 stay in scalar pairs across the chunk loop, beside a
    // uniform pose row (30 registers) and 17 argument pointers, and that instantiation then spills 25 of them.  The pose row is therefore read
    // through a per-lane address (its doubles live in vector registers) and the table and output pointers are held in vector registers as well.
    double P[15];
    {
        const auto row = in_vector_regs(A.pose + (size_t)15 * b);
#pragma unroll
        for (int k = 0; k < 15; ++k) P[k] = row[k];
    }
    const auto i_pos_w = in_vector_regs(A.pos_w);
    const auto i_min_dist = in_vector_regs(A.min_dist), i_max_dist = in_vector_regs(A.max_dist);
    const auto o_reproj_d = in_vector_regs(A.reproj_d), o_reproj2_d = in_vector_regs(A.reproj2_d);
    const auto o_reproj = in_vector_regs(A.reproj), o_reproj2 = in_vector_regs(A.reproj2);
    const auto o_x_right = in_vector_regs(A.x_right), o_x_right2 = in_vector_regs(A.x_right2);
    const auto o_level = in_vector_regs(A.level);
    const auto o_valid = in_vector_regs(A.valid), o_status = in_vector_regs(A.status);
    double cs[3] = {0.0, 0.0, 0.0}, ce[3] = {0.0, 0.0, 0.0};   // (u, v, x_right) before the first write (D6)
    int total = 0;
    for (int base = 0; base < n; base += 256) {   // uniform over the workgroup
        const int i = base + t;
        const size_t o = (size_t)b * A.m_cap + i;
        const size_t l = A.shared ? (size_t)i : o;
        bool ws = false, we = false, ok = false;
        double s[3] = {0.0, 0.0, 0.0}, e[3] = {0.0, 0.0, 0.0};
        int level = 0, st = PLP_PROJECT_SKIPPED;
        if (i < n && !(A.skip && A.skip[o])) {
            const auto p = i_pos_w + 6 * l;
            const double x0 = p[0], y0 = p[1], z0 = p[2], x1 = p[3], y1 = p[4], z1 = p[5];
            const Reproj rs = reproject<MODEL>(A, P, x0, y0, z0);
            const Reproj re = reproject<MODEL>(A, P, x1, y1, z1);
            ws = rs.wrote; we = re.wrote;
            s[0] = rs.u; s[1] = rs.v; s[2] = rs.xr;
            e[0] = re.u; e[1] = re.v; e[2] = re.xr;
            const double mx = 0.5 * (x0 + x1), my = 0.5 * (y0 + y1), mz = 0.5 * (z0 + z1);   // 0.5 * (pos_w_sp + pos_w_ep)
            st = PLP_PROJECT_NOT_IN_IMAGE;
            bool in = rs.in || re.in;
            if (in && !(rs.in && re.in)) {   // partial occlusion: the midpoint decides
                in = reproject<MODEL>(A, P, mx, my, mz).in;
                st = PLP_PROJECT_MIDPOINT_OUT;
            }
            if (in) {
                const double max_d = (double)(float)(1.2 * (double)i_max_dist[l]);   // Line::get_max_valid_distance (landmark_line.cc:360-364)
                const double min_d = (double)(float)(0.8 * (double)i_min_dist[l]);   // Line::get_min_valid_distance (:354-358)
                const double dist_mp = norm3(mx - P[12], my - P[13], mz - P[14]);
                bool out;
                if (A.line_dist_mode == PLP_PROJECT_LINE_ENDPOINTS) {   // fuse.cc:398-411: both end points; the level from the midpoint
                    const double dist_sp = norm3(x0 - P[12], y0 - P[13], z0 - P[14]);
                    const double dist_ep = norm3(x1 - P[12], y1 - P[13], z1 - P[14]);
                    out = dist_sp < min_d || max_d < dist_sp || dist_ep < min_d || max_d < dist_ep;
                } else {                                                // projection.cc:722-730
                    out = dist_mp < min_d || max_d < dist_mp;
                }
                st = PLP_PROJECT_DISTANCE;
                if (!out) {
                    st = PLP_PROJECT_KEPT;
                    ok = true;
                    level = predict_level(i_max_dist[l], (float)dist_mp, A.log_sf, A.num_levels);
                }
            }
        }
        total += carry_chunk<3>(ws, we, ok, s, e, cs, ce);
        if (i < n) {
            if (o_reproj_d) {
                o_reproj_d[2 * o] = s[0]; o_reproj_d[2 * o + 1] = s[1];
                o_reproj2_d[2 * o] = e[0]; o_reproj2_d[2 * o + 1] = e[1];
            }
            if (o_reproj) {
                o_reproj[2 * o] = (float)s[0]; o_reproj[2 * o + 1] = (float)s[1];
                o_reproj2[2 * o] = (float)e[0]; o_reproj2[2 * o + 1] = (float)e[1];
            }
            if (o_x_right) o_x_right[o] = (float)s[2];
            if (o_x_right2) o_x_right2[o] = (float)e[2];
            o_valid[o] = ok ? 1 : 0;
            if (o_status) o_status[o] = (uint8_t)st;
            if (ok && o_level) o_level[o] = level;
        }
    }
    if (t == 0 && A.num_valid) A.num_valid[b] = total;
}

}  // namespace

hipError_t launch_project_points(hipStream_t st, const ProjectArgs& A, int B) {
    if (A.num_valid) {   // the kernel adds each wave's count to it
        const hipError_t e = hipMemsetAsync(A.num_valid, 0, (size_t)B * sizeof(int32_t), st);
        if (e != hipSuccess) return e;
    }
    const dim3 grid((A.m_cap + 255) / 256, B);
    if (A.model == PLP_CAMERA_FISHEYE) hipLaunchKernelGGL(k_project_points<PLP_CAMERA_FISHEYE>, grid, dim3(256), 0, st, A);
    else if (A.model == PLP_CAMERA_EQUIRECTANGULAR) hipLaunchKernelGGL(k_project_points<PLP_CAMERA_EQUIRECTANGULAR>, grid, dim3(256), 0, st, A);
    else hipLaunchKernelGGL(k_project_points<PLP_CAMERA_PERSPECTIVE>, grid, dim3(256), 0, st, A);
    return hipGetLastError();
}

hipError_t launch_project_lines(hipStream_t st, const ProjectArgs& A, int B) {
    if (A.model == PLP_CAMERA_FISHEYE) hipLaunchKernelGGL(k_project_lines<PLP_CAMERA_FISHEYE>, dim3(B), dim3(256), 0, st, A);
    else if (A.model == PLP_CAMERA_EQUIRECTANGULAR) hipLaunchKernelGGL(k_project_lines<PLP_CAMERA_EQUIRECTANGULAR>, dim3(B), dim3(256), 0, st, A);
    else hipLaunchKernelGGL(k_project_lines<PLP_CAMERA_PERSPECTIVE>, dim3(B), dim3(256), 0, st, A);
    return hipGetLastError();
}

}  // namespace plp
