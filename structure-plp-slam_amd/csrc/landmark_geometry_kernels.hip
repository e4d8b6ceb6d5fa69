// Landmark normals and valid distance ranges (plp_landmark_geometry_* / plp_landmark_line_geometry_*, include/plp_front.h): what
// landmark::update_normal_and_depth (data/landmark.cc:249-295) and Line::update_information (data/landmark_line.cc:311-352) write, for L
// landmarks with ragged observation lists.  Numeric contract: DESIGN.md section 5, D11 (the file is compiled with -ffp-contract=off); the
// arithmetic and the statuses are those of landmark_geometry.hpp, which the host model runs too.
//
// k_landmark_geometry_points: a workgroup owns a run of kLgRun landmarks, whose observations are one contiguous range of the lists, and
// walks that range in tiles of kLgTile observations.  Per tile every lane takes one observation -- obs_kf is read coalesced, the owning
// landmark is found by a binary search in the LDS copy of the run's offsets, the centre is gathered from the pose row, the unit vector (one
// f64 sqrt, three f64 divisions) goes to LDS -- and then the lane that owns a landmark adds the landmark's terms of the tile in list order to
// the sum it carries in registers.  A list that crosses a tile edge, or that is longer than a tile, is carried from tile to tile: the order
// of the sum is the list's for every length.  The run is short (32 landmarks for 256 lanes) because the kernel is a chain of latencies, not
// of bytes: a local-BA window of 8 000 landmarks has to become enough workgroups to fill the chip, and a tile of typical lists (2-15
// observations) is filled by 32 of them.  The ordered sum is unrolled by four so that its LDS reads are issued ahead of the additions, which
// stay in program order.  One lane per landmark, a longer run and a copy of the centres in LDS were measured against this:
// profiles/r11_landmark_geometry.md.
//
// k_landmark_geometry_lines: no reduction, one lane per landmark.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "landmark_geometry.hpp"
#include "plp_barrier.hpp"

namespace plp {
namespace {

constexpr int kLgTile = 256;          // observations of a tile = the lanes of a workgroup
constexpr int kLgRun = 32;            // landmarks of a workgroup, a power of two <= kLgTile: its first kLgRun lanes own one each

__global__ __launch_bounds__(256) void k_landmark_geometry_points(LandmarkGeometryArgs A) {
    __shared__ int s_off[kLgRun + 1];
    __shared__ double s_px[kLgRun], s_py[kLgRun], s_pz[kLgRun];
    __shared__ double s_ux[kLgTile], s_uy[kLgTile], s_uz[kLgTile];
    __shared__ int s_kf[kLgTile];
    const int tid = threadIdx.x, l0 = blockIdx.x * kLgRun, n = min(kLgRun, A.L - l0), l = l0 + tid;
    // the run's offsets; the slots behind a short last run repeat its end, so that the search below stays inside the run
    if (tid < kLgRun) s_off[tid] = A.obs_offsets[l0 + min(tid, n)];
    if (tid == 0) s_off[kLgRun] = A.obs_offsets[l0 + n];
    if (tid < n) {
        const double* p = A.pos_w + (size_t)3 * l;
        s_px[tid] = p[0]; s_py[tid] = p[1]; s_pz[tid] = p[2];
    }
    wg_barrier();
    const int o_begin = s_off[0], o_end = s_off[kLgRun];
    const bool owner = tid < kLgRun;
    const int beg = owner ? s_off[tid] : 0, end = owner ? s_off[tid + 1] : 0;
    const int ref = tid < n ? A.ref_kf[l] : -1;
    double sx = 0.0, sy = 0.0, sz = 0.0;   // Vec3_t::Zero() (:272)
    int found = -1;
    bool bad = false;
    for (int base = o_begin; base < o_end; base += kLgTile) {   // uniform over the workgroup
        const int o = base + tid;
        if (o < o_end) {
            const int kf = A.obs_kf[o];
            int lo = 0, hi = kLgRun;           // s_off[lo] <= o < s_off[hi]: the owner is the last landmark whose list starts at or before o
#pragma unroll
            for (int span = kLgRun; span > 1; span >>= 1) {
                const int mid = (lo + hi) >> 1;
                if (s_off[mid] <= o) lo = mid; else hi = mid;
            }
            LgVec3 u = {0.0, 0.0, 0.0};
            if ((unsigned)kf < (unsigned)A.F) {   // a key frame outside the table is not followed: the owner sees it in s_kf
                const double* c = A.pose + (size_t)15 * kf + 12;
                u = lg_normalized(s_px[lo] - c[0], s_py[lo] - c[1], s_pz[lo] - c[2]);   // (pos_w_ - cam_center).normalized() (:278-279)
            }
            s_ux[tid] = u.x; s_uy[tid] = u.y; s_uz[tid] = u.z;
            s_kf[tid] = kf;
        }
        wg_barrier();
        const int a = max(beg, base), b = min(end, min(base + kLgTile, o_end));
#pragma unroll 4
        for (int o2 = a; o2 < b; ++o2) {    // mean_normal = mean_normal + normal.normalized(), in list order (:279)
            const int i = o2 - base;
            sx = sx + s_ux[i]; sy = sy + s_uy[i]; sz = sz + s_uz[i];
            const int kf = s_kf[i];
            if ((unsigned)kf >= (unsigned)A.F) bad = true;
            else if (found < 0 && kf == ref) found = o2;
        }
        wg_barrier();
    }
    if (tid < n) A.status[l] = lg_point_finish(A, l, end - beg, sx, sy, sz, found, bad);
}

__global__ __launch_bounds__(256) void k_landmark_geometry_lines(LandmarkGeometryArgs A) {
    const int l = blockIdx.x * 256 + threadIdx.x;
    if (l < A.L) A.status[l] = lg_line(A, l);
}

}  // namespace

hipError_t launch_landmark_geometry_points(hipStream_t st, const LandmarkGeometryArgs& A) {
    hipLaunchKernelGGL(k_landmark_geometry_points, dim3((A.L + kLgRun - 1) / kLgRun), dim3(256), 0, st, A);
    return hipGetLastError();
}

hipError_t launch_landmark_geometry_lines(hipStream_t st, const LandmarkGeometryArgs& A) {
    hipLaunchKernelGGL(k_landmark_geometry_lines, dim3((A.L + 255) / 256), dim3(256), 0, st, A);
    return hipGetLastError();
}

}  // namespace plp
