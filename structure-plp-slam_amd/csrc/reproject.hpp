// Device helpers shared by observe_kernels.hip, project_kernels.hip and sim3.hpp (which builds reproject<MODEL> for the host too): camera::*::reproject_to_image of the three models,
// predict_scale_level, the norm of cam_to_lm_vec and the carried end-point temporaries of the line loops.
// Every translation unit that includes this file is compiled with -ffp-contract=off; the helpers have internal linkage.
#pragma once
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include "../../include/plp_front.h"
#include "plp_barrier.hpp"

namespace plp {
namespace {

struct Reproj {
    double u, v, xr;
    bool wrote, in;   // wrote: reproj / x_right were assigned (z > 0, or equirectangular); in: the function's result
};

// camera::*::reproject_to_image.  P = rot_cw_ row-major (0-8), trans_cw_ (9-11), cam_center_ (12-14).  A: ObserveArgs or ProjectArgs (the
// camera fields model-independent code reads: fx, fy, cx, cy, fxb, cols_d, rows_d, bounds).
template <int MODEL, class Args>
__host__ __device__ __forceinline__ Reproj reproject(const Args& A, const double* P, double x, double y, double z) {
    Reproj r;
    const double xc = ((P[0] * x + P[1] * y) + P[2] * z) + P[9];   // rot_cw * pos_w + trans_cw
    const double yc = ((P[3] * x + P[4] * y) + P[5] * z) + P[10];
    const double zc = ((P[6] * x + P[7] * y) + P[8] * z) + P[11];
    if constexpr (MODEL == PLP_CAMERA_EQUIRECTANGULAR) {   // equirectangular.cc:104-119
        const double sq = (xc * xc + yc * yc) + zc * zc;     // Eigen 3.3 normalized(): v / sqrt(squaredNorm), a zero vector stays zero
        double bx = xc, by = yc, bz = zc;
        if (sq > 0.0) {
            const double s = sqrt(sq);
            bx = xc / s; by = yc / s; bz = zc / s;
        }
        const double latitude = -asin(by);
        const double longitude = atan2(bx, bz);
        r.u = A.cols_d * (0.5 + longitude / (2.0 * 3.14159265358979323846));
        r.v = A.rows_d * (0.5 - latitude / 3.14159265358979323846);
        r.xr = 0.0;
        r.wrote = true; r.in = true;
        return r;
    } else {   // perspective.cc:190-209; fisheye.cc:231-249 is the same formula
        r.u = 0.0; r.v = 0.0; r.xr = 0.0;
        if (zc <= 0.0) { r.wrote = false; r.in = false; return r; }
        const double z_inv = 1.0 / zc;
        r.u = (A.fx * xc) * z_inv + A.cx;
        r.v = (A.fy * yc) * z_inv + A.cy;
        r.xr = r.u - A.fxb * z_inv;
        r.wrote = true;
        r.in = (double)A.bounds[0] < r.u && r.u < (double)A.bounds[1] && (double)A.bounds[2] < r.v && r.v < (double)A.bounds[3];
        return r;
    }
}

// landmark::predict_scale_level (landmark.cc:319-340) / Line::predict_scale_level (landmark_line.cc:366-387)
__device__ __forceinline__ int predict_level(float max_valid, float dist, float log_sf, int num_levels) {
    const float ratio = max_valid / dist;
    const float lg = (float)log((double)ratio);          // std::log(float) = logf, defined as (float)log((double)x) (D5 item 3)
    const float c = ceilf(lg / log_sf);
    // static_cast<int> of a value outside int's range (inf, NaN included) is undefined; defined as x86's cvttss2si: INT_MIN (D5 item 4)
    const int p = (c >= -2147483648.f && c < 2147483648.f) ? (int)c : INT_MIN;
    if (p < 0) return 0;
    if ((unsigned)num_levels <= (unsigned)p) return num_levels - 1;
    return p;
}

// |v| of cam_to_lm_vec, left to right
__device__ __forceinline__ double norm3(double x, double y, double z) { return sqrt((x * x + y * y) + z * z); }

// The reference's end-point temporaries across one chunk of 256 slots of a workgroup of four waves (D5 item 5, D6).  On entry s / e hold
// this lane's own values (meaningful where ws / we: its slot wrote that end point), K values each (u, v [, x_right]; T = float, or double
// for the f64 queries of the fuse modes); on exit, the temporaries after this slot's turn: the nearest writer at or below this lane in the
// wave (64-bit ballot), else the last writer of an earlier wave (LDS), else what the previous chunks carried (cs / ce, updated to the
// chunk's last writers).  Returns the number of ok lanes of the chunk.  Uniform over the workgroup; ends with the barrier behind which
// the next call may rewrite the LDS.
template <int K, class T>
__device__ __forceinline__ int carry_chunk(bool ws, bool we, bool ok, T (&s)[K], T (&e)[K], T (&cs)[K], T (&ce)[K]) {
    __shared__ T s_last[4][2 * K];   // per wave: its last start-point writer's values, then its last end-point writer's
    __shared__ int s_has[4][2];
    __shared__ int s_num[4];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const unsigned long long at_or_below = ~0ull >> (63 - lane);
    const unsigned long long ms = __ballot(ws), me = __ballot(we), mv = __ballot(ok);
    const unsigned long long ks = ms & at_or_below, ke = me & at_or_below;
    const int src_s = ks ? 63 - __clzll(ks) : lane, src_e = ke ? 63 - __clzll(ke) : lane;
#pragma unroll
    for (int k = 0; k < K; ++k) { s[k] = __shfl(s[k], src_s); e[k] = __shfl(e[k], src_e); }
    if (lane == 63) {
#pragma unroll
        for (int k = 0; k < K; ++k) { s_last[w][k] = s[k]; s_last[w][K + k] = e[k]; }
        s_has[w][0] = ms != 0; s_has[w][1] = me != 0;
        s_num[w] = (int)__popcll(mv);
    }
    wg_barrier();
    // what precedes this wave: the last wave before it with a writer, else the carry; what follows the chunk: the same over all four
    int total = 0;
    for (int v = 0; v < 4; ++v) {
        if (v == w) {
#pragma unroll
            for (int k = 0; k < K; ++k) {
                if (!ks) s[k] = cs[k];
                if (!ke) e[k] = ce[k];
            }
        }
#pragma unroll
        for (int k = 0; k < K; ++k) {
            if (s_has[v][0]) cs[k] = s_last[v][k];
            if (s_has[v][1]) ce[k] = s_last[v][K + k];
        }
        total += s_num[v];
    }
    wg_barrier();   // the next chunk rewrites s_last
    return total;
}

}  // namespace
}  // namespace plp
