// Key-frame pair line triangulation (plp_median_depth_* / plp_triangulate_keyline_pairs_*, include/plp_front.h).
//
// k_median_depth: keyframe::compute_median_depth(abs) (data/keyframe.cc:825-857).  One workgroup per key frame: the float depths as
// order-preserving 32-bit keys in LDS, the element of rank (n - 1) / 2 by a four-pass radix selection (a 256-bin LDS histogram per pass).
//
// k_keyline_pair_geometry: the gates of mapping_module::triangulate_line_with_two_keyframes (mapping_module.cc:506-533) and
// module::two_view_triangulator_line::triangulate (module/two_view_triangulator_line.cc:52-296) for every query slot of every pair, one lane
// per slot in f64, grid = (P, ceil(cap / 256)).  No LDS, no barrier: triangulate is a pure function of the two key lines.
//
// k_keyline_pair_resolve: the duplicate check of the loop (:564), which is sequential in the reference.  One workgroup per group walks the
// group's pairs in order; per pair an LDS atomicMin finds, per train index, the first slot that creates a landmark, and every later slot
// with that train index becomes OCCUPIED_NGH; cur's occupancy is carried from pair to pair in LDS.
// Numeric contract: DESIGN.md section 5, D8 (the file is compiled with -ffp-contract=off).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "line3d.hpp"
#include "match_device.hpp"
#include "plp_barrier.hpp"

namespace plp {
namespace {

__device__ __forceinline__ int clamp_count(const int32_t* counts, int b, int cap) { return counts ? min(max(counts[b], 0), cap) : cap; }

// ---------------------------------------------------------------------------------------------------------------- median depth
// float -> key with the order of the floats (finite inputs: the key 0xFFFFFFFF, a NaN's, is free for the empty slots)
__device__ __forceinline__ uint32_t depth_key(float d) {
    const uint32_t b = __float_as_uint(d);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float key_depth(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k); }

constexpr uint32_t kNoDepth = 0xFFFFFFFFu;

__global__ __launch_bounds__(256) void k_median_depth(MedianDepthArgs A) {
    extern __shared__ uint32_t md_keys[];          // m_cap keys
    __shared__ uint32_t hist[256];
    __shared__ uint32_t wave_tot[4];
    __shared__ uint32_t sel[3];                    // valid count, selected bin, rank inside the bin
    const int f = blockIdx.x, tid = threadIdx.x;
    const int n = clamp_count(A.counts, f, A.m_cap);
    const double* P = A.pose + (size_t)15 * f;
    const double r20 = P[6], r21 = P[7], r22 = P[8];
    const double tz = (double)(float)P[11];        // const float trans_cw_z (keyframe.cc:840)
    if (tid == 0) sel[0] = 0;
    wg_barrier();
    uint32_t mine = 0;
    for (int i = tid; i < n; i += 256) {
        const size_t o = (size_t)f * A.m_cap + i;
        uint32_t key = kNoDepth;
        if (!A.valid || A.valid[o]) {
            const double* X = A.pos_w + 3 * o;
            double z = ((r20 * X[0] + r21 * X[1]) + r22 * X[2]) + tz;
            if (A.abs_flag) z = fabs(z);
            float d = (float)z;
            if (d == 0.0f) d = 0.0f;               // -0.0 and 0.0 tie in std::sort: the library returns +0.0 (D8)
            key = depth_key(d);
            ++mine;
        }
        md_keys[i] = key;
    }
    if (mine) atomicAdd(&sel[0], mine);
    wg_barrier();
    const uint32_t cnt = sel[0];
    if (cnt == 0) {                                // the reference throws std::out_of_range here
        if (tid == 0) { A.median[f] = 0.0f; A.count[f] = 0; }
        return;
    }
    uint32_t rank = (cnt - 1) / 2, prefix = 0, mask = 0;
    for (int shift = 24; shift >= 0; shift -= 8) {
        hist[tid] = 0;
        wg_barrier();
        for (int i = tid; i < n; i += 256) {
            const uint32_t k = md_keys[i];
            if (k != kNoDepth && (k & mask) == prefix) atomicAdd(&hist[(k >> shift) & 255u], 1u);
        }
        wg_barrier();
        // inclusive scan of the 256 bins: inside each wave by shuffles, the four wave totals through LDS
        const uint32_t h = hist[tid];
        uint32_t inc = h;
        const int lane = tid & 63;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t v = __shfl_up(inc, d, 64);
            if (lane >= d) inc += v;
        }
        if (lane == 63) wave_tot[tid >> 6] = inc;
        wg_barrier();
        uint32_t base = 0;
        for (int w = 0; w < (tid >> 6); ++w) base += wave_tot[w];
        inc += base;
        if (h != 0 && inc - h <= rank && rank < inc) { sel[1] = (uint32_t)tid; sel[2] = rank - (inc - h); }
        wg_barrier();
        prefix |= sel[1] << shift;
        mask |= 255u << shift;
        rank = sel[2];
        wg_barrier();                              // sel and hist are rewritten by the next pass
    }
    if (tid == 0) { A.median[f] = key_depth(prefix); A.count[f] = (int32_t)cnt; }
}

// ---------------------------------------------------------------------------------------------------------------- geometry
enum : uint8_t {
    kCreated = PLP_KLP_CREATED, kGateDistance = PLP_KLP_GATE_DISTANCE, kGateEndpoints = PLP_KLP_GATE_ENDPOINTS, kGateAngle = PLP_KLP_GATE_ANGLE,
    kOccupiedCur = PLP_KLP_OCCUPIED_CUR, kOccupiedNgh = PLP_KLP_OCCUPIED_NGH, kNoParallax = PLP_KLP_NO_PARALLAX, kTooClose = PLP_KLP_TOO_CLOSE,
    kTooLong = PLP_KLP_TOO_LONG, kDepth = PLP_KLP_DEPTH, kReprojMid = PLP_KLP_REPROJ_MID, kReprojEnd = PLP_KLP_REPROJ_END,
    kScale = PLP_KLP_SCALE, kNonFinite = PLP_KLP_NON_FINITE, kKpDepthRange = PLP_KLP_KP_DEPTH_RANGE
};

__device__ __forceinline__ float point_distance(float x, float y) { return (float)sqrt((double)(x * x + y * y)); }

// :68-85: the bearing of the key line's middle point, turned by rot_w? = rot_?w^T (row i of rot_w? is column i of the pose row's rot_cw)
__device__ __forceinline__ void bearing_w(const KeylinePairArgs& A, const double* P, float px, float py, double (&w)[3]) {
    const double x = ((double)px - A.cx) / A.fx, y = ((double)py - A.cy) / A.fy;
    const double n = sqrt((x * x + y * y) + 1.0);
    const double c[3] = {x / n, y / n, 1.0 / n};
#pragma unroll
    for (int i = 0; i < 3; ++i) w[i] = (P[i] * c[0] + P[3 + i] * c[1]) + P[6 + i] * c[2];
}

__device__ __forceinline__ double norm3(const double (&a)[3], const double* b) {
    const double dx = a[0] - b[0], dy = a[1] - b[1], dz = a[2] - b[2];
    return sqrt((dx * dx + dy * dy) + dz * dz);
}

__device__ __forceinline__ double depth_in(const double* P, const double (&p)[3]) { return ((P[6] * p[0] + P[7] * p[1]) + P[8] * p[2]) + P[11]; }

// camera::perspective::reproject_to_image (perspective.cc:190-209), the sums of plp_observe_*'s reproject<PERSPECTIVE>; false = z <= 0, nothing written
__device__ __forceinline__ bool reproject(const KeylinePairArgs& A, const double* P, const double (&p)[3], double& u, double& v) {
    const double xc = ((P[0] * p[0] + P[1] * p[1]) + P[2] * p[2]) + P[9];
    const double yc = ((P[3] * p[0] + P[4] * p[1]) + P[5] * p[2]) + P[10];
    const double zc = ((P[6] * p[0] + P[7] * p[1]) + P[8] * p[2]) + P[11];
    if (zc <= 0.0) return false;
    const double z_inv = 1.0 / zc;
    u = (A.fx * xc) * z_inv + A.cx;
    v = (A.fy * yc) * z_inv + A.cy;
    return true;
}

// check_scale_factors (.h:134-151)
__device__ __forceinline__ bool scale_ok(const double (&p)[3], const double* P1, const double* P2, float sf1, float sf2, float ratio_factor) {
    const double d1 = norm3(p, P1 + 12), d2 = norm3(p, P2 + 12);
    if (d1 == 0 || d2 == 0) return false;
    const double ratio_dists = d2 / d1;
    const float ratio_octave = sf1 / sf2;
    return (double)ratio_octave / ratio_dists < (double)ratio_factor && ratio_dists / (double)ratio_octave < (double)ratio_factor;
}

// two_view_triangulator_line::triangulate(idx_1 = j of key frame f1, idx_2 = t of key frame f2) -> the status, sp / ep where it is kCreated
__device__ uint8_t triangulate_pair_of_keyframes(const KeylinePairArgs& A, int f1, int f2, int j, int t, double (&sp)[3], double (&ep)[3]) {
    const size_t o1 = (size_t)f1 * A.cap + j, o2 = (size_t)f2 * A.cap + t;
    const plp_keyline& k1 = A.kl[o1];
    const plp_keyline& k2 = A.kl[o2];
    const double* P1 = A.pose + (size_t)15 * f1;
    const double* P2 = A.pose + (size_t)15 * f2;
    const bool s1 = 0.0f <= A.x_right[2 * o1], s2 = 0.0f <= A.x_right[2 * o2];
    double w1[3], w2[3];
    bearing_w(A, P1, k1.pt_x, k1.pt_y, w1);
    bearing_w(A, P2, k2.pt_x, k2.pt_y, w2);
    const double cr = (w1[0] * w2[0] + w1[1] * w2[1]) + w1[2] * w2[2];
    // depths_.at(idx): the KEY POINTS' depths read with a key-line index (D8 item 2)
    double c1 = 2.0, c2 = 2.0;
    if (s1) {
        if (j >= (A.kp_counts ? min(max(A.kp_counts[f1], 0), A.kp_cap) : A.kp_cap)) return kKpDepthRange;
        c1 = cos(2.0 * atan2(A.half_baseline, (double)A.kp_depths[(size_t)f1 * A.kp_cap + j]));
    }
    if (s2) {
        if (t >= (A.kp_counts ? min(max(A.kp_counts[f2], 0), A.kp_cap) : A.kp_cap)) return kKpDepthRange;
        c2 = cos(2.0 * atan2(A.half_baseline, (double)A.kp_depths[(size_t)f2 * A.kp_cap + t]));
    }
    const double cs = c2 < c1 ? c2 : c1;   // std::min
    const bool two = ((!s1 && !s2) && 0.0 < cr && cr < (double)A.cos_thr) || ((s1 || s2) && 0.0 < cr && cr < cs);
    if (two) {
        // P_k = eigen_cam_matrix_ * Tcw_k, three terms per coefficient, the zero entries of the camera matrix included
        double Pa[12], Pb[12], T[18];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const double a0 = c < 3 ? P1[c] : P1[9], a1 = c < 3 ? P1[3 + c] : P1[10], a2 = c < 3 ? P1[6 + c] : P1[11];
            const double b0 = c < 3 ? P2[c] : P2[9], b1 = c < 3 ? P2[3 + c] : P2[10], b2 = c < 3 ? P2[6 + c] : P2[11];
            Pa[c] = (A.fx * a0 + 0.0 * a1) + A.cx * a2;
            Pa[4 + c] = (0.0 * a0 + A.fy * a1) + A.cy * a2;
            Pa[8 + c] = (0.0 * a0 + 0.0 * a1) + 1.0 * a2;
            Pb[c] = (A.fx * b0 + 0.0 * b1) + A.cx * b2;
            Pb[4 + c] = (0.0 * b0 + A.fy * b1) + A.cy * b2;
            Pb[8 + c] = (0.0 * b0 + 0.0 * b1) + 1.0 * b2;
        }
        // transformation_line_cw's top rows: rot_1w_ | skew(trans_1w_) * rot_1w_, skew = (0, -tz, ty; tz, 0, -tx; -ty, tx, 0)
        const double tx = P1[9], ty = P1[10], tz = P1[11];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double r0 = P1[c], r1 = P1[3 + c], r2 = P1[6 + c];
            T[c] = r0; T[6 + c] = r1; T[12 + c] = r2;
            T[3 + c] = (0.0 * r0 + (-tz) * r1) + ty * r2;
            T[9 + c] = (tz * r0 + 0.0 * r1) + (-tx) * r2;
            T[15 + c] = ((-ty) * r0 + tx * r1) + 0.0 * r2;
        }
        const double K[9] = {A.fy, 0.0, 0.0, 0.0, A.fx, 0.0, -A.fy * A.cx, -A.fx * A.cy, A.fx * A.fy};
        if (!line3d_triangulate_pair(Pa, Pb, T, K, k1.startPointX, k1.startPointY, k1.endPointX, k1.endPointY, k2.startPointX, k2.startPointY,
                                     k2.endPointX, k2.endPointY, sp, ep))
            return kNonFinite;
    } else {
        const double* row;
        if (s1 && c1 < c2) row = A.lines_3d + 6 * o1;          // keyfrm_1_->triangulate_stereo_for_line(idx_1), a zero row included
        else if (s2 && c2 < c1) row = A.lines_3d + 6 * o2;
        else return kNoParallax;
        if (A.setup_type == 0 || !A.lines_3d) return kNoParallax;   // the reference leaves sp_3D / ep_3D unset: no landmark (D8 item 4)
#pragma unroll
        for (int i = 0; i < 3; ++i) { sp[i] = row[i]; ep[i] = row[3 + i]; }
    }
#pragma unroll
    for (int i = 0; i < 3; ++i)
        if (!isfinite(sp[i]) || !isfinite(ep[i])) return kNonFinite;
    const double med = (double)A.median[f2];                    // key frame 2's, all three times (:246-253)
    if (norm3(sp, P1 + 12) / med < 0.3 || norm3(ep, P2 + 12) / med < 0.3) return kTooClose;
    if (norm3(ep, sp) / med > 0.9) return kTooLong;
    if (!(0 < depth_in(P1, sp)) || !(0 < depth_in(P2, sp)) || !(0 < depth_in(P1, ep)) || !(0 < depth_in(P2, ep))) return kDepth;
    const double mid[3] = {0.5 * (sp[0] + ep[0]), 0.5 * (sp[1] + ep[1]), 0.5 * (sp[2] + ep[2])};
    const int oc1 = min(max(k1.octave, 0), A.num_levels - 1), oc2 = min(max(k2.octave, 0), A.num_levels - 1);
    const float lim1 = 5.99146f * A.level_sigma_sq[oc1], lim2 = 5.99146f * A.level_sigma_sq[oc2];
    double u, v;
    // the midpoint in both key frames: squaredNorm of reproj - pt (f64) against the float product
    if (!reproject(A, P1, mid, u, v)) return kReprojMid;
    {
        const double ex = u - (double)k1.pt_x, ey = v - (double)k1.pt_y, sq = ex * ex + ey * ey;
        if (!isfinite(sq)) return kNonFinite;
        if ((double)lim1 < sq) return kReprojMid;
    }
    if (!reproject(A, P2, mid, u, v)) return kReprojMid;
    {
        const double ex = u - (double)k2.pt_x, ey = v - (double)k2.pt_y, sq = ex * ex + ey * ey;
        if (!isfinite(sq)) return kNonFinite;
        if ((double)lim2 < sq) return kReprojMid;
    }
    // the end points against the key-line functions: the f64 quotient rounded to float, the float abs, no square (:313-316)
#pragma unroll
    for (int view = 0; view < 2; ++view) {
        const double* P = view ? P2 : P1;
        const double* fn = A.line_fn + 3 * (view ? o2 : o1);
        const double l0 = fn[0], l1 = fn[1], l2 = fn[2];
        const float lim = view ? lim2 : lim1;
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            if (!reproject(A, P, e ? ep : sp, u, v)) return kNonFinite;   // not reachable: the same sum was just found positive
            const float err = (float)(((l0 * u + l1 * v) + l2) / sqrt(l0 * l0 + l1 * l1));
            if (!isfinite(err)) return kNonFinite;
            if (lim < fabsf(err)) return kReprojEnd;
        }
    }
    const float sf1 = A.scale_factors[oc1], sf2 = A.scale_factors[oc2];
    if (!scale_ok(sp, P1, P2, sf1, sf2, A.ratio_factor) || !scale_ok(ep, P1, P2, sf1, sf2, A.ratio_factor)) return kScale;
    return kCreated;
}

__global__ __launch_bounds__(256) void k_keyline_pair_geometry(KeylinePairArgs A) {
    const int p = blockIdx.x, j = blockIdx.y * 256 + threadIdx.x;
    const int f1 = A.pairs[2 * p], f2 = A.pairs[2 * p + 1];
    if ((unsigned)f1 >= (unsigned)A.F || (unsigned)f2 >= (unsigned)A.F) return;   // outside the table: nothing read, nothing written
    if (j >= clamp_count(A.counts, f1, A.cap)) return;
    const int n2 = clamp_count(A.counts, f2, A.cap);
    const size_t o = (size_t)p * A.cap + j;
    const int t = A.train_idx[o];
    uint8_t st;
    double sp[3] = {0.0, 0.0, 0.0}, ep[3] = {0.0, 0.0, 0.0};
    // DMatch.distance (float) < dist_thr; the 1-NN's "nothing within 128" (-1, 256) and any index outside key frame 2 stop here
    if (!((float)A.dist[o] < A.dist_thr && t >= 0 && t < n2)) {
        st = kGateDistance;
    } else {
        const plp_keyline& l1 = A.kl[(size_t)f1 * A.cap + j];
        const plp_keyline& l2 = A.kl[(size_t)f2 * A.cap + t];
        const float ds = point_distance(l1.startPointX - l2.startPointX, l1.startPointY - l2.startPointY);
        const float de = point_distance(l1.endPointX - l2.endPointX, l1.endPointY - l2.endPointY);
        const float angle = (float)((double)(fabsf(fabsf(l1.angle) - fabsf(l2.angle)) * 180.f) / 3.14);   // D7 items 1-2
        if (!(ds < A.endpoint_thr && de < A.endpoint_thr)) st = kGateEndpoints;
        else if (!(angle < A.angle_thr)) st = kGateAngle;
        else st = triangulate_pair_of_keyframes(A, f1, f2, j, t, sp, ep);
    }
    const bool made = st == kCreated;
    A.out_status[o] = st;
    A.out_match[o] = made ? t : -1;
    double* out = A.out_pos_w + 6 * o;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        out[i] = made ? sp[i] : 0.0;
        out[3 + i] = made ? ep[i] : 0.0;
    }
}

// ---------------------------------------------------------------------------------------------------------------- resolve
__global__ __launch_bounds__(256) void k_keyline_pair_resolve(KeylinePairArgs A) {
    extern __shared__ int32_t first_winner[];                  // cap: per train index of the pair, the first slot that creates a landmark
    uint8_t* occ_cur = (uint8_t*)(first_winner + A.cap);       // cap: cur's slots, carried from pair to pair
    const int g = blockIdx.x, tid = threadIdx.x;
    const int begin = min(max(A.group_offsets[g], 0), A.P), end = min(max(A.group_offsets[g + 1], 0), A.P);
    if (begin >= end) return;                                  // an empty group has no cur
    const int f1 = A.pairs[2 * begin];
    if ((unsigned)f1 >= (unsigned)A.F) return;
    const int n1 = clamp_count(A.counts, f1, A.cap);
    for (int j = tid; j < n1; j += 256) occ_cur[j] = A.occupied[(size_t)f1 * A.cap + j] ? 1 : 0;   // slot j is only ever touched by this lane
    for (int p = begin; p < end; ++p) {
        const int f2 = A.pairs[2 * p + 1];
        if (A.pairs[2 * p] != f1 || (unsigned)f2 >= (unsigned)A.F) continue;   // not a pair of this group (uniform): the geometry's statuses stay
        const uint8_t* occ_ngh = A.occupied + (size_t)f2 * A.cap;
        const size_t base = (size_t)p * A.cap;
        if (A.skip_occupied) {
            const int n2 = clamp_count(A.counts, f2, A.cap);
            for (int t = tid; t < n2; t += 256) first_winner[t] = 0x7FFFFFFF;
            wg_barrier();
            for (int j = tid; j < n1; j += 256)
                if (A.out_status[base + j] == kCreated && !occ_cur[j]) atomicMin(&first_winner[A.out_match[base + j]], j);
            wg_barrier();
        }
        for (int j = tid; j < n1; j += 256) {
            const uint8_t st = A.out_status[base + j];
            if (st == kGateDistance || st == kGateEndpoints || st == kGateAngle) continue;   // never reached the duplicate check
            uint8_t now = st;
            if (A.skip_occupied) {
                const int t = A.train_idx[base + j];           // inside key frame 2: the slot passed the gates
                if (occ_cur[j]) now = kOccupiedCur;
                else if (occ_ngh[t] || first_winner[t] < j) now = kOccupiedNgh;
            }
            if (now != st) {
                A.out_status[base + j] = now;
                if (st == kCreated) {
                    A.out_match[base + j] = -1;
                    double* out = A.out_pos_w + 6 * (base + j);
#pragma unroll
                    for (int i = 0; i < 6; ++i) out[i] = 0.0;
                }
            }
            if (now == kCreated) occ_cur[j] = 1;               // add_landmark_line(lm_line, queryIdx)
        }
        if (A.skip_occupied) wg_barrier();                     // first_winner is reset by the next pair
    }
    for (int j = tid; j < n1; j += 256) A.out_occ_cur[(size_t)g * A.cap + j] = occ_cur[j];
}

}  // namespace

hipError_t launch_median_depth(hipStream_t st, const MedianDepthArgs& A, int F) {
    hipLaunchKernelGGL(k_median_depth, dim3(F), dim3(256), (size_t)A.m_cap * 4, st, A);
    return hipGetLastError();
}

hipError_t launch_keyline_pairs(hipStream_t st, const KeylinePairArgs& A) {
    hipLaunchKernelGGL(k_keyline_pair_geometry, dim3(A.P, (A.cap + 255) / 256), dim3(256), 0, st, A);
    if (hipError_t e = hipGetLastError()) return e;
    hipLaunchKernelGGL(k_keyline_pair_resolve, dim3(A.G), dim3(256), (size_t)A.cap * 5, st, A);
    return hipGetLastError();
}

}  // namespace plp
