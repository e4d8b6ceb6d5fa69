// landmark::update_normal_and_depth (data/landmark.cc:249-295) and Line::update_information (data/landmark_line.cc:311-352), one definition
// of the arithmetic and of the statuses for host and device (plp_landmark[_line]_geometry_* / plp_model_landmark_geometry_host,
// include/plp_front.h).  f64 with IEEE + - * / sqrt only, every sum left to right, no libm call; translation units
// that include this file are compiled with -ffp-contract=off.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/plp_front.h"

namespace plp {

struct LandmarkGeometryArgs {
    int F, cap, L;
    int num_levels, num_levels_lsd;
    float scale_factors[16], scale_factors_lsd[16];
    const double* pose; const int32_t* counts; const plp_keypoint* kps; const plp_keyline* kl;
    const double* pos_w; const int32_t* ref_kf; const uint8_t* skip;
    const int32_t* obs_offsets; const int32_t* obs_kf; const int32_t* obs_idx;
    double* normal; float* min_dist; float* max_dist; uint8_t* status;
};
// both return the first error of their launch (landmark_geometry_kernels.hip)
hipError_t launch_landmark_geometry_points(hipStream_t st, const LandmarkGeometryArgs& A);
hipError_t launch_landmark_geometry_lines(hipStream_t st, const LandmarkGeometryArgs& A);

struct LgVec3 { double x, y, z; };

// Eigen 3.3 normalized(): v / sqrt(squaredNorm) when the squared norm is positive, else v as it is (D5 item 1)
__host__ __device__ __forceinline__ LgVec3 lg_normalized(double x, double y, double z) {
    const double sq = (x * x + y * y) + z * z;
    if (sq > 0.0) {
        const double s = __builtin_sqrt(sq);
        return {x / s, y / s, z / s};
    }
    return {x, y, z};
}

__host__ __device__ __forceinline__ double lg_norm(double x, double y, double z) { return __builtin_sqrt((x * x + y * y) + z * z); }

// max_valid_dist_ = dist * scale_factor: double * float in f64, stored to the float member; min_valid_dist_ = max_valid_dist_ / scale_factors_.at(n - 1): float / float
__host__ __device__ __forceinline__ void lg_valid_range(double dist, float sf_level, float sf_last, float* out_min, float* out_max) {
    const float mx = (float)(dist * (double)sf_level);
    *out_max = mx;
    *out_min = mx / sf_last;
}

__host__ __device__ __forceinline__ int lg_count(const LandmarkGeometryArgs& A, int f) {
    if (!A.counts) return A.cap;
    const int n = A.counts[f];
    return n < 0 ? 0 : (n > A.cap ? A.cap : n);
}

// What landmark::update_normal_and_depth does with the sum of the unit vectors (sx, sy, sz) of landmark l, which has n_obs observations.
// found: the list position of the first observation whose key frame is ref_kf[l], -1 = none; bad: an obs_kf of the list lies outside the
// table.  Writes the three value outputs where the status is PLP_LG_UPDATED and returns the status (the caller stores it).
__host__ __device__ __forceinline__ uint8_t lg_point_finish(const LandmarkGeometryArgs& A, int l, int n_obs, double sx, double sy, double sz, int found,
                                                            bool bad) {
    if (A.skip && A.skip[l]) return PLP_LG_SKIPPED;                      // will_be_erased_ (:257-260)
    if (n_obs <= 0) return PLP_LG_NO_OBSERVATIONS;                        // :266-269
    const int ref = A.ref_kf[l];
    if (bad || (unsigned)ref >= (unsigned)A.F) return PLP_LG_INDEX_RANGE;
    if (found < 0) return PLP_LG_REF_NOT_OBSERVED;                        // observations.at(ref_keyfrm) throws (:285)
    const int idx = A.obs_idx[found];
    if ((unsigned)idx >= (unsigned)lg_count(A, ref)) return PLP_LG_INDEX_RANGE;   // undist_keypts_.at(idx) throws
    const int octave = A.kps[(size_t)ref * A.cap + idx].octave;
    if ((unsigned)octave >= (unsigned)A.num_levels) return PLP_LG_OCTAVE_RANGE;   // scale_factors_.at(scale_level) throws (:286)
    const double* p = A.pos_w + (size_t)3 * l;
    const double* c = A.pose + (size_t)15 * ref + 12;
    const double dist = lg_norm(p[0] - c[0], p[1] - c[1], p[2] - c[2]);   // cam_to_lm_vec.norm() (:283-284)
    lg_valid_range(dist, A.scale_factors[octave], A.scale_factors[A.num_levels - 1], A.min_dist + l, A.max_dist + l);
    const LgVec3 n = lg_normalized(sx, sy, sz);                           // mean_normal.normalized() (:293)
    double* out = A.normal + (size_t)3 * l;
    out[0] = n.x; out[1] = n.y; out[2] = n.z;
    return PLP_LG_UPDATED;
}

// Line::update_information for landmark l, whole: the walk over its observations looks for the reference key frame's feature index only
// (observations[ref_kf] is operator[]: a key frame that is not among them gives index 0, :343).  Writes the two value outputs where the
// status is PLP_LG_UPDATED and returns the status.
__host__ __device__ __forceinline__ uint8_t lg_line(const LandmarkGeometryArgs& A, int l) {
    if (A.skip && A.skip[l]) return PLP_LG_SKIPPED;                      // _will_be_erased (:324-325)
    const int beg = A.obs_offsets[l], end = A.obs_offsets[l + 1];
    if (end <= beg) return PLP_LG_NO_OBSERVATIONS;                        // :333-334
    const int ref = A.ref_kf[l];
    if ((unsigned)ref >= (unsigned)A.F) return PLP_LG_INDEX_RANGE;
    int idx = 0;
    bool found = false, bad = false;
    for (int o = beg; o < end; ++o) {
        const int kf = A.obs_kf[o];
        if ((unsigned)kf >= (unsigned)A.F) bad = true;
        else if (!found && kf == ref) { found = true; idx = A.obs_idx[o]; }
    }
    if (bad) return PLP_LG_INDEX_RANGE;
    if ((unsigned)idx >= (unsigned)lg_count(A, ref)) return PLP_LG_INDEX_RANGE;
    const int level = A.kl[(size_t)ref * A.cap + idx].octave;
    if ((unsigned)level >= (unsigned)A.num_levels_lsd) return PLP_LG_OCTAVE_RANGE;
    const double* p = A.pos_w + (size_t)6 * l;
    const double* c = A.pose + (size_t)15 * ref + 12;
    const double mx = 0.5 * (p[0] + p[3]), my = 0.5 * (p[1] + p[4]), mz = 0.5 * (p[2] + p[5]);   // mp = 0.5 * (sp + ep) (:339)
    const double distance = lg_norm(mx - c[0], my - c[1], mz - c[2]);    // :342
    // :349-350: the LSD table at the key line's level, then the ORB table at the LSD level count
    lg_valid_range(distance, A.scale_factors_lsd[level], A.scale_factors[A.num_levels_lsd - 1], A.min_dist + l, A.max_dist + l);
    return PLP_LG_UPDATED;
}

}  // namespace plp
