// Two-view line triangulation by plane intersection and end-point trimming, in f64: the algebra of frame::triangulate_stereo_for_line's
// stereo branch (data/frame.cc:1009-1104) and of two_view_triangulator_line::triangulate (module/two_view_triangulator_line.cc:117-205),
// which differ only in P1, P2 and the line transformation.  Numeric contract: DESIGN.md section 5, D7.  Every Eigen expression is written out
// left to right with all of its terms, the zero entries of the matrices included (the file including this one is compiled with
// -ffp-contract=off), so that a non-finite value reaches every sum it feeds.
#pragma once
#include <hip/hip_runtime.h>

namespace plp {

// Eigen 3.3 MatrixBase::cross: (a1 b2 - a2 b1, a2 b0 - a0 b2, a0 b1 - a1 b0)
__host__ __device__ __forceinline__ void line3d_cross(const double (&a)[3], const double (&b)[3], double (&r)[3]) {
    r[0] = a[1] * b[2] - a[2] * b[1];
    r[1] = a[2] * b[0] - a[0] * b[2];
    r[2] = a[0] * b[1] - a[1] * b[0];
}

// line^T * P (Vec4_t plane = line.transpose() * P) and P^T * line (Vec4_t plane = P.transpose() * line): the same sums,
// plane(j) = (line(0) P(0,j) + line(1) P(1,j)) + line(2) P(2,j); P is 3 x 4 row-major
__host__ __device__ __forceinline__ void line3d_plane(const double (&P)[12], const double (&l)[3], double (&pl)[4]) {
#pragma unroll
    for (int j = 0; j < 4; ++j) pl[j] = (l[0] * P[j] + l[1] * P[4 + j]) + l[2] * P[8 + j];
}

__host__ __device__ __forceinline__ bool line3d_finite(double v) { return __builtin_isfinite(v); }

// One end point p of view 1 trimmed to the 3-D line (Pluecker matrix M, 4 x 4 row-major; l = its reprojection into view 1, den = l1 l1 + l2 l2):
//   x_closet = -(p.y - (l2 / l1) * p.x + (l3 / l2)) * ((l1 * l2) / (l1 * l1 + l2 * l2)),  y_closet = -(l1 / l2) * x_closet - (l3 / l2)
//   x_0 = 0, y_0 = p.y - (l2 / l1) * p.x;  line_temp = (x_closet, y_closet, 1).cross((x_0, y_0, 1));  plane3d_temp = P1^T * line_temp
//   intersect_endpoint = M * plane3d_temp (row sums left to right);  out = intersect_endpoint(0..2) / intersect_endpoint(3)
// Returns false when the intersection or the end point is not finite.
__host__ __device__ __forceinline__ bool line3d_trim(const double (&P1)[12], const double (&M)[16], double l1, double l2, double l3, double den, float px,
                                            float py, double (&out)[3]) {
    const double x = (double)px, y = (double)py;
    const double xc = -((y - (l2 / l1) * x) + (l3 / l2)) * ((l1 * l2) / den);
    const double yc = -(l1 / l2) * xc - (l3 / l2);
    const double y0 = y - (l2 / l1) * x;
    const double pc[3] = {xc, yc, 1.0}, p0[3] = {0.0, y0, 1.0};
    double lt[3], pt[4], I[4];
    line3d_cross(pc, p0, lt);
    line3d_plane(P1, lt, pt);
#pragma unroll
    for (int i = 0; i < 4; ++i) I[i] = ((M[4 * i] * pt[0] + M[4 * i + 1] * pt[1]) + M[4 * i + 2] * pt[2]) + M[4 * i + 3] * pt[3];
    bool ok = true;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        out[i] = I[i] / I[3];
        ok = ok && line3d_finite(out[i]);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) ok = ok && line3d_finite(I[i]);
    return ok;
}

// The 3-D line through two image lines of views P1 / P2 (end points s1-e1 in view 1, s2-e2 in view 2, pixel coordinates as the reference's
// cv::Point2f), its end points trimmed against view 1's segment.  T: the top three rows of transformation_line_cw (3 x 6 row-major), K: the
// line projection matrix _K (3 x 3 row-major).  sp / ep = the trimmed end points in P1's frame (intersect_endpoint(0..2) / intersect_endpoint(3)).
// Returns false when a value on the way is not finite (D7): the divisors l1, l2, l1^2 + l2^2, the two homogeneous intersections and the end
// points are tested; every other intermediate reaches one of them through a product or a sum of the written-out expressions.
__device__ __forceinline__ bool line3d_triangulate_pair(const double (&P1)[12], const double (&P2)[12], const double (&T)[18], const double (&K)[9],
                                                        float s1x, float s1y, float e1x, float e1y, float s2x, float s2y, float e2x, float e2y,
                                                        double (&sp)[3], double (&ep)[3]) {
    // construct two planes: line_k = xs_k.cross(xe_k), plane_1 = line_1^T * P1, plane_2 = line_2^T * P2
    const double xs1[3] = {(double)s1x, (double)s1y, 1.0}, xe1[3] = {(double)e1x, (double)e1y, 1.0};
    const double xs2[3] = {(double)s2x, (double)s2y, 1.0}, xe2[3] = {(double)e2x, (double)e2y, 1.0};
    double line1[3], line2[3], pl1[4], pl2[4];
    line3d_cross(xs1, xe1, line1);
    line3d_cross(xs2, xe2, line2);
    line3d_plane(P1, line1, pl1);
    line3d_plane(P2, line2, pl2);
    // L_star = plane_1 * plane_2^T - plane_2 * plane_1^T, element (i, j) = p1(i) p2(j) - p2(i) p1(j); only the entries read are formed:
    // d = (L(2,1), L(0,2), L(1,0)), m = L.block<3,1>(0,3)
    const double d[3] = {pl1[2] * pl2[1] - pl2[2] * pl1[1], pl1[0] * pl2[2] - pl2[0] * pl1[2], pl1[1] * pl2[0] - pl2[1] * pl1[0]};
    const double m[3] = {pl1[0] * pl2[3] - pl2[0] * pl1[3], pl1[1] * pl2[3] - pl2[1] * pl1[3], pl1[2] * pl2[3] - pl2[2] * pl1[3]};
    const double pk[6] = {m[0], m[1], m[2], d[0], d[1], d[2]};   // plucker_coord
    // (transformation_line_cw * plucker_coord).block<3,1>(0,0): v(i) = sum over k = 0..5 of T(i,k) pk(k), left to right
    double v[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        double s = T[6 * i] * pk[0];
#pragma unroll
        for (int k = 1; k < 6; ++k) s = s + T[6 * i + k] * pk[k];
        v[i] = s;
    }
    // reproj_line_function = _K * v: r(i) = (K(i,0) v0 + K(i,1) v1) + K(i,2) v2
    const double l1 = (K[0] * v[0] + K[1] * v[1]) + K[2] * v[2];
    const double l2 = (K[3] * v[0] + K[4] * v[1]) + K[5] * v[2];
    const double l3 = (K[6] * v[0] + K[7] * v[1]) + K[8] * v[2];
    const double den = l1 * l1 + l2 * l2;
    bool ok = line3d_finite(l1) && line3d_finite(l2) && line3d_finite(den);
    // the Pluecker matrix: skew(m) | d over -d^T | 0 (Eigen::Matrix4d::Zero() with three blocks assigned)
    const double M[16] = {0.0, -m[2], m[1], d[0],
                          m[2], 0.0, -m[0], d[1],
                          -m[1], m[0], 0.0, d[2],
                          -d[0], -d[1], -d[2], 0.0};
    // end points trimming (using view 1), each end point as written at frame.cc:1062-1097
    ok = line3d_trim(P1, M, l1, l2, l3, den, s1x, s1y, sp) && ok;
    ok = line3d_trim(P1, M, l1, l2, l3, den, e1x, e1y, ep) && ok;
    return ok;
}

}  // namespace plp
