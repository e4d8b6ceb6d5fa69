"""CPU restatement of the key-frame pair point triangulation (plp_keyframe_pair_geometry_* / plp_triangulate_keypoint_pairs_*): the point half
of mapping_module::create_new_landmarks (mapping_module.cc:359-479) around robust::match_for_triangulation -- the baseline gate (:386-402),
solve::essential_solver::create_E_21 (essential_solver.cc:188-194), the epipole of match/robust.cc:50-55 with
camera::*::reproject_to_bearing, module::two_view_triangulator::triangulate (two_view_triangulator.cc:45-158, .h:114-137),
solve::triangulator::triangulate (solve/triangulator.h:105-119) and keyframe::triangulate_stereo (data/keyframe.cc:589-640) -- written
from the reference's sources with the numeric contract of DESIGN.md section 5, D10.  A literal serial loop: neighbour after neighbour,
match after match.  Not compiled from the reference (unpinned, like D5-D9).

A key frame is a dict: keypts (n records of plp.KP_DTYPE), bearings (n, 3) f64, x_right (n,) f32, depths (n,) f32, pose (15,) f64
(frame_pose).  Cameras are the dicts of landmark_observe_ref."""
import math

import numpy as np

from landmark_observe_ref import frame_pose, reproject  # noqa: F401  (frame_pose re-exported for the tests)

f32, f64 = np.float32, np.float64
MONOCULAR, STEREO, RGBD = 0, 1, 2
(CREATED, PAIR_SKIPPED, NO_MATCH, NO_PARALLAX, DEPTH, REPROJ_1, REPROJ_2, SCALE, NON_FINITE, INDEX_RANGE) = range(10)
STATUS_NAMES = ("CREATED", "PAIR_SKIPPED", "NO_MATCH", "NO_PARALLAX", "DEPTH", "REPROJ_1", "REPROJ_2", "SCALE", "NON_FINITE", "INDEX_RANGE")
CHI_SQ_2D, CHI_SQ_3D = f32(5.99146), f32(7.81473)

# ---------------------------------------------------------------------------------------------------------------- the null vector (D10)
NULL4_PAIRS = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))
NULL4_SWEEP_LIMIT = 30
NULL4_SKIP_TOL = f64(2.0 ** -100)


def _sq4(U, p, q):
    return ((U[p] * U[q] + U[4 + p] * U[4 + q]) + U[8 + p] * U[8 + q]) + U[12 + p] * U[12 + q]


def null_vector4(A):
    """csrc/null4.hpp in Python: cyclic one-sided Jacobi on the columns of U = A (row-major, 16 values), V = I -> (v [4], sweeps that rotated)"""
    one, zero, two = f64(1.0), f64(0.0), f64(2.0)
    with np.errstate(all="ignore"):
        U = [f64(a) for a in np.asarray(A, np.float64).reshape(16)]
        V = [one if i % 5 == 0 else zero for i in range(16)]
        n = 0
        while n < NULL4_SWEEP_LIMIT:
            rotated = False
            for p, q in NULL4_PAIRS:
                alpha, beta, gamma = _sq4(U, p, p), _sq4(U, q, q), _sq4(U, p, q)
                if not (gamma * gamma > (NULL4_SKIP_TOL * alpha) * beta):
                    continue
                rotated = True
                zeta = (beta - alpha) / (two * gamma)
                root = np.sqrt(one + zeta * zeta)
                t = one / (zeta + root) if zeta >= zero else -one / (root - zeta)
                c = one / np.sqrt(one + t * t)
                s = c * t
                for M in (U, V):
                    for r in range(4):
                        mp, mq = M[4 * r + p], M[4 * r + q]
                        M[4 * r + p] = c * mp - s * mq
                        M[4 * r + q] = s * mp + c * mq
            if not rotated:
                break
            n += 1
        best, nb = 0, _sq4(U, 0, 0)
        for k in (1, 2, 3):
            nk = _sq4(U, k, k)
            if nk < nb:
                best, nb = k, nk
        return [V[4 * r + best] for r in range(4)], n


def null_vector4_svd(A):
    """the same vector from LAPACK: the last right singular vector (numpy.linalg.svd) -> (v [4], 0)"""
    _, _, vt = np.linalg.svd(np.asarray(A, np.float64).reshape(4, 4))
    return [f64(x) for x in vt[3]], 0


# ---------------------------------------------------------------------------------------------------------------- pair geometry
def _norm3(x, y, z):
    return np.sqrt((x * x + y * y) + z * z)


def pair_geometry(cam, setup_type, true_baseline, P1, P2, median_depth_2):
    """per pair (kf1 = cur with pose row P1, kf2 = ngh with P2) -> (skip, epipolar [12] f64, baseline_dist)"""
    with np.errstate(all="ignore"):
        P1, P2 = [f64(v) for v in P1], [f64(v) for v in P2]
        dist = _norm3(P2[12] - P1[12], P2[13] - P1[13], P2[14] - P1[14])
        if setup_type == MONOCULAR:
            skip = bool(dist < f64(0.02) * f64(f32(median_depth_2)))            # :389
        else:
            skip = bool(dist < f64(true_baseline))                              # :397
        # create_E_21(ngh, cur): rot_21 = rot_cur * rot_ngh^T, trans_21 = -rot_21 * trans_ngh + trans_cur, E = skew(trans_21) * rot_21
        R = [[(P1[3 * i] * P2[3 * k] + P1[3 * i + 1] * P2[3 * k + 1]) + P1[3 * i + 2] * P2[3 * k + 2] for k in range(3)] for i in range(3)]
        tr = [(((-R[i][0]) * P2[9] + (-R[i][1]) * P2[10]) + (-R[i][2]) * P2[11]) + P1[9 + i] for i in range(3)]
        z = f64(0.0)
        S = [[z, -tr[2], tr[1]], [tr[2], z, -tr[0]], [-tr[1], tr[0], z]]
        E = [(S[i][0] * R[0][k] + S[i][1] * R[1][k]) + S[i][2] * R[2][k] for i in range(3) for k in range(3)]
        # the epipole: reproject_to_bearing(rot_2w, trans_2w, cam_center_1), its return value ignored (robust.cc:55)
        x, y, zz = P1[12], P1[13], P1[14]
        b = [((P2[3 * r] * x + P2[3 * r + 1] * y) + P2[3 * r + 2] * zz) + P2[9 + r] for r in range(3)]
        if cam["model"] == "equirectangular" or not (b[2] <= 0.0):             # perspective / fisheye: z <= 0 returns before normalize()
            sq = (b[0] * b[0] + b[1] * b[1]) + b[2] * b[2]
            if sq > 0.0:
                s = np.sqrt(sq)
                b = [b[0] / s, b[1] / s, b[2] / s]
        return skip, np.array(E + b, np.float64), dist


# ---------------------------------------------------------------------------------------------------------------- triangulate
def _rel_gap(a, b):
    m = max(abs(float(a)), abs(float(b)))
    return abs(float(a) - float(b)) / m if m > 0 else 0.0


def cos_parallax_thr(deg):
    """cos_rays_parallax_thr_: the float of cos(thr * M_PI / 180.0), thr a float (.cc:42, .h:110)"""
    return f32(math.cos(float(f32(deg)) * math.pi / 180.0))


def solve_matrix(b1, b2, P1, P2):
    """the 4 x 4 matrix of solve::triangulator::triangulate, row-major: rows from the bearings and cam_pose_cw = (rot_cw | trans_cw)"""
    def row(P, r):
        return [P[3 * r], P[3 * r + 1], P[3 * r + 2], P[9 + r]]
    A = []
    for b, P in ((b1, P1), (b2, P2)):
        r0, r1, r2 = row(P, 0), row(P, 1), row(P, 2)
        A += [b[0] * r2[c] - b[2] * r0[c] for c in range(4)]
        A += [b[1] * r2[c] - b[2] * r1[c] for c in range(4)]
    return A


def _triangulate_stereo(cam, P, kp, depth):
    """keyframe::triangulate_stereo: the float unproj_x / unproj_y, rot_wc * pos_c + cam_center; depth <= 0: the zero vector"""
    if not (0.0 < float(depth)):
        return [f64(0.0)] * 3
    fx_inv, fy_inv = f64(1.0) / f64(cam["fx"]), f64(1.0) / f64(cam["fy"])
    ux = f32(((f64(f32(kp["x"])) - f64(cam["cx"])) * f64(depth)) * fx_inv)
    uy = f32(((f64(f32(kp["y"])) - f64(cam["cy"])) * f64(depth)) * fy_inv)
    c = [f64(ux), f64(uy), f64(depth)]
    return [((P[i] * c[0] + P[3 + i] * c[1]) + P[6 + i] * c[2]) + P[12 + i] for i in range(3)]


def triangulate(cam, setup_type, true_baseline, scale_factors, level_sigma_sq, scale_factor, cos_thr, kf1, kf2, j, t, null=null_vector4,
                gaps=None, info=None):
    """two_view_triangulator::triangulate(idx_1 = j, idx_2 = t) -> (status, pos_w [3] or None).  null: the null-vector routine.
    gaps: a list that receives (kind, relative gap) of every strict comparison one side of which depends on the null vector or on a libm
    result (cos / atan2 of the stereo parallax, asin / atan2 of the equirectangular reprojection).  info: a dict that receives branch
    (1 two cameras, 2 / 3 stereo of key frame 1 / 2), sweeps and the matrix."""
    with np.errstate(all="ignore"):
        k1, k2 = kf1["keypts"][j], kf2["keypts"][t]
        P1, P2 = [f64(v) for v in kf1["pose"]], [f64(v) for v in kf2["pose"]]
        equi = cam["model"] == "equirectangular"
        stereo_setup = setup_type != MONOCULAR and not equi      # a monocular setup holds -1 in every stereo_x_right_: not read
        xr1 = f32(kf1["x_right"][j]) if stereo_setup else f32(-1.0)
        xr2 = f32(kf2["x_right"][t]) if stereo_setup else f32(-1.0)
        s1, s2 = bool(f32(0) <= xr1), bool(f32(0) <= xr2)
        b1, b2 = [f64(v) for v in kf1["bearings"][j]], [f64(v) for v in kf2["bearings"][t]]
        w1 = [(P1[i] * b1[0] + P1[3 + i] * b1[1]) + P1[6 + i] * b1[2] for i in range(3)]
        w2 = [(P2[i] * b2[0] + P2[3 + i] * b2[1]) + P2[6 + i] * b2[2] for i in range(3)]
        cr = (w1[0] * w2[0] + w1[1] * w2[1]) + w1[2] * w2[2]
        half = f64(true_baseline) / f64(2.0)
        c1 = c2 = f64(2.0)
        d1 = d2 = f32(0.0)
        if s1:
            d1 = f32(kf1["depths"][j])
            c1 = f64(math.cos(2.0 * math.atan2(float(half), float(d1))))
        if s2:
            d2 = f32(kf2["depths"][t])
            c2 = f64(math.cos(2.0 * math.atan2(float(half), float(d2))))
        cs = c2 if c2 < c1 else c1                              # std::min
        if not (s1 or s2):
            two = bool(f64(0.0) < cr and cr < f64(cos_thr))
        else:
            two = bool(f64(0.0) < cr and cr < cs)
            if gaps is not None and f64(0.0) < cr:
                gaps.append(("rays", _rel_gap(cr, cs)))
        dep = two or equi                                       # what follows depends on the null vector or on asin / atan2
        if two:
            A = solve_matrix(b1, b2, P1, P2)
            v, sweeps = null(A)
            if info is not None:
                info.update(branch=1, sweeps=sweeps, matrix=A)
            if v[3] == 0.0:
                return NON_FINITE, None
            pos = [v[0] / v[3], v[1] / v[3], v[2] / v[3]]
        else:
            if gaps is not None and (s1 or s2):
                gaps.append(("stereo_equal_inputs" if (s1 and s2 and d1 == d2) else "stereo", _rel_gap(c1, c2)))
            if s1 and c1 < c2:
                pos = _triangulate_stereo(cam, P1, k1, d1)
                if info is not None:
                    info.update(branch=2)
            elif s2 and c2 < c1:
                pos = _triangulate_stereo(cam, P2, k2, d2)
                if info is not None:
                    info.update(branch=3)
            else:
                return NO_PARALLAX, None
        if not np.all(np.isfinite(pos)):
            return NON_FINITE, None

        def note(kind, a, b):
            if gaps is not None and dep:
                gaps.append((kind, _rel_gap(a, b)))
        if not equi:                                            # check_depth_is_positive
            for P in (P1, P2):
                rot = (P[6] * pos[0] + P[7] * pos[1]) + P[8] * pos[2]
                note("depth", rot, -P[11])
                if not (0 < rot + P[11]):
                    return DEPTH, None
        oc1 = min(max(int(k1["octave"]), 0), len(scale_factors) - 1)
        oc2 = min(max(int(k2["octave"]), 0), len(scale_factors) - 1)
        for P, kp, xr, st, oc, fail in ((P1, k1, xr1, s1, oc1, REPROJ_1), (P2, k2, xr2, s2, oc2, REPROJ_2)):
            sig = f32(level_sigma_sq[oc])
            wrote, _, u, v_, xri = reproject(cam, (0, 0, 0, 0), P, *pos)
            if not wrote:                                       # z <= 0: not reachable behind check_depth_is_positive
                return fail, None
            ex, ey = f64(u) - f64(f32(kp["x"])), f64(v_) - f64(f32(kp["y"]))   # Vec2_t - cv::Point2f: the key point widened
            sq = ex * ex + ey * ey
            if st:
                exr = f32(f32(xri) - xr)
                sq = sq + f64(f32(exr * exr))
                lim = f64(f32(CHI_SQ_3D * sig))
            else:
                lim = f64(f32(CHI_SQ_2D * sig))
            if not np.isfinite(sq):
                return NON_FINITE, None
            note("reproj", lim, sq)
            if lim < sq:
                return fail, None
        l1 = _norm3(pos[0] - P1[12], pos[1] - P1[13], pos[2] - P1[14])
        l2 = _norm3(pos[0] - P2[12], pos[1] - P2[13], pos[2] - P2[14])
        if l1 == 0 or l2 == 0:
            return SCALE, None
        ratio_dists = l2 / l1
        ratio_octave = f64(f32(f32(scale_factors[oc1]) / f32(scale_factors[oc2])))
        ratio_factor = f64(f32(f32(2.0) * f32(scale_factor)))   # 2.0f * max(scale_factor_, scale_factor_)
        note("scale", ratio_octave / ratio_dists, ratio_factor)
        if not (ratio_octave / ratio_dists < ratio_factor):
            return SCALE, None
        note("scale", ratio_dists / ratio_octave, ratio_factor)
        if not (ratio_dists / ratio_octave < ratio_factor):
            return SCALE, None
        return CREATED, np.array(pos, np.float64)


# ---------------------------------------------------------------------------------------------------------------- the loop
def triangulate_pair(cam, setup_type, true_baseline, scale_factors, level_sigma_sq, scale_factor, rays_parallax_deg_thr, kf1, kf2, match_q,
                     q_feature=None, m_cap=None, pair_skip=False, occupied_1=None, occupied_2=None, null=null_vector4, gaps=None, infos=None):
    """the loop over the matches of triangulate_with_two_keyframes (:441-478) in the array form of plp_triangulate_keypoint_pairs_*:
    match_q [n2] = the query slot per key point of key frame 2, q_feature [m_cap] = key-point index per query slot (None: identity).
    Returns (idx_1 [n2] i32, pos_w [n2, 3], status [n2] u8) -- for a skipped pair only the status means something -- and updates
    occupied_1 / occupied_2 (arrays over the key points of kf1 / kf2) in place as add_landmark does."""
    n1, n2 = len(kf1["keypts"]), len(kf2["keypts"])
    idx = np.full(n2, -1, np.int32); pos = np.zeros((n2, 3), np.float64); st = np.zeros(n2, np.uint8)
    if pair_skip:
        st[:] = PAIR_SKIPPED
        return idx, pos, st
    if m_cap is None:
        m_cap = n1 if q_feature is None else len(q_feature)
    cos_thr = cos_parallax_thr(rays_parallax_deg_thr)
    for t in range(n2):
        q = int(match_q[t])
        if q < 0 or q >= m_cap:
            st[t] = NO_MATCH
            continue
        j = q if q_feature is None else int(q_feature[q])
        idx[t] = j
        if j < 0 or j >= n1:
            st[t] = INDEX_RANGE
            continue
        info = {} if infos is not None else None
        s, p = triangulate(cam, setup_type, true_baseline, scale_factors, level_sigma_sq, scale_factor, cos_thr, kf1, kf2, j, t, null, gaps, info)
        st[t] = s
        if infos is not None:
            infos.append((t, j, s, info))
        if s == CREATED:
            pos[t] = p
            if occupied_1 is not None:
                occupied_1[j] = 1
            if occupied_2 is not None:
                occupied_2[t] = 1
    return idx, pos, st
