"""CPU restatement of the seven matcher loops of the reference up to their search (plp_project_landmarks_* / plp_project_landmark_lines_*):
  fuse::replace_duplication (match/fuse.cc:169-236), replace_duplication_line (:335-420), detect_duplication (:40-111),
  projection::match_by_Sim3_transform (match/projection.cc:781-848), match_keyframes_mutually (:894-993, :1029-1087),
  match_frame_and_keyframe (:529-593), match_frame_and_keyframe_line (:648-743).
Plain Python f64 per landmark in the reference's order, built on landmark_observe_ref's reproject,
predict_scale_level and d5_logf; float rounding is spelled out with numpy.float32 where the reference stores or computes in float.

A pose is the 15-double row of plp_project_args: the matrix handed to reproject_to_image row-major, its translation, cam_center."""
import math

import numpy as np

import landmark_observe_ref as R

f32 = np.float32
KEPT, SKIPPED, NOT_IN_IMAGE, MIDPOINT_OUT, DISTANCE, RAY = range(6)
DIST_CENTER, DIST_CAMERA = 0, 1
LINE_ENDPOINTS, LINE_MIDPOINT = 0, 1

# the flag combinations the reference's loops use: name -> (lines, dist_mode, ray_test, line_dist_mode)
LOOPS = {
    "replace_duplication": (False, DIST_CENTER, True, 0),
    "detect_duplication": (False, DIST_CENTER, True, 0),
    "match_by_Sim3_transform": (False, DIST_CENTER, True, 0),
    "match_keyframes_mutually": (False, DIST_CAMERA, False, 0),
    "match_frame_and_keyframe": (False, DIST_CENTER, False, 0),
    "replace_duplication_line": (True, DIST_CENTER, False, LINE_ENDPOINTS),
    "match_frame_and_keyframe_line": (True, DIST_CENTER, False, LINE_MIDPOINT),
}


def _norm(dx, dy, dz):
    return math.sqrt((dx * dx + dy * dy) + dz * dz)


def _mat3(m):
    return [[float(v) for v in row] for row in np.asarray(m, np.float64).reshape(3, 3)]


def _mul33(A, B):
    return [[(A[i][0] * B[0][j] + A[i][1] * B[1][j]) + A[i][2] * B[2][j] for j in range(3)] for i in range(3)]


def _mul3v(A, v):
    return [(A[i][0] * v[0] + A[i][1] * v[1]) + A[i][2] * v[2] for i in range(3)]


def sim3_pose(Sim3_cw):
    """fuse.cc:46-50 / projection.cc:787-791"""
    S = [[float(v) for v in row] for row in np.asarray(Sim3_cw, np.float64).reshape(4, 4)]
    s_cw = math.sqrt((S[0][0] * S[0][0] + S[0][1] * S[0][1]) + S[0][2] * S[0][2])
    rot = [[S[i][j] / s_cw for j in range(3)] for i in range(3)]
    trans = [S[i][3] / s_cw for i in range(3)]
    return R.frame_pose(rot, trans)


def mutual_poses(s_12, rot_12, trans_12, rot_1w, trans_1w, rot_2w, trans_2w):
    """projection.cc:906-908, 941-942, 1035-1036: row 0 = s_rot_21w, trans_21w; row 1 = s_rot_12w, trans_12w; entries 12-14 are 0"""
    s = float(f32(s_12))
    R12, R1w, R2w = _mat3(rot_12), _mat3(rot_1w), _mat3(rot_2w)
    t12, t1w, t2w = ([float(v) for v in np.asarray(t, np.float64).reshape(3)] for t in (trans_12, trans_1w, trans_2w))
    inv = 1.0 / s
    s_rot_12 = [[s * R12[i][j] for j in range(3)] for i in range(3)]
    s_rot_21 = [[inv * R12[j][i] for j in range(3)] for i in range(3)]
    trans_21 = _mul3v([[-v for v in row] for row in s_rot_21], t12)
    s_rot_21w = _mul33(s_rot_21, R1w)
    trans_21w = [a + b for a, b in zip(_mul3v(s_rot_21, t1w), trans_21)]
    s_rot_12w = _mul33(s_rot_12, R2w)
    trans_12w = [a + b for a, b in zip(_mul3v(s_rot_12, t2w), t12)]
    flat = lambda M: M[0] + M[1] + M[2]
    return np.array([flat(s_rot_21w) + trans_21w + [0.0] * 3, flat(s_rot_12w) + trans_12w + [0.0] * 3], np.float64)


def project_point(cam, bounds, P, pos, normal, min_valid, max_valid, dist_mode, ray_test, log_sf, num_levels, logf=R.d5_logf):
    """one iteration of a point loop after its skip tests -> (status, u, v, x_right, level)"""
    P = [float(v) for v in P]
    x, y, z = (float(v) for v in pos)
    _, inside, u, v, xr = R.reproject(cam, bounds, P, x, y, z)
    if not inside:
        return NOT_IN_IMAGE, u, v, xr, None
    if dist_mode == DIST_CAMERA:                                  # pos_2 = s_rot_21w * pos_w + trans_21w; pos_2.norm() (projection.cc:962, 976)
        dx = ((P[0] * x + P[1] * y) + P[2] * z) + P[9]
        dy = ((P[3] * x + P[4] * y) + P[5] * z) + P[10]
        dz = ((P[6] * x + P[7] * y) + P[8] * z) + P[11]
    else:                                                         # cam_to_lm_vec = pos_w - cam_center
        dx, dy, dz = x - P[12], y - P[13], z - P[14]
    dist = _norm(dx, dy, dz)
    max_d = float(f32(1.3 * float(f32(max_valid))))               # float get_max_valid_distance(), widened by the f64 comparison
    min_d = float(f32(0.7 * float(f32(min_valid))))
    if dist < min_d or max_d < dist:
        return DISTANCE, u, v, xr, None
    if ray_test:
        n = [float(t) for t in normal]
        if ((dx * n[0] + dy * n[1]) + dz * n[2]) < 0.5 * dist:    # no division, 0.5 a double
            return RAY, u, v, xr, None
    return KEPT, u, v, xr, R.predict_scale_level(max_valid, f32(dist), log_sf, num_levels, logf)


def project_points(cam, bounds, P, pos_w, normals, min_valid, max_valid, skip, dist_mode, ray_test, log_sf, num_levels, logf=R.d5_logf):
    """one problem: dict(reproj_d [m,2] f64, reproj [m,2] f32, x_right [m] f32, level [m] i32, valid [m] u8, status [m] u8, num_valid);
    reproj_d / reproj / x_right / level of invalid slots hold 0"""
    m = len(pos_w)
    out = dict(reproj_d=np.zeros((m, 2), np.float64), reproj=np.zeros((m, 2), np.float32), x_right=np.zeros(m, np.float32),
               level=np.zeros(m, np.int32), valid=np.zeros(m, np.uint8), status=np.zeros(m, np.uint8))
    for j in range(m):
        if skip is not None and skip[j]:
            out["status"][j] = SKIPPED
            continue
        st, u, v, xr, lvl = project_point(cam, bounds, P, pos_w[j], None if normals is None else normals[j], min_valid[j], max_valid[j],
                                          dist_mode, ray_test, log_sf, num_levels, logf)
        out["status"][j] = st
        if st == KEPT:
            out["valid"][j] = 1
            out["reproj_d"][j] = (u, v)
            out["reproj"][j] = (f32(u), f32(v))
            out["x_right"][j] = f32(xr)
            out["level"][j] = lvl
    out["num_valid"] = int(out["valid"].sum())
    return out


def project_lines(cam, bounds, P, pos_w, min_valid, max_valid, skip, line_dist_mode, log_sf, num_levels, logf=R.d5_logf):
    """one problem of a line loop.  reproj_sp / reproj_ep and x_right_sp / x_right_ep are declared inside the reference's loop and left
    unwritten for z <= 0; as D6 defines them: the values of the most recent earlier non-skipped slot whose matching end point was written,
    (0, 0) / 0 before the first.  dict(reproj_sp_d, reproj_ep_d [m,2] f64, reproj_sp, reproj_ep [m,2] f32, x_right_sp, x_right_ep [m] f32
    (all: the temporaries after every slot's turn), level [m] i32 (0 where invalid), valid, status [m] u8, num_valid)"""
    m = len(pos_w)
    P = [float(v) for v in P]
    out = dict(reproj_sp_d=np.zeros((m, 2), np.float64), reproj_ep_d=np.zeros((m, 2), np.float64), reproj_sp=np.zeros((m, 2), np.float32),
               reproj_ep=np.zeros((m, 2), np.float32), x_right_sp=np.zeros(m, np.float32), x_right_ep=np.zeros(m, np.float32),
               level=np.zeros(m, np.int32), valid=np.zeros(m, np.uint8), status=np.zeros(m, np.uint8))
    sp_t, ep_t = (0.0, 0.0, 0.0), (0.0, 0.0, 0.0)
    for j in range(m):
        if skip is not None and skip[j]:
            st = SKIPPED
        else:
            p = [float(t) for t in pos_w[j]]
            ws, in_s, us, vs, xs = R.reproject(cam, bounds, P, *p[:3])
            we, in_e, ue, ve, xe = R.reproject(cam, bounds, P, *p[3:])
            if ws:
                sp_t = (us, vs, xs)
            if we:
                ep_t = (ue, ve, xe)
            mid = (0.5 * (p[0] + p[3]), 0.5 * (p[1] + p[4]), 0.5 * (p[2] + p[5]))
            st = KEPT
            if not in_s and not in_e:
                st = NOT_IN_IMAGE
            elif not (in_s and in_e) and not R.reproject(cam, bounds, P, *mid)[1]:
                st = MIDPOINT_OUT
            if st == KEPT:
                max_d = float(f32(1.2 * float(f32(max_valid[j]))))   # Line::get_max_valid_distance (landmark_line.cc:360-364)
                min_d = float(f32(0.8 * float(f32(min_valid[j]))))
                d_mp = _norm(mid[0] - P[12], mid[1] - P[13], mid[2] - P[14])
                if line_dist_mode == LINE_ENDPOINTS:               # fuse.cc:398-411
                    d_sp = _norm(p[0] - P[12], p[1] - P[13], p[2] - P[14])
                    d_ep = _norm(p[3] - P[12], p[4] - P[13], p[5] - P[14])
                    gone = d_sp < min_d or max_d < d_sp or d_ep < min_d or max_d < d_ep
                else:                                              # projection.cc:722-730
                    gone = d_mp < min_d or max_d < d_mp
                if gone:
                    st = DISTANCE
                else:
                    out["level"][j] = R.predict_scale_level(max_valid[j], f32(d_mp), log_sf, num_levels, logf)
                    out["valid"][j] = 1
        out["status"][j] = st
        out["reproj_sp_d"][j] = sp_t[:2]; out["reproj_ep_d"][j] = ep_t[:2]
        out["reproj_sp"][j] = (f32(sp_t[0]), f32(sp_t[1])); out["reproj_ep"][j] = (f32(ep_t[0]), f32(ep_t[1]))
        out["x_right_sp"][j] = f32(sp_t[2]); out["x_right_ep"][j] = f32(ep_t[2])
    out["num_valid"] = int(out["valid"].sum())
    return out


def status_shares(status):
    """share of every status among the slots, as a list of six"""
    s = np.asarray(status).ravel()
    return [float((s == k).mean()) for k in range(6)]


def reachable(model, lines, ray_test):
    """the statuses a camera model can reach: the equirectangular model never leaves the image"""
    if lines:
        return [KEPT, SKIPPED, DISTANCE] + ([] if model == "equirectangular" else [NOT_IN_IMAGE, MIDPOINT_OUT])
    return [KEPT, SKIPPED, DISTANCE] + ([RAY] if ray_test else []) + ([] if model == "equirectangular" else [NOT_IN_IMAGE])


def assert_coverage(model, lines, ray_test, status, floor=0.02):
    """every status the camera model can reach occurs in at least 2 % of the slots: a scene cannot go quiet"""
    sh = status_shares(status)
    for k in reachable(model, lines, ray_test):
        assert sh[k] >= floor, (model, "lines" if lines else "points", k, sh)
    return sh
