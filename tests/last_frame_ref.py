"""CPU restatement of the last-frame query preparation (plp_project_last_frame_* / plp_project_last_frame_lines_*): the loops of
projection::match_current_and_last_frames (match/projection.cc:214-358) and match_current_and_last_frames_line (:361-527) up to their
searches, with the reprojection of tests/landmark_observe_ref.py and the end points of D6.

Cameras, bounds and pose rows as in landmark_observe_ref: a pose is the 15-double row of frame_pose (rot_cw row-major, trans_cw, cam_center)."""
import numpy as np

from landmark_observe_ref import frame_pose, reproject  # noqa: F401  (frame_pose re-exported for the tests)

f32 = np.float32
MONOCULAR, STEREO, RGBD = 0, 1, 2


def trans_lc_z(pose_curr, pose_last):
    """trans_lc(2) of projection.cc:219-227: rot_lw * trans_wc + trans_lw with trans_wc = -rot_cw^T trans_cw = the current frame's cam_center_"""
    P = [float(v) for v in pose_curr]
    L = [float(v) for v in pose_last]
    return ((L[6] * P[12] + L[7] * P[13]) + L[8] * P[14]) + L[11]


def direction(setup_type, true_baseline, pose_curr, pose_last):
    """0 neither, 1 assume_forward, 2 assume_backward (:229-236); a monocular setup is always 0"""
    if setup_type == MONOCULAR:
        return 0
    z = trans_lc_z(pose_curr, pose_last)
    tb = float(true_baseline)
    if z > tb:
        return 1
    if -z > tb:
        return 2
    return 0


def project_points(cam, bounds, P, pos_w, octave, angle, skip):
    """one problem: dict(reproj [m,2] f32, x_right [m] f32, level [m] i32, angle [m] f32, valid [m] u8, num_valid); invalid slots hold 0"""
    m = len(pos_w)
    out = dict(reproj=np.zeros((m, 2), np.float32), x_right=np.zeros(m, np.float32), level=np.zeros(m, np.int32), angle=np.zeros(m, np.float32),
               valid=np.zeros(m, np.uint8))
    for j in range(m):
        if skip is not None and skip[j]:                       # !lm || outlier_flags_[idx_last]
            continue
        _, inside, u, v, xr = reproject(cam, bounds, P, *pos_w[j])
        if not inside:
            continue
        out["valid"][j] = 1
        out["reproj"][j] = (f32(u), f32(v))
        out["x_right"][j] = f32(xr)
        out["level"][j] = int(octave[j])
        out["angle"][j] = f32(angle[j])
    out["num_valid"] = int(out["valid"].sum())
    return out


def project_lines(cam, bounds, P, pos_w, octave, skip):
    """one problem, match_current_and_last_frames_line up to its search (:395-440) with D6: reproj_sp / reproj_ep and x_right_sp / x_right_ep
    of every slot are the values after its turn, an end point with z <= 0 keeping those of the most recent earlier non-skipped slot whose matching
    end point was written, (0, 0) / 0 before the first one.  dict(reproj_sp, reproj_ep [m,2] f32, x_right_sp, x_right_ep [m] f32, level [m] i32
    (0 where invalid), valid [m] u8, num_valid)"""
    m = len(pos_w)
    out = dict(reproj_sp=np.zeros((m, 2), np.float32), reproj_ep=np.zeros((m, 2), np.float32), x_right_sp=np.zeros(m, np.float32),
               x_right_ep=np.zeros(m, np.float32), level=np.zeros(m, np.int32), valid=np.zeros(m, np.uint8))
    sp_t, ep_t = (0.0, 0.0, 0.0), (0.0, 0.0, 0.0)
    for j in range(m):
        if not (skip is not None and skip[j]):
            p = [float(t) for t in pos_w[j]]
            ws, in_s, us, vs, xs = reproject(cam, bounds, P, *p[:3])
            we, in_e, ue, ve, xe = reproject(cam, bounds, P, *p[3:])
            if ws:
                sp_t = (us, vs, xs)
            if we:
                ep_t = (ue, ve, xe)
            ok = in_s or in_e
            if ok and not (in_s and in_e):                     # partial occlusion: the midpoint decides
                ok = reproject(cam, bounds, P, 0.5 * (p[0] + p[3]), 0.5 * (p[1] + p[4]), 0.5 * (p[2] + p[5]))[1]
            if ok:
                out["level"][j] = int(octave[j])
            out["valid"][j] = 1 if ok else 0
        out["reproj_sp"][j] = (f32(sp_t[0]), f32(sp_t[1]))
        out["reproj_ep"][j] = (f32(ep_t[0]), f32(ep_t[1]))
        out["x_right_sp"][j] = f32(sp_t[2])
        out["x_right_ep"][j] = f32(ep_t[2])
    out["num_valid"] = int(out["valid"].sum())
    return out


def d6_end_point_used(cam, bounds, P, pos_w, skip):
    """slots whose stored end point is a D6 value: valid lines with an end point behind the camera (perspective / fisheye only)"""
    used = np.zeros(len(pos_w), bool)
    for j in range(len(pos_w)):
        if skip is not None and skip[j]:
            continue
        p = [float(t) for t in pos_w[j]]
        ws, in_s, *_ = reproject(cam, bounds, P, *p[:3])
        we, in_e, *_ = reproject(cam, bounds, P, *p[3:])
        if (in_s or in_e) and not (ws and we):
            used[j] = reproject(cam, bounds, P, 0.5 * (p[0] + p[3]), 0.5 * (p[1] + p[4]), 0.5 * (p[2] + p[5]))[1]
    return used
