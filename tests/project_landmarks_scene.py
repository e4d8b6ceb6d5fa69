"""Scenes for the fuse / Sim3 / relocalisation query tests (plp_project_landmark[_line]s_*).

Points reuse point_scene of tests/test_gpu_landmark_observe.py (kept 49 %, skipped 10 %, not in image 22 %, distance 9 %, ray 10 % on the
perspective and fisheye cameras; the equirectangular one never leaves the image).  Its line_scene never has both end points out of the image
and never fails the midpoint distance range, so the line loops get a generator of their own with those kinds added, and with more end points
behind the camera of lines that are kept (the carried end points of D6).  Measured with the restatement on 4 000 slots, seed 7, perspective
and fisheye: kept 50 % (end-point distances) / 61 % (midpoint distance), skipped 10 %, both end points out 8 %, midpoint out 10 %, distance
22 % / 11 %, kept with a carried end point 22 %; tests/test_project_landmarks_cpu.py holds every reachable status to at least 2 %."""
import numpy as np

import landmark_observe_ref as R
import project_landmarks_ref as PR
from test_gpu_landmark_observe import back_project, point_scene, random_pose, rotation, to_world   # noqa: F401  (re-exported)

f32 = np.float32


def whole_image(cm):
    """camera::base img_bounds_ of a camera without distortion: the image itself"""
    return np.array([0.0, cm.cols, 0.0, cm.rows], np.float32)


def scaled_pose(rng):
    """one pass of match_keyframes_mutually: (row for the device: the scaled matrix s R, its translation, cam_center ignored (0);
    the unscaled frame_pose (R, t / s) the scene is generated with; s).  The reprojection does not depend on s, the camera-frame
    distance is s times the unscaled one."""
    s = float(f32(rng.uniform(0.5, 2.0)))
    Rm, t = rotation(rng), rng.normal(size=3)
    row = np.concatenate([(s * Rm).ravel(), t, np.zeros(3)])
    return row, R.frame_pose(Rm, t / s), s


def point_scene_camera(rng, cm, bounds, P_unscaled, s, m, lsf):
    """point_scene for PLP_PROJECT_DIST_CAMERA with a scaled pose: the valid-distance range follows the scale"""
    pos, nm, mn, mx, skip = point_scene(rng, cm, bounds, P_unscaled, m, lsf)
    return pos, nm, (mn * f32(s)).astype(np.float32), (mx * f32(s)).astype(np.float32), skip


def line_scene(rng, cm, bounds, P, m):
    """m line landmarks for the two line loops: both end points in; one out with the midpoint in / out; both out; one end behind the camera of
    a line whose midpoint is in front (kept, the end point carried); the midpoint distance out of range; the range at the midpoint distance
    +- 1 float ulp (the f64 comparison against the float bound); an end-point distance out of range with the midpoint's in (the two
    line_dist_modes differ); skipped ones"""
    b = [float(t) for t in bounds]
    cc = P[12:15]
    pos = np.zeros((m, 6)); mn = np.zeros(m, np.float32); mx = np.zeros(m, np.float32)
    for j in range(m):
        kind = int(rng.integers(0, 12))
        z0, z1 = float(rng.uniform(0.5, 15)), float(rng.uniform(0.5, 15))
        u0, v0 = rng.uniform(b[0], b[1]), rng.uniform(b[2], b[3])
        u1, v1 = rng.uniform(b[0], b[1]), rng.uniform(b[2], b[3])
        w = b[1] - b[0]
        if kind == 2:   # end point out of the image, midpoint likely in
            u1 = b[1] + w * float(rng.uniform(0.01, 0.6))
        if kind == 3:   # start point far out: midpoint out too
            u0 = b[0] - w * float(rng.uniform(2.0, 5.0))
        if kind == 4:   # both end points out, on the same side
            side = 1.0 if rng.integers(0, 2) else -1.0
            u0 = (b[1] if side > 0 else b[0]) + side * w * float(rng.uniform(0.05, 2.0))
            u1 = (b[1] if side > 0 else b[0]) + side * w * float(rng.uniform(0.05, 2.0))
        p0 = back_project(cm, bounds, P, u0, v0, z0); p1 = back_project(cm, bounds, P, u1, v1, z1)
        if kind in (5, 6, 7):   # one end just behind the camera, the other well in front: the midpoint stays in front
            zf = float(rng.uniform(3.0, 15.0))
            front = back_project(cm, bounds, P, rng.uniform(0.7 * b[0] + 0.3 * b[1], 0.3 * b[0] + 0.7 * b[1]),
                                 rng.uniform(0.7 * b[2] + 0.3 * b[3], 0.3 * b[2] + 0.7 * b[3]), zf)
            back = to_world(P, np.array([rng.normal() * 0.2, rng.normal() * 0.2, -float(rng.uniform(0.05, 1.0))]))
            p0, p1 = (front, back) if kind != 6 else (back, front)
        pos[j, :3], pos[j, 3:] = p0, p1
        d_mp = float(np.linalg.norm(0.5 * (p0 + p1) - cc))
        d_sp, d_ep = float(np.linalg.norm(p0 - cc)), float(np.linalg.norm(p1 - cc))
        lo, hi = min(d_sp, d_ep, d_mp), max(d_sp, d_ep, d_mp)
        mn[j] = f32(lo * rng.uniform(0.3, 1.1)); mx[j] = f32(hi * rng.uniform(0.9, 4.0))
        if kind == 8:   # the midpoint distance out of range
            if rng.integers(0, 2): mx[j] = f32(d_mp * rng.uniform(0.2, 0.8))
            else: mn[j] = f32(d_mp * rng.uniform(1.3, 3.0))
        if kind == 9:   # 0.8 x min / 1.2 x max at the midpoint distance, +- 1 ulp: the f64 distance against the float bound
            fd = f32(d_mp)
            if rng.integers(0, 2):
                mn[j] = np.nextafter(f32(float(fd) / 0.8), f32(rng.choice([-np.inf, np.inf]))) if rng.integers(0, 2) else f32(float(fd) / 0.8)
                mx[j] = f32(hi * 4.0)
            else:
                mx[j] = np.nextafter(f32(float(fd) / 1.2), f32(rng.choice([-np.inf, np.inf]))) if rng.integers(0, 2) else f32(float(fd) / 1.2)
                mn[j] = f32(lo * 0.1)
        if kind == 10:   # an end point out of range, the midpoint in: ENDPOINTS rejects, MIDPOINT keeps
            mn[j] = f32(d_mp * 0.5); mx[j] = f32(0.5 * (d_mp + hi) / 1.2) if hi > d_mp * 1.05 else f32(hi * 2.0)
    skip = (rng.uniform(size=m) < 0.1).astype(np.uint8)
    return pos, mn, mx, skip


def carried_kept_share(cam, bounds, P, pos, skip, want):
    """share of the slots that are kept with an end point the reference left unwritten (z <= 0): what D6 defines"""
    n = 0
    for j in np.flatnonzero(want["valid"]):
        ws = R.reproject(cam, bounds, P, *pos[j, :3])[0]
        we = R.reproject(cam, bounds, P, *pos[j, 3:])[0]
        n += not (ws and we)
    return n / max(len(pos), 1)


def ref_cam(cm):
    return {"model": {0: "perspective", 1: "fisheye", 2: "equirectangular"}[cm.model], "cols": cm.cols, "rows": cm.rows,
            **{k: getattr(cm, k) for k in ("fx", "fy", "cx", "cy", "focal_x_baseline")}}
