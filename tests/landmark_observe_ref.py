"""CPU restatement of the local-landmark visibility tests of the reference (plp_observe_landmarks_* / plp_observe_landmark_lines_*):
tracking_module::search_local_landmarks[_line] (tracking_module.cc:908-1064) -> frame::can_observe / can_observe_line (data/frame.cc:797-878)
with camera::*::reproject_to_image.  Plain Python f64 per landmark in the reference's order; float rounding is spelled
out with numpy.float32 where the reference stores or computes in float; asin / atan2 / log are math's (glibc).

Cameras are dicts with the plp_camera_model fields the step reads: model ("perspective" | "fisheye" | "equirectangular"), cols, rows, fx, fy,
cx, cy, focal_x_baseline.  A pose is the 15-double row of plp_observe_args (plp.frame_pose): rot_cw row-major, trans_cw, cam_center."""
import ctypes
import math

import numpy as np

f32 = np.float32
INT_MIN = -2 ** 31


def frame_pose(rot_cw, trans_cw):
    """frame::update_pose_params (frame.cc:745-751): cam_center_ = -rot_cw_^T trans_cw_, each coefficient a left-to-right sum"""
    R = [[float(v) for v in row] for row in np.asarray(rot_cw, np.float64).reshape(3, 3)]
    t = [float(v) for v in np.asarray(trans_cw, np.float64).reshape(3)]
    cc = [((-R[0][i]) * t[0] + (-R[1][i]) * t[1]) + (-R[2][i]) * t[2] for i in range(3)]
    return np.array(R[0] + R[1] + R[2] + t + cc, np.float64)


def reproject(cam, bounds, P, x, y, z):
    """camera::*::reproject_to_image -> (wrote, in_image, u, v, x_right); wrote = the function assigned reproj / x_right"""
    P = [float(v) for v in P]
    x, y, z = float(x), float(y), float(z)
    xc = ((P[0] * x + P[1] * y) + P[2] * z) + P[9]
    yc = ((P[3] * x + P[4] * y) + P[5] * z) + P[10]
    zc = ((P[6] * x + P[7] * y) + P[8] * z) + P[11]
    if cam["model"] == "equirectangular":                      # equirectangular.cc:104-119
        sq = (xc * xc + yc * yc) + zc * zc
        bx, by, bz = xc, yc, zc
        if sq > 0.0:                                           # Eigen 3.3 normalized(): a zero vector stays zero
            s = math.sqrt(sq)
            bx, by, bz = xc / s, yc / s, zc / s
        lat = -(math.asin(by) if -1.0 <= by <= 1.0 else math.nan)
        lon = math.atan2(bx, bz)
        u = float(cam["cols"]) * (0.5 + lon / (2.0 * math.pi))
        v = float(cam["rows"]) * (0.5 - lat / math.pi)
        return True, True, u, v, 0.0
    if zc <= 0.0:                                              # perspective.cc:190-209 (fisheye.cc:231-249: the same formula)
        return False, False, 0.0, 0.0, 0.0
    z_inv = 1.0 / zc
    u = (float(cam["fx"]) * xc) * z_inv + float(cam["cx"])
    v = (float(cam["fy"]) * yc) * z_inv + float(cam["cy"])
    xr = u - float(cam["focal_x_baseline"]) * z_inv
    b = [float(f32(t)) for t in bounds]
    return True, (b[0] < u and u < b[1] and b[2] < v and v < b[3]), u, v, xr


def d5_logf(x):
    """std::log(float) as D5 defines it: (float)log((double)x), glibc's f64 log"""
    x = float(f32(x))
    if math.isnan(x) or x < 0.0:
        return f32(math.nan)
    if x == 0.0:
        return f32(-math.inf)
    if math.isinf(x):
        return f32(math.inf)
    return f32(math.log(x))


_libm = None


def glibc_logf(x):
    """this machine's logf (what a reference build calls), through ctypes"""
    global _libm
    if _libm is None:
        _libm = ctypes.CDLL("libm.so.6")
        _libm.logf.restype = ctypes.c_float
        _libm.logf.argtypes = [ctypes.c_float]
    return f32(_libm.logf(float(f32(x))))


def int_cast(c):
    """static_cast<int>(float), defined as x86 does it: INT_MIN outside int's range, for inf and NaN (D5 item 4)"""
    c = float(c)
    return int(c) if (-2147483648.0 <= c < 2147483648.0) else INT_MIN


def predict_scale_level(max_valid, dist_f, log_sf, num_levels, logf=d5_logf):
    """landmark::predict_scale_level (landmark.cc:319-340) / Line::predict_scale_level (landmark_line.cc:366-387); dist_f is the float argument"""
    with np.errstate(all="ignore"):
        ratio = f32(max_valid) / f32(dist_f)
        q = f32(logf(ratio)) / f32(log_sf)
        p = int_cast(np.ceil(f32(q)))
    if p < 0:
        return 0
    if num_levels <= p:
        return num_levels - 1
    return p


def _norm(dx, dy, dz):
    return math.sqrt((dx * dx + dy * dy) + dz * dz)


def can_observe(cam, bounds, P, pos, normal, min_valid, max_valid, ray_cos_thr, log_sf, num_levels, logf=d5_logf):
    """frame::can_observe (frame.cc:797-824) -> (valid, u, v, x_right, level); normal None = reprojection only (level None)"""
    _, inside, u, v, xr = reproject(cam, bounds, P, *pos)
    if not inside:
        return False, u, v, xr, None
    if normal is None:
        return True, u, v, xr, None
    dx, dy, dz = float(pos[0]) - float(P[12]), float(pos[1]) - float(P[13]), float(pos[2]) - float(P[14])
    dist = _norm(dx, dy, dz)
    fd = f32(dist)
    max_d = f32(1.3 * float(f32(max_valid)))                  # landmark::get_max_valid_distance (landmark.cc:303-307)
    min_d = f32(0.7 * float(f32(min_valid)))
    if not (min_d <= fd and fd <= max_d):
        return False, u, v, xr, None
    n = [float(t) for t in normal]
    with np.errstate(all="ignore"):
        ray_cos = np.float64(((dx * n[0] + dy * n[1]) + dz * n[2])) / np.float64(dist)
    if ray_cos < float(f32(ray_cos_thr)):
        return False, u, v, xr, None
    return True, u, v, xr, predict_scale_level(max_valid, fd, log_sf, num_levels, logf)


def observe_points(cam, bounds, P, pos_w, normals, min_valid, max_valid, skip, ray_cos_thr, log_sf, num_levels, logf=d5_logf):
    """one problem: dict(reproj [m,2] f32, x_right [m] f32, level [m] i32, valid [m] u8, num_valid); invalid slots hold 0"""
    m = len(pos_w)
    out = dict(reproj=np.zeros((m, 2), np.float32), x_right=np.zeros(m, np.float32), level=np.zeros(m, np.int32), valid=np.zeros(m, np.uint8))
    for j in range(m):
        if skip is not None and skip[j]:
            continue
        ok, u, v, xr, lvl = can_observe(cam, bounds, P, pos_w[j], None if normals is None else normals[j],
                                        None if min_valid is None else min_valid[j], None if max_valid is None else max_valid[j],
                                        ray_cos_thr, log_sf, num_levels, logf)
        if ok:
            out["valid"][j] = 1
            out["reproj"][j] = (f32(u), f32(v))
            out["x_right"][j] = f32(xr)
            out["level"][j] = 0 if lvl is None else lvl
    out["num_valid"] = int(out["valid"].sum())
    return out


def observe_lines(cam, bounds, P, pos_w, min_valid, max_valid, skip, log_sf, num_levels, logf=d5_logf):
    """one problem, frame::can_observe_line (frame.cc:827-878) in local_landmarks_ order with the reference's temporaries reproj_sp / reproj_ep
    declared before the loop (tracking_module.cc:1010-1012): reproj_sp / reproj_ep of every slot = the temporaries after its turn, (0, 0) before
    the first write (D5 item 5).  dict(reproj_sp, reproj_ep [m,2] f32, level [m] i32 (0 where invalid), valid [m] u8, num_valid)"""
    m = len(pos_w)
    out = dict(reproj_sp=np.zeros((m, 2), np.float32), reproj_ep=np.zeros((m, 2), np.float32), level=np.zeros(m, np.int32),
               valid=np.zeros(m, np.uint8))
    sp_t, ep_t = (0.0, 0.0), (0.0, 0.0)
    for j in range(m):
        if not (skip is not None and skip[j]):
            p = [float(t) for t in pos_w[j]]
            ws, in_s, us, vs, _ = reproject(cam, bounds, P, *p[:3])
            we, in_e, ue, ve, _ = reproject(cam, bounds, P, *p[3:])
            if ws:
                sp_t = (us, vs)
            if we:
                ep_t = (ue, ve)
            mid = (0.5 * (p[0] + p[3]), 0.5 * (p[1] + p[4]), 0.5 * (p[2] + p[5]))
            ok = in_s or in_e
            if ok and not (in_s and in_e):
                ok = reproject(cam, bounds, P, *mid)[1]
            if ok:
                fd = f32(_norm(mid[0] - float(P[12]), mid[1] - float(P[13]), mid[2] - float(P[14])))
                max_d = f32(1.2 * float(f32(max_valid[j])))    # Line::get_max_valid_distance (landmark_line.cc:360-364)
                min_d = f32(0.8 * float(f32(min_valid[j])))
                ok = min_d <= fd and fd <= max_d
                if ok:
                    out["level"][j] = predict_scale_level(max_valid[j], fd, log_sf, num_levels, logf)
            out["valid"][j] = 1 if ok else 0
        out["reproj_sp"][j] = (f32(sp_t[0]), f32(sp_t[1]))
        out["reproj_ep"][j] = (f32(ep_t[0]), f32(ep_t[1]))
    out["num_valid"] = int(out["valid"].sum())
    return out


def scale_factors(scale_factor, num_levels):
    """orb_params::calc_scale_factors: float products"""
    sf = [f32(1.0)]
    for _ in range(1, num_levels):
        sf.append(f32(sf[-1] * f32(scale_factor)))
    return np.array(sf, np.float32)


def creation_distances(rng, n, scale_factor=1.2, num_levels=8):
    """landmarks seen at the distance they were created at (landmark::update_normal_and_depth, landmark.cc:283-292):
    max_valid_dist_ = (float)(dist * scale_factors[level]), min_valid_dist_ = max_valid_dist_ / scale_factors[num_levels - 1], dist f64.
    Returns (dist, min_valid, max_valid, creation level) arrays."""
    sf = scale_factors(scale_factor, num_levels)
    dist = rng.uniform(0.3, 40.0, n)
    k = rng.integers(0, num_levels, n)
    mx = np.array([f32(float(d) * float(sf[i])) for d, i in zip(dist, k)], np.float32)
    mn = (mx / sf[num_levels - 1]).astype(np.float32)
    return dist, mn, mx, k
