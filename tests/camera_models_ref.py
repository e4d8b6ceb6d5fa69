"""CPU restatement of the per-key-point camera steps of the reference's fisheye and equirectangular models (and the image bounds of all
three), for the tests of plp_post_extract_model_*.  Plain Python f64 per point; tan / sin / cos are math's (glibc), as in the reference's
host build.  Float rounding is spelled out with numpy.float32 where the reference stores or computes in float.

Cameras are dicts with the plp_camera_model fields: model ("perspective" | "fisheye" | "equirectangular"), cols, rows, fx, fy, cx, cy,
k1, k2, p1, p2, k3, k4."""
import math

import numpy as np

f32 = np.float32
SENTINEL = f32(-1000000.0)


def fisheye_undistort_point(cam, x, y):
    """cv::fisheye::undistortPoints(pts, pts, K, D, noArray(), K) for one point, as camera/fisheye.cc:172-204 calls it (OpenCV 3.4.16
    calib3d fisheye.cpp: the guarded loop -- 10 Newton steps on theta, exit when |theta_fix| < 1e-8, the (-1e6, -1e6) result for a point
    that did not converge or whose theta changed sign).  K and D are the float cv_cam_matrix_ / cv_dist_params_ (fisheye.cc:47-48).
    Returns the float32 pair."""
    fx, fy, cx, cy = (float(f32(cam[k])) for k in ("fx", "fy", "cx", "cy"))
    k = [float(f32(cam[n])) for n in ("k1", "k2", "k3", "k4")]
    pwx = (float(f32(x)) - cx) / fx
    pwy = (float(f32(y)) - cy) / fy
    theta_d = math.sqrt(pwx * pwx + pwy * pwy)
    theta_d = min(max(-math.pi / 2, theta_d), math.pi / 2)    # valid up to 180 degrees of field of view
    scale, converged, theta = 1.0, False, theta_d
    if theta_d > 1e-8:
        for _ in range(10):
            t2 = theta * theta
            t4 = t2 * t2
            t6 = t4 * t2
            t8 = t6 * t2
            a, b, c, d = k[0] * t2, k[1] * t4, k[2] * t6, k[3] * t8
            fix = (theta * (1 + a + b + c + d) - theta_d) / (1 + 3 * a + 5 * b + 7 * c + 9 * d)
            theta = theta - fix
            if abs(fix) < 1e-8:
                converged = True
                break
        scale = math.tan(theta) / theta_d
    else:
        converged = True
    flipped = (theta_d < 0 and theta > 0) or (theta_d > 0 and theta < 0)
    if not converged or flipped:
        return SENTINEL, SENTINEL
    pux, puy = pwx * scale, pwy * scale
    # P (pu, 1) with P = K: sums from 0, the zero entries of the matrix included
    p0 = 0.0 + fx * pux + 0.0 * puy + cx * 1.0
    p1 = 0.0 + 0.0 * pux + fy * puy + cy * 1.0
    p2 = 0.0 + 0.0 * pux + 0.0 * puy + 1.0 * 1.0
    return f32(p0 / p2), f32(p1 / p2)


def fisheye_undistort(cam, x, y):
    out = [fisheye_undistort_point(cam, a, b) for a, b in zip(np.asarray(x, np.float32), np.asarray(y, np.float32))]
    return np.array([o[0] for o in out], np.float32), np.array([o[1] for o in out], np.float32)


def pinhole_bearings(cam, ux, uy):
    """convert_keypoints_to_bearings of camera::perspective (perspective.cc:165-175) and camera::fisheye (fisheye.cc:206-216): the
    normalised point (true double intrinsics, float coordinates) scaled to unit length"""
    out = np.zeros((len(ux), 3), np.float64)
    for i, (a, b) in enumerate(zip(np.asarray(ux, np.float32), np.asarray(uy, np.float32))):
        xn = (float(a) - cam["cx"]) / cam["fx"]
        yn = (float(b) - cam["cy"]) / cam["fy"]
        l2 = math.sqrt(xn * xn + yn * yn + 1.0)
        out[i] = (xn / l2, yn / l2, 1.0 / l2)
    return out


def equirect_bearings(cam, x, y):
    """camera::equirectangular::convert_keypoints_to_bearings (equirectangular.cc:75-88): x / cols is a float division (unsigned int ->
    float), the subtraction of 0.5 is in double; longitude in [-pi, pi), latitude in (-pi/2, pi/2]"""
    cols, rows = f32(cam["cols"]), f32(cam["rows"])
    out = np.zeros((len(x), 3), np.float64)
    for i, (a, b) in enumerate(zip(np.asarray(x, np.float32), np.asarray(y, np.float32))):
        lon = (float(f32(a / cols)) - 0.5) * (2 * math.pi)
        lat = -(float(f32(b / rows)) - 0.5) * math.pi
        out[i] = (math.cos(lat) * math.sin(lon), -math.sin(lat), math.cos(lat) * math.cos(lon))
    return out


def image_bounds(cam, undistort=None):
    """compute_image_bounds() of the three models, as float32 (min_x, max_x, min_y, max_y) (camera/base.h:68-82):
    perspective.cc:100-128, fisheye.cc:98-168, equirectangular.cc:62-67.  undistort(xs, ys) -> (xs, ys) float32 is the model's
    undistortion (default: the fisheye restatement above; the perspective tests pass the oracle's)."""
    cols, rows = f32(cam["cols"]), f32(cam["rows"])
    whole = np.array([0.0, cols, 0.0, rows], np.float32)
    model = cam["model"]
    if model == "equirectangular":
        return whole
    if undistort is None:
        undistort = lambda xs, ys: fisheye_undistort(cam, xs, ys)   # noqa: E731
    dist = ("k1", "k2", "p1", "p2", "k3") if model == "perspective" else ("k1", "k2", "k3", "k4")
    if all(cam[k] == 0 for k in dist):
        return whole

    def corners():
        ux, uy = undistort(np.array([0, cols, 0, cols], np.float32), np.array([0, 0, rows, rows], np.float32))
        return np.array([min(ux[0], ux[2]), max(ux[1], ux[3]), min(uy[0], uy[1]), max(uy[2], uy[3])], np.float32)

    if model == "perspective":
        return corners()
    pwx, pwy = (0.0 - cam["cx"]) / cam["fx"], (0.0 - cam["cy"]) / cam["fy"]
    if not math.sqrt(pwx * pwx + pwy * pwy) > math.pi / 2:
        return corners()
    # super wide: the corners are out of view; the edge midpoints, limited to 85 degrees of incidence
    cx, cy = cam["cx"], cam["cy"]
    ux, uy = undistort(np.array([cx, cols, 0, cx], np.float32), np.array([0, cy, cy, rows], np.float32))
    tx = f32(cam["fx"] / math.tan(5.0 * math.pi / 180.0))
    ty = f32(cam["fy"] / math.tan(5.0 * math.pi / 180.0))
    min_x_thr, max_x_thr = f32(-float(tx) + cx), f32(float(tx) + cx)
    min_y_thr, max_y_thr = f32(-float(ty) + cy), f32(float(ty) + cy)
    mnx, mxx, mny, mxy = ux[2], ux[1], uy[0], uy[3]
    return np.array([min_x_thr if (mnx < min_x_thr or float(mnx) > cx) else mnx,
                     max_x_thr if (mxx > max_x_thr or float(mxx) < cx) else mxx,
                     min_y_thr if (mny < min_y_thr or float(mny) > cy) else mny,
                     max_y_thr if (mxy > max_y_thr or float(mxy) < cy) else mxy], np.float32)


def grid_cells(bounds, num_cols=64, num_rows=48):
    """inv_cell_width / inv_cell_height of the constructors (e.g. fisheye.cc:55-56): double count over the float extent"""
    return (float(np.float64(num_cols) / np.float64(f32(bounds[1] - bounds[0]))),
            float(np.float64(num_rows) / np.float64(f32(bounds[3] - bounds[2]))))
