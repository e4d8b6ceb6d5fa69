"""The CPU restatement of the stereo key-line association and of the 3-D key lines (tests/stereo_keylines_ref.py) on hand-worked cases: each
gate of frame.cc:400-418 on both sides of its threshold, the two readings of the unqualified abs, the 1-NN's
"nothing found", and a 3-D segment seen by a rectified stereo pair and by a depth map, recovered by triangulate_stereo_for_line's two branches."""
import numpy as np

import stereo_keylines_ref as SK
from plp import plp

f32 = np.float32
KL = plp.KL_DTYPE
CAM = {"fx": 512.0, "fy": 512.0, "cx": 320.0, "cy": 240.0, "focal_x_baseline": 64.0}   # powers of two: the synthetic pixels are exact floats


def _kl(sx, sy, ex, ey, angle=None):
    k = SK.make_keyline(KL, sx, sy, ex, ey)
    if angle is not None:
        k["angle"] = f32(angle)
    return k


def _pair(dx=0.0, dy=0.0, a1=0.5, a2=0.5):
    """a left line and its right partner whose start and end points differ by (dx, dy)"""
    return _kl(100, 100, 300, 150, a1), _kl(100 - dx, 100 - dy, 300 - dx, 150 - dy, a2)


def test_distance_gate_at_29_and_30():
    l, r = _pair()
    assert SK.keep_match(l, r, 29) and SK.keep_match(l, r, 0)
    assert not SK.keep_match(l, r, 30) and not SK.keep_match(l, r, 31)


def test_end_point_distance_exactly_200_is_rejected():
    assert SK.point_distance(f32(120), f32(160)) == f32(200.0)               # 120^2 + 160^2 = 200^2 exactly in float
    l, r = _pair(120.0, 160.0)
    assert not SK.keep_match(l, r, 10)
    l, r = _pair(119.0, 160.0)                                              # 199.40 px
    assert SK.keep_match(l, r, 10)
    # only the end point too far: rejected as well
    l = _kl(100, 100, 300, 150, 0.5)
    r = _kl(100, 100, 300 - 120, 150 - 160, 0.5)
    assert not SK.keep_match(l, r, 10)


def test_angle_just_inside_and_outside_5_degrees():
    assert SK.angle_deg(1.0872, 1.0) < f32(5) < SK.angle_deg(1.0873, 1.0)    # 4.9987 and 5.0044 degrees
    l, r = _pair(a1=1.0872, a2=1.0)
    assert SK.keep_match(l, r, 10)
    l, r = _pair(a1=1.0873, a2=1.0)
    assert not SK.keep_match(l, r, 10)
    l, r = _pair(a1=-1.0872, a2=1.0)                                        # abs of each angle first: the sign does not count
    assert SK.keep_match(l, r, 10)


def test_the_two_abs_readings_differ_between_5_and_57_degrees():
    # a difference of 0.2 rad = 11.5 degrees: the float abs (D7) rejects it, the int abs truncates both angles to 0 and keeps it
    assert SK.angle_deg(0.5, 0.3, "float") == f32(f32(f32(abs(f32(0.5) - f32(0.3))) * f32(180)).astype(np.float64) / 3.14)
    assert 11.4 < SK.angle_deg(0.5, 0.3, "float") < 11.5 and SK.angle_deg(0.5, 0.3, "int") == 0
    l, r = _pair(a1=0.5, a2=0.3)
    assert not SK.keep_match(l, r, 10, "float") and SK.keep_match(l, r, 10, "int")
    # 0.9 rad = 51.6 degrees, still inside one radian: only the int reading keeps it; at 1.2 rad both reject
    l, r = _pair(a1=1.95, a2=1.05)
    assert not SK.keep_match(l, r, 10, "float") and SK.keep_match(l, r, 10, "int")
    l, r = _pair(a1=2.2, a2=1.0)
    assert not SK.keep_match(l, r, 10, "float") and not SK.keep_match(l, r, 10, "int")


def test_nothing_found_and_empty_sides():
    l, r = _pair()
    kls = np.array([l, l, l], KL)
    krs = np.array([r, r], KL)
    good, dep, xr = SK.stereo_keylines(kls, krs, np.array([-1, 0, 1], np.int32), np.array([256, 5, 29], np.int32))
    assert good.tolist() == [-1, 0, 1]
    assert dep.tolist() == [[-1, -1], [1, 1], [1, 1]] and np.array_equal(dep, xr)
    good, dep, _ = SK.stereo_keylines(kls, np.zeros(0, KL), np.array([-1, -1, -1], np.int32), np.array([256, 256, 256], np.int32))
    assert good.tolist() == [-1, -1, -1] and (dep == -1).all()


def _rotation(rng, scale=0.2):
    w = rng.normal(size=3) * scale
    th = np.linalg.norm(w)
    k = w / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx


def _segment(rng):
    """a segment chosen in the left camera frame so that its pixels, depths and disparities are exact floats: (camera points [2, 3],
    left pixels [2, 2], depths [2])"""
    while True:
        u = rng.integers(20, 620, 2).astype(np.float64)
        v = rng.integers(20, 460, 2).astype(np.float64)
        if abs(u[1] - u[0]) > 40 and abs(v[1] - v[0]) > 40:     # neither horizontal nor vertical
            break
    z = np.array([2.0, 4.0])[rng.permutation(2)]
    X = np.stack([(u - CAM["cx"]) * z / CAM["fx"], (v - CAM["cy"]) * z / CAM["fy"], z], 1)
    return X, np.stack([u, v], 1), z


def test_stereo_and_depth_recover_a_synthetic_segment():
    rng = np.random.default_rng(5)
    for _ in range(20):
        X, px, z = _segment(rng)
        R = _rotation(rng)                                          # rot_cw
        c = np.array([0.3, -0.2, 1.0]) + rng.normal(size=3) * 0.1   # camera centre in the world
        t = -R @ c
        P = SK.frame_pose(R, t)
        W = (R.T @ X.T).T + c                                       # the world segment
        want = np.concatenate([W[0], W[1]])
        left = _kl(px[0, 0], px[0, 1], px[1, 0], px[1, 1])
        disp = CAM["focal_x_baseline"] / z                          # rectified right view: u - focal_x_baseline / z
        right = _kl(px[0, 0] - disp[0], px[0, 1], px[1, 0] - disp[1], px[1, 1])
        got, ok = SK.keyline_3d(CAM, SK.STEREO, P, left, good=0, kl_right=np.array([right], KL))
        if (W[:, 2] > 0).all():
            assert ok and np.allclose(got, want, rtol=1e-9, atol=0), (got, want)
        else:
            assert not ok and (got == 0).all()
        got, ok = SK.keyline_3d(CAM, SK.RGBD, P, left, depth_pair=np.array(z, np.float32))
        assert ok and np.allclose(got, want, rtol=1e-9, atol=0), (got, want)


def test_zero_vector_cases():
    P = SK.frame_pose(np.eye(3), np.zeros(3))
    flat = _kl(100, 200, 300, 200)                                  # horizontal: l1 = 0, l2 / l1 is not finite (D7)
    got, ok = SK.keyline_3d(CAM, SK.STEREO, P, flat, good=0, kl_right=np.array([_kl(90, 200, 290, 200)], KL))
    assert not ok and (got == 0).all()
    line = _kl(100, 100, 300, 200)
    assert not SK.keyline_3d(CAM, SK.STEREO, P, line, good=-1, kl_right=np.zeros(0, KL))[1]   # no good match
    right = _kl(84, 100, 284, 200)                                  # disparity 16: z = 4 in the camera...
    got, ok = SK.keyline_3d(CAM, SK.STEREO, P, line, good=0, kl_right=np.array([right], KL))
    assert ok and np.allclose(got[[2, 5]], 4.0, rtol=1e-12)
    below = SK.frame_pose(np.eye(3), np.array([0.0, 0.0, 5.0]))       # ... and the camera 5 m below the world origin: world z = -1 < 0
    got, ok = SK.keyline_3d(CAM, SK.STEREO, below, line, good=0, kl_right=np.array([right], KL))
    assert not ok and (got == 0).all()
    # RGB-D: a zero depth (what compute_stereo_from_depth stores for no depth) or the (-1, -1) initial value
    for d in ((0.0, 2.0), (2.0, 0.0), (-1.0, -1.0)):
        got, ok = SK.keyline_3d(CAM, SK.RGBD, P, line, depth_pair=np.array(d, np.float32))
        assert not ok and (got == 0).all()
