"""The fuse / Sim3 / relocalisation queries without a GPU: the restatement tests/project_landmarks_ref.py on hand-derived cases (every status,
both dist_modes, both line_dist_modes, the two places the loops differ from frame::can_observe, the D6 carry), the pose helpers of the Python
mirror, the ABI, and the coverage floor of the scenes the GPU tests use."""
import math
import pathlib
import re

import numpy as np
import pytest

import landmark_observe_ref as R
import project_landmarks_ref as PR
import project_landmarks_scene as S
from plp import plp
from test_gpu_landmark_observe import CAMERAS, yaml_of

f32 = np.float32
CAM = {"model": "perspective", "cols": 640, "rows": 480, "fx": 500.0, "fy": 500.0, "cx": 320.0, "cy": 240.0, "focal_x_baseline": 40.0}
BOUNDS = np.array([0.0, 640.0, 0.0, 480.0], np.float32)
EYE = R.frame_pose(np.eye(3), np.zeros(3))
LSF = R.d5_logf(f32(1.2))
LSF_LSD = R.d5_logf(f32(2.0))


def point(pos, normal=(0, 0, 1.0), mn=2.0, mx=8.0, P=EYE, dist_mode=PR.DIST_CENTER, ray_test=True, cam=CAM):
    return PR.project_point(cam, BOUNDS, P, pos, normal, f32(mn), f32(mx), dist_mode, ray_test, LSF, 8)


def test_every_point_status_by_hand():
    st, u, v, xr, lvl = point((0, 0, 4.0))
    # ratio 8 / 4 = 2: log 2 / log 1.2 = 3.80 -> level 4; the principal point; x_right = u - 40 / 4
    assert (st, u, v, xr, lvl) == (PR.KEPT, 320.0, 240.0, 310.0, 4)
    assert point((10.0, 0, 1.0))[0] == PR.NOT_IN_IMAGE                # u = 5320
    assert point((0, 0, -1.0))[0] == PR.NOT_IN_IMAGE                  # behind the camera
    assert point((0, 0, 4.0), mx=3.0)[0] == PR.DISTANCE               # 1.3 x 3 = 3.9 < 4
    assert point((0, 0, 4.0), mn=6.0)[0] == PR.DISTANCE               # 4 < 0.7 x 6 = 4.2
    assert point((0, 0, 4.0), normal=(1.0, 0, 0))[0] == PR.RAY        # dot 0 < 2
    assert point((0, 0, 4.0), normal=(1.0, 0, 0), ray_test=False)[0] == PR.KEPT
    out = PR.project_points(CAM, BOUNDS, EYE, np.array([[0, 0, 4.0], [0, 0, 4.0]]), np.array([[0, 0, 1.0]] * 2), np.full(2, 2, f32), np.full(2, 8, f32),
                            np.array([1, 0], np.uint8), PR.DIST_CENTER, True, LSF, 8)
    assert out["status"].tolist() == [PR.SKIPPED, PR.KEPT] and out["valid"].tolist() == [0, 1] and out["num_valid"] == 1
    assert out["reproj_d"][1].tolist() == [320.0, 240.0] and out["reproj"][0].tolist() == [0, 0]


def test_both_dist_modes_by_hand():
    """a mutual pass: the matrix 2 I, translation (0, 0, 1); pos (0, 0, 4) -> pos_2 = (0, 0, 9): the camera-frame distance is 9, the distance
    to entries 12-14 (0 here) is 4"""
    P = np.concatenate([(2.0 * np.eye(3)).ravel(), [0, 0, 1.0], np.zeros(3)])
    assert point((0, 0, 4.0), mx=5.0, P=P, dist_mode=PR.DIST_CENTER, ray_test=False)[0] == PR.KEPT       # 4 <= 6.5
    assert point((0, 0, 4.0), mx=5.0, P=P, dist_mode=PR.DIST_CAMERA, ray_test=False)[0] == PR.DISTANCE   # 6.5 < 9
    st, u, v, xr, lvl = point((0, 0, 4.0), mx=9.0, P=P, dist_mode=PR.DIST_CAMERA, ray_test=False)
    assert (st, u, v, xr, lvl) == (PR.KEPT, 320.0, 240.0, 320.0 - 40.0 / 9.0, 0)                           # ratio 1: level 0
    # entries 12-14 are not read in the camera mode
    P2 = P.copy(); P2[12:15] = (100.0, -50.0, 7.0)
    assert point((0, 0, 4.0), mx=9.0, P=P2, dist_mode=PR.DIST_CAMERA, ray_test=False) == (st, u, v, xr, lvl)


def test_the_distance_range_is_compared_in_f64_not_in_float():
    """frame::can_observe narrows the distance to float before it compares (is_inside_in_orb_scale(const float)); these loops compare the f64
    distance with the float bound widened.  A distance 1e-9 below the bound: out of range here, inside for can_observe."""
    mn = f32(10.0)
    min_d = f32(0.7 * float(mn))
    dist = float(min_d) - 1e-9
    assert f32(dist) == min_d and dist < float(min_d)                 # the two comparisons disagree
    assert point((0, 0, dist), mn=mn, mx=20.0)[0] == PR.DISTANCE
    assert R.can_observe(CAM, BOUNDS, EYE, (0, 0, dist), (0, 0, 1.0), mn, f32(20.0), 0.5, LSF, 8)[0]
    mx = f32(10.0)
    max_d = f32(1.3 * float(mx))
    dist = float(max_d) + 1e-9
    assert f32(dist) == max_d and float(max_d) < dist
    assert point((0, 0, dist), mn=1.0, mx=mx)[0] == PR.DISTANCE
    assert R.can_observe(CAM, BOUNDS, EYE, (0, 0, dist), (0, 0, 1.0), f32(1.0), mx, 0.5, LSF, 8)[0]
    assert point((0, 0, float(max_d)), mn=1.0, mx=mx)[0] == PR.KEPT  # on the bound: kept


def test_the_viewing_angle_is_dot_less_than_half_the_distance_without_a_division():
    assert point((0, 0, 4.0), normal=(0, 0, 0.5))[0] == PR.KEPT                          # dot 2 == 0.5 x 4: not less
    assert point((0, 0, 4.0), normal=(0, 0, float(np.nextafter(0.5, 0.0))))[0] == PR.RAY
    # on the boundary with an inexact product: dist = 3 (1 + 2^-52), normal z one ulp below 0.5; the rounded dot decides, not the angle
    d = 3.0 * (1.0 + 2.0 ** -52)
    for nz in (0.5, float(np.nextafter(0.5, 0.0)), float(np.nextafter(0.5, 1.0))):
        dot = d * nz
        assert point((0, 0, d), normal=(0, 0, nz), mn=0.5, mx=8.0)[0] == (PR.RAY if dot < 0.5 * d else PR.KEPT)
    # dist = 0 (the landmark at the camera centre, equirectangular: in the image): 0 < 0.5 x 0 is false, the slot is not rejected by the ray test
    eq = {"model": "equirectangular", "cols": 1920, "rows": 960, "fx": 0.0, "fy": 0.0, "cx": 0.0, "cy": 0.0, "focal_x_baseline": 0.0}
    assert point((0, 0, 0.0), normal=(0, 0, 1.0), mn=0.0, mx=8.0, cam=eq)[0] == PR.KEPT


def lines(pos, mn, mx, mode, skip=None):
    pos = np.asarray(pos, np.float64)
    m = len(pos)
    return PR.project_lines(CAM, BOUNDS, EYE, pos, np.full(m, mn, f32) if np.isscalar(mn) else np.asarray(mn, f32),
                            np.full(m, mx, f32) if np.isscalar(mx) else np.asarray(mx, f32), skip, mode, LSF_LSD, 2)


def test_every_line_status_and_both_line_dist_modes_by_hand():
    pos = [[-0.5, 0, 4.0, 0.5, 0, 4.0],      # both end points in
           [0, 0, 4.0, 3.0, 0, 4.0],         # end point out (u = 695), midpoint (1.5, 0, 4) in (u = 507.5)
           [0, 0, 4.0, 20.0, 0, 4.0],        # end point out, midpoint (10, 0, 4) out
           [10.0, 0, 4.0, 20.0, 0, 4.0],     # both out
           [-0.5, 0, 4.0, 0.5, 0, 4.0]]      # skipped
    out = lines(pos, 2.0, 8.0, PR.LINE_ENDPOINTS, skip=[0, 0, 0, 0, 1])
    assert out["status"].tolist() == [PR.KEPT, PR.KEPT, PR.MIDPOINT_OUT, PR.NOT_IN_IMAGE, PR.SKIPPED]
    assert out["reproj_sp_d"][0].tolist() == [320.0 - 62.5, 240.0] and out["reproj_ep_d"][0].tolist() == [320.0 + 62.5, 240.0]
    assert out["level"][0] == 1 and out["num_valid"] == 2             # ratio 8 / 4 = 2: log 2 / log 2 = 1
    # the start point at distance 2, the end point at 10, the midpoint at 6; 0.8 x min = 4, 1.2 x max = 8.4
    far = [[0, 0, 2.0, 0, 0, 10.0]]
    assert lines(far, 5.0, 7.0, PR.LINE_ENDPOINTS)["status"].tolist() == [PR.DISTANCE]    # 2 < 4 (and 8.4 < 10)
    mid = lines(far, 5.0, 7.0, PR.LINE_MIDPOINT)
    assert mid["status"].tolist() == [PR.KEPT] and mid["level"].tolist() == [1]             # 4 <= 6 <= 8.4; ratio 7 / 6: ceil(0.22) = 1
    assert lines(far, 5.0, 4.0, PR.LINE_MIDPOINT)["status"].tolist() == [PR.DISTANCE]      # 1.2 x 4 = 4.8 < 6
    assert lines(far, 1.0, 9.0, PR.LINE_ENDPOINTS)["status"].tolist() == [PR.KEPT]         # 0.8 <= 2, 10 <= 10.8


def test_the_d6_carry_on_five_lines():
    """reproj_sp / reproj_ep and x_right_sp / x_right_ep are declared inside the reference's loops; an end point with z <= 0 is not written.
    D6: it reads the most recent earlier non-skipped slot's value, (0, 0) / 0 before the first."""
    pos = [[0, 0, 4.0, 0, 0, -1.0],          # 0: end point behind, midpoint (0, 0, 1.5) in: kept, end point (0, 0) / 0
           [1.0, 0, 4.0, 1.0, 0.5, 4.0],     # 1: skipped: writes nothing
           [0.4, 0, 2.0, 0.8, 0, 2.0],       # 2: both written, rejected by the distance range: still the writer
           [0, 0, -1.0, 0, 0, 4.0],          # 3: start point behind: carried from 2; kept
           [0, 0.4, 4.0, 0, 0, -2.0]]        # 4: end point behind: carried from 3; kept
    mx = [8.0, 8.0, 1.0, 8.0, 8.0]
    out = lines(pos, 0.1, mx, PR.LINE_MIDPOINT, skip=[0, 1, 0, 0, 0])
    assert out["status"].tolist() == [PR.KEPT, PR.SKIPPED, PR.DISTANCE, PR.KEPT, PR.KEPT]
    assert out["reproj_ep_d"][0].tolist() == [0.0, 0.0] and out["x_right_ep"][0] == 0.0
    assert out["reproj_sp_d"][1].tolist() == [320.0, 240.0] and out["reproj_ep_d"][1].tolist() == [0.0, 0.0]     # after a skipped slot: unchanged
    assert out["reproj_sp_d"][2].tolist() == [420.0, 240.0] and out["reproj_ep_d"][2].tolist() == [520.0, 240.0]
    assert out["reproj_sp_d"][3].tolist() == [420.0, 240.0] and out["x_right_sp"][3] == f32(420.0 - 20.0)         # carried from slot 2
    assert out["reproj_ep_d"][3].tolist() == [320.0, 240.0]
    assert out["reproj_sp_d"][4].tolist() == [320.0, 290.0] and out["reproj_ep_d"][4].tolist() == [320.0, 240.0]  # end point carried from slot 3
    assert out["x_right_ep"][4] == f32(310.0)
    assert np.array_equal(out["reproj_sp"], out["reproj_sp_d"].astype(np.float32)) and np.array_equal(out["reproj_ep"], out["reproj_ep_d"].astype(np.float32))


# ---- pose helpers of the Python mirror (these fail on a tree without plp.sim3_pose / plp.mutual_poses)
def rot_z90():
    return np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])


def test_sim3_pose_by_hand():
    S3 = np.eye(4); S3[:3, :3] *= 2.0; S3[:3, 3] = (2.0, 4.0, -6.0)          # scale 2, identity rotation
    assert plp.sim3_pose(S3).tolist() == [1, 0, 0, 0, 1, 0, 0, 0, 1, 1.0, 2.0, -3.0, -1.0, -2.0, 3.0]
    S3 = np.eye(4); S3[:3, :3] = 4.0 * rot_z90(); S3[:3, 3] = (4.0, 8.0, 12.0)   # scale 4, 90 degrees about z
    got = plp.sim3_pose(S3)
    assert got[:12].tolist() == [0, -1, 0, 1, 0, 0, 0, 0, 1, 1.0, 2.0, 3.0]
    assert got[12:].tolist() == [-2.0, 1.0, -3.0]                             # -R^T t
    assert np.array_equal(got, PR.sim3_pose(S3))


def test_mutual_poses_by_hand():
    I3, z = np.eye(3), np.zeros(3)
    # scale 2, identity rotations: s_rot_21w = 0.5 I, trans_21w = 0.5 trans_1w - 0.5 trans_12; s_rot_12w = 2 I, trans_12w = 2 trans_2w + trans_12
    got = plp.mutual_poses(2.0, I3, (2.0, 4.0, 6.0), I3, (1.0, 1.0, 1.0), I3, (0.5, 0.25, 0.125))
    assert got.shape == (2, 15)
    assert got[0].tolist() == [0.5, 0, 0, 0, 0.5, 0, 0, 0, 0.5, -0.5, -1.5, -2.5, 0, 0, 0]
    assert got[1].tolist() == [2, 0, 0, 0, 2, 0, 0, 0, 2, 3.0, 4.5, 6.25, 0, 0, 0]
    # rot_12 = 90 degrees about z, scale 1, key frames at the origin: s_rot_21w = R^T, trans_21w = -R^T trans_12
    got = plp.mutual_poses(1.0, rot_z90(), (1.0, 2.0, 3.0), I3, z, I3, z)
    assert got[0].tolist() == [0, 1, 0, -1, 0, 0, 0, 0, 1, -2.0, 1.0, -3.0, 0, 0, 0]
    assert got[1].tolist() == [0, -1, 0, 1, 0, 0, 0, 0, 1, 1.0, 2.0, 3.0, 0, 0, 0]
    # s_12 is a float in the reference
    a = plp.mutual_poses(1.1, I3, z, I3, z, I3, z)
    assert a[1][0] == float(f32(1.1)) and a[0][0] == 1.0 / float(f32(1.1))


def test_pose_helpers_against_numpy_on_random_inputs():
    rng = np.random.default_rng(5)
    for _ in range(200):
        s = float(rng.uniform(0.3, 3.0))
        Rm, t = S.rotation(rng), rng.normal(size=3)
        S3 = np.eye(4); S3[:3, :3] = s * Rm; S3[:3, 3] = t
        got = plp.sim3_pose(S3)
        assert np.array_equal(got, PR.sim3_pose(S3))
        assert np.abs(got[:9].reshape(3, 3) - Rm).max() < 1e-12 and np.abs(got[9:12] - t / s).max() < 1e-12
        assert np.abs(got[12:] - (-Rm.T @ (t / s))).max() < 1e-12
        R12, R1, R2 = S.rotation(rng), S.rotation(rng), S.rotation(rng)
        t12, t1, t2 = rng.normal(size=3), rng.normal(size=3), rng.normal(size=3)
        got = plp.mutual_poses(s, R12, t12, R1, t1, R2, t2)
        assert np.array_equal(got, PR.mutual_poses(s, R12, t12, R1, t1, R2, t2))
        sf = float(f32(s))
        s21 = (1.0 / sf) * R12.T
        assert np.abs(got[0, :9].reshape(3, 3) - s21 @ R1).max() < 1e-12
        assert np.abs(got[0, 9:12] - (s21 @ t1 - s21 @ t12)).max() < 1e-12
        assert np.abs(got[1, :9].reshape(3, 3) - sf * R12 @ R2).max() < 1e-12
        assert np.abs(got[1, 9:12] - (sf * R12 @ t2 + t12)).max() < 1e-12
        assert not got[:, 12:].any()


def test_abi_lists_the_four_entry_points():
    header = (pathlib.Path(plp.ROOT) / "include" / "plp_front.h").read_text()
    names = ["plp_project_landmarks_device", "plp_project_landmarks_host", "plp_project_landmark_lines_device", "plp_project_landmark_lines_host"]
    for n in names:
        assert re.search(r"plp_status\s+" + n + r"\s*\(", header), n
        assert n in plp.api_symbols(), n
    assert "typedef struct plp_project_args" in header
    # (that the mirror's struct follows the header's field order: tests/test_abi_and_model.py, for every struct)
    assert (plp.PROJECT_KEPT, plp.PROJECT_SKIPPED, plp.PROJECT_NOT_IN_IMAGE, plp.PROJECT_MIDPOINT_OUT, plp.PROJECT_DISTANCE, plp.PROJECT_RAY) == \
        (PR.KEPT, PR.SKIPPED, PR.NOT_IN_IMAGE, PR.MIDPOINT_OUT, PR.DISTANCE, PR.RAY)
    for k, name in enumerate(("KEPT", "SKIPPED", "NOT_IN_IMAGE", "MIDPOINT_OUT", "DISTANCE", "RAY")):
        assert re.search(rf"PLP_PROJECT_{name} = {k}\b", header), name


# ---- the coverage floor of the scenes: every status a camera model can reach in at least 2 % of the slots
@pytest.mark.parametrize("name", CAMERAS)
def test_scenes_reach_every_status(name):
    """4 000 slots, seed 7, per loop flavour.  The bounds are the image itself here (the distorted cameras' own bounds come from the device's
    undistortion; the GPU tests assert the same floor on them)."""
    cm = plp.camera_model(yaml_of(name))
    bounds = S.whole_image(cm)
    rc = S.ref_cam(cm)
    m = 4000
    rng = np.random.default_rng(7)
    P = S.random_pose(rng, False)
    pos, nm, mn, mx, skip = S.point_scene(rng, cm, bounds, P, m, LSF)
    w = PR.project_points(rc, bounds, P, pos, nm, mn, mx, skip, PR.DIST_CENTER, True, LSF, 8)
    PR.assert_coverage(rc["model"], False, True, w["status"])
    row, Pu, s = S.scaled_pose(rng)
    pos, nm, mn, mx, skip = S.point_scene_camera(rng, cm, bounds, Pu, s, m, LSF)
    w = PR.project_points(rc, bounds, row, pos, None, mn, mx, skip, PR.DIST_CAMERA, False, LSF, 8)
    PR.assert_coverage(rc["model"], False, False, w["status"])
    pos, mn, mx, skip = S.line_scene(rng, cm, bounds, P, m)
    for mode in (PR.LINE_ENDPOINTS, PR.LINE_MIDPOINT):
        w = PR.project_lines(rc, bounds, P, pos, mn, mx, skip, mode, LSF_LSD, 2)
        sh = PR.assert_coverage(rc["model"], True, False, w["status"])
        if rc["model"] != "equirectangular":      # kept with an end point behind the camera: the carried values of D6 are read
            assert S.carried_kept_share(rc, bounds, P, pos, skip, w) >= 0.02, (name, mode, sh)
