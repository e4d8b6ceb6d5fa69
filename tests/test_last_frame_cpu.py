"""The CPU restatement of the last-frame query preparation (tests/last_frame_ref.py) on hand-built cases: the motion direction on both sides of
+-true_baseline and for a monocular setup, the midpoint rule of match_current_and_last_frames_line, and the D6 end points across skipped slots."""
import numpy as np

import last_frame_ref as LF

f32 = np.float32
CAM = {"model": "perspective", "cols": 640, "rows": 480, "fx": 500.0, "fy": 500.0, "cx": 320.0, "cy": 240.0, "focal_x_baseline": 40.0}
BOUNDS = np.array([0, 640, 0, 480], np.float32)
IDENTITY = LF.frame_pose(np.eye(3), np.zeros(3))


def _pair(tz_curr, tz_last=0.0):
    """current camera at world z = -tz_curr (trans_cw = (0, 0, tz_curr)), last camera with trans_lw = (0, 0, tz_last): trans_lc(2) = tz_last - tz_curr"""
    return LF.frame_pose(np.eye(3), np.array([0.0, 0.0, tz_curr])), LF.frame_pose(np.eye(3), np.array([0.0, 0.0, tz_last]))


def test_direction_on_both_sides_of_the_baseline():
    tb = 0.05
    for tz_curr, want in ((-0.2, 1), (-0.0500001, 1), (-0.0499999, 0), (0.0, 0), (0.0499999, 0), (0.0500001, 2), (0.2, 2)):
        pc, pl = _pair(tz_curr)
        assert LF.trans_lc_z(pc, pl) == -tz_curr + 0.0
        for setup in (LF.STEREO, LF.RGBD):
            assert LF.direction(setup, tb, pc, pl) == want, (tz_curr, setup)
        assert LF.direction(LF.MONOCULAR, tb, pc, pl) == 0
    # exactly at the threshold: strict comparisons, neither
    pc, pl = _pair(-0.25)
    assert LF.trans_lc_z(pc, pl) == 0.25 and LF.direction(LF.RGBD, 0.25, pc, pl) == 0
    pc, pl = _pair(0.25)
    assert LF.direction(LF.RGBD, 0.25, pc, pl) == 0
    # a rotated last frame: rot_lw * cam_center + trans_lw, z row only
    rot = np.array([[1.0, 0.0, 0.0], [0.0, 0.0, -1.0], [0.0, 1.0, 0.0]])
    pc = LF.frame_pose(np.eye(3), np.array([0.0, -0.3, 0.0]))           # cam_center (0, 0.3, 0)
    pl = LF.frame_pose(rot, np.array([0.0, 0.0, 0.1]))
    assert LF.trans_lc_z(pc, pl) == 0.3 + 0.1 and LF.direction(LF.STEREO, 0.2, pc, pl) == 1


def test_points_reprojection_only_with_octave_and_angle():
    pos = np.array([[0.0, 0.0, 2.0], [0.2, -0.1, 2.0], [0.0, 0.0, -1.0], [1.28, 0.0, 2.0], [0.0, 0.0, 2.0]])
    octave = np.array([0, 3, 1, 2, 5], np.int32)
    angle = np.array([10.5, 20.25, 30.0, 40.0, 50.0], np.float32)
    skip = np.array([0, 0, 0, 0, 1], np.uint8)
    out = LF.project_points(CAM, BOUNDS, IDENTITY, pos, octave, angle, skip)
    assert out["valid"].tolist() == [1, 1, 0, 0, 0] and out["num_valid"] == 2
    assert out["reproj"][1].tolist() == [370.0, 215.0] and out["x_right"][1] == f32(370.0 - 40.0 * 0.5)
    assert out["level"].tolist() == [0, 3, 0, 0, 0] and out["angle"].tolist() == [10.5, 20.25, 0, 0, 0]


def test_lines_midpoint_rule():
    P = IDENTITY
    on = lambda u, v, z: [(u - 320.0) / 500.0 * z, (v - 240.0) / 500.0 * z, z]
    pos = np.array([
        on(100, 100, 2) + on(500, 400, 3),      # both in
        on(600, 240, 2) + on(900, 240, 2),      # end out of the image, midpoint (750) out: dropped
        on(500, 240, 2) + on(700, 240, 2),      # end out, midpoint (600) in: kept
        on(-400, 240, 2) + on(-100, 240, 2),    # both out
    ])
    out = LF.project_lines(CAM, BOUNDS, P, pos, np.array([1, 2, 3, 4], np.int32), None)
    assert out["valid"].tolist() == [1, 0, 1, 0] and out["level"].tolist() == [1, 0, 3, 0]
    assert out["reproj_ep"][2].tolist() == [700.0, 240.0]                           # out of the image but z > 0: a real value
    # end point behind the camera: the midpoint decides
    pos2 = np.array([on(320, 240, 2) + [0.0, 0.0, -1.0],                            # midpoint z = 0.5, at the centre: kept
                     on(630, 240, 2) + [4.0, 0.0, -1.0]])                           # midpoint projects at u > 640: dropped
    out = LF.project_lines(CAM, BOUNDS, P, pos2, np.array([2, 2], np.int32), None)
    assert out["valid"].tolist() == [1, 0]
    assert LF.d6_end_point_used(CAM, BOUNDS, P, pos2, None).tolist() == [True, False]


def test_d6_carry_across_skipped_slots():
    P = IDENTITY
    on = lambda u, v, z: [(u - 320.0) / 500.0 * z, (v - 240.0) / 500.0 * z, z]
    behind = [0.01, 0.02, -0.5]
    pos = np.array([
        on(320, 240, 2) + behind,               # 0: no earlier writer: (0, 0) / 0
        on(100, 100, 2) + on(200, 210, 4),      # 1: writes both
        on(300, 300, 2) + on(400, 410, 4),      # 2: skipped: writes nothing
        on(320, 240, 1) + behind,               # 3: end point from slot 1
        behind + behind,                        # 4: both behind, not kept, writes nothing
        behind + on(320, 240, 1),               # 5: start point from slot 3, end point its own
        on(-300, 240, 2) + on(-200, 240, 3),    # 6: both out of the image (z > 0): not kept, but writes both
        on(320, 240, 1) + behind,               # 7: end point from slot 6
    ])
    skip = np.array([0, 0, 1, 0, 0, 0, 0, 0], np.uint8)
    out = LF.project_lines(CAM, BOUNDS, P, pos, np.arange(8, dtype=np.int32), skip)
    assert out["valid"].tolist() == [1, 1, 0, 1, 0, 1, 0, 1]
    assert out["reproj_ep"][0].tolist() == [0.0, 0.0] and out["x_right_ep"][0] == 0.0
    assert out["reproj_ep"][3].tolist() == out["reproj_ep"][1].tolist() == [200.0, 210.0]
    assert out["x_right_ep"][3] == out["x_right_ep"][1] == f32(200.0 - 40.0 / 4)
    assert out["reproj_sp"][5].tolist() == out["reproj_sp"][3].tolist() and out["x_right_sp"][5] == out["x_right_sp"][3]
    assert out["reproj_ep"][7].tolist() == [-200.0, 240.0] and out["x_right_ep"][7] == f32(-200.0 - 40.0 / 3)
    assert LF.d6_end_point_used(CAM, BOUNDS, P, pos, skip).tolist() == [True, False, False, True, False, True, False, True]
