"""The CPU restatement of local-landmark visibility (tests/landmark_observe_ref.py) on hand-derived cases, and the cost of D5's logf definition
on landmarks seen at their creation distance."""
import math

import numpy as np

import landmark_observe_ref as R
from plp import plp

f32 = np.float32
PERSP = {"model": "perspective", "cols": 640, "rows": 480, "fx": 500.0, "fy": 500.0, "cx": 320.0, "cy": 240.0, "focal_x_baseline": 40.0}
EQUI = {"model": "equirectangular", "cols": 1920, "rows": 960, "fx": 0.0, "fy": 0.0, "cx": 0.0, "cy": 0.0, "focal_x_baseline": 0.0}
BOUNDS = np.array([0, 640, 0, 480], np.float32)
EQ_BOUNDS = np.array([0, 1920, 0, 960], np.float32)
IDENTITY = R.frame_pose(np.eye(3), np.zeros(3))
LSF = R.d5_logf(f32(1.2))


def test_frame_pose_matches_the_mirror_and_update_pose_params():
    rng = np.random.default_rng(3)
    for _ in range(20):
        q = rng.normal(size=4); q /= np.linalg.norm(q)
        w, x, y, z = q
        rot = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                        [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                        [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])
        t = rng.normal(size=3)
        p = R.frame_pose(rot, t)
        assert np.array_equal(p, plp.frame_pose(rot, t))
        assert np.allclose(p[12:], -rot.T @ t, atol=1e-12)
    assert np.array_equal(IDENTITY[12:], np.zeros(3)) and all(math.copysign(1, v) < 0 for v in IDENTITY[12:])   # -0.0: -R^T 0


def test_identity_pose_and_the_optical_axis():
    wrote, inside, u, v, xr = R.reproject(PERSP, BOUNDS, IDENTITY, 0.0, 0.0, 2.0)
    assert wrote and inside and (u, v) == (320.0, 240.0) and xr == 320.0 - 40.0 * 0.5
    wrote, inside, u, v, xr = R.reproject(PERSP, BOUNDS, IDENTITY, 0.2, -0.1, 2.0)    # ((500 * 0.2) * 0.5) + 320
    assert (u, v) == (370.0, 215.0) and inside
    assert R.reproject(PERSP, BOUNDS, IDENTITY, 0.0, 0.0, 0.0)[:2] == (False, False)    # z <= 0: nothing written
    assert R.reproject(PERSP, BOUNDS, IDENTITY, 0.0, 0.0, -1.0)[:2] == (False, False)
    assert R.reproject(PERSP, BOUNDS, IDENTITY, 1.28, 0.0, 2.0)[:2] == (True, False)   # u = 640 = max_x: strict
    ok, u, v, xr, lvl = R.can_observe(PERSP, BOUNDS, IDENTITY, (0.0, 0.0, 2.0), (0.0, 0.0, 1.0), 1.0, 2.0, 0.5, LSF, 8)
    assert ok and lvl == 0                                                            # ratio 1: log 0, ceil 0
    ok, *_ = R.can_observe(PERSP, BOUNDS, IDENTITY, (0.0, 0.0, 2.0), (0.0, 1.0, 0.0), 1.0, 2.0, 0.5, LSF, 8)
    assert not ok                                                                     # ray_cos 0 < 0.5


def test_equirectangular_quadrants_and_the_zero_vector():
    cases = {(0.0, 0.0, 1.0): (960.0, 480.0), (1.0, 0.0, 0.0): (1440.0, 480.0), (0.0, 0.0, -1.0): (1920.0, 480.0),
             (-1.0, 0.0, 0.0): (480.0, 480.0), (0.0, -1.0, 0.0): (960.0, 0.0), (0.0, 1.0, 0.0): (960.0, 960.0),
             (0.0, 0.0, 0.0): (960.0, 480.0)}                                        # the zero vector stays zero: asin 0, atan2(0, 0)
    for p, want in cases.items():
        wrote, inside, u, v, xr = R.reproject(EQUI, EQ_BOUNDS, IDENTITY, *p)
        assert wrote and inside and xr == 0.0 and (u, v) == want, (p, u, v)
    # quadrants between the axes
    for sx, sz in ((1, 1), (1, -1), (-1, 1), (-1, -1)):
        _, _, u, v, _ = R.reproject(EQUI, EQ_BOUNDS, IDENTITY, float(sx), 0.0, float(sz))
        assert u == 1920.0 * (0.5 + math.atan2(sx, sz) / (2 * math.pi)) and v == 480.0


def test_level_clamps_and_the_int_cast():
    assert R.predict_scale_level(1.0, 4.0, LSF, 8) == 0                              # ratio 1/4: ceil(-7.6) = -7 -> 0
    assert R.predict_scale_level(1000.0, 1.0, LSF, 8) == 7                           # ceil(37.9) -> top level
    assert R.predict_scale_level(f32(1.2) ** 3, 1.0, LSF, 8) in (3, 4)
    assert R.int_cast(math.inf) == R.INT_MIN and R.int_cast(-math.inf) == R.INT_MIN and R.int_cast(math.nan) == R.INT_MIN
    # ratio = inf (distance 0): x86's cast gives INT_MIN -> level 0; a saturating cast would give the top level
    assert R.predict_scale_level(5.0, 0.0, LSF, 8) == 0
    assert R.predict_scale_level(0.0, 0.0, LSF, 8) == 0                              # 0 / 0: NaN
    # reachable through can_observe: an equirectangular landmark at the camera centre with min_valid_dist_ 0 (ray_cos NaN passes)
    ok, u, v, xr, lvl = R.can_observe(EQUI, EQ_BOUNDS, IDENTITY, (0.0, 0.0, 0.0), (0.0, 0.0, 1.0), 0.0, 5.0, 0.5, LSF, 8)
    assert ok and lvl == 0


def test_stale_line_end_points_on_a_hand_example():
    """five lines, identity pose (tracking_module.cc:1010-1012: the temporaries outlive each landmark's turn)"""
    pos = np.array([
        [0.0, 0.0, 2.0, 0.2, 0.0, 2.0],     # 0 both in: sp (320, 240), ep (370, 240)
        [0.1, 0.1, 2.0, 0.3, 0.3, 2.0],     # 1 skipped: nothing written
        [0.0, 0.2, 2.0, 0.0, 0.0, -1.0],    # 2 ep behind, midpoint (0, .1, .5) in: valid with ep of line 0
        [10.0, 0.0, 1.0, 0.0, 0.0, -2.0],   # 3 sp out of the image (written: (5320, 240)), ep behind, midpoint behind: rejected
        [0.0, 0.0, -1.0, 0.0, -0.2, 2.0],   # 4 sp behind, midpoint in: valid with sp of the REJECTED line 3
    ])
    skip = np.array([0, 1, 0, 0, 0], np.uint8)
    mn, mx = np.full(5, 0.1, np.float32), np.full(5, 100.0, np.float32)
    out = R.observe_lines(PERSP, BOUNDS, IDENTITY, pos, mn, mx, skip, R.d5_logf(f32(2.0)), 2)
    assert out["valid"].tolist() == [1, 0, 1, 0, 1] and out["num_valid"] == 3
    assert out["reproj_sp"].tolist() == [[320, 240], [320, 240], [320, 290], [5320, 240], [5320, 240]]
    assert out["reproj_ep"].tolist() == [[370, 240], [370, 240], [370, 240], [370, 240], [320, 190]]
    # a leading stale slot: (0, 0) before the first write
    out = R.observe_lines(PERSP, BOUNDS, IDENTITY, pos[2:3], mn[:1], mx[:1], None, R.d5_logf(f32(2.0)), 2)
    assert out["valid"].tolist() == [1] and out["reproj_ep"].tolist() == [[0, 0]] and out["reproj_sp"].tolist() == [[320, 290]]


def test_logf_definition_against_glibc_on_the_creation_distance_boundary():
    """Landmarks seen at the distance they were created at: ratio = scale_factor^k up to float rounding, so log(ratio) / log_scale_factor lies
    within an ulp of the integer k and ceil decides between k and k + 1.  D5 defines std::log(float) as (float)log((double)x); on these 20 000
    cases it picks the same level as this machine's glibc logf every time, and the two logf values themselves agree on every case."""
    rng = np.random.default_rng(1)
    dist, mn, mx, k = R.creation_distances(rng, 20000)
    glibc_lsf = R.glibc_logf(f32(1.2))
    assert glibc_lsf == LSF
    lv_d5, lv_glibc, logf_diff = [], [], 0
    for d, a in zip(dist, mx):
        fd = f32(d)
        ratio = f32(a) / fd
        logf_diff += R.d5_logf(ratio) != R.glibc_logf(ratio)
        lv_d5.append(R.predict_scale_level(a, fd, LSF, 8))
        lv_glibc.append(R.predict_scale_level(a, fd, glibc_lsf, 8, R.glibc_logf))
    lv_d5, lv_glibc = np.array(lv_d5), np.array(lv_glibc)
    assert int((lv_d5 != lv_glibc).sum()) == 0 and logf_diff == 0
    # the set does sit on the boundary: ceil lands on k for most and on k + 1 for the others
    assert 0.02 < float((lv_d5 != k).mean()) < 0.5 and set(np.unique(lv_d5 - k)) <= {0, 1}
