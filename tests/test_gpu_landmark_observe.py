"""Local-landmark visibility on the device (plp_observe_landmarks_* / plp_observe_landmark_lines_*) against the CPU restatement
tests/landmark_observe_ref.py, for the three camera models, and end to end into plp_match_device."""
import ctypes as C
import math

import numpy as np
import pytest

import landmark_observe_ref as R
import oracle_lib as O
from plp import plp

pytestmark = pytest.mark.gpu
f32 = np.float32

# the five perspective cameras of tests/test_gpu_camera_models.py (fx, fy, cx, cy, k1, k2, p1, p2, k3, focal_x_baseline)
PERSP = {
    "fr1": (517.306408, 516.469215, 318.643040, 255.313989, 0.262383, -0.953104, -0.005358, 0.002628, 1.163314, 40.0),
    "fr2": (520.908620, 521.007327, 325.141442, 249.701764, 0.231222, -0.784899, -0.003257, -0.000105, 0.917205, 40.0),
    "fr3": (535.4, 539.2, 320.1, 247.6, 0.0, 0.0, 0.0, 0.0, 0.0, 40.0),
    "kitti": (718.856, 718.856, 607.1928, 185.2157, 0.0, 0.0, 0.0, 0.0, 0.0, 386.1448),
    "wide": (300.0, 305.0, 322.0, 241.0, -0.35, 0.12, 0.001, -0.0007, -0.02, 30.0),
}
TUM_VI_MONO = {"Camera.model": "fisheye", "Camera.cols": 512, "Camera.rows": 512,
               "Camera.fx": 190.97847715128717, "Camera.fy": 190.9733070521226, "Camera.cx": 254.93170605935475, "Camera.cy": 256.8974428996504,
               "Camera.k1": 0.0034823894022493434, "Camera.k2": 0.0007150348452162257, "Camera.k3": -0.0020532361418706202,
               "Camera.k4": 0.00020293673591811182, "Camera.focal_x_baseline": 30.0}
WIDE_FISHEYE = {**TUM_VI_MONO, "Camera.fx": 100.0, "Camera.fy": 100.0, "Camera.cx": 256.0, "Camera.cy": 256.0}
EQUIRECT = {"Camera.model": "equirectangular", "Camera.cols": 1920, "Camera.rows": 960}


def yaml_of(name):
    if name in PERSP:
        v = PERSP[name]
        cols, rows = (1241, 376) if name == "kitti" else (640, 480)
        return {"Camera.model": "perspective", "Camera.cols": cols, "Camera.rows": rows,
                **{f"Camera.{k}": x for k, x in zip(("fx", "fy", "cx", "cy", "k1", "k2", "p1", "p2", "k3", "focal_x_baseline"), v)}}
    return {"tum_vi": TUM_VI_MONO, "wide_fisheye": WIDE_FISHEYE, "equirect": EQUIRECT}[name]


CAMERAS = list(PERSP) + ["tum_vi", "wide_fisheye", "equirect"]


def ref_cam(cm):
    return {"model": {0: "perspective", 1: "fisheye", 2: "equirectangular"}[cm.model], "cols": cm.cols, "rows": cm.rows,
            **{k: getattr(cm, k) for k in ("fx", "fy", "cx", "cy", "focal_x_baseline")}}


def rotation(rng):
    q = rng.normal(size=4); q /= np.linalg.norm(q)
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def random_pose(rng, axis_aligned):
    if axis_aligned:   # exact camera coordinates: z = 0 and the image bounds can be hit exactly
        return R.frame_pose(np.eye(3), np.array([0.5, -0.25, 1.0]) * float(rng.integers(-2, 3)))
    return R.frame_pose(rotation(rng), rng.normal(size=3))


def to_world(P, pc):
    """camera coordinates -> world (approximately: the test does not need the inverse to be exact)"""
    Rm = P[:9].reshape(3, 3)
    return (pc - P[9:12]) @ Rm


def back_project(cm, bounds, P, u, v, z):
    if cm.model == plp.CAMERA_EQUIRECTANGULAR:
        lon = (u / cm.cols - 0.5) * 2 * math.pi
        lat = -(v / cm.rows - 0.5) * math.pi
        pc = np.array([math.cos(lat) * math.sin(lon), -math.sin(lat), math.cos(lat) * math.cos(lon)]) * z
    else:
        pc = np.array([(u - cm.cx) / cm.fx * z, (v - cm.cy) / cm.fy * z, z])
    return to_world(P, pc)


def point_scene(rng, cm, bounds, P, m, lsf):
    """m point landmarks: inside, out of every bound (just inside / outside), behind, on z = 0, ray_cos at 0.5 +- ulp, distances at
    0.7 min / 1.3 max +- ulp, landmarks seen at their creation distance, skipped ones"""
    cc = P[12:15]
    pos = np.zeros((m, 3)); nm = np.zeros((m, 3)); mn = np.zeros(m, np.float32); mx = np.zeros(m, np.float32)
    b = [float(t) for t in bounds]
    sf = R.scale_factors(1.2, 8)
    for j in range(m):
        kind = rng.integers(0, 10)
        z = float(rng.uniform(0.5, 20.0))
        u, v = rng.uniform(b[0], b[1]), rng.uniform(b[2], b[3])
        if kind == 1:   # near a bound, either side
            e = float(rng.choice([-1e-3, -1e-7, -1e-10, 0.0, 1e-10, 1e-7, 1e-3]))
            side = rng.integers(0, 4)
            if side < 2: u = b[side] + e
            else: v = b[side] + e
        p = back_project(cm, bounds, P, u, v, z)
        if kind == 2:   # far outside
            p = back_project(cm, bounds, P, u * 3 - b[1], v * 3 - b[3], z)
        if kind == 3:   # behind the camera / on z = 0
            pc = np.array([rng.normal(), rng.normal(), -abs(rng.normal()) if rng.integers(0, 2) else 0.0])
            p = to_world(P, pc)
        pos[j] = p
        d = pos[j] - cc
        dist = float(np.linalg.norm(d))
        dirn = d / max(dist, 1e-300)
        perp = np.cross(dirn, rng.normal(size=3)); perp /= np.linalg.norm(perp)
        ang = float(rng.uniform(0, 1.2))
        if kind == 4:   # ray_cos at 0.5 (60 degrees), nudged
            ang = math.pi / 3 + float(rng.choice([-1e-15, 0.0, 1e-15, -1e-9, 1e-9]))
        nm[j] = math.cos(ang) * dirn + math.sin(ang) * perp
        fd = f32(dist)
        lo, hi = fd * f32(rng.uniform(0.1, 0.9)), fd * f32(rng.uniform(1.1, 6.0))
        if kind == 5:   # 0.7 x min at the distance, +- 1 ulp
            lo = np.nextafter(f32(float(fd) / 0.7), f32(rng.choice([-np.inf, np.inf]))) if rng.integers(0, 2) else f32(float(fd) / 0.7)
        if kind == 6:   # 1.3 x max at the distance
            hi = np.nextafter(f32(float(fd) / 1.3), f32(rng.choice([-np.inf, np.inf]))) if rng.integers(0, 2) else f32(float(fd) / 1.3)
        if kind in (7, 8):   # created at this distance (landmark.cc:283-292): the level sits on the ceil boundary
            k = int(rng.integers(0, 8))
            hi = f32(dist * float(sf[k])); lo = f32(hi / sf[7])
        mn[j], mx[j] = lo, hi
    skip = (rng.uniform(size=m) < 0.1).astype(np.uint8)
    return pos, nm, mn, mx, skip


def line_scene(rng, cm, bounds, P, m):
    """m line landmarks: both end points in, one out with the midpoint in / out, one behind the camera; stale end points"""
    b = [float(t) for t in bounds]
    pos = np.zeros((m, 6)); mn = np.zeros(m, np.float32); mx = np.zeros(m, np.float32)
    for j in range(m):
        kind = rng.integers(0, 6)
        z0, z1 = float(rng.uniform(0.5, 15)), float(rng.uniform(0.5, 15))
        u0, v0 = rng.uniform(b[0], b[1]), rng.uniform(b[2], b[3])
        u1, v1 = rng.uniform(b[0], b[1]), rng.uniform(b[2], b[3])
        if kind == 1:   # end point out of the image, midpoint likely in
            u1 = b[1] + (b[1] - b[0]) * float(rng.uniform(0.01, 0.6))
        if kind == 2:   # start point far out: midpoint out too
            u0 = b[0] - (b[1] - b[0]) * float(rng.uniform(2.0, 5.0))
        p0 = back_project(cm, bounds, P, u0, v0, z0); p1 = back_project(cm, bounds, P, u1, v1, z1)
        if kind in (3, 4):   # one end behind the camera
            back = to_world(P, np.array([rng.normal(), rng.normal(), -float(rng.uniform(0.1, 3.0))]))
            if kind == 3: p1 = back
            else: p0 = back
        pos[j, :3], pos[j, 3:] = p0, p1
        d = float(np.linalg.norm(0.5 * (p0 + p1) - P[12:15]))
        mn[j] = f32(d * rng.uniform(0.3, 1.1)); mx[j] = f32(d * rng.uniform(0.9, 4.0))
    skip = (rng.uniform(size=m) < 0.1).astype(np.uint8)
    return pos, mn, mx, skip


def equirect_close(a, b):
    """D4 / D5 item 2: within 1 float ulp -- or within 1e-9 px, where the pixel is near 0 and `cols * (0.5 + lon / 2 pi)` cancels: there the
    last-bit difference of the f64 asin / atan2 (a few 1e-13 px) is more than one ulp of the tiny float result"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return within_ulp(a, b) | (np.abs(a.astype(np.float64) - b.astype(np.float64)).ravel() <= 1e-9)


def within_ulp(a, b, n=1):
    a, b = np.asarray(a, np.float32).ravel(), np.asarray(b, np.float32).ravel()
    ia, ib = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
    ia = np.where(ia < 0, -(ia & 0x7FFFFFFF), ia); ib = np.where(ib < 0, -(ib & 0x7FFFFFFF), ib)
    return np.abs(ia - ib) <= n


@pytest.fixture(scope="module")
def cams():
    return {name: plp.camera_model(yaml_of(name)) for name in CAMERAS}


def compare_points(cm, got, want, valid_only_level=True, label=""):
    v = want["valid"].astype(bool)
    assert np.array_equal(got["valid"], want["valid"]), label
    assert int(got["num_valid"]) == want["num_valid"], label
    if "level" in want and valid_only_level:
        assert np.array_equal(got["level"][v], want["level"][v]), label
    if cm.model == plp.CAMERA_EQUIRECTANGULAR:
        ok = equirect_close(got["reproj"][v], want["reproj"][v])
        assert ok.all(), (label, got["reproj"][v].ravel()[~ok], want["reproj"][v].ravel()[~ok])
        return int((got["reproj"][v] != want["reproj"][v]).any(axis=1).sum())
    assert np.array_equal(got["reproj"][v].view(np.uint32), want["reproj"][v].view(np.uint32)), label
    assert np.array_equal(got["x_right"][v].view(np.uint32), want["x_right"][v].view(np.uint32)), label
    return 0


@pytest.mark.parametrize("name", CAMERAS)
def test_points_equal_the_restatement(cams, name):
    cm = cams[name]
    bounds = cm.img_bounds
    rc = ref_cam(cm)
    mt = plp.matcher()
    lsf = R.d5_logf(f32(1.2))
    rng = np.random.default_rng(CAMERAS.index(name))
    inexact = total = 0
    for trial in range(6):
        P = random_pose(rng, trial % 2 == 0)
        m = int(rng.integers(1, 600))
        pos, nm, mn, mx, skip = point_scene(rng, cm, bounds, P, m, lsf)
        want = R.observe_points(rc, bounds, P, pos, nm, mn, mx, skip, 0.5, lsf, 8)
        got = mt.observe_landmarks(cm, P, pos, nm, mn, mx, skip, log_scale_factor=lsf, num_levels=8)
        inexact += compare_points(cm, got, want, label=(name, trial)); total += want["num_valid"]
        # reprojection only (match_current_and_last_frames, projection.cc:254-262)
        want = R.observe_points(rc, bounds, P, pos, None, None, None, skip, 0.5, lsf, 8)
        got = mt.observe_landmarks(cm, P, pos, skip=skip)
        compare_points(cm, got, want, valid_only_level=False, label=(name, trial, "reproj-only"))
    if cm.model == plp.CAMERA_EQUIRECTANGULAR:
        print(f"equirectangular: {inexact} of {total} valid reprojections differ from the glibc restatement (within 1 float ulp or 1e-9 px)")
    assert total > 0


@pytest.mark.parametrize("name", CAMERAS)
def test_lines_equal_the_restatement(cams, name):
    cm = cams[name]
    bounds = cm.img_bounds
    rc = ref_cam(cm)
    mt = plp.matcher()
    lsf = R.d5_logf(f32(2.0))
    rng = np.random.default_rng(100 + CAMERAS.index(name))
    for trial in range(4):
        P = random_pose(rng, trial % 2 == 0)
        m = int(rng.integers(1, 700))
        pos, mn, mx, skip = line_scene(rng, cm, bounds, P, m)
        want = R.observe_lines(rc, bounds, P, pos, mn, mx, skip, lsf, 2)
        got = mt.observe_landmark_lines(cm, P, pos, mn, mx, skip, log_scale_factor=lsf, num_levels=2)
        v = want["valid"].astype(bool)
        assert np.array_equal(got["valid"], want["valid"]) and int(got["num_valid"]) == want["num_valid"]
        assert np.array_equal(got["level"][v], want["level"][v])
        for k in ("reproj_sp", "reproj_ep"):   # every slot: the carried temporaries
            if cm.model == plp.CAMERA_EQUIRECTANGULAR:
                assert equirect_close(got[k], want[k]).all(), (name, trial, k)
            else:
                assert np.array_equal(got[k].view(np.uint32), want[k].view(np.uint32)), (name, trial, k)


def test_stale_end_points_across_chunk_and_wave_boundaries(cams):
    """the writer of a carried end point more than 256 and more than 1024 slots before its reader, skipped landmarks in between, a leading stale slot"""
    cm = cams["fr3"]
    bounds = cm.img_bounds
    rc = ref_cam(cm)
    P = R.frame_pose(np.eye(3), np.zeros(3))
    m = 2000
    rng = np.random.default_rng(11)
    behind = lambda: np.array([rng.normal(), rng.normal(), -float(rng.uniform(0.5, 2))])
    pos = np.zeros((m, 6)); mn = np.full(m, 0.01, np.float32); mx = np.full(m, 1e4, np.float32)
    skip = np.zeros(m, np.uint8)
    for j in range(m):   # filler: start point in, end point behind (writes only the start point); the midpoint decides
        pos[j, :3] = back_project(cm, bounds, P, rng.uniform(50, 600), rng.uniform(50, 430), float(rng.uniform(1, 3)))
        pos[j, 3:] = behind()
    skip[rng.uniform(size=m) < 0.3] = 1
    skip[0] = 0                                                           # slot 0: leading stale end point (0, 0)
    for w in (3, 700):                                                    # writers of the end point, rejected by distance
        pos[w, 3:] = back_project(cm, bounds, P, 100.0 + w / 10, 200.0, 2.0)
        skip[w] = 0; mx[w] = 1e-3
    for r in (3 + 300, 700 + 1100, 1400):                                # readers far behind their writers
        if r < m:
            skip[r] = 0
            pos[r, :3] = back_project(cm, bounds, P, 320.0, 240.0, 0.8)
            pos[r, 3:] = np.array([0.01, 0.01, -0.2])
    want = R.observe_lines(rc, bounds, P, pos, mn, mx, skip, R.d5_logf(f32(2.0)), 2)
    assert want["reproj_ep"][0].tolist() == [0, 0]
    assert want["valid"][303] and want["reproj_ep"][303].tolist() == want["reproj_ep"][3].tolist() and not want["valid"][3]
    assert want["valid"][1800] and want["reproj_ep"][1800].tolist() == want["reproj_ep"][700].tolist() and not want["valid"][700]
    got = plp.matcher().observe_landmark_lines(cm, P, pos, mn, mx, skip, log_scale_factor=R.d5_logf(f32(2.0)), num_levels=2)
    for k in ("reproj_sp", "reproj_ep"):
        assert np.array_equal(got[k].view(np.uint32), want[k].view(np.uint32)), k
    assert np.array_equal(got["valid"], want["valid"]) and int(got["num_valid"]) == want["num_valid"]


def _device_batch(cm, B, m_cap, counts, P, pos, nm, mn, mx, skip, lines, lsf, num_levels):
    import torch
    dev = torch.device("cuda:0")
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    out = dict(reproj=torch.full((B, m_cap, 2), -77.0, dtype=torch.float32, device=dev), level=torch.full((B, m_cap), -77, dtype=torch.int32, device=dev),
               valid=torch.full((B, m_cap), 77, dtype=torch.uint8, device=dev), num_valid=torch.full((B,), -1, dtype=torch.int32, device=dev))
    mt = plp.matcher()
    if lines:
        out["reproj_ep"] = torch.full((B, m_cap, 2), -77.0, dtype=torch.float32, device=dev)
        mt.observe_landmark_lines_device(cm, B, m_cap, T(P), T(pos), T(mn), T(mx), out["reproj"], out["reproj_ep"], out["level"], out["valid"],
                                         skip=T(skip), counts=T(counts), out_num_valid=out["num_valid"], log_scale_factor=lsf, num_levels=num_levels)
    else:
        out["x_right"] = torch.full((B, m_cap), -77.0, dtype=torch.float32, device=dev)
        mt.observe_landmarks_device(cm, B, m_cap, T(P), T(pos), out["reproj"], out["valid"], obs_mean_normal=T(nm), min_valid_dist=T(mn),
                                    max_valid_dist=T(mx), skip=T(skip), counts=T(counts), out_x_right=out["x_right"], out_level=out["level"],
                                    out_num_valid=out["num_valid"], log_scale_factor=lsf, num_levels=num_levels)
    torch.cuda.synchronize()
    res = {k: v.cpu().numpy() for k, v in out.items()}
    host = (mt.observe_landmark_lines(cm, P, pos, mn, mx, skip, counts, log_scale_factor=lsf, num_levels=num_levels) if lines else
            mt.observe_landmarks(cm, P, pos, nm, mn, mx, skip, counts, log_scale_factor=lsf, num_levels=num_levels))
    return res, host


@pytest.mark.parametrize("lines", [False, True])
def test_batches_ragged_counts_and_host_equals_device(cams, lines):
    cm = cams["fr1"]
    bounds = cm.img_bounds
    rc = ref_cam(cm)
    rng = np.random.default_rng(21 + lines)
    lsf = R.d5_logf(f32(2.0 if lines else 1.2))
    nl = 2 if lines else 8
    for B, m_cap in ((1, 20000 if not lines else 5000), (64, 300)):
        counts = np.array([m_cap] if B == 1 else rng.integers(0, m_cap + 1, B), np.int32)
        counts[-1] = min(counts[-1], m_cap)
        P = np.stack([random_pose(rng, b % 3 == 0) for b in range(B)])
        w = 6 if lines else 3
        pos = np.full((B, m_cap, w), np.nan); nm = np.full((B, m_cap, 3), np.nan)
        mn = np.full((B, m_cap), np.nan, np.float32); mx = np.full((B, m_cap), np.nan, np.float32); skip = np.ones((B, m_cap), np.uint8)
        for b in range(B):
            n = int(counts[b])
            if lines:
                pos[b, :n], mn[b, :n], mx[b, :n], skip[b, :n] = line_scene(rng, cm, bounds, P[b], n)
            else:
                pos[b, :n], nm[b, :n], mn[b, :n], mx[b, :n], skip[b, :n] = point_scene(rng, cm, bounds, P[b], n, lsf)
        got, host = _device_batch(cm, B, m_cap, counts, P, pos, nm, mn, mx, skip, lines, lsf, nl)
        for b in range(B):
            n = int(counts[b])
            assert (got["valid"][b, n:] == 77).all() and (got["level"][b, n:] == -77).all(), "slots past the count were written"
            for k in host:   # the host wrapper's outputs start at 0: slots past the count stay 0
                if k != "num_valid":
                    assert (host[k][b, n:] == 0).all(), ("host slots past the count were written", b, k)
            if lines:
                want = R.observe_lines(rc, bounds, P[b], pos[b, :n], mn[b, :n], mx[b, :n], skip[b, :n], lsf, nl)
                keys = ("reproj", "reproj_ep")
            else:
                want = R.observe_points(rc, bounds, P[b], pos[b, :n], nm[b, :n], mn[b, :n], mx[b, :n], skip[b, :n], 0.5, lsf, nl)
                keys = ("reproj", "x_right")
            v = want["valid"].astype(bool)
            assert np.array_equal(got["valid"][b, :n], want["valid"]) and got["num_valid"][b] == want["num_valid"], b
            assert np.array_equal(got["level"][b, :n][v], want["level"][v]), b
            assert np.array_equal(host["valid"][b, :n], want["valid"]) and host["num_valid"][b] == want["num_valid"], b
            assert np.array_equal(host["level"][b, :n][v], got["level"][b, :n][v]), b
            for k in keys:
                wk = want["reproj_sp" if (lines and k == "reproj") else k]
                hk = host["reproj_sp" if (lines and k == "reproj") else k]
                sel = slice(None) if lines else v
                assert np.array_equal(got[k][b, :n][sel].view(np.uint32), np.asarray(wk, np.float32)[sel].view(np.uint32)), (b, k)
                assert np.array_equal(hk[b, :n][sel].view(np.uint32), got[k][b, :n][sel].view(np.uint32)), (b, k)


def _raw_args(cm, B, m_cap, arrays):
    a = plp.observe_args_c()
    a.camera = plp.camera_model_c.from_buffer_copy(cm)
    a.img_bounds[:] = [float(t) for t in cm.img_bounds]
    a.ray_cos_thr, a.log_scale_factor, a.num_levels, a.B, a.m_cap = 0.5, float(R.d5_logf(f32(1.2))), 8, B, m_cap
    for k, v in arrays.items():
        setattr(a, k, v.ctypes.data if v is not None else None)
    return a


@pytest.mark.parametrize("lines", [False, True])
def test_host_entry_leaves_unwritten_slots_alone(cams, lines):
    """plp_observe_landmark[_line]s_host stages through the context's reused slab: slots past counts[b], and the point slots the kernel does not
    write (reproj / x_right / level of invalid landmarks), must come back as the caller's own values -- not what an earlier call left in the slab"""
    cm = cams["fr1"]
    bounds = cm.img_bounds
    rc = ref_cam(cm)
    rng = np.random.default_rng(51 + lines)
    L, mt = plp.lib(), plp.matcher()
    entry = L.plp_observe_landmark_lines_host if lines else L.plp_observe_landmarks_host
    lsf = R.d5_logf(f32(2.0 if lines else 1.2))
    B, m_cap = 4, 400
    P = np.stack([random_pose(rng, False) for _ in range(B)])
    pos = np.zeros((B, m_cap, 6 if lines else 3)); nm = np.zeros((B, m_cap, 3)); mn = np.zeros((B, m_cap), np.float32); mx = np.zeros((B, m_cap), np.float32)
    skip = np.zeros((B, m_cap), np.uint8)
    for b in range(B):
        if lines:
            pos[b], mn[b], mx[b], skip[b] = line_scene(rng, cm, bounds, P[b], m_cap)
        else:
            pos[b], nm[b], mn[b], mx[b], skip[b] = point_scene(rng, cm, bounds, P[b], m_cap, lsf)

    def run(counts, fill):
        outs = dict(out_reproj=np.full((B, m_cap, 2), fill, np.float32), out_reproj2=np.full((B, m_cap, 2), fill, np.float32),
                    out_x_right=np.full((B, m_cap), fill, np.float32), out_level=np.full((B, m_cap), int(fill), np.int32),
                    out_valid=np.full((B, m_cap), 77, np.uint8), out_num_valid=np.full(B, -1, np.int32))
        a = _raw_args(cm, B, m_cap, dict(pose=P, pos_w=pos, obs_mean_normal=None if lines else nm, min_valid_dist=mn, max_valid_dist=mx, skip=skip,
                                         counts=counts, **outs))
        a.log_scale_factor, a.num_levels = float(lsf), 2 if lines else 8
        assert entry(mt._h, C.byref(a)) == plp.PLP_OK
        return outs

    run(np.full(B, m_cap, np.int32), 5.0)            # leaves every slot of the slab written
    counts = np.array([0, 1, 257, 399], np.int32)
    outs = run(counts, -123.0)
    for b in range(B):
        n = int(counts[b])
        for k, v in outs.items():
            if k != "out_num_valid":
                want = 77 if k == "out_valid" else -123
                assert (v[b, n:] == want).all(), ("slot past the count changed", b, k)
        if lines:
            w = R.observe_lines(rc, bounds, P[b], pos[b, :n], mn[b, :n], mx[b, :n], skip[b, :n], lsf, 2)
        else:
            w = R.observe_points(rc, bounds, P[b], pos[b, :n], nm[b, :n], mn[b, :n], mx[b, :n], skip[b, :n], 0.5, lsf, 8)
        v = w["valid"].astype(bool)
        assert np.array_equal(outs["out_valid"][b, :n], w["valid"]) and outs["out_num_valid"][b] == w["num_valid"], b
        assert (outs["out_level"][b, :n][~v] == -123).all(), b            # level: valid slots only
        if not lines:                                                      # points: reproj / x_right of valid slots only
            assert (outs["out_reproj"][b, :n][~v] == -123).all() and (outs["out_x_right"][b, :n][~v] == -123).all(), b
        assert (outs["out_x_right"][b] == -123).all() if lines else (outs["out_reproj2"][b] == -123).all()   # ignored arrays stay untouched


def test_empty_problems_and_invalid_arguments(cams):
    cm = cams["fr3"]
    mt = plp.matcher()
    L = plp.lib()
    P = np.zeros((2, 15)); pos = np.zeros((2, 4, 6)); mn = np.ones((2, 4), np.float32); mx = np.ones((2, 4), np.float32)
    rp = np.zeros((2, 4, 2), np.float32); rp2 = np.zeros((2, 4, 2), np.float32); lv = np.zeros((2, 4), np.int32); va = np.zeros((2, 4), np.uint8)
    num = np.full(2, 9, np.int32)
    full = dict(pose=P, pos_w=pos, min_valid_dist=mn, max_valid_dist=mx, out_reproj=rp, out_reproj2=rp2, out_level=lv, out_valid=va, out_num_valid=num)
    # m_cap = 0: OK, counts 0, on both entries
    for entry in (L.plp_observe_landmarks_host, L.plp_observe_landmark_lines_host):
        num[:] = 9
        assert entry(mt._h, C.byref(_raw_args(cm, 2, 0, full))) == plp.PLP_OK and num.tolist() == [0, 0]
    import torch
    d_num = torch.full((2,), 9, dtype=torch.int32, device="cuda:0")
    a = _raw_args(cm, 2, 0, dict(pose=P))
    a.pose, a.pos_w, a.out_reproj, a.out_reproj2, a.out_valid, a.out_level, a.min_valid_dist, a.max_valid_dist = [d_num.data_ptr()] * 8
    a.out_num_valid = d_num.data_ptr()
    assert L.plp_observe_landmark_lines_device(mt._h, C.byref(a), torch.cuda.current_stream().cuda_stream) == plp.PLP_OK
    torch.cuda.synchronize()
    assert d_num.cpu().tolist() == [0, 0]
    # invalid: checked before the empty fast path
    bad_model = _raw_args(cm, 2, 0, full); bad_model.camera.model = 7
    no_pose = _raw_args(cm, 2, 4, {**full, "pose": None})
    no_reproj2 = _raw_args(cm, 2, 4, {**full, "out_reproj2": None})
    zero_b = _raw_args(cm, 0, 4, full)
    neg_b = _raw_args(cm, -1, 0, full)
    no_levels = _raw_args(cm, 2, 0, full); no_levels.num_levels = 0
    for a, entries in ((bad_model, "pl"), (no_pose, "pl"), (no_reproj2, "l"), (zero_b, "pl"), (neg_b, "pl"), (no_levels, "pl")):
        num[:] = 9
        for e in entries:
            entry = L.plp_observe_landmark_lines_host if e == "l" else L.plp_observe_landmarks_host
            assert entry(mt._h, C.byref(a)) == plp.PLP_ERR_INVALID_ARG
            assert num.tolist() == [9, 9]
    assert L.plp_observe_landmarks_host(None, C.byref(_raw_args(cm, 2, 4, full))) == plp.PLP_ERR_INVALID_ARG
    assert L.plp_observe_landmarks_host(mt._h, None) == plp.PLP_ERR_INVALID_ARG
    # points with normals need the distances and out_level
    nm = np.zeros((2, 4, 3))
    assert L.plp_observe_landmarks_host(mt._h, C.byref(_raw_args(cm, 2, 4, {**full, "obs_mean_normal": nm, "out_level": None}))) == plp.PLP_ERR_INVALID_ARG
    with pytest.raises(plp.PlpError):
        mt.observe_landmarks(bad_model.camera, P[0], np.zeros((3, 3)), img_bounds=cm.img_bounds)


def test_infinite_ratio_gives_level_zero(cams):
    """D5 item 4: a landmark at the camera centre with min_valid_dist_ 0 (equirectangular: always in the image, ray_cos NaN passes) has
    ratio = inf; x86's int cast clamps the level to 0, a saturating cast would give the top level"""
    cm = cams["equirect"]
    P = R.frame_pose(np.eye(3), np.array([0.5, -1.0, 2.0]))
    pos = np.array([P[12:15], P[12:15] + [0, 0, 1.0]])
    got = plp.matcher().observe_landmarks(cm, P, pos, np.array([[0, 0, 1.0], [0, 0, 1.0]]), np.zeros(2, np.float32), np.array([3.0, 1000.0], np.float32),
                                          log_scale_factor=R.d5_logf(f32(1.2)), num_levels=8)
    assert got["valid"].tolist() == [1, 1] and got["level"].tolist() == [0, 7]


def _kp_scene(rng, reproj, level, valid, desc, n_extra, cols, rows):
    """key points of the current frame near the valid reprojections (and some elsewhere), descriptors close to the landmarks'"""
    idx = np.flatnonzero(valid)
    idx = idx[rng.uniform(size=len(idx)) < 0.8]
    n = len(idx) + n_extra
    kps = np.zeros(n, O.KP_DTYPE)
    kps["x"][:len(idx)] = reproj[idx, 0] + rng.normal(0, 2, len(idx)); kps["y"][:len(idx)] = reproj[idx, 1] + rng.normal(0, 2, len(idx))
    kps["octave"][:len(idx)] = np.clip(level[idx] + rng.integers(-1, 2, len(idx)), 0, 7)
    kps["x"][len(idx):] = rng.uniform(0, cols, n_extra); kps["y"][len(idx):] = rng.uniform(0, rows, n_extra)
    kps["octave"][len(idx):] = rng.integers(0, 8, n_extra)
    kps["angle"] = rng.uniform(0, 360, n).astype(np.float32)
    d = np.concatenate([desc[idx], rng.integers(0, 256, (n_extra, 32), dtype=np.uint8)])
    flip = rng.integers(0, 32, n)
    d[np.arange(n), flip] ^= (np.uint8(1) << rng.integers(0, 8, n).astype(np.uint8))
    return kps, d


@pytest.mark.parametrize("name", ["fr1", "tum_vi"])
def test_end_to_end_into_the_matcher_points(cams, name):
    """observe on the device -> its output pointers straight into plp_match_device (LANDMARKS), against restatement -> oracle"""
    import torch
    cm = cams[name]
    bounds = cm.img_bounds
    rc = ref_cam(cm)
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(31)
    lsf = R.d5_logf(f32(1.2))
    B, m_cap, n_cap = 6, 800, 900
    SF = R.scale_factors(1.2, 8)
    grid = cm.grid()
    P = np.stack([random_pose(rng, False) for _ in range(B)])
    counts = rng.integers(200, m_cap + 1, B).astype(np.int32)
    pos = np.zeros((B, m_cap, 3)); nm = np.zeros((B, m_cap, 3)); mn = np.zeros((B, m_cap), np.float32); mx = np.zeros((B, m_cap), np.float32)
    skip = np.ones((B, m_cap), np.uint8)
    q_desc = rng.integers(0, 256, (B, m_cap, 32), dtype=np.uint8)
    for b in range(B):
        n = int(counts[b])
        pos[b, :n], nm[b, :n], mn[b, :n], mx[b, :n], skip[b, :n] = point_scene(rng, cm, bounds, P[b], n, lsf)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    o_rp = torch.zeros((B, m_cap, 2), dtype=torch.float32, device=dev); o_xr = torch.zeros((B, m_cap), dtype=torch.float32, device=dev)
    o_lv = torch.zeros((B, m_cap), dtype=torch.int32, device=dev); o_va = torch.zeros((B, m_cap), dtype=torch.uint8, device=dev)
    mt = plp.matcher(0.8, True)
    mt.observe_landmarks_device(cm, B, m_cap, T(P), T(pos), o_rp, o_va, obs_mean_normal=T(nm), min_valid_dist=T(mn), max_valid_dist=T(mx), skip=T(skip),
                                counts=T(counts), out_x_right=o_xr, out_level=o_lv, log_scale_factor=lsf, num_levels=8)
    wants, tk = [], []
    t_kps = np.zeros((B, n_cap), O.KP_DTYPE); t_desc = np.zeros((B, n_cap, 32), np.uint8); t_counts = np.zeros(B, np.int32)
    for b in range(B):
        n = int(counts[b])
        w = R.observe_points(rc, bounds, P[b], pos[b, :n], nm[b, :n], mn[b, :n], mx[b, :n], skip[b, :n], 0.5, lsf, 8)
        kps, d = _kp_scene(rng, w["reproj"], w["level"], w["valid"], q_desc[b, :n], 150, cm.cols, cm.rows)
        kps, d = kps[:n_cap], d[:n_cap]
        t_kps[b, :len(kps)] = kps; t_desc[b, :len(kps)] = d; t_counts[b] = len(kps)
        wants.append(w); tk.append((kps, d))
    fields = dict(t_kps=T(t_kps.view(np.uint8)), t_desc=T(t_desc), t_x_right=T(np.full((B, n_cap), -1, np.float32)), t_occupied=T(np.zeros((B, n_cap), np.uint8)),
                  t_counts=T(t_counts), q_valid=o_va, q_reproj=o_rp, q_x_right=o_xr, q_level=o_lv, q_desc=T(q_desc),
                  q_has_obs=T(np.ones((B, m_cap), np.uint8)), q_counts=T(counts))
    out_match = torch.full((B, n_cap), -7, dtype=torch.int32, device=dev); out_num = torch.zeros(B, dtype=torch.int32, device=dev)
    mt.match_device(plp.MODE_LANDMARKS, n_cap, m_cap, fields, out_match, out_num, margin=10.0, scale_factors=SF, grid=grid, B=B)
    torch.cuda.synchronize()
    om, on = out_match.cpu().numpy(), out_num.cpu().numpy()
    total = 0
    for b in range(B):
        n = int(counts[b]); w = wants[b]; kps, d = tk[b]
        want, wn = O.match_frame_and_landmarks(O.grid6(grid), kps, d, np.full(len(kps), -1, np.float32), np.zeros(len(kps), np.uint8), SF, w["valid"],
                                               w["reproj"], w["x_right"], w["level"], q_desc[b, :n], np.ones(n, np.uint8), 10.0, 0.8)
        assert on[b] == wn and np.array_equal(om[b, :len(kps)], want), b
        total += wn
    assert total > 50, total


def test_end_to_end_into_the_matcher_lines(cams):
    """observe_landmark_lines on the device -> plp_match_device (LANDMARKS_LINE), against restatement -> oracle (stale end points included)"""
    import torch
    cm = cams["fr1"]
    bounds = cm.img_bounds
    rc = ref_cam(cm)
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(41)
    lsf = R.d5_logf(f32(2.0))
    sf_lsd = np.array([1.0, 2.0], np.float32)
    B, m_cap, n_cap = 8, 300, 256
    P = np.stack([random_pose(rng, False) for _ in range(B)])
    counts = rng.integers(50, m_cap + 1, B).astype(np.int32)
    pos = np.zeros((B, m_cap, 6)); mn = np.zeros((B, m_cap), np.float32); mx = np.zeros((B, m_cap), np.float32); skip = np.ones((B, m_cap), np.uint8)
    q_desc = rng.integers(0, 256, (B, m_cap, 32), dtype=np.uint8)
    for b in range(B):
        n = int(counts[b])
        pos[b, :n], mn[b, :n], mx[b, :n], skip[b, :n] = line_scene(rng, cm, bounds, P[b], n)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    o_sp = torch.zeros((B, m_cap, 2), dtype=torch.float32, device=dev); o_ep = torch.zeros((B, m_cap, 2), dtype=torch.float32, device=dev)
    o_lv = torch.zeros((B, m_cap), dtype=torch.int32, device=dev); o_va = torch.zeros((B, m_cap), dtype=torch.uint8, device=dev)
    mt = plp.matcher(0.8, False)
    mt.observe_landmark_lines_device(cm, B, m_cap, T(P), T(pos), T(mn), T(mx), o_sp, o_ep, o_lv, o_va, skip=T(skip), counts=T(counts),
                                     log_scale_factor=lsf, num_levels=2)
    t_kl = np.zeros((B, n_cap), O.KL_DTYPE); t_desc = np.zeros((B, n_cap, 32), np.uint8); t_oct = np.zeros((B, n_cap), np.int32); t_counts = np.zeros(B, np.int32)
    wants, tl = [], []
    for b in range(B):
        n = int(counts[b])
        w = R.observe_lines(rc, bounds, P[b], pos[b, :n], mn[b, :n], mx[b, :n], skip[b, :n], lsf, 2)
        idx = np.flatnonzero(w["valid"])[:n_cap - 40]
        k = len(idx) + 40
        kl = np.zeros(k, O.KL_DTYPE)
        src_sp = np.concatenate([w["reproj_sp"][idx], rng.uniform(0, 640, (40, 2))]); src_ep = np.concatenate([w["reproj_ep"][idx], rng.uniform(0, 480, (40, 2))])
        kl["startPointX"], kl["startPointY"] = src_sp[:, 0] + rng.normal(0, 2, k), src_sp[:, 1] + rng.normal(0, 2, k)
        kl["endPointX"], kl["endPointY"] = src_ep[:, 0] + rng.normal(0, 2, k), src_ep[:, 1] + rng.normal(0, 2, k)
        kl["octave"] = rng.integers(0, 2, k)
        d = np.concatenate([q_desc[b, idx], rng.integers(0, 256, (40, 32), dtype=np.uint8)])
        d[np.arange(k), rng.integers(0, 32, k)] ^= np.uint8(4)
        oct_ = rng.integers(0, 8, k).astype(np.int32)
        t_kl[b, :k] = kl; t_desc[b, :k] = d; t_oct[b, :k] = oct_; t_counts[b] = k
        wants.append(w); tl.append((kl, d, oct_))
    fields = dict(t_kl=T(t_kl.view(np.uint8)), t_desc=T(t_desc), t_kp_octave=T(t_oct), t_occupied=T(np.zeros((B, n_cap), np.uint8)), t_counts=T(t_counts),
                  q_valid=o_va, q_reproj=o_sp, q_reproj2=o_ep, q_level=o_lv, q_desc=T(q_desc), q_has_obs=T(np.ones((B, m_cap), np.uint8)), q_counts=T(counts))
    out_match = torch.full((B, n_cap), -7, dtype=torch.int32, device=dev); out_num = torch.zeros(B, dtype=torch.int32, device=dev)
    mt.match_device(plp.MODE_LANDMARKS_LINE, n_cap, m_cap, fields, out_match, out_num, margin=12.0, scale_factors=sf_lsd, B=B)
    torch.cuda.synchronize()
    om, on = out_match.cpu().numpy(), out_num.cpu().numpy()
    total = 0
    for b in range(B):
        n = int(counts[b]); w = wants[b]; kl, d, oct_ = tl[b]
        want, wn = O.match_frame_and_landmarks_line(kl, d, oct_, np.zeros(len(kl), np.uint8), sf_lsd, w["valid"], w["reproj_sp"], w["reproj_ep"],
                                                    w["level"], q_desc[b, :n], np.ones(n, np.uint8), 12.0, 0.8)
        assert on[b] == wn and np.array_equal(om[b, :len(kl)], want), b
        total += wn
    assert total > 20, total
