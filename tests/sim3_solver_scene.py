"""Seeded scenes for solve::sim3_solver (tests/test_sim3_solver_cpu.py, tests/test_gpu_sim3_solver.py): two key-frame poses whose camera
frames are related by a known Sim3, n common points 3-9 m in front of key frame 1, 1 cm noise on the second set, a share of gross outliers,
octaves 0-7 with sigma 1.2^level, holes in `valid`, and distinct sample triples."""
import numpy as np

CAMERAS = {
    "perspective": {"Camera.model": "perspective", "Camera.cols": 640, "Camera.rows": 480, "Camera.fx": 517.3, "Camera.fy": 516.5, "Camera.cx": 318.6,
                    "Camera.cy": 255.3, "Camera.k1": 0.0, "Camera.k2": 0.0, "Camera.p1": 0.0, "Camera.p2": 0.0, "Camera.k3": 0.0},
    "fisheye": {"Camera.model": "fisheye", "Camera.cols": 512, "Camera.rows": 512, "Camera.fx": 190.97, "Camera.fy": 190.97, "Camera.cx": 254.93,
                "Camera.cy": 256.89, "Camera.k1": 0.0, "Camera.k2": 0.0, "Camera.k3": 0.0, "Camera.k4": 0.0},
    "equirectangular": {"Camera.model": "equirectangular", "Camera.cols": 1920, "Camera.rows": 960},
}
MODEL_ID = {"perspective": 0, "fisheye": 1, "equirectangular": 2}
SIGMA_SQ = ((np.float32(1.2) ** np.arange(8)).astype(np.float32) ** 2).astype(np.float32)      # level_sigma_sq_ (orb_params.cc)


def ref_camera(name):
    """the camera as tests/sim3_solver_ref.py reads it"""
    y = CAMERAS[name]
    c = dict(model=MODEL_ID[name], cols=float(y["Camera.cols"]), rows=float(y["Camera.rows"]))
    for k in ("fx", "fy", "cx", "cy"):
        c[k] = float(y.get("Camera." + k, 0.0))
    return c


def rotation(rng, max_angle):
    axis = rng.standard_normal(3)
    axis /= np.linalg.norm(axis)
    a = rng.uniform(-max_angle, max_angle)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * (K @ K)


def pose_row(R, t):
    return np.concatenate([R.reshape(-1), t, -R.T @ t])


def problem(seed, n_valid, n_slots=None, outliers=0.4, fix_scale=False, iters=200, behind_own=0, noise=0.01, all_outliers=False):
    """one problem: dict(valid, pos_w_1, pos_w_2, octave_1, octave_2 per slot, pose_1, pose_2, sigma_sq_1/2, samples (iters, 3), iters, truth=(s, R, t)
    of X2 = s R X1 + t, is_outlier per common point)"""
    rng = np.random.default_rng(seed)
    n_slots = n_valid if n_slots is None else n_slots
    assert n_slots >= n_valid
    valid = np.zeros(n_slots, np.uint8)
    valid[np.sort(rng.choice(n_slots, n_valid, replace=False))] = 1
    # camera-frame points of key frame 1: inside a 40 degree cone, 3-9 m deep
    depth = rng.uniform(3.0, 9.0, n_slots)
    x1 = np.stack([depth * np.tan(rng.uniform(-0.35, 0.35, n_slots)), depth * np.tan(rng.uniform(-0.25, 0.25, n_slots)), depth], 1)
    s = 1.0 if fix_scale else rng.uniform(0.8, 1.25)
    R, t = rotation(rng, 0.12), rng.uniform(-0.3, 0.3, 3)
    x2 = s * x1 @ R.T + t + rng.normal(0.0, noise, (n_slots, 3))
    is_out = rng.random(n_slots) < (1.0 if all_outliers else outliers)
    far = np.stack([rng.uniform(-3, 3, n_slots), rng.uniform(-2, 2, n_slots), rng.uniform(3.0, 9.0, n_slots)], 1)
    x2[is_out] = far[is_out]
    common = np.flatnonzero(valid)
    for k in common[:behind_own]:                        # a point behind its own camera (key frame 1): never an inlier (D13)
        x1[k, 2] = -x1[k, 2]
        is_out[k] = True
    R1, t1 = rotation(rng, 3.0), rng.uniform(-5, 5, 3)
    R2, t2 = rotation(rng, 3.0), rng.uniform(-5, 5, 3)
    pos_w_1 = (x1 - t1) @ R1                             # R1^T (x - t1)
    pos_w_2 = (x2 - t2) @ R2
    garbage = valid == 0                                 # what a hole holds must not matter
    pos_w_1[garbage] = rng.uniform(-1e3, 1e3, (int(garbage.sum()), 3))
    pos_w_2[garbage] = np.nan
    octave_1 = rng.integers(0, 8, n_slots).astype(np.int32)
    octave_2 = rng.integers(0, 8, n_slots).astype(np.int32)
    samples = np.zeros((iters, 3), np.int32)
    if n_valid >= 3:
        for i in range(iters):
            samples[i] = rng.choice(n_valid, 3, replace=False)
    return dict(valid=valid, pos_w_1=pos_w_1, pos_w_2=pos_w_2, octave_1=octave_1, octave_2=octave_2, pose_1=pose_row(R1, t1), pose_2=pose_row(R2, t2),
                sigma_sq_1=SIGMA_SQ, sigma_sq_2=SIGMA_SQ, samples=samples, iters=iters, truth=(s, R, t), is_outlier=is_out[common], n_valid=n_valid)


def pack(problems, n_cap=None, sentinel=False):
    """the problems of one call as the library's arrays: dict(valid (P, n_cap), pos_w_1, pos_w_2, octave_1, octave_2, pose_1, pose_2, counts, samples).
    All problems must share `iters`.  Slots at or above a problem's count hold garbage."""
    P = len(problems)
    n_cap = max(len(q["valid"]) for q in problems) if n_cap is None else n_cap
    iters = problems[0]["iters"]
    rng = np.random.default_rng(99)
    a = dict(valid=np.ones((P, n_cap), np.uint8), pos_w_1=rng.uniform(-9, 9, (P, n_cap, 3)), pos_w_2=rng.uniform(-9, 9, (P, n_cap, 3)),
             octave_1=np.full((P, n_cap), 3, np.int32), octave_2=np.full((P, n_cap), 99, np.int32), pose_1=np.zeros((P, 15)), pose_2=np.zeros((P, 15)),
             counts=np.zeros(P, np.int32), samples=np.zeros((P, iters, 3), np.int32))
    for p, q in enumerate(problems):
        m = len(q["valid"])
        assert q["iters"] == iters and m <= n_cap
        for k in ("valid", "pos_w_1", "pos_w_2", "octave_1", "octave_2"):
            a[k][p, :m] = q[k]
        a["pose_1"][p], a["pose_2"][p], a["counts"][p], a["samples"][p] = q["pose_1"], q["pose_2"], m, q["samples"]
    return a
