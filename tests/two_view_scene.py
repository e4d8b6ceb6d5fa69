"""Seeded two-view scenes for solve::essential_solver (tests/test_two_view_cpu.py, tests/test_gpu_two_view.py): frame 1 at the origin, frame 2
at a known (R, t) of X_2 = R X_1 + t, a cloud 4 to 8 units from frame 1 in the directions its camera model sees, a baseline that gives 3 to 6
degrees of parallax at the middle of the cloud, bearing noise, a stated share of mismatched pairs, holes in the match table (slots without a
match), a permuted frame 2 with key points no match names, and distinct sample octuples.

The solver sees bearings only; the camera model decides where they point (as tests/pnp_solver_scene.py):
  perspective      within 35 degrees of the optical axis
  fisheye          within 95 degrees of it (a few with z < 0)
  equirectangular  the whole sphere"""
import numpy as np

from pnp_solver_scene import MAX_ANGLE, MODELS, directions, rotation  # noqa: F401

SIZES = (8, 64, 200, 500)
NOISES = (0.0, 1e-3, 2e-3)


def unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def problem(seed, n_matches, model="perspective", n_slots=None, noise=0.0, mismatch=0.0, iters=24, kind="cloud"):
    """one problem: dict(bearing_1 (n_slots, 3), bearing_2 (m, 3), match (n_slots,), samples (iters, 8), iters, truth=(R, t), is_mismatch per
    match, noise, model, kind).  kind: cloud, planar (all points in one plane), rotation (no baseline), near_rotation (a twentieth of it)."""
    rng = np.random.default_rng(seed)
    n_slots = n_matches if n_slots is None else n_slots
    assert n_slots >= n_matches
    R = rotation(rng, np.deg2rad(8.0))
    parallax = np.deg2rad(rng.uniform(3.0, 6.0))
    t = unit(rng.standard_normal(3)) * (6.0 * parallax)
    if kind == "rotation":
        t = np.zeros(3)
    if kind == "near_rotation":
        t = t * 0.05                                                     # a twentieth of the baseline: 0.15 to 0.3 degrees of parallax
    d = directions(rng, n_slots, MAX_ANGLE[model])
    X1 = d * rng.uniform(4.0, 8.0, n_slots)[:, None]
    if kind == "planar":
        nrm = unit(np.array([0.2, -0.1, 1.0]))
        X1 = d * (6.0 / (d @ nrm))[:, None]                              # the plane nrm . X = 6; a bearing almost in the plane points the other way
    X2 = X1 @ R.T + t
    m = n_slots + 5                                                      # five key points of frame 2 that no match names
    where = rng.permutation(m)[:n_slots]                                 # slot s is key point where[s] of frame 2
    bearing_1 = unit(X1 + noise * rng.standard_normal((n_slots, 3)) * np.linalg.norm(X1, axis=1, keepdims=True))
    bearing_2 = unit(rng.standard_normal((m, 3)))
    bearing_2[where] = unit(X2 + noise * rng.standard_normal((n_slots, 3)) * np.linalg.norm(X2, axis=1, keepdims=True))
    match = np.full(n_slots, -1, np.int32)
    slots = np.sort(rng.choice(n_slots, n_matches, replace=False))       # holes: a match's index differs from its slot
    match[slots] = where[slots]
    is_mis = rng.random(n_matches) < mismatch
    match[slots[is_mis]] = rng.integers(0, m, int(is_mis.sum()))
    samples = np.zeros((iters, 8), np.int32)
    for i in range(iters):
        samples[i] = rng.choice(n_matches, 8, replace=False) if n_matches >= 8 else np.arange(8)
    return dict(bearing_1=bearing_1, bearing_2=bearing_2, match=match, samples=samples, iters=iters, truth=(R, t), is_mismatch=is_mis, noise=noise,
                model=model, kind=kind, seed=seed)


def scenes():
    """name -> problem: every size with every camera model, every noise level and mismatch shares from 0 to 50 %, and the special scenes"""
    out = {}
    k = 0
    for n in SIZES:
        for model in MODELS:
            noise = NOISES[k % 3]
            mismatch = (0.0, 0.2, 0.35, 0.5)[k % 4] if n > 8 else 0.0
            out[f"{model}_{n}"] = problem(100 + k, n, model, n_slots=n + (k % 3) * 7, noise=noise, mismatch=mismatch, iters=8 if n >= 200 else 24)
            k += 1
    out["planar"] = problem(300, 120, "perspective", n_slots=130, noise=1e-3, mismatch=0.1, kind="planar")
    out["rotation"] = problem(301, 120, "fisheye", n_slots=120, noise=1e-3, mismatch=0.1, kind="rotation")
    out["all_mismatched"] = problem(302, 60, "equirectangular", mismatch=1.0)
    out["seven"] = problem(303, 7, "perspective", n_slots=12)
    out["none"] = problem(304, 0, "perspective", n_slots=9)
    return out


ANCHORS = ("perspective_64", "fisheye_64", "equirectangular_64", "perspective_200", "fisheye_200", "planar")   # the six scenes held against numpy's svd


def degenerate_problem():
    """the degenerate samples in one problem: iteration 0 a bad index, 1 a repeated index, 2 a negative index, 3 a sample of exact matches,
    4 the same sample again (a tie), 5 eight matches of one point (A^T A of rank one: the null vector is whichever column the Jacobi leaves last), 6 the sample
    of 3 in another order, 7 another sample of exact matches"""
    q = problem(71, 40, "equirectangular", n_slots=48, mismatch=0.2, iters=8)
    slots = np.flatnonzero(q["match"] >= 0)
    good = np.flatnonzero(~q["is_mismatch"])
    good = good[good > 18]
    for k in range(10, 18):                                              # eight equal pairs
        q["bearing_1"][slots[k]] = q["bearing_1"][slots[10]]
        q["bearing_2"][q["match"][slots[k]]] = q["bearing_2"][q["match"][slots[10]]]
    q["samples"][0] = [0, 5, 40, 7, 1, 2, 3, 4]
    q["samples"][1] = [4, 9, 4, 8, 1, 2, 3, 5]
    q["samples"][2] = [0, 5, -1, 7, 1, 2, 3, 4]
    q["samples"][3] = good[:8]
    q["samples"][4] = good[:8]
    q["samples"][5] = np.arange(10, 18)
    q["samples"][6] = good[:8][::-1]
    q["samples"][7] = good[3:11]
    return q


def nan_problem():
    """one NaN bearing among the matches: its residuals pass both comparisons (:221, :240) and make every score a NaN, which never wins (:87)"""
    q = problem(72, 30, "perspective", n_slots=34, iters=6)
    q["bearing_1"][np.flatnonzero(q["match"] >= 0)[11]] = np.nan
    return q


def pack(problems, n_cap=None, m_cap=None):
    """the [P][n_cap] / [P][m_cap] arrays of plp_essential_ransac_args for problems of one iteration count: slots at or above a problem's own
    hold matches that counts_1 hides, key points of frame 2 at or above its own are named by such slots only"""
    P = len(problems)
    n_cap = max(len(q["match"]) for q in problems) if n_cap is None else n_cap
    m_cap = max(len(q["bearing_2"]) for q in problems) if m_cap is None else m_cap
    iters = problems[0]["iters"]
    a = dict(bearing_1=np.full((P, n_cap, 3), 0.5), bearing_2=np.full((P, m_cap, 3), 0.5), match=np.zeros((P, n_cap), np.int32),
             samples=np.zeros((P, iters, 8), np.int32), counts_1=np.zeros(P, np.int32), counts_2=np.zeros(P, np.int32))
    for p, q in enumerate(problems):
        n, m = len(q["match"]), len(q["bearing_2"])
        assert q["iters"] == iters and n <= n_cap and m <= m_cap
        a["bearing_1"][p, :n], a["bearing_2"][p, :m], a["match"][p, :n] = q["bearing_1"], q["bearing_2"], q["match"]
        a["samples"][p] = q["samples"]
        a["counts_1"][p], a["counts_2"][p] = n, m
    return a


def run_ref(q, recompute=True, samples="given", seed=0, p=0, linalg="jacobi"):
    import two_view_ref as TR
    return TR.find_via_ransac(q["bearing_1"], q["bearing_2"], q["match"], iters=q["iters"], recompute=recompute,
                              samples=q["samples"] if samples == "given" else None, seed=seed, p=p, linalg=linalg)


# ---------------------------------------------------------------------------------------------------------------- scenes for the pose entry
from sim3_solver_scene import CAMERAS, ref_camera  # noqa: E402

POSE_MAX_ANGLE = {"perspective": np.deg2rad(22.0), "fisheye": np.deg2rad(48.0), "equirectangular": np.pi}


def project(cam, d):
    """the undistorted key point of a bearing (n, 3): camera::*::reproject_to_image without distortion, as float32 (x, y)"""
    if cam["model"] == 2:
        lon, lat = np.arctan2(d[:, 0], d[:, 2]), -np.arcsin(np.clip(d[:, 1], -1.0, 1.0))
        uv = np.stack([cam["cols"] * (0.5 + lon / (2 * np.pi)), cam["rows"] * (0.5 - lat / np.pi)], 1)
    else:
        with np.errstate(all="ignore"):
            uv = np.stack([cam["fx"] * d[:, 0] / d[:, 2] + cam["cx"], cam["fy"] * d[:, 1] / d[:, 2] + cam["cy"]], 1)
        uv[~(d[:, 2] > 0)] = -1000.0
    return uv.astype(np.float32)


def keypoints(uv):
    import importlib
    kp = np.zeros(len(uv), importlib.import_module("structure-plp-slam_amd").KP_DTYPE)
    kp["x"], kp["y"], kp["class_id"] = uv[:, 0], uv[:, 1], -1
    return kp


def bounds(cam):
    """img_bounds_ of a camera without distortion: min_x, max_x, min_y, max_y"""
    return np.array([0.0, cam["cols"], 0.0, cam["rows"]], np.float32)


def pose_problem(seed, n_matches, model="perspective", n_slots=None, noise=1e-3, mismatch=0.0, iters=24, kind="cloud", max_angle=None):
    """problem() with the cameras of tests/sim3_solver_scene.py: adds camera (name), undist_1 / undist_2 (key points of both frames, the projections
    of the bearings) and bounds.  kind "mirrored": every other match comes from the motion (R, -t), which has the same essential matrix up to
    sign, so that the hypotheses (R, t) and (R, -t) each explain half of the inliers."""
    saved = MAX_ANGLE[model]
    MAX_ANGLE[model] = POSE_MAX_ANGLE[model] if max_angle is None else max_angle
    try:
        q = problem(seed, n_matches, model, n_slots, noise, mismatch, iters, "cloud" if kind == "mirrored" else kind)
    finally:
        MAX_ANGLE[model] = saved
    cam = ref_camera(model)
    if kind == "mirrored":
        R, t = q["truth"]
        slots = np.flatnonzero(q["match"] >= 0)[1::2]
        X1 = q["bearing_1"][slots] * 6.0
        q["bearing_2"][q["match"][slots]] = unit(X1 @ R.T - t)
    q.update(camera=model, kind=kind, undist_1=keypoints(project(cam, q["bearing_1"])), undist_2=keypoints(project(cam, q["bearing_2"])), bounds=bounds(cam))
    return q


def pose_scenes():
    """name -> pose problem: the three cameras at 64, 200 and 500 matches, and the special scenes"""
    out = {}
    k = 0
    for n in (64, 200, 500):
        for model in MODELS:
            out[f"{model}_{n}"] = pose_problem(400 + k, n, model, n_slots=n + (k % 3) * 7, noise=NOISES[k % 3], mismatch=(0.0, 0.2, 0.35)[k % 3], iters=8 if n >= 200 else 16)
            k += 1
    out["exact"] = pose_problem(450, 150, "perspective", n_slots=160, noise=0.0)
    out["border"] = pose_problem(451, 250, "perspective", noise=1e-3, max_angle=np.deg2rad(34.0), iters=12)
    out["planar"] = pose_problem(452, 150, "perspective", n_slots=160, noise=5e-4, kind="planar")
    out["rotation"] = pose_problem(453, 150, "fisheye", noise=1e-3, kind="rotation")
    out["mirrored"] = pose_problem(454, 160, "equirectangular", noise=5e-4, kind="mirrored")
    out["few"] = pose_problem(455, 30, "fisheye", n_slots=40, noise=5e-4)
    out["all_mismatched"] = pose_problem(456, 60, "equirectangular", mismatch=1.0)
    return out


def pose_pack(problems):
    """pack() plus the key-point tables"""
    import importlib
    KP = importlib.import_module("structure-plp-slam_amd").KP_DTYPE
    a = pack(problems)
    P, n_cap, m_cap = len(problems), a["match"].shape[1], a["bearing_2"].shape[1]
    a["undist_1"], a["undist_2"] = np.zeros((P, n_cap), KP), np.zeros((P, m_cap), KP)
    for p, q in enumerate(problems):
        a["undist_1"][p, :len(q["undist_1"])], a["undist_2"][p, :len(q["undist_2"])] = q["undist_1"], q["undist_2"]
    return a
