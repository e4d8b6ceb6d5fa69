"""Seeded scenes for solve::pnp_solver (tests/test_pnp_solver_cpu.py, tests/test_gpu_pnp_solver.py): a known pose (R, t) of the frame, n
matches whose landmarks lie 2-10 m from the camera in the directions its model sees, exact bearings, a stated share of gross outliers (a
random direction in place of the bearing), octaves over all levels, holes in `valid`, and distinct sample quadruples.

The solver sees bearings only; the camera model decides where they point:
  perspective      within 35 degrees of the optical axis
  fisheye          within 95 degrees of it (a few with z < 0)
  equirectangular  the whole sphere: half of the bearings have z < 0, which is signs_ = -1 in add_correspondence"""
import numpy as np

MODELS = ("perspective", "fisheye", "equirectangular")
MAX_ANGLE = {"perspective": np.deg2rad(35.0), "fisheye": np.deg2rad(95.0), "equirectangular": np.pi}
SCALE_FACTORS = (np.float32(1.2) ** np.arange(8)).astype(np.float32)      # scale_factors_ (orb_params.cc)


def rotation(rng, max_angle=np.pi):
    axis = rng.standard_normal(3)
    axis /= np.linalg.norm(axis)
    a = rng.uniform(-max_angle, max_angle)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * (K @ K)


def directions(rng, n, max_angle):
    """n unit vectors, uniform on the cap of half-angle max_angle around +z"""
    z = rng.uniform(np.cos(max_angle), 1.0, n)
    phi = rng.uniform(0.0, 2 * np.pi, n)
    s = np.sqrt(np.maximum(0.0, 1.0 - z * z))
    return np.stack([s * np.cos(phi), s * np.sin(phi), z], axis=1)


def problem(seed, n_valid, model="perspective", n_slots=None, outliers=0.3, iters=30, all_outliers=False, coplanar=False):
    """one problem: dict(valid, bearing, pos_w, octave per slot, samples (iters, 4), iters, truth=(R, t) of X_c = R X_w + t, is_outlier per
    match, model)"""
    rng = np.random.default_rng(seed)
    n_slots = n_valid if n_slots is None else n_slots
    assert n_slots >= n_valid
    R, t = rotation(rng), rng.uniform(-2.0, 2.0, 3)
    valid = np.zeros(n_slots, np.uint8)
    valid[np.sort(rng.choice(n_slots, n_valid, replace=False))] = 1       # holes: the ranks differ from the slots
    d = directions(rng, n_slots, MAX_ANGLE[model])
    pc = d * rng.uniform(2.0, 10.0, n_slots)[:, None]
    if coplanar:
        pc[:, 2] = 5.0 + 0.25 * pc[:, 0]                                   # all landmarks in one plane
        d = pc / np.linalg.norm(pc, axis=1, keepdims=True)
    pos_w = (pc - t) @ R                                                   # R^T (X_c - t)
    bearing = d.copy()
    is_out = np.ones(n_slots, bool) if all_outliers else rng.random(n_slots) < outliers
    bearing[is_out] = directions(rng, int(is_out.sum()), np.pi)
    octave = rng.integers(0, len(SCALE_FACTORS), n_slots).astype(np.int32)
    samples = np.zeros((iters, 4), np.int32)
    for i in range(iters):
        samples[i] = rng.choice(n_valid, 4, replace=False) if n_valid >= 4 else np.arange(4)
    return dict(valid=valid, bearing=bearing, pos_w=pos_w, octave=octave, samples=samples, iters=iters, truth=(R, t), is_outlier=is_out[valid != 0],
                model=model)


def degenerate_problem():
    """the degenerate samples of the CPU census in one problem: iteration 0 a bad index, 1 a repeated index, 2 all four bearings with z == 0,
    3 one bearing with z == 0 (three correspondences), 4 a sample of exact matches, 5 a sample with two octaves outside the table, 6 a sample
    of four equal landmarks (a non-finite pose), 7 / 8 two more samples of exact matches (equal counts: a tie)"""
    q = problem(71, 40, "equirectangular", n_slots=48, outliers=0.2, iters=9)
    slots = np.flatnonzero(q["valid"])
    R, t = q["truth"]
    for k in (0, 1, 2, 3):                                                        # matches 0 .. 3: bearing z == 0
        b = q["bearing"][slots[k]]
        b[2] = 0.0
        b /= np.linalg.norm(b)
    q["octave"][slots[5]] = 8
    q["octave"][slots[6]] = -1
    for k in (10, 11, 12, 13):                                                    # four equal landmarks
        q["pos_w"][slots[k]] = q["pos_w"][slots[10]]
    good = np.flatnonzero(~q["is_outlier"])
    good = good[good > 13]
    q["samples"][0] = [0, 5, 40, 7]
    q["samples"][1] = [4, 9, 4, 8]
    q["samples"][2] = [0, 1, 2, 3]
    q["samples"][3] = [good[0], 2, good[1], good[2]]
    q["samples"][4] = good[:4]
    q["samples"][5] = [5, 6, good[4], good[5]]
    q["samples"][6] = [10, 11, 12, 13]
    q["samples"][7] = good[[0, 3, 6, 9]]
    q["samples"][8] = good[[1, 4, 7, 10]]
    return q


def pack(problems, n_cap=None):
    """the [P][n_cap] arrays of plp_pnp_ransac_args for problems of one iteration count; slots at or above a problem's own are invalid"""
    P = len(problems)
    n_cap = max(len(q["valid"]) for q in problems) if n_cap is None else n_cap
    iters = problems[0]["iters"]
    a = dict(valid=np.zeros((P, n_cap), np.uint8), bearing=np.zeros((P, n_cap, 3)), pos_w=np.zeros((P, n_cap, 3)), octave=np.zeros((P, n_cap), np.int32),
             samples=np.zeros((P, iters, 4), np.int32), counts=np.zeros(P, np.int32))
    for p, q in enumerate(problems):
        m = len(q["valid"])
        assert q["iters"] == iters and m <= n_cap
        for k in ("valid", "bearing", "pos_w", "octave"):
            a[k][p, :m] = q[k]
        a["samples"][p] = q["samples"]
        a["counts"][p] = m
    return a
