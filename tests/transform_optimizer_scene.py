"""Seeded scenes for optimize::transform_optimizer (tests/test_transform_optimizer_cpu.py, tests/test_gpu_transform_optimizer.py), on the geometry
of tests/sim3_solver_scene.py: two key-frame poses whose camera frames are related by a known Sim3_12 (x1 = s R x2 + t), n matches 3-9 m in front
of key frame 1, key points that are the float-rounded projections (plus optional Gaussian pixel noise by octave and a share of gross outliers,
displaced by at least 20 px in one image), octaves 0-7, a start estimate that is the truth perturbed as a RANSAC result would be (about 0.02 rad,
a few centimetres, +- 3 % scale); pack() lays problems out as the ragged [P, n_cap] slot arrays of plp_transform_optimize_args, with holes that
hold NaN or garbage."""
import math

import numpy as np

import pose_optimizer_scene as PS
import sim3_solver_scene as SS
import transform_optimizer_ref as REF
from plp import plp

NUM_LEVELS = PS.NUM_LEVELS
INV_SIGMA_SQ = PS.INV_SIGMA_SQ
camera = PS.camera


def make_problem(seed, n, model="perspective", noise=0.0, outlier_share=0.0, rot=0.02, trans=0.03, scale=0.03, fix_scale=False, outlier_px=(20.0, 60.0)):
    """One pair: dict(model, fix_scale, truth (s, R, t), pose_1, pose_2 (15,), rot_12 (9,), trans_12, scale_12 (the start), per match x1, y1, octave1, x2, y2,
    octave2, pos_w_1, pos_w_2, label (1 = gross outlier))."""
    rng = np.random.default_rng(seed)
    _, fx, fy, cx, cy, _ = PS.CAMERAS[model]
    depth = rng.uniform(3.0, 9.0, n)
    x1 = np.stack([depth * np.tan(rng.uniform(-0.35, 0.35, n)), depth * np.tan(rng.uniform(-0.25, 0.25, n)), depth], 1)
    s = 1.0 if fix_scale else rng.uniform(0.8, 1.25)
    R, t = SS.rotation(rng, 0.12), rng.uniform(-0.3, 0.3, 3)
    x2 = (x1 - t) @ R / s                                # R^T (x1 - t) / s
    R1, t1 = SS.rotation(rng, 3.0), rng.uniform(-5, 5, 3)
    R2, t2 = SS.rotation(rng, 3.0), rng.uniform(-5, 5, 3)
    o1 = rng.integers(0, NUM_LEVELS, n).astype(np.int32); o2 = rng.integers(0, NUM_LEVELS, n).astype(np.int32)
    label = (rng.uniform(size=n) < outlier_share).astype(np.uint8)
    ang = rng.uniform(0, 2 * math.pi, n); mag = rng.uniform(*outlier_px, size=n) * label
    in_2 = rng.uniform(size=n) < 0.5                     # the image the outlier's key point is displaced in
    u1 = fx * x1[:, 0] / x1[:, 2] + cx + noise * PS.SCALE ** o1 * rng.normal(size=n) + np.where(in_2, 0.0, mag * np.cos(ang))
    v1 = fy * x1[:, 1] / x1[:, 2] + cy + noise * PS.SCALE ** o1 * rng.normal(size=n) + np.where(in_2, 0.0, mag * np.sin(ang))
    u2 = fx * x2[:, 0] / x2[:, 2] + cx + noise * PS.SCALE ** o2 * rng.normal(size=n) + np.where(in_2, mag * np.cos(ang), 0.0)
    v2 = fy * x2[:, 1] / x2[:, 2] + cy + noise * PS.SCALE ** o2 * rng.normal(size=n) + np.where(in_2, mag * np.sin(ang), 0.0)
    Rs = PS.rodrigues(rng.normal(size=3) * rot / math.sqrt(3.0)) @ R
    ss = s if fix_scale else s * (1.0 + rng.uniform(-scale, scale))
    return dict(model=model, fix_scale=fix_scale, truth=(s, R, t), pose_1=SS.pose_row(R1, t1), pose_2=SS.pose_row(R2, t2), rot_12=Rs.reshape(9),
                trans_12=t + rng.normal(size=3) * trans, scale_12=np.float32(ss), x1=u1.astype(np.float32), y1=v1.astype(np.float32), octave1=o1,
                x2=u2.astype(np.float32), y2=v2.astype(np.float32), octave2=o2, pos_w_1=(x1 - t1) @ R1, pos_w_2=(x2 - t2) @ R2, label=label)


def pack(problems, n_cap=None, holes=0.0, seed=0):
    """Problems (one camera model, one fix_scale) as slot arrays: dict(camera, fix_scale, valid, pos_w_1, pos_w_2, undist_1, undist_2, pose_1, pose_2,
    rot_12, trans_12, scale_12, counts, slot (per problem: the slot of match k)).  holes: the share of unused slots strewn between the matches (valid 0;
    NaN positions in key frame 2, finite junk in key frame 1, octaves inside the tables); slots behind counts[p] hold the same junk with valid 1.  Octaves
    outside the tables are a case of their own (census_problems)."""
    rng = np.random.default_rng(seed)
    P = len(problems)
    need = [int(math.ceil(len(q["x1"]) / (1.0 - holes))) if holes else len(q["x1"]) for q in problems]
    N = n_cap if n_cap is not None else max(need + [1])
    A = dict(camera=camera(problems[0]["model"]), fix_scale=problems[0]["fix_scale"], valid=np.ones((P, N), np.uint8), pos_w_1=rng.normal(size=(P, N, 3)) + 5.0,
             pos_w_2=np.full((P, N, 3), np.nan), undist_1=np.zeros((P, N), plp.KP_DTYPE), undist_2=np.zeros((P, N), plp.KP_DTYPE), pose_1=np.zeros((P, 15)),
             pose_2=np.zeros((P, 15)), rot_12=np.zeros((P, 9)), trans_12=np.zeros((P, 3)), scale_12=np.zeros(P, np.float32), counts=np.zeros(P, np.int32), slot=[])
    # what is not a match -- the holes (valid 0) and the slots behind counts[p] (valid 1) -- carries octaves INSIDE the sigma tables on both sides, so that only
    # the `valid` byte and `counts` keep those slots out: the positions of key frame 2 there are NaN and would poison every sum
    A["undist_1"]["x"] = 3.0; A["undist_1"]["octave"] = 1; A["undist_2"]["x"] = 7.0; A["undist_2"]["y"] = 5.0; A["undist_2"]["octave"] = 2
    for p, q in enumerate(problems):
        for k in ("pose_1", "pose_2", "rot_12", "trans_12", "scale_12"):
            A[k][p] = q[k]
        n = len(q["x1"])
        cnt = min(N, need[p])
        slots = np.sort(rng.choice(cnt, size=n, replace=False)) if n else np.zeros(0, np.int64)
        A["counts"][p] = cnt
        A["valid"][p, :cnt] = 0
        A["valid"][p, slots] = 1
        for side in ("1", "2"):
            kp = A["undist_" + side]
            kp["x"][p, slots] = q["x" + side]; kp["y"][p, slots] = q["y" + side]; kp["octave"][p, slots] = q["octave" + side]
            A["pos_w_" + side][p, slots] = q["pos_w_" + side]
        A["slot"].append(slots)
    return A


def call_args(A, **kw):
    """the arguments of model_transform_optimize / matcher.transform_optimize for a pack"""
    a = {k: A[k] for k in ("camera", "fix_scale", "valid", "pos_w_1", "pos_w_2", "undist_1", "undist_2", "pose_1", "pose_2", "rot_12", "trans_12", "scale_12", "counts")}
    a.update(inv_level_sigma_sq_1=INV_SIGMA_SQ, inv_level_sigma_sq_2=INV_SIGMA_SQ)
    a.update(kw)
    return a


def ref_problems(A, chi_sq=10.0, sig1=INV_SIGMA_SQ):
    """the pack as tests/transform_optimizer_ref.py Problem objects (slots behind counts are cut off)"""
    c = A["camera"]
    cam = REF.Cam(c.fx, c.fy, c.cx, c.cy)
    out = []
    for p in range(len(A["pose_1"])):
        k1, k2 = A["undist_1"][p], A["undist_2"][p]
        slots = [dict(valid=int(A["valid"][p, s]), x1=float(k1["x"][s]), y1=float(k1["y"][s]), octave1=int(k1["octave"][s]), x2=float(k2["x"][s]),
                      y2=float(k2["y"][s]), octave2=int(k2["octave"][s]), pos_w_1=[float(v) for v in A["pos_w_1"][p, s]],
                      pos_w_2=[float(v) for v in A["pos_w_2"][p, s]]) for s in range(int(A["counts"][p]))]
        out.append(REF.Problem(cam, A["fix_scale"], A["pose_1"][p], A["pose_2"][p], A["rot_12"][p], A["trans_12"][p], A["scale_12"][p], slots, sig1,
                               INV_SIGMA_SQ, chi_sq))
    return out


def z0_problem(n=14, fix_scale=False, model="perspective"):
    """a pair at rest at its truth (Sim3_12 = identity, both key frames at the origin) whose match 3 has z == 0.0 exactly in key frame 1: non-finite errors from
    the first pass on"""
    q = make_problem(11, n, fix_scale=fix_scale, model=model)
    _, fx, fy, cx, cy, _ = PS.CAMERAS[q["model"]]
    x1 = q["pos_w_1"] @ q["pose_1"][:9].reshape(3, 3).T + q["pose_1"][9:12]
    ident = SS.pose_row(np.eye(3), np.zeros(3))
    q.update(pose_1=ident, pose_2=ident, rot_12=np.eye(3).reshape(9), trans_12=np.zeros(3), scale_12=np.float32(1.0), truth=(1.0, np.eye(3), np.zeros(3)),
             pos_w_1=x1.copy(), pos_w_2=x1.copy())
    for side in ("1", "2"):
        q["x" + side] = (fx * x1[:, 0] / x1[:, 2] + cx).astype(np.float32); q["y" + side] = (fy * x1[:, 1] / x1[:, 2] + cy).astype(np.float32)
    q["pos_w_2"][3] = [0.375, -0.25, 0.0]
    return q


def census_problems(model, fix_scale):
    """the ragged problems of one call that reach both statuses, rejected steps, the ten tries, rho == 0, a NaN chi2 in round 1 (round 2's is
    nan_in_round_2_problem, which needs its own sigma table), drops in both rounds, odd octaves and the small counts"""
    pr = [make_problem(31, 0, model=model, fix_scale=fix_scale), make_problem(32, 1, model=model, fix_scale=fix_scale),
          make_problem(33, 9, model=model, fix_scale=fix_scale), make_problem(34, 10, model=model, fix_scale=fix_scale),
          make_problem(35, 60, model=model, fix_scale=fix_scale, noise=1.0, outlier_share=0.25, rot=0.05, trans=0.1),
          make_problem(36, 40, model=model, fix_scale=fix_scale, noise=0.5, outlier_share=0.8),          # too few left after round 1
          make_problem(37, 150, model=model, fix_scale=fix_scale, noise=1.0, outlier_share=0.1), z0_problem(fix_scale=fix_scale, model=model), inf_problem(model, fix_scale),
          ten_tries_problem(model, fix_scale), make_problem(3000, 80, model=model, fix_scale=fix_scale, noise=1.6, outlier_share=0.1)]     # drops in round 2 too
    odd = make_problem(38, 25, model=model, fix_scale=fix_scale, noise=0.5)
    odd["octave1"][[2, 7]] = [NUM_LEVELS, -1]
    odd["octave2"][5] = 12
    pr.append(odd)
    for q in pr:
        q["model"], q["fix_scale"] = model, fix_scale
    return pr


def inf_problem(model="perspective", fix_scale=False, n=30):
    """a noise-free pair whose match 4 has an infinite coordinate in key frame 2's landmark: its forward chi2 is NaN (inf - inf) from the first pass on, the
    system is non-finite, every step is rejected, and round 1 drops the match (a NaN is an outlier there) and whatever the start estimate leaves above chi_sq"""
    q = make_problem(41, n, model=model, fix_scale=fix_scale)
    q["pos_w_2"][4] = [np.inf, 1.0, 2.0]
    return q


def _at_rest(n, seed, scale=1.0, trans=(0.0, 0.0, 0.0), share=0.0, s_out=1.0, start=1.0):
    """a pair with both key frames at the world's origin, Sim3_12 = (scale, I, trans), key points of octave 0 without noise; the landmarks in key frame 2 of
    the matches of a share `share` (label 1; never match 0) are consistent with scale * s_out instead; the start is the truth with its scale times `start`"""
    rng = np.random.default_rng(seed)
    _, fx, fy, cx, cy, _ = PS.CAMERAS["perspective"]
    t0 = np.asarray(trans, np.float64)
    depth = rng.uniform(3.0, 9.0, n)
    x1 = np.stack([depth * np.tan(rng.uniform(-0.35, 0.35, n)), depth * np.tan(rng.uniform(-0.25, 0.25, n)), depth], 1)
    label = (rng.uniform(size=n) < share).astype(np.uint8)
    label[0] = 0
    x2 = (x1 - t0) / (scale * np.where(label, s_out, 1.0))[:, None]
    x2t = (x1 - t0) / scale
    ident = SS.pose_row(np.eye(3), np.zeros(3))
    return dict(model="perspective", fix_scale=False, truth=(scale, np.eye(3), t0), pose_1=ident, pose_2=ident, rot_12=np.eye(3).reshape(9), trans_12=t0.copy(),
                scale_12=np.float32(scale * start), x1=(fx * x1[:, 0] / x1[:, 2] + cx).astype(np.float32), y1=(fy * x1[:, 1] / x1[:, 2] + cy).astype(np.float32),
                octave1=np.zeros(n, np.int32), x2=(fx * x2t[:, 0] / x2t[:, 2] + cx).astype(np.float32), y2=(fy * x2t[:, 1] / x2t[:, 2] + cy).astype(np.float32),
                octave2=np.zeros(n, np.int32), pos_w_1=x1.copy(), pos_w_2=x2.copy(), label=label)


# the sigma table of key frame 1 for nan_in_round_2_problem: level 7 has weight 0
INV_SIGMA_SQ_W0 = INV_SIGMA_SQ.copy()
INV_SIGMA_SQ_W0[7] = 0.0


def nan_in_round_2_problem(n=40):
    """A pair whose match 0 is an inlier of round 1 with a finite chi2 and has a NaN chi2 at the end of round 2 (a NaN is an inlier there).  Truth scale 2, start
    1.98; a third of the matches is consistent with scale 1.8, so round 1 (Huber) settles near 1.9936, drops them, and round 2's tries jump to 2.0.  Match 0 is observed at
    level 7, whose weight in INV_SIGMA_SQ_W0 is 0, so its forward chi2 is e (0 e) = 0 for a finite error; its landmark in key frame 2 is so far off
    (x = DBL_MAX / (fx 1.997), z = x / 100) that fx x overflows once the scale passes 1.997: the error is -inf, 0 * inf is NaN, the try is rejected (rho is NaN),
    and the match keeps the NaN of that last evaluation.  Call it with inv_level_sigma_sq_1 = INV_SIGMA_SQ_W0."""
    q = _at_rest(n, 5, scale=2.0, trans=(1.5, 1.0, 0.5), share=0.3, s_out=0.9, start=0.99)
    fx = PS.CAMERAS["perspective"][1]
    big = 1.7976931348623157e308 / (2.0 * 0.9985) / fx
    q["pos_w_2"][0] = [big, 0.0, big / 100.0]
    q["x1"][0] = 100.0; q["y1"][0] = 248.375; q["octave1"][0] = 7
    return q


def ten_tries_problem(model="perspective", fix_scale=False):
    """a small noisy pair (found with the host build; tests/test_transform_optimizer_cpu.py asserts what it reaches) whose round 2 ends at its minimum with
    the ten tries: every further step raises chi2 by rounding"""
    return make_problem(1001, 12, model=model, fix_scale=fix_scale, noise=0.3)
