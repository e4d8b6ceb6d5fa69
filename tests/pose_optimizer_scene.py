"""Synthetic frames for the pose optimiser's tests (tests/test_pose_optimizer_cpu.py, tests/test_gpu_pose_optimizer.py): a ground-truth pose,
landmarks in front of the camera, Pluecker lines from two 3-D points, observations from the true projection with optional Gaussian pixel noise
by octave and a share of gross outliers (displaced by at least 20 px), a perturbed start pose; pack() lays frames out as the ragged
[B, n_cap] / [B, l_cap] slot arrays of plp_pose_optimize_args, with holes."""
import math

import numpy as np

import pose_optimizer_ref as REF
from plp import plp

NUM_LEVELS = 8
SCALE = 1.2
INV_SIGMA_SQ = np.array([1.0 / (SCALE ** l) ** 2 for l in range(NUM_LEVELS)], np.float32)
INV_SIGMA_SQ_LSD = np.array([1.0 / (2.0 ** l) ** 2 for l in range(2)], np.float32)       # the line extractor's two octaves, scale 2
CAMERAS = {   # model -> fx, fy, cx, cy, focal_x_baseline
    "perspective": (plp.CAMERA_PERSPECTIVE, 458.654, 457.296, 367.215, 248.375, 50.4),
    "fisheye": (plp.CAMERA_FISHEYE, 190.978, 190.973, 254.931, 256.897, 21.0),
}
MONO, STEREO, RGBD = 0, 1, 2


def camera(model):
    m, fx, fy, cx, cy, fxb = CAMERAS[model]
    c = plp.camera_model_c()
    c.model, c.cols, c.rows = m, 752, 480
    c.fx, c.fy, c.cx, c.cy, c.focal_x_baseline = fx, fy, cx, cy, fxb
    return c


def rodrigues(w):
    th = float(np.linalg.norm(w))
    if th == 0.0:
        return np.eye(3)
    k = np.asarray(w, np.float64) / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + math.sin(th) * K + (1 - math.cos(th)) * (K @ K)


def make_frame(seed, n, model="perspective", setup=MONO, n_lines=0, noise=0.0, outlier_share=0.0, rot=0.02, trans=0.05, mono_share=0.3, z_range=(2.0, 10.0),
               outlier_px=(20.0, 60.0)):
    """One frame: dict(model, setup, R, t (ground truth), pose_start (12,), points: x, y, octave, x_right, pos_w, label (1 = gross outlier);
    lines: sx, sy, ex, ey, octave, pos_w (n_lines, 6), label)."""
    rng = np.random.default_rng(seed)
    _, fx, fy, cx, cy, fxb = CAMERAS[model]
    R = rodrigues(rng.normal(size=3) * 0.3)
    t = rng.normal(size=3) * 0.5

    def landmarks(m):
        z = rng.uniform(*z_range, size=m)
        u = rng.uniform(40.0, 2 * cx - 40.0, size=m); v = rng.uniform(40.0, 2 * cy - 40.0, size=m)
        pc = np.stack([(u - cx) / fx * z, (v - cy) / fy * z, z], 1)
        return (pc - t) @ R          # R^T (pc - t)

    def project(pw):
        pc = pw @ R.T + t
        return fx * pc[:, 0] / pc[:, 2] + cx, fy * pc[:, 1] / pc[:, 2] + cy, pc[:, 2]

    def displace(m):
        ang = rng.uniform(0, 2 * math.pi, size=m); mag = rng.uniform(*outlier_px, size=m)
        return mag * np.cos(ang), mag * np.sin(ang)

    pw = landmarks(n)
    u, v, z = project(pw)
    octave = rng.integers(0, NUM_LEVELS, size=n).astype(np.int32)
    sig = SCALE ** octave
    label = (rng.uniform(size=n) < outlier_share).astype(np.uint8)
    dx, dy = displace(n)
    nu = u + noise * sig * rng.normal(size=n) + label * dx
    nv = v + noise * sig * rng.normal(size=n) + label * dy
    xr = np.full(n, -1.0)
    if setup != MONO:
        xr = nu - fxb / z + noise * sig * rng.normal(size=n)
        if setup == RGBD:
            xr = np.where(rng.uniform(size=n) < mono_share, -1.0, xr)
    f = dict(model=model, setup=setup, R=R, t=t, x=nu.astype(np.float32), y=nv.astype(np.float32), octave=octave, x_right=xr.astype(np.float32), pos_w=pw, label=label)
    Rs = rodrigues(rng.normal(size=3) * rot) @ R
    f["pose_start"] = np.concatenate([Rs.reshape(9), t + rng.normal(size=3) * trans])
    if n_lines:
        P = landmarks(n_lines); Q = P + rng.normal(size=(n_lines, 3)) * 0.5
        Q = np.where((project(Q)[2] > 0.5)[:, None], Q, P + np.array([0.3, 0.1, 0.0]) @ R)
        us, vs, _ = project(P); ue, ve, _ = project(Q)
        lo = rng.integers(0, len(INV_SIGMA_SQ_LSD), size=n_lines).astype(np.int32)
        ll = (rng.uniform(size=n_lines) < outlier_share).astype(np.uint8)
        # an outlier line is moved across itself by at least 20 px
        nx, ny = -(ve - vs), ue - us
        nn = np.sqrt(nx * nx + ny * ny); nx, ny = nx / nn, ny / nn
        mag = rng.uniform(*outlier_px, size=n_lines) * ll
        ls = 2.0 ** lo
        f.update(l_sx=(us + mag * nx + noise * ls * rng.normal(size=n_lines)).astype(np.float32), l_sy=(vs + mag * ny + noise * ls * rng.normal(size=n_lines)).astype(np.float32),
                 l_ex=(ue + mag * nx + noise * ls * rng.normal(size=n_lines)).astype(np.float32), l_ey=(ve + mag * ny + noise * ls * rng.normal(size=n_lines)).astype(np.float32),
                 l_octave=lo, l_pos_w=np.concatenate([np.cross(P, Q), Q - P], 1), l_label=ll)
    return f


def n_lines_of(f):
    return len(f["l_sx"]) if "l_sx" in f else 0


def pack(frames, n_cap=None, l_cap=None, holes=0.0, seed=0, with_lines=None):
    """Frames (one camera model and set-up) as slot arrays: dict(camera, setup_type, pose_in (B, 15), valid, undist, x_right, pos_w, counts,
    lines (None, or the dict model_pose_optimize takes), slot (per frame: the slot of observation k), line_slot).  holes: the share of unused
    slots strewn between the observations (valid 0, filled with finite junk); slots behind counts[b] hold junk with valid 1."""
    rng = np.random.default_rng(seed)
    B = len(frames)
    need = [int(math.ceil(len(f["x"]) / (1.0 - holes))) if holes else len(f["x"]) for f in frames]
    N = n_cap if n_cap is not None else max(need + [1])
    nl = [n_lines_of(f) for f in frames]
    lines = with_lines if with_lines is not None else any(nl)
    lneed = [int(math.ceil(k / (1.0 - holes))) if holes else k for k in nl]
    L = (l_cap if l_cap is not None else max(lneed + [1])) if lines else 0
    P = dict(camera=camera(frames[0]["model"]), setup_type=frames[0]["setup"], pose_in=np.zeros((B, 15)), valid=np.ones((B, N), np.uint8),
             undist=np.zeros((B, N), plp.KP_DTYPE), x_right=np.full((B, N), 7.0, np.float32), pos_w=rng.normal(size=(B, N, 3)) + 5.0,
             counts=np.zeros(B, np.int32), slot=[], line_slot=[], lines=None)
    P["undist"]["x"] = 3.0; P["undist"]["octave"] = 1
    if lines:
        ln = dict(valid=np.ones((B, L), np.uint8), keylines=np.zeros((B, L), plp.KL_DTYPE), pos_w=rng.normal(size=(B, L, 6)), counts=np.zeros(B, np.int32),
                  inv_level_sigma_sq_lsd=INV_SIGMA_SQ_LSD)
        ln["keylines"]["endPointX"] = 9.0
        P["lines"] = ln
    for b, f in enumerate(frames):
        P["pose_in"][b, :12] = f["pose_start"]
        n = len(f["x"])
        cnt = min(N, need[b])
        slots = np.sort(rng.choice(cnt, size=n, replace=False)) if n else np.zeros(0, np.int64)
        P["counts"][b] = cnt
        P["valid"][b, :cnt] = 0
        P["valid"][b, slots] = 1
        P["undist"]["x"][b, slots] = f["x"]; P["undist"]["y"][b, slots] = f["y"]; P["undist"]["octave"][b, slots] = f["octave"]
        P["x_right"][b, slots] = f["x_right"]; P["pos_w"][b, slots] = f["pos_w"]
        P["slot"].append(slots)
        if lines:
            k = nl[b]
            cnt = min(L, lneed[b])
            ls = np.sort(rng.choice(cnt, size=k, replace=False)) if k else np.zeros(0, np.int64)
            ln["counts"][b] = cnt
            ln["valid"][b, :cnt] = 0
            if k:
                ln["valid"][b, ls] = 1
                kl = ln["keylines"]
                kl["startPointX"][b, ls] = f["l_sx"]; kl["startPointY"][b, ls] = f["l_sy"]; kl["endPointX"][b, ls] = f["l_ex"]; kl["endPointY"][b, ls] = f["l_ey"]
                kl["octave"][b, ls] = f["l_octave"]; ln["pos_w"][b, ls] = f["l_pos_w"]
            P["line_slot"].append(ls)
    if frames[0]["setup"] == MONO:
        P["x_right"][:] = -1.0
    return P


def call_args(P, **kw):
    """the arguments of model_pose_optimize / matcher.pose_optimize for a pack"""
    a = dict(camera=P["camera"], setup_type=P["setup_type"], pose_in=P["pose_in"], valid=P["valid"], undist=P["undist"], pos_w=P["pos_w"],
             inv_level_sigma_sq=INV_SIGMA_SQ, x_right=P["x_right"], counts=P["counts"], lines=P["lines"])
    a.update(kw)
    return a


def ref_frames(P):
    """the pack as tests/pose_optimizer_ref.py Frame objects (slots behind counts are cut off)"""
    ref = REF
    c = P["camera"]
    cam = ref.Cam(c.fx, c.fy, c.cx, c.cy, c.focal_x_baseline)
    out = []
    for b in range(len(P["pose_in"])):
        cnt = int(P["counts"][b])
        kp = P["undist"][b]
        pts = [dict(valid=int(P["valid"][b, s]), x=float(kp["x"][s]), y=float(kp["y"][s]), octave=int(kp["octave"][s]), x_right=float(P["x_right"][b, s]),
                    pos_w=[float(v) for v in P["pos_w"][b, s]]) for s in range(cnt)]
        lines = None
        sl = ()
        if P["lines"] is not None:
            ln = P["lines"]; kl = ln["keylines"][b]
            lines = [dict(valid=int(ln["valid"][b, s]), sx=float(kl["startPointX"][s]), sy=float(kl["startPointY"][s]), ex=float(kl["endPointX"][s]),
                          ey=float(kl["endPointY"][s]), octave=int(kl["octave"][s]), pos_w=[float(v) for v in ln["pos_w"][b, s]]) for s in range(int(ln["counts"][b]))]
            sl = ln["inv_level_sigma_sq_lsd"]
        out.append(ref.Frame(cam, P["setup_type"] == MONO, P["pose_in"][b, :12], pts, INV_SIGMA_SQ, lines, sl))
    return out


# seeds found with the host build (tests/test_pose_optimizer_cpu.py asserts what they reach): (setup, model, lines) -> (seed, n) of a frame whose
# trial loop breaks in trial 2; every set-up breaks in trial 0 with seed 0, n 7
BREAK_IN_TRIAL_2 = {(MONO, "perspective", 6): (737, 12), (MONO, "fisheye", 6): (280, 11), (STEREO, "perspective", 0): (837, 10), (STEREO, "fisheye", 6): (908, 9),
                    (RGBD, "fisheye", 6): (173, 12)}


def break_frame(seed, n, model, setup, n_lines):
    return make_frame(seed, n, model=model, setup=setup, n_lines=n_lines, noise=1.5, outlier_share=0.35, rot=0.05, trans=0.1)


def z0_frame(setup=MONO, n=12):
    """a frame at rest at its ground truth (rotation I) whose landmark 3 has z_c == 0.0 exactly at the start pose: non-finite errors from the first pass on"""
    f = make_frame(11, n, setup=setup)
    t = np.array([0.5, 0.25, 1.0])
    pc = f["pos_w"] @ f["R"].T + f["t"]
    f["R"], f["t"] = np.eye(3), t
    f["pos_w"] = pc - t
    f["pos_w"][3] = [0.375, -0.25, -1.0]
    f["pose_start"] = np.concatenate([np.eye(3).reshape(9), t])
    return f


def one_point_frame(n=12):
    f = make_frame(1, n)
    f["pos_w"][:] = f["pos_w"][0]
    return f


def census_frames(model, setup):
    """the ragged frames of one call that reach both statuses, the early breaks, rejected steps, the ten tries, mixed edges and odd octaves"""
    nl = 6
    fr = [make_frame(21, 4, model=model, setup=setup, n_lines=3), make_frame(22, 5, model=model, setup=setup, n_lines=3),
          break_frame(0, 7, model, setup, nl),
          make_frame(23, 70, model=model, setup=setup, n_lines=9, noise=1.0, outlier_share=0.2, rot=0.1, trans=0.3),
          make_frame(24, 33, model=model, setup=setup, n_lines=0), z0_frame(setup), one_point_frame()]
    for (su, mo, k), (seed, n) in BREAK_IN_TRIAL_2.items():
        if su == setup and mo == model:
            fr.append(break_frame(seed, n, model, setup, k))
    odd = make_frame(25, 20, model=model, setup=setup, n_lines=4, noise=0.5)
    odd["octave"][[2, 7]] = [NUM_LEVELS, -1]
    odd["l_octave"][1] = 5
    fr.append(odd)
    for f in fr:
        f["model"], f["setup"] = model, setup
        if setup == MONO:
            f["x_right"][:] = -1.0
    return fr
