"""Scenes for the line map update of DESIGN.md section 5, D25 (tests/test_line_update_cpu.py, tests/test_gpu_line_update*.py): true 3-D segments in front of
a few perspective key frames, key lines that are the float32 projections of the true end points (a few pixels of noise on some), ragged observation lists,
and directed rows behind the undirected ones for every place the trim can leave."""
import math

import numpy as np

from plp import plp

CAM = (520.0, 515.0, 320.5, 240.25)                  # fx, fy, cx, cy
CAM_YAML = {"Camera.model": "perspective", "Camera.cols": 640, "Camera.rows": 480, "Camera.fx": CAM[0], "Camera.fy": CAM[1], "Camera.cx": CAM[2], "Camera.cy": CAM[3],
            "Camera.k1": 0.0, "Camera.k2": 0.0, "Camera.p1": 0.0, "Camera.p2": 0.0, "Camera.k3": 0.0}
DIRECTED = ("erased", "no_ref", "ref_outside", "ref_erased", "not_observing", "idx_minus_one", "idx_at_counts", "behind", "horizontal", "vertical", "moved",
            "nan_pose")


def camera():
    return plp.camera_model(CAM_YAML)


def _rot(ax, ay, az):
    cx, sx, cy, sy, cz, sz = math.cos(ax), math.sin(ax), math.cos(ay), math.sin(ay), math.cos(az), math.sin(az)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]], np.float64)
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]], np.float64)
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]], np.float64)
    return Rz @ Ry @ Rx


def pose_row(R, t):
    return np.concatenate([R.reshape(-1), t, -R.T @ t])


def project(pose, X, cam=CAM):
    """pixel of the world point X in the key frame of the pose row, as float32 (cv::Point2f)"""
    pc = pose[:9].reshape(3, 3) @ X + pose[9:12]
    return np.float32(cam[0] * pc[0] / pc[2] + cam[2]), np.float32(cam[1] * pc[1] / pc[2] + cam[3])


def pluecker_of(sp, ep, scale=1.0):
    """(m, d) with d = scale (ep - sp), m = sp x d"""
    d = scale * (ep - sp)
    return np.concatenate([np.cross(sp, d), d])


def scene(seed, F=5, n_lines=120, stride=15, noise_every=4, slack=2):
    """F live key frames (row 0 has the identity pose) + two directed rows (an erased one, one with a NaN pose entry); n_lines undirected lines followed by
    the DIRECTED ones.  Returns a dict of numpy arrays; `directed` name -> row, `undirected` = n_lines."""
    rng = np.random.default_rng(seed)
    FT = F + 2
    pose = np.zeros((FT, stride))
    for f in range(FT):
        R = np.eye(3) if f == 0 else _rot(*rng.uniform(-0.12, 0.12, 3))
        t = np.zeros(3) if f == 0 else -R @ rng.uniform(-0.6, 0.6, 3)
        pose[f, :15] = pose_row(R, t)
        pose[f, 15:] = 1e30                                # behind a longer stride: never read
    kf_erased = np.zeros(FT, np.uint8)
    kf_erased[F] = 1
    pose[F + 1, 10] = np.nan
    lines, obs = [], []                                    # (sp, ep), [(kf, keyline or None = a slot index is given)]
    slots = [[] for _ in range(FT)]                        # per key frame: (sx, sy, ex, ey)

    def seg(z_lo=3.0, z_hi=8.0):
        sp = np.array([rng.uniform(-1.5, 1.5), rng.uniform(-1.0, 1.0), rng.uniform(z_lo, z_hi)])
        ep = sp + rng.uniform(-1.0, 1.0, 3) * np.array([1.0, 1.0, 0.5])
        return sp, ep

    def observe(f, sp, ep, noise=0.0):
        a, b = project(pose[f], sp), project(pose[f], ep)
        n = rng.normal(0.0, noise, 4).astype(np.float32) if noise else np.zeros(4, np.float32)
        slots[f].append((a[0] + n[0], a[1] + n[1], b[0] + n[2], b[1] + n[3]))
        return len(slots[f]) - 1

    lengths = [0, 1] + [min(F, 12)] * 2
    for l in range(n_lines):
        sp, ep = seg()
        n_obs = lengths[l] if l < len(lengths) else int(rng.integers(1, min(F, 12) + 1))
        kfs = [int(k) for k in rng.permutation(F)[:n_obs]]
        noise = 2.0 if noise_every and l % noise_every == 1 else 0.0
        lines.append((sp, ep, kfs[int(rng.integers(0, n_obs))] if n_obs else int(rng.integers(0, F))))
        obs.append([(k, observe(k, sp, ep, noise)) for k in kfs])
    directed = {}

    def add(name, sp, ep, ref, ob):
        directed[name] = len(lines)
        lines.append((sp, ep, ref))
        obs.append(ob)
    sp, ep = seg()
    add("erased", sp, ep, 1 % F, [(1 % F, observe(1 % F, sp, ep))])
    sp, ep = seg()
    add("no_ref", sp, ep, -1, [(0, observe(0, sp, ep))])
    sp, ep = seg()
    add("ref_outside", sp, ep, FT, [(0, observe(0, sp, ep))])
    sp, ep = seg()
    add("ref_erased", sp, ep, F, [(F, observe(F, sp, ep))])
    sp, ep = seg()
    add("not_observing", sp, ep, F - 1, [(k, observe(k, sp, ep)) for k in range(F - 1)])
    sp, ep = seg()
    add("idx_minus_one", sp, ep, 0, [(0, -1)])
    sp, ep = seg()
    add("idx_at_counts", sp, ep, 0, [(0, None)])           # filled in below: counts[0]
    sp, ep = seg(-8.0, -3.0)
    add("behind", sp, ep, 0, [(0, observe(0, sp, ep))])
    sp = np.array([-0.75, 0.5, 5.0]); ep = np.array([1.25, 0.5, 5.0])                   # parallel to x seen from the identity pose: l1 == 0
    add("horizontal", sp, ep, 0, [(0, observe(0, sp, ep))])
    sp = np.array([0.25, -0.75, 4.0]); ep = np.array([0.25, 1.0, 4.0])                  # parallel to y: l2 == 0
    add("vertical", sp, ep, 0, [(0, observe(0, sp, ep))])
    sp, ep = seg()
    add("moved", sp, ep, 0, [(0, observe(0, sp, ep))])
    sp, ep = seg()
    add("nan_pose", sp, ep, F + 1, [(F + 1, len(slots[F + 1]))])
    slots[F + 1].append((100.0, 120.0, 300.0, 200.0))
    assert tuple(directed) == DIRECTED
    counts = np.array([len(s) for s in slots], np.int32)
    cap = int(counts.max()) + slack
    keylines = np.zeros((FT, cap), plp.KL_DTYPE)
    for name in ("startPointX", "startPointY", "endPointX", "endPointY"):
        keylines[name] = rng.uniform(0.0, 600.0, (FT, cap)).astype(np.float32)          # unused slots: any segment
    for f in range(FT):
        for j, s in enumerate(slots[f]):
            keylines["startPointX"][f, j], keylines["startPointY"][f, j], keylines["endPointX"][f, j], keylines["endPointY"][f, j] = s
    L = len(lines)
    obs[directed["idx_at_counts"]] = [(0, int(counts[0]))]
    obs_offsets = np.zeros(L + 1, np.int32)
    obs_offsets[1:] = np.cumsum([len(o) for o in obs])
    obs_kf = np.array([k for o in obs for k, _ in o], np.int32)
    obs_idx = np.array([i for o in obs for _, i in o], np.int32)
    true_pos = np.array([np.concatenate([sp, ep]) for sp, ep, _ in lines])
    pluecker = np.array([pluecker_of(sp, ep, rng.uniform(0.5, 2.0)) for sp, ep, _ in lines])
    pos_old = true_pos + rng.normal(0.0, 0.01, true_pos.shape)
    pos_old[directed["moved"], :3] += np.array([0.0, 1.0, 0.0])                          # 1.0 / median 5 = 0.2 > 0.1
    skip = np.zeros(L, np.uint8)
    skip[directed["erased"]] = 1
    return dict(camera=camera(), cam=CAM, pose=pose, kf_erased=kf_erased, keylines=keylines, counts=counts, median_depth=np.full(FT, 5.0, np.float32),
                pluecker=pluecker, true_pos_w=true_pos, pos_w_old=pos_old, ref_kf=np.array([r for _, _, r in lines], np.int32), skip=skip,
                obs_offsets=obs_offsets, obs_kf=obs_kf, obs_idx=obs_idx, directed=directed, undirected=n_lines, F_live=F)


def trim_kwargs(sc, mode, counts=True):
    """the keyword arguments of (model_)trim_line_endpoints and of line_update_ref.trim_line_endpoints but the camera"""
    kw = dict(pluecker=sc["pluecker"], ref_kf=sc["ref_kf"], obs_offsets=sc["obs_offsets"], obs_kf=sc["obs_kf"], obs_idx=sc["obs_idx"], pose=sc["pose"],
              keylines=sc["keylines"], mode=mode, skip=sc["skip"], kf_erased=sc["kf_erased"], counts=sc["counts"] if counts else None)
    if mode == 1:
        kw.update(pos_w_old=sc["pos_w_old"], median_depth=sc["median_depth"])
    return kw


def same_bits(a, b):
    """equal bit for bit, a NaN equal to any NaN (its sign and payload are the processor's)"""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind != "f":
        return bool(np.array_equal(a, b))
    u = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    nan = np.isnan(a) & np.isnan(b)
    return bool(np.all(nan | (a.view(u) == b.view(u))))


def random_sim3(rng, F, scale_spread=0.05):
    """(sim3_cw, corrected_wc) (F, 8) {qx, qy, qz, qw, tx, ty, tz, s}: unit quaternions, scales around 1"""
    out = []
    for _ in range(2):
        q = rng.normal(0.0, 1.0, (F, 4))
        q[:, 3] = np.abs(q[:, 3]) + 2.0
        q /= np.linalg.norm(q, axis=1, keepdims=True)
        out.append(np.concatenate([q, rng.uniform(-1.0, 1.0, (F, 3)), 1.0 + rng.uniform(-scale_spread, scale_spread, (F, 1))], axis=1))
    return out[0], out[1]


def correct_case(sc, seed):
    """the keyword arguments of (model_)correct_landmark_lines over a scene: random Sim3 rows, corr_kf differing from ref_kf on every fifth line and outside
    the table on one, the scene's skip and kf_erased"""
    rng = np.random.default_rng(seed)
    FT, L = len(sc["pose"]), len(sc["pluecker"])
    cw, wc = random_sim3(rng, FT)
    corr = sc["ref_kf"].copy()
    corr[::5] = rng.integers(0, sc["F_live"], len(corr[::5]))
    if L > 3:
        corr[3] = FT + 1
    return dict(pluecker=sc["pluecker"], ref_kf=sc["ref_kf"], sim3_cw=cw, corrected_wc=wc, corr_kf=corr, lm_erased=sc["skip"], kf_erased=sc["kf_erased"])


def propagate_case(sc, seed):
    """the keyword arguments of (model_)loop_ba_propagate_lines over a scene: the scene's poses before, moved poses after, every key-frame status, some lines
    optimised"""
    rng = np.random.default_rng(seed)
    FT, L = len(sc["pose"]), len(sc["pluecker"])
    after = np.zeros((FT, 15))
    for f in range(FT):
        R = _rot(*rng.uniform(-0.05, 0.05, 3)) @ sc["pose"][f, :9].reshape(3, 3)
        after[f] = pose_row(R, sc["pose"][f, 9:12] + rng.uniform(-0.2, 0.2, 3))
    status = rng.integers(1, 3, FT).astype(np.uint8)
    status[sc["F_live"]] = 3
    if sc["F_live"] > 2:
        status[sc["F_live"] - 1] = 0
    opt = (rng.uniform(0, 1, L) < 0.3).astype(np.uint8)
    return dict(pose_after=after, pose_before=np.ascontiguousarray(sc["pose"][:, :12]), kf_status=status, pluecker=sc["pluecker"], ref_kf=sc["ref_kf"],
                line_optimized=opt, pluecker_after=sc["pluecker"] + rng.normal(0, 0.01, sc["pluecker"].shape), lm_erased=sc["skip"])


def map_lines(seed, pose, kf_erased, n_lines, max_obs=4, slack=3, cam=CAM):
    """Line landmarks for a map whose key frames are given (pose (F, >= 12), any layout of cameras): every line is a segment in front of its reference key
    frame, seen by it and up to max_obs - 1 others in key-line slots of their own; some lines erased, a few with a reference key frame that is erased or
    outside the table, one with no observation.  Returns (kl (F, cap) KL_DTYPE, kl_counts (F,), dict of the *_lines tables)."""
    rng = np.random.default_rng(seed)
    F = len(pose)
    live = [f for f in range(F) if not kf_erased[f]]
    slots = [[] for _ in range(F)]
    pk, pos, ref, obs = [], [], [], []
    for l in range(n_lines):
        r = int(live[int(rng.integers(0, len(live)))])
        Rm, t = pose[r, :9].reshape(3, 3), pose[r, 9:12]
        sc_ = np.array([rng.uniform(-1.5, 1.5), rng.uniform(-1.0, 1.0), rng.uniform(3.0, 8.0)])
        ec_ = sc_ + rng.uniform(-1.0, 1.0, 3) * np.array([1.0, 1.0, 0.5])
        sp, ep = Rm.T @ (sc_ - t), Rm.T @ (ec_ - t)
        kfs = [r] + [int(k) for k in rng.permutation(live)[:int(rng.integers(0, max_obs))] if k != r]
        rng.shuffle(kfs)
        o = []
        for k in kfs:
            a, b = project(pose[k], sp, cam), project(pose[k], ep, cam)
            slots[k].append((a[0], a[1], b[0], b[1]))
            o.append((k, len(slots[k]) - 1))
        pk.append(pluecker_of(sp, ep, rng.uniform(0.5, 2.0)))
        pos.append(np.concatenate([sp, ep]) + rng.normal(0.0, 0.01, 6))
        ref.append(r)
        obs.append(o)
    ref = np.array(ref, np.int32)
    skip = (rng.uniform(size=n_lines) < 0.08).astype(np.uint8)
    erased = np.flatnonzero(kf_erased)
    if n_lines > 12:
        ref[5] = F + 2
        ref[9] = erased[0] if len(erased) else -1
        obs[11] = []
    counts = np.array([len(s) for s in slots], np.int32)
    cap = int(counts.max()) + slack
    kl = np.zeros((F, cap), plp.KL_DTYPE)
    for name in ("startPointX", "startPointY", "endPointX", "endPointY"):
        kl[name] = rng.uniform(0.0, 600.0, (F, cap)).astype(np.float32)
    for f in range(F):
        for j, s in enumerate(slots[f]):
            kl["startPointX"][f, j], kl["startPointY"][f, j], kl["endPointX"][f, j], kl["endPointY"][f, j] = s
    off = np.zeros(n_lines + 1, np.int32)
    off[1:] = np.cumsum([len(o) for o in obs])
    return kl, counts, dict(pluecker_lines=np.array(pk), pos_w_lines=np.array(pos), ref_kf_lines=ref, skip_lines=skip, obs_offsets_lines=off,
                            obs_kf_lines=np.array([k for o in obs for k, _ in o], np.int32), obs_idx_lines=np.array([i for o in obs for _, i in o], np.int32))


def take(sc, idx):
    """the scene with the lines idx only, in that order (the observation lists rebuilt)"""
    idx = np.asarray(idx, np.int64)
    off = sc["obs_offsets"]
    parts = [np.arange(off[l], off[l + 1]) for l in idx]
    sel = np.concatenate(parts).astype(np.int64) if len(parts) else np.zeros(0, np.int64)
    new_off = np.zeros(len(idx) + 1, np.int32)
    new_off[1:] = np.cumsum([len(p) for p in parts])
    out = dict(sc, obs_offsets=new_off, obs_kf=sc["obs_kf"][sel], obs_idx=sc["obs_idx"][sel])
    for k in ("pluecker", "true_pos_w", "pos_w_old", "ref_kf", "skip"):
        out[k] = np.ascontiguousarray(sc[k][idx])
    return out
