"""Seeded map tables with line landmarks for the tests of the local adjuster with lines (tests/test_local_ba_lines_cpu.py,
tests/test_gpu_local_ba_lines.py): tests/local_ba_scene.py's key frames and landmarks, and 3-D segments whose end points are projected into the key
frames as key lines (floats), with optional pixel noise and displaced end points, perturbed start lines; the tables as the arrays of
plp_local_ba_lines_args and as tests/local_ba_lines_ref.py values."""
import numpy as np

import local_ba_lines_ref as LREF
import local_ba_scene as S
import pose_optimizer_scene as PS
from plp import plp

MONO, STEREO, RGBD = S.MONO, S.STEREO, S.RGBD
INV_SIGMA_SQ_LSD = np.array([1.0, 0.51, 0.26, 0.13, 0.07], np.float32)


def pluecker(s, e):
    d = (e - s) / np.linalg.norm(e - s)
    return np.concatenate([np.cross(s, d), d])


def add_lines(sc, seed, n_ln=12, obs_share=0.8, min_obs=2, noise=0.0, outliers=0, ln_noise=0.02, kl_stride=None, rows=None, octaves=4):
    """the scene `sc` of S.make_scene with n_ln line landmarks seen by its key frames `rows` (default: every key frame that is local or not erased and
    sees landmarks): keylines (F, KL), kl_counts, pluecker start, pluecker_gt, obs_offsets_lines, obs_kf_lines, obs_idx_lines, label_lines (TL,) 1 = an
    end point displaced, line_erased, ends_gt (LL, 6)"""
    rng = np.random.default_rng(seed)
    m, fx, fy, cx, cy, fxb = PS.CAMERAS[sc["model"]]
    F = len(sc["pose"])
    rows = [f for f in range(F) if sc["counts"][f] > 0] if rows is None else list(rows)
    kls = [[] for _ in range(F)]
    obs, label, ends = [], [], []
    for l in range(n_ln):
        c = np.array([rng.uniform(-1.8, 1.8), rng.uniform(-1.0, 1.0), rng.uniform(4.5, 8.5)])
        h = rng.normal(size=3); h = h / np.linalg.norm(h) * rng.uniform(0.3, 0.8)
        s, e = c - h, c + h
        ends.append(np.concatenate([s, e]))
        seen = [f for f in rows if rng.random() < obs_share]
        while len(seen) < min(min_obs, len(rows)):
            f = rows[int(rng.integers(len(rows)))]
            if f not in seen:
                seen.append(f)
        rng.shuffle(seen)
        lst = []
        for f in seen:
            Rm, t = sc["pose_gt"][f, :9].reshape(3, 3), sc["pose_gt"][f, 9:12]
            octave = int(rng.integers(0, octaves))
            sd = noise * 1.2 ** octave
            # a key line is a piece of the projected line: its end points slide along the segment
            a, b = rng.uniform(0.0, 0.2), rng.uniform(0.8, 1.0)
            px = []
            for p in (s + a * (e - s), s + b * (e - s)):
                pc = Rm @ p + t
                px += [fx * pc[0] / pc[2] + cx + rng.normal() * sd, fy * pc[1] / pc[2] + cy + rng.normal() * sd]
            lst.append((f, len(kls[f])))
            kls[f].append(px + [octave])
            label.append(0)
        obs.append(lst)
    TL = len(label)
    offs = np.cumsum([0] + [len(o) for o in obs])
    for t in rng.choice(TL, size=min(outliers, TL), replace=False) if outliers else []:
        l = int(np.searchsorted(offs, t, side="right")) - 1
        lo = int(offs[l])
        if any(label[lo:lo + len(obs[l])]) or len(obs[l]) < 3:   # at most one per line, and only where the other views still fix the line
            continue
        f, idx = obs[l][t - lo]
        # across the key line: a displacement along it leaves the distance to the projected line as it was
        k = kls[f][idx]
        nrm = np.array([-(k[3] - k[1]), k[2] - k[0]]); nrm = nrm / np.linalg.norm(nrm)
        d = rng.uniform(30.0, 60.0) * (1.0 if rng.random() < 0.5 else -1.0)
        k[0] += d * nrm[0]; k[1] += d * nrm[1]
        label[t] = 1
    KL = max(max(len(k) for k in kls) + 2, 1) if kl_stride is None else kl_stride
    keylines = np.zeros((F, KL), plp.KL_DTYPE)
    keylines["octave"] = 99
    for f in range(F):
        for i, (xs, ys, xe, ye, o) in enumerate(kls[f]):
            k = keylines[f, i]
            k["startPointX"], k["startPointY"], k["endPointX"], k["endPointY"], k["octave"] = xs, ys, xe, ye, o
    ends = np.array(ends).reshape(-1, 6)
    gt = np.array([pluecker(r[:3], r[3:]) for r in ends]).reshape(-1, 6)
    start = np.array([pluecker(r[:3] + rng.normal(size=3) * ln_noise, r[3:] + rng.normal(size=3) * ln_noise) for r in ends]).reshape(-1, 6)
    out = dict(sc)
    out.update(keylines=keylines, kl_counts=np.array([len(k) for k in kls], np.int32), pluecker=start, pluecker_gt=gt, ends_gt=ends,
               obs_offsets_lines=offs.astype(np.int32), obs_kf_lines=np.array([f for o in obs for f, _ in o], np.int32),
               obs_idx_lines=np.array([i for o in obs for _, i in o], np.int32), label_lines=np.array(label, np.uint8), line_erased=np.zeros(n_ln, np.uint8))
    return out


def make_scene(seed, n_free=3, n_fixed=2, n_lm=40, n_ln=12, line_obs_share=0.8, line_min_obs=2, line_noise=None, line_outliers=0, ln_noise=0.02, line_octaves=4, **kw):
    sc = S.make_scene(seed, n_free, n_fixed, n_lm, **kw)
    return add_lines(sc, seed + 1000, n_ln, line_obs_share, line_min_obs, kw.get("noise", 0.0) if line_noise is None else line_noise, line_outliers, ln_noise, octaves=line_octaves)


def without_points(sc):
    """the scene with an empty landmark table"""
    out = dict(sc)
    out.update(pos_w=np.zeros((0, 3)), pos_gt=np.zeros((0, 3)), obs_offsets=np.zeros(1, np.int32), obs_kf=np.zeros(0, np.int32), obs_idx=np.zeros(0, np.int32),
               label=np.zeros(0, np.uint8), lm_erased=np.zeros(0, np.uint8))
    return out


def add_line(sc, ends, views, octave=0):
    """one more line through the end points `ends` (6,), seen noise-free by the key frames `views`; returns its row"""
    m, fx, fy, cx, cy, fxb = PS.CAMERAS[sc["model"]]
    l = len(sc["pluecker"])
    kf, idx = [], []
    for f in views:
        Rm, t = sc["pose_gt"][f, :9].reshape(3, 3), sc["pose_gt"][f, 9:12]
        i = int(sc["kl_counts"][f])
        assert i < sc["keylines"].shape[1]
        k = sc["keylines"][f, i]
        ps, pe = Rm @ ends[:3] + t, Rm @ ends[3:] + t
        k["startPointX"], k["startPointY"] = fx * ps[0] / ps[2] + cx, fy * ps[1] / ps[2] + cy
        k["endPointX"], k["endPointY"] = fx * pe[0] / pe[2] + cx, fy * pe[1] / pe[2] + cy
        k["octave"] = octave
        sc["kl_counts"][f] += 1
        kf.append(f); idx.append(i)
    p = pluecker(ends[:3], ends[3:])[None]
    sc["pluecker"] = np.concatenate([sc["pluecker"], p]); sc["pluecker_gt"] = np.concatenate([sc["pluecker_gt"], p]); sc["ends_gt"] = np.concatenate([sc["ends_gt"], ends[None]])
    sc["obs_kf_lines"] = np.concatenate([sc["obs_kf_lines"], np.array(kf, np.int32)]); sc["obs_idx_lines"] = np.concatenate([sc["obs_idx_lines"], np.array(idx, np.int32)])
    sc["obs_offsets_lines"] = np.concatenate([sc["obs_offsets_lines"], np.array([len(sc["obs_kf_lines"])], np.int32)])
    sc["label_lines"] = np.concatenate([sc["label_lines"], np.zeros(len(views), np.uint8)]); sc["line_erased"] = np.concatenate([sc["line_erased"], np.zeros(1, np.uint8)])
    return l


def call_args(sc, kf_local=None, **kw):
    a = S.call_args(sc, kf_local)
    a.update(keylines=sc["keylines"], pluecker=sc["pluecker"], obs_offsets_lines=sc["obs_offsets_lines"], obs_kf_lines=sc["obs_kf_lines"], obs_idx_lines=sc["obs_idx_lines"],
             inv_level_sigma_sq_lsd=sc.get("sigma_lsd", INV_SIGMA_SQ_LSD), kl_counts=sc["kl_counts"], line_erased=sc["line_erased"])
    a.update(kw)
    return a


def ref_tables(sc):
    F, LL = len(sc["pose"]), len(sc["pluecker"])
    kc = sc["kl_counts"] if sc["kl_counts"] is not None else np.full(F, sc["keylines"].shape[1])
    kls = []
    for f in range(F):
        k = sc["keylines"][f]
        kls.append([(float(k["startPointX"][i]), float(k["startPointY"][i]), float(k["endPointX"][i]), float(k["endPointY"][i]), int(k["octave"][i]))
                    for i in range(max(0, min(int(kc[f]), len(k))))])
    oo = sc["obs_offsets_lines"]
    obs = [[(t, int(sc["obs_kf_lines"][t]), int(sc["obs_idx_lines"][t])) for t in range(int(oo[l]), int(oo[l + 1]))] for l in range(LL)]
    le = None if sc["line_erased"] is None else [int(x) for x in sc["line_erased"]]
    return LREF.LineTables(S.ref_tables(sc), sc.get("sigma_lsd", INV_SIGMA_SQ_LSD), kls, [[float(v) for v in r] for r in sc["pluecker"]], obs, le)


def dims(sc):
    return len(sc["pose"]), len(sc["pos_w"]), len(sc["obs_kf"]), len(sc["pluecker"]), len(sc["obs_kf_lines"])


def sentinel_out(G, F, L, T, LL, TL):
    o = S.sentinel_out(G, F, L, T)
    o.update(line_role=np.full((G, LL), 77, np.uint8), pluecker=np.full((G, LL, 6), -7.5), outlier_lines=np.full((G, TL), 77, np.uint8))
    return o


def expected(sc, kf_local, out, g, num_first_iter=5, num_second_iter=10):
    """the restatement's result of problem g written into the arrays `out` (model_local_ba_lines' dict, pre-filled by the caller); returns the result dict"""
    r = LREF.optimize(ref_tables(sc), [int(v) for v in kf_local], num_first_iter, num_second_iter)
    out["status"][g] = r["status"]
    out["kf_role"][g] = r["kf_role"]; out["lm_role"][g] = r["lm_role"]; out["line_role"][g] = r["line_role"]
    for f, p in r["pose"].items():
        out["pose"][g, f] = p
    for l, p in r["pos_w"].items():
        out["pos_w"][g, l] = p
    for l, p in r["pluecker"].items():
        out["pluecker"][g, l] = p
    for t, v in r["outlier"].items():
        out["outlier"][g, t] = v
    for t, v in r["outlier_lines"].items():
        out["outlier_lines"][g, t] = v
    out["round_info"][g] = r["round_info"]; out["round_chi2"][g] = r["round_chi2"]
    return r


def census():
    """name -> scene: what tests/test_local_ba_lines_cpu.py's census has to reach"""
    C = {}
    C["mono"] = make_scene(41, 3, 2, 40, 12, noise=0.8, outliers=4, line_outliers=3)
    C["rgbd"] = make_scene(42, 3, 2, 40, 12, setup=RGBD, noise=0.6, outliers=4, line_outliers=3)
    C["fisheye"] = make_scene(43, 2, 2, 20, 8, model="fisheye", noise=0.8, outliers=2, line_outliers=2)
    C["far_start"] = make_scene(44, 3, 2, 30, 10, noise=1.0, outliers=3, line_outliers=2, pose_noise=0.08, lm_noise=0.5, ln_noise=0.3)
    C["lines_only"] = without_points(make_scene(45, 2, 2, 5, 14, noise=0.5, line_outliers=2))
    s = make_scene(46, 2, 2, 25, 8, noise=0.5, n_other=2)
    # a key frame that only a line makes a constant vertex: the last one, neither local nor erased, sees no landmark
    s["kf_erased"][5] = 0
    s["undist"]["octave"][5] = 99; s["counts"][5] = 0
    keep = s["obs_kf"] != 5
    lm = np.repeat(np.arange(len(s["pos_w"])), np.diff(s["obs_offsets"]))[keep]
    s["obs_kf"], s["obs_idx"], s["label"] = s["obs_kf"][keep], s["obs_idx"][keep], s["label"][keep]
    s["obs_offsets"] = np.concatenate([[0], np.cumsum(np.bincount(lm, minlength=len(s["pos_w"])))]).astype(np.int32)
    add_line(s, np.array([-0.5, 0.2, 6.0, 0.6, -0.3, 6.5]), [0, 1, 5])
    # a line behind its only observer, a local key frame: its edge fits and fails the depth test alone, and the line leaves round 2
    Rm, t = s["pose_gt"][1, :9].reshape(3, 3), s["pose_gt"][1, 9:12]
    cen = -Rm.T @ t
    behind = np.concatenate([cen - 5.0 * Rm[2] + 0.4 * Rm[0] + 0.1 * Rm[1], cen - 6.0 * Rm[2] - 0.5 * Rm[0] + 0.3 * Rm[1]])
    add_line(s, behind, [1])
    C["through_a_line"] = s
    s = without_points(make_scene(47, 2, 1, 5, 6, line_obs_share=0.0, line_min_obs=1))   # every line seen once, no information: every 4 x 4 inverse fails
    s["sigma_lsd"] = np.zeros(5, np.float32)
    C["no_information"] = s
    s = make_scene(48, 2, 2, 20, 6, noise=0.5)
    s["kf_local"][:] = 0
    C["no_edges"] = s
    return C
