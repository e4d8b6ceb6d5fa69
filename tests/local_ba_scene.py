"""Seeded map tables for the local bundle adjuster's tests (tests/test_local_ba_cpu.py, tests/test_gpu_local_ba.py): key frames on an arc that look
at a cloud of landmarks, observations from the true projection (floats) with optional pixel noise and gross outliers, perturbed start poses and
positions; the tables as the arrays of plp_local_ba_args and as tests/local_ba_ref.py values."""
import numpy as np

import local_ba_ref as REF
import pose_optimizer_ref as R15
import pose_optimizer_scene as PS
from plp import plp

MONO, STEREO, RGBD = PS.MONO, PS.STEREO, PS.RGBD
INV_SIGMA_SQ = PS.INV_SIGMA_SQ


def make_scene(seed, n_free=3, n_fixed=2, n_lm=40, model="perspective", setup=MONO, noise=0.0, outliers=0, n_other=1, obs_share=0.8, min_obs=1, pose_noise=0.01,
               lm_noise=0.02, mono_share=0.3, kp_stride=None, pose_stride=15, origin=False, n_blind=0):
    """dict(camera, setup_type, pose (F, pose_stride) start, pose_gt (F, 12), undist (F, K), x_right (F, K), counts, pos_w start, pos_gt, obs_offsets, obs_kf,
    obs_idx, label (T,) 1 = displaced observation, kf_local (F,), kf_erased, kf_is_origin, lm_erased).  Key frames 0 .. n_free - 1 are local, the next
    n_fixed see the same landmarks, n_other more are marked erased and appear in some observation lists, n_blind more are local and observe nothing."""
    rng = np.random.default_rng(seed)
    m, fx, fy, cx, cy, fxb = PS.CAMERAS[model]
    F = n_free + n_fixed + n_other + n_blind
    FS = F - n_blind                                         # the key frames that see landmarks
    Rs, ts = [], []
    for f in range(F):
        Rm = PS.rodrigues(rng.normal(size=3) * 0.05 + np.array([0.0, 0.08 * (f - F / 2), 0.0]))
        c = np.array([0.4 * (f - F / 2), rng.normal() * 0.1, rng.normal() * 0.1])
        Rs.append(Rm); ts.append(-Rm @ c)
    pos = np.stack([rng.uniform(-2.0, 2.0, n_lm), rng.uniform(-1.2, 1.2, n_lm), rng.uniform(4.0, 9.0, n_lm)], 1)
    kps = [[] for _ in range(F)]
    obs = []
    label = []
    for l in range(n_lm):
        seen = [f for f in range(FS) if rng.random() < obs_share]
        while len(seen) < min(min_obs, FS):
            f = int(rng.integers(FS))
            if f not in seen:
                seen.append(f)
        rng.shuffle(seen)
        lst = []
        for f in seen:
            pc = Rs[f] @ pos[l] + ts[f]
            octave = int(rng.integers(0, 4))
            sd = noise * 1.2 ** octave
            u = fx * pc[0] / pc[2] + cx + rng.normal() * sd
            v = fy * pc[1] / pc[2] + cy + rng.normal() * sd
            xr = -1.0
            if setup != MONO and rng.random() >= mono_share:
                xr = u - fxb / pc[2] + rng.normal() * sd
            lst.append((f, len(kps[f])))
            kps[f].append([u, v, octave, xr])
            label.append(0)
        obs.append(lst)
    T = len(label)
    offs = np.cumsum([0] + [len(o) for o in obs])
    for t in rng.choice(T, size=min(outliers, T), replace=False) if outliers else []:
        # at most one displaced observation per landmark
        l = int(np.searchsorted(offs, t, side="right")) - 1
        lo = int(offs[l])
        if any(label[lo:lo + len(obs[l])]):
            continue
        f, idx = obs[l][t - lo]
        ang = rng.uniform(0, 2 * np.pi)
        d = rng.uniform(20.0, 60.0)
        kps[f][idx][0] += d * np.cos(ang); kps[f][idx][1] += d * np.sin(ang)
        label[t] = 1
    K = max(max(len(k) for k in kps) + 3, 1) if kp_stride is None else kp_stride
    undist = np.zeros((F, K), plp.KP_DTYPE)
    undist["octave"] = 99                                    # slots behind counts: out of the sigma table
    x_right = np.full((F, K), 5.0, np.float32)
    counts = np.array([len(k) for k in kps], np.int32)
    for f in range(F):
        for i, (u, v, o, xr) in enumerate(kps[f]):
            undist["x"][f, i], undist["y"][f, i], undist["octave"][f, i] = u, v, o
            x_right[f, i] = xr
    pose_gt = np.array([np.concatenate([Rs[f].reshape(-1), ts[f]]) for f in range(F)])
    pose = np.full((F, pose_stride), 7.0)
    for f in range(F):
        Rm, t = Rs[f], ts[f]
        if f < n_free and not (origin and f == 0):
            Rm = PS.rodrigues(rng.normal(size=3) * pose_noise) @ Rm
            t = t + rng.normal(size=3) * pose_noise * 3
        pose[f, :9] = Rm.reshape(-1); pose[f, 9:12] = t
    kf_local = np.zeros(F, np.uint8); kf_local[:n_free] = 1; kf_local[FS:] = 1
    kf_erased = np.zeros(F, np.uint8); kf_erased[n_free + n_fixed:FS] = 1
    kf_is_origin = np.zeros(F, np.uint8); kf_is_origin[0] = int(origin)
    return dict(camera=PS.camera(model), model=model, setup_type=setup, pose=pose, pose_gt=pose_gt, undist=undist, x_right=x_right if setup != MONO else None, counts=counts,
                pos_w=pos + rng.normal(size=pos.shape) * lm_noise, pos_gt=pos, obs_offsets=np.cumsum([0] + [len(o) for o in obs]).astype(np.int32),
                obs_kf=np.array([f for o in obs for f, _ in o], np.int32), obs_idx=np.array([i for o in obs for _, i in o], np.int32),
                label=np.array(label, np.uint8), kf_local=kf_local, kf_erased=kf_erased, kf_is_origin=kf_is_origin, lm_erased=np.zeros(n_lm, np.uint8))


def call_args(S, kf_local=None, **kw):
    a = dict(camera=S["camera"], setup_type=S["setup_type"], pose=S["pose"], undist=S["undist"], pos_w=S["pos_w"], obs_offsets=S["obs_offsets"], obs_kf=S["obs_kf"],
             obs_idx=S["obs_idx"], kf_local=S["kf_local"] if kf_local is None else kf_local, inv_level_sigma_sq=S.get("sigma", INV_SIGMA_SQ), x_right=S["x_right"],
             counts=S["counts"], kf_erased=S["kf_erased"], kf_is_origin=S["kf_is_origin"], lm_erased=S["lm_erased"])
    a.update(kw)
    return a


def ref_tables(S):
    m, fx, fy, cx, cy, fxb = PS.CAMERAS[S["model"]]
    F, L = len(S["pose"]), len(S["pos_w"])
    counts = S["counts"] if S["counts"] is not None else np.full(F, S["undist"].shape[1])
    kps = []
    for f in range(F):
        k = S["undist"][f]
        kps.append([(float(k["x"][i]), float(k["y"][i]), int(k["octave"][i]), float(S["x_right"][f, i]) if S["x_right"] is not None else -1.0)
                    for i in range(max(0, min(int(counts[f]), len(k))))])
    oo = S["obs_offsets"]
    obs = [[(t, int(S["obs_kf"][t]), int(S["obs_idx"][t])) for t in range(int(oo[l]), int(oo[l + 1]))] for l in range(L)]
    none = lambda v: None if v is None else [int(x) for x in v]
    return REF.Tables(R15.Cam(fx, fy, cx, cy, fxb), S["setup_type"] == MONO, S.get("sigma", INV_SIGMA_SQ), [[float(v) for v in r] for r in S["pose"]], kps,
                      [[float(v) for v in r] for r in S["pos_w"]], obs, none(S["kf_erased"]), none(S["kf_is_origin"]), none(S["lm_erased"]))


def expected(S, kf_local, out, g, num_first_iter=5, num_second_iter=10):
    """the restatement's result of problem g written into the arrays `out` (model_local_ba's dict, pre-filled by the caller); returns the result dict"""
    r = REF.optimize(ref_tables(S), [int(v) for v in kf_local], num_first_iter, num_second_iter)
    out["status"][g] = r["status"]
    out["kf_role"][g] = r["kf_role"]; out["lm_role"][g] = r["lm_role"]
    for f, p in r["pose"].items():
        out["pose"][g, f] = p
    for l, p in r["pos_w"].items():
        out["pos_w"][g, l] = p
    for t, v in r["outlier"].items():
        out["outlier"][g, t] = v
    out["round_info"][g] = r["round_info"]; out["round_chi2"][g] = r["round_chi2"]
    return r


def sentinel_out(G, F, L, T):
    return dict(status=np.full(G, 77, np.uint8), kf_role=np.full((G, F), 77, np.uint8), lm_role=np.full((G, L), 77, np.uint8), pose=np.full((G, F, 15), -7.5),
                pos_w=np.full((G, L, 3), -7.5), outlier=np.full((G, T), 77, np.uint8), round_info=np.full((G, 2, 4), -7, np.int32), round_chi2=np.full((G, 2, 2), -7.5))


def same(a, b):
    """bit for bit; a NaN equals a NaN (sign and payload are the machine's, as in tests/test_pose_optimizer_cpu.py)"""
    for k in a:
        x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
        if x.shape != y.shape or x.dtype != y.dtype:
            return False
        if x.dtype.kind == "f":
            if not np.array_equal(np.isnan(x), np.isnan(y)) or np.nan_to_num(x, nan=0.0).tobytes() != np.nan_to_num(y, nan=0.0).tobytes():
                return False
        elif x.tobytes() != y.tobytes():
            return False
    return True


def spread(S, rows, F):
    """the scene with its key frames moved to the table rows `rows` of a table of F rows; the other rows are key frames nothing observes (not local, not
    erased, no key point)"""
    rows = np.asarray(rows)
    assert len(rows) == len(S["pose"]) and len(set(rows.tolist())) == len(rows) and rows.max() < F
    out = dict(S)
    pose = np.full((F, S["pose"].shape[1]), 7.0); pose[:, :12] = [1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0]; pose[rows] = S["pose"]
    gt = np.tile(np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], float), (F, 1)); gt[rows] = S["pose_gt"]
    undist = np.zeros((F, S["undist"].shape[1]), S["undist"].dtype); undist["octave"] = 99; undist[rows] = S["undist"]
    def put(v, fill, dtype):
        if v is None:
            return None
        o = np.full((F,) + v.shape[1:], fill, dtype); o[rows] = v
        return o
    out.update(pose=pose, pose_gt=gt, undist=undist, x_right=put(S["x_right"], 5.0, np.float32), counts=put(S["counts"], 0, np.int32),
               kf_local=put(S["kf_local"], 0, np.uint8), kf_erased=put(S["kf_erased"], 0, np.uint8), kf_is_origin=put(S["kf_is_origin"], 0, np.uint8),
               obs_kf=rows[S["obs_kf"]].astype(np.int32))
    return out


def displace(S, t, d=40.0):
    """observation entry t becomes a gross outlier"""
    S["undist"]["x"][S["obs_kf"][t], S["obs_idx"][t]] += np.float32(d)
    S["label"][t] = 1


def census():
    """name -> scene: what tests/test_local_ba_cpu.py's census has to reach, and a spread of set-ups, models and sizes"""
    C = {}
    C["mono"] = make_scene(11, 3, 2, 60, noise=0.8, outliers=6, n_blind=1)
    C["rgbd"] = make_scene(12, 4, 3, 80, setup=RGBD, noise=0.8, outliers=8)
    C["fisheye"] = make_scene(13, 2, 1, 20, model="fisheye", noise=1.0, outliers=2, obs_share=0.5)
    C["fisheye_rgbd"] = make_scene(14, 6, 4, 120, model="fisheye", setup=RGBD, noise=0.6, outliers=10)
    C["large"] = make_scene(15, 5, 4, 300, setup=STEREO, noise=0.7, outliers=20, obs_share=0.85)
    C["far_start"] = make_scene(16, 3, 2, 40, noise=1.5, outliers=4, pose_noise=0.08, lm_noise=0.5)
    C["at_truth"] = make_scene(17, 2, 2, 30, pose_noise=0.0, lm_noise=0.0)                      # rho == 0 ends optimize()
    s = make_scene(18, 2, 2, 25, noise=0.5)                                                      # no information: ten failed solves end optimize()
    s["sigma"] = INV_SIGMA_SQ.copy(); s["sigma"][:4] = 0.0
    C["no_information"] = s
    s = make_scene(19, 3, 2, 50, noise=0.5, obs_share=0.35)                                      # a landmark seen once loses its only edge
    once = [l for l in range(50) if s["obs_offsets"][l + 1] - s["obs_offsets"][l] == 1 and s["obs_kf"][s["obs_offsets"][l]] < 5]
    displace(s, int(s["obs_offsets"][once[0]]), 60.0)
    C["seen_once"] = s
    s = make_scene(20, 3, 2, 40, noise=0.5)                                                      # a landmark starts behind a fixed camera
    t = int(np.where(s["obs_kf"] == 3)[0][0])
    l = int(np.searchsorted(s["obs_offsets"], t, side="right") - 1)
    Rm, tr = s["pose_gt"][3, :9].reshape(3, 3), s["pose_gt"][3, 9:12]
    s["pos_w"][l] = -Rm.T @ tr - 2.0 * Rm[2]
    C["behind"] = s
    s = make_scene(21, 2, 2, 30, noise=0.5)                                                      # 0 / 0: a landmark in a fixed camera's centre
    s["pose"][2, :12] = [1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0]
    t = int(np.where(s["obs_kf"] == 2)[0][0])
    l = int(np.searchsorted(s["obs_offsets"], t, side="right") - 1)
    s["pos_w"][l] = 0.0
    C["nan"] = s
    C["no_free_pose"] = make_scene(22, 1, 2, 30, noise=0.5, origin=True)
    s = make_scene(23, 2, 2, 20, noise=0.5)
    s["kf_local"][:] = 0
    C["no_edges"] = s
    return C
