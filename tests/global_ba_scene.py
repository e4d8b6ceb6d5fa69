"""Seeded maps for the global bundle adjuster's tests (tests/test_global_ba_cpu.py, tests/test_gpu_global_ba.py, tests/test_gpu_loop_ba_step.py), built on
tests/local_ba_scene.make_scene: key frame 0 is the origin at its true pose, the other key frames and the landmarks start perturbed; spanning trees with
key frames the adjuster did not optimise for the loop adjuster's map update."""
import numpy as np

import global_ba_ref as REF
import local_ba_scene as LS

MONO, STEREO, RGBD = LS.MONO, LS.STEREO, LS.RGBD


def make(seed, P, n_lm, setup=RGBD, model="perspective", per_kf=None, **kw):
    """P free key frames behind the origin; per_kf: about that many observations per key frame (default: make_scene's obs_share)"""
    if per_kf is not None:
        kw.setdefault("obs_share", min(1.0, per_kf / n_lm))
        kw.setdefault("min_obs", 2)
    kw.setdefault("n_other", 0)
    return LS.make_scene(seed, n_free=P + 1, n_fixed=0, n_lm=n_lm, model=model, setup=setup, origin=True, **kw)


def call_args(S, **kw):
    a = LS.call_args(S)
    a.pop("kf_local")
    a.update(kw)
    return a


def dims(S):
    return len(S["pose"]), len(S["pos_w"]), len(S["obs_kf"])


def sentinel_out(S, names=None):
    from plp import plp
    F, L, T = dims(S)
    return {k: np.full(shape(F, L, T), REF.SENTINEL[k], dt) for k, (shape, dt, _) in plp.GLOBAL_BA_OUTPUTS.items() if names is None or k in names}


def expected(S, num_iter=10, use_huber_kernel=True, stop=False):
    """the restatement's result written over sentinels; returns (arrays, result dict)"""
    r = REF.optimize(LS.ref_tables(S), num_iter, use_huber_kernel, stop)
    out = sentinel_out(S)
    out["status"][0] = r["status"]
    if r["status"] == REF.STOPPED:
        return out, r
    out["kf_optimized"][:] = r["kf_optimized"]; out["lm_optimized"][:] = r["lm_optimized"]
    for f, p in r["pose"].items():
        out["pose"][f] = p
    for l, p in r["pos_w"].items():
        out["pos_w"][l] = p
    out["info"][:] = r["info"]; out["chi2"][:] = r["chi2"]
    return out, r


def census():
    """name -> (scene, num_iter, use_huber_kernel): what tests/test_global_ba_cpu.py's census has to reach; P <= 20"""
    C = {}
    C["mono_huber"] = (make(31, 5, 60, setup=MONO, noise=0.8, outliers=5), 6, True)
    C["rgbd_plain"] = (make(32, 8, 80, noise=0.8), 5, False)
    C["fisheye_stereo"] = (make(33, 6, 70, setup=STEREO, model="fisheye", noise=0.6, outliers=4), 5, True)
    C["p20"] = (make(34, 20, 120, noise=0.5, obs_share=0.3, min_obs=2), 3, False)
    C["far_start"] = (make(35, 4, 40, setup=MONO, noise=1.5, outliers=4, pose_noise=0.08, lm_noise=0.5), 8, True)
    C["at_truth"] = (make(36, 3, 30, pose_noise=0.0, lm_noise=0.0), 30, False)                # rho == 0 ends optimize()
    C["rejected"] = (make(55, 4, 40, setup=MONO, noise=1.0, pose_noise=0.15, lm_noise=1.0), 10, False)     # steps are rejected on the way down
    s = make(37, 3, 25, noise=0.5)
    s["sigma"] = LS.INV_SIGMA_SQ.copy(); s["sigma"][:4] = 0.0                                  # no information: ten failed solves end optimize()
    C["no_information"] = (s, 4, True)
    s = make(38, 3, 40, noise=0.5)                                                            # a landmark starts behind a camera
    t = int(np.where(s["obs_kf"] == 2)[0][0])
    l = int(np.searchsorted(s["obs_offsets"], t, side="right") - 1)
    Rm, tr = s["pose_gt"][2, :9].reshape(3, 3), s["pose_gt"][2, 9:12]
    s["pos_w"][l] = -Rm.T @ tr - 2.0 * Rm[2]
    C["behind"] = (s, 4, True)
    s = make(39, 2, 30, noise=0.5)                                                            # 0 / 0: a landmark in the origin's centre
    s["pose"][0, :12] = [1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0]
    t = int(np.where(s["obs_kf"] == 0)[0][0])
    l = int(np.searchsorted(s["obs_offsets"], t, side="right") - 1)
    s["pos_w"][l] = 0.0
    C["nan"] = (s, 3, True)
    s = make(40, 4, 50, noise=0.5, n_other=2, n_blind=1, obs_share=0.5)                       # erased key frames, a key frame without an edge
    s["lm_erased"][3] = 1
    lo, hi = s["obs_offsets"][7], s["obs_offsets"][8]
    s["obs_idx"][lo:hi] = 10 ** 6                                                             # landmark 7 has no edge
    C["holes"] = (s, 4, True)
    C["origin_only"] = (make(41, 0, 20, noise=0.5), 4, False)                                 # P = 0: the landmarks move against the constant origin
    s = make(42, 3, 20, noise=0.5)
    s["lm_erased"][:] = 1
    C["no_edges"] = (s, 4, True)
    return C


# ---- spanning trees for the loop adjuster's map update
def tree(name, seed=5, n_lm=40):
    """dict(pose (F, 15), kf_parent, kf_optimized, pose_after (F, 15), kf_erased, kf_is_origin, pos_w, ref_kf, lm_optimized, pos_after, lm_erased): key frame 0 is the
    origin; `name` picks the shape"""
    rng = np.random.default_rng(seed)
    shapes = dict(
        leaves=([-1, 0, 1, 1, 2, 2, 3], [1, 1, 1, 1, 1, 0, 0]),                     # unoptimised leaves
        deep=([-1, 0, 1, 2, 3, 4, 2, 6, 7], [1, 1, 1, 0, 0, 0, 0, 0, 1]),          # chains of unoptimised key frames two and three deep, an optimised one below them
        broken=([-1, 0, 1, 99, 3, -1, 5], [1, 1, 1, 0, 0, 1, 0]),                  # a parent outside the table, a second root
        cycle=([-1, 0, 1, 5, 3, 4, 6], [1, 1, 0, 0, 0, 1, 0]),                     # 3 -> 5 -> 4 -> 3, and 6 its own parent
        erased=([-1, 0, 1, 2, 3, 1], [1, 1, 1, 0, 0, 0]),                          # key frame 2 erased: its subtree is not reached
        origin_unoptimised=([-1, 0, 1, 2], [0, 0, 1, 0]))
    parent, opt = shapes[name]
    F = len(parent)
    def poses(scale):
        out = np.full((F, 15), 7.0)
        for f in range(F):
            Rm = LS.PS.rodrigues(rng.normal(size=3) * scale)
            out[f, :9] = Rm.reshape(-1); out[f, 9:12] = rng.normal(size=3)
            out[f, 12:15] = -Rm.T @ out[f, 9:12]
        return out
    pose, after = poses(0.4), poses(0.4)
    kf_erased = np.zeros(F, np.uint8)
    if name == "erased":
        kf_erased[2] = 1
    kf_is_origin = np.zeros(F, np.uint8); kf_is_origin[0] = 1
    ref = rng.integers(-1, F + 1, n_lm).astype(np.int32)
    lm_opt = (rng.random(n_lm) < 0.4).astype(np.uint8)
    lm_erased = (rng.random(n_lm) < 0.1).astype(np.uint8)
    return dict(pose=pose, kf_parent=np.array(parent, np.int32), kf_optimized=np.array(opt, np.uint8), pose_after=after, kf_erased=kf_erased,
                kf_is_origin=kf_is_origin, pos_w=rng.normal(size=(n_lm, 3)) * 3, ref_kf=ref, lm_optimized=lm_opt, pos_after=rng.normal(size=(n_lm, 3)) * 3,
                lm_erased=lm_erased)


TREES = ["leaves", "deep", "broken", "cycle", "erased", "origin_unoptimised"]


def prop_sentinel(Tr):
    from plp import plp
    F, L = len(Tr["pose"]), len(Tr["pos_w"])
    return {k: np.full(shape(F, L), REF.PROP_SENTINEL[k], dt) for k, (shape, dt) in plp.LOOP_BA_PROPAGATE_OUTPUTS.items()}


def prop_expected(Tr):
    r = REF.propagate(**{k: (v.tolist() if k not in ("pose", "pose_after", "pos_w", "pos_after") else v) for k, v in Tr.items()})
    out = prop_sentinel(Tr)
    out["kf_status"][:] = r["kf_status"]; out["lm_status"][:] = r["lm_status"]
    for f, p in r["pose"].items():
        out["pose"][f] = p
        out["pose_before"][f] = r["pose_before"][f]
    for l, p in r["pos_w"].items():
        out["pos_w"][l] = p
    return out, r
