"""Workload for profiles/r34_local_ba_lines.md: plp_local_ba_lines_device on one mapping-sized problem and on G = 8 of them over one map -- 50 key frames
every 0.3 m along a line, the problem's 20 local ones (19 free and the origin where it is among them) and the five on either side that its landmarks and lines
make constant vertices, 2 000 landmarks seen by the six key frames nearest to them and 300 lines seen by four to six, RGB-D, 0.5 px noise, perturbed start, the
adjuster's 5 and 10 iterations.  Equal bits with the CPU build of the same header (plp_model_local_ba_lines_host, one thread) are checked first; then every
device call runs six times on one stream, the first a warm-up, timed with device events, against the CPU build once and against plp_local_ba_device on the
same scene without its lines.

  python tools/local_ba_lines_bench.py [G ...]
"""
import importlib
import os
import sys
import time

import numpy as np

CALLS, F, L, LL, PER_LM, LOCAL = 6, 50, 2000, 300, 6, 20


def scene(plp, seed=1):
    import local_ba_lines_scene as LS
    import pose_optimizer_scene as PS
    rng = np.random.default_rng(seed)
    m, fx, fy, cx, cy, fxb = PS.CAMERAS["perspective"]
    cen = np.stack([0.3 * np.arange(F), rng.normal(size=F) * 0.05, rng.normal(size=F) * 0.05], 1)
    Rs = np.stack([PS.rodrigues(rng.normal(size=3) * 0.03) for _ in range(F)])
    ts = -np.einsum("fij,fj->fi", Rs, cen)
    proj = lambda f, p: (lambda pc: (fx * pc[0] / pc[2] + cx, fy * pc[1] / pc[2] + cy, pc[2]))(Rs[f] @ p + ts[f])
    # landmarks: the six key frames from `first` on see each
    first = np.minimum(rng.integers(0, F, L), F - PER_LM)
    pos = cen[first + PER_LM // 2] + np.stack([rng.uniform(-1.5, 1.5, L), rng.uniform(-1.0, 1.0, L), rng.uniform(4.0, 9.0, L)], 1)
    kps = [[] for _ in range(F)]
    obs_kf, obs_idx = [], []
    for l in range(L):
        for f in range(first[l], first[l] + PER_LM):
            u, v, z = proj(f, pos[l])
            obs_kf.append(f); obs_idx.append(len(kps[f]))
            kps[f].append((u + rng.normal() * 0.5, v + rng.normal() * 0.5, int(rng.integers(0, 4)), u - fxb / z + rng.normal() * 0.5))
    K = max(len(k) for k in kps) + 1
    undist = np.zeros((F, K), plp.KP_DTYPE); undist["octave"] = 99
    x_right = np.full((F, K), -1.0, np.float32)
    for f in range(F):
        for i, (u, v, o, xr) in enumerate(kps[f]):
            undist["x"][f, i], undist["y"][f, i], undist["octave"][f, i], x_right[f, i] = u, v, o, xr
    # lines: four to six key frames from `lfirst` on see each
    views = rng.integers(4, 7, LL)
    lfirst = np.minimum(rng.integers(0, F, LL), F - views)
    kls = [[] for _ in range(F)]
    pk, obs_kf_l, obs_idx_l, offs = [], [], [], [0]
    for l in range(LL):
        c = cen[lfirst[l] + views[l] // 2] + np.array([rng.uniform(-1.3, 1.3), rng.uniform(-0.8, 0.8), rng.uniform(4.5, 8.5)])
        h = rng.normal(size=3); h = h / np.linalg.norm(h) * rng.uniform(0.3, 0.8)
        s, e = c - h, c + h
        pk.append(LS.pluecker(s + rng.normal(size=3) * 0.02, e + rng.normal(size=3) * 0.02))
        for f in range(lfirst[l], lfirst[l] + views[l]):
            us, vs, _ = proj(f, s); ue, ve, _ = proj(f, e)
            obs_kf_l.append(f); obs_idx_l.append(len(kls[f]))
            kls[f].append((us + rng.normal() * 0.5, vs + rng.normal() * 0.5, ue + rng.normal() * 0.5, ve + rng.normal() * 0.5, int(rng.integers(0, 2))))
        offs.append(len(obs_kf_l))
    KL = max(len(k) for k in kls) + 1
    keylines = np.zeros((F, KL), plp.KL_DTYPE); keylines["octave"] = 99
    for f in range(F):
        for i, (xs, ys, xe, ye, o) in enumerate(kls[f]):
            k = keylines[f, i]
            k["startPointX"], k["startPointY"], k["endPointX"], k["endPointY"], k["octave"] = xs, ys, xe, ye, o
    pose = np.zeros((F, 15))
    for f in range(F):
        Rm, t = Rs[f], ts[f]
        if f:
            Rm = PS.rodrigues(rng.normal(size=3) * 0.005) @ Rm
            t = t + rng.normal(size=3) * 0.01
        pose[f, :9], pose[f, 9:12] = Rm.reshape(-1), t
    origin = np.zeros(F, np.uint8); origin[0] = 1
    points = dict(camera=PS.camera("perspective"), setup_type=PS.RGBD, pose=pose, undist=undist, x_right=x_right, counts=np.array([len(k) for k in kps], np.int32),
                  pos_w=pos + rng.normal(size=pos.shape) * 0.02, obs_offsets=(np.arange(L + 1) * PER_LM).astype(np.int32), obs_kf=np.array(obs_kf, np.int32),
                  obs_idx=np.array(obs_idx, np.int32), kf_is_origin=origin, inv_level_sigma_sq=PS.INV_SIGMA_SQ)
    lines = dict(keylines=keylines, kl_counts=np.array([len(k) for k in kls], np.int32), pluecker=np.array(pk), obs_offsets_lines=np.array(offs, np.int32),
                 obs_kf_lines=np.array(obs_kf_l, np.int32), obs_idx_lines=np.array(obs_idx_l, np.int32), inv_level_sigma_sq_lsd=PS.INV_SIGMA_SQ_LSD)
    return points, lines


def problems(G):
    """G windows of 20 local key frames, spread over the map"""
    kl = np.zeros((G, F), np.uint8)
    for g in range(G):
        a = (F - LOCAL) * g // max(G - 1, 1) if G > 1 else (F - LOCAL) // 2
        kl[g, a:a + LOCAL] = 1
    return kl


def run(sizes):
    import torch
    root = os.path.dirname(os.path.abspath(__file__))
    sys.path[:0] = [os.path.join(root, ".."), os.path.join(root, "..", "tests")]
    plp = importlib.import_module("structure-plp-slam_amd")
    mt = plp.matcher()
    points, lines = scene(plp)
    T, TL, K, KL = len(points["obs_kf"]), len(lines["obs_kf_lines"]), points["undist"].shape[1], lines["keylines"].shape[1]
    d = lambda v: torch.from_numpy((v.view(np.uint8) if v.dtype.fields else v).copy()).cuda()
    dev = {k: d(np.ascontiguousarray(v)) for k, v in {**points, **lines}.items() if isinstance(v, np.ndarray) and not k.startswith("inv_")}
    print(f"F {F}, L {L}, T {T}, LL {LL}, TL {TL}")
    print("| G | free / fixed key frames of problem 0 | iterations | rejected | to level 1 | with lines: device call (ms), calls 2-6 | mean | CPU build, one thread (ms) | CPU / device "
          "| points only: device (ms) | CPU (ms) |")
    print("|---|---|---|---|---|---|---|---|---|---|---|")

    def timed(call, want):
        times = []
        for _ in range(CALLS):
            o = {k: d(np.zeros_like(v)) for k, v in want.items()}
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call(o)
            e1.record()
            torch.cuda.synchronize()
            times.append(e0.elapsed_time(e1))
        return o, times[1:]
    for G in sizes:
        kl = problems(G)
        t0 = time.perf_counter()
        want = plp.model_local_ba_lines(**points, **lines, kf_local=kl)
        cpu_ms = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        want_p = plp.model_local_ba(**points, kf_local=kl)
        cpu_p_ms = (time.perf_counter() - t0) * 1e3
        dkl = d(kl)

        def with_lines(o):
            mt.local_ba_lines_device(points["camera"], points["setup_type"], G, F, L, T, K, dev["pose"], dev["undist"], dev["pos_w"], dev["obs_offsets"], dev["obs_kf"],
                                     dev["obs_idx"], dkl, points["inv_level_sigma_sq"], LL, TL, KL, dev["keylines"], dev["pluecker"], dev["obs_offsets_lines"],
                                     dev["obs_kf_lines"], dev["obs_idx_lines"], lines["inv_level_sigma_sq_lsd"], o, x_right=dev["x_right"], counts=dev["counts"],
                                     kf_is_origin=dev["kf_is_origin"], kl_counts=dev["kl_counts"])

        def points_only(o):
            mt.local_ba_device(points["camera"], points["setup_type"], G, F, L, T, K, dev["pose"], dev["undist"], dev["pos_w"], dev["obs_offsets"], dev["obs_kf"],
                               dev["obs_idx"], dkl, points["inv_level_sigma_sq"], o, x_right=dev["x_right"], counts=dev["counts"], kf_is_origin=dev["kf_is_origin"])
        o, tm = timed(with_lines, want)
        assert all(np.array_equal(o[k].cpu().numpy(), want[k], equal_nan=True) for k in want) and (want["status"] == plp.LOCAL_BA_OK).all(), "the device and the CPU build differ"
        op, tp = timed(points_only, want_p)
        assert all(np.array_equal(op[k].cpu().numpy(), want_p[k], equal_nan=True) for k in want_p), "the device and the CPU build differ (points)"
        mean, mean_p = sum(tm) / len(tm), sum(tp) / len(tp)
        role, info = want["kf_role"][0], want["round_info"][0]
        print(f"| {G} | {(role == 1).sum()} / {(role == 3).sum()} | {info[0, 0]} + {info[1, 0]} | {info[0, 1]} + {info[1, 1]} | {info[0, 2]} | {', '.join(f'{x:.1f}' for x in tm)} | "
              f"{mean:.1f} | {cpu_ms:.0f} | {cpu_ms / mean:.2f} | {mean_p:.1f} | {cpu_p_ms:.0f} |", flush=True)


if __name__ == "__main__":
    run([int(v) for v in sys.argv[1:]] or [1, 8])
