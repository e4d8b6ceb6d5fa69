"""Workload for profiles/r27_global_ba.md: plp_global_ba_device on corridor maps of P = 100, 400 and 1000 free key frames behind the origin (a camera every
0.3 m along a line, looking ahead and to the side; about 100 landmarks seen per key frame, every landmark seen by the 6 key frames nearest to it, RGB-D,
0.5 px noise, perturbed start), Huber off, 2 iterations; every call six times on one stream, the first a warm-up, timed with device events on the launch
stream (the entry is synchronous, so the events bracket the whole run).  It also times the CPU build of the same header (plp_model_global_ba_host, one
thread) on the same inputs once, checks first that both gave the same bits in every output, and prints the call times and the sizes of the systems.

  python tools/global_ba_bench.py [P ...]
"""
import importlib
import os
import sys
import time

import numpy as np

CALLS, ITERS, PER_KF, PER_LM = 6, 2, 100, 6


def corridor(plp, P, seed=1):
    import pose_optimizer_scene as PS
    rng = np.random.default_rng(seed)
    F = P + 1
    L = F * PER_KF // PER_LM
    m, fx, fy, cx, cy, fxb = PS.CAMERAS["perspective"]
    cen = np.stack([0.3 * np.arange(F), rng.normal(size=F) * 0.05, rng.normal(size=F) * 0.05], 1)
    Rs = np.stack([PS.rodrigues(rng.normal(size=3) * 0.03) for _ in range(F)])
    ts = -np.einsum("fij,fj->fi", Rs, cen)
    first = np.minimum(rng.integers(0, F, L), F - PER_LM)                     # the first of the landmark's six key frames
    mid = cen[first + PER_LM // 2]
    pos = mid + np.stack([rng.uniform(-1.5, 1.5, L), rng.uniform(-1.0, 1.0, L), rng.uniform(4.0, 9.0, L)], 1)
    obs_kf = (first[:, None] + np.arange(PER_LM)[None]).astype(np.int32)     # [L, 6]
    order = np.argsort(obs_kf.reshape(-1), kind="stable")
    slot = np.empty(L * PER_LM, np.int32)
    kf_sorted = obs_kf.reshape(-1)[order]
    starts = np.searchsorted(kf_sorted, np.arange(F))
    slot[order] = np.arange(L * PER_LM) - starts[kf_sorted]
    counts = np.bincount(obs_kf.reshape(-1), minlength=F).astype(np.int32)
    K = int(counts.max()) + 1
    pc = np.einsum("lkij,lj->lki", Rs[obs_kf], pos) + ts[obs_kf]
    u = fx * pc[..., 0] / pc[..., 2] + cx + rng.normal(size=(L, PER_LM)) * 0.5
    v = fy * pc[..., 1] / pc[..., 2] + cy + rng.normal(size=(L, PER_LM)) * 0.5
    undist = np.zeros((F, K), plp.KP_DTYPE)
    undist["octave"] = 99
    x_right = np.full((F, K), -1.0, np.float32)
    kk, ss = obs_kf.reshape(-1), slot
    undist["x"][kk, ss], undist["y"][kk, ss], undist["octave"][kk, ss] = u.reshape(-1), v.reshape(-1), rng.integers(0, 4, L * PER_LM)
    x_right[kk, ss] = (u - fxb / pc[..., 2]).reshape(-1)
    pose = np.zeros((F, 15))
    for f in range(F):
        Rm, t = Rs[f], ts[f]
        if f:
            Rm = PS.rodrigues(rng.normal(size=3) * 0.005) @ Rm
            t = t + rng.normal(size=3) * 0.01
        pose[f, :9], pose[f, 9:12] = Rm.reshape(-1), t
    origin = np.zeros(F, np.uint8); origin[0] = 1
    return dict(camera=PS.camera("perspective"), setup_type=PS.RGBD, pose=pose, undist=undist, x_right=x_right, counts=counts, pos_w=pos + rng.normal(size=pos.shape) * 0.02,
                obs_offsets=(np.arange(L + 1) * PER_LM).astype(np.int32), obs_kf=obs_kf.reshape(-1), obs_idx=slot, kf_is_origin=origin, inv_level_sigma_sq=PS.INV_SIGMA_SQ)


def run(sizes):
    import torch
    root = os.path.dirname(os.path.abspath(__file__))
    sys.path[:0] = [os.path.join(root, ".."), os.path.join(root, "..", "tests")]
    plp = importlib.import_module("structure-plp-slam_amd")
    mt = plp.matcher()
    print(f"library {plp.LIB_PATH.name}, panel {plp.GLOBAL_BA_PANEL}, rows per workgroup {plp.GLOBAL_BA_ROWS}")
    print("| P | rows of S | landmarks | observations | iterations | rejected | factorisations | device call (ms), calls 2-6 | mean | CPU build, one thread (ms) | CPU / device |")
    print("|---|---|---|---|---|---|---|---|---|---|---|")
    d = lambda v: torch.from_numpy((v.view(np.uint8) if v.dtype.fields else v).copy()).cuda()
    for P in sizes:
        sc = corridor(plp, P)
        F, L, T = len(sc["pose"]), len(sc["pos_w"]), len(sc["obs_kf"])
        t0 = time.perf_counter()
        want = plp.model_global_ba(**sc, num_iter=ITERS, use_huber_kernel=False)
        cpu_ms = (time.perf_counter() - t0) * 1e3
        dev = {k: d(np.ascontiguousarray(sc[k])) for k in ("pose", "undist", "x_right", "counts", "pos_w", "obs_offsets", "obs_kf", "obs_idx", "kf_is_origin")}
        times = []
        for _ in range(CALLS):
            o = {k: d(np.zeros_like(v)) for k, v in want.items()}
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            mt.global_ba_device(sc["camera"], sc["setup_type"], F, L, T, sc["undist"].shape[1], dev["pose"], dev["undist"], dev["pos_w"], dev["obs_offsets"], dev["obs_kf"],
                                dev["obs_idx"], sc["inv_level_sigma_sq"], o, x_right=dev["x_right"], counts=dev["counts"], kf_is_origin=dev["kf_is_origin"], num_iter=ITERS,
                                use_huber_kernel=False)
            e1.record()
            torch.cuda.synchronize()
            times.append(e0.elapsed_time(e1))
            if len(times) == 1:                              # equal bits first
                assert all(np.array_equal(o[k].cpu().numpy(), want[k], equal_nan=True) for k in want) and want["status"][0] == plp.GLOBAL_BA_OK, "the device and the CPU build differ"
        tm = times[1:]
        mean = sum(tm) / len(tm)
        print(f"| {P} | {6 * P} | {L} | {T} | {int(want['info'][0])} | {int(want['info'][1])} | {int(want['info'][2])} | {', '.join(f'{x:.1f}' for x in tm)} | {mean:.1f} | "
              f"{cpu_ms:.0f} | {cpu_ms / mean:.1f} |", flush=True)


if __name__ == "__main__":
    run([int(v) for v in sys.argv[1:]] or [100, 400, 1000])
