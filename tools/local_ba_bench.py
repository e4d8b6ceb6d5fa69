"""Workload for profiles/r17_local_ba.md: plp_local_ba_device on a mapping-sized problem -- 20 free and 40 fixed key frames, 2 000 landmarks, about
12 000 edges (RGB-D, pixel noise 0.8, 200 displaced observations, start poses off by 0.003 rad and 0.01, positions by 0.01; tests/local_ba_scene.py), 5 + 10 iterations -- for G = 1 and G = 8 problems over
the same tables (the G problems differ in which of the 20 key frames are local); every call four times on one stream, the first a warm-up.  It also
times the CPU build of the same header (plp_model_local_ba_host, one thread) on the same inputs, checks that both gave the same values of every
output, and prints the call times taken with device events on the launch stream.

  python tools/local_ba_bench.py
"""
import importlib
import os
import sys
import time

import numpy as np

CALLS = 4
TABLES = ("pose", "kf_erased", "kf_is_origin", "undist", "x_right", "counts", "pos_w", "lm_erased", "obs_offsets", "obs_kf", "obs_idx")


def run():
    import torch
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
    sys.path[:0] = [root, os.path.join(root, "tests")]
    plp = importlib.import_module("structure-plp-slam_amd")
    import local_ba_scene as S
    mt = plp.matcher()
    tt = {np.uint8: torch.uint8, np.int32: torch.int32, np.float64: torch.float64}

    def d(v):
        v = np.ascontiguousarray(v)
        return torch.from_numpy((v.view(np.uint8) if v.dtype.fields else v).copy()).cuda()
    sc = S.make_scene(1700, 20, 40, 2000, setup=S.RGBD, noise=0.8, outliers=200, n_other=0, obs_share=0.1, min_obs=2, pose_noise=0.003, lm_noise=0.01)
    F, L, T = len(sc["pose"]), len(sc["pos_w"]), len(sc["obs_kf"])
    dev = {k: d(sc[k]) for k in TABLES}
    print(f"F = {F}, L = {L}, T = {T}")
    print("| G | free / fixed key frames, landmarks, edges (problem 0) | device call (ms), calls 2-4 | mean | CPU build, one thread (ms) | CPU / device |")
    print("|---|---|---|---|---|---|")
    for G in (1, 8):
        kl = np.zeros((G, F), np.uint8)
        for g in range(G):
            kl[g, :20 - g] = 1                      # problem g frees 20 - g key frames
        out = {k: torch.zeros((G,) + shape(F, L, T), dtype=tt[dt], device="cuda") for k, (shape, dt, _) in plp.LOCAL_BA_OUTPUTS.items()}
        dkl = d(kl)
        times = []
        for _ in range(CALLS):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            mt.local_ba_device(sc["camera"], sc["setup_type"], G, F, L, T, sc["undist"].shape[1], dev["pose"], dev["undist"], dev["pos_w"], dev["obs_offsets"],
                               dev["obs_kf"], dev["obs_idx"], dkl, S.INV_SIGMA_SQ, out, x_right=dev["x_right"], counts=dev["counts"], kf_erased=dev["kf_erased"],
                               kf_is_origin=dev["kf_is_origin"], lm_erased=dev["lm_erased"])
            e1.record()
            torch.cuda.synchronize()
            times.append(e0.elapsed_time(e1))
        t0 = time.perf_counter()
        want = plp.model_local_ba(**S.call_args(sc, kf_local=kl))
        cpu_ms = (time.perf_counter() - t0) * 1e3
        for k, w in want.items():
            assert S.same({k: out[k].cpu().numpy()}, {k: w}), (G, k)
        t = times[1:]
        mean = sum(t) / len(t)
        role = want["kf_role"][0]
        edges = int((plp.model_local_ba(**S.call_args(sc, kf_local=kl[:1]), out=S.sentinel_out(1, F, L, T))["outlier"][0] != 77).sum())
        print(f"| {G} | {int((role == 1).sum())} / {int((role == 3).sum())}, {int(want['lm_role'][0].sum())}, {edges} | {', '.join(f'{x:.2f}' for x in t)} | {mean:.2f} | {cpu_ms:.1f} | "
              f"{cpu_ms / mean:.2f} |  rounds {want['round_info'][0].tolist()}", flush=True)
    print("device and CPU build gave the same values of every output")


if __name__ == "__main__":
    run()
