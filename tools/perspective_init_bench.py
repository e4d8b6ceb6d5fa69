"""Workload for the profile note of DESIGN.md D27: plp_perspective_ransac_device followed by plp_perspective_pose_device for P = 1, 8 and 32 frame pairs of
n = 100, 500 and 2 000 matches (bearing noise 1e-3, 30 % mismatches, holes in a tenth of the slots), 100 iterations per solver drawn from a seed, refit
on -- initialize::perspective's call --, every chain six times on one stream, the first a warm-up.  It also times the CPU build of the same header on the
same inputs (one thread), checks that both gave the same bits of every output, and prints the call times taken with device events on the launch
stream.  tools/essential_bench.py at the same P, n and iteration count is the bearing-vector path to set beside it.

  python tools/perspective_init_bench.py
"""
import importlib
import os
import sys
import time

import numpy as np

CONFIGS = [(P, n, 100) for n in (100, 500, 2000) for P in (1, 8, 32)]
CALLS = 6


def run():
    import torch
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
    sys.path[:0] = [root, os.path.join(root, "tests")]
    plp = importlib.import_module("structure-plp-slam_amd")
    import perspective_init_scene as S
    import two_view_scene as TS
    mt = plp.matcher()
    cam = plp.camera_model(TS.CAMERAS["perspective"])
    tt = {np.uint8: torch.uint8, np.int32: torch.int32, np.float64: torch.float64, np.float32: torch.float32}
    dev = lambda v: torch.from_numpy(np.ascontiguousarray(v).view(np.uint8).copy() if v.dtype == plp.KP_DTYPE else np.ascontiguousarray(v).copy()).cuda()
    print("| P | n | iters | RANSAC + pose on the device (us), calls 2-6 | mean | RANSAC alone, mean | CPU build, one thread (us) | CPU / device | H / F / none |")
    print("|---|---|---|---|---|---|---|---|---|")
    for P, n, iters in CONFIGS:
        base = [S.problem(7000 + n + i, n, "perspective", n + n // 10, noise=1e-3, mismatch=0.3, iters=1, kind=("cloud", "planar")[i % 2]) for i in range(min(P, 8))]
        qs = [base[i % len(base)] for i in range(P)]
        a = S.pack(qs)
        n_cap, m_cap = a["match"].shape[1], a["undist_2"].shape[1]
        b1, b2 = np.full((P, n_cap, 3), 0.5), np.full((P, m_cap, 3), 0.5)
        for p, q in enumerate(qs):
            b1[p, :len(q["bearing_1"])], b2[p, :len(q["bearing_2"])] = q["bearing_1"], q["bearing_2"]
        d = {k: dev(a[k]) for k in ("undist_1", "undist_2", "match", "counts_1", "counts_2")}
        d["bearing_1"], d["bearing_2"] = dev(b1), dev(b2)
        out = {k: torch.zeros((P,) + shape(n_cap, iters), dtype=tt[dt], device="cuda") for k, (shape, dt, _) in plp.PERSPECTIVE_RANSAC_OUTPUTS.items()}
        pout = {k: torch.zeros((P,) + shape(n_cap), dtype=tt[dt], device="cuda") for k, (shape, dt, _) in plp.PERSPECTIVE_POSE_OUTPUTS.items()}
        times, ransac_times = [], []
        for _ in range(CALLS):
            e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
            e0.record()
            mt.perspective_ransac_device(P, n_cap, m_cap, d["undist_1"], d["undist_2"], d["match"], out, iters=iters, recompute=True, seed=7, counts_1=d["counts_1"],
                                         counts_2=d["counts_2"])
            e1.record()
            mt.perspective_pose_device(cam, P, n_cap, m_cap, out["choice"], out["H_21"], out["F_21"], out["inliers"], d["match"], d["bearing_1"], d["bearing_2"],
                                       d["undist_1"], d["undist_2"], pout, counts_1=d["counts_1"], counts_2=d["counts_2"], img_bounds=qs[0]["bounds"])
            e2.record()
            torch.cuda.synchronize()
            times.append(e0.elapsed_time(e2) * 1e3)
            ransac_times.append(e0.elapsed_time(e1) * 1e3)
        t0 = time.perf_counter()
        want = plp.model_perspective_ransac(a["undist_1"], a["undist_2"], a["match"], iters=iters, recompute=True, seed=7, counts_1=a["counts_1"], counts_2=a["counts_2"])
        pwant = plp.model_perspective_pose(cam, want["choice"], want["H_21"], want["F_21"], want["inliers"], a["match"], b1, b2, a["undist_1"], a["undist_2"],
                                           counts_1=a["counts_1"], counts_2=a["counts_2"], img_bounds=qs[0]["bounds"])
        cpu_us = (time.perf_counter() - t0) * 1e6
        for o, w in ((out, want), (pout, pwant)):
            for k, v in w.items():
                assert o[k].cpu().numpy().tobytes() == v.tobytes(), (P, n, iters, k)
        t = times[1:]
        mean, rmean = sum(t) / len(t), sum(ransac_times[1:]) / len(t)
        ch = np.bincount(want["choice"], minlength=3)
        print(f"| {P} | {n} | {iters} | {', '.join(f'{x:.0f}' for x in t)} | {mean:.0f} | {rmean:.0f} | {cpu_us:.0f} | {cpu_us / mean:.1f} | {ch[1]} / {ch[2]} / {ch[0]} |", flush=True)
    print("device and CPU build gave the same bits of every output")


if __name__ == "__main__":
    run()
