"""Workload for profiles/r15_pose_optimizer.md: plp_pose_optimize_device for B = 1, 64 and 2048 frames of n = 300 and 1 000 point observations
with 0 and 150 line observations (RGB-D set-up, pixel noise 1, 15 % gross outliers, holes in a tenth of the slots; eight distinct frames, repeated),
4 trials of 10 iterations; every call six times on one stream, the first a warm-up.  It also times the CPU build of the same header
(plp_model_pose_optimize_host, one thread) on the same inputs -- on the first 64 frames where there are more, scaled to B -- checks that both
gave the same bits of every output, and prints the call times taken with device events on the launch stream.

  python tools/pose_optimizer_bench.py
"""
import importlib
import os
import sys
import time

import numpy as np

CONFIGS = [(B, n, l) for n in (300, 1000) for l in (0, 150) for B in (1, 64, 2048)]
CALLS, CPU_FRAMES = 6, 64


def run():
    import torch
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
    sys.path[:0] = [root, os.path.join(root, "tests")]
    plp = importlib.import_module("structure-plp-slam_amd")
    import pose_optimizer_scene as S
    mt = plp.matcher()
    tt = {np.uint8: torch.uint8, np.int32: torch.int32, np.float64: torch.float64}

    def d(v):
        v = np.ascontiguousarray(v)
        return torch.from_numpy((v.view(np.uint8) if v.dtype.fields else v).copy()).cuda()
    print("| B | n | lines | device call (us), calls 2-6 | mean | CPU build, one thread (us) | CPU / device | OK |")
    print("|---|---|---|---|---|---|---|---|")
    for B, n, l in CONFIGS:
        base = [S.make_frame(9000 + n + i, n, setup=S.RGBD, n_lines=l, noise=1.0, outlier_share=0.15, rot=0.05, trans=0.1) for i in range(min(B, 8))]
        P8 = S.pack(base, holes=0.1, seed=1)
        rep = lambda a: np.ascontiguousarray(np.concatenate([a] * ((B + len(base) - 1) // len(base)))[:B])
        P = dict(P8, pose_in=rep(P8["pose_in"]), valid=rep(P8["valid"]), undist=rep(P8["undist"]), x_right=rep(P8["x_right"]), pos_w=rep(P8["pos_w"]),
                 counts=rep(P8["counts"]))
        if P8["lines"] is not None:
            P["lines"] = {k: (v if k == "inv_level_sigma_sq_lsd" else rep(v)) for k, v in P8["lines"].items()}
        N = P["valid"].shape[1]
        ln = P["lines"]
        L = 0 if ln is None else ln["valid"].shape[1]
        dev = dict(pose=d(P["pose_in"]), valid=d(P["valid"]), undist=d(P["undist"]), pos_w=d(P["pos_w"]), x_right=d(P["x_right"]), counts=d(P["counts"]))
        kw = {}
        if ln is not None:
            dev.update(lv=d(ln["valid"]), kl=d(ln["keylines"]), lw=d(ln["pos_w"]), lc=d(ln["counts"]))
            kw = dict(l_cap=L, line_valid=dev["lv"], keylines=dev["kl"], pos_w_lines=dev["lw"], inv_level_sigma_sq_lsd=ln["inv_level_sigma_sq_lsd"], line_counts=dev["lc"])
        out = {k: torch.zeros((B,) + shape(N, L, 4), dtype=tt[dt], device="cuda") for k, (shape, dt, _) in plp.POSE_OPT_OUTPUTS.items()}
        passed = {k: v for k, v in out.items() if v.numel()}
        times = []
        for _ in range(CALLS):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            mt.pose_optimize_device(P["camera"], S.RGBD, B, N, dev["pose"], dev["valid"], dev["undist"], dev["pos_w"], S.INV_SIGMA_SQ, passed, x_right=dev["x_right"],
                                    counts=dev["counts"], **kw)
            e1.record()
            torch.cuda.synchronize()
            times.append(e0.elapsed_time(e1) * 1e3)
        C = min(B, CPU_FRAMES)
        a = S.call_args(P)
        for k in ("pose_in", "valid", "undist", "pos_w", "x_right", "counts"):
            a[k] = a[k][:C]
        if ln is not None:
            a["lines"] = {k: (v if k == "inv_level_sigma_sq_lsd" else v[:C]) for k, v in ln.items()}
        t0 = time.perf_counter()
        want = plp.model_pose_optimize(**a)
        cpu_us = (time.perf_counter() - t0) * 1e6 * B / C
        for k, w in want.items():
            if w.size:
                assert out[k][:C].cpu().numpy().tobytes() == w.tobytes(), (B, n, l, k)
        t = times[1:]
        mean = sum(t) / len(t)
        ok = int((want["status"] == plp.POSE_OPT_OK).sum())
        print(f"| {B} | {n} | {l} | {', '.join(f'{x:.0f}' for x in t)} | {mean:.0f} | {cpu_us:.0f} | {cpu_us / mean:.1f} | {ok} of {C} |", flush=True)
    print("device and CPU build gave the same bits of every output")


if __name__ == "__main__":
    run()
