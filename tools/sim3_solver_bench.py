"""Workload and summary for profiles/r13_sim3_solver.md: plp_sim3_ransac_device for P = 1 and P = 64 problems of n = 300 and n = 2 000 common
points (30 % outliers, holes in a tenth of the slots), 200 iterations drawn from a seed, perspective camera; every call six times on one stream,
the first a warm-up.  `run` also times the CPU build of the same header (plp_model_sim3_ransac_host, one thread) on the same inputs, checks that
both gave the same bits of every output, and prints the call times taken with device events.

  rocprofv3 --kernel-trace --stats -d OUT -o kt -- python tools/sim3_solver_bench.py run
  python tools/sim3_solver_bench.py summary OUT/kt_results.db          (markdown: per kernel and configuration the calls 2-6 and their mean)
"""
import importlib
import os
import sqlite3
import sys
import time

import numpy as np

CONFIGS = [(1, 300), (64, 300), (1, 2000), (64, 2000)]
CALLS, ITERS = 6, 200
KERNELS = ("k_sim3_hypotheses", "k_sim3_count", "k_sim3_finish")


def run():
    import torch
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
    sys.path[:0] = [root, os.path.join(root, "tests")]
    plp = importlib.import_module("structure-plp-slam_amd")
    import sim3_solver_scene as S
    cam = plp.camera_model(S.CAMERAS["perspective"])
    mt = plp.matcher()
    tt = {np.uint8: torch.uint8, np.int32: torch.int32, np.float32: torch.float32, np.float64: torch.float64}
    print("| P | n | device call (us), calls 2-6 | mean | CPU build, one thread (us) | CPU / device |")
    print("|---|---|---|---|---|---|")
    for P, n in CONFIGS:
        base = [S.problem(5000 + n + i, n, n + n // 10, 0.3, iters=ITERS) for i in range(min(P, 8))]
        a = S.pack([base[i % len(base)] for i in range(P)])
        n_cap = a["valid"].shape[1]
        d = {k: torch.from_numpy(a[k]).cuda() for k in ("valid", "pos_w_1", "pos_w_2", "octave_1", "octave_2", "pose_1", "pose_2", "counts")}
        out = {k: torch.zeros((P,) + shape(n_cap, ITERS), dtype=tt[dt], device="cuda") for k, (shape, dt, _) in plp.SIM3_OUTPUTS.items()}
        times = []
        for _ in range(CALLS):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            mt.sim3_ransac_device(cam, P, n_cap, d["valid"], d["pos_w_1"], d["pos_w_2"], d["octave_1"], d["octave_2"], d["pose_1"], d["pose_2"], S.SIGMA_SQ,
                                  S.SIGMA_SQ, out, iters=ITERS, seed=7, counts=d["counts"])
            e1.record()
            torch.cuda.synchronize()
            times.append(e0.elapsed_time(e1) * 1e3)
        t0 = time.perf_counter()
        want = plp.model_sim3_ransac(cam, a["valid"], a["pos_w_1"], a["pos_w_2"], a["octave_1"], a["octave_2"], a["pose_1"], a["pose_2"], S.SIGMA_SQ,
                                     S.SIGMA_SQ, iters=ITERS, seed=7, counts=a["counts"])
        cpu_us = (time.perf_counter() - t0) * 1e6
        for k, w in want.items():
            assert out[k].cpu().numpy().tobytes() == w.tobytes(), (P, n, k)
        t = times[1:]
        mean = sum(t) / len(t)
        print(f"| {P} | {n} | {', '.join(f'{x:.0f}' for x in t)} | {mean:.0f} | {cpu_us:.0f} | {cpu_us / mean:.1f} |", flush=True)
    print("device and CPU build gave the same bits of every output")


def summary(path):
    db = sqlite3.connect(path)
    cols = [r[1] for r in db.execute("pragma table_info(kernels)")]
    name_c = "name" if "name" in cols else "kernel_name"
    s_c = "start" if "start" in cols else "start_timestamp"
    e_c = "end" if "end" in cols else "end_timestamp"
    rows = [(nm, (e - s) / 1e3) for nm, s, e in db.execute(f"select {name_c}, {s_c}, {e_c} from kernels order by {s_c}") if "k_sim3_" in nm]
    print("| kernel | P | n | per call (us), calls 2-6 | mean |")
    print("|---|---|---|---|---|")
    for kern in KERNELS:
        us = [t for nm, t in rows if kern in nm]
        assert len(us) == CALLS * len(CONFIGS), (kern, len(us))
        for i, (P, n) in enumerate(CONFIGS):
            t = us[i * CALLS + 1:(i + 1) * CALLS]
            print(f"| `{kern}` | {P} | {n} | {', '.join(f'{x:.1f}' for x in t)} | {sum(t) / len(t):.1f} |")


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "summary":
        summary(sys.argv[2])
    else:
        run()
