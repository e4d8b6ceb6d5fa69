"""Workload and summary for profiles/r21_plane_ransac.md: plp_plane_ransac_device, PLANE_CREATE at 50 iterations for P = 1 and P = 64 planes of
n = 200 and n = 2 000 landmarks, PLANE_UPDATE at 50 iterations for one plane of n = 2 000 and n = 8 000 (5 % gross outliers, a few erased and
unowned slots, samples drawn from a seed; tests/plane_ransac_scene.py); every call six times on one stream, the first a warm-up.  `run` also
times the CPU build of the same header (plp_model_plane_ransac_host, one thread) on the same inputs, checks that both gave the same bits of
every output, and prints the call times taken with device events.

  python tools/plane_ransac_bench.py run
  rocprofv3 --kernel-trace --stats -d OUT -o kt -- python tools/plane_ransac_bench.py run
  python tools/plane_ransac_bench.py summary OUT/kt_results.db          (markdown: per kernel and configuration the calls 2-6 and their mean)
"""
import importlib
import os
import sqlite3
import sys
import time

import numpy as np

CONFIGS = [("CREATE", 1, 200), ("CREATE", 64, 200), ("CREATE", 1, 2000), ("CREATE", 64, 2000), ("UPDATE", 1, 2000), ("UPDATE", 1, 8000)]
CALLS, ITERS = 6, 50
KERNELS = ("k_plane_hypotheses", "k_plane_finish")


def run():
    import torch
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
    sys.path[:0] = [root, os.path.join(root, "tests")]
    plp = importlib.import_module("structure-plp-slam_amd")
    import plane_ransac_scene as S
    mt = plp.matcher()
    tt = {np.uint8: torch.uint8, np.int32: torch.int32, np.float64: torch.float64}
    print("| mode | P | n | device call (us), calls 2-6 | mean | CPU build, one thread (us) | CPU / device | iterations that ran |")
    print("|---|---|---|---|---|---|---|---|")
    for mode_name, P, n in CONFIGS:
        mode = plp.PLANE_CREATE if mode_name == "CREATE" else plp.PLANE_UPDATE
        # error_thresh = 0: CREATE never breaks, so that all 50 iterations are what is timed on both sides
        base = [S.problem(7000 + n + i, n, mode=mode, outliers=0.05, erased=n // 50, unowned=n // 50 if mode else 0, iters=ITERS, error_thresh=0.0)
                for i in range(min(P, 8))]
        a = S.pack([base[i % len(base)] for i in range(P)])
        n_cap = a["flags"].shape[1]
        d = {k: torch.from_numpy(a[k]).cuda() for k in ("pos_w", "flags", "counts", "dist_thresh", "error_thresh", "best_error_in", "equation_in")}
        out = {k: torch.zeros((P,) + shape(n_cap, ITERS), dtype=tt[dt], device="cuda") for k, (shape, dt, _) in plp.PLANE_RANSAC_OUTPUTS.items()}
        times = []
        for _ in range(CALLS):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            mt.plane_ransac_device(mode, P, n_cap, d["pos_w"], d["flags"], d["dist_thresh"], d["error_thresh"], out, iters=ITERS, seed=7,
                                   best_error_in=d["best_error_in"], equation_in=d["equation_in"], counts=d["counts"])
            e1.record()
            torch.cuda.synchronize()
            times.append(e0.elapsed_time(e1) * 1e3)
        t0 = time.perf_counter()
        want = plp.model_plane_ransac(mode, a["pos_w"], a["flags"], a["dist_thresh"], a["error_thresh"], iters=ITERS, seed=7,
                                      best_error_in=a["best_error_in"], equation_in=a["equation_in"], counts=a["counts"])
        cpu_us = (time.perf_counter() - t0) * 1e6
        for k, w in want.items():
            assert out[k].cpu().numpy().tobytes() == w.tobytes(), (mode_name, P, n, k)
        t = times[1:]
        mean = sum(t) / len(t)
        print(f"| {mode_name} | {P} | {n} | {', '.join(f'{x:.0f}' for x in t)} | {mean:.0f} | {cpu_us:.0f} | {cpu_us / mean:.1f} | "
              f"{int(want['last_iter'].min()) + 1} |", flush=True)
    print("device and CPU build gave the same bits of every output")


def summary(path):
    db = sqlite3.connect(path)
    cols = [r[1] for r in db.execute("pragma table_info(kernels)")]
    name_c = "name" if "name" in cols else "kernel_name"
    s_c = "start" if "start" in cols else "start_timestamp"
    e_c = "end" if "end" in cols else "end_timestamp"
    rows = [(nm, (e - s) / 1e3) for nm, s, e in db.execute(f"select {name_c}, {s_c}, {e_c} from kernels order by {s_c}") if "k_plane_" in nm]
    print("| kernel | mode | P | n | per call (us), calls 2-6 | mean |")
    print("|---|---|---|---|---|---|")
    for kern in KERNELS:
        us = [t for nm, t in rows if kern in nm]
        assert len(us) == CALLS * len(CONFIGS), (kern, len(us))
        for i, (mode_name, P, n) in enumerate(CONFIGS):
            t = us[i * CALLS + 1:(i + 1) * CALLS]
            print(f"| `{kern}` | {mode_name} | {P} | {n} | {', '.join(f'{x:.1f}' for x in t)} | {sum(t) / len(t):.1f} |")


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "summary":
        summary(sys.argv[2])
    else:
        run()
