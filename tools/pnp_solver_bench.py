"""Workload and summary for profiles/r14_pnp_solver.md: plp_pnp_ransac_device for C = 1, 8 and 32 relocalisation candidates of n = 50, 200 and
1 000 matches (30 % outliers, holes in a tenth of the slots), 30 iterations drawn from a seed, refit on; every call six times on one stream, the
first a warm-up.  `run` also times the CPU build of the same header (plp_model_pnp_ransac_host, one thread) on the same inputs, checks that both
gave the same bits of every output, and prints the call times taken with device events on the launch stream.

  rocprofv3 --kernel-trace --stats -d OUT -o kt -- python tools/pnp_solver_bench.py run
  python tools/pnp_solver_bench.py summary OUT/kt_results.db          (markdown: per kernel and configuration the calls 2-6 and their mean)
"""
import importlib
import os
import sqlite3
import sys
import time

import numpy as np

CONFIGS = [(C, n) for n in (50, 200, 1000) for C in (1, 8, 32)]
CALLS, ITERS = 6, 30
KERNELS = ("k_pnp_prepare", "k_pnp_hypotheses", "k_pnp_count", "k_pnp_refit", "k_pnp_finish")


def run():
    import torch
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
    sys.path[:0] = [root, os.path.join(root, "tests")]
    plp = importlib.import_module("structure-plp-slam_amd")
    import pnp_solver_scene as S
    mt = plp.matcher()
    tt = {np.uint8: torch.uint8, np.int32: torch.int32, np.float64: torch.float64}
    print("| C | n | device call (us), calls 2-6 | mean | CPU build, one thread (us) | CPU / device | OK |")
    print("|---|---|---|---|---|---|---|")
    for C, n in CONFIGS:
        base = [S.problem(7000 + n + i, n, S.MODELS[i % 3], n + n // 10, 0.3, iters=ITERS) for i in range(min(C, 8))]
        a = S.pack([base[i % len(base)] for i in range(C)])
        n_cap = a["valid"].shape[1]
        d = {k: torch.from_numpy(a[k]).cuda() for k in ("valid", "bearing", "pos_w", "octave", "counts")}
        out = {k: torch.zeros((C,) + shape(n_cap, ITERS), dtype=tt[dt], device="cuda") for k, (shape, dt, _) in plp.PNP_OUTPUTS.items()}
        times = []
        for _ in range(CALLS):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            mt.pnp_ransac_device(C, n_cap, d["valid"], d["bearing"], d["pos_w"], d["octave"], S.SCALE_FACTORS, out, iters=ITERS, seed=7, counts=d["counts"])
            e1.record()
            torch.cuda.synchronize()
            times.append(e0.elapsed_time(e1) * 1e3)
        t0 = time.perf_counter()
        want = plp.model_pnp_ransac(a["valid"], a["bearing"], a["pos_w"], a["octave"], S.SCALE_FACTORS, iters=ITERS, seed=7, counts=a["counts"])
        cpu_us = (time.perf_counter() - t0) * 1e6
        for k, w in want.items():
            assert out[k].cpu().numpy().tobytes() == w.tobytes(), (C, n, k)
        t = times[1:]
        mean = sum(t) / len(t)
        ok = int((want["status"] == plp.PNP_OK).sum())
        print(f"| {C} | {n} | {', '.join(f'{x:.0f}' for x in t)} | {mean:.0f} | {cpu_us:.0f} | {cpu_us / mean:.1f} | {ok} of {C} |", flush=True)
    print("device and CPU build gave the same bits of every output")


def summary(path):
    db = sqlite3.connect(path)
    cols = [r[1] for r in db.execute("pragma table_info(kernels)")]
    name_c = "name" if "name" in cols else "kernel_name"
    s_c = "start" if "start" in cols else "start_timestamp"
    e_c = "end" if "end" in cols else "end_timestamp"
    rows = [(nm, (e - s) / 1e3) for nm, s, e in db.execute(f"select {name_c}, {s_c}, {e_c} from kernels order by {s_c}") if "k_pnp_" in nm]
    print("| kernel | C | n | per call (us), calls 2-6 | mean |")
    print("|---|---|---|---|---|")
    for kern in KERNELS:
        us = [t for nm, t in rows if kern in nm]
        assert len(us) == CALLS * len(CONFIGS), (kern, len(us))
        for i, (C, n) in enumerate(CONFIGS):
            t = us[i * CALLS + 1:(i + 1) * CALLS]
            print(f"| `{kern}` | {C} | {n} | {', '.join(f'{x:.1f}' for x in t)} | {sum(t) / len(t):.1f} |")


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "summary":
        summary(sys.argv[2])
    else:
        run()
