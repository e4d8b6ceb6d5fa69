"""Workload and summary for profiles/r28_two_view.md: plp_essential_ransac_device for P = 1, 8 and 32 frame pairs of n = 100, 500 and 2 000
matches (bearing noise 1e-3, 30 % mismatches, holes in a tenth of the slots), 100 iterations drawn from a seed, refit on -- the initialiser's
call -- and the robust match's 50 iterations without the refit; every call six times on one stream, the first a warm-up.  `run` also times the
CPU build of the same header (plp_model_essential_ransac_host, one thread) on the same inputs, checks that both gave the same bits of every
output, and prints the call times taken with device events on the launch stream.

  rocprofv3 --kernel-trace --stats -d OUT -o kt -- python tools/essential_bench.py run
  python tools/essential_bench.py summary OUT/kt_results.db          (markdown: per kernel and configuration the calls 2-6 and their mean)
"""
import importlib
import os
import sqlite3
import sys
import time

import numpy as np

CONFIGS = [(P, n, iters, rec) for iters, rec in ((100, True), (50, False)) for n in (100, 500, 2000) for P in (1, 8, 32)]
CALLS = 6
KERNELS = ("k_ess_prepare", "k_ess_hypotheses", "k_ess_count", "k_ess_refit", "k_ess_finish")


def run():
    import torch
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
    sys.path[:0] = [root, os.path.join(root, "tests")]
    plp = importlib.import_module("structure-plp-slam_amd")
    import two_view_scene as S
    mt = plp.matcher()
    tt = {np.uint8: torch.uint8, np.int32: torch.int32, np.float64: torch.float64, np.float32: torch.float32}
    print("| P | n | iters | refit | device call (us), calls 2-6 | mean | CPU build, one thread (us) | CPU / device | OK |")
    print("|---|---|---|---|---|---|---|---|---|")
    for P, n, iters, rec in CONFIGS:
        base = [S.problem(7000 + n + i, n, S.MODELS[i % 3], n + n // 10, noise=1e-3, mismatch=0.3, iters=1) for i in range(min(P, 8))]
        a = S.pack([base[i % len(base)] for i in range(P)])
        n_cap, m_cap = a["match"].shape[1], a["bearing_2"].shape[1]
        d = {k: torch.from_numpy(a[k]).cuda() for k in ("bearing_1", "bearing_2", "match", "counts_1", "counts_2")}
        out = {k: torch.zeros((P,) + shape(n_cap, iters), dtype=tt[dt], device="cuda") for k, (shape, dt, _) in plp.ESSENTIAL_OUTPUTS.items()}
        times = []
        for _ in range(CALLS):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            mt.essential_ransac_device(P, n_cap, m_cap, d["bearing_1"], d["bearing_2"], d["match"], out, iters=iters, recompute=rec, seed=7,
                                       counts_1=d["counts_1"], counts_2=d["counts_2"])
            e1.record()
            torch.cuda.synchronize()
            times.append(e0.elapsed_time(e1) * 1e3)
        t0 = time.perf_counter()
        want = plp.model_essential_ransac(a["bearing_1"], a["bearing_2"], a["match"], iters=iters, recompute=rec, seed=7, counts_1=a["counts_1"],
                                          counts_2=a["counts_2"])
        cpu_us = (time.perf_counter() - t0) * 1e6
        for k, w in want.items():
            assert out[k].cpu().numpy().tobytes() == w.tobytes(), (P, n, iters, k)
        t = times[1:]
        mean = sum(t) / len(t)
        ok = int((want["status"] == plp.ESSENTIAL_OK).sum())
        print(f"| {P} | {n} | {iters} | {'on' if rec else 'off'} | {', '.join(f'{x:.0f}' for x in t)} | {mean:.0f} | {cpu_us:.0f} | {cpu_us / mean:.1f} | {ok} of {P} |",
              flush=True)
    print("device and CPU build gave the same bits of every output")


def summary(path):
    db = sqlite3.connect(path)
    table = [r[0] for r in db.execute("select name from sqlite_master where type in ('table', 'view') and name like '%kernels%'")]
    table = "kernels" if "kernels" in table else table[0]
    cols = [r[1] for r in db.execute(f"pragma table_info({table})")]
    name_c = "name" if "name" in cols else "kernel_name"
    s_c = "start" if "start" in cols else "start_timestamp"
    e_c = "end" if "end" in cols else "end_timestamp"
    rows = [(nm, (e - s) / 1e3) for nm, s, e in db.execute(f"select {name_c}, {s_c}, {e_c} from {table} order by {s_c}") if "k_ess_" in nm]
    print("| kernel | P | n | iters | refit | per call (us), calls 2-6 | mean |")
    print("|---|---|---|---|---|---|---|")
    for kern in KERNELS:
        us = [t for nm, t in rows if kern in nm]
        assert len(us) == CALLS * len(CONFIGS), (kern, len(us))
        for i, (P, n, iters, rec) in enumerate(CONFIGS):
            t = us[i * CALLS + 1:(i + 1) * CALLS]
            print(f"| `{kern}` | {P} | {n} | {iters} | {'on' if rec else 'off'} | {', '.join(f'{x:.1f}' for x in t)} | {sum(t) / len(t):.1f} |")


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "summary":
        summary(sys.argv[2])
    else:
        run()
