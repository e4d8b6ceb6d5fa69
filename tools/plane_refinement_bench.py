"""Workload for profiles/r31_plane_refinement.md: plp_plane_refinement_device, refinement() at 50 iterations over G maps of NP planes of n members
(parallel planes two units apart, noise a quarter of the distance threshold), in three states of the map: `settled` (every row refined: the pair
loop and refine_points only), `one_merge` (row 1 is a second list of row 0's plane: one merge, two updates), `all_new` (every row needs
refinement, as create_new_plane leaves it: NP updates).  Every call six times on one stream from fresh copies of the tables, the first a warm-up;
call times by device events, their mean over calls 2-6.  The CPU build of the same header (plp_model_plane_refinement_host, one thread) runs on
the same inputs, and every table and output must have the same bits before a time is printed.

  python tools/plane_refinement_bench.py            (all configurations)
  python tools/plane_refinement_bench.py quick      (G = 1, 8 and 64 planes)
"""
import importlib
import os
import sys
import time

import numpy as np

# (G, planes, members); G = 64 with 64 planes of 2 000 members and with 512 planes is left out (minutes of the one-thread CPU build)
CONFIGS = [(1, 8, 200), (1, 8, 2000), (1, 64, 200), (1, 64, 2000), (1, 512, 200), (1, 512, 2000), (64, 8, 200), (64, 8, 2000), (64, 64, 200)]
STATES = ("settled", "one_merge", "all_new")
CALLS, ITERS, PPR, DIST, ERR = 6, 50, 18, 0.02, 0.002


def tables(G, NP, n, state, seed):
    rng = np.random.default_rng(seed)
    L, M = NP * n, 2 * n
    t = dict(pl_state=np.full((G, NP), 7 if state == "all_new" else 3, np.uint8), pl_equation=np.zeros((G, NP, 4)), pl_best_error=np.ones((G, NP)),
             pl_count=np.full((G, NP), n, np.int32), pl_lm=np.full((G, NP, M), -1, np.int32), pos_w=rng.uniform(-2.0, 2.0, (G, L, 3)),
             lm_erased=np.zeros((G, L), np.uint8), lm_owner=np.repeat(np.arange(NP, dtype=np.int32), n)[None].repeat(G, 0))
    height = 2.0 * np.arange(NP)
    if state == "one_merge":
        height[1] = height[0]
        t["pl_count"][:, 1] = n // 2
    t["pl_equation"][:, :, 2] = 1.0
    t["pl_equation"][:, :, 3] = -height
    t["pos_w"][:, :, 2] = np.repeat(height, n)[None] + rng.uniform(-DIST / 4, DIST / 4, (G, L))
    t["pl_lm"][:, :, :n] = np.arange(L, dtype=np.int32).reshape(NP, n)[None]
    return t


def run(configs):
    import torch
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
    sys.path[:0] = [root]
    plp = importlib.import_module("structure-plp-slam_amd")
    mt = plp.matcher()
    kw = dict(points_per_ransac=PPR, iters=ITERS, dot_product_threshold=0.8, offset_delta_factor=6, seed=7, merge_cap=4)
    print("| G | planes | members | map | device call (us), calls 2-6 | mean | CPU build, one thread (us) | CPU / device | merges | updates |")
    print("|---|---|---|---|---|---|---|---|---|---|")
    for G, NP, n in configs:
        for state in STATES:
            t = tables(G, NP, n, state, 100 * NP + n)
            d0 = {k: torch.from_numpy(v).cuda() for k, v in t.items()}
            thr = torch.full((G,), DIST, dtype=torch.float64, device="cuda"), torch.full((G,), ERR, dtype=torch.float64, device="cuda")
            times = []
            for _ in range(CALLS):
                d = {k: v.clone() for k, v in d0.items()}
                out = {k: torch.zeros((G,) + shape(NP, NP * n, 4), dtype=getattr(torch, dt.__name__), device="cuda") for k, (shape, dt) in plp.PLANE_REFINEMENT_OUTPUTS.items()}
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                mt.plane_refinement_device(G, NP, 2 * n, NP * n, d, thr[0], thr[1], out, **kw)
                e1.record()
                torch.cuda.synchronize()
                times.append(e0.elapsed_time(e1) * 1e3)
            t0 = time.perf_counter()
            want = plp.model_plane_refinement(t, DIST, ERR, **kw)
            cpu_us = (time.perf_counter() - t0) * 1e6
            for k, w in want.items():
                assert out[k].cpu().numpy().tobytes() == w.tobytes(), (G, NP, n, state, k)
            for k, w in t.items():
                assert d[k].cpu().numpy().tobytes() == w.tobytes(), (G, NP, n, state, k)
            ts = times[1:]
            mean = sum(ts) / len(ts)
            print(f"| {G} | {NP} | {n} | {state} | {', '.join(f'{x:.0f}' for x in ts)} | {mean:.0f} | {cpu_us:.0f} | {cpu_us / mean:.2f} | "
                  f"{int(want['num_merges'].sum())} | {int(want['num_updates'].sum())} |", flush=True)
    print("device and CPU build gave the same bits of every table and output")


if __name__ == "__main__":
    run([c for c in CONFIGS if c[0] == 1 and c[1] <= 64] if len(sys.argv) > 1 and sys.argv[1] == "quick" else CONFIGS)
