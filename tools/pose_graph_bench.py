"""Workload for profiles/r26_pose_graph.md: plp_pose_graph_optimize_device for ring-plus-band graphs of F = 100, 400 and 1000 key frames (the chain of
parents, two band edges per key frame, the loop connection of the last key frame onto the first, which is fixed), G = 1 and G = 8 problems over one
table; every call four times on one stream, the first a warm-up, timed with device events on the launch stream.  It also times the CPU build of the
same header (plp_model_pose_graph_optimize_host, one thread) on the same inputs once, checks that both gave the same values of every output, and
prints the call times, the iteration counts and the sizes of the systems.

  python tools/pose_graph_bench.py [F ...]
  PLP_FRONT_LIB=build_exp/<name>.so python tools/pose_graph_bench.py      # another build of the library (tools/build_variant.sh)
"""
import importlib
import os
import sys
import time

import numpy as np

CALLS = 4


def run(sizes):
    import torch
    root = os.path.dirname(os.path.abspath(__file__))
    sys.path[:0] = [os.path.join(root, ".."), os.path.join(root, "..", "tests")]
    plp = importlib.import_module("structure-plp-slam_amd")
    import pose_graph_scene as S
    mt = plp.matcher()
    print(f"library {plp.LIB_PATH.name}")
    print("| F | G | edges | vertices | envelope blocks | iterations | rejected | device call (ms), calls 2-4 | mean | CPU build, one thread (ms) | CPU / device |")
    print("|---|---|---|---|---|---|---|---|---|---|---|")
    d = lambda v: torch.from_numpy(np.ascontiguousarray(v).copy()).cuda()
    for F in sizes:
        extra = 2 * F - 5
        t, prs, _ = S.ring(F, extra=extra, turn=1.0 - 1.0 / F)
        E, env = S.edge_count(F, extra) + 8, 5 * F
        for G in (1, 8):
            problems = [dict(prs[0], fix_scale=bool(g & 1)) for g in range(G)]
            t0 = time.perf_counter()
            want = plp.model_pose_graph_optimize(t, problems, edge_cap=E, env_cap=env)
            cpu_ms = (time.perf_counter() - t0) * 1e3
            tables = {k: d(t[k] if np.asarray(t[k]).size else np.zeros(1, np.int32)) for k in plp.POSE_GRAPH_TABLES}
            pr = {k: d(v) if v.size else d(np.zeros(8, v.dtype)) for k, v in plp.pose_graph_problems(problems).items()}
            times = []
            for _ in range(CALLS):
                o = {k: d(np.zeros_like(v)) for k, v in want.items()}
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                mt.pose_graph_optimize_device(G, F, tables, pr, o, t["kf_conn"].shape[1], t["kf_covis"].shape[1], E, env)
                e1.record()
                torch.cuda.synchronize()
                times.append(e0.elapsed_time(e1))
            same = all(np.array_equal(o[k].cpu().numpy(), want[k], equal_nan=True) for k in want if k != "edges") and \
                np.array_equal(o["edges"].cpu().numpy()[:, :want["num_edges"][0]], want["edges"][:, :want["num_edges"][0]])
            assert same and (want["status"] == plp.POSE_GRAPH_OK).all(), "the device and the CPU build differ"
            tm = times[1:]
            mean = sum(tm) / len(tm)
            print(f"| {F} | {G} | {int(want['num_edges'][0])} | {int(want['info'][0, 3])} | <= {env} | {want['info'][:, 0].tolist()} | {want['info'][:, 1].tolist()} | "
                  f"{', '.join(f'{x:.1f}' for x in tm)} | {mean:.1f} | {cpu_ms:.0f} | {cpu_ms / mean:.2f} |", flush=True)


if __name__ == "__main__":
    run([int(v) for v in sys.argv[1:]] or [100, 400, 1000])
