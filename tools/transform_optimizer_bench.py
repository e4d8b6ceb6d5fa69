"""Workload for profiles/r16_transform_optimizer.md: plp_transform_optimize_device for P = 1, 8 and 64 problems of n = 150 matches (pixel noise 1,
15 % gross outliers, holes in a tenth of the slots; eight distinct pairs, repeated), 5 + 10 iterations; every call six times on one stream, the
first a warm-up.  It also times the CPU build of the same header (plp_model_transform_optimize_host, one thread) on the same inputs, checks that
both gave the same bits of every output, and prints the call times taken with device events on the launch stream.

  python tools/transform_optimizer_bench.py
"""
import importlib
import os
import sys
import time

import numpy as np

CONFIGS = [(P, 150) for P in (1, 8, 64)]
CALLS = 6
INPUTS = ("valid", "pos_w_1", "pos_w_2", "undist_1", "undist_2", "pose_1", "pose_2", "rot_12", "trans_12", "scale_12", "counts")


def run():
    import torch
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
    sys.path[:0] = [root, os.path.join(root, "tests")]
    plp = importlib.import_module("structure-plp-slam_amd")
    import transform_optimizer_scene as S
    mt = plp.matcher()
    tt = {np.uint8: torch.uint8, np.int32: torch.int32, np.float64: torch.float64}

    def d(v):
        v = np.ascontiguousarray(v)
        return torch.from_numpy((v.view(np.uint8) if v.dtype.fields else v).copy()).cuda()
    print("| P | n | device call (us), calls 2-6 | mean | CPU build, one thread (us) | CPU / device | OK |")
    print("|---|---|---|---|---|---|---|")
    for P, n in CONFIGS:
        base = [S.make_problem(9000 + n + i, n, noise=1.0, outlier_share=0.15, rot=0.05, trans=0.1) for i in range(min(P, 8))]
        A8 = S.pack(base, holes=0.1, seed=1)
        rep = lambda a: np.ascontiguousarray(np.concatenate([a] * ((P + len(base) - 1) // len(base)))[:P])
        A = dict(A8, **{k: rep(A8[k]) for k in INPUTS})
        N = A["valid"].shape[1]
        dev = {k: d(A[k]) for k in INPUTS}
        out = {k: torch.zeros((P,) + shape(N), dtype=tt[dt], device="cuda") for k, (shape, dt, _) in plp.TRANSFORM_OPT_OUTPUTS.items()}
        times = []
        for _ in range(CALLS):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            mt.transform_optimize_device(A["camera"], A["fix_scale"], P, N, dev["valid"], dev["pos_w_1"], dev["pos_w_2"], dev["undist_1"], dev["undist_2"], dev["pose_1"],
                                         dev["pose_2"], dev["rot_12"], dev["trans_12"], dev["scale_12"], S.INV_SIGMA_SQ, S.INV_SIGMA_SQ, out, counts=dev["counts"])
            e1.record()
            torch.cuda.synchronize()
            times.append(e0.elapsed_time(e1) * 1e3)
        t0 = time.perf_counter()
        want = plp.model_transform_optimize(**S.call_args(A))
        cpu_us = (time.perf_counter() - t0) * 1e6
        for k, w in want.items():
            assert out[k].cpu().numpy().tobytes() == w.tobytes(), (P, n, k)
        t = times[1:]
        mean = sum(t) / len(t)
        ok = int((want["status"] == plp.TRANSFORM_OPT_OK).sum())
        print(f"| {P} | {n} | {', '.join(f'{x:.0f}' for x in t)} | {mean:.0f} | {cpu_us:.0f} | {cpu_us / mean:.1f} | {ok} of {P} |", flush=True)
    print("device and CPU build gave the same bits of every output")


if __name__ == "__main__":
    run()
