"""Phase clocks of k_quadtree from a DIAGNOSTIC build of the library (csrc/quadtree_kernel.hip, -DPLP_QT_PROF), on the benchmark's frames:

    bash tools/build_variant.sh qtprof "-DPLP_QT_PROF"                              # the tree's kernel
    bash tools/build_variant.sh qtprof_large "-DPLP_QT_PROF -DPLP_QT_PROF_SMALL_N=0"  # every level down the radix path
    PLP_FRONT_LIB=build_exp/qtprof.so python tools/quadtree_phases.py [--batch 2048] [--launches 4]

Prints one markdown row per level: shader-clock ticks per workgroup and phase (thread 0's clock; the stamps themselves cost some per cent), the mean candidate
count, the phase-1 and phase-2 passes per workgroup, the largest population of a final node and the share of workgroups on the small path.  The shipped library has
no such entry point: this tool refuses it."""
import argparse
import ctypes as C
import pathlib
import sys

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import importlib  # noqa: E402

PHASES = ("gather", "sort", "key copy", "initial nodes", "phase 1", "phase 2", "selection")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=2048)
    ap.add_argument("--launches", type=int, default=4)
    ap.add_argument("--keypoints", type=int, default=1000)
    args = ap.parse_args()
    import torch
    plp = importlib.import_module("structure-plp-slam_amd")
    synth = importlib.import_module("structure-plp-slam_amd.synth")
    L = plp.lib()
    if not hasattr(L, "plp_debug_quadtree_phases"):
        sys.exit("this library was not built with -DPLP_QT_PROF (set PLP_FRONT_LIB to a diagnostic build)")
    L.plp_debug_quadtree_phases.restype = C.c_int
    L.plp_debug_quadtree_phases.argtypes = [C.c_void_p, C.c_int]
    dev = torch.device("cuda:0")
    B, cap = args.batch, 2 * args.keypoints + 64
    frames = torch.from_numpy(synth.replay(1234, 64, 480, 640)).to(dev)
    frames = frames.repeat((B + 63) // 64, 1, 1)[:B].contiguous()
    ex = plp.orb_extractor(args.keypoints)
    d_kps = torch.zeros((B, cap, 28), dtype=torch.uint8, device=dev)
    d_desc = torch.zeros((B, cap, 32), dtype=torch.uint8, device=dev)
    d_cnt = torch.zeros(B, dtype=torch.int32, device=dev)
    ex.extract_batch(frames, d_kps, d_desc, d_cnt)      # warm-up
    torch.cuda.synchronize()
    assert L.plp_debug_quadtree_phases(None, 1) == 0
    for _ in range(args.launches):
        ex.extract_batch(frames, d_kps, d_desc, d_cnt)
    torch.cuda.synchronize()
    ex.last_batch_status()
    acc = np.zeros((16, 16), np.uint64)
    assert L.plp_debug_quadtree_phases(acc.ctypes.data_as(C.c_void_p), 0) == 0
    print(f"k_quadtree phase clocks: {B} frames x {args.launches} launches, K = {args.keypoints}; ticks per workgroup (thread 0)")
    print("| level | candidates | " + " | ".join(PHASES) + " | all | phase-1 passes | phase-2 passes | largest node | final nodes | small path % |")
    print("|---|---:|" + "---:|" * (len(PHASES) + 6))
    tot = np.zeros(7)
    rows = 0
    for l in range(16):
        wg = int(acc[l, 7])
        if not wg:
            continue
        t = acc[l, :7].astype(np.float64) / wg
        tot += t
        rows += 1
        print(f"| {l} | {acc[l, 8] / wg:.0f} | " + " | ".join(f"{v:.0f}" for v in t) + f" | {t.sum():.0f} | {acc[l, 9] / wg:.2f} | {acc[l, 10] / wg:.2f} | "
              f"{int(acc[l, 11])} | {acc[l, 12] / wg:.0f} | {100.0 * acc[l, 13] / wg:.0f} |")
    if rows:
        print("| mean | | " + " | ".join(f"{v / rows:.0f}" for v in tot) + f" | {tot.sum() / rows:.0f} | | | | | |")


if __name__ == "__main__":
    main()
