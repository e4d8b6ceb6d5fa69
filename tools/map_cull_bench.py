"""Workload for profiles/r22_map_cull.md: plp_cull_keyframes_device for G = 1, 64 and 2048 problems of 30 and 100 covisibilities over a map of
2 000 key frames of 2 000 key points and 100 000 landmarks with about 6 observations each (every landmark observed by key frames around a
centre); every call six times on one stream, the first a warm-up.  Two maps: one in which no key frame is redundant, and one in which every
twentieth key frame sees all its landmarks at a coarser scale than anyone else, with one of them first in every list, so that the first entry is
removed and every later one is counted again against the removed set.  It also times the CPU build of the same header
(plp_model_cull_keyframes_host, one thread) on the same inputs, checks that both gave the same values of every output, and prints the call
times taken with device events on the launch stream.

  python tools/map_cull_bench.py [G ...]
  PLP_FRONT_LIB=build_exp/<name>.so python tools/map_cull_bench.py      # another build of the library (tools/build_variant.sh)
"""
import importlib
import os
import sys
import time

import numpy as np

CALLS = 6
F, L, CAP = 2000, 100000, 2000


def make_map(forced, seed=22):
    rng = np.random.default_rng(seed)
    centre = rng.integers(0, F, L)
    n = rng.integers(4, 10, L)                                    # about 6 observations, every landmark above num_better_obs_thr
    off = np.concatenate([[0], np.cumsum(n)]).astype(np.int32)
    lm_of = np.repeat(np.arange(L), n)
    kf = np.clip(centre[lm_of] + rng.integers(-8, 9, len(lm_of)), 0, F - 1).astype(np.int32)
    order = np.argsort(kf, kind="stable")
    start = np.searchsorted(kf[order], np.arange(F))
    idx = np.zeros(len(kf), np.int32)
    idx[order] = np.arange(len(kf)) - start[kf[order]]
    assert idx.max() < CAP
    kf_lm = np.full((F, CAP), -1, np.int32)
    kf_lm[kf, idx] = lm_of
    plp = importlib.import_module("structure-plp-slam_amd")
    undist = np.zeros((F, CAP), plp.KP_DTYPE)
    undist["octave"] = rng.integers(0, 8, (F, CAP))
    if forced:
        undist["octave"][::20] = 100
    counts = np.bincount(kf, minlength=F).astype(np.int32)
    return dict(kf_lm=kf_lm, kf_counts=counts, undist=undist, kf_id=np.arange(F, dtype=np.uint32), obs_offsets=off, obs_kf=kf, obs_idx=idx), rng


def problems(rng, G, Cv, forced):
    cur = rng.integers(200, F - 200, G).astype(np.int32)
    covis = np.empty((G, Cv), np.int32)
    for g in range(G):
        near = np.concatenate([np.arange(cur[g] - 80, cur[g] - 2), np.arange(cur[g] + 1, cur[g] + 80)])    # the window of three is left out
        pick = rng.permutation(near)[:Cv]
        if forced:                                                # a key frame of the coarse set first
            first = (cur[g] // 20 + 1) * 20
            pick = np.concatenate([[first], pick[pick != first][:Cv - 1]])
        covis[g] = pick
    return cur, (np.arange(G + 1) * Cv).astype(np.int32), covis.reshape(-1)


def run(batches):
    import torch
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
    sys.path[:0] = [root]
    plp = importlib.import_module("structure-plp-slam_amd")
    mt = plp.matcher()
    print(f"library {plp.LIB_PATH.name}; F = {F}, L = {L}, cap = {CAP}")
    print("| map | covisibilities | G | removed per problem (mean) | device call (ms), calls 2-6 | mean | CPU build, one thread (ms) | CPU / device |")
    print("|---|---|---|---|---|---|---|---|")
    tt = {np.uint8: torch.uint8, np.int32: torch.int32}
    for forced in (False, True):
        m, rng = make_map(forced)
        T = len(m["obs_kf"])
        as_dev = lambda v: torch.from_numpy(v.view(np.uint8).reshape(v.shape + (-1,)) if v.dtype.fields else v.view(np.int32) if v.dtype == np.uint32 else v).cuda()
        dev = {k: as_dev(v) for k, v in m.items()}
        for Cv in (30, 100):
            for G in batches:
                cur, off, covis = problems(rng, G, Cv, forced)
                p = dict(cur_kf=cur, covis_offsets=off, covis=covis)
                dev.update({k: as_dev(v) for k, v in p.items()})
                out = {k: torch.zeros(shape(G, G * Cv, F, L), dtype=tt[dt], device="cuda") for k, (shape, dt, optional) in plp.CULL_KEYFRAMES_OUTPUTS.items()
                       if not optional}
                dims = dict(F=F, L=L, T=T, cap=CAP, kp_stride=CAP, G=G, Cv=G * Cv)
                times = []
                for _ in range(CALLS):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    mt.cull_keyframes_device(dims, dev, out, origin_id=0, is_monocular=True)
                    e1.record()
                    torch.cuda.synchronize()
                    times.append(e0.elapsed_time(e1))
                for _ in range(2 if G <= 64 else 1):              # the small calls once more: the first touches the tables' pages
                    t0 = time.perf_counter()
                    want = plp.model_cull_keyframes(origin_id=0, is_monocular=True, outputs=(), **m, **p)
                    cpu_ms = (time.perf_counter() - t0) * 1e3
                for k, w in want.items():
                    assert np.array_equal(out[k].cpu().numpy(), w), (forced, Cv, G, k)
                t = times[1:]
                mean = sum(t) / len(t)
                print(f"| {'early removal' if forced else 'no removal'} | {Cv} | {G} | {want['num_removed'].mean():.2f} | {', '.join(f'{x:.3f}' for x in t)} | "
                      f"{mean:.3f} | {cpu_ms:.1f} | {cpu_ms / mean:.2f} |", flush=True)
    print("device and CPU build gave the same values of every output")


if __name__ == "__main__":
    run([int(a) for a in sys.argv[1:]] or [1, 64, 2048])
