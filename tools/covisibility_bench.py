"""Workload for profiles/r23_covisibility.md: plp_covisibility_update_device for G = 1, 30 and F owners and plp_covisibility_erase_device for 1
and 16 key frames over the map of tools/map_cull_bench.py (2 000 key frames of 2 000 key points, 100 000 landmarks of about 6 observations),
on a graph that every key frame's update has settled; every call six times on one stream, the first a warm-up, each from the same state.  It
also times the CPU build of the same header (plp_model_covisibility_*_host, one thread) on the same inputs, checks that both gave the same
values of every table and every output, and prints the call times taken with device events on the launch stream.

  python tools/covisibility_bench.py
  PLP_FRONT_LIB=build_exp/<name>.so python tools/covisibility_bench.py      # another build of the library (tools/build_variant.sh)
"""
import importlib
import os
import sys
import time

import numpy as np

CALLS = 6
CAPS = 96


def run():
    import torch
    root = os.path.dirname(os.path.abspath(__file__))
    sys.path[:0] = [os.path.join(root, ".."), root]
    from map_cull_bench import CAP, F, L, make_map
    plp = importlib.import_module("structure-plp-slam_amd")
    mt = plp.matcher()
    m, rng = make_map(False)
    m = {k: m[k] for k in ("kf_lm", "kf_counts", "obs_offsets", "obs_kf", "kf_id")}
    T = len(m["obs_kf"])
    print(f"library {plp.LIB_PATH.name}; F = {F}, L = {L}, cap = {CAP}, T = {T}, conn_cap = covis_cap = {CAPS}")
    as_dev = lambda v: torch.from_numpy(v.view(np.int32) if v.dtype == np.uint32 else v).cuda()
    dev = {k: as_dev(v) for k, v in m.items()}
    tt = {np.uint8: torch.uint8, np.int32: torch.int32}
    # the settled graph: every key frame an owner, on the CPU build
    settled = plp.covisibility_state(F, CAPS, CAPS)
    first = plp.model_covisibility_update(state=settled, owners=np.arange(F, dtype=np.int32), **m)
    assert (first["touched"] == 1).all() and (first["status"] == plp.COVIS_OK).all()
    print(f"connected per key frame: mean {settled['kf_n_conn'].mean():.1f}, max {settled['kf_n_conn'].max()}; ordered: mean "
          f"{settled['kf_n_covis'].mean():.1f}, max {settled['kf_n_covis'].max()}")
    print("| call | G | device call (ms), calls 2-6 | mean | CPU build, one thread (ms) | CPU / device |")
    print("|---|---|---|---|---|---|")

    def timed(call, state_names):
        times = []
        for _ in range(CALLS):
            state = {k: as_dev(settled[k]) for k in state_names}
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = call(state)
            e1.record()
            torch.cuda.synchronize()
            times.append(e0.elapsed_time(e1))
        return times[1:], state, out

    def report(name, G, t, cpu_ms):
        mean = sum(t) / len(t)
        print(f"| {name} | {G} | {', '.join(f'{x:.3f}' for x in t)} | {mean:.3f} | {cpu_ms:.2f} | {cpu_ms / mean:.2f} |", flush=True)

    for G in (1, 30, F):
        owners = np.arange(F, dtype=np.int32) if G == F else (1000 + np.arange(G) * 3 - G).astype(np.int32)   # a new key frame; a loop's neighbours; a map load
        d_own = as_dev(owners)

        def call(state):
            out = {k: torch.zeros(G if per == "G" else F, dtype=tt[dt], device="cuda") for k, (per, dt, _) in plp.COVISIBILITY_OUTPUTS.items()}
            mt.covisibility_update_device(dict(F=F, L=L, T=T, cap=CAP, conn_cap=CAPS, covis_cap=CAPS, G=G), dict(dev, owners=d_own, **state), out)
            return out
        t, state, out = timed(call, tuple(plp.COVISIBILITY_STATE))
        for _ in range(2 if G < F else 1):                    # the small calls once more: the first touches the tables' pages
            host = {k: v.copy() for k, v in settled.items()}
            t0 = time.perf_counter()
            want = plp.model_covisibility_update(state=host, owners=owners, **m)
            cpu_ms = (time.perf_counter() - t0) * 1e3
        for k, w in list(want.items()) + list(host.items()):
            got = (out[k] if k in out else state[k]).cpu().numpy()
            assert np.array_equal(got, w), ("update", G, k)
        report("update", G, t, cpu_ms)
    for G in (1, 16):
        mask = np.zeros(F, np.uint8)
        mask[1000 + np.arange(G) * 2] = 1
        d_mask = as_dev(mask)

        def call(state):
            out = dict(status=torch.zeros(F, dtype=torch.uint8, device="cuda"), touched=torch.zeros(F, dtype=torch.uint8, device="cuda"))
            mt.covisibility_erase_device(dict(F=F, conn_cap=CAPS, covis_cap=CAPS), dict(state, erased=d_mask), out)
            return out
        t, state, out = timed(call, plp.COVISIBILITY_ERASE_STATE)
        for _ in range(2):
            host = {k: settled[k].copy() for k in plp.COVISIBILITY_ERASE_STATE}
            t0 = time.perf_counter()
            want = plp.model_covisibility_erase(host, mask)
            cpu_ms = (time.perf_counter() - t0) * 1e3
        for k, w in list(want.items()) + list(host.items()):
            got = (out[k] if k in out else state[k]).cpu().numpy()
            assert np.array_equal(got, w), ("erase", G, k)
        report("erase", G, t, cpu_ms)
    print("device and CPU build gave the same values of every table and every output")


if __name__ == "__main__":
    run()
