"""Workload and summary for profiles/r29_line_map_update.md: plp_trim_line_endpoints_device (both modes), plp_correct_landmark_lines_device and
plp_loop_ba_propagate_lines_device for L = 10 000 and 100 000 line landmarks over 1 000 key frames of 128 key-line slots, lists of 1 - 6 observations,
every call six times on one stream, the first a warm-up.  `run` prints the call times taken with device events on the launch stream and the time of one call of
the CPU build of the same header (plp_model_*_host, one thread), and checks that both gave the same bits of every output.

  rocprofv3 --kernel-trace --stats -d OUT -o kt -- python tools/line_update_bench.py run
  python tools/line_update_bench.py summary OUT/kt_results.db          (markdown: per kernel and size the calls 2-6, their mean, bytes and GB/s)
"""
import importlib
import os
import sqlite3
import sys
import time

import numpy as np

SIZES = (10_000, 100_000)
F, CAP, CALLS = 1000, 128, 6
KERNELS = ("k_trim_line_endpoints", "k_correct_landmark_lines", "k_loop_ba_propagate_lines")
# what a kernel must move per line: 48 B of Pluecker coordinates in, 48 B of coordinates or end points out, the status bytes, and per line the indices and
# gathered rows it reads (counted once per line: with 1 000 key frames they come from L2 after the first touch)
BYTES = dict(k_trim_line_endpoints=48 + 48 + 2 + 4 + 8 + 3.5 * 8 + 16 + 96, k_correct_landmark_lines=48 + 48 + 1 + 8 + 128,
             k_loop_ba_propagate_lines=48 + 48 + 1 + 4 + 1 + 96 + 120)


def workload(L, seed=29):
    """lines in front of their reference key frames, key lines = their float32 projections"""
    rng = np.random.default_rng(seed)
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
    sys.path[:0] = [root, os.path.join(root, "tests")]
    import line_update_scene as S
    plp = importlib.import_module("structure-plp-slam_amd")
    pose = np.zeros((F, 15))
    for f in range(F):
        R = S._rot(*rng.uniform(-0.3, 0.3, 3))
        pose[f] = S.pose_row(R, -R @ rng.uniform(-20.0, 20.0, 3))
    ref = np.sort(rng.integers(0, F, L)).astype(np.int32)       # a map's tables hold the lines of a key frame near one another
    n_obs = rng.integers(1, 7, L)
    off = np.zeros(L + 1, np.int32)
    off[1:] = np.cumsum(n_obs)
    obs_kf = rng.integers(0, F, off[-1]).astype(np.int32)
    obs_idx = rng.integers(0, CAP, off[-1]).astype(np.int32)
    at = off[:-1] + rng.integers(0, n_obs)                       # where the reference key frame stands in the list
    obs_kf[at] = ref
    Rm, t = pose[ref, :9].reshape(L, 3, 3), pose[ref, 9:12]
    pc = np.stack([rng.uniform(-1.5, 1.5, (L, 2)), rng.uniform(-1.0, 1.0, (L, 2)), rng.uniform(3.0, 8.0, (L, 2))], 2)   # (L, 2 points, 3) in the camera
    kl = np.zeros((F, CAP), plp.KL_DTYPE)
    px = (S.CAM[0] * pc[..., 0] / pc[..., 2] + S.CAM[2]).astype(np.float32)
    py = (S.CAM[1] * pc[..., 1] / pc[..., 2] + S.CAM[3]).astype(np.float32)
    kl["startPointX"][ref, obs_idx[at]], kl["startPointY"][ref, obs_idx[at]] = px[:, 0], py[:, 0]
    kl["endPointX"][ref, obs_idx[at]], kl["endPointY"][ref, obs_idx[at]] = px[:, 1], py[:, 1]
    pw = np.einsum("lji,lpj->lpi", Rm, pc - t[:, None, :])      # R^T (p - t)
    d = pw[:, 1] - pw[:, 0]
    pk = np.concatenate([np.cross(pw[:, 0], d), d], 1)
    cw, wc = S.random_sim3(rng, F)
    after = np.zeros((F, 15))
    for f in range(F):
        R = S._rot(*rng.uniform(-0.02, 0.02, 3)) @ pose[f, :9].reshape(3, 3)
        after[f] = S.pose_row(R, pose[f, 9:12] + rng.uniform(-0.1, 0.1, 3))
    return plp, S, dict(pose=pose, kl=kl, pk=pk, old=pw.reshape(L, 6) + rng.normal(0, 0.01, (L, 6)), ref=ref, off=off, obs_kf=obs_kf, obs_idx=obs_idx, cw=cw, wc=wc,
                        after=after, before=np.ascontiguousarray(pose[:, :12]), status=rng.integers(1, 3, F).astype(np.uint8), median=np.full(F, 5.0, np.float32))


def run():
    import torch
    print("| entry | L | device call (us), calls 2-6 | mean | CPU build, one thread (us) | CPU / device | rows written |")
    print("|---|---|---|---|---|---|---|")
    for L in SIZES:
        plp, S, w = workload(L)
        mt, cam = plp.matcher(), S.camera()
        dv = lambda v: torch.from_numpy((v.view(np.uint8).reshape(v.shape + (-1,)) if v.dtype.fields else v).copy()).cuda()
        d = {k: dv(v) for k, v in w.items()}
        pos, st, er, pk2 = (torch.zeros(s, dtype=t, device="cuda") for s, t in (((L, 6), torch.float64), ((L,), torch.uint8), ((L,), torch.uint8), ((L, 6), torch.float64)))
        entries = (
            ("trim, depth", lambda: mt.trim_line_endpoints_device(cam, L, F, CAP, d["pk"], d["ref"], d["off"], d["obs_kf"], d["obs_idx"], d["pose"], d["kl"], pos, st, er),
             lambda: plp.model_trim_line_endpoints(cam, w["pk"], w["ref"], w["off"], w["obs_kf"], w["obs_idx"], w["pose"], w["kl"]), dict(pos_w=pos, status=st, erase=er)),
            ("trim, max change", lambda: mt.trim_line_endpoints_device(cam, L, F, CAP, d["pk"], d["ref"], d["off"], d["obs_kf"], d["obs_idx"], d["pose"], d["kl"], pos, st, er,
                                                                       mode=plp.TRIM_MAX_CHANGE, pos_w_old=d["old"], median_depth=d["median"]),
             lambda: plp.model_trim_line_endpoints(cam, w["pk"], w["ref"], w["off"], w["obs_kf"], w["obs_idx"], w["pose"], w["kl"], mode=plp.TRIM_MAX_CHANGE,
                                                   pos_w_old=w["old"], median_depth=w["median"]), dict(pos_w=pos, status=st, erase=er)),
            ("correct lines", lambda: mt.correct_landmark_lines_device(L, F, d["pk"], d["ref"], d["cw"], d["wc"], pk2, st),
             lambda: plp.model_correct_landmark_lines(w["pk"], w["ref"], w["cw"], w["wc"]), dict(pluecker=pk2, status=st)),
            ("propagate lines", lambda: mt.loop_ba_propagate_lines_device(L, F, d["after"], d["before"], d["status"], d["pk"], d["ref"], pk2, st),
             lambda: plp.model_loop_ba_propagate_lines(w["after"], w["before"], w["status"], w["pk"], w["ref"]), dict(pluecker=pk2, status=st)))
        for name, device, host, outs in entries:
            written = (plp.LOOP_BA_LM_OPTIMIZED, plp.LOOP_BA_LM_MOVED) if name == "propagate lines" else (0,)     # TRIM_OK = CORRECT_LINE_OK = 0
            for o in outs.values():
                o.zero_()
            times = []
            for _ in range(CALLS):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                device()
                e1.record()
                torch.cuda.synchronize()
                times.append(e0.elapsed_time(e1) * 1e3)
            t0 = time.perf_counter()
            want = host()
            cpu_us = (time.perf_counter() - t0) * 1e6
            for k, o in outs.items():
                assert S.same_bits(o.cpu().numpy(), want[k]), (name, L, k)
            t = times[1:]
            mean = sum(t) / len(t)
            print(f"| {name} | {L} | {', '.join(f'{x:.0f}' for x in t)} | {mean:.0f} | {cpu_us:.0f} | {cpu_us / mean:.1f} | {int(np.isin(want['status'], written).sum())} |", flush=True)
    print("device and CPU build gave the same bits of every output")


def summary(path, hbm_gbs=8000.0):
    db = sqlite3.connect(path)
    table = [r[0] for r in db.execute("select name from sqlite_master where type in ('table', 'view') and name like '%kernels%'")]
    table = "kernels" if "kernels" in table else table[0]
    cols = [r[1] for r in db.execute(f"pragma table_info({table})")]
    name_c = "name" if "name" in cols else "kernel_name"
    s_c = "start" if "start" in cols else "start_timestamp"
    e_c = "end" if "end" in cols else "end_timestamp"
    rows = [(nm, (e - s) / 1e3) for nm, s, e in db.execute(f"select {name_c}, {s_c}, {e_c} from {table} order by {s_c}")]
    print("| kernel | L | per call (us), calls 2-6 | mean | bytes per line | GB/s | of the HBM figure |")
    print("|---|---|---|---|---|---|---|")
    for kern in KERNELS:
        us = [t for nm, t in rows if kern in nm]
        per = len(us) // (CALLS * len(SIZES))                  # the trim runs in two modes
        assert per * CALLS * len(SIZES) == len(us) and per, (kern, len(us))
        for i, L in enumerate(SIZES):
            for m in range(per):
                t = us[(i * per + m) * CALLS + 1:(i * per + m + 1) * CALLS]
                mean = sum(t) / len(t)
                gbs = BYTES[kern] * L / (mean * 1e-6) / 1e9
                print(f"| `{kern}`{' (max change)' if m else ''} | {L} | {', '.join(f'{x:.1f}' for x in t)} | {mean:.1f} | {BYTES[kern]:.0f} | {gbs:.0f} | {100 * gbs / hbm_gbs:.1f} % |")


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "summary":
        summary(sys.argv[2], *(float(v) for v in sys.argv[3:4]))
    else:
        run()
