"""Workload and summary for profiles/r12_bow_database.md: plp_bow_query_device on a database of N = 10 000 rows x about 900 words (100 places of
100 key frames that share a core of words; a query is one more view of a place) for Q = 1 and Q = 64 on both count paths, and
plp_bow_score_pairs_device at P = 10 000; every call six times on one stream, the first a warm-up.

  rocprofv3 --kernel-trace --stats -d OUT -o kt -- python tools/bow_database_bench.py run
  python tools/bow_database_bench.py summary OUT/kt_results.db          (markdown: per kernel and configuration the calls 2-6 and their mean)
"""
import importlib
import os
import sqlite3
import sys

import numpy as np

CONFIGS = [("bitmap", 1), ("bitmap", 64), ("bisection", 1), ("bisection", 64)]
CALLS = 6
N, STRIDE, N_WORDS, PLACES, P = 10000, 1024, 1_000_000, 100, 10000


def scene(rng):
    per = N // PLACES
    cores = [rng.choice(N_WORDS, 2000, replace=False) for _ in range(PLACES)]

    def view(place):
        w = np.unique(np.concatenate([rng.choice(cores[place], 700, replace=False), rng.integers(0, N_WORDS, 200)])).astype(np.uint32)
        v = rng.random(len(w)) + 0.05
        return w, v / v.sum()
    word, value, n = np.zeros((N, STRIDE), np.uint32), np.zeros((N, STRIDE)), np.zeros(N, np.int32)
    for k in range(N):
        w, v = view(k // per)
        word[k, :len(w)], value[k, :len(w)], n[k] = w, v, len(w)
    qw, qv, qn = np.zeros((64, STRIDE), np.uint32), np.zeros((64, STRIDE)), np.zeros(64, np.int32)
    for q in range(64):
        w, v = view(q % PLACES)
        qw[q, :len(w)], qv[q, :len(w)], qn[q] = w, v, len(w)
    covis = np.zeros((N, 10), np.int32)
    for k in range(N):
        covis[k] = (k // per) * per + (k % per + 1 + np.arange(10)) % per
    return word, value, n, qw, qv, qn, covis


def run():
    import torch
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    plp = importlib.import_module("structure-plp-slam_amd")
    dev = torch.device("cuda", 0)
    word, value, n, qw, qv, qn, covis = scene(np.random.default_rng(0))
    T = lambda a: torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to(dev)
    d_value, d_n, d_qv, d_qn, d_covis = T(value), T(n), T(qv), T(qn), T(covis)
    d_ncov = torch.full((N,), 10, dtype=torch.int32, device=dev)
    tables = {"bitmap": (N_WORDS, T(word), T(qw)), "bisection": (N_WORDS + 1_400_000, T(word + np.uint32(1_400_000)), T(qw + np.uint32(1_400_000)))}
    mt = plp.matcher()
    tt = {np.uint32: torch.int32, np.float32: torch.float32, np.int32: torch.int32, np.uint8: torch.uint8}
    results = {}
    for path, Q in CONFIGS:
        n_words, d_word, d_qw = tables[path]
        out = {k: torch.empty((Q, N) if rows else (Q,), dtype=tt[dt], device=dev) for k, (rows, dt) in plp.BOW_QUERY_OUTPUTS.items()}
        for _ in range(CALLS):
            mt.bow_query_device(n_words, N, STRIDE, d_word, d_value, d_n, Q, STRIDE, d_qw, d_qv, d_qn, out, covis_cap=10, covis=d_covis, n_covis=d_ncov)
            torch.cuda.synchronize()
        results[(path, Q)] = {k: v.cpu().numpy() for k, v in out.items()}
    rng = np.random.default_rng(1)
    a_row, b_row = T(rng.integers(0, 64, P).astype(np.int32)), T(rng.integers(0, N, P).astype(np.int32))
    score = torch.empty(P, dtype=torch.float32, device=dev)
    n_words, d_word, d_qw = tables["bitmap"]
    for _ in range(CALLS):
        mt.bow_score_pairs_device(64, STRIDE, d_qw, d_qv, d_qn, N, STRIDE, d_word, d_value, d_n, P, a_row, b_row, score)
        torch.cuda.synchronize()
    for Q in (1, 64):
        for k in plp.BOW_QUERY_OUTPUTS:
            assert np.array_equal(results[("bitmap", Q)][k], results[("bisection", Q)][k]), (Q, k)
    r = results[("bitmap", 64)]
    scored = (r["score"].view(np.float32) >= 0).sum(axis=1)
    print(f"words per row {n.mean():.0f}, database words {int(n.sum())}, max_common {r['max_common'].view(np.uint32).min()}-{r['max_common'].view(np.uint32).max()}, "
          f"rows scored per query {scored.min()}-{scored.max()}, n_final {r['n_final'].min()}-{r['n_final'].max()}, status {np.bincount(r['status'], minlength=4).tolist()}; "
          f"both count paths gave the same bits of every output")


def summary(path):
    db = sqlite3.connect(path)
    cols = [r[1] for r in db.execute("pragma table_info(kernels)")]
    name_c = "name" if "name" in cols else "kernel_name"
    s_c = "start" if "start" in cols else "start_timestamp"
    e_c = "end" if "end" in cols else "end_timestamp"
    rows = [(nm, (e - s) / 1e3) for nm, s, e in db.execute(f"select {name_c}, {s_c}, {e_c} from kernels order by {s_c}") if "k_bow_" in nm]
    by = {}
    for nm, us in rows:
        short = nm.split("(")[0].replace("void ", "").replace("plp::", "").replace("(anonymous namespace)::", "")
        by.setdefault(short, []).append(us)
    print("| kernel | configuration | per call (us), calls 2-6 | mean |")
    print("|---|---|---|---|")
    for short, us in by.items():
        if "count<true>" in short or "ILb1" in short:
            cfgs = [c for c in CONFIGS if c[0] == "bitmap"]
        elif "count" in short:
            cfgs = [c for c in CONFIGS if c[0] == "bisection"]
        elif "pairs" in short:
            cfgs = [("P", P)]
        else:
            cfgs = CONFIGS
        assert len(us) == CALLS * len(cfgs), (short, len(us))
        for i, c in enumerate(cfgs):
            t = us[i * CALLS + 1:(i + 1) * CALLS]
            print(f"| `{short}` | {c[0]} {c[1]} | {', '.join(f'{x:.1f}' for x in t)} | {sum(t) / len(t):.1f} |")


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "summary":
        summary(sys.argv[2])
    else:
        run()
