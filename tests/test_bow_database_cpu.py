"""CPU checks of the place-recognition entries (plp_bow_query_* / plp_bow_score_pairs_*): the census of the branches the
scenes of tests/bow_database_ref.py reach in the restatement alone (so that the device test cannot pass by missing one); the host build of
csrc/bow_score.hpp (plp_model_bow_score_host, the terms and the order the kernels keep) against the restatement's score, bit for bit; and the
same header under AddressSanitizer and UBSan in a stand-alone program (tools/bow_score_sanitized.cpp).  The device is held to the same
restatement in tests/test_gpu_bow_database.py."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import bow_database_ref as B
from plp import plp

f32, f64 = np.float32, np.float64
SEEDS = (1, 2, 3)                     # the scenes tests/test_gpu_bow_database.py runs on the device
ROOT = os.path.join(os.path.dirname(__file__), "..")


@pytest.mark.parametrize("seed", SEEDS)
def test_the_restatement_reaches_every_branch_on_the_committed_seeds(seed):
    S = B.scene(seed)
    R = B.run(S)
    c = B.census(S, R)
    print(seed, c)
    for name, n in c.items():
        assert n >= 1, (name, c)
    assert c["shared_best_kf"] >= 1 and R["n_final"][0] >= 2 and R["status"].tolist() == [0, 3, 1]
    # the relocalisation form of the same scene (no rejected key frames, min_score 0) differs: the checks of reject and min_score are not vacuous
    R2 = B.run(S, use_reject=False, use_min_score=False)
    assert R2["max_common"][0] > R["max_common"][0] and R2["status"][1] == 0 and not np.array_equal(R2["final"], R["final"])


def vectors():
    """(name, wa, va, wb, vb): lengths 0, 1, 63, 64, 65 and 8192, disjoint, identical and interleaved vectors"""
    rng = np.random.default_rng(12)
    out = []

    def vec(n, universe):
        w = np.sort(rng.choice(universe, n, replace=False)).astype(np.uint32)
        v = rng.random(n) + 0.01
        return w, v / v.sum()
    for n in (0, 1, 63, 64, 65, 8192):
        a = vec(n, max(2 * n, 4))
        b = vec(n, max(2 * n, 4))                              # about half of the words shared
        out.append((f"n{n}", *a, *b))
        out.append((f"n{n}_vs_100", *a, *vec(100, 200)))
        out.append((f"identical{n}", *a, *a))
    a, b = vec(300, 1000), vec(300, 1000)
    out.append(("disjoint", a[0] * 2, a[1], b[0] * 2 + 1, b[1]))               # even against odd ids
    w = np.arange(0, 600, dtype=np.uint32)
    out.append(("interleaved", w[w % 3 != 0], vec(400, 400)[1], w[w % 3 != 1], vec(400, 400)[1]))   # runs of shared and unshared words alternate
    out.append(("negative_values", a[0], a[1] - 0.002, a[0], b[1] - 0.002))    # fabs() matters
    return out


def ref_score(wa, va, wb, vb):
    return B.l1_score(B.bow_vec_of(wa, va, len(wa)), B.bow_vec_of(wb, vb, len(wb)))


def test_model_score_equals_the_restatement_bit_for_bit():
    worst = 0.0
    for name, wa, va, wb, vb in vectors():
        got, want = f64(plp.model_bow_score(wa, va, wb, vb)), ref_score(wa, va, wb, vb)
        assert got.tobytes() == f64(want).tobytes(), (name, got, want)
        if name.startswith("identical") and len(wa):
            worst = max(worst, abs(float(got) - 1.0))
        if name == "disjoint" or name.endswith("n0") or name.startswith("n0"):
            assert float(got) == 0.0, name
    print("identical vectors: worst |score - 1| =", worst)
    assert worst < 1e-12                                                         # 8192 terms of rounding, not 0: recorded, not assumed
    # the order of the arguments is part of the definition: (|v - w| - |v|) - |w|
    assert ref_score(*vectors()[3][1:]) == plp.model_bow_score(*vectors()[3][1:])


def test_the_score_header_runs_clean_under_address_and_ub_sanitizers(tmp_path):
    """a stand-alone program with its own main, not code loaded into python"""
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed"
    exe = tmp_path / "bow_score_sanitized"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", str(exe),
                    os.path.join(ROOT, "tools", "bow_score_sanitized.cpp")], check=True)
    cases = vectors()
    blob = struct.pack("<i", len(cases))
    for _, wa, va, wb, vb in cases:
        blob += struct.pack("<ii", len(wa), len(wb)) + wa.astype("<u4").tobytes() + va.astype("<f8").tobytes() + wb.astype("<u4").tobytes() + vb.astype("<f8").tobytes()
    path = tmp_path / "cases.bin"
    path.write_bytes(blob)
    r = subprocess.run([str(exe), str(path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.split("\n")
    scores = [l.split()[1] for l in lines if l.startswith("score ")]
    assert len(scores) == len(cases)
    for (name, wa, va, wb, vb), got in zip(cases, scores):
        assert got == f64(ref_score(wa, va, wb, vb)).tobytes()[::-1].hex(), name
    thr = {int(l.split()[1]): int(l.split()[2]) for l in lines if l.startswith("thr ")}
    assert len(thr) == 2001 and all(v == int(f32(f32(0.8) * f32(m))) for m, v in thr.items())
    mt = {int(l.split()[1]): l.split()[2] for l in lines if l.startswith("min_total ")}
    assert len(mt) == 65 and all(v == f32(f32(0.75) * f32(f32(i) / f32(7.0))).tobytes()[::-1].hex() for i, v in mt.items())
