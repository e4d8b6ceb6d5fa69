"""plane_step.run against the host chain (restatement of the grouping -> plp_color_vote_device through the existing entry -> the restatement
tests/plane_ransac_ref.py) on a synthetic instance mask with three labels over two key frames: one label below min_points_before_ransac, one
non-planar, one planar."""
import importlib

import numpy as np
import pytest

import oracle_lib as O
import plane_ransac_ref as PR
import plane_ransac_scene as PS
from plp import plp

pytestmark = pytest.mark.gpu
ROWS, COLS, CAP, C_CAP, ITERS = 120, 160, 200, 4, 10
LABELS = {"few": (10, 0, 0), "bumpy": (0, 20, 0), "flat": (5, 6, 7)}          # colour -> label c0 + (c1 << 8) + (c2 << 16)
REGION = {"few": (10, 50, 10, 60), "bumpy": (10, 50, 80, 150), "flat": (65, 110, 10, 150)}   # y0, y1, x0, x1


def scene(seed):
    """two key frames over one landmark table: dict of numpy arrays"""
    rng = np.random.default_rng(seed)
    G, L = 2, 2 * CAP + 7
    mask = np.zeros((G, ROWS, COLS, 3), np.uint8)
    und = np.zeros((G, CAP), O.KP_DTYPE)
    counts = np.array([CAP, CAP - 23], np.int32)
    lm_index = np.full((G, CAP), -1, np.int32)
    pos_w = rng.uniform(-50.0, 50.0, (L, 3))
    flags = np.zeros(L, np.uint8)
    perm = rng.permutation(L)
    for g in range(G):
        for name, (y0, y1, x0, x1) in REGION.items():
            mask[g, y0:y1, x0:x1] = LABELS[name]
        nrm, u, v, origin = PS.random_plane(rng)
        kinds = rng.choice(["few", "bumpy", "flat", "none"], CAP, p=[0.04, 0.3, 0.5, 0.16])
        kinds[:9] = "few"
        few = np.flatnonzero(kinds == "few")
        kinds[few[11:] if g == 0 else few] = "none"                                 # key frame 0: at most 11, below min_points_before_ransac = 12; key frame 1: none
        for i in range(CAP):
            k = kinds[i]
            if k == "none":
                und["x"][g, i], und["y"][g, i] = rng.uniform(0, COLS), rng.uniform(52, 63)         # between the regions: label 0
            else:
                y0, y1, x0, x1 = REGION[k]
                und["x"][g, i], und["y"][g, i] = rng.uniform(x0 + 2, x1 - 2), rng.uniform(y0 + 2, y1 - 2)
            lm = perm[g * CAP + i]
            lm_index[g, i] = lm if rng.random() > 0.05 else -1
            a, b = rng.uniform(-2, 2, 2)
            h = np.clip(rng.normal(0, PS.DIST_THRESH / 8), -PS.DIST_THRESH / 4, PS.DIST_THRESH / 4) if k == "flat" else rng.uniform(-1, 1)
            if k == "flat" and rng.random() < 0.03:
                h = 10 * PS.DIST_THRESH
            pos_w[lm] = origin + a * u + b * v + h * nrm
    flags[perm[:2 * CAP:17]] = PR.LM_ERASED
    flags[perm[5:2 * CAP:19]] = PR.LM_OWNED
    return dict(mask=mask, undist=und, counts=counts, lm_index=lm_index, pos_w=pos_w, plane_flags=flags)


def host_chain(sc, labels, seed):
    """the grouping restated (labels ascending, key points in key-point order), then the restatement per plane row"""
    G, L, P = 2, len(sc["pos_w"]), 2 * C_CAP
    res, slot_lm, plane_label = [], np.full((P, CAP), -1, np.int32), np.zeros(P, np.int32)
    for g in range(G):
        found = sorted(set(int(l) for l in labels[g] if l != 0))
        for c in range(C_CAP):
            row = g * C_CAP + c
            kps = [i for i in range(CAP) if c < len(found) and labels[g, i] == found[c]]
            plane_label[row] = found[c] if c < len(found) else 0
            slot_lm[row, :len(kps)] = sc["lm_index"][g, kps]
            lms = slot_lm[row, :len(kps)]
            res.append(PR.ransac(PR.CREATE, sc["pos_w"][lms], sc["plane_flags"][lms], PS.DIST_THRESH, PS.ERROR_THRESH, iters=ITERS, seed=seed, p=row))
    want = PR.expected(res, CAP, ITERS)
    lm_plane = np.full(L, -1, np.int32)
    for row, r in enumerate(res):
        if r["status"] == PR.OK:
            lm_plane[slot_lm[row, :len(r["inliers"])][r["inliers"] == 1]] = row
    return want, res, slot_lm, plane_label, lm_plane


def test_plane_step_equals_the_host_chain():
    import torch
    PST = importlib.import_module("structure-plp-slam_amd.plane_step")
    sc = scene(5)
    dev = torch.device("cuda", 0)
    d = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(dev)
    kf = dict(mask=d(sc["mask"]), undist=d(sc["undist"].view(np.uint8).reshape(2, CAP, 28)), counts=d(sc["counts"]), lm_index=d(sc["lm_index"]),
              dist_thresh=d(np.full(2, PS.DIST_THRESH)), error_thresh=PS.ERROR_THRESH)
    lmk = dict(pos_w=d(sc["pos_w"]), plane_flags=d(sc["plane_flags"]))
    step = PST.plane_step(plp, c_cap=C_CAP, iters=ITERS, seed=77)
    out = step.run(kf, lmk, hypotheses=True)
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in out.items()}
    # the vote through the existing entry, with the step's own `valid`
    lm = sc["lm_index"]
    valid = ((lm >= 0) & (sc["plane_flags"][np.clip(lm, 0, None)] == 0)).astype(np.uint8)
    d_lab = torch.full((2, CAP), -5, dtype=torch.int32, device=dev)
    plp._check(plp.lib().plp_color_vote_device(step.mt._h, kf["mask"].data_ptr(), ROWS, COLS, COLS * 3, ROWS * COLS * 3, kf["undist"].data_ptr(),
                                              d(valid).data_ptr(), kf["counts"].data_ptr(), CAP, 2, 1, d_lab.data_ptr(), None))
    torch.cuda.synchronize()
    labels = d_lab.cpu().numpy()
    assert np.array_equal(got["labels"], labels)
    want, res, slot_lm, plane_label, lm_plane = host_chain(sc, labels, 77)
    assert np.array_equal(got["plane_label"], plane_label) and np.array_equal(got["slot_lm"], slot_lm)
    assert np.array_equal(got["num_labels"], [3, 2]) and np.array_equal(got["counts"], (slot_lm >= 0).sum(1))
    for k, w in want.items():
        if k in ("equation", "best_error"):                 # CREATE leaves them alone where it returns before its loop: the step's zeros
            w = np.where(w == PR.SENTINEL[k], 0.0, w)
        if k == "inliers":
            w = np.where(w == PR.SENTINEL[k], 0, w).astype(np.uint8)
        assert np.array_equal(got[k], w, equal_nan=False), (k, got[k], w)
    assert np.array_equal(got["lm_plane"], lm_plane)
    # the three labels: too few points (gated), non-planar (no plane), planar (a plane that keeps most of its points); rows beyond the labels are empty
    order = sorted(LABELS, key=lambda n: LABELS[n][0] + (LABELS[n][1] << 8) + (LABELS[n][2] << 16))
    row = {n: order.index(n) for n in order}
    st, fl = got["status"], got["flags"]
    assert st[row["few"]] == PR.TOO_FEW_POINTS and fl[row["few"]] == PR.FLAG_GATED
    assert st[row["bumpy"]] in (PR.NOT_FOUND, PR.ERROR_ABOVE_THRESHOLD)
    assert st[row["flat"]] == PR.OK and got["active"][row["flat"]] == 1 and got["num_inliers"][row["flat"]] > 50
    assert (got["counts"][[3, 6, 7]] == 0).all() and (got["active"].sum() == 2) and (lm_plane >= 0).sum() == got["num_inliers"][got["active"] == 1].sum()
