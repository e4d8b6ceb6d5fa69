"""relocalization_step.run for the C candidates of one frame, end to end: the BoW match on the device (PLP_MATCH_MODE_BOW: targets = the frame's
key points, queries = the candidate's key points with a landmark in BoW node order) -> the step's gather -> plp_pnp_ransac_device, against
the oracle's BoW match (tests/oracle_lib.py match_bow) -> a gather on the host -> the plain-Python restatement tests/pnp_solver_ref.py.  One
candidate finds its pose, one has fewer than ten matches, one is matched to landmarks that were erased after the match.  The pose rows the
step leaves are then the `pose` of plp_project_landmarks_device, whose output is held to the restatement tests/project_landmarks_ref.py for
the recovered pose."""
import importlib

import numpy as np
import pytest

import landmark_observe_ref as R
import oracle_lib as O
import pnp_solver_ref as REF
import pnp_solver_scene as S
import project_landmarks_ref as PR
import project_landmarks_scene as PS
from plp import plp
from test_gpu_landmark_observe import yaml_of

pytestmark = pytest.mark.gpu
CAP, CAP2, M_CAP, ITERS, NODES = 150, 170, 140, 30, 12
LSF = R.d5_logf(np.float32(1.2))


def tables(C):
    """the map of the test: the frame sees 120 landmarks 3 - 9 m in front of it at its first 120 key points; candidate c holds copies of
    them (rows 200 + 150 c ...) at shuffled key points, 30 % of the copies somewhere else (wrong matches).  A key point of the candidate
    that is to match frame key point k carries k's descriptor with up to six bits flipped, its BoW node and nearly its angle; every other
    descriptor is random (some 128 bits from anything).  The queries of candidate c are its key points with a landmark, in node order."""
    rng = np.random.default_rng(42)
    L = 200 + 150 * 3
    pos_w = rng.uniform(-50, 50, (L, 3))
    erased = np.zeros(L, np.uint8)
    depth = rng.uniform(3.0, 9.0, 120)
    xc = np.stack([depth * np.tan(rng.uniform(-0.35, 0.35, 120)), depth * np.tan(rng.uniform(-0.25, 0.25, 120)), depth], 1)
    Rcw, tcw = S.rotation(rng, 3.0), rng.uniform(-5, 5, 3)
    bearing = np.zeros((CAP, 3))
    bearing[:120] = xc / np.linalg.norm(xc, axis=1, keepdims=True)
    bearing[120:] = S.directions(rng, CAP - 120, 0.5)
    octave = rng.integers(0, 8, CAP).astype(np.int32)
    t_desc = rng.integers(0, 256, (CAP, 32)).astype(np.uint8)
    t_angle = rng.uniform(0.0, 360.0, CAP).astype(np.float32)
    t_node = rng.integers(0, NODES, CAP).astype(np.int32)
    cand_lm = np.full((3, CAP2), -1, np.int32)
    q_feature = np.zeros((3, M_CAP), np.int32)
    q_desc = np.zeros((3, M_CAP, 32), np.uint8)
    q_angle = np.zeros((3, M_CAP), np.float32)
    q_node = np.zeros((3, M_CAP), np.int32)
    q_counts = np.zeros(3, np.int32)
    n_matched = (110, 8, 100)                                                      # candidate 1: below min_num_inliers = 10
    for c in range(3):
        rows = 200 + 150 * c + np.arange(120)
        pos_w[rows] = (xc - tcw) @ Rcw                                             # rot_cw^T (x_c - trans_cw)
        wrong = rng.random(120) < 0.3
        pos_w[rows[wrong]] = rng.uniform(-50, 50, (int(wrong.sum()), 3))
        kp2 = rng.permutation(CAP2)[:120]                                          # landmark k of the candidate sits at its key point kp2[k]
        cand_lm[c, kp2] = rows
        desc = rng.integers(0, 256, (CAP2, 32)).astype(np.uint8)
        angle = rng.uniform(0.0, 360.0, CAP2).astype(np.float32)
        node = rng.integers(0, NODES, CAP2).astype(np.int32)
        for k in rng.choice(120, n_matched[c], replace=False):                    # matched pairs (frame key point k, candidate key point kp2[k])
            d = t_desc[k].copy()
            for bit in rng.choice(256, int(rng.integers(0, 7)), replace=False):
                d[bit // 8] ^= np.uint8(1 << (bit % 8))
            desc[kp2[k]], node[kp2[k]] = d, t_node[k]
            angle[kp2[k]] = np.float32((float(t_angle[k]) + rng.uniform(-2.0, 2.0)) % 360.0)
        live = np.flatnonzero(cand_lm[c] >= 0)
        order = live[np.argsort(node[live], kind="stable")]                        # the reference walks the key frame's features in node order
        n = len(order)
        q_feature[c, :n], q_desc[c, :n], q_angle[c, :n], q_node[c, :n], q_counts[c] = order, desc[order], angle[order], node[order], n
        if c == 2:
            erased[rows] = 1                                                       # candidate 2: every matched landmark is erased after the match
    t = dict(q_feature=q_feature, q_desc=q_desc, q_angle=q_angle, q_node=q_node, q_counts=q_counts, cand_lm=cand_lm, bearing=bearing, octave=octave,
             pos_w=pos_w, erased=erased, t_desc=t_desc, t_angle=t_angle, t_node=t_node)
    for k in ("q_feature", "q_desc", "q_angle", "q_node", "q_counts", "cand_lm"):
        t[k] = t[k][:C].copy()
    return t, (Rcw, tcw)


def oracle_bow_match(t):
    """bow_tree::match_frame_and_keyframe by the oracle, candidate by candidate: out_match[c][idx] = the query matched to key point idx of
    the frame, -1 = none"""
    C = len(t["q_counts"])
    out = np.full((C, CAP), -1, np.int32)
    for c in range(C):
        n = int(t["q_counts"][c])
        out[c], _ = O.match_bow(t["q_desc"][c, :n], t["q_angle"][c, :n], t["q_node"][c, :n], np.ones(n, np.uint8), t["t_desc"], t["t_angle"], t["t_node"],
                                np.zeros(CAP, np.uint8), 0.75, True)
    return out


def device_bow_match(mt_bow, t):
    """the same by PLP_MATCH_MODE_BOW, all candidates in one call; the result stays on the device"""
    import torch
    C = len(t["q_counts"])
    d = lambda v: torch.from_numpy(np.ascontiguousarray(v)).cuda()
    rep = lambda v: d(np.broadcast_to(v, (C,) + v.shape).copy())
    out_match = torch.full((C, CAP), -77, dtype=torch.int32, device="cuda")
    out_num = torch.zeros(C, dtype=torch.int32, device="cuda")
    fields = dict(t_desc=rep(t["t_desc"]), t_angle=rep(t["t_angle"]), t_group=rep(t["t_node"]), q_desc=d(t["q_desc"]), q_angle=d(t["q_angle"]),
                  q_group=d(t["q_node"]), q_counts=d(t["q_counts"]))
    mt_bow.match_device(plp.MODE_BOW, CAP, M_CAP, fields, out_match, out_num, B=C)
    return out_match, fields


def host_gather(t, out_match):
    """extract_valid_indices + setup_pnp_solver (module/relocalizer.cc:254-291) over the tables, candidate by candidate, key point by key point"""
    C = len(out_match)
    g = dict(valid=np.zeros((C, CAP), np.uint8), bearing=np.zeros((C, CAP, 3)), pos_w=np.zeros((C, CAP, 3)), octave=np.zeros((C, CAP), np.int32))
    for c in range(C):
        for idx in range(CAP):
            g["bearing"][c, idx], g["octave"][c, idx] = t["bearing"][idx], t["octave"][idx]
            q = out_match[c, idx]
            if q < 0:
                continue
            lm = int(t["cand_lm"][c, t["q_feature"][c, q]])                        # matched_landmarks.at(idx)
            if lm < 0 or t["erased"][lm]:
                continue
            g["valid"][c, idx] = 1
            g["pos_w"][c, idx] = t["pos_w"][lm]
    return g


@pytest.mark.parametrize("C", [1, 3])
def test_the_step_equals_the_oracle_match_a_host_gather_and_the_restatement(C):
    import torch
    step_mod = importlib.import_module("structure-plp-slam_amd.relocalization_step")
    t, (Rcw, tcw) = tables(C)
    want_match = oracle_bow_match(t)
    g = host_gather(t, want_match)
    want = [REF.find_via_ransac(g["valid"][c].tolist(), g["bearing"][c].tolist(), g["pos_w"][c].tolist(), g["octave"][c].tolist(), S.SCALE_FACTORS.tolist(),
                                iters=ITERS, seed=31, p=c) for c in range(C)]
    assert [w["status"] for w in want] == [REF.OK, REF.TOO_FEW_MATCHES, REF.TOO_FEW_MATCHES][:C]
    assert want[0]["num_matches"] >= 80
    if C == 3:
        assert 4 <= want[1]["num_matches"] < 10 and want[2]["num_matches"] == 0 and (want_match[2] >= 0).sum() >= 80
    mt = plp.matcher()
    step = step_mod.relocalization_step(plp, S.SCALE_FACTORS, iters=ITERS, mt=mt)
    out_match, keep = device_bow_match(plp.matcher(0.75, True), t)                  # relocalizer's bow_matcher_(0.75, true)
    d = {k: torch.from_numpy(v.copy()).cuda() for k, v in t.items() if k in ("q_feature", "cand_lm", "bearing", "octave", "pos_w", "erased")}
    out = step.run(out_match, d["q_feature"], d["cand_lm"], d["bearing"], d["octave"], d["pos_w"], d["erased"], seed=31)
    # the projection match that follows (relocalizer.cc:137) takes the pose rows as they lie in HBM: all landmarks of every candidate
    cm = plp.camera_model(yaml_of("fr1"))
    m = 120
    lm_pos = np.stack([t["pos_w"][200 + 150 * c + np.arange(m)] for c in range(C)])
    mn, mx = np.full((C, m), 0.5, np.float32), np.full((C, m), 40.0, np.float32)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    full = lambda shape, val, dt: torch.full(shape, val, dtype=dt, device="cuda")
    o = dict(reproj_d=full((C, m, 2), -77.0, torch.float64), reproj=full((C, m, 2), -77.0, torch.float32), x_right=full((C, m), -77.0, torch.float32),
             level=full((C, m), -77, torch.int32), valid=full((C, m), 77, torch.uint8), status=full((C, m), 77, torch.uint8),
             num_valid=full((C,), -1, torch.int32))
    mt.project_landmarks_device(cm, C, m, out["pose"], T(lm_pos), T(mn), T(mx), o["valid"], out_reproj_d=o["reproj_d"], out_reproj=o["reproj"],
                                out_x_right=o["x_right"], out_level=o["level"], out_status=o["status"], out_num_valid=o["num_valid"],
                                ray_test=False, log_scale_factor=LSF, num_levels=8)
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in out.items()}
    assert np.array_equal(out_match.cpu().numpy(), want_match)                      # the device BoW match is the oracle's
    v = g["valid"].astype(bool)
    assert np.array_equal(got["valid"], g["valid"])
    assert np.array_equal(got["pos_w"][v], g["pos_w"][v])                          # what a slot that is not valid holds does not matter
    assert np.array_equal(got["bearing"], g["bearing"]) and np.array_equal(got["octave"], g["octave"])
    for c, w in enumerate(want):                                                   # the restatement, bit for bit
        assert (int(got["status"][c]), int(got["num_matches"][c]), int(got["num_inliers"][c]), int(got["best_iter"][c])) == \
               (w["status"], w["num_matches"], w["num_inliers"], w["best_iter"]), c
        assert got["inliers"][c].tolist() == w["inliers"], c
        assert got["rot_cw"][c].tobytes() == np.array(w["R"]).tobytes() and got["trans_cw"][c].tobytes() == np.array(w["t"]).tobytes(), c
    want = dict(rot_cw=got["rot_cw"], trans_cw=got["trans_cw"])
    for c in range(C):
        row = plp.frame_pose(want["rot_cw"][c], want["trans_cw"][c])
        assert got["pose"][c].tobytes() == row.tobytes(), c
    # the projection on the recovered pose equals the restatement's, and sees the landmarks the frame sees
    p = {k: x.cpu().numpy() for k, x in o.items()}
    ref = PR.project_points(PS.ref_cam(cm), cm.img_bounds, got["pose"][0], lm_pos[0], None, mn[0], mx[0], None, PR.DIST_CENTER, False, LSF, 8)
    assert int(p["num_valid"][0]) == ref["num_valid"] >= 60
    assert np.array_equal(p["valid"][0], ref["valid"]) and np.array_equal(p["status"][0], ref["status"])
    kept = ref["valid"].astype(bool)                                               # the other outputs are written where the landmark is kept
    for k in ("level", "reproj_d", "reproj", "x_right"):
        assert np.array_equal(p[k][0][kept], ref[k][kept]), k
