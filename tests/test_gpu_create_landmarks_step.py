"""The landmark-creation step (structure-plp-slam_amd/create_landmarks_step.py) for G current key frames x N neighbours, from poses and feature
tables, against the host chain it replaces: restatement geometry (tests/keypoint_pairs_ref.py) -> oracle match_for_triangulation
(tests/oracle_lib.py) -> restatement triangulation, the occupancy carried from rank to rank as keyframe::add_landmark does."""
import importlib

import numpy as np
import pytest

import keypoint_pairs_ref as KR
import keypoint_pairs_scene as S
import oracle_lib as O
from plp import plp

pytestmark = pytest.mark.gpu
CAP = S.CAP
MODEL_ID = dict(perspective=0, fisheye=1, equirectangular=2)
step_mod = importlib.import_module("structure-plp-slam_amd.create_landmarks_step")


def _camera(d):
    c = plp.camera_model_c()
    c.model, c.cols, c.rows = MODEL_ID[d["model"]], d["cols"], d["rows"]
    for k in ("fx", "fy", "cx", "cy", "focal_x_baseline"):
        setattr(c, k, float(d[k]))
    return c


def _t(a):
    import torch
    a = np.ascontiguousarray(a)
    if a.dtype.fields is not None:
        a = a.view(np.uint8).reshape(a.shape + (-1,))
    return torch.from_numpy(a).to(torch.device("cuda", 0))


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _scene(setup, model, seed):
    sc = S.add_descriptors(S.make_scene(seed, setup, model, F=12, n_pts=90), seed + 1)
    rng = np.random.default_rng(seed + 2)
    for kf in sc["kfs"]:                                        # some key points hold a landmark already
        # the matcher reads scale_factors[octave] unclamped, as the reference's at() would throw: keep the scene's planted octaves inside the table
        kf["keypts"]["octave"] = np.clip(kf["keypts"]["octave"], 0, S.NUM_LEVELS - 1)
        kf["occupied"] = (rng.uniform(size=len(kf["keypts"])) < 0.15).astype(np.uint8)
        # the key frame's landmarks for compute_median_depth: the points it sees (any set does: both sides read the same numbers)
        kf["lm_pos_w"] = sc["points"][kf["pid"]]
    return sc


def host_chain(sc, cur, neighbours, carry=True):
    """create_new_landmarks per current key frame: neighbour after neighbour -> per (rank, g): idx_1, pos_w, status over the neighbour's key
    points, skip, num_matches; the final occupancy of cur; the neighbours' occupancy"""
    sf, ls = S.scale_tables()
    G, N = neighbours.shape
    idx = np.full((N, G, CAP), -1, np.int32); pos = np.zeros((N, G, CAP, 3)); st = np.zeros((N, G, CAP), np.uint8)
    skip = np.zeros((N, G), np.uint8); num = np.zeros((N, G), np.int32)
    occ_cur_out = np.zeros((G, CAP), np.uint8); occ_ngh_out = np.zeros((N, G, CAP), np.uint8)
    for g in range(G):
        k1 = sc["kfs"][cur[g]]
        n1 = len(k1["keypts"])
        occ1 = k1["occupied"].copy()
        order = np.argsort(k1["node"], kind="stable")           # the BoW node order of cur's key points
        for i in range(N):
            k2 = sc["kfs"][neighbours[g, i]]
            n2 = len(k2["keypts"])
            occ2 = k2["occupied"].copy()
            lm2 = k2["lm_pos_w"]
            med = KR_median(k2["pose"], lm2)
            s, epi, _ = KR.pair_geometry(sc["cam"], sc["setup_type"], S.TRUE_BASELINE, k1["pose"], k2["pose"], med)
            skip[i, g] = s
            if s:
                st[i, g, :n2] = KR.PAIR_SKIPPED
                occ_ngh_out[i, g, :n2] = occ2
                continue
            mono = sc["setup_type"] == KR.MONOCULAR
            q_xr = np.full(n1, -1, np.float32) if mono else k1["x_right"][order]
            t_xr = np.full(n2, -1, np.float32) if mono else k2["x_right"]
            has_lm = occ1 if carry else k1["occupied"]
            match_t = np.full(n1, -1, np.int32)
            if n1 and n2:
                match_t, num[i, g] = O.match_for_triangulation(
                    k1["desc"][order], k1["keypts"]["angle"][order], k1["node"][order], has_lm[order], q_xr, k1["keypts"]["octave"][order],
                    k1["bearings"][order], k2["desc"], k2["keypts"]["angle"], k2["node"], occ2, t_xr, k2["bearings"], sf, epi[:9], epi[9:], False)
            match_q = np.full(n2, -1, np.int32)
            sel = match_t >= 0
            match_q[match_t[sel]] = np.nonzero(sel)[0]
            o1 = occ1 if carry else occ1.copy()
            a, b, c = KR.triangulate_pair(sc["cam"], sc["setup_type"], S.TRUE_BASELINE, sf, ls, S.SCALE_FACTOR, 1.0, k1, k2, match_q, order, CAP,
                                          False, o1, occ2)
            idx[i, g, :n2], pos[i, g, :n2], st[i, g, :n2] = a, b, c
            occ_ngh_out[i, g, :n2] = occ2
        occ_cur_out[g, :n1] = occ1
    return dict(idx_1=idx, pos_w=pos, status=st, skip=skip, num_matches=num, occupied_cur=occ_cur_out, occupied_ngh=occ_ngh_out)


def KR_median(pose, lm_pos_w):
    from keyline_pairs_ref import median_depth
    return median_depth(pose, lm_pos_w, None, True)[0]


def run_step(sc, cur, neighbours):
    import torch
    F = sc["F"]
    t = S.table(sc)
    desc, node, occ = np.zeros((F, CAP, 32), np.uint8), np.zeros((F, CAP), np.int32), np.zeros((F, CAP), np.uint8)
    m = max(len(kf["lm_pos_w"]) for kf in sc["kfs"])
    lm, lv = np.zeros((F, m, 3)), np.zeros((F, m), np.uint8)
    for k, kf in enumerate(sc["kfs"]):
        n = len(kf["keypts"])
        desc[k, :n], node[k, :n], occ[k, :n] = kf["desc"], kf["node"], kf["occupied"]
        lm[k, :n], lv[k, :n] = kf["lm_pos_w"], 1
    # what lies past a key frame's count must not matter
    rng = np.random.default_rng(5)
    for k, kf in enumerate(sc["kfs"]):
        n = len(kf["keypts"])
        desc[k, n:], node[k, n:], occ[k, n:] = rng.integers(0, 256, (CAP - n, 32)), rng.integers(0, 12, CAP - n), 0
    table = dict(kps=_t(t["keypts"]), desc=_t(desc), node=_t(node), bearings=_t(t["bearings"]), counts=_t(t["counts"]), occupied=_t(occ),
                 pose=_t(t["pose"]), x_right=_t(t["x_right"]), depths=_t(t["depths"]), lm_pos_w=_t(lm), lm_valid=_t(lv))
    step = step_mod.create_landmarks_step(plp, _camera(sc["cam"]), setup_type=sc["setup_type"], true_baseline=S.TRUE_BASELINE,
                                          scale_factor=S.SCALE_FACTOR, num_levels=S.NUM_LEVELS)
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    out = step.run(table, _t(np.asarray(cur, np.int64)), _t(np.asarray(neighbours, np.int64)), stream=st)
    st.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


@pytest.mark.parametrize("setup,model", [(KR.MONOCULAR, "perspective"), (KR.MONOCULAR, "equirectangular"), (KR.RGBD, "fisheye"),
                                         (KR.STEREO, "perspective")])
def test_step_equals_the_host_chain(setup, model):
    sc = _scene(setup, model, 900 + 10 * setup + MODEL_ID[model])
    F = sc["F"]
    cur = np.arange(8)                                          # G = 8 current key frames
    neighbours = np.array([[(g + 1) % 10, (g + 2) % 10, (g + 4) % 10, F - 1 if g == 5 else (g + 7) % 10] for g in cur])   # N = 4, one empty
    assert (neighbours != cur[:, None]).all()
    want = host_chain(sc, cur, neighbours)
    got = run_step(sc, cur, neighbours)
    G, N = neighbours.shape
    assert np.array_equal(got["skip"], want["skip"]) and want["skip"].any() and not want["skip"].all()
    assert np.array_equal(got["num_matches"], want["num_matches"])
    made = 0
    for i in range(N):
        for g in range(G):
            n2 = len(sc["kfs"][neighbours[g, i]]["keypts"])
            made += int((want["status"][i, g, :n2] == KR.CREATED).sum())
            assert np.array_equal(got["status"][i, g, :n2], want["status"][i, g, :n2]), (i, g)
            assert np.array_equal(got["idx_1"][i, g, :n2], want["idx_1"][i, g, :n2]), (i, g)
            assert np.array_equal(_bits(got["pos_w"][i, g, :n2]), _bits(want["pos_w"][i, g, :n2])), (i, g)
            assert np.array_equal(got["occupied_ngh"][i, g, :n2], want["occupied_ngh"][i, g, :n2]), (i, g)
    assert made > 250, made
    for g in range(G):
        n1 = len(sc["kfs"][cur[g]]["keypts"])
        assert np.array_equal(got["occupied_cur"][g, :n1], want["occupied_cur"][g, :n1]), g
    # a key point that got a landmark at rank i is skipped by rank i + 1's matcher: without the carried occupancy it would be matched again
    free = host_chain(sc, cur, neighbours, carry=False)
    shown = 0
    for g in range(G):
        for i in range(N - 1):
            created = set(want["idx_1"][i, g][want["status"][i, g] == KR.CREATED].tolist())
            again = set(free["idx_1"][i + 1, g][free["idx_1"][i + 1, g] >= 0].tolist())
            now = set(want["idx_1"][i + 1, g][want["idx_1"][i + 1, g] >= 0].tolist())
            assert not (created & now), (g, i)
            shown += len(created & again)
    assert shown > 20, shown


def test_no_neighbour_or_no_key_frame():
    import torch
    sc = _scene(KR.MONOCULAR, "perspective", 77)
    t = S.table(sc)
    F = sc["F"]
    dev = torch.device("cuda", 0)
    table = dict(kps=_t(t["keypts"]), desc=torch.zeros((F, CAP, 32), dtype=torch.uint8, device=dev), node=torch.zeros((F, CAP), dtype=torch.int32, device=dev),
                 bearings=_t(t["bearings"]), counts=_t(t["counts"]), occupied=torch.zeros((F, CAP), dtype=torch.uint8, device=dev), pose=_t(t["pose"]),
                 lm_pos_w=torch.zeros((F, 1, 3), dtype=torch.float64, device=dev))
    step = step_mod.create_landmarks_step(plp, _camera(sc["cam"]))
    out = step.run(table, torch.arange(3, device=dev), torch.zeros((3, 0), dtype=torch.int64, device=dev))
    assert out["status"].shape == (0, 3, CAP) and out["occupied_cur"].shape == (3, CAP)
