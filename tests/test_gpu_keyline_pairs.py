"""GPU parity of the key-frame pair line triangulation (plp_median_depth_* / plp_triangulate_keyline_pairs_*) against the CPU restatement
tests/keyline_pairs_ref.py: scenes with ground truth (tests/keyline_pairs_scene.py; that they reach every status
and hold no near tie of the parallax comparisons is asserted without a GPU in tests/test_keyline_pairs_cpu.py), batched groups with
sentinel-filled outputs, directed cases, chained calls, host entries against device entries, argument validation, the median depth.  The
triangulation cases here run a capacity of 64 query slots, less than one workgroup (256) of the geometry kernel and one trip of the resolve
kernel's loops; more than one, duplicates across trips and the capacity limit of 8192 are in tests/test_gpu_pair_kernels_wide.py."""
import ctypes as C

import numpy as np
import pytest

import keyline_pairs_ref as KP
import keyline_pairs_scene as S
from plp import plp

pytestmark = pytest.mark.gpu
CAP = S.CAP


def _camera(d=S.CAM, model=None):
    c = plp.camera_model_c()
    c.model, c.cols, c.rows = plp.CAMERA_PERSPECTIVE if model is None else model, d["cols"], d["rows"]
    for k in ("fx", "fy", "cx", "cy", "focal_x_baseline"):
        setattr(c, k, float(d[k]))
    return c


def _dev():
    import torch
    return torch, torch.device("cuda", 0)


def _t(a):
    torch, dev = _dev()
    a = np.ascontiguousarray(a)
    if a.dtype.fields is not None:
        a = a.view(np.uint8)
    return torch.from_numpy(a).to(dev)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _pairs(groups):
    pairs = np.array([(k1, k2) for k1, ngh in groups for k2 in ngh], np.int32).reshape(-1, 2)
    offs = np.zeros(len(groups) + 1, np.int32)
    offs[1:] = np.cumsum([len(n) for _, n in groups])
    return pairs, offs


def _sentinels(P, G):
    return dict(match=np.full((P, CAP), S.SENT_I32, np.int32), pos_w=np.full((P, CAP, 6), S.SENT_F64, np.float64),
                status=np.full((P, CAP), S.SENT_U8, np.uint8), occupied_cur=np.full((G, CAP), S.SENT_U8, np.uint8))


def run_device(mt, scene, groups, matches, gates, occupied=None, median=None, lines_3d=None):
    """the _device entry on tensors, every output pre-filled with its sentinel -> (match, pos_w, status, occupied_cur) as numpy"""
    torch, dev = _dev()
    t = S.table(scene, occupied)
    ti, di = S.flat_matches(groups, matches)
    pairs, offs = _pairs(groups)
    sf, ls = S.scale_tables()
    d = {k: (None if v is None else _t(v)) for k, v in t.items()}
    if lines_3d is not None:
        d["lines_3d"] = lines_3d
    out = {k: _t(v) for k, v in _sentinels(len(pairs), len(groups)).items()}
    mt.triangulate_keyline_pairs_device(
        _camera(), scene["setup_type"], scene["F"], CAP, len(pairs), len(groups), _t(pairs), _t(offs), _t(ti), _t(di), d["keylines"],
        d["line_functions"], d["kl_x_right"], d["pose"], d["median_depth"] if median is None else median, d["occupied"], out["match"], out["pos_w"],
        out["status"], out["occupied_cur"], sf, ls, counts=d["counts"], kp_depths=d["kp_depths"], kp_counts=d["kp_counts"],
        kp_cap=t["kp_depths"].shape[1], lines_3d=d["lines_3d"], true_baseline=S.TRUE_BASELINE, scale_factor=S.SCALE_FACTOR, **gates)
    torch.cuda.synchronize()
    return tuple(out[k].cpu().numpy() for k in ("match", "pos_w", "status", "occupied_cur"))


def run_host(mt, scene, groups, matches, gates, occupied=None, **kw):
    t = S.table(scene, occupied)
    ti, di = (None, None) if matches is None else S.flat_matches(groups, matches)
    sf, ls = S.scale_tables()
    P = sum(len(n) for _, n in groups)
    r = mt.triangulate_keyline_pairs(
        _camera(), scene["setup_type"], groups, t["keylines"], t["line_functions"], t["kl_x_right"], t["pose"], t["median_depth"], t["occupied"],
        sf, ls, counts=t["counts"], kp_depths=t["kp_depths"], kp_counts=t["kp_counts"], lines_3d=t["lines_3d"], lbd=t["lbd"], train_idx=ti, dist=di,
        true_baseline=S.TRUE_BASELINE, scale_factor=S.SCALE_FACTOR, out=_sentinels(P, len(groups)), **gates, **kw)
    return r


def assert_same(got, want, what=""):
    gm, gp, gs, go = got
    wm, wp, ws, wo = want
    assert np.array_equal(gs, ws), (what, "status", np.argwhere(gs != ws)[:5], gs[gs != ws][:5], ws[gs != ws][:5])
    assert np.array_equal(gm, wm), (what, "match")
    assert np.array_equal(go, wo), (what, "occupied_cur")
    assert np.array_equal(_bits(gp), _bits(wp)), (what, "pos_w", np.argwhere(_bits(gp) != _bits(wp))[:5])


def device_lines_3d(mt, scene):
    """lines_3d as the library builds them (matcher.keylines_3d); equal to the restatement's, which the scene holds"""
    if scene["setup_type"] == KP.MONOCULAR:
        return None
    t = S.table(scene)
    F = scene["F"]
    kw = {}
    if scene["setup_type"] == KP.RGBD:
        kd = np.full((F, CAP, 2), -1.0, np.float32)
        for k, kf in enumerate(scene["kfs"]):
            kd[k, :len(kf["kl_depths"])] = kf["kl_depths"]
        kw = dict(kl_depths=kd)
    else:
        klr, good = np.zeros((F, CAP), plp.KL_DTYPE), np.full((F, CAP), -1, np.int32)
        for k, kf in enumerate(scene["kfs"]):
            n = len(kf["keylines"])
            klr[k, :n], good[k, :n] = kf["keylines_right"], kf["good_match"]
        kw = dict(good_match=good, keylines_right=klr, counts_right=t["counts"])
    got = mt.keylines_3d(_camera(), scene["setup_type"], t["pose"], t["keylines"], counts=t["counts"], **kw)["pos_w"]
    for k, kf in enumerate(scene["kfs"]):
        n = len(kf["keylines"])
        assert np.array_equal(_bits(got[k, :n]), _bits(kf["lines_3d"])), k
    return got


# ------------------------------------------------------------------------------------------------------------ 1. scenes with ground truth
@pytest.mark.parametrize("name", [s[0] for s in S.SCENES])
def test_scene_parity(name):
    scene, groups, matches, gates, ref, _, _ = S.scene_case(name)
    mt = plp.matcher()
    l3 = device_lines_3d(mt, scene)
    got = run_device(mt, scene, groups, matches, gates, lines_3d=None if l3 is None else _t(l3))
    assert_same(got, ref, name)
    assert (ref[2] == KP.CREATED).sum() >= 100


def test_unperturbed_scene_parity():
    """the scenes of the accuracy test (tests/test_keyline_pairs_cpu.py: the restatement against ground truth): the device equals the restatement"""
    mt = plp.matcher()
    for seed, setup in ((41, KP.MONOCULAR), (42, KP.RGBD)):
        scene = S.make_scene(seed, setup, perturb=0.0, occupied_rate=0.0)
        groups = S.make_groups(seed, scene["F"])
        matches = S.match_all(scene, groups)
        assert_same(run_device(mt, scene, groups, matches, KP.INITIALIZER_GATES), S.run_ref(scene, groups, matches, KP.INITIALIZER_GATES), seed)


# ------------------------------------------------------------------------------------------------------------ 2. directed cases
def test_non_finite_and_kp_depth_range():
    mt = plp.matcher()
    scene = S.make_scene(31, KP.MONOCULAR, extra_horizontal=True)
    groups = [(0, [2, 4, 6])]
    matches = S.match_all(scene, groups)
    ref = S.run_ref(scene, groups, matches, KP.INITIALIZER_GATES)
    assert (ref[2] == KP.NON_FINITE).sum() >= 3
    assert_same(run_device(mt, scene, groups, matches, KP.INITIALIZER_GATES), ref, "horizontal")
    scene = S.make_scene(32, KP.RGBD)
    groups = [(4, [0, 2, 5]), (2, [4, 6])]
    matches = S.match_all(scene, groups)
    ref = S.run_ref(scene, groups, matches, KP.INITIALIZER_GATES)
    assert (ref[2] == KP.KP_DEPTH_RANGE).sum() >= 5
    assert_same(run_device(mt, scene, groups, matches, KP.INITIALIZER_GATES), ref, "few key points")


# ------------------------------------------------------------------------------------------------------------ 5. chaining
def test_one_group_equals_single_pair_calls_chained():
    scene, groups, matches, gates, ref, _, _ = S.scene_case("rgbd-mapping")
    mt = plp.matcher()
    g = max(range(len(groups)), key=lambda i: len(groups[i][1]) if len(scene["kfs"][groups[i][0]]["keylines"]) else 0)
    kf1, ngh = groups[g]
    whole = run_device(mt, scene, [groups[g]], [matches[g]], gates)
    occupied = [kf["occupied"].copy() for kf in scene["kfs"]]
    n = len(occupied[kf1])
    for k, kf2 in enumerate(ngh):
        one = run_device(mt, scene, [(kf1, [kf2])], [[matches[g][k]]], gates, occupied=occupied)
        assert np.array_equal(one[0][0], whole[0][k]) and np.array_equal(one[2][0], whole[2][k]) and np.array_equal(_bits(one[1][0]), _bits(whole[1][k]))
        occupied[kf1] = one[3][0][:n].copy()                    # out_occupied_cur -> occupied
    assert np.array_equal(one[3][0], whole[3][0])
    assert (whole[2] == KP.OCCUPIED_CUR).sum() > 0


# ------------------------------------------------------------------------------------------------------------ 6. host = device, validation
def test_host_equals_device_and_runs_the_1nn_itself():
    mt = plp.matcher()
    for name in ("stereo-mapping", "mono-init"):
        scene, groups, matches, gates, ref, _, _ = S.scene_case(name)
        r = run_host(mt, scene, groups, matches, gates)
        assert_same((r["match"], r["pos_w"], r["status"], r["occupied_cur"]), ref, name)
        # without train_idx the mirror runs the batched 1-NN on the device; the restatement gets what it returned
        r = run_host(mt, scene, groups, None, gates)
        ti, di = r["train_idx"], r["dist"]
        m2, p = [], 0
        for kf1, ngh in groups:
            n = len(scene["kfs"][kf1]["keylines"])
            m2.append([(ti[p + k, :n], di[p + k, :n]) for k in range(len(ngh))])
            p += len(ngh)
        bt, bd = S.flat_matches(groups, matches)
        for p_ in range(len(ti)):
            n = len(scene["kfs"][r["pairs"][p_][0]]["keylines"])
            assert np.array_equal(di[p_, :n], bd[p_, :n])      # the nearest distance is unique even where the nearest line is not
        assert_same((r["match"], r["pos_w"], r["status"], r["occupied_cur"]), S.run_ref(scene, groups, m2, gates), name + " 1-NN")


def _args(scene, groups, matches, gates, out):
    """a plp_keyline_pairs_args over host arrays (kept alive in the returned list)"""
    t = S.table(scene)
    ti, di = S.flat_matches(groups, matches)
    pairs, offs = _pairs(groups)
    sf, ls = S.scale_tables()
    a = plp.keyline_pairs_args_c()
    a.camera = _camera()
    a.setup_type, a.true_baseline, a.num_levels, a.scale_factor, a.rays_parallax_deg_thr = scene["setup_type"], S.TRUE_BASELINE, len(sf), S.SCALE_FACTOR, 1.0
    a.dist_thr, a.endpoint_thr, a.angle_thr, a.skip_occupied = gates["dist_thr"], gates["endpoint_thr"], gates["angle_thr"], gates["skip_occupied"]
    a.F, a.cap, a.kp_cap, a.P, a.G = scene["F"], CAP, t["kp_depths"].shape[1], len(pairs), len(groups)
    keep = [t, ti, di, pairs, offs, sf, ls, out]
    for k, v in dict(scale_factors=sf, level_sigma_sq=ls, keylines=t["keylines"], counts=t["counts"], line_functions=t["line_functions"],
                     kl_x_right=t["kl_x_right"], kp_depths=t["kp_depths"], kp_counts=t["kp_counts"], pose=t["pose"], median_depth=t["median_depth"],
                     lines_3d=t["lines_3d"], occupied=t["occupied"], pairs=pairs, group_offsets=offs, train_idx=ti, dist=di,
                     out_match=out["match"], out_pos_w=out["pos_w"], out_status=out["status"], out_occupied_cur=out["occupied_cur"]).items():
        setattr(a, k, None if v is None else v.ctypes.data)
    return a, keep, pairs


def test_argument_validation_writes_nothing():
    scene, groups, matches, gates, ref, _, _ = S.scene_case("rgbd-mapping")
    mt = plp.matcher()
    L = plp.lib()
    P, G = sum(len(n) for _, n in groups), len(groups)
    out = _sentinels(P, G)
    untouched = lambda: all(np.array_equal(out[k], v) for k, v in _sentinels(P, G).items())

    def status(**changes):
        a, keep, pairs = _args(scene, groups, matches, gates, out)
        for k, v in changes.items():
            if k == "camera_model":
                a.camera.model = v
            elif k == "mix":
                pairs[1, 0] = (pairs[0, 0] + 1) % scene["F"]
            elif k == "repeat":
                pairs[1, 1] = pairs[0, 1]
            elif k == "self":
                pairs[0, 1] = pairs[0, 0]
            else:
                setattr(a, k, v)
        st = L.plp_triangulate_keyline_pairs_host(mt._h, C.byref(a))
        assert untouched(), changes
        return st

    assert L.plp_triangulate_keyline_pairs_host(mt._h, None) == plp.PLP_ERR_INVALID_ARG
    assert L.plp_triangulate_keyline_pairs_host(None, None) == plp.PLP_ERR_INVALID_ARG
    for field in ("keylines", "line_functions", "kl_x_right", "pose", "median_depth", "occupied", "pairs", "group_offsets", "train_idx", "dist",
                  "out_match", "out_pos_w", "out_status", "out_occupied_cur", "scale_factors", "level_sigma_sq", "kp_depths", "lines_3d"):
        assert status(**{field: None}) == plp.PLP_ERR_INVALID_ARG, field
    assert status(camera_model=plp.CAMERA_FISHEYE) == plp.PLP_ERR_UNSUPPORTED
    assert status(cap=8193) == plp.PLP_ERR_UNSUPPORTED
    for bad in (dict(setup_type=3), dict(num_levels=0), dict(num_levels=17), dict(F=0), dict(cap=-1), dict(P=-1), dict(G=-1), dict(kp_cap=-1)):
        assert status(**bad) == plp.PLP_ERR_INVALID_ARG, bad
    for bad in ("mix", "repeat", "self"):                       # the _host path checks what is a precondition of _device
        assert status(**{bad: True}) == plp.PLP_ERR_INVALID_ARG, bad
    assert status(F=3) == plp.PLP_ERR_INVALID_ARG               # a key frame outside the table
    # nothing to do: PLP_OK and nothing written
    for empty in (dict(cap=0), dict(P=0), dict(G=0)):
        assert status(**empty) == plp.PLP_OK, empty
    # the median: NULL pointers, too many slots, nothing to do
    med, cnt = np.full(2, -1.0, np.float32), np.full(2, -7, np.int32)
    pose, pos = np.zeros((2, 15)), np.zeros((2, 4, 3))
    m = plp.median_depth_args_c()

    def mstatus(**kw):
        f = dict(F=2, m_cap=4, abs_flag=1, pose=pose.ctypes.data, pos_w=pos.ctypes.data, valid=None, counts=None, out_median=med.ctypes.data,
                 out_count=cnt.ctypes.data)
        f.update(kw)
        for k, v in f.items():
            setattr(m, k, v)
        st = L.plp_median_depth_host(mt._h, C.byref(m))
        return st

    for bad in (dict(pose=None), dict(pos_w=None), dict(out_median=None), dict(out_count=None), dict(F=0), dict(m_cap=-1)):
        assert mstatus(**bad) == plp.PLP_ERR_INVALID_ARG and (med == -1).all() and (cnt == -7).all(), bad
    assert mstatus(m_cap=8193) == plp.PLP_ERR_UNSUPPORTED and (med == -1).all() and (cnt == -7).all()
    assert mstatus(m_cap=0, pos_w=None) == plp.PLP_OK and (med == 0).all() and (cnt == 0).all()


# ------------------------------------------------------------------------------------------------------------ 7. median depth
def test_median_depth_64_key_frames():
    torch, dev = _dev()
    rng = np.random.default_rng(700)
    F, M = 64, 8192
    counts = rng.integers(0, M + 1, F).astype(np.int32)
    counts[:6] = (0, 1, 2, 3, M, M - 1)
    pose = np.stack([S.SK.frame_pose(S._rot(rng.normal(size=3) * 0.5), rng.normal(size=3) * 2) for _ in range(F)])
    pos = rng.normal(size=(F, M, 3)) * 6
    valid = (rng.random((F, M)) < 0.85).astype(np.uint8)
    valid[7] = 0                                                # every slot a nullptr
    for f in range(8, F, 3):                                    # duplicates of the median value: copy the landmark that holds it
        n = int(counts[f])
        idx = np.nonzero(valid[f, :n])[0]
        if len(idx) > 20:
            d = np.array([KP.depth_of(pose[f], pos[f, i], True) for i in idx])
            at = idx[np.argsort(d, kind="stable")[(len(idx) - 1) // 2]]
            pos[f, idx[:9]] = pos[f, at]
    mt = plp.matcher()
    for abs_flag in (True, False):
        want = [KP.median_depth(pose[f], pos[f, :counts[f]], valid[f, :counts[f]], abs_flag) for f in range(F)]
        wm, wc = np.array([w[0] for w in want], np.float32), np.array([w[1] for w in want], np.int32)
        gm, gc = mt.median_depth(pose, pos, valid, counts, abs_flag)
        assert np.array_equal(gc, wc) and np.array_equal(gm.view(np.uint32), wm.view(np.uint32)), (abs_flag, np.nonzero(gm != wm)[0][:5])
        dm = torch.full((F,), -1.0, dtype=torch.float32, device=dev)
        dc = torch.full((F,), -7, dtype=torch.int32, device=dev)
        mt.median_depth_device(F, M, _t(pose), _t(pos), dm, dc, valid=_t(valid), counts=_t(counts), abs_flag=abs_flag)
        torch.cuda.synchronize()
        assert np.array_equal(dm.cpu().numpy().view(np.uint32), wm.view(np.uint32)) and np.array_equal(dc.cpu().numpy(), wc)
    assert wc[0] == 0 and wc[7] == 0 and wm[7] == 0 and (wc[8:] > 0).all()
    # one key frame, no flags, no counts
    m1, c1 = mt.median_depth(pose[9], pos[9, :101])
    assert (m1, c1) == KP.median_depth(pose[9], pos[9, :101], None, True)


def test_device_median_feeds_the_triangulation():
    torch, dev = _dev()
    scene, groups, matches, gates, ref, _, _ = S.scene_case("mono-mapping")
    mt = plp.matcher()
    F = scene["F"]
    cloud = np.stack([kf["cloud"] for kf in scene["kfs"]])
    valid = np.stack([kf["cloud_valid"] for kf in scene["kfs"]])
    pose = np.stack([kf["pose"] for kf in scene["kfs"]])
    dm = torch.zeros(F, dtype=torch.float32, device=dev)
    dc = torch.zeros(F, dtype=torch.int32, device=dev)
    mt.median_depth_device(F, cloud.shape[1], _t(pose), _t(cloud), dm, dc, valid=_t(valid))     # the same stream: no synchronisation in between
    got = run_device(mt, scene, groups, matches, gates, median=dm)
    assert np.array_equal(dm.cpu().numpy(), np.array([kf["median_depth"] for kf in scene["kfs"]], np.float32))
    assert_same(got, ref, "device median")
