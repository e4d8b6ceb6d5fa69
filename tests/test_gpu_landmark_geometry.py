"""Landmark normals and valid distance ranges on the device (plp_landmark_geometry_* / plp_landmark_line_geometry_*, landmark_refresh_step) against
the CPU restatement tests/landmark_geometry_ref.py, bit for bit, on the scene of tests/landmark_geometry_scene.py:
ragged lists around one and several tiles of the kernel, one list over all 600 key frames, every status, sentinel-filled outputs.  That the
scene's lists can tell the reference's order of summation from another is asserted without a GPU in tests/test_landmark_geometry_cpu.py."""
import ctypes as C

import numpy as np
import pytest

import landmark_geometry_ref as G
import landmark_geometry_scene as S
import landmark_observe_ref as R
from plp import plp

pytestmark = pytest.mark.gpu
f32 = np.float32


@pytest.fixture(scope="module")
def mt():
    return plp.matcher()


def host(mt, sc, name, rows=None, out=None):
    t = sc[name]
    lines = name == "lines"
    pos, ref, skip, off, kf, idx = S.sublist(t, np.arange(t["L"]) if rows is None else rows)
    out = S.sentinels(len(pos), lines) if out is None else out
    if lines:
        return mt.landmark_line_geometry(sc["pose"], t["feats"], pos, ref, off, kf, idx, sc["scale_factors"], sc["scale_factors_lsd"], skip=skip,
                                         counts=t["counts"], out=out)
    return mt.landmark_geometry(sc["pose"], t["feats"], pos, ref, off, kf, idx, sc["scale_factors"], skip=skip, counts=t["counts"], out=out)


def assert_same(got, want, label=""):
    assert np.array_equal(got["status"], want["status"]), label
    for k in want:                                              # the values where UPDATED and the sentinels elsewhere, all bytes
        assert S.same_bits(got[k], want[k]), (label, k)


@pytest.mark.parametrize("name", ["points", "lines"])
def test_host_entry_equals_the_restatement(mt, name):
    sc = S.scene()
    want = S.want_points() if name == "points" else S.want_lines()
    assert_same(host(mt, sc, name), want, name)
    assert (want["status"] == G.UPDATED).sum() > 200 and (want["min_dist"] == S.SENT_F32).sum() > 20


def _dev(a, dtype=None):
    import torch
    a = np.ascontiguousarray(a) if dtype is None else np.ascontiguousarray(a, dtype)
    if a.dtype.fields is not None:                              # key points / key lines: bytes
        a = a.view(np.uint8).reshape(a.shape + (a.dtype.itemsize,))
    return torch.from_numpy(a.copy()).cuda()


@pytest.mark.parametrize("name", ["points", "lines"])
def test_device_entry_equals_the_restatement(mt, name):
    import torch
    sc = S.scene()
    t = sc[name]
    lines = name == "lines"
    want = S.want_points() if name == "points" else S.want_lines()
    o = {k: _dev(v) for k, v in S.sentinels(t["L"], lines).items()}
    args = [sc["F"], sc["cap"], t["L"], _dev(sc["pose"]), _dev(t["feats"]), _dev(t["pos_w"]), _dev(t["ref_kf"]), _dev(t["obs_offsets"]), _dev(t["obs_kf"]),
            _dev(t["obs_idx"])]
    kw = dict(skip=_dev(t["skip"]), counts=_dev(t["counts"]))
    if lines:
        mt.landmark_line_geometry_device(*args, o["min_dist"], o["max_dist"], o["status"], sc["scale_factors"], sc["scale_factors_lsd"], **kw)
    else:
        mt.landmark_geometry_device(*args, o["normal"], o["min_dist"], o["max_dist"], o["status"], sc["scale_factors"], **kw)
    torch.cuda.synchronize()
    assert_same({k: v.cpu().numpy() for k, v in o.items()}, want, name)


def test_rows_do_not_depend_on_where_a_run_starts(mt):
    """the same landmarks in two calls, cut where no workgroup's run of the whole call ends, and one landmark at a time around the long lists"""
    sc = S.scene()
    want = S.want_points()
    L = sc["points"]["L"]
    for rows in (np.arange(0, 301), np.arange(301, L), np.arange(1, 2), np.arange(250, 263)):
        got = host(mt, sc, "points", rows)
        assert_same(got, {k: v[rows] for k, v in want.items()}, (rows[0], rows[-1]))
    wl = S.want_lines()
    rows = np.arange(77, sc["lines"]["L"])
    assert_same(host(mt, sc, "lines", rows), {k: v[rows] for k, v in wl.items()})


def test_no_landmark_and_one_landmark(mt):
    sc = S.scene()
    t = sc["points"]
    got = mt.landmark_geometry(sc["pose"], t["feats"], np.zeros((0, 3)), [], [0], [], [], sc["scale_factors"])
    assert got["status"].shape == (0,) and got["normal"].shape == (0, 3)
    got = mt.landmark_line_geometry(sc["pose"], sc["lines"]["feats"], np.zeros((0, 6)), [], [0], [], [], sc["scale_factors"], sc["scale_factors_lsd"])
    assert got["status"].shape == (0,)
    pos = np.array([[0.5, -0.25, 9.0]])
    got = mt.landmark_geometry(sc["pose"], t["feats"], pos, [17], [0, 1], [17], [3], sc["scale_factors"])
    want = G.refresh(sc["pose"], t["feats"]["octave"], None, sc["scale_factors"], pos, [17], None, [0, 1], [17], [3])
    assert want["status"][0] == G.UPDATED
    assert_same(got, want)
    c = sc["pose"][17, 12:15]
    assert got["normal"][0].tolist() == list(G.normalized(*G.normalized(0.5 - c[0], -0.25 - c[1], 9.0 - c[2])))


def _raw_args(sc, name, o):
    """the args struct of a valid call on the first 40 landmarks, HOST pointers, and what keeps them alive"""
    t = sc[name]
    lines = name == "lines"
    pos, ref, skip, off, kf, idx = S.sublist(t, np.arange(40))
    keep = dict(pose=np.ascontiguousarray(sc["pose"]), feats=np.ascontiguousarray(t["feats"]), pos=np.ascontiguousarray(pos), ref=np.ascontiguousarray(ref),
                off=off, kf=np.ascontiguousarray(kf), idx=np.ascontiguousarray(idx), sf=sc["scale_factors"], sl=sc["scale_factors_lsd"],
                skip=np.ascontiguousarray(skip), counts=np.ascontiguousarray(t["counts"]))
    P = lambda v: v.ctypes.data
    a = plp.landmark_geometry_args_c()
    a.F, a.cap, a.L, a.num_levels, a.num_levels_lsd = sc["F"], sc["cap"], 40, len(keep["sf"]), len(keep["sl"])
    a.pose, a.scale_factors, a.scale_factors_lsd = P(keep["pose"]), P(keep["sf"]), P(keep["sl"])
    a.skip, a.counts = P(keep["skip"]), P(keep["counts"])
    a.keypts, a.keylines = (None, P(keep["feats"])) if lines else (P(keep["feats"]), None)
    a.pos_w, a.ref_kf, a.obs_offsets, a.obs_kf, a.obs_idx = P(keep["pos"]), P(keep["ref"]), P(keep["off"]), P(keep["kf"]), P(keep["idx"])
    a.out_mean_normal = None if lines else P(o["normal"])
    a.out_min_valid_dist, a.out_max_valid_dist, a.out_status = P(o["min_dist"]), P(o["max_dist"]), P(o["status"])
    return a, keep


@pytest.mark.parametrize("name", ["points", "lines"])
def test_bad_arguments_leave_the_outputs_untouched(mt, name):
    sc = S.scene()
    lines = name == "lines"
    L, INV = plp.lib(), plp.PLP_ERR_INVALID_ARG
    host_fn = L.plp_landmark_line_geometry_host if lines else L.plp_landmark_geometry_host
    dev_fn = L.plp_landmark_line_geometry_device if lines else L.plp_landmark_geometry_device
    o = S.sentinels(40, lines)
    untouched = lambda: all((v == s).all() for v, s in ((o["status"], S.SENT_U8), (o["min_dist"], S.SENT_F32), (o["max_dist"], S.SENT_F32))) and \
        (lines or (o["normal"] == S.SENT_F64).all())
    bad = [("F", 0), ("F", -1), ("cap", -1), ("L", -1), ("num_levels", 0), ("num_levels", 17), ("scale_factors", None), ("pose", None), ("pos_w", None),
           ("ref_kf", None), ("obs_offsets", None), ("obs_kf", None), ("obs_idx", None), ("out_min_valid_dist", None), ("out_max_valid_dist", None),
           ("out_status", None), ("keylines" if lines else "keypts", None)]
    bad += [("num_levels_lsd", 0), ("num_levels_lsd", 17), ("scale_factors_lsd", None)] if lines else [("out_mean_normal", None)]
    for field, value in bad:
        for fn, extra in ((host_fn, ()), (dev_fn, (None,))):   # the device entry refuses before it follows a pointer: host pointers are never read
            a, keep = _raw_args(sc, name, o)
            setattr(a, field, value)
            assert fn(mt._h, C.byref(a), *extra) == INV and untouched(), (field, value)
    a, keep = _raw_args(sc, name, o)
    assert host_fn(None, C.byref(a)) == INV and host_fn(mt._h, None) == INV and dev_fn(None, C.byref(a), None) == INV and dev_fn(mt._h, None, None) == INV
    if lines:                                                   # more LSD levels than ORB levels: the reference would read past scale_factors_
        a.num_levels = 1
        assert host_fn(mt._h, C.byref(a)) == INV and dev_fn(mt._h, C.byref(a), None) == INV and untouched()
    # the host entry reads the offsets: they start at 0 and do not decrease
    for at, value in ((0, 1), (7, -1)):
        a, keep = _raw_args(sc, name, o)
        keep["off"][at] = value
        assert host_fn(mt._h, C.byref(a)) == INV and untouched(), at
    # L == 0 is a valid call that writes nothing, whatever the pointers; and the unchanged struct is a valid call
    a, keep = _raw_args(sc, name, o)
    a.L, a.pos_w, a.out_status = 0, None, None
    assert host_fn(mt._h, C.byref(a)) == plp.PLP_OK and dev_fn(mt._h, C.byref(a), None) == plp.PLP_OK and untouched()
    a, keep = _raw_args(sc, name, o)
    assert host_fn(mt._h, C.byref(a)) == plp.PLP_OK and not untouched()
    want = S.want_points() if name == "points" else S.want_lines()
    assert_same(o, {k: v[:40] for k, v in want.items()})


# ---------------------------------------------------------------------------------------------------------------- the step
def _step_tables(sc):
    kf = dict(kps=_dev(sc["points"]["feats"]), desc=_dev(sc["points"]["desc"]), counts=_dev(sc["points"]["counts"]), pose=_dev(sc["pose"]),
              kl=_dev(sc["lines"]["feats"]), lbd=_dev(sc["lines"]["desc"]), kl_counts=_dev(sc["lines"]["counts"]), kf_erased=_dev(sc["kf_erased"]))
    lm = {}
    for name, sfx in (("points", ""), ("lines", "_lines")):
        t = sc[name]
        sent = S.sentinels(t["L"], name == "lines")
        lm.update({"pos_w" + sfx: _dev(t["pos_w"]), "ref_kf" + sfx: _dev(t["ref_kf"]), "skip" + sfx: _dev(t["skip"]), "obs_offsets" + sfx: _dev(t["obs_offsets"]),
                   "obs_kf" + sfx: _dev(t["obs_kf"]), "obs_idx" + sfx: _dev(t["obs_idx"]), "desc" + sfx: _dev(t["desc_lm"]),
                   "min_dist" + sfx: _dev(sent["min_dist"]), "max_dist" + sfx: _dev(sent["max_dist"])})
        if name == "points":
            lm["normal"] = _dev(sent["normal"])
    return kf, lm


def _want_descriptors(mt, sc, name):
    """landmark::compute_descriptor per landmark on the host entry: the rows of the key frames that stay, in list order -> (desc table, best row)"""
    t = sc[name]
    rows, off = [], [0]
    for l in range(t["L"]):
        for o in range(t["obs_offsets"][l], t["obs_offsets"][l + 1]):
            k, i = int(t["obs_kf"][o]), int(t["obs_idx"][o])
            if 0 <= k < sc["F"] and 0 <= i < sc["cap"] and not sc["kf_erased"][k]:
                rows.append(t["desc"][k, i])
        off.append(len(rows))
    rows = np.array(rows, np.uint8).reshape(-1, 32)
    best = mt.landmark_descriptors(rows, np.array(off, np.int32))
    want = t["desc_lm"].copy()
    for l in range(t["L"]):
        if best[l] >= 0 and not t["skip"][l]:
            want[l] = rows[off[l] + best[l]]
    return want, best, np.diff(off)


@pytest.fixture(scope="module")
def refreshed():
    import importlib
    import torch
    sc = S.scene()
    step_mod = importlib.import_module("structure-plp-slam_amd.landmark_refresh_step")
    step = step_mod.landmark_refresh_step(plp, num_levels=S.NUM_LEVELS, num_levels_lsd=S.NUM_LEVELS_LSD)
    kf, lm = _step_tables(sc)
    out = step.run(kf, lm)
    torch.cuda.synchronize()
    return sc, step, kf, lm, out


def test_refresh_step_equals_restatement_and_descriptor_entry(mt, refreshed):
    sc, step, kf, lm, out = refreshed
    assert np.array_equal(step.sf, sc["scale_factors"]) and np.array_equal(step.sf_lsd, sc["scale_factors_lsd"])
    for name, sfx, want in (("points", "", S.want_points()), ("lines", "_lines", S.want_lines())):
        got = {k: out[k + sfx].cpu().numpy() for k in want}
        assert_same(got, want, name)
        assert out["min_dist" + sfx] is lm["min_dist" + sfx] and out["desc" + sfx] is lm["desc" + sfx]       # the caller's tables, in place
        wd, best, kept = _want_descriptors(mt, sc, name)
        assert np.array_equal(out["best_idx" + sfx].cpu().numpy(), best), name
        assert np.array_equal(out["desc" + sfx].cpu().numpy(), wd), name
        t = sc[name]
        lens = np.diff(t["obs_offsets"])
        # erased key frames were left out of the vote of many landmarks, and the table changed where the reference changes it
        assert (kept < lens).sum() > 100 and (wd != t["desc_lm"]).any(axis=1).sum() > 150 and (best < 0).sum() > 20
    with pytest.raises(plp.PlpError):
        step.run({**kf, "pose": kf["pose"].new_zeros((1025, 15))}, lm)


def test_refreshed_tables_go_straight_into_observe(mt, refreshed):
    """normal / min_dist / max_dist as the step left them in HBM -> plp_observe_landmarks_device, against frame::can_observe restated on the restated
    tables"""
    import torch
    sc, step, kf, lm, out = refreshed
    want_t = S.want_points()
    cm = plp.camera_model({"Camera.model": "perspective", "Camera.cols": 640, "Camera.rows": 480, "Camera.fx": 535.4, "Camera.fy": 539.2, "Camera.cx": 320.1,
                           "Camera.cy": 247.6, "Camera.k1": 0.0, "Camera.k2": 0.0, "Camera.p1": 0.0, "Camera.p2": 0.0, "Camera.k3": 0.0,
                           "Camera.focal_x_baseline": 40.0})
    rc = {"model": "perspective", "cols": cm.cols, "rows": cm.rows, **{k: getattr(cm, k) for k in ("fx", "fy", "cx", "cy", "focal_x_baseline")}}
    t = sc["points"]
    L = t["L"]
    lsf = R.d5_logf(f32(1.2))
    skip = ((want_t["status"] != G.UPDATED) | (t["skip"] != 0)).astype(np.uint8)
    total = 0
    for f in (0, 311):
        P = sc["pose"][f]
        want = R.observe_points(rc, cm.img_bounds, P, t["pos_w"], want_t["normal"], want_t["min_dist"], want_t["max_dist"], skip, 0.5, lsf, S.NUM_LEVELS)
        reproj = torch.zeros((1, L, 2), dtype=torch.float32, device="cuda")
        level = torch.zeros((1, L), dtype=torch.int32, device="cuda")
        valid = torch.zeros((1, L), dtype=torch.uint8, device="cuda")
        mt.observe_landmarks_device(cm, 1, L, kf["pose"][f:f + 1].contiguous(), lm["pos_w"], reproj, valid, obs_mean_normal=out["normal"],
                                    min_valid_dist=out["min_dist"], max_valid_dist=out["max_dist"], skip=_dev(skip), out_level=level, log_scale_factor=lsf,
                                    num_levels=S.NUM_LEVELS)
        torch.cuda.synchronize()
        v = want["valid"].astype(bool)
        assert np.array_equal(valid.cpu().numpy()[0], want["valid"])
        assert np.array_equal(level.cpu().numpy()[0][v], want["level"][v])
        assert np.array_equal(reproj.cpu().numpy()[0][v].view(np.uint32), want["reproj"][v].view(np.uint32))
        total += int(v.sum())
    assert total > 300
