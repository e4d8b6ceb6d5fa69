"""GPU parity of the key-frame pair point triangulation (plp_keyframe_pair_geometry_* / plp_triangulate_keypoint_pairs_*) against the CPU
restatement tests/keypoint_pairs_ref.py, bit for bit: scenes with ground truth for every setup and camera
(tests/keypoint_pairs_scene.py; that they reach every status and keep a gap in every comparison the device decides with its own cos /
atan2 / asin is asserted without a GPU in tests/test_keypoint_pairs_cpu.py), sentinel-filled outputs, ragged counts, a capacity that is
not a multiple of 64, empty key frames, P = 0, host entries against device entries, argument validation.  Every case here runs a capacity
of 80 slots, less than one workgroup of the triangulation kernel (256 slots of key frame 2); counts around and above a workgroup, the
packing layouts and the capacity limit of 8192 are in tests/test_gpu_pair_kernels_wide.py."""
import ctypes as C

import numpy as np
import pytest

import keypoint_pairs_ref as KR
import keypoint_pairs_scene as S
from plp import plp

pytestmark = pytest.mark.gpu
CAP = S.CAP
MODEL_ID = dict(perspective=0, fisheye=1, equirectangular=2)


def _camera(d):
    c = plp.camera_model_c()
    c.model, c.cols, c.rows = MODEL_ID[d["model"]], d["cols"], d["rows"]
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


def _case(si):
    setup, model = S.SETUPS[si]
    sc = S.make_scene(100 + si, setup, model)
    pairs = S.default_pairs(sc)
    mq, qf = S.make_matches(sc, pairs, 200 + si)
    return sc, pairs, mq, qf


def _occupancy(rng, Pn):
    """what the caller holds before the call: zeros, ones and other non-zero bytes, so that 'only where created' shows"""
    o = rng.choice(np.array([0, 0, 0, 1, 7], np.uint8), (Pn, CAP))
    return o.copy(), rng.permutation(o.ravel()).reshape(Pn, CAP).copy()


def _sentinels(Pn):
    return dict(idx_1=np.full((Pn, CAP), S.SENT_I32, np.int32), pos_w=np.full((Pn, CAP, 3), S.SENT_F64, np.float64),
                status=np.full((Pn, CAP), S.SENT_U8, np.uint8))


def _geometry_sentinels(Pn):
    return dict(skip=np.full(Pn, S.SENT_U8, np.uint8), epipolar=np.full((Pn, 12), S.SENT_F64, np.float64), baseline=np.full(Pn, S.SENT_F64, np.float64))


def geometry_device(mt, sc, pairs, t=None):
    torch, _ = _dev()
    t = S.table(sc) if t is None else t
    out = {k: _t(v) for k, v in _geometry_sentinels(len(pairs)).items()}
    mt.keyframe_pair_geometry_device(_camera(sc["cam"]), sc["setup_type"], sc["F"], len(pairs), _t(t["pose"]), _t(pairs), out["skip"], out["epipolar"],
                                     out["baseline"], median_depth=_t(t["median_depth"]), true_baseline=S.TRUE_BASELINE)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def pairs_device(mt, sc, pairs, mq, qf, skip, occ1, occ2, m_cap=CAP):
    torch, _ = _dev()
    t = S.table(sc)
    sf, ls = S.scale_tables()
    out = {k: _t(v) for k, v in _sentinels(len(pairs)).items()}
    o1, o2 = (None if occ1 is None else _t(occ1)), (None if occ2 is None else _t(occ2))
    mt.triangulate_keypoint_pairs_device(
        _camera(sc["cam"]), sc["setup_type"], sc["F"], CAP, m_cap, len(pairs), _t(t["keypts"]), _t(t["bearings"]), _t(t["pose"]), _t(pairs), _t(mq),
        out["idx_1"], out["pos_w"], out["status"], sf, ls, x_right=_t(t["x_right"]), depths=_t(t["depths"]), counts=_t(t["counts"]),
        q_feature=None if qf is None else _t(qf), pair_skip=None if skip is None else _t(skip), occupied_1_io=o1, occupied_2_io=o2,
        true_baseline=S.TRUE_BASELINE, scale_factor=S.SCALE_FACTOR)
    torch.cuda.synchronize()
    r = {k: v.cpu().numpy() for k, v in out.items()}
    r["occupied_1"], r["occupied_2"] = (None if o1 is None else o1.cpu().numpy()), (None if o2 is None else o2.cpu().numpy())
    return r


def pairs_host(mt, sc, pairs, mq, qf, skip, occ1, occ2, m_cap=None):
    t = S.table(sc)
    sf, ls = S.scale_tables()
    o1, o2 = (None if occ1 is None else occ1.copy()), (None if occ2 is None else occ2.copy())
    return mt.triangulate_keypoint_pairs(_camera(sc["cam"]), sc["setup_type"], t["keypts"], t["bearings"], t["pose"], pairs, mq, sf, ls,
                                         x_right=t["x_right"], depths=t["depths"], counts=t["counts"], q_feature=qf, m_cap=m_cap, pair_skip=skip,
                                         occupied_1=o1, occupied_2=o2, true_baseline=S.TRUE_BASELINE, scale_factor=S.SCALE_FACTOR,
                                         out=_sentinels(len(pairs)))


def expect_occupancy(sc, pairs, idx, st, occ1, occ2):
    """occupied_*_io after the call: the caller's bytes, 1 at idx_1 / t of every created landmark"""
    e1, e2 = occ1.copy(), occ2.copy()
    for p in range(len(pairs)):
        for t in np.nonzero(st[p] == KR.CREATED)[0]:
            e1[p, idx[p, t]] = 1
            e2[p, t] = 1
    return e1, e2


def check(got, want, e1, e2, what):
    idx, pos, st = want[:3]
    assert np.array_equal(got["status"], st), (what, np.argwhere(got["status"] != st)[:5])
    assert np.array_equal(got["idx_1"], idx), (what, np.argwhere(got["idx_1"] != idx)[:5])
    assert np.array_equal(_bits(got["pos_w"]), _bits(pos)), (what, np.argwhere(_bits(got["pos_w"]) != _bits(pos))[:5])
    if e1 is not None:
        assert np.array_equal(got["occupied_1"], e1) and np.array_equal(got["occupied_2"], e2), what


@pytest.mark.parametrize("si", range(len(S.SETUPS)))
def test_geometry_and_triangulation_equal_the_restatement_bit_for_bit(si):
    sc, pairs, mq, qf = _case(si)
    mt = plp.matcher()
    # geometry: device, then host
    skip, epi, base = S.reference_geometry(sc, pairs)
    g = geometry_device(mt, sc, pairs)
    assert np.array_equal(g["skip"], skip)
    assert np.array_equal(_bits(g["epipolar"]), _bits(epi)), np.argwhere(_bits(g["epipolar"]) != _bits(epi))[:5]
    assert np.array_equal(_bits(g["baseline"]), _bits(base))
    t = S.table(sc)
    h = mt.keyframe_pair_geometry(_camera(sc["cam"]), sc["setup_type"], t["pose"], pairs, median_depth=t["median_depth"],
                                  true_baseline=S.TRUE_BASELINE, out=_geometry_sentinels(len(pairs)))
    assert np.array_equal(h["skip"], skip) and np.array_equal(_bits(h["epipolar"]), _bits(epi)) and np.array_equal(_bits(h["baseline"]), _bits(base))
    # triangulation with the geometry's skip flags and a caller's occupancy
    rng = np.random.default_rng(si)
    occ1, occ2 = _occupancy(rng, len(pairs))
    want = S.reference_pairs(sc, pairs, mq, qf, skip)
    e1, e2 = expect_occupancy(sc, pairs, want[0], want[2], occ1, occ2)
    assert (want[2] == KR.CREATED).sum() > 250 and (want[2] == KR.PAIR_SKIPPED).any() and (want[2] == S.SENT_U8).any()
    check(pairs_device(mt, sc, pairs, mq, qf, g["skip"], occ1, occ2), want, e1, e2, "device")
    check(pairs_host(mt, sc, pairs, mq, qf, skip, occ1, occ2), want, e1, e2, "host")


def test_without_skip_flags_occupancy_and_query_order():
    """pair_skip, occupied_*_io and q_feature are optional: NULL = no pair skipped, nothing marked, query slot = key point"""
    sc, pairs, mq, qf = _case(3)
    mt = plp.matcher()
    direct = np.full_like(mq, -1)                               # the same matches with the key-point index in place of the query slot
    for p in range(len(pairs)):
        n2 = len(sc["kfs"][pairs[p][1]]["keypts"])
        for t in range(n2):
            direct[p, t] = qf[p, mq[p, t]] if 0 <= mq[p, t] < CAP else -1
    want = S.reference_pairs(sc, pairs, direct, None, None)
    assert (want[2] == KR.INDEX_RANGE).any() and not (want[2] == KR.PAIR_SKIPPED).any()
    direct_full = direct.copy()
    check(pairs_device(mt, sc, pairs, direct_full, None, None, None, None), want, None, None, "device")
    check(pairs_host(mt, sc, pairs, direct_full, None, None, None, None), want, None, None, "host")
    # a smaller m_cap turns the query slots at and above it into NO_MATCH
    m_cap = 40
    want = list(S.reference_pairs(sc, pairs, mq, qf[:, :m_cap], None))
    assert (want[2] == KR.NO_MATCH).sum() > (S.reference_pairs(sc, pairs, mq, qf, None)[2] == KR.NO_MATCH).sum()
    check(pairs_device(mt, sc, pairs, mq, np.ascontiguousarray(qf[:, :m_cap]), None, None, None, m_cap=m_cap), want, None, None, "device m_cap")
    check(pairs_host(mt, sc, pairs, mq, np.ascontiguousarray(qf[:, :m_cap]), None, None, None, m_cap=m_cap), want, None, None, "host m_cap")


def test_more_pairs_than_one_launch_holds():
    """the pair index runs along y (65 535 at most per launch): 70 000 copies of one pair all equal the first"""
    torch, _ = _dev()
    sc, pairs, mq, qf = _case(0)
    Pn = 70000
    small = np.tile(pairs[:1], (Pn, 1))
    mt = plp.matcher()
    t = S.table(sc)
    sf, ls = S.scale_tables()
    mqs, qfs = _t(np.tile(mq[:1], (Pn, 1))), _t(np.tile(qf[:1], (Pn, 1)))
    out = dict(idx_1=torch.full((Pn, CAP), S.SENT_I32, dtype=torch.int32, device=mqs.device),
               pos_w=torch.full((Pn, CAP, 3), S.SENT_F64, dtype=torch.float64, device=mqs.device),
               status=torch.full((Pn, CAP), S.SENT_U8, dtype=torch.uint8, device=mqs.device))
    mt.triangulate_keypoint_pairs_device(_camera(sc["cam"]), sc["setup_type"], sc["F"], CAP, CAP, Pn, _t(t["keypts"]), _t(t["bearings"]), _t(t["pose"]),
                                         _t(small), mqs, out["idx_1"], out["pos_w"], out["status"], sf, ls, counts=_t(t["counts"]), q_feature=qfs,
                                         scale_factor=S.SCALE_FACTOR)
    torch.cuda.synchronize()
    want = S.reference_pairs(sc, pairs[:1], mq[:1], qf[:1], None)
    for k, w in (("idx_1", want[0]), ("pos_w", want[1]), ("status", want[2])):
        g = out[k].cpu().numpy()
        assert np.array_equal(g[0].view(np.uint8), w[0].view(np.uint8)), k
        assert (g.reshape(Pn, -1).view(np.uint8) == g[0].reshape(1, -1).view(np.uint8)).all(), k


def test_nothing_to_do_writes_nothing():
    sc, pairs, mq, qf = _case(0)
    mt = plp.matcher()
    t = S.table(sc)
    sf, ls = S.scale_tables()
    cam = _camera(sc["cam"])
    # P = 0
    r = mt.triangulate_keypoint_pairs(cam, 0, t["keypts"], t["bearings"], t["pose"], np.zeros((0, 2), np.int32), np.zeros((0, CAP), np.int32), sf, ls)
    assert r["status"].shape == (0, CAP)
    g = mt.keyframe_pair_geometry(cam, 0, t["pose"], np.zeros((0, 2), np.int32), median_depth=t["median_depth"])
    assert g["skip"].shape == (0,)
    # cap = 0
    r = mt.triangulate_keypoint_pairs(cam, 0, np.zeros((sc["F"], 0), plp.KP_DTYPE), np.zeros((sc["F"], 0, 3)), t["pose"], pairs,
                                      np.zeros((len(pairs), 0), np.int32), sf, ls, m_cap=4)
    assert r["status"].shape == (len(pairs), 0)
    # only empty key frames on the kf2 side: every output keeps its sentinel
    F = sc["F"]
    empty = np.array([(0, F - 1), (1, F - 1)], np.int32)
    got = pairs_device(mt, sc, empty, mq[:2], qf[:2], None, None, None)
    for k, v in _sentinels(2).items():
        assert np.array_equal(got[k].view(np.uint8), v.view(np.uint8)), k
    # a pair outside the table is a precondition of the device entry: it is left unwritten, the others are not
    torch, _ = _dev()
    odd = pairs.copy()
    odd[1] = (0, F + 3)
    odd[2] = (-1, 0)
    got = pairs_device(mt, sc, odd, mq, qf, None, None, None)
    want = S.reference_pairs(sc, pairs, mq, qf, None)
    for p in range(len(pairs)):
        for k, w in (("idx_1", want[0]), ("pos_w", want[1]), ("status", want[2])):
            ref = _sentinels(1)[k][0] if p in (1, 2) else w[p]
            assert np.array_equal(got[k][p].view(np.uint8), ref.view(np.uint8)), (p, k)
    gd = geometry_device(mt, sc, odd)
    assert gd["skip"][1] == S.SENT_U8 and gd["skip"][2] == S.SENT_U8 and gd["skip"][0] != S.SENT_U8
    assert (gd["epipolar"][1] == S.SENT_F64).all() and gd["baseline"][2] == S.SENT_F64


def _geom_args(mt, sc, pairs, over=None):
    t = S.table(sc)
    keep = dict(pose=t["pose"], median=t["median_depth"], pairs=np.ascontiguousarray(pairs, np.int32), skip=np.zeros(len(pairs), np.uint8),
                epi=np.zeros((len(pairs), 12)), base=np.zeros(len(pairs)))
    a = plp.pair_geometry_args_c()
    a.camera = plp.camera_model_c.from_buffer_copy(_camera(sc["cam"]))
    a.setup_type, a.true_baseline, a.F, a.P = sc["setup_type"], S.TRUE_BASELINE, sc["F"], len(pairs)
    a.pose, a.median_depth, a.pairs = keep["pose"].ctypes.data, keep["median"].ctypes.data, keep["pairs"].ctypes.data
    a.out_skip, a.out_epipolar, a.out_baseline = keep["skip"].ctypes.data, keep["epi"].ctypes.data, keep["base"].ctypes.data
    for k, v in (over or {}).items():
        setattr(a, k, v)
    return a, keep


def _pairs_args(mt, sc, pairs, mq, qf, over=None):
    t = S.table(sc)
    sf, ls = S.scale_tables()
    Pn = len(pairs)
    keep = dict(t=t, sf=sf, ls=ls, pairs=np.ascontiguousarray(pairs, np.int32), mq=mq, qf=qf, **_sentinels(Pn))
    a = plp.keypoint_pairs_args_c()
    a.camera = plp.camera_model_c.from_buffer_copy(_camera(sc["cam"]))
    a.setup_type, a.true_baseline, a.num_levels, a.scale_factor, a.rays_parallax_deg_thr = sc["setup_type"], S.TRUE_BASELINE, len(sf), S.SCALE_FACTOR, 1.0
    a.scale_factors, a.level_sigma_sq = sf.ctypes.data, ls.ctypes.data
    a.F, a.cap, a.m_cap, a.P = sc["F"], CAP, CAP, Pn
    a.keypts, a.bearings, a.x_right, a.depths = t["keypts"].ctypes.data, t["bearings"].ctypes.data, t["x_right"].ctypes.data, t["depths"].ctypes.data
    a.counts, a.pose, a.pairs, a.match_q, a.q_feature = t["counts"].ctypes.data, t["pose"].ctypes.data, keep["pairs"].ctypes.data, mq.ctypes.data, qf.ctypes.data
    a.out_idx_1, a.out_pos_w, a.out_status = keep["idx_1"].ctypes.data, keep["pos_w"].ctypes.data, keep["status"].ctypes.data
    for k, v in (over or {}).items():
        setattr(a, k, v)
    return a, keep


def test_invalid_arguments_are_refused_before_anything_is_written():
    sc, pairs, mq, qf = _case(3)                                # RGB-D, perspective
    mt = plp.matcher()
    L = plp.lib()
    INV, UNS = plp.PLP_ERR_INVALID_ARG, plp.PLP_ERR_UNSUPPORTED
    equi = plp.camera_model_c.from_buffer_copy(_camera(S.CAMS["equirectangular"]))
    nofx = plp.camera_model_c.from_buffer_copy(_camera(S.CAMS["perspective"])); nofx.fx = 0.0
    unknown = plp.camera_model_c.from_buffer_copy(_camera(S.CAMS["perspective"])); unknown.model = 9
    outside = pairs.copy(); outside[3] = (0, sc["F"])

    cases = [(dict(setup_type=3), INV), (dict(setup_type=-1), INV), (dict(F=0), INV), (dict(P=-1), INV), (dict(pose=None), INV),
             (dict(pairs=None), INV), (dict(out_skip=None), INV), (dict(out_epipolar=None), INV), (dict(out_baseline=None), INV),
             (dict(camera=nofx), INV), (dict(camera=unknown), INV), (dict(setup_type=0, median_depth=None), INV)]
    for over, want in cases:
        a, keep = _geom_args(mt, sc, pairs, over)
        for fn, extra in ((L.plp_keyframe_pair_geometry_host, ()), (L.plp_keyframe_pair_geometry_device, (None,))):
            assert fn(mt._h, C.byref(a), *extra) == want, (over, fn)
        assert not keep["skip"].any() and not keep["epi"].any()
    a, keep = _geom_args(mt, sc, outside)
    assert L.plp_keyframe_pair_geometry_host(mt._h, C.byref(a)) == INV and not keep["epi"].any()
    assert L.plp_keyframe_pair_geometry_host(None, C.byref(a)) == INV and L.plp_keyframe_pair_geometry_host(mt._h, None) == INV
    a, keep = _geom_args(mt, sc, pairs, dict(median_depth=None))      # not read for RGB-D
    assert L.plp_keyframe_pair_geometry_host(mt._h, C.byref(a)) == plp.PLP_OK and keep["epi"].any()

    cases = [(dict(setup_type=3), INV), (dict(num_levels=0), INV), (dict(num_levels=17), INV), (dict(F=0), INV), (dict(cap=-1), INV),
             (dict(m_cap=0), INV), (dict(P=-1), INV), (dict(scale_factors=None), INV), (dict(level_sigma_sq=None), INV), (dict(keypts=None), INV),
             (dict(bearings=None), INV), (dict(pose=None), INV), (dict(pairs=None), INV), (dict(match_q=None), INV), (dict(out_idx_1=None), INV),
             (dict(out_pos_w=None), INV), (dict(out_status=None), INV), (dict(x_right=None), INV), (dict(depths=None), INV),
             (dict(camera=nofx), INV), (dict(camera=unknown), INV), (dict(camera=equi), UNS), (dict(cap=8193), UNS)]
    for over, want in cases:
        a, keep = _pairs_args(mt, sc, pairs, mq, qf, over)
        for fn, extra in ((L.plp_triangulate_keypoint_pairs_host, ()), (L.plp_triangulate_keypoint_pairs_device, (None,))):
            assert fn(mt._h, C.byref(a), *extra) == want, (over, fn)
        for k, v in _sentinels(len(pairs)).items():
            assert np.array_equal(keep[k].view(np.uint8), v.view(np.uint8)), (over, k)
    a, keep = _pairs_args(mt, sc, outside, mq, qf)
    assert L.plp_triangulate_keypoint_pairs_host(mt._h, C.byref(a)) == INV and (keep["status"] == S.SENT_U8).all()
    assert L.plp_triangulate_keypoint_pairs_host(None, C.byref(a)) == INV and L.plp_triangulate_keypoint_pairs_host(mt._h, None) == INV
    # monocular: x_right and depths are not read and may be NULL; the equirectangular camera is accepted
    a, keep = _pairs_args(mt, sc, pairs, mq, qf, dict(setup_type=0, x_right=None, depths=None))
    assert L.plp_triangulate_keypoint_pairs_host(mt._h, C.byref(a)) == plp.PLP_OK and (keep["status"] != S.SENT_U8).any()
    a, keep = _pairs_args(mt, sc, pairs, mq, qf, dict(setup_type=0, camera=equi))
    assert L.plp_triangulate_keypoint_pairs_host(mt._h, C.byref(a)) == plp.PLP_OK
