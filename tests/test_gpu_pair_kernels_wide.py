"""GPU parity of the pair-triangulation kernels above one workgroup of slots: k_triangulate_keypoint_pairs (256 slots of key frame 2 per
workgroup, the matched ones packed to the front), k_keyline_pair_geometry / k_keyline_pair_resolve (256 query slots per workgroup / per
trip of the resolve loops) and k_stereo_keylines / k_keylines_3d (256 key lines per workgroup), bit for bit against the CPU restatements.
The other GPU files of these entries run capacities of 64 to 96; here the capacities are 300, 520, 600 and 8192, the counts stand around
256 and 512, and directed layouts fill or empty whole workgroups and waves.  The scenes come from tests/keypoint_pairs_scene.py,
tests/keyline_pairs_scene.py and tests/stereo_keylines_wide.py; that each shows the edge it is named for, and keeps the gap of D8 / D10 in
every comparison the device decides with its own libm, is asserted without a GPU in tests/test_pair_kernels_wide_cpu.py.  Outputs are
sentinel-filled and compared whole, floats by their bits, the caller's occupancy bytes except where a landmark is created."""
import numpy as np
import pytest

import keyline_pairs_ref as KP
import keyline_pairs_scene as LS
import keypoint_pairs_ref as KR
import keypoint_pairs_scene as PS
import stereo_keylines_wide as SW
from plp import plp
from test_gpu_keyline_pairs import _camera as line_camera, _pairs as group_pairs, assert_same
from test_gpu_keypoint_pairs import _camera as point_camera, _dev, _t, check, expect_occupancy
from test_gpu_stereo_keylines import EUROC, _camera as stereo_camera, _check_3d

pytestmark = pytest.mark.gpu


# ================================================================================================================ key points
def _kp_sentinels(Pn, cap):
    return dict(idx_1=np.full((Pn, cap), PS.SENT_I32, np.int32), pos_w=np.full((Pn, cap, 3), PS.SENT_F64, np.float64),
                status=np.full((Pn, cap), PS.SENT_U8, np.uint8))


def _kp_occupancy(seed, Pn, cap):
    """what the caller holds before the call: zeros, ones and other non-zero bytes, so that 'only where created' shows"""
    rng = np.random.default_rng(seed)
    o = rng.choice(np.array([0, 0, 0, 1, 7], np.uint8), (Pn, cap))
    return o.copy(), rng.permutation(o.ravel()).reshape(Pn, cap).copy()


def kp_device(mt, sc, pairs, mq, qf, skip, occ1, occ2, cap):
    torch, _ = _dev()
    t = PS.table(sc, cap)
    sf, ls = PS.scale_tables()
    out = {k: _t(v) for k, v in _kp_sentinels(len(pairs), cap).items()}
    o1, o2 = _t(occ1), _t(occ2)
    mt.triangulate_keypoint_pairs_device(
        point_camera(sc["cam"]), sc["setup_type"], sc["F"], cap, cap, len(pairs), _t(t["keypts"]), _t(t["bearings"]), _t(t["pose"]), _t(pairs),
        _t(mq), out["idx_1"], out["pos_w"], out["status"], sf, ls, x_right=_t(t["x_right"]), depths=_t(t["depths"]), counts=_t(t["counts"]),
        q_feature=None if qf is None else _t(qf), pair_skip=None if skip is None else _t(skip), occupied_1_io=o1, occupied_2_io=o2,
        true_baseline=PS.TRUE_BASELINE, scale_factor=PS.SCALE_FACTOR)
    torch.cuda.synchronize()
    r = {k: v.cpu().numpy() for k, v in out.items()}
    r["occupied_1"], r["occupied_2"] = o1.cpu().numpy(), o2.cpu().numpy()
    return r


def kp_host(mt, sc, pairs, mq, qf, skip, occ1, occ2, cap):
    t = PS.table(sc, cap)
    sf, ls = PS.scale_tables()
    return mt.triangulate_keypoint_pairs(point_camera(sc["cam"]), sc["setup_type"], t["keypts"], t["bearings"], t["pose"], pairs, mq, sf, ls,
                                         x_right=t["x_right"], depths=t["depths"], counts=t["counts"], q_feature=qf, m_cap=cap, pair_skip=skip,
                                         occupied_1=occ1.copy(), occupied_2=occ2.copy(), true_baseline=PS.TRUE_BASELINE,
                                         scale_factor=PS.SCALE_FACTOR, out=_kp_sentinels(len(pairs), cap))


def _kp_expect(sc, pairs, want, seed, cap):
    occ1, occ2 = _kp_occupancy(seed, len(pairs), cap)
    e1, e2 = expect_occupancy(sc, pairs, want[0], want[2], occ1, occ2)
    return occ1, occ2, e1, e2


@pytest.mark.parametrize("permuted", [True, False], ids=["q_feature", "no-q_feature"])
@pytest.mark.parametrize("wi", range(len(PS.WIDE_SETUPS)), ids=[f"{('mono', 'stereo', 'rgbd')[s]}-{m}" for s, m in PS.WIDE_SETUPS])
def test_k1_keypoint_counts_around_the_workgroup(wi, permuted):
    """cap 520, key frame 1 full, key frame 2 with 255 .. 513 key points, six pairs in one call: workgroups 1 and 2 (t0 = 256, 512), the early
    return of a workgroup at or above the count, waves 2 and 3 in the packing, idx_1 at and above 256"""
    sc, pairs, mq, qf = PS.wide_counts_case(wi)
    if not permuted:
        mq, qf = PS.direct_matches(sc, pairs, mq, qf), None
    want = PS.wide_reference("counts", wi, permuted)["ref"]
    occ1, occ2, e1, e2 = _kp_expect(sc, pairs, want, 10 + wi, PS.WIDE_CAP)
    check(kp_device(plp.matcher(), sc, pairs, mq, qf, None, occ1, occ2, PS.WIDE_CAP), want, e1, e2, f"device {wi} {permuted}")


def test_k2_k4_packing_layouts_and_a_skipped_pair():
    """cap 520, both key frames full: a workgroup with all 256 slots matched beside one with none, matches in the last wave only, one match
    per wave at lane 0 and at lane 63, matches at slots 255 / 256 / 519 only, no match at all; then a skipped pair over three workgroups
    (one status per slot, idx_1 and pos_w untouched) beside the same pair computed"""
    sc, pairs, mq, qf, skip = PS.wide_layout_case()
    want = PS.wide_reference("layout")["ref"]
    n = len(PS.WIDE_LAYOUTS)
    assert (want[2][n] == KR.PAIR_SKIPPED).all() and (want[0][n] == PS.SENT_I32).all() and (want[1][n] == PS.SENT_F64).all()
    assert (want[2][n + 1] == KR.CREATED).sum() > 400
    occ1, occ2, e1, e2 = _kp_expect(sc, pairs, want, 20, PS.WIDE_CAP)
    mt = plp.matcher()
    check(kp_device(mt, sc, pairs, mq, qf, skip, occ1, occ2, PS.WIDE_CAP), want, e1, e2, "device")
    check(kp_host(mt, sc, pairs, mq, qf, skip, occ1, occ2, PS.WIDE_CAP), want, e1, e2, "host")


def test_k3_keypoints_at_the_capacity_limit():
    """cap = m_cap = 8192: 32 workgroups per pair, slot 8191 with key point 7999, slot 0 with key point 7998, INDEX_RANGE at key point 8000,
    NO_MATCH at query m_cap, an empty key frame 2 and one with 8000 of 8192 slots; the occupancy arrays whole"""
    sc, pairs, mq, qf, planted = PS.limit_case()
    want = PS.wide_reference("limit")["ref"]
    for p, t, j in planted["created"]:
        assert want[2][p, t] == KR.CREATED and want[0][p, t] == j
    occ1, occ2, e1, e2 = _kp_expect(sc, pairs, want, 30, PS.LIMIT_CAP)
    assert e1[0, 7999] == 1 and e2[0, 8191] == 1
    mt = plp.matcher()
    check(kp_device(mt, sc, pairs, mq, qf, None, occ1, occ2, PS.LIMIT_CAP), want, e1, e2, "device")
    check(kp_host(mt, sc, pairs, mq, qf, None, occ1, occ2, PS.LIMIT_CAP), want, e1, e2, "host")


def test_k5_keypoint_host_entry_at_the_wide_counts():
    sc, pairs, mq, qf = PS.wide_counts_case(0)
    want = PS.wide_reference("counts", 0, True)["ref"]
    occ1, occ2, e1, e2 = _kp_expect(sc, pairs, want, 40, PS.WIDE_CAP)
    check(kp_host(plp.matcher(), sc, pairs, mq, qf, None, occ1, occ2, PS.WIDE_CAP), want, e1, e2, "host")


# ================================================================================================================ key lines
def _kl_sentinels(P, G, cap):
    return dict(match=np.full((P, cap), LS.SENT_I32, np.int32), pos_w=np.full((P, cap, 6), LS.SENT_F64, np.float64),
                status=np.full((P, cap), LS.SENT_U8, np.uint8), occupied_cur=np.full((G, cap), LS.SENT_U8, np.uint8))


def kl_device(mt, scene, groups, matches, gates, cap, occupied=None):
    """the _device entry on tensors, every output pre-filled with its sentinel -> (match, pos_w, status, occupied_cur) as numpy"""
    torch, _ = _dev()
    t = LS.table(scene, occupied, cap)
    ti, di = LS.flat_matches(groups, matches, cap)
    pairs, offs = group_pairs(groups)
    sf, ls = LS.scale_tables()
    d = {k: (None if v is None else _t(v)) for k, v in t.items()}
    out = {k: _t(v) for k, v in _kl_sentinels(len(pairs), len(groups), cap).items()}
    mt.triangulate_keyline_pairs_device(
        line_camera(), scene["setup_type"], scene["F"], cap, len(pairs), len(groups), _t(pairs), _t(offs), _t(ti), _t(di), d["keylines"],
        d["line_functions"], d["kl_x_right"], d["pose"], d["median_depth"], d["occupied"], out["match"], out["pos_w"], out["status"],
        out["occupied_cur"], sf, ls, counts=d["counts"], kp_depths=d["kp_depths"], kp_counts=d["kp_counts"], kp_cap=t["kp_depths"].shape[1],
        lines_3d=d["lines_3d"], true_baseline=LS.TRUE_BASELINE, scale_factor=LS.SCALE_FACTOR, **gates)
    torch.cuda.synchronize()
    return tuple(out[k].cpu().numpy() for k in ("match", "pos_w", "status", "occupied_cur"))


def kl_host(mt, scene, groups, matches, gates, cap, occupied=None):
    t = LS.table(scene, occupied, cap)
    ti, di = (None, None) if matches is None else LS.flat_matches(groups, matches, cap)
    sf, ls = LS.scale_tables()
    P = sum(len(n) for _, n in groups)
    return mt.triangulate_keyline_pairs(
        line_camera(), scene["setup_type"], groups, t["keylines"], t["line_functions"], t["kl_x_right"], t["pose"], t["median_depth"], t["occupied"],
        sf, ls, counts=t["counts"], kp_depths=t["kp_depths"], kp_counts=t["kp_counts"], lines_3d=t["lines_3d"], lbd=t["lbd"], train_idx=ti, dist=di,
        true_baseline=LS.TRUE_BASELINE, scale_factor=LS.SCALE_FACTOR, out=_kl_sentinels(P, len(groups), cap), **gates)


def _host_tuple(r):
    return r["match"], r["pos_w"], r["status"], r["occupied_cur"]


GATES = dict(mapping=KP.MAPPING_GATES, unchecked=LS.NO_GATES_CHECK)


@pytest.mark.parametrize("gates", ["mapping", "unchecked"])
def test_l1_keyline_counts_around_the_workgroup(gates):
    """cap 300, cur with 255 / 256 / 257 / 300 key lines, neighbours with 70 and with 300, four groups of three pairs in one call, with the
    duplicate check and without: the geometry kernel's second blockIdx.y, the second trip of the resolve loops, train indices above 255"""
    scene, groups, matches = LS.wide_counts_case()
    want = LS.wide_reference("counts", gates)["ref"]
    assert_same(kl_device(plp.matcher(), scene, groups, matches, GATES[gates], LS.WIDE_CAP), want, gates)


@pytest.mark.parametrize("occupancy", LS.SHARED_CASES)
def test_l2_duplicates_across_trips_of_the_resolve_loop(occupancy):
    """query slots 10, 266 and 290 share train index 260 (280 at the second neighbour): the atomicMin between slots of different trips,
    first_winner[t] with t >= 256, occ_cur carried from pair to pair for slots above 255; out_occ_cur over the whole capacity"""
    scene, groups, matches, occ = LS.shared_train_case()
    want = LS.wide_reference("shared", "mapping", occupancy)["ref"]
    mt = plp.matcher()
    assert_same(kl_device(mt, scene, groups, matches, KP.MAPPING_GATES, LS.WIDE_CAP, occ[occupancy]), want, occupancy)
    assert_same(_host_tuple(kl_host(mt, scene, groups, matches, KP.MAPPING_GATES, LS.WIDE_CAP, occ[occupancy])), want, occupancy + " host")


def test_l3_kp_depth_range_above_255():
    """stereo, 260 key points, key lines up to slot 299: the key points' depths read with a key-line index at and above 256"""
    scene, groups, matches = LS.kp_depth_case()
    want = LS.wide_reference("kp", "unchecked")["ref"]
    assert (want[2][:, LS.KP_COUNT:] == KP.KP_DEPTH_RANGE).sum() >= 20 and not (want[2][:, :LS.KP_COUNT] == KP.KP_DEPTH_RANGE).any()
    assert_same(kl_device(plp.matcher(), scene, groups, matches, LS.NO_GATES_CHECK, LS.WIDE_CAP), want, "kp depths")


def test_l4_keylines_at_the_capacity_limit():
    """cap = 8192: 32 workgroups per pair in the geometry kernel, 32 trips in the resolve kernel, 40 960 B of dynamic LDS"""
    scene, groups, matches, planted = LS.limit_case()
    want = LS.wide_reference("limit")["ref"]
    for p, j, t in planted["created"]:
        assert want[2][p, j] == KP.CREATED and want[0][p, j] == t
    mt = plp.matcher()
    hip_last_error = plp.lib().hipGetLastError                  # the runtime the library is bound to
    hip_last_error()
    got = kl_device(mt, scene, groups, matches, KP.MAPPING_GATES, LS.LIMIT_CAP)    # any status but PLP_OK raises
    assert hip_last_error() == 0
    assert_same(got, want, "device")
    assert_same(_host_tuple(kl_host(mt, scene, groups, matches, KP.MAPPING_GATES, LS.LIMIT_CAP)), want, "host")


def test_l5_keyline_host_entry_runs_the_1nn_at_the_wide_counts():
    scene, groups, matches = LS.wide_counts_case()
    mt = plp.matcher()
    assert_same(_host_tuple(kl_host(mt, scene, groups, matches, KP.MAPPING_GATES, LS.WIDE_CAP)), LS.wide_reference("counts", "mapping")["ref"], "host")
    # without train_idx the entry runs the batched 1-NN on the device; the restatement gets what it returned
    r = kl_host(mt, scene, groups, None, KP.MAPPING_GATES, LS.WIDE_CAP)
    ti, di = r["train_idx"], r["dist"]
    bt, bd = LS.flat_matches(groups, matches, LS.WIDE_CAP)
    m2, p = [], 0
    for kf1, ngh in groups:
        n = len(scene["kfs"][kf1]["keylines"])
        for k in range(len(ngh)):
            assert np.array_equal(di[p + k, :n], bd[p + k, :n])    # the nearest distance is unique even where the nearest line is not
        m2.append([(ti[p + k, :n], di[p + k, :n]) for k in range(len(ngh))])
        p += len(ngh)
    assert (ti >= 256).sum() > 50
    assert_same(_host_tuple(r), LS.run_ref(scene, groups, m2, KP.MAPPING_GATES, cap=LS.WIDE_CAP), "host 1-NN")


# ================================================================================================================ stereo key lines
@pytest.mark.parametrize("caps", SW.CAPS, ids=[f"{a}x{b}" for a, b in SW.CAPS])
def test_s1_stereo_association_above_one_workgroup(caps):
    """left counts 0, 255, 256, 257, cap, 1 at capacities of two and three workgroups, device and host"""
    torch, dev = _dev()
    cap_l, cap_r = caps
    a = SW.association(cap_l, cap_r)
    T = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(dev)
    d_good = torch.full((SW.B, cap_l), -12345, dtype=torch.int32, device=dev)
    d_dep = torch.full((SW.B, cap_l, 2), 777.0, dtype=torch.float32, device=dev)
    d_xr = torch.full((SW.B, cap_l, 2), 555.0, dtype=torch.float32, device=dev)
    mt = plp.matcher()
    mt.stereo_keylines_device(SW.B, cap_l, cap_r, T(a["kl_l"].view(np.uint8)), T(a["kl_r"].view(np.uint8)), T(a["idx"]), T(a["dist"]), d_good, d_dep,
                              d_xr, counts_left=T(a["cl"]), counts_right=T(a["cr"]))
    torch.cuda.synchronize()
    good, dep, xr = d_good.cpu().numpy(), d_dep.cpu().numpy(), d_xr.cpu().numpy()
    for b in range(SW.B):
        n = a["cl"][b]
        assert np.array_equal(good[b][:n], a["good"][b]) and np.array_equal(dep[b][:n], a["depths"][b]) and np.array_equal(xr[b][:n], a["x_right"][b]), b
        assert (good[b][n:] == -12345).all() and (dep[b][n:] == 777.0).all() and (xr[b][n:] == 555.0).all(), b
    out = dict(good_match=np.full((SW.B, cap_l), -12345, np.int32), kl_depths=np.full((SW.B, cap_l, 2), 777.0, np.float32),
               kl_x_right=np.full((SW.B, cap_l, 2), 555.0, np.float32))
    h = mt.stereo_keylines(a["kl_l"], a["kl_r"], a["idx"], a["dist"], counts_left=a["cl"], counts_right=a["cr"], out=out)
    assert np.array_equal(h["good_match"], good) and np.array_equal(h["kl_depths"], dep) and np.array_equal(h["kl_x_right"], xr)


@pytest.mark.parametrize("route", ["stereo", "rgbd"])
def test_s2_keylines_3d_above_one_workgroup(route):
    """cap 600, the same left counts: the stereo branch with good_match from S1's association, the RGB-D branch with key-line depths"""
    torch, dev = _dev()
    d = SW.lines_3d(route)
    cap, B = SW.CAP_3D, SW.B
    T = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(dev)
    d_pos = torch.full((B, cap, 6), 9.5, dtype=torch.float64, device=dev)
    d_val = torch.full((B, cap), 7, dtype=torch.uint8, device=dev)
    cam = stereo_camera(EUROC)
    mt = plp.matcher()
    host_out = dict(pos_w=np.full((B, cap, 6), 9.5), valid=np.full((B, cap), 7, np.uint8))
    if route == "stereo":
        mt.keylines_3d_device(cam, plp.SETUP_STEREO, B, cap, T(d["poses"]), T(d["kl"].view(np.uint8)), d_pos, good_match=T(d["good_match"]),
                              keylines_right=T(d["kl_r"].view(np.uint8)), cap_right=d["kl_r"].shape[1], counts=T(d["cl"]), counts_right=T(d["cr"]),
                              out_valid=d_val)
        h = mt.keylines_3d(cam, plp.SETUP_STEREO, d["poses"], d["kl"], good_match=d["good_match"], keylines_right=d["kl_r"], counts=d["cl"],
                           counts_right=d["cr"], out=host_out)
    else:
        mt.keylines_3d_device(cam, plp.SETUP_RGBD, B, cap, T(d["poses"]), T(d["kl"].view(np.uint8)), d_pos, kl_depths=T(d["kl_depths"]),
                              counts=T(d["cl"]), out_valid=d_val)
        h = mt.keylines_3d(cam, plp.SETUP_RGBD, d["poses"], d["kl"], kl_depths=d["kl_depths"], counts=d["cl"], out=host_out)
    torch.cuda.synchronize()
    pos, val = d_pos.cpu().numpy(), d_val.cpu().numpy()
    for b in range(B):
        n = d["cl"][b]
        _check_3d(pos[b][:n], val[b][:n], d["pos_w"][b], d["valid"][b], f"{route} frame {b}")
        assert (pos[b][n:] == 9.5).all() and (val[b][n:] == 7).all(), b
    assert np.array_equal(h["pos_w"].view(np.uint64), pos.view(np.uint64)) and np.array_equal(h["valid"], val)
