"""The scenes of tests/test_gpu_pair_kernels_wide.py held to their names, without a GPU: on the restatement alone every scene shows the edge
it was built for -- landmarks created in the second and third workgroup, key points and train indices at and above 256, whole workgroups
and waves matched or empty exactly as planted, duplicates that meet across trips of the resolve loop, the planted slots at the capacity
limit -- and every comparison that depends on the null vector or on a libm result keeps the relative gap of the other CPU tests
(DESIGN.md section 5, D8 item 3, D10).  A device that handled only the slots below 256 could not equal these references."""
import collections

import numpy as np
import pytest

import keyline_pairs_ref as KP
import keyline_pairs_scene as LS
import keypoint_pairs_ref as KR
import keypoint_pairs_scene as PS
import stereo_keylines_wide as SW

GATE_GAP = 1e-9                                                 # the relative gap every dependent comparison keeps (D8 item 3, D10)
WIDE = range(len(PS.WIDE_SETUPS))


def _keeps_gap(gaps, what):
    smallest = {}
    for kind, g in gaps:
        smallest[kind] = min(smallest.get(kind, 1.0), g)
    print(what, smallest)
    for kind, g in smallest.items():
        if kind != "stereo_equal_inputs":                       # equal depths: both sides bit-identical on any libm
            assert g >= GATE_GAP, (what, kind, g)


# ================================================================================================================ key points
@pytest.mark.parametrize("permuted", [True, False])
@pytest.mark.parametrize("wi", WIDE)
def test_k1_landmarks_are_created_in_every_workgroup(wi, permuted):
    sc, pairs, mq, qf = PS.wide_counts_case(wi)
    idx, pos, st, _, _ = PS.wide_reference("counts", wi, permuted)["ref"]
    assert [len(sc["kfs"][f1]["keypts"]) for f1, _ in pairs] == [PS.WIDE_CAP] * 6
    assert tuple(len(sc["kfs"][f2]["keypts"]) for _, f2 in pairs) == PS.WIDE_COUNTS
    for p, n2 in enumerate(PS.WIDE_COUNTS):
        assert (st[p, :n2] != PS.SENT_U8).all() and (st[p, n2:] == PS.SENT_U8).all() and (idx[p, n2:] == PS.SENT_I32).all()
        made = st[p] == KR.CREATED
        assert made[:256].any()
        assert made[256:].any() == (n2 > 256), (p, n2)
        assert made[512:].any() == (n2 > 512), (p, n2)
        assert (idx[p][made] >= 256).any() and (idx[p][made] < 256).any()
        if p != 1:                                              # key frame 2 stands 16 cm from key frame 0: little parallax, few landmarks
            assert made[:256].sum() >= 30 and (idx[p][made] >= 256).sum() >= 30 and (idx[p][made] < 256).sum() >= 30
            if n2 > 257:
                assert made[256:].sum() >= 30 and (idx[p, 256:][made[256:]] >= 256).sum() >= 10     # both indices of the pair above 255


def test_k1_every_status_is_reached_at_and_above_slot_256():
    for permuted in (True, False):
        seen = np.zeros(10, np.int64)
        for wi in WIDE:
            hi = PS.wide_reference("counts", wi, permuted)["ref"][2][:, 256:]
            seen += np.bincount(hi[hi != PS.SENT_U8], minlength=10)
        print(permuted, dict(zip(KR.STATUS_NAMES, seen.tolist())))
        for code in range(10):
            if code == KR.PAIR_SKIPPED or (code == KR.INDEX_RANGE and not permuted):   # key frame 1 fills the capacity: without q_feature
                continue                                                               # no index in [0, m_cap) lies outside it
            assert seen[code] > 0, (permuted, KR.STATUS_NAMES[code])


def _matched_slots(infos_p):
    return sorted(t for t, _, _, _ in infos_p)


def test_k2_the_layouts_are_the_planted_ones():
    sc, pairs, mq, qf, skip = PS.wide_layout_case()
    r = PS.wide_reference("layout")
    idx, pos, st, _, _ = r["ref"]
    assert [len(kf["keypts"]) for kf in sc["kfs"][:2]] == [PS.WIDE_CAP, PS.WIDE_CAP]
    per_wave = lambda slots: collections.Counter((t // 256, (t % 256) // 64) for t in slots)
    want_waves = [
        {(0, w): 64 for w in range(4)},                                                         # workgroup 0 full, 1 and 2 empty
        {(0, 3): 64, (1, 3): 64},                                                               # the three waves in front are empty
        {(g, w): 1 for g in range(2) for w in range(4)} | {(2, 0): 1},                          # lane 0 of every wave, the partial one included
        {(g, w): 1 for g in range(2) for w in range(4)},                                        # lane 63: the last wave has 8 lanes
        {(0, 3): 1, (1, 0): 1, (2, 0): 1},
        {},
    ]
    for p, (name, slots) in enumerate(PS.WIDE_LAYOUTS):
        matched = _matched_slots(r["infos"][p])                 # the slots the restatement triangulates: what the device packs
        assert matched == sorted(slots), name
        assert dict(per_wave(matched)) == want_waves[p], name
        others = np.setdiff1d(np.arange(PS.WIDE_CAP), slots)
        assert (st[p, others] == KR.NO_MATCH).all(), name
        if slots:
            assert (st[p, slots] == KR.CREATED).sum() >= 0.8 * len(slots), (name, int((st[p, slots] == KR.CREATED).sum()))
    lane = lambda t: t % 64
    assert {lane(t) for t in PS.WIDE_LAYOUTS[2][1]} == {0} and {lane(t) for t in PS.WIDE_LAYOUTS[3][1]} == {63}
    # K4: the skipped pair holds one status in every slot and nothing else; the same pair beside it is computed
    n = len(PS.WIDE_LAYOUTS)
    assert skip.tolist() == [0] * n + [1, 0]
    assert (st[n] == KR.PAIR_SKIPPED).all() and (idx[n] == PS.SENT_I32).all() and (pos[n] == PS.SENT_F64).all()
    assert (st[n + 1] == KR.CREATED).sum() >= 0.8 * PS.WIDE_CAP and (st[n + 1, 512:] == KR.CREATED).sum() >= 4
    assert len(_matched_slots(r["infos"][n + 1])) == PS.WIDE_CAP                                # total = 256 in workgroups 0 and 1


def test_k3_the_planted_slots_at_the_capacity_limit():
    sc, pairs, mq, qf, planted = PS.limit_case()
    idx, pos, st, _, _ = PS.wide_reference("limit")["ref"]
    assert mq.shape == qf.shape == (3, PS.LIMIT_CAP) and [len(kf["keypts"]) for kf in sc["kfs"]] == [8000, PS.LIMIT_CAP, 0]
    assert planted["created"] == [(0, 8191, 7999), (0, 0, 7998)]
    for p, t, j in planted["created"]:
        assert st[p, t] == KR.CREATED and idx[p, t] == j and np.isfinite(pos[p, t]).all()
    for p, t, j in planted["index_range"]:
        assert st[p, t] == KR.INDEX_RANGE and idx[p, t] == j == 8000
    for p, t in planted["no_match"]:
        assert st[p, t] == KR.NO_MATCH and mq[p, t] == PS.LIMIT_CAP and idx[p, t] == -1
    work = (st[0] != KR.NO_MATCH) & (st[0] != KR.INDEX_RANGE)
    assert 200 <= work.sum() <= 500 and (st[0] == KR.CREATED).sum() >= 100
    assert (st[1] == PS.SENT_U8).all()                          # key frame 2 is empty
    assert (st[2, :8000] != PS.SENT_U8).all() and (st[2, 8000:] == PS.SENT_U8).all() and st[2, 7999] != KR.NO_MATCH
    assert (st[2] == KR.CREATED).sum() >= 30 and (idx[2][st[2] == KR.CREATED] >= 8000).any()    # key points of the full key frame above 8000


def test_keypoint_scenes_keep_the_gap():
    for wi in WIDE:
        for permuted in (True, False):
            _keeps_gap(PS.wide_reference("counts", wi, permuted)["gaps"], f"K1 {wi} {permuted}")
    _keeps_gap(PS.wide_reference("layout")["gaps"], "K2 / K4")
    _keeps_gap(PS.wide_reference("limit")["gaps"], "K3")
    kinds = {k for wi in WIDE for k, _ in PS.wide_reference("counts", wi, True)["gaps"]}
    assert kinds >= {"rays", "stereo", "depth", "reproj", "scale"}, kinds


# ================================================================================================================ key lines
def _passed_gates(scene, groups, matches, gates):
    """per pair the query slots that pass the three gates, from the restatement's gate on the inputs"""
    out = []
    for g, (kf1, ngh) in enumerate(groups):
        cur = scene["kfs"][kf1]
        for k, kf2 in enumerate(ngh):
            other, (ti, di) = scene["kfs"][kf2], matches[g][k]
            out.append({j for j in range(len(cur["keylines"])) if 0 <= ti[j] < len(other["keylines"]) and
                        KP.gate(cur["keylines"][j], other["keylines"][ti[j]], di[j], gates["dist_thr"], gates["endpoint_thr"], gates["angle_thr"])
                        == KP.CREATED})
    return out


@pytest.mark.parametrize("gates", ["mapping", "unchecked"])
def test_l1_counts_around_the_workgroup(gates):
    scene, groups, matches = LS.wide_counts_case()
    r = LS.wide_reference("counts", gates)
    om, op, st, oc = r["ref"]
    n = [len(kf["keylines"]) for kf in scene["kfs"]]
    assert [n[kf1] for kf1, _ in groups] == [255, 256, 257, 300] and all(len(ngh) == 3 for _, ngh in groups)
    assert all(sorted(n[k] for k in ngh)[0] == 70 and sorted(n[k] for k in ngh)[-1] == 300 for _, ngh in groups)
    p = 0
    high_train = low_only = 0
    for g, (kf1, ngh) in enumerate(groups):
        assert (oc[g, :n[kf1]] != LS.SENT_U8).all() and (oc[g, n[kf1]:] == LS.SENT_U8).all()
        for kf2 in ngh:
            assert (st[p, :n[kf1]] != LS.SENT_U8).all() and (st[p, n[kf1]:] == LS.SENT_U8).all()
            made = om[p][st[p] == KP.CREATED]
            assert (made < n[kf2]).all()
            if n[kf2] == 300:
                high_train += int((made >= 256).sum())
            else:
                low_only += len(made)
            p += 1
    assert high_train >= 30 and low_only >= 30, (high_train, low_only)
    hi = st[:, 256:]
    assert (hi == KP.CREATED).sum() >= 15 and (oc[:, 256:] == 1).sum() >= 15
    assert (st[9:, 256:] == KP.CREATED).sum() >= 10             # cur with 300 key lines: 44 slots of the second trip
    assert st[6, 256] != LS.SENT_U8 and st[3, 256] == LS.SENT_U8   # cur with 257: one slot of the second trip; with 256: none
    if gates == "mapping":
        causes = collections.Counter((c, j >= 256) for notes in r["info"] for j, c in notes)
        print(dict(causes))
        for cause in ("input", "earlier neighbour", "earlier winner"):
            assert causes[(cause, True)] >= 1 and causes[(cause, False)] >= 5, (cause, causes)
        assert (hi == KP.OCCUPIED_CUR).sum() >= 5 and (hi == KP.OCCUPIED_NGH).sum() >= 2
    else:
        assert not (st == KP.OCCUPIED_CUR).any() and not (st == KP.OCCUPIED_NGH).any()


def test_l2_duplicates_meet_across_trips_of_the_resolve_loop():
    scene, groups, matches, occ = LS.shared_train_case()
    q0, q1, q2 = LS.SHARED_QUERIES
    t0, t1 = LS.SHARED_TRAIN
    assert q0 < 256 <= q1 < q2 and t0 >= 256 and t1 >= 256
    assert groups == [(0, [2, 4])] and all(len(scene["kfs"][k]["keylines"]) == LS.WIDE_CAP for k in (0, 2, 4))
    (ti0, _), (ti1, _) = matches[0]
    assert [int(ti0[q]) for q in LS.SHARED_QUERIES] == [t0] * 3 and [int(ti1[q]) for q in LS.SHARED_QUERIES] == [t1] * 3
    assert (ti0 == t0).sum() == 3 and (ti1 == t1).sum() == 3    # nobody else names the planted train index
    passed = _passed_gates(scene, groups, matches[:1], KP.MAPPING_GATES)
    assert all(set(LS.SHARED_QUERIES) <= s for s in passed)
    for k, (kf2, t) in enumerate(zip(groups[0][1], LS.SHARED_TRAIN)):   # each of them alone becomes a landmark
        assert all(LS.created_alone(scene, 0, kf2, q, t) for q in LS.SHARED_QUERIES)
    C, OC, ON = KP.CREATED, KP.OCCUPIED_CUR, KP.OCCUPIED_NGH
    want = {"free": ([C, ON, ON], [OC, C, ON], [1, 1, 0]),      # status at the first neighbour, at the second, occupied_cur
            "cur occupied": ([OC, C, ON], [OC, OC, C], [1, 1, 1]),
            "train occupied": ([ON, ON, ON], [C, ON, ON], [1, 0, 0])}
    for case in LS.SHARED_CASES:
        r = LS.wide_reference("shared", "mapping", case)
        om, op, st, oc = r["ref"]
        first, second, after = want[case]
        qs = list(LS.SHARED_QUERIES)
        assert st[0, qs].tolist() == first and st[1, qs].tolist() == second and oc[0, qs].tolist() == after, case
        assert [om[0, q] for q in qs] == [t0 if s == C else -1 for s in first] and [om[1, q] for q in qs] == [t1 if s == C else -1 for s in second]
        for p in range(2):                                      # the restatement's notes: the planted slots reached the duplicate check
            noted = {j for j, _ in r["info"][p]}
            assert set(qs) <= noted, (case, p)
        causes = [{j: c for j, c in r["info"][p]} for p in range(2)]
        if case == "free":
            assert causes[0][q1] == causes[0][q2] == "earlier winner" and causes[1][q0] == "earlier neighbour" and causes[1][q2] == "earlier winner"
        elif case == "cur occupied":
            assert causes[0][q0] == "input" and causes[0][q2] == "earlier winner" and causes[1][q1] == "earlier neighbour"   # created above 255, carried
        else:
            assert [causes[0][q] for q in qs] == ["input"] * 3
        assert oc.shape == (1, LS.WIDE_CAP) and (oc != LS.SENT_U8).all()


def test_l3_kp_depth_range_above_255():
    scene, groups, matches = LS.kp_depth_case()
    om, op, st, oc = LS.wide_reference("kp", "unchecked")["ref"]
    cur = scene["kfs"][0]
    assert scene["setup_type"] == KP.STEREO and len(cur["kp_depths"]) == LS.KP_COUNT == 260 and len(cur["keylines"]) == LS.WIDE_CAP
    assert all(len(scene["kfs"][k]["kp_depths"]) > len(scene["kfs"][k]["keylines"]) for k in groups[0][1])
    passed = _passed_gates(scene, groups, matches, LS.NO_GATES_CHECK)
    stereo = cur["kl_x_right"][:, 0] >= 0
    n_range = 0
    for p, slots in enumerate(passed):
        for j in slots:
            if j >= LS.KP_COUNT and stereo[j]:
                assert st[p, j] == KP.KP_DEPTH_RANGE, (p, j)
                n_range += 1
            else:
                assert st[p, j] != KP.KP_DEPTH_RANGE, (p, j)
        assert not (st[p, :LS.KP_COUNT] == KP.KP_DEPTH_RANGE).any()
    assert n_range >= 20 and n_range == (st == KP.KP_DEPTH_RANGE).sum()
    assert (st[:, 256:LS.KP_COUNT] == KP.CREATED).any()         # stereo slots in [256, 260) still read a depth
    assert any(st[p, j] == KP.CREATED for p, slots in enumerate(passed) for j in slots if j >= LS.KP_COUNT and not stereo[j])


def test_l4_the_planted_slots_at_the_capacity_limit():
    scene, groups, matches, planted = LS.limit_case()
    r = LS.wide_reference("limit")
    om, op, st, oc = r["ref"]
    n = [len(kf["keylines"]) for kf in scene["kfs"]]
    assert groups == [(0, [2, 4])] and n[0] == n[2] == LS.LIMIT_CAP and st.shape == (2, LS.LIMIT_CAP)
    (p0, j0, t0), (p1, j1, t1) = planted["created"]
    assert j0 == LS.LIMIT_CAP - 1 and t1 > 8000
    passed = _passed_gates(scene, groups, matches, KP.MAPPING_GATES)
    for p, j, t in planted["created"]:
        assert j in passed[p] and st[p, j] == KP.CREATED and om[p, j] == t and oc[0, j] == 1
    assert (st[0] == KP.GATE_DISTANCE).sum() > 8000 and (st[0] == KP.CREATED).sum() >= 10
    assert (oc != LS.SENT_U8).all()


def test_keyline_scenes_keep_the_gap():
    for gates in ("mapping", "unchecked"):
        g = LS.wide_reference("counts", gates)["gaps"]
        assert len(g) >= 300
        _keeps_gap(g, f"L1 {gates}")
    for case in LS.SHARED_CASES:
        _keeps_gap(LS.wide_reference("shared", "mapping", case)["gaps"], f"L2 {case}")
    g = LS.wide_reference("kp", "unchecked")["gaps"]
    assert len(g) >= 100
    _keeps_gap(g, "L3")
    _keeps_gap(LS.wide_reference("limit")["gaps"], "L4")


# ================================================================================================================ stereo key lines
@pytest.mark.parametrize("caps", SW.CAPS)
def test_s1_matches_are_kept_above_slot_255(caps):
    cap_l, cap_r = caps
    a = SW.association(cap_l, cap_r)
    assert a["cl"].tolist() == [0, 255, 256, 257, cap_l, 1] and a["cr"][0] == 0 and a["cr"][4] == cap_r
    for b in (3, 4):
        assert a["good"][b][256] >= 0 and a["good"][b][a["cl"][b] - 1] >= 0, b
    assert all((g >= 0).sum() >= 2 for g in a["good"][1:5]) and all((g == -1).sum() >= 2 for g in a["good"][1:5])
    if cap_l > 512:
        g = a["good"][4]
        assert (g[256:512] >= 0).sum() >= 10 and (g[512:] >= 0).sum() >= 5 and (g >= 256).sum() >= 10 and (g >= 512).any()


@pytest.mark.parametrize("route", ["stereo", "rgbd"])
def test_s2_lines_are_built_above_slot_255(route):
    d = SW.lines_3d(route)
    v = d["valid"][4]
    assert len(v) == SW.CAP_3D and v[256:512].any() and v[512:].any() and not v.all()
    assert d["valid"][3][256] in (0, 1) and len(d["valid"][3]) == 257
    if route == "rgbd":
        assert v[256:].sum() >= 100 and d["valid"][3][256] == 1
