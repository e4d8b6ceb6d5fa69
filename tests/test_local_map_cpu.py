"""plp_model_local_map_host (the host build of csrc/local_map.hpp, a team of one lane) against the restatement of DESIGN.md section 5, D18 in
tests/local_map_ref.py: exact equality of every output over sentinel-filled arrays, so that what the library leaves unwritten is checked too;
and a census, on the restatement alone, that the committed scenes reach every branch D18 names."""
import importlib

import numpy as np
import pytest

import local_map_ref as R
import local_map_scene as S

plp = importlib.import_module("structure-plp-slam_amd")

_results, _events = {}, {}


def results(name):
    """the restatement of a scene, computed once"""
    if name not in _results:
        sc, ev = S.scene(name), set()
        _results[name] = R.run_scene(sc, sc["max_kf"], ev)
        _events[name] = ev
    return _results[name]


def sentinels(want):
    return {k: np.full_like(v, R.SENTINEL[k]) for k, v in want.items()}


def check(fn, name, k_cap, m_cap, ml_cap, **over):
    sc = S.scene(name)
    lines = sc["kf_lm_lines"] is not None
    want = R.expected(results(name), k_cap, m_cap, ml_cap, lines)
    got = fn(k_cap=k_cap, m_cap=m_cap, ml_cap=ml_cap, out=sentinels(want), **S.call_args(sc, **over))
    assert set(got) == set(want)
    for k in want:
        assert np.array_equal(got[k], want[k]), (name, k, np.argwhere(got[k] != want[k])[:4].tolist())
    return want


def roomy(name):
    sc = S.scene(name)
    return len(sc["kf_parent"]) + 2, len(sc["obs_offsets"]) + 1, sc["LL"] + 2


# the caps around the true lengths of one frame of a scene: (scene, frame)
EDGE = ("f65", 2)


def edge_caps():
    r = results(EDGE[0])[EDGE[1]]
    nk, nm, nl = len(r["first"]) + len(r["second"]), len(r["local_lm"]), len(r["local_lines"])
    kc, mc, mlc = roomy(EDGE[0])
    out = []
    for d in (-1, 0, 1):
        out += [(nk + d, mc, mlc, R.KF_OVERFLOW if d < 0 else R.OK), (kc, nm + d, mlc, R.LM_OVERFLOW if d < 0 else R.OK),
                (kc, mc, nl + d, R.LINE_OVERFLOW if d < 0 else R.OK)]
    return out


@pytest.mark.parametrize("name", list(S.SCENES))
def test_host_build_equals_restatement(name):
    check(plp.model_local_map, name, *roomy(name))


@pytest.mark.parametrize("i", range(9))
def test_host_build_at_the_caps(i):
    """every list at cap - 1, cap and cap + 1 of one frame's true length: the count is the true length, rows [0, cap) are written, a key-frame
    overflow leaves the landmark lists alone"""
    kc, mc, mlc, st = edge_caps()[i]
    want = check(plp.model_local_map, EDGE[0], kc, mc, mlc)
    assert want["status"][EDGE[1]] == st


def test_host_build_zero_caps_and_no_optionals():
    """caps of 0 (NULL list outputs), no first_weight, NULL counts and erased flags"""
    sc = S.scene("f63_points")
    args = S.call_args(sc, kf_counts=None, frm_counts=None, kf_erased=None, lm_erased=None)
    bare = dict(sc, kf_counts=None, frm_counts=None, kf_erased=None, lm_erased=None)
    res = R.run_scene(bare, sc["max_kf"])
    want = R.expected(res, 0, 0, 0, False)
    del want["first_weight"]
    got = plp.model_local_map(k_cap=0, m_cap=0, ml_cap=0, out=sentinels(want), outputs=(), **args)
    for k in want:
        assert np.array_equal(got[k], want[k]), k
    kc, mc, mlc = roomy("f63_points")
    want = R.expected(res, kc, mc, mlc, False)
    got = plp.model_local_map(k_cap=kc, m_cap=mc, ml_cap=mlc, out=sentinels(want), **args)
    for k in want:
        assert np.array_equal(got[k], want[k]), k


def test_mirror_class():
    sc = S.scene("f130")
    r = results("f130")
    tables = {k: sc[k] for k in ("kf_covis", "kf_parent", "kf_children_offsets", "kf_children", "kf_lm", "obs_offsets", "obs_kf", "kf_erased", "kf_counts",
                                 "kf_lm_lines", "kf_kl_counts", "lm_erased", "lm_erased_lines")}
    for b in (1, 3, 4):
        u = plp.local_map_updater(sc["max_kf"])
        found = u.acquire_local_map(tables, R.frame_slots(sc, b), R.frame_slots(sc, b, True))
        assert found == r[b]["found"]
        if found:
            assert u.get_local_keyframes().tolist() == r[b]["first"] + r[b]["second"]
            assert u.get_local_landmarks().tolist() == r[b]["local_lm"]
            assert u.get_local_landmarks_line().tolist() == r[b]["local_lines"]
            assert u.get_nearest_covisibility() == r[b]["nearest"]


def test_refusals():
    sc = S.scene("f1")
    kc, mc, mlc = roomy("f1")
    a = S.call_args(sc)

    def code(**over):
        with pytest.raises(plp.PlpError) as e:
            plp.model_local_map(**{**dict(a, k_cap=kc, m_cap=mc, ml_cap=mlc), **over})
        return e.value.status
    assert code(k_cap=-1) == plp.PLP_ERR_INVALID_ARG
    assert code(m_cap=-1) == plp.PLP_ERR_INVALID_ARG
    assert code(ml_cap=-1) == plp.PLP_ERR_INVALID_ARG
    assert code(max_num_local_keyfrms=-1) == plp.PLP_ERR_INVALID_ARG
    assert code(obs_offsets=sc["obs_offsets"][::-1].copy()) == plp.PLP_ERR_INVALID_ARG
    assert code(fcap=plp.LOCAL_MAP_MAX_SLOTS + 1, frm_lm=np.zeros((1, plp.LOCAL_MAP_MAX_SLOTS + 1), np.int32), frm_counts=None, frm_lm_lines=None,
                frm_kl_counts=None) == plp.PLP_ERR_UNSUPPORTED
    big = plp.LOCAL_MAP_MAX_KF + 1
    assert code(kf_parent=np.full(big, -1, np.int32), kf_covis=np.full((big, 10), -1, np.int32), kf_children_offsets=np.zeros(big + 1, np.int32),
                kf_children=np.zeros(0, np.int32), kf_lm=np.full((big, 1), -1, np.int32), kf_lm_lines=None, kf_counts=None, kf_kl_counts=None,
                kf_erased=None) == plp.PLP_ERR_UNSUPPORTED


# ---- the census: what the committed scenes reach, read off the restatement alone
CENSUS = [
    "cut_mid_list", "cut_at_first_iteration", "cut_never", "cut_exactly_at_max_still_runs",
    "covis_later", "covis_local", "covis_erased", "covis_none", "covis_all_rejected",
    "child_added", "children_all_rejected",
    "parent_added", "parent_rejected", "parent_minus_one",
    "child_then_covis", "erased_heaviest", "tie_for_nearest", "every_voted_erased", "no_keyframes",
    "duplicate_across_kf_lm", "duplicate_inside_kf_lm", "erased_in_kf_lm", "erased_in_frm_lm", "held_twice", "held_kf_lm", "not_held_kf_lm",
    "duplicate_across_kf_lm_lines", "duplicate_inside_kf_lm_lines", "erased_in_kf_lm_lines", "held_kf_lm_lines", "not_held_kf_lm_lines",
    "out_of_table_frm_lm", "out_of_table_kf_lm", "out_of_table_obs_kf", "covis_out_of_table", "parent_out_of_table", "child_out_of_table",
]


@pytest.mark.parametrize("event", CENSUS)
def test_census(event):
    for name in S.SCENES:
        results(name)
    assert any(event in ev for ev in _events.values()), event


def test_census_cut_at_sixty():
    """the cut of the reference's own 60 is taken mid-list, at the first iteration and never, in scenes that pass 60"""
    ev = set()
    for name in ("f130", "f130_mid"):
        assert S.scene(name)["max_kf"] == 60
        results(name)
        ev |= _events[name]
    assert {"cut_mid_list", "cut_at_first_iteration", "cut_never", "cut_exactly_at_max_still_runs"} <= ev
    assert any(r["found"] and len(r["first"]) >= 61 for r in results("f130"))


def test_census_shapes():
    """runs of 0, 1 and more than 64 observations; a frame without a landmark; every voted key frame erased gives OK with empty lists"""
    sc = S.scene("f130")
    runs = np.diff(sc["obs_offsets"])
    assert (runs == 0).any() and (runs == 1).any() and (runs > 64).any()
    r = results("f130")
    assert not r[3]["found"]
    assert r[4]["found"] and r[4]["first"] == [] and r[4]["second"] == [] and r[4]["nearest"] == -1 and r[4]["local_lm"] == []
    assert R.status_of(r[4], 0, 0, 0) == R.OK
    assert sorted(len(S.scene(n)["kf_parent"]) for n in S.SCENES) == [1, 63, 63, 64, 65, 130, 130]


def test_census_overflow_statuses():
    """each overflow status at cap - 1, and OK at cap and cap + 1"""
    got = [(i % 3, st) for i, (_, _, _, st) in enumerate(edge_caps())]
    assert got == [(0, R.KF_OVERFLOW), (1, R.LM_OVERFLOW), (2, R.LINE_OVERFLOW)] + [(0, R.OK), (1, R.OK), (2, R.OK)] * 2
    r = results(EDGE[0])[EDGE[1]]
    assert len(r["first"]) + len(r["second"]) > 1 and len(r["local_lm"]) > 1 and len(r["local_lines"]) > 1
