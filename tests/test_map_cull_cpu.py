"""plp_model_cull_keyframes_host and plp_model_cull_landmarks_host (the host build of csrc/map_cull.hpp, a team of one lane) against the object-level
restatement of module::local_map_cleaner in tests/map_cull_ref.py: exact equality of every output over sentinel-filled arrays, so that what the
library leaves unwritten is checked too.  The library computes D20's closed form and the restatement mutates objects as the
reference does, so equality here is the proof of the closed form; the census shows that the committed scenes reach every case D20 names."""
import importlib

import numpy as np
import pytest

import map_cull_ref as R
import map_cull_scene as S

plp = importlib.import_module("structure-plp-slam_amd")

_results, _events = {}, set()


def results(name):
    """the restatement of a scene's problems, computed once"""
    if name not in _results:
        sc = S.scene(name)
        _results[name] = [R.remove_redundant_keyframes(sc, g, _events) for g in range(len(sc["cur_kf"]))]
    return _results[name]


def lm_results(name):
    if ("lm", name) not in _results:
        _results[("lm", name)] = R.expected_landmarks(S.lm_scene(name), _events)
    return _results[("lm", name)]


def sentinels(want):
    return {k: np.full_like(v, R.SENTINEL[k]) for k, v in want.items()}


def equal(got, want, what):
    assert set(got) == set(want), what
    for k in want:
        assert np.array_equal(got[k], want[k]), (what, k, np.argwhere(got[k] != want[k])[:4].tolist())


def check(fn, name, optional=True, **over):
    sc = S.scene(name)
    want = R.expected_keyframes(results(name), sc, optional)
    got = fn(out=sentinels(want), outputs=None if optional else (), **S.call_args(sc, **over))
    equal(got, want, name)
    return want


@pytest.mark.parametrize("name", S.SCENES)
def test_host_build_equals_restatement(name):
    check(plp.model_cull_keyframes, name)


@pytest.mark.parametrize("name", list(S.LM_SCENES))
def test_landmark_host_build_equals_restatement(name):
    want = lm_results(name)
    equal(plp.model_cull_landmarks(out=sentinels(want), **S.lm_call_args(S.lm_scene(name))), want, name)


CENSUS = ("SKIP_ORIGIN", "SKIP_WINDOW", "KEPT", "REMOVED", "REMOVED_HELD", "ABSENT", "window_at_cur_skipped", "window_at_cur_minus_2_skipped",
          "window_below_counted", "window_above_counted", "num_valid_0", "ratio_9_10_removed", "ratio_8_9_kept", "num_observations_3",
          "num_observations_4", "third_better_is_last", "cascade_changes_num_valid", "flip_to_removed", "flip_to_kept", "two_removals",
          "erased_keyframe_in_list", "depth_negative", "depth_above_thr", "depth_nan",
          "branch_erased", "branch_ratio", "branch_few_observers", "branch_enough_observers", "branch_not_clear", "ratio_plane", "ratio_no_plane",
          "few_plane", "few_no_plane", "line_variant", "ratio_0_0", "ratio_x_0", "row_outside", "first_plus_2_equals_cur_few",
          "first_plus_2_equals_cur_many", "first_plus_2_one_below_cur_few", "first_plus_2_one_below_cur_many")


def test_census_of_the_scenes():
    """on the restatement alone: every case D20 names happens in a committed scene"""
    for name in S.SCENES:
        results(name)
    for name in S.LM_SCENES:
        lm_results(name)
    assert not [c for c in CENSUS if c not in _events]
    assert "ratio_9_10_kept" not in _events and "ratio_8_9_removed" not in _events


def test_scene_sizes():
    """the sizes the kernels' loops treat apart are in the scenes"""
    sc = S.scene("mono97")
    assert {63, 64, 65, 257} <= set(int(v) for v in sc["kf_counts"])
    n = np.diff(sc["obs_offsets"])
    assert {0, 1, 3, 4} <= set(int(v) for v in n) and n.max() > 64
    assert max(np.diff(sc["covis_offsets"])) > 64
    assert {0, 1} <= set(int(v) for v in np.diff(S.scene("stereo97")["covis_offsets"]))
    assert {sc["kf_lm"].shape[0], S.scene("mono65")["kf_lm"].shape[0]} == {97, 65}
    assert S.scene("stereo97")["x_right"].min() < 0 <= S.scene("stereo97")["x_right"].max() and S.scene("rgbd65")["depths"] is not None


def test_snapshot_tables_are_consistent():
    """every observation names a slot that holds its landmark (what D20 asks of the caller)"""
    for name in S.SCENES:
        sc = S.scene(name)
        F, cap = sc["kf_lm"].shape
        lm = np.repeat(np.arange(len(sc["obs_offsets"]) - 1), np.diff(sc["obs_offsets"]))
        ok = (sc["obs_kf"] >= 0) & (sc["obs_kf"] < F) & (sc["obs_idx"] >= 0) & (sc["obs_idx"] < cap)
        assert np.array_equal(sc["kf_lm"][sc["obs_kf"][ok], sc["obs_idx"][ok]], lm[ok]), name


def test_derived_and_given_num_observations_agree():
    for name in ("mono65", "rgbd65"):
        sc = S.scene(name)
        assert sc["lm_num_obs"] is not None
        check(plp.model_cull_keyframes, name, lm_num_obs=None)


@pytest.mark.parametrize("drop", ["kf_erased", "optional_outputs"])
def test_null_optionals_change_nothing(drop):
    """kf_erased is never read; without the optional outputs the others are the same"""
    if drop == "kf_erased":
        check(plp.model_cull_keyframes, "mono97", kf_erased=None)
    else:
        check(plp.model_cull_keyframes, "mono97", optional=False)


def test_null_optional_tables():
    """NULL x_right is every weight 1, NULL kf_cannot_erase and lm_erased none, NULL kf_counts the cap: against the restatement of such a scene"""
    sc = dict(S.scene("mono65"), x_right=None, kf_cannot_erase=None, lm_erased=None, kf_counts=None, lm_num_obs=None)
    want = R.expected_keyframes([R.remove_redundant_keyframes(sc, g) for g in range(len(sc["cur_kf"]))], sc)
    equal(plp.model_cull_keyframes(out=sentinels(want), **S.call_args(sc)), want, "NULL tables")
    assert R.REMOVED_HELD not in want["decision"] and R.REMOVED in want["decision"]
    lsc = dict(S.lm_scene("points"), lm_erased=None, owning_plane=None)
    lwant = R.expected_landmarks(lsc)
    equal(plp.model_cull_landmarks(out=sentinels(lwant), **S.lm_call_args(lsc)), lwant, "NULL landmark tables")


def test_no_problem_writes_nothing():
    sc = S.scene("mono65")
    out = sentinels(R.expected_keyframes([], dict(sc, covis=sc["covis"][:0], covis_offsets=sc["covis_offsets"][:1])))
    got = plp.model_cull_keyframes(out=out, **S.call_args(sc, cur_kf=sc["cur_kf"][:0], covis_offsets=[0], covis=sc["covis"][:0]))
    assert all(v.size == 0 for v in got.values())
    lsc = S.lm_scene("points")
    got = plp.model_cull_landmarks(**S.lm_call_args(lsc, fresh_offsets=[0], cur_kf_id=[], num_obs_thr=[]), out=dict(
        state=np.full(len(lsc["fresh"]), 0xEE, np.uint8), fresh=np.full(len(lsc["fresh"]), -77, np.int32)))
    assert (got["state"] == 0xEE).all() and (got["fresh"] == -77).all()


def _kf_struct(**over):
    """a well-formed plp_cull_keyframes_args over one tiny problem, every pointer at an array of its own"""
    n = lambda dt, k: np.zeros(k, dt)
    arrs = dict(kf_lm=n(np.int32, 8), undist=n(plp.KP_DTYPE, 8), depths=n(np.float32, 8), depth_thr=n(np.float32, 2), kf_id=n(np.uint32, 2),
                obs_offsets=n(np.int32, 4), obs_kf=n(np.int32, 1), obs_idx=n(np.int32, 1), cur_kf=n(np.int32, 1), covis_offsets=np.array([0, 1], np.int32),
                covis=n(np.int32, 1), out_num_removed=n(np.int32, 1), out_decision=n(np.uint8, 1), out_num_valid=n(np.int32, 1),
                out_num_redundant=n(np.int32, 1))
    arrs["obs_offsets"][3] = 1
    a = plp.cull_keyframes_args_c()
    for k, v in dict(F=2, L=3, T=1, cap=4, kp_stride=4, G=1, Cv=1, origin_id=9, is_monocular=0).items():
        setattr(a, k, v)
    for k, v in arrs.items():
        setattr(a, k, v.ctypes.data)
    for k, v in over.items():
        setattr(a, k, v)
    return a, arrs


KF_INVALID = [dict(F=-1), dict(L=-1), dict(T=-1), dict(cap=-1), dict(kp_stride=-1), dict(G=-1), dict(Cv=-1), dict(kp_stride=3), dict(cur_kf=None),
              dict(covis_offsets=None), dict(covis=None), dict(kf_id=None), dict(kf_lm=None), dict(undist=None), dict(obs_offsets=None), dict(obs_kf=None),
              dict(obs_idx=None), dict(depths=None), dict(depth_thr=None), dict(out_num_removed=None), dict(out_decision=None), dict(out_num_valid=None),
              dict(out_num_redundant=None)]
KF_UNSUPPORTED = [dict(F=8193), dict(cap=8193, kp_stride=0), dict(G=65536)]


@pytest.mark.parametrize("i", range(len(KF_INVALID) + len(KF_UNSUPPORTED)))
def test_keyframe_argument_checks(i):
    bad = (KF_INVALID + KF_UNSUPPORTED)[i]
    a, arrs = _kf_struct(**bad)
    want = plp.PLP_ERR_INVALID_ARG if i < len(KF_INVALID) else plp.PLP_ERR_UNSUPPORTED
    assert plp.lib().plp_model_cull_keyframes_host(plp.C.byref(a)) == -want, bad
    assert arrs["out_decision"][0] == 0 and arrs["out_num_removed"][0] == 0
    a, _ = _kf_struct()
    assert plp.lib().plp_model_cull_keyframes_host(plp.C.byref(a)) == 1
    assert plp.lib().plp_model_cull_keyframes_host(None) == -plp.PLP_ERR_INVALID_ARG


def test_keyframe_offsets_must_rise():
    for field, bad in (("obs_offsets", [0, 2, 1, 1]), ("obs_offsets", [1, 1, 1, 1]), ("obs_offsets", [0, 0, 0, 2]), ("covis_offsets", [1, 1]),
                       ("covis_offsets", [0, 2])):
        a, arrs = _kf_struct()
        arrs[field][:] = bad
        assert plp.lib().plp_model_cull_keyframes_host(plp.C.byref(a)) == -plp.PLP_ERR_INVALID_ARG, (field, bad)
    a, _ = _kf_struct(is_monocular=1, depths=None, depth_thr=None)      # the depth tables are not needed then
    assert plp.lib().plp_model_cull_keyframes_host(plp.C.byref(a)) == 1


def _lm_struct(**over):
    n = lambda dt, k: np.zeros(k, dt)
    arrs = dict(fresh_offsets=np.array([0, 2], np.int32), fresh=n(np.int32, 2), num_observed=n(np.uint32, 3), num_observable=n(np.uint32, 3),
                first_kf_id=n(np.uint32, 3), num_obs=n(np.uint32, 3), cur_kf_id=n(np.uint32, 1), num_obs_thr=n(np.uint32, 1), out_state=n(np.uint8, 2),
                out_num_removed=n(np.int32, 1), out_num_fresh=n(np.int32, 1), out_fresh=n(np.int32, 2))
    a = plp.cull_landmarks_args_c()
    a.R, a.N, a.L = 1, 2, 3
    for k, v in arrs.items():
        setattr(a, k, v.ctypes.data)
    for k, v in over.items():
        setattr(a, k, v)
    return a, arrs


LM_INVALID = [dict(R=-1), dict(N=-1), dict(L=-1)] + [{k: None} for k in ("fresh_offsets", "fresh", "num_observed", "num_observable", "first_kf_id", "num_obs",
                                                                          "cur_kf_id", "num_obs_thr", "out_state", "out_num_removed", "out_num_fresh", "out_fresh")]


@pytest.mark.parametrize("i", range(len(LM_INVALID)))
def test_landmark_argument_checks(i):
    a, arrs = _lm_struct(**LM_INVALID[i])
    arrs["out_state"][:] = 0xEE
    assert plp.lib().plp_model_cull_landmarks_host(plp.C.byref(a)) == -plp.PLP_ERR_INVALID_ARG, LM_INVALID[i]
    assert (arrs["out_state"] == 0xEE).all()
    a, arrs = _lm_struct()
    assert plp.lib().plp_model_cull_landmarks_host(plp.C.byref(a)) == 1
    a, arrs = _lm_struct()
    arrs["fresh_offsets"][:] = [0, 1]
    assert plp.lib().plp_model_cull_landmarks_host(plp.C.byref(a)) == -plp.PLP_ERR_INVALID_ARG


def test_mirror_class_runs_the_reference_surface():
    """module::local_map_cleaner's surface over rows, on the host build"""
    sc, lsc = S.scene("mono97"), S.lm_scene("points")
    cl = plp.local_map_cleaner(is_monocular=True)
    cl.set_origin_keyframe_id(sc["origin_id"])
    n = cl.remove_redundant_keyframes(int(sc["cur_kf"][0]), sc["covis"], sc)
    assert n == results("mono97")[0]["num_removed"] and np.array_equal(cl.last["kf_removed"][0], results("mono97")[0]["kf_removed"])
    lo, hi = int(lsc["fresh_offsets"][2]), int(lsc["fresh_offsets"][3])
    for lm in lsc["fresh"][lo:hi]:
        cl.add_fresh_landmark(lm)
        cl.add_fresh_landmark_line(lm)
    states, kept, removed = R.remove_redundant_landmarks(lsc, 2)
    assert cl.remove_redundant_landmarks(int(lsc["cur_kf_id"][2]), lsc) == removed and cl.fresh_landmarks == kept
    lines = dict(lsc, owning_plane=None, num_obs_thr=np.full(5, 3, np.uint32))
    assert cl.remove_redundant_landmarks_line(int(lsc["cur_kf_id"][2]), lsc) == R.remove_redundant_landmarks(lines, 2)[2]
    cl.reset()
    assert cl.fresh_landmarks == [] and cl.fresh_landmarks_line == []
