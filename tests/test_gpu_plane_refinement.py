"""plp_plane_refinement_device and plp_plane_refinement_host against the host build of the same header (plp_model_plane_refinement_host, which
tests/test_plane_refinement_cpu.py holds against the restatement): every table and every output bit for bit, sentinels in the slots the call
leaves alone.  DESIGN.md section 5, D26.  iters = 8 and the smallest shapes at which a path can go wrong: 2 and 3 planes, plane rows with gaps,
runs of 1, 2 and 3 invalid rows in the middle and at the end, lists of 17 / 18 and 35 / 36 members (points_per_ransac and twice that), of
63 / 64 / 65 and 255 / 256 / 257 (the ballot and the workgroup edge of the compactions), a merge that lands on n_cap and one that passes it by one,
65 candidates of one parent (more than a wave), 6 updates in one problem (more than the four waves), 1, 3 and 70 ragged problems with
TOO_FEW_PLANES problems between full ones, L = 1, a NaN position, each single stage, two calls on one stream."""
import importlib

import numpy as np
import pytest

import plane_refinement_ref as RR
import plane_refinement_scene as RS
from plane_refinement_scene import DEAD, NEW, P
from plp import plp

pytestmark = pytest.mark.gpu


def same(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def run_model(t, dist, err, kw):
    tt = {k: v.copy() for k, v in t.items()}
    return tt, plp.model_plane_refinement(tt, dist, err, out=RS.sentinel_out(t, kw["merge_cap"]), **kw)


def run_host(mt, t, dist, err, kw):
    tt = {k: v.copy() for k, v in t.items()}
    return tt, mt.plane_refinement(tt, dist, err, out=RS.sentinel_out(t, kw["merge_cap"]), **kw)


def run_device(mt, t, dist, err, kw, calls=1):
    import torch
    dev = torch.device("cuda", 0)
    d = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(dev)
    G, NP = t["pl_state"].shape
    tt = {k: d(v) for k, v in t.items()}
    out = None
    for _ in range(calls):
        out = {k: d(v) for k, v in RS.sentinel_out(t, kw["merge_cap"]).items()}
        mt.plane_refinement_device(G, NP, t["pl_lm"].shape[2], t["lm_owner"].shape[1], tt, d(np.broadcast_to(np.asarray(dist, np.float64), (G,))),
                                   d(np.broadcast_to(np.asarray(err, np.float64), (G,))), out, **kw)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in tt.items()}, {k: v.cpu().numpy() for k, v in out.items()}


def check(t, dist, err, stages=RR.STAGE_ALL, merge_cap=4, forms=("device", "host")):
    """both forms of the entry against the host build; returns the host build's (tables, outputs)"""
    kw = RS.call_kwargs(stages, merge_cap=merge_cap)
    want_t, want_o = run_model(t, dist, err, kw)
    defined = want_o["status"] != RR.OVERFLOW                   # a problem that overflowed has its status and nothing else
    mt = plp.matcher()
    for form in forms:
        got_t, got_o = run_device(mt, t, dist, err, kw) if form == "device" else run_host(mt, t, dist, err, kw)
        assert same(got_o["status"], want_o["status"]), (form, got_o["status"], want_o["status"])
        for k in want_o:
            assert got_o[k].dtype == want_o[k].dtype and same(got_o[k][defined], want_o[k][defined]), (form, k, got_o[k][defined], want_o[k][defined])
        for k in want_t:
            assert got_t[k].dtype == want_t[k].dtype and same(got_t[k][defined], want_t[k][defined]), (form, k)
    return want_t, want_o


def tables_of(spec, seed=1):
    return RS.build(spec, np.random.default_rng(seed))


@pytest.mark.parametrize("stages", [7, 1, 2, 4])
def test_the_census_scenes_in_one_call_each_stage_alone(stages):
    """13 ragged problems: 2, 3, 4, 6 and 11 planes, the runs of invalid rows, a NaN position, a TOO_FEW_PLANES problem at the end"""
    t, dist, err, names = RS.census_call()
    _, o = check(t, dist, err, stages)
    if stages == 7:
        assert o["status"][names.index("too_few_planes")] == RR.TOO_FEW_PLANES and o["num_merges"].sum() >= 6 and o["points_changed"].sum() >= 8
        assert same(o["merges"][names.index("mixed")], np.full((4, 2), RR.SENTINEL["merges"], np.int32))


def test_plane_rows_with_gaps():
    t0, _ = RS.scene_tables("skip_runs")
    _, o = check(RS.pack([RS.with_gaps(t0, [0, 2, 3, 5, 6, 7, 9, 12, 13, 14, 17])], NP_cap=21), RS.DIST, RS.ERR)
    assert o["num_merges"][0] >= 1


def test_lists_around_points_per_ransac_and_twice_that():
    spec = [P(0, 17, NEW), P(1, 18, NEW), P(2, 35), P(3, 36), P(4, 17), P(5, 18)]
    for stages in (7, 2, 4):
        t_, o = check(RS.pack([tables_of(spec)]), RS.DIST, RS.ERR, stages)
        if stages == 2:
            assert o["update_status"][0, 0] == plp.PLANE_TOO_FEW_POINTS and o["num_updates"][0] == 2 and o["removed"][0].tolist() == [0, 0, 2, 0, 2, 2]


def test_lists_at_the_ballot_and_the_workgroup_edge_and_more_updates_than_waves():
    spec = [P(g, n, NEW, erased=3, unowned=2, outliers=4) for g, n in enumerate((63, 64, 65, 255, 256, 257))]
    _, o = check(RS.pack([tables_of(spec)]), RS.DIST, RS.ERR)
    assert o["num_updates"][0] == 6 and (o["update_status"][0] == plp.PLANE_OK).all() and o["planes_changed"][0] == 1


@pytest.mark.parametrize("over", [0, 1])
def test_a_merge_that_lands_on_n_cap_and_one_that_passes_it(over):
    _, o = check(RS.overflow_tables(over), RS.DIST, RS.ERR)
    assert o["status"][0] == (RR.OVERFLOW if over else RR.OK)


def test_more_candidates_than_a_wave_and_a_merge_behind_them():
    spec = [P(0, 40)] + [P(1 + k % 5, 20, DEAD if k % 7 == 3 else RS.LIVE) for k in range(65)] + [P(0, 30)]
    _, o = check(RS.pack([tables_of(spec)]), RS.DIST, RS.ERR, stages=RR.STAGE_MERGE)
    assert o["num_merges"][0] >= 1 and [0, 66] in o["merges"][0].tolist()


@pytest.mark.parametrize("G", [1, 3, 70])
def test_ragged_problems_with_too_few_planes_between_full_ones(G):
    names = ["one_plane_two_lists", "too_few_planes", "equal_sizes", "refine_arms", "too_few_planes", "already_present", "two_planes_apart"]
    ts = [RS.scene_tables(names[g % len(names)], g)[0] for g in range(G)]
    _, o = check(RS.pack(ts), RS.DIST, RS.ERR, forms=("device",) if G == 70 else ("device", "host"))
    assert [int(s) for s in o["status"]] == [RR.TOO_FEW_PLANES if names[g % len(names)] == "too_few_planes" else RR.OK for g in range(G)]


def test_one_landmark():
    t = dict(pl_state=np.full((1, 2), RS.LIVE, np.uint8), pl_equation=np.tile(np.array([0.0, 0.0, 1.0, -1.0]), (1, 2, 1)), pl_best_error=np.ones((1, 2)),
             pl_count=np.ones((1, 2), np.int32), pl_lm=np.array([[[0, RS.PAD], [0, RS.PAD]]], np.int32), pos_w=np.array([[[0.5, 0.25, 1.001]]]),
             lm_erased=np.zeros((1, 1), np.uint8), lm_owner=np.zeros((1, 1), np.int32))
    t_, o = check(t, RS.DIST, RS.ERR)
    assert o["num_merges"][0] == 1 and o["update_status"][0].tolist() == [255, plp.PLANE_TOO_FEW_POINTS] and o["removed"][0].tolist() == [1, 2]


def test_two_calls_on_one_stream():
    t, dist, err, _ = RS.census_call()
    kw = RS.call_kwargs()
    t1, _ = run_model(t, dist, err, kw)
    t2, o2 = run_model(t1, dist, err, kw)
    got_t, got_o = run_device(plp.matcher(), t, dist, err, kw, calls=2)
    defined = (o2["status"] != RR.OVERFLOW)
    assert all(same(got_o[k][defined], o2[k][defined]) for k in o2) and all(same(got_t[k][defined], t2[k][defined]) for k in t2)


def test_bad_arguments_are_refused_before_anything_is_written():
    t = RS.pack([RS.scene_tables("two_planes_apart")[0]])
    mt = plp.matcher()
    for kw in (dict(iters=1025), dict(stages=0), dict(points_per_ransac=0)):
        tt = {k: v.copy() for k, v in t.items()}
        out = RS.sentinel_out(t)
        with pytest.raises(plp.PlpError):
            mt.plane_refinement(tt, RS.DIST, RS.ERR, out=out, **{**RS.call_kwargs(), **kw})
        assert all(same(tt[k], t[k]) for k in t) and all(same(out[k], RS.sentinel_out(t)[k]) for k in out)
