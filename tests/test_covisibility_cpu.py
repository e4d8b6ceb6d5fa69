"""plp_model_covisibility_update_host and plp_model_covisibility_erase_host (the host build of csrc/covisibility.hpp, a team of one lane) against
the object-level restatement of data::graph_node in tests/covisibility_ref.py: exact equality of every state table and every output.  The outputs
start filled with sentinels and the state rows carry a sentinel behind their last entry, so that what the library leaves unwritten is checked
too.  The library computes D21's closed form and the restatement mutates objects one call after another, so equality here
is the proof of the closed form; the census shows that the committed scenes reach every case D21 names."""
import importlib

import numpy as np
import pytest

import covisibility_ref as R
import covisibility_scene as S

plp = importlib.import_module("structure-plp-slam_amd")

_results, _events = {}, set()
LISTS = ("one", "three", "all", "stale")
MASKS = ("one", "pair", "many")


def updated(name, which):
    """the restatement of one owner list over a scene's initial graph, computed once: (per-owner results, the graph afterwards)"""
    if (name, which) not in _results:
        sc = S.scene(name)
        g = sc["graph"].copy()
        _results[(name, which)] = (R.run_update(g, sc, sc["owners"][which], _events), g)
    return _results[(name, which)]


def erased(name, which):
    """the restatement of one erase mask over the graph the `stale` list leaves"""
    if (name, "erase", which) not in _results:
        sc = S.scene(name)
        g = updated(name, "stale")[1].copy()
        mask = np.zeros(len(g.connected), np.uint8)
        mask[sc["erase"][which]] = 1
        R.run_erase(g, mask, _events)
        _results[(name, "erase", which)] = (mask, g)
    return _results[(name, "erase", which)]


def sentinels(want):
    return {k: np.full_like(v, R.SENTINEL[k]) for k, v in want.items()}


def equal(got, want, what):
    assert set(got) == set(want), what
    for k in want:
        assert np.array_equal(got[k], want[k]), (what, k, np.argwhere(got[k] != want[k])[:4].tolist())


def row_caps(*graphs):
    c = [S.caps(g) for g in graphs]
    return max(v[0] for v in c), max(v[1] for v in c)


def check_update(fn, name, which, **over):
    sc = S.scene(name)
    res, g = updated(name, which)
    cc, vc = row_caps(sc["graph"], g)
    before = R.with_slack(R.tables(sc["graph"], cc, vc))
    state = {k: v.copy() for k, v in before.items()}
    want = R.expected_update(res, g, len(g.connected))
    got = fn(state=state, owners=sc["owners"][which], out=sentinels(want), **S.call_args(sc, **over))
    equal(got, want, (name, which))
    equal(state, R.expected_state(before, g, cc, vc), (name, which, "state"))
    return want


def check_erase(fn, name, which):
    g0 = updated(name, "stale")[1]
    mask, g = erased(name, which)
    cc, vc = row_caps(g0, g)
    before = R.with_slack(R.tables(g0, cc, vc))
    state = {k: before[k].copy() for k in plp.COVISIBILITY_ERASE_STATE}
    want = R.expected_erase(g, len(mask))
    equal(fn(state=state, erased=mask, out=sentinels(want)), want, (name, which))
    equal(state, R.expected_state({k: before[k] for k in state}, g, cc, vc), (name, which, "state"))


@pytest.mark.parametrize("which", LISTS)
@pytest.mark.parametrize("name", S.SCENES)
def test_host_build_update_equals_restatement(name, which):
    check_update(plp.model_covisibility_update, name, which)


@pytest.mark.parametrize("which", MASKS)
@pytest.mark.parametrize("name", S.SCENES)
def test_host_build_erase_equals_restatement(name, which):
    check_erase(plp.model_covisibility_erase, name, which)


def queries(name):
    """the four queries of every key frame on the restatement; the census of get_covisibilities_over_weight"""
    g = updated(name, "all")[1]
    for k in range(len(g.connected)):
        for w in (1, 16, 20, 10 ** 6):
            g.get_covisibilities_over_weight(k, w, _events)
    return g


CENSUS = ("no_shared", "single_node_below_thr", "weight_14", "weight_15", "weight_16", "weight_17", "tie_at_max_weight", "tie_among_pairs",
          "back_edge_equal_weight", "back_edge_equal_weight_list_stays_thresholded", "back_edge_changes_stale_weight",
          "rebuilt_list_shows_entries_at_or_below_thr", "mutual_owners_low_row_first", "mutual_owners_high_row_first",
          "empty_owner_receives_before_and_after", "slot_none", "landmark_erased", "landmark_row_outside_table", "observer_row_outside_table",
          "landmark_in_two_slots", "run_cut_at_T", "parent_set", "parent_id_0", "parent_flag_already_clear", "erase_one",
          "erase_mutually_connected_pair", "stale_one_sided_entry_survives", "erase_target_does_not_hold_me", "over_weight_proper_prefix",
          "over_weight_all_qualify_returns_empty")


def cut_scene(name="f70"):
    """the snapshot with T one third into the observation table: the runs behind it are cut or empty (the device entry alone takes such a T)"""
    sc = S.scene(name)
    return dict(sc, T=len(sc["obs_kf"]) // 3)


def test_census_of_the_scenes():
    """on the restatement alone: every case D21 names happens in a committed scene"""
    for name in S.SCENES:
        for which in LISTS:
            updated(name, which)
        for which in MASKS:
            erased(name, which)
        queries(name)
    sc = cut_scene()
    R.run_update(sc["graph"].copy(), sc, sc["owners"]["all"], _events)
    assert not [c for c in CENSUS if c not in _events]


def test_scene_sizes():
    """the sizes the kernels' loops treat apart are in the scenes"""
    assert [S.scene(n)["kf_lm"].shape[0] for n in S.SCENES] == [5, 70, 300, 1100]
    for name in S.SCENES:
        sc = S.scene(name)
        assert 48 <= sc["kf_lm"].shape[1] <= 96
        assert {len(v) for k, v in sc["owners"].items() if k != "stale"} == {1, 3, sc["kf_lm"].shape[0]}
    n = np.diff(S.scene("f1100")["obs_offsets"])
    assert n.min() == 0 and n.max() == 40 and len(set(int(v) for v in n)) > 20


def test_no_shared_owner_leaves_its_row_bit_for_bit():
    """f70's key frame without a slot of its own: NO_SHARED, and its row -- which the owners before it in the list wrote into -- is the
    restatement's, slack and all where nothing was written"""
    sc = S.scene("f70")
    res, g = updated("f70", "all")
    at = sc["owners"]["all"].index(sc["z"])
    assert res[at] == (R.NO_SHARED, -1, 0) and g.connected[sc["z"]]
    alone = sc["graph"].copy()
    out = R.run_update(alone, sc, [sc["z"]])
    assert out == [(R.NO_SHARED, -1, 0)] and not alone.written
    cc, vc = row_caps(alone)
    before = R.with_slack(R.tables(alone, cc, vc))
    state = {k: v.copy() for k, v in before.items()}
    got = plp.model_covisibility_update(state=state, owners=[sc["z"]], **S.call_args(sc))
    assert got["status"][0] == plp.COVIS_NO_SHARED and not got["touched"].any()
    equal(state, before, "untouched")


@pytest.mark.parametrize("which", ["conn", "covis"])
@pytest.mark.parametrize("name", ["f5", "f70", "f300"])
def test_overflow_of_each_cap(name, which):
    """every key frame an owner over an empty graph, one table too short.  A short ordered table loses nothing but its tail: every table and every
    count is the restatement's, the rows that outgrew it carry 2.  A short connected table costs the rows named 2 their validity; every other row
    is the restatement's"""
    sc = S.scene(name)
    F = sc["kf_lm"].shape[0]
    g = R.graph(F)
    res = R.run_update(g, sc, sc["owners"]["all"])
    cc, vc = S.caps(g)
    lens = sorted(len(c) for c in g.connected)
    cc, vc = (max(lens[0], lens[F // 3] - 1), vc) if which == "conn" else (cc, 2)    # a third of the rows fit the short connected table
    before = R.with_slack(R.tables(R.graph(F), cc, vc))
    state = {k: v.copy() for k, v in before.items()}
    got = plp.model_covisibility_update(state=state, owners=sc["owners"]["all"], **S.call_args(sc))
    want, want_out = R.expected_state(before, g, cc, vc), R.expected_update(res, g, F)
    n_conn, n_covis = want["kf_n_conn"], want["kf_n_covis"]
    pos = {k: i for i, k in enumerate(sc["owners"]["all"])}
    assert (got["touched"] == 2).any() and (got["status"] == plp.COVIS_OVERFLOW).any()
    if which == "covis":
        over = n_covis > vc
        want_out["touched"][over] = 2
        for k in np.flatnonzero(over):
            if want_out["status"][pos[int(k)]] == R.OK:
                want_out["status"][pos[int(k)]] = R.OVERFLOW
        equal(got, want_out, (name, which))
        equal(state, want, (name, which, "state"))
        return
    good = got["touched"] != 2
    assert ((n_conn > cc) <= ~good).all() and good.any()
    assert (state["kf_n_conn"][n_conn > cc] > cc).all()
    for k in want:
        assert np.array_equal(state[k][good], want[k][good]), k
    assert np.array_equal(got["touched"][good], want_out["touched"][good])
    for k in np.flatnonzero(good):
        if want_out["status"][pos[int(k)]] == R.OK:
            assert got["status"][pos[int(k)]] == R.OK


def test_mirror_class_regrows_and_answers_the_queries():
    """data::graph_node's surface over rows, on the host build, from tables of two slots: the overflow protocol, then every query"""
    sc = S.scene("f70")
    F = sc["kf_lm"].shape[0]
    g = R.graph(F)
    res = R.run_update(g, sc, sc["owners"]["all"])
    cg = plp.covisibility_graph(F, conn_cap=2, covis_cap=2)
    status = cg.update_connections(sc["owners"]["all"], **S.call_args(sc))
    assert [int(v) for v in status] == [r[0] for r in res]
    for k in range(F):
        assert cg.get_covisibilities(k) == g.get_covisibilities(k)
        assert cg.get_top_n_covisibilities(k, 10) == g.get_top_n_covisibilities(k, 10)
        assert cg.get_connected_keyframes(k) == g.get_connected_keyframes(k)
        for w in (1, 16, 20, 10 ** 6):
            assert cg.get_covisibilities_over_weight(k, w) == g.get_covisibilities_over_weight(k, w), (k, w)
        assert cg.get_spanning_parent(k) == g.parent[k]
    for a, b in ((0, 1), (1, 0), (3, 60), (sc["z"], sc["z"] + 1)):
        assert cg.get_weight(a, b) == g.get_weight(a, b)
    R.run_erase(g, np.isin(np.arange(F), sc["erase"]["pair"]))
    cg.erase_all_connections(sc["erase"]["pair"])
    want = R.tables(g, cg.state["kf_conn"].shape[1], cg.state["kf_covis"].shape[1])
    equal({k: cg.state[k] for k in plp.COVISIBILITY_ERASE_STATE}, {k: want[k] for k in plp.COVISIBILITY_ERASE_STATE}, "after the erase")


def test_chained_sequence():
    """the mapping loop's calls on one state: the new key frame, the neighbours after a fusion with changed tables, an erase, an update again;
    the state is carried through the calls and compared after each one"""
    sc = S.scene("f300")
    F = sc["kf_lm"].shape[0]
    g = sc["graph"].copy()
    cc, vc = 140, 140
    state = R.with_slack(R.tables(g, cc, vc))
    fused = dict(sc, lm_erased=np.where(np.arange(len(sc["lm_erased"])) % 7 == 0, 1, sc["lm_erased"]).astype(np.uint8))
    gone = np.zeros(F, np.uint8)
    gone[[F - 2, 40]] = 1
    steps = [("update", sc, [F - 1]), ("update", fused, list(range(F - 12, F))), ("erase", gone, None), ("update", fused, [F - 4, 41, 39, F - 1])]
    for i, (what, arg, owners) in enumerate(steps):
        before = {k: v.copy() for k, v in state.items()}
        if what == "update":
            res = R.run_update(g, arg, owners)
            want = R.expected_update(res, g, F)
            equal(plp.model_covisibility_update(state=state, owners=owners, out=sentinels(want), **S.call_args(arg)), want, i)
        else:
            R.run_erase(g, arg)
            want = R.expected_erase(g, F)
            equal(plp.model_covisibility_erase({k: state[k] for k in plp.COVISIBILITY_ERASE_STATE}, arg, out=sentinels(want)), want, i)
        equal(state, R.expected_state(before, g, cc, vc), (i, "state"))


def _update_struct(**over):
    """a well-formed plp_covisibility_update_args over one tiny problem, every pointer at an array of its own"""
    n = lambda dt, k: np.zeros(k, dt)
    arrs = dict(kf_lm=n(np.int32, 8), obs_offsets=n(np.int32, 4), obs_kf=n(np.int32, 1), kf_id=n(np.uint32, 2), kf_conn=n(np.int32, 6),
                kf_conn_w=n(np.int32, 6), kf_n_conn=n(np.int32, 2), kf_covis=n(np.int32, 4), kf_covis_w=n(np.int32, 4), kf_n_covis=n(np.int32, 2),
                kf_parent=n(np.int32, 2), kf_parent_unset=n(np.uint8, 2), owners=np.array([0, 1], np.int32), out_status=np.full(2, 0xEE, np.uint8))
    arrs["obs_offsets"][3] = 1
    a = plp.covisibility_update_args_c()
    for k, v in dict(F=2, L=3, T=1, cap=4, conn_cap=3, covis_cap=2, G=2).items():
        setattr(a, k, v)
    for k, v in arrs.items():
        setattr(a, k, v.ctypes.data)
    for k, v in over.items():
        setattr(a, k, v)
    return a, arrs


UP_INVALID = [dict(F=-1), dict(L=-1), dict(T=-1), dict(cap=-1), dict(conn_cap=-1), dict(covis_cap=-1), dict(G=-1)] + [
    {k: None} for k in ("kf_lm", "obs_offsets", "obs_kf", "kf_id", "kf_conn", "kf_conn_w", "kf_n_conn", "kf_covis", "kf_covis_w", "kf_n_covis",
                        "kf_parent", "kf_parent_unset", "owners", "out_status")]
UP_UNSUPPORTED = [dict(F=8193), dict(cap=8193), dict(conn_cap=8193), dict(covis_cap=8193), dict(G=8193)]


@pytest.mark.parametrize("i", range(len(UP_INVALID) + len(UP_UNSUPPORTED)))
def test_update_argument_checks(i):
    bad = (UP_INVALID + UP_UNSUPPORTED)[i]
    a, arrs = _update_struct(**bad)
    want = plp.PLP_ERR_INVALID_ARG if i < len(UP_INVALID) else plp.PLP_ERR_UNSUPPORTED
    assert plp.lib().plp_model_covisibility_update_host(plp.C.byref(a)) == -want, bad
    assert (arrs["out_status"] == 0xEE).all()
    a, arrs = _update_struct()
    assert plp.lib().plp_model_covisibility_update_host(plp.C.byref(a)) == 2 and (arrs["out_status"] == plp.COVIS_NO_SHARED).all()
    assert plp.lib().plp_model_covisibility_update_host(None) == -plp.PLP_ERR_INVALID_ARG


def test_update_refuses_bad_offsets_and_a_duplicate_owner():
    for bad in ([0, 2, 1, 1], [1, 1, 1, 1], [0, 0, 0, 2]):
        a, arrs = _update_struct()
        arrs["obs_offsets"][:] = bad
        assert plp.lib().plp_model_covisibility_update_host(plp.C.byref(a)) == -plp.PLP_ERR_INVALID_ARG, bad
    a, arrs = _update_struct()
    arrs["owners"][:] = [1, 1]
    assert plp.lib().plp_model_covisibility_update_host(plp.C.byref(a)) == -plp.PLP_ERR_INVALID_ARG
    assert (arrs["out_status"] == 0xEE).all()


def test_update_conventions():
    """G == 0 writes nothing; an owner outside the table is ROW_ABSENT, also when there is no key frame at all"""
    a, arrs = _update_struct(G=0, owners=None, out_status=None)
    assert plp.lib().plp_model_covisibility_update_host(plp.C.byref(a)) == 0
    a, arrs = _update_struct()
    arrs["owners"][:] = [2, -1]
    assert plp.lib().plp_model_covisibility_update_host(plp.C.byref(a)) == 2 and (arrs["out_status"] == plp.COVIS_ROW_ABSENT).all()
    a, arrs = _update_struct(F=0)
    assert plp.lib().plp_model_covisibility_update_host(plp.C.byref(a)) == 2 and (arrs["out_status"] == plp.COVIS_ROW_ABSENT).all()


def _erase_struct(**over):
    n = lambda dt, k: np.zeros(k, dt)
    arrs = dict(kf_conn=n(np.int32, 6), kf_conn_w=n(np.int32, 6), kf_n_conn=n(np.int32, 2), kf_covis=n(np.int32, 4), kf_covis_w=n(np.int32, 4),
                kf_n_covis=n(np.int32, 2), erased=n(np.uint8, 2), out_status=np.full(2, 0xEE, np.uint8))
    a = plp.covisibility_erase_args_c()
    a.F, a.conn_cap, a.covis_cap = 2, 3, 2
    for k, v in arrs.items():
        setattr(a, k, v.ctypes.data)
    for k, v in over.items():
        setattr(a, k, v)
    return a, arrs


ER_BAD = [(dict(F=-1), "I"), (dict(conn_cap=-1), "I"), (dict(covis_cap=-1), "I"), (dict(F=8193), "U"), (dict(conn_cap=8193), "U"),
          (dict(covis_cap=8193), "U")] + [({k: None}, "I") for k in ("kf_conn", "kf_conn_w", "kf_n_conn", "kf_covis", "kf_covis_w", "kf_n_covis",
                                                                     "erased", "out_status")]


@pytest.mark.parametrize("i", range(len(ER_BAD)))
def test_erase_argument_checks(i):
    bad, kind = ER_BAD[i]
    a, arrs = _erase_struct(**bad)
    want = plp.PLP_ERR_INVALID_ARG if kind == "I" else plp.PLP_ERR_UNSUPPORTED
    assert plp.lib().plp_model_covisibility_erase_host(plp.C.byref(a)) == -want, bad
    assert (arrs["out_status"] == 0xEE).all()
    a, arrs = _erase_struct()
    assert plp.lib().plp_model_covisibility_erase_host(plp.C.byref(a)) == 2 and (arrs["out_status"] == plp.COVIS_OK).all()
    a, arrs = _erase_struct(F=0)
    assert plp.lib().plp_model_covisibility_erase_host(plp.C.byref(a)) == 0 and (arrs["out_status"] == 0xEE).all()
    assert plp.lib().plp_model_covisibility_erase_host(None) == -plp.PLP_ERR_INVALID_ARG
