"""data::graph_node on the device (plp_covisibility_update_* / plp_covisibility_erase_*, csrc/covisibility_kernels.hip) against the object-level
restatement tests/covisibility_ref.py and the host build, on the scenes tests/test_covisibility_cpu.py holds the host build to: exact equality of
every state table and every output, over sentinel-filled outputs and state rows with a sentinel behind their last entry.  The widths the kernels
use are in the scenes: F = 5, 70, 300 and 1100 key frames against the wave of 64 and the workgroup's stride of 256 lanes (the tables of F
counters, the compaction tiles, the owners dealt to the lanes of k_covis_apply when G = F)."""
import numpy as np
import pytest

import covisibility_ref as R
import covisibility_scene as S
from plp import plp
from test_covisibility_cpu import LISTS, MASKS, cut_scene, equal, erased, row_caps, sentinels, updated
from test_gpu_map_cull import to_device

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mt():
    return plp.matcher()


def dims_of(sc, state, G):
    return dict(F=sc["kf_lm"].shape[0], L=len(sc["obs_offsets"]) - 1, T=sc.get("T", len(sc["obs_kf"])), cap=sc["kf_lm"].shape[1],
                conn_cap=state["kf_conn"].shape[1], covis_cap=state["kf_covis"].shape[1], G=G)


def enqueue(mt, sc, before, owners, want, shift=False, drop=(), drop_out=()):
    """plp_covisibility_update_device on device copies of the state `before` and sentinel-filled device outputs; nothing is synchronised"""
    dev = {k: to_device(sc[k], shift) for k in S.TABLES if k not in drop}
    dev["owners"] = to_device(np.asarray(owners, np.int32), shift)
    state = {k: to_device(v, shift) for k, v in before.items()}
    out = {k: to_device(v, shift) for k, v in sentinels(want).items()}
    mt.covisibility_update_device(dims_of(sc, before, len(owners)), dict(dev, **state), {k: v for k, v in out.items() if k not in drop_out})
    return out, state, dev


def fetch(dev, want):
    import torch
    torch.cuda.synchronize()
    return {k: dev[k].cpu().numpy().reshape(want[k].shape).view(want[k].dtype) for k in want}


def problem(name, which):
    sc = S.scene(name)
    res, g = updated(name, which)
    cc, vc = row_caps(sc["graph"], g)
    before = R.with_slack(R.tables(sc["graph"], cc, vc))
    return sc, before, R.expected_update(res, g, len(g.connected)), R.expected_state(before, g, cc, vc)


@pytest.mark.parametrize("which", LISTS)
@pytest.mark.parametrize("name", S.SCENES)
def test_device_update_equals_restatement(mt, name, which):
    sc, before, want, want_state = problem(name, which)
    out, state, _ = enqueue(mt, sc, before, sc["owners"][which], want)
    equal(fetch(out, want), want, (name, which))
    equal(fetch(state, want_state), want_state, (name, which, "state"))


@pytest.mark.parametrize("which", ["three", "all"])
@pytest.mark.parametrize("name", S.SCENES)
def test_host_entry_update_equals_restatement_and_host_build(mt, name, which):
    sc, before, want, want_state = problem(name, which)
    state = {k: v.copy() for k, v in before.items()}
    equal(mt.covisibility_update(state=state, owners=sc["owners"][which], out=sentinels(want), **S.call_args(sc)), want, (name, which))
    equal(state, want_state, (name, which, "state"))
    model = {k: v.copy() for k, v in before.items()}
    equal(plp.model_covisibility_update(state=model, owners=sc["owners"][which], out=sentinels(want), **S.call_args(sc)), want, "host build")
    equal(state, model, "host build, state")


def erase_problem(name, which):
    g0 = updated(name, "stale")[1]
    mask, g = erased(name, which)
    cc, vc = row_caps(g0, g)
    before = {k: v for k, v in R.with_slack(R.tables(g0, cc, vc)).items() if k in plp.COVISIBILITY_ERASE_STATE}
    return mask, before, R.expected_erase(g, len(mask)), R.expected_state(before, g, cc, vc)


@pytest.mark.parametrize("which", MASKS)
@pytest.mark.parametrize("name", S.SCENES)
def test_erase_equals_restatement(mt, name, which):
    mask, before, want, want_state = erase_problem(name, which)
    state = {k: to_device(v) for k, v in before.items()}
    out = {k: to_device(v) for k, v in sentinels(want).items()}
    F, cc, vc = len(mask), before["kf_conn"].shape[1], before["kf_covis"].shape[1]
    mt.covisibility_erase_device(dict(F=F, conn_cap=cc, covis_cap=vc), dict(state, erased=to_device(mask)), out)
    equal(fetch(out, want), want, (name, which))
    equal(fetch(state, want_state), want_state, (name, which, "state"))
    host = {k: v.copy() for k, v in before.items()}
    equal(mt.covisibility_erase(host, mask, out=sentinels(want)), want, (name, which, "host entry"))
    equal(host, want_state, (name, which, "host entry, state"))


def test_duplicate_and_absent_owners(mt):
    """the device entry alone takes such a list: the repeats and the rows outside the table are named and not processed"""
    sc = S.scene("f300")
    F = sc["kf_lm"].shape[0]
    owners = [F - 1, 7, F + 2, 7, 8, -1, F - 1, 9, 8]
    g = sc["graph"].copy()
    res = R.run_update(g, sc, owners)
    assert [r[0] for r in res].count(R.DUPLICATE) == 3 and [r[0] for r in res].count(R.ROW_ABSENT) == 2
    cc, vc = row_caps(sc["graph"], g)
    before = R.with_slack(R.tables(sc["graph"], cc, vc))
    want, want_state = R.expected_update(res, g, F), R.expected_state(before, g, cc, vc)
    out, state, _ = enqueue(mt, sc, before, owners, want)
    equal(fetch(out, want), want, "duplicates")
    equal(fetch(state, want_state), want_state, "duplicates, state")
    with pytest.raises(plp.PlpError) as e:
        mt.covisibility_update(state={k: v.copy() for k, v in before.items()}, owners=owners, **S.call_args(sc))
    assert e.value.status == plp.PLP_ERR_INVALID_ARG


def test_runs_cut_at_T(mt):
    """T one third into the observation table: a run that crosses it is cut, a run behind it is empty"""
    sc = cut_scene()
    g = sc["graph"].copy()
    owners = sc["owners"]["all"]
    res = R.run_update(g, sc, owners)
    cc, vc = row_caps(sc["graph"], g)
    before = R.with_slack(R.tables(sc["graph"], cc, vc))
    want, want_state = R.expected_update(res, g, len(g.connected)), R.expected_state(before, g, cc, vc)
    out, state, _ = enqueue(mt, sc, before, owners, want)
    equal(fetch(out, want), want, "cut")
    equal(fetch(state, want_state), want_state, "cut, state")


def test_misaligned_bases(mt):
    """every base one element past an allocation's"""
    sc, before, want, want_state = problem("f70", "all")
    out, state, _ = enqueue(mt, sc, before, sc["owners"]["all"], want, shift=True)
    equal(fetch(out, want), want, "shifted")
    equal(fetch(state, want_state), want_state, "shifted, state")


def test_null_optionals(mt):
    """without the optional outputs their sentinel-filled arrays stay as they are; NULL kf_counts is the cap and NULL lm_erased none"""
    sc, before, want, want_state = problem("f70", "three")
    out, state, _ = enqueue(mt, sc, before, sc["owners"]["three"], want, drop_out=("nearest", "max_weight", "touched"))
    got = fetch(out, want)
    for k in ("nearest", "max_weight", "touched"):
        assert (got[k] == R.SENTINEL[k]).all(), k
    assert np.array_equal(got["status"], want["status"])
    equal(fetch(state, want_state), want_state, "no optional outputs, state")
    nul = dict(sc, kf_counts=None, lm_erased=None)
    g = sc["graph"].copy()
    res = R.run_update(g, nul, sc["owners"]["all"])
    cc, vc = row_caps(sc["graph"], g)
    before = R.with_slack(R.tables(sc["graph"], cc, vc))
    nwant, nstate = R.expected_update(res, g, len(g.connected)), R.expected_state(before, g, cc, vc)
    out, state, _ = enqueue(mt, nul, before, sc["owners"]["all"], nwant, drop=("kf_counts", "lm_erased"))
    equal(fetch(out, nwant), nwant, "NULL tables")
    equal(fetch(state, nstate), nstate, "NULL tables, state")


def test_no_owner_writes_nothing(mt):
    sc, before, want, _ = problem("f70", "one")
    out, state, _ = enqueue(mt, sc, before, [], {k: v[:0] if k != "touched" else v for k, v in want.items()})
    import torch
    torch.cuda.synchronize()
    assert (out["touched"].cpu().numpy() == R.SENTINEL["touched"]).all()
    equal(fetch(state, before), before, "G == 0")


def test_two_calls_on_one_context_at_different_sizes(mt):
    """the context's scratch serves both calls, the larger one first; one synchronisation at the end"""
    a, b = problem("f1100", "all"), problem("f5", "all")
    oa, sa, keep_a = enqueue(mt, a[0], a[1], a[0]["owners"]["all"], a[2])
    ob, sb, keep_b = enqueue(mt, b[0], b[1], b[0]["owners"]["all"], b[2])
    oa2, sa2, keep_a2 = enqueue(mt, a[0], a[1], a[0]["owners"]["all"], a[2])
    for out, state, p, what in ((oa, sa, a, "first"), (ob, sb, b, "second"), (oa2, sa2, a, "third")):
        equal(fetch(out, p[2]), p[2], what)
        equal(fetch(state, p[3]), p[3], (what, "state"))


@pytest.mark.parametrize("which", ["conn", "covis"])
def test_overflow_equals_host_build(mt, which):
    """every key frame of f300 an owner over an empty graph with one table too short: the device's tables and outputs are the host build's, which
    tests/test_covisibility_cpu.py holds to the restatement"""
    sc = S.scene("f300")
    F = sc["kf_lm"].shape[0]
    g = R.graph(F)
    R.run_update(g, sc, sc["owners"]["all"])
    cc, vc = S.caps(g)
    cc, vc = (sorted(len(c) for c in g.connected)[F // 3], vc) if which == "conn" else (cc, 2)
    before = R.with_slack(R.tables(R.graph(F), cc, vc))
    model = {k: v.copy() for k, v in before.items()}
    want = plp.model_covisibility_update(state=model, owners=sc["owners"]["all"], **S.call_args(sc))
    assert (want["touched"] == 2).any() and (want["status"] == plp.COVIS_OVERFLOW).any()
    out, state, _ = enqueue(mt, sc, before, sc["owners"]["all"], want)
    equal(fetch(out, want), want, which)
    equal(fetch(state, model), model, (which, "state"))


def test_mirror_class_on_the_device(mt):
    sc = S.scene("f70")
    F = sc["kf_lm"].shape[0]
    g = R.graph(F)
    res = R.run_update(g, sc, sc["owners"]["all"])
    cg = plp.covisibility_graph(F, conn_cap=2, covis_cap=2, mt=mt)
    status = cg.update_connections(sc["owners"]["all"], **S.call_args(sc))
    assert [int(v) for v in status] == [r[0] for r in res]
    R.run_erase(g, np.isin(np.arange(F), sc["erase"]["pair"]))
    cg.erase_all_connections(sc["erase"]["pair"])
    for k in range(F):
        assert cg.get_covisibilities(k) == g.get_covisibilities(k) and cg.get_connected_keyframes(k) == g.get_connected_keyframes(k)
        assert cg.get_covisibilities_over_weight(k, 20) == g.get_covisibilities_over_weight(k, 20) and cg.get_spanning_parent(k) == g.parent[k]
