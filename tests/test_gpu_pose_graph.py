"""optimize::graph_optimizer's pose graph on the device (plp_pose_graph_optimize_device / _host, plp_correct_landmarks_*, csrc/pose_graph_kernels.hip)
against the CPU build of the same header (plp.model_pose_graph_optimize, which tests/test_pose_graph_cpu.py holds bit for bit to the restatement
tests/pose_graph_ref.py): every output bit for bit on sentinel-filled device arrays, at the smallest shapes at which the
kernels can go wrong.  The widths the kernels use: the workgroup of 512 lanes (TEAM: the stride of every loop over edges, key frames, rows of the
system and coefficients, and the LDS tile of the chains over the edges), the wave of 64 (WAVE: the ballot of the ordered compactions), one lane per
edge in a pass (edge counts around WAVE and TEAM), one lane per scalar row in the factorisation and the substitutions, whose 7 rows per vertex cross
a wave at 10 vertices of the system and the team at 74, and 256 lanes per workgroup of the landmark correction."""
import numpy as np
import pytest

import pose_graph_ref as REF
import pose_graph_scene as S
from plp import plp

pytestmark = pytest.mark.gpu
TEAM, WAVE, LM_BLOCK = 512, 64, 256       # kPgThreads of csrc/pose_graph.hpp, the wave size, the workgroup of k_pg_correct_landmarks
SHAPES = dict(status=lambda G, F, E: (G,), num_edges=lambda G, F, E: (G,), edges=lambda G, F, E: (G, E, 3), sim3_cw=lambda G, F, E: (G, F, 8),
              corrected_wc=lambda G, F, E: (G, F, 8), pose=lambda G, F, E: (G, F, 15), info=lambda G, F, E: (G, 4), chi2=lambda G, F, E: (G, 2))


@pytest.fixture(scope="module")
def mt():
    return plp.matcher()


def sentinel_out(G, F, E, names=None):
    return {k: np.full(SHAPES[k](G, F, E), REF.SENTINEL[k], plp.POSE_GRAPH_OUTPUTS[k][1]) for k in SHAPES if names is None or k in names}


def host_model(t, prs, edge_cap, env_cap, names=None):
    return plp.model_pose_graph_optimize(t, prs, edge_cap=edge_cap, env_cap=env_cap, outputs=names, out=sentinel_out(len(prs), len(t["kf_parent"]), edge_cap, names))


def enqueue_device(mt, t, prs, edge_cap, env_cap, names=None, keep=None):
    """plp_pose_graph_optimize_device on sentinel-filled device outputs; returns the output tensors (nothing is synchronised)"""
    import torch
    d = lambda v: torch.from_numpy(np.ascontiguousarray(v).copy()).cuda()
    F, G = len(t["kf_parent"]), len(prs)
    o = {k: d(v) for k, v in sentinel_out(G, F, edge_cap, names).items()}
    if keep is not None:
        keep.update(o)
    tables = {k: d(t[k] if np.asarray(t[k]).size else np.zeros(1, np.int32)) for k in plp.POSE_GRAPH_TABLES if t.get(k) is not None}   # a list without an entry: the array is still required
    pr = {k: d(v) if v.size else d(np.zeros(8, v.dtype)) for k, v in plp.pose_graph_problems(prs).items()}
    mt.pose_graph_optimize_device(G, F, tables, pr, o, t["kf_conn"].shape[1], t["kf_covis"].shape[1], edge_cap, env_cap, pose_stride=t["pose"].shape[1])
    return o, (tables, pr)


def check(mt, t, prs, edge_cap, env_cap, names=None):
    import torch
    want = host_model(t, prs, edge_cap, env_cap, names)
    o, _ = enqueue_device(mt, t, prs, edge_cap, env_cap, names)
    torch.cuda.synchronize()
    for k in want:
        assert np.array_equal(o[k].cpu().numpy(), want[k], equal_nan=True), k
    return want


@pytest.mark.parametrize("E", [WAVE - 1, WAVE, WAVE + 1])
def test_edge_counts_around_a_wave(mt, E):
    F = 40
    t, prs, _ = S.ring(F, extra=E - F)
    want = check(mt, t, prs, edge_cap=E, env_cap=1024)
    assert want["status"][0] == REF.OK and want["num_edges"][0] == E == S.edge_count(F, E - F) and want["info"][0, 0] > 0


@pytest.mark.parametrize("E", [TEAM - 1, TEAM, TEAM + 1])
def test_edge_counts_around_the_team(mt, E):
    F = 200
    t, prs, _ = S.ring(F, extra=E - F)
    want = check(mt, t, prs, edge_cap=E, env_cap=4096)
    assert want["status"][0] == REF.OK and want["num_edges"][0] == E and want["info"][0, 3] == F - 1


@pytest.mark.parametrize("fix_scale", [False, True])
@pytest.mark.parametrize("n", [1, 9, 10, 11, 73, 74])
def test_vertices_of_the_system_around_a_wave_and_the_team_of_rows(mt, n, fix_scale):
    F = n + 1                                                # the loop key frame is fixed; F = 2: one free vertex
    t, prs, _ = S.ring(F, extra=min(4, max(F - 2, 0)), fix_scale=fix_scale)
    want = check(mt, t, prs, edge_cap=128, env_cap=1024)
    assert want["status"][0] == REF.OK and want["info"][0, 3] == n and (7 * n > WAVE) == (n >= 10) and (7 * n > TEAM) == (n >= 74)
    if fix_scale:
        assert np.array_equal(want["corrected_wc"][0, :, 7], np.ones(F))


@pytest.mark.parametrize("arrow", [False, True])
def test_band_and_arrow_envelopes(mt, arrow):
    F = 30
    t, prs, _ = S.ring(F, extra=2 * F - 5, arrow=arrow)
    g = REF.Graph(t, prs[0])
    width = [i - f for i, f in enumerate(g.first)]
    assert max(width[:-1]) == 3 and (width[-1] == len(width) - 1 if arrow else width[-1] <= 3)       # a band of three blocks; the arrow's last row starts at row 1's vertex, the first of the system
    n_env = sum(w + 1 for w in width)
    want = check(mt, t, prs, edge_cap=128, env_cap=n_env)
    assert want["status"][0] == REF.OK and want["num_edges"][0] == S.edge_count(F, 2 * F - 5, arrow)
    # one block fewer than the envelope needs: a status of the problem, which the device alone can see
    want = check(mt, t, prs, edge_cap=128, env_cap=n_env - 1)
    assert want["status"][0] == REF.ENVELOPE_TOO_LARGE and (want["pose"] == REF.SENTINEL["pose"]).all()


def test_three_problems_over_one_table_and_the_census(mt):
    F = 20
    t, prs, gt = S.ring(F, extra=12)
    prs = [dict(prs[0]), dict(prs[0], loop_kf=5, fix_scale=True), dict(prs[0], loop_kf=F - 3, pre_corrected={}, non_corrected={}, loop_connections={F - 1: {F - 3}})]
    want = check(mt, t, prs, edge_cap=64, env_cap=512)
    assert (want["status"] == REF.OK).all() and not np.array_equal(want["pose"][0], want["pose"][1]) and not np.array_equal(want["pose"][0], want["pose"][2])
    t, prs = S.census()
    want = check(mt, t, prs, edge_cap=40, env_cap=512)
    assert want["status"].tolist() == [REF.OK, REF.OK, REF.BAD_LOOP_KF]


def test_optional_outputs_absent_and_too_many_edges(mt):
    t, prs, _ = S.ring(12, extra=5)
    check(mt, t, prs, edge_cap=32, env_cap=256, names=("status", "pose"))
    check(mt, t, prs, edge_cap=32, env_cap=256, names=("status",))
    want = check(mt, t, prs, edge_cap=S.edge_count(12, 5) - 1, env_cap=256)
    assert want["status"][0] == REF.TOO_MANY_EDGES and want["num_edges"][0] == S.edge_count(12, 5)


def test_a_cap_exceeded_is_refused_with_nothing_written(mt):
    import torch
    t, prs, _ = S.ring(12, extra=5)
    for kw in (dict(edge_cap=plp.POSE_GRAPH_MAX_EDGES + 1, env_cap=64), dict(edge_cap=32, env_cap=plp.POSE_GRAPH_MAX_ENV + 1)):
        keep = {}
        with pytest.raises(plp.PlpError) as e:
            enqueue_device(mt, t, prs, names=("status", "num_edges", "pose", "info"), keep=keep, **kw)
        assert e.value.status == plp.PLP_ERR_UNSUPPORTED
        torch.cuda.synchronize()
        sent = sentinel_out(1, 12, 1, names=tuple(keep))
        assert all(np.array_equal(keep[k].cpu().numpy(), sent[k]) for k in keep)
    with pytest.raises(plp.PlpError) as e:
        enqueue_device(mt, t, prs * (plp.POSE_GRAPH_MAX_PROBLEMS + 1), 32, 64, names=("status",))
    assert e.value.status == plp.PLP_ERR_UNSUPPORTED


def test_host_pointer_entry_equals_the_device_entry(mt):
    t, prs, _ = S.ring(16, extra=9, arrow=True)
    want = host_model(t, prs, 48, 512)
    got = mt.pose_graph_optimize(t, prs, edge_cap=48, env_cap=512, out=sentinel_out(1, 16, 48))
    for k in want:
        assert np.array_equal(got[k], want[k], equal_nan=True), k
    r = plp.graph_optimizer(t, False, mt=mt, edge_cap=48, env_cap=512).optimize(0, 15, prs[0]["non_corrected"], prs[0]["pre_corrected"], prs[0]["loop_connections"])
    assert np.array_equal(r["pose"], want["pose"][0])


@pytest.mark.parametrize("L", [2 * LM_BLOCK - 1, 2 * LM_BLOCK, 2 * LM_BLOCK + 1])
def test_correct_landmarks_around_a_workgroup(mt, L):
    import torch
    F = 12
    t, prs, _ = S.ring(F, extra=5)
    r = host_model(t, prs, 32, 256)
    erased = np.zeros(F, np.uint8)
    erased[4] = 1
    pos, ref, er = S.landmarks(F, L)
    want = plp.model_correct_landmarks(pos, ref, r["sim3_cw"][0], r["corrected_wc"][0], lm_erased=er, kf_erased=erased,
                                       out=dict(pos_w=np.full((L, 3), -7.25), status=np.full(L, 0xEE, np.uint8)))
    assert set(want["status"].tolist()) == {REF.LM_OK, REF.LM_ERASED, REF.LM_NO_VERTEX}
    d = lambda v: torch.from_numpy(np.ascontiguousarray(v).copy()).cuda()
    o_pos, o_st = d(np.full((L, 3), -7.25)), d(np.full(L, 0xEE, np.uint8))
    mt.correct_landmarks_device(L, F, d(pos), d(ref), d(r["sim3_cw"][0]), d(r["corrected_wc"][0]), o_pos, o_st, lm_erased=d(er), kf_erased=d(erased))
    torch.cuda.synchronize()
    assert np.array_equal(o_pos.cpu().numpy(), want["pos_w"]) and np.array_equal(o_st.cpu().numpy(), want["status"])
    got = mt.correct_landmarks(pos, ref, r["sim3_cw"][0], r["corrected_wc"][0], lm_erased=er, kf_erased=erased,
                               out=dict(pos_w=np.full((L, 3), -7.25), status=np.full(L, 0xEE, np.uint8)))
    assert np.array_equal(got["pos_w"], want["pos_w"]) and np.array_equal(got["status"], want["status"])
    # in place: the positions are their own output
    p_dev = d(pos)
    mt.correct_landmarks_device(L, F, p_dev, d(ref), d(r["sim3_cw"][0]), d(r["corrected_wc"][0]), p_dev, o_st, lm_erased=d(er), kf_erased=d(erased))
    torch.cuda.synchronize()
    ok = want["status"] == REF.LM_OK
    assert np.array_equal(p_dev.cpu().numpy()[ok], want["pos_w"][ok]) and np.array_equal(p_dev.cpu().numpy()[~ok], pos[~ok])
