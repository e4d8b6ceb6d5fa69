"""The pose graph of loop closing on the CPU (no GPU): the host build of csrc/pose_graph.hpp against the plain-Python
restatement tests/pose_graph_ref.py bit for bit on sentinel-filled outputs; log and acos against the restatement and, within D22's recorded bound,
against math.log / math.acos; Sim3::log on all four branches and both sides of both thresholds, against exp, and on non-finite input; the block
skyline solve against a dense solve; a census of the edge rules the scenes reach; an anchor that does not rest on D22 (a ring with accumulated
drift moves towards its ground truth); the refusals of the C ABI."""
import functools
import math

import numpy as np
import pytest

import pose_graph_ref as REF
import pose_graph_scene as S
import transform_optimizer_ref as D16
from plp import plp

# D22: the largest relative error of pose_log against math.log measured on 400 001 dense arguments of [0.5, 2], 400 000 random ones of [e^-690, e^690]
# and 100 001 dense ones of 1 +- 1e-4 is 2.22e-16; of pose_acos against math.acos on 400 001 dense and 400 000 random arguments of [-1, 1] and 200 000
# within e^-36 .. 1 of either end 2.22e-16.  The bounds are twice that: another libm may differ in the last place.
LOG_MEASURED, LOG_BOUND = 2.22e-16, 4.44e-16
ACOS_MEASURED, ACOS_BOUND = 2.22e-16, 4.44e-16


def same_values(a, b):
    return np.array_equal(np.asarray(a, np.float64), np.asarray(b, np.float64), equal_nan=True)


def log_arguments():
    rng = np.random.default_rng(11)
    return np.concatenate([np.linspace(0.5, 2.0, 400001), np.exp(rng.uniform(-690, 690, 400000)), 1.0 + np.linspace(-1e-4, 1e-4, 100001), [1e-300, 1e300, 1.0]])


def acos_arguments():
    rng = np.random.default_rng(12)
    return np.concatenate([np.linspace(-1, 1, 400001), rng.uniform(-1, 1, 400000), 1.0 - np.exp(rng.uniform(-36, 0, 100000)),
                           -1.0 + np.exp(rng.uniform(-36, 0, 100000))])


def test_pose_log_and_acos_are_the_restatements_bit_for_bit():
    x = np.concatenate([log_arguments()[::7], [np.nextafter(1e-300, 0), np.nextafter(1e300, np.inf), 0.0, -1.0, 5e-324, np.inf, -np.inf, np.nan]])
    assert same_values(plp.model_pose_log(x), [REF.log(float(v)) for v in x])
    assert np.isnan(plp.model_pose_log(x[-8:])).all()
    y = np.concatenate([acos_arguments()[::7], [1.0, -1.0, 0.5, -0.5, 0.0, 2.0 ** -58, np.nextafter(1.0, 2.0), np.nextafter(-1.0, -2.0), np.inf, np.nan]])
    assert same_values(plp.model_pose_acos(y), [REF.acos(float(v)) for v in y])
    assert np.isnan(plp.model_pose_acos(y[-4:])).all()


def test_pose_log_and_acos_against_libm_within_the_recorded_bound():
    x = log_arguments()
    got, want = plp.model_pose_log(x), np.array([math.log(float(v)) for v in x])
    m = want != 0.0
    err = float(np.max(np.abs(got[m] - want[m]) / np.abs(want[m])))
    print(f"pose_log: largest relative error {err:.3e} (recorded {LOG_MEASURED:.3e}, bound {LOG_BOUND:.3e})")
    assert err <= LOG_BOUND and np.array_equal(got[~m], want[~m])
    y = acos_arguments()
    got, want = plp.model_pose_acos(y), np.array([math.acos(float(v)) for v in y])
    m = want != 0.0
    err = float(np.max(np.abs(got[m] - want[m]) / np.abs(want[m])))
    print(f"pose_acos: largest relative error {err:.3e} (recorded {ACOS_MEASURED:.3e}, bound {ACOS_BOUND:.3e})")
    assert err <= ACOS_BOUND and np.array_equal(got[~m], want[~m])


def log_cases():
    """updates u whose Sim3 exp(u) reaches every branch of Sim3::log, with sigma and the angle on both sides of the thresholds"""
    eps = 1e-5
    small_angle = math.sqrt(2 * eps)                         # d = cos(theta) crosses 1 - eps here
    us = []
    for sigma in (0.0, 0.5 * eps, np.nextafter(eps, 0), eps, 2 * eps, -0.5 * eps, -2 * eps, 0.3, -0.4):
        for theta in (0.0, 1e-9, 0.5 * small_angle, 0.999 * small_angle, 1.001 * small_angle, 2 * small_angle, 0.7, 2.5, 3.1):
            axis = np.array([0.3, -0.5, 0.8]) / math.sqrt(0.98)
            us.append(np.concatenate([theta * axis, [0.4, -1.1, 2.0], [sigma]]))
    return np.array(us)


def test_sim3_log_bit_for_bit_on_every_branch_and_against_exp():
    us = log_cases()
    ident = [0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0]
    sims = np.array([D16.oplus([float(v) for v in u], ident) for u in us])
    got = plp.model_sim3_log(sims)
    want = np.array([REF.sim3_log([float(v) for v in s]) for s in sims])
    assert same_values(got, want)
    assert {REF.log_branch([float(v) for v in s]) for s in sims} == {(a, b) for a in (False, True) for b in (False, True)}
    # log(exp(u)) = u where exp and log take matching branches.  Between them they do not: exp switches at theta = 1e-5, log at cos(theta) = 1 - 1e-5, and the
    # small-angle branch of both carries g2o's B = (sigma^2 / 2 - sigma + 1) s / sigma^3 (the closed form lacks its "- 1"), which a rotation of a few mrad
    # turns into an upsilon that is off by a third; those cases are held bit for bit above and not to u.
    theta, sg = np.linalg.norm(us[:, :3], axis=1), np.abs(us[:, 6])
    clean = ((theta <= 1e-9) | (theta >= 0.7)) & ((sg <= 0.5e-5) | (sg >= 0.3))
    assert clean.sum() >= 20
    err = np.abs(got - us)[clean]
    assert err.max() < 1e-9, err.max()
    assert np.abs(got - us)[clean & (theta >= 0.7) & (theta < 3.0)].max() < 1e-12


def test_sim3_log_of_non_finite_and_degenerate_input():
    bad = np.array([[0, 0, 0, 1, 1, 2, 3, np.nan], [0, 0, 0, 1, 1, 2, 3, np.inf], [0, 0, 0, 1, 1, 2, 3, 0.0], [0, 0, 0, 1, 1, 2, 3, -1.0],
                    [np.nan, 0, 0, 1, 1, 2, 3, 1.0], [0, 0, 0, 1, np.inf, 2, 3, 1.0], [0, 0, 0, 2.0, 1, 2, 3, 1.0], [0, 0, 0, 0, 1, 2, 3, 1.0]], np.float64)
    got = plp.model_sim3_log(bad)
    want = np.array([REF.sim3_log([float(v) for v in s]) for s in bad])
    assert same_values(got, want)
    assert np.isnan(got[:4, 6]).all() and np.isnan(got[4]).any() and not np.isfinite(got[5, 3:6]).all()


def test_block_skyline_solve_bit_for_bit_and_against_a_dense_solve():
    rng = np.random.default_rng(5)
    for n, first in ((1, [0]), (4, [0, 0, 1, 2]), (6, [0, 0, 1, 2, 3, 0]), (5, [0, 1, 2, 3, 4]), (7, [0, 0, 0, 2, 3, 3, 1])):
        N = 7 * n
        mask = np.zeros((N, N), bool)
        for i, f in enumerate(first):
            mask[7 * i:7 * i + 7, 7 * f:7 * i + 7] = True
        mask |= mask.T
        A = rng.normal(size=(N, N)) * mask
        H = A @ A.T * 0.1 + np.diag(rng.uniform(1, 2, N))
        H = (H + H.T) * 0.5 * mask
        b = rng.normal(size=N)
        x, ok = plp.model_block_chol7(H, first, b, 0.25)
        Hd = {(p, c): float(H[p, c]) for p in range(N) for c in range(7 * first[p // 7], p + 1)}
        xr, okr = REF.skyline_solve(Hd, list(first), [float(v) for v in b], 0.25)
        assert ok and okr and same_values(x, xr), (n, first)
        assert np.allclose(x, np.linalg.solve(H + 0.25 * np.eye(N), b), rtol=1e-9, atol=1e-11)
    # a pivot that is not positive: the solve fails, x is zero
    H = -np.eye(7)
    x, ok = plp.model_block_chol7(H, [0], np.ones(7), 0.5)
    assert not ok and not x.any()
    x, ok = plp.model_block_chol7(np.eye(7) * np.nan, [0], np.ones(7), 0.5)
    assert not ok and not x.any()


SCENES = {
    "ring8": lambda: S.ring(8, extra=3)[:2],
    "ring12_fixed_scale_arrow": lambda: S.ring(12, extra=5, fix_scale=True, arrow=True)[:2],
    "ring9_scale_drift": lambda: S.ring(9, extra=2, scale_drift=1.08, n_pre=3)[:2],
    "two_keyframes": lambda: S.ring(2)[:2],
    "census": S.census,
}


@functools.lru_cache(maxsize=None)
def reference(name, edge_cap=40, env_cap=2048):
    t, prs = SCENES[name]()
    ev = set()
    graphs = REF.run(t, prs, edge_cap, env_cap, 50, ev)
    return t, prs, graphs, ev


def filled(want):
    return {k: np.full_like(v, REF.SENTINEL[k]) for k, v in want.items()}


@pytest.mark.parametrize("name", sorted(SCENES))
def test_host_build_equals_the_restatement_bit_for_bit(name):
    t, prs, graphs, _ = reference(name)
    want = REF.expected(graphs, len(t["kf_parent"]), 40)
    got = plp.model_pose_graph_optimize(t, prs, edge_cap=40, env_cap=2048, out=filled(want))
    for k in want:
        assert np.array_equal(got[k], want[k], equal_nan=True), k
    assert (want["status"] != REF.BAD_LOOP_KF).any() and all(g.num_edges > 0 for g in graphs if g.status == REF.OK)


def test_edge_list_alone_and_the_optimizer_mirror():
    t, prs, graphs, _ = reference("census")
    want = REF.expected(graphs, len(t["kf_parent"]), 40, names=("status", "num_edges", "edges", "sim3_cw"))
    got = plp.model_pose_graph_edges(t, prs, edge_cap=40, out=filled(want))
    for k in want:
        assert np.array_equal(got[k], want[k]), k
    pr = prs[0]
    r = plp.graph_optimizer(t, pr["fix_scale"], edge_cap=40, env_cap=2048).optimize(pr["loop_kf"], pr["curr_kf"], pr["non_corrected"], pr["pre_corrected"],
                                                                                      pr["loop_connections"])
    one = REF.expected(graphs[:1], len(t["kf_parent"]), 40)
    vertices = t["kf_erased"] == 0
    assert r["status"] == REF.OK and np.array_equal(r["pose"][vertices], one["pose"][0][vertices]) and np.array_equal(r["info"], one["info"][0])


def test_census_of_the_edge_rules():
    """every edge type, every exclusion of :252-285, the id skips, the weight gate and its exemption, the over-weight quirk, pre- and non-corrected rows, an
    erased key frame, a vertex without edges, a component that is not connected to the fixed vertex"""
    _, _, graphs, ev = reference("census")
    need = {("edge", REF.LOOP_CONNECTION), ("edge", REF.PARENT), ("edge", REF.LOOP), ("edge", REF.COVIS), "covis_without_parent", "covis_is_the_parent",
            "covis_is_a_child", "covis_is_a_loop_edge", "covis_is_erased", "covis_id_skip", "covis_pair_already_inserted", "loop_edge_id_skip",
            "parent_id_not_below_leaves_the_keyframe", "loop_connection_below_weight_skipped", "curr_loop_exempt_from_weight",
            "over_weight_all_qualify_returns_empty", "over_weight_proper_prefix", "pre_corrected_vertex", "non_corrected_used", "erased_keyframe_is_no_vertex",
            "edge_with_a_missing_end_not_inserted", "vertex_without_edges", "component_without_the_fixed_vertex"}
    assert need <= ev, need - ev
    assert [g.status for g in graphs] == [REF.OK, REF.OK, REF.BAD_LOOP_KF]
    assert {k for _, _, k, _ in graphs[0].edges} == {1, 2, 3, 4}


def pose_distance(a, b):
    """(angle between the rotations, distance of the camera centres) of two pose rows"""
    Ra, Rb = a[:9].reshape(3, 3), b[:9].reshape(3, 3)
    c = (np.trace(Ra @ Rb.T) - 1.0) * 0.5
    return math.acos(min(1.0, max(-1.0, c))), float(np.linalg.norm(a[12:15] - b[12:15]))


@pytest.mark.parametrize("fix_scale", [False, True])
def test_anchor_a_drifted_ring_moves_towards_its_ground_truth(fix_scale):
    F = 24
    t, prs, gt = S.ring(F, extra=10, fix_scale=fix_scale, turn=1.0 - 1.0 / F, n_pre=1)
    prs[0]["pre_corrected"] = {F - 1: S.sim3_of(gt[F - 1])}   # the true loop constraint: where the current key frame really is
    first = plp.model_pose_graph_optimize(t, prs, edge_cap=64, env_cap=2048, max_iter=0)
    r = plp.model_pose_graph_optimize(t, prs, edge_cap=64, env_cap=2048)
    assert r["status"][0] == REF.OK and r["info"][0, 0] >= 3
    # chi2 falls: max_iter = 0 leaves the estimates; the chi2 at the start is the restatement's
    g = REF.Graph(t, prs[0], 64, 2048)
    start = sum(c for _, c in g.errors(g.est))
    assert r["chi2"][0, 0] < 0.05 * start, (r["chi2"][0], start)
    assert np.array_equal(first["pose"][0, :, :9], np.array([REF.pose_from_sim3(g.Sim3s_cw[i])[:9] for i in range(F)]))
    for i in range(1, F - 1):                                # row 0 is fixed at the truth; the current key frame starts at the truth
        before, after = pose_distance(t["pose"][i], gt[i]), pose_distance(r["pose"][0, i], gt[i])
        assert after[0] < before[0] and after[1] < before[1], (i, before, after)
    scales = 1.0 / r["corrected_wc"][0, :, 7]
    if fix_scale:
        assert np.array_equal(r["corrected_wc"][0, :, 7], np.ones(F))
    else:
        assert np.abs(scales - 1.0).max() > 1e-4             # the translations carry 2 % of drift, which only a scale can take up


def test_caps_and_refusals():
    t, prs, _ = S.ring(8, extra=3)
    E = S.edge_count(8, 3)
    got = plp.model_pose_graph_optimize(t, prs, edge_cap=E, env_cap=2048)
    assert got["status"][0] == REF.OK and got["num_edges"][0] == E
    want = REF.expected(REF.run(t, prs, E - 1, 2048), 8, E - 1)
    got = plp.model_pose_graph_optimize(t, prs, edge_cap=E - 1, env_cap=2048, out=filled(want))
    assert got["status"][0] == REF.TOO_MANY_EDGES and all(np.array_equal(got[k], want[k]) for k in want)
    n_env = sum(i - f + 1 for i, f in enumerate(REF.Graph(t, prs[0]).first))
    assert plp.model_pose_graph_optimize(t, prs, edge_cap=E, env_cap=n_env)["status"][0] == REF.OK
    want = REF.expected(REF.run(t, prs, E, n_env - 1), 8, E)
    got = plp.model_pose_graph_optimize(t, prs, edge_cap=E, env_cap=n_env - 1, out=filled(want))
    assert got["status"][0] == REF.ENVELOPE_TOO_LARGE and all(np.array_equal(got[k], want[k]) for k in want)
    # the limits of a call: refused before anything is written
    for kw in (dict(edge_cap=plp.POSE_GRAPH_MAX_EDGES + 1), dict(env_cap=plp.POSE_GRAPH_MAX_ENV + 1)):
        out = filled(REF.expected(REF.run(t, prs, 4, 4, solve=False), 8, 4))
        out.pop("edges")
        before = {k: v.copy() for k, v in out.items()}
        with pytest.raises(plp.PlpError) as e:
            plp.model_pose_graph_optimize(t, prs, **{**dict(edge_cap=4, env_cap=4), **kw}, outputs=tuple(out), out=out)
        assert e.value.status == plp.PLP_ERR_UNSUPPORTED and all(np.array_equal(out[k], before[k]) for k in out)
    with pytest.raises(plp.PlpError) as e:
        plp.model_pose_graph_optimize(t, prs * (plp.POSE_GRAPH_MAX_PROBLEMS + 1), edge_cap=16, env_cap=64)
    assert e.value.status == plp.PLP_ERR_UNSUPPORTED
    big = S.graph_tables(plp.POSE_GRAPH_MAX_KF + 1, np.zeros((plp.POSE_GRAPH_MAX_KF + 1, 15)), {}, [-1] * (plp.POSE_GRAPH_MAX_KF + 1))
    with pytest.raises(plp.PlpError) as e:
        plp.model_pose_graph_optimize(big, prs, edge_cap=16, env_cap=64)
    assert e.value.status == plp.PLP_ERR_UNSUPPORTED
    with pytest.raises(plp.PlpError) as e:
        plp.model_pose_graph_optimize(t, prs, edge_cap=0, env_cap=64)
    assert e.value.status == plp.PLP_ERR_INVALID_ARG


def test_landmark_correction_equals_the_restatement():
    t, prs, _ = S.ring(8, extra=3)
    r = plp.model_pose_graph_optimize(t, prs, edge_cap=32, env_cap=512)
    erased = np.zeros(8, np.uint8)
    erased[4] = 1
    pos, ref, er = S.landmarks(8, 100)
    want, status = REF.correct_landmarks(pos, ref, r["sim3_cw"][0], r["corrected_wc"][0], er, erased)
    got = plp.model_correct_landmarks(pos, ref, r["sim3_cw"][0], r["corrected_wc"][0], lm_erased=er, kf_erased=erased,
                                      out=dict(pos_w=np.full((100, 3), -7.25), status=np.full(100, 0xEE, np.uint8)))
    assert np.array_equal(got["pos_w"], want) and np.array_equal(got["status"], status)
    assert set(status.tolist()) == {REF.LM_OK, REF.LM_ERASED, REF.LM_NO_VERTEX}
    # the correction moves a landmark with its reference key frame: what it sees from there stays what it saw
    l = int(np.flatnonzero(status == REF.LM_OK)[0])
    cw, wc = r["sim3_cw"][0, ref[l]], r["corrected_wc"][0, ref[l]]
    seen = D16.sim3_map([float(v) for v in cw], [float(v) for v in pos[l]])
    again = D16.sim3_map(D16.inverse([float(v) for v in wc]), [float(v) for v in got["pos_w"][l]])
    assert np.allclose(seen, again, atol=1e-9)
