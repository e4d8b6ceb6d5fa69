"""optimize::local_bundle_adjuster without a GPU: the host build of csrc/local_ba.hpp (plp.model_local_ba*) against the plain-Python restatement of
DESIGN.md D17 (tests/local_ba_ref.py) bit for bit on a census of scenes, and against anchors that do not depend on the definition: D15's pose sums,
central differences, numpy's dense solve, the ground truth, the generating outlier labels, the chi2 of a round."""
import functools
import math

import numpy as np
import pytest

import local_ba_ref as REF
import local_ba_scene as S
import pose_optimizer_ref as R15
from plp import plp

# what the restatement alone achieves on these scenes (measured by these tests, which print their figures), and the bound: ten times that -- key points are floats
MEASURED_JACOBIAN, BOUND_JACOBIAN = 1.05e-10, 1.05e-9        # (b) landmark Jacobian against central differences of the error, relative to the largest entry
MEASURED_SOLVE, BOUND_SOLVE = 5.2e-14, 5.2e-13            # (c) the Schur solve against numpy.linalg.solve on the dense damped system, relative to max |x|
MEASURED_TRUTH, BOUND_TRUTH = 7.6e-5, 7.6e-4               # (d) poses (12 entries) and positions against the ground truth after 5 + 10 iterations, absolute (4.3e-5 mono, 7.6e-5 RGB-D fisheye)


def dims(sc):
    return len(sc["pose"]), len(sc["pos_w"]), len(sc["obs_kf"])


@functools.lru_cache(None)
def census():
    return S.census()


@functools.lru_cache(None)
def run(name):
    sc = census()[name]
    F, L, T = dims(sc)
    got = plp.model_local_ba(**S.call_args(sc), out=S.sentinel_out(1, F, L, T))
    want = S.sentinel_out(1, F, L, T)
    r = S.expected(sc, sc["kf_local"], want, 0)
    return got, want, r


NAMES = ["mono", "rgbd", "fisheye", "fisheye_rgbd", "large", "far_start", "at_truth", "no_information", "seen_once", "behind", "nan", "no_free_pose", "no_edges"]


def test_the_census_names_every_scene():
    assert sorted(NAMES) == sorted(census())


@pytest.mark.parametrize("name", NAMES)
def test_host_build_equals_the_restatement(name):
    got, want, r = run(name)
    for k in want:
        assert S.same({k: got[k]}, {k: want[k]}), k


def test_the_census_reaches_what_it_has_to():
    seen = set()
    sizes = dict(free=set(), fixed=set(), lms=[])
    for name in NAMES:
        sc = census()[name]
        got, want, r = run(name)
        info = r["round_info"]
        if r["status"] == REF.NO_EDGES:
            seen.add("zero edges")
            continue
        P = r["problem"]
        sizes["free"].add(len(P.free)); sizes["fixed"].add(sum(v == REF.KF_FIXED for v in P.role)); sizes["lms"].append(sum(P.lm_role))
        seen.add(("mono" if sc["setup_type"] == S.MONO else "depth") + " " + sc["model"])
        if any(i[1] > 0 for i in info): seen.add("rejected steps")
        if any(i[3] == R15.END_TRIES for i in info): seen.add("ten tries")
        if any(i[3] == R15.END_RHO_ZERO for i in info): seen.add("rho zero")
        per_lm = {}
        for e in P.edges:
            per_lm.setdefault(e.l, []).append(e)
        if any(len(v) == 1 for v in per_lm.values()): seen.add("seen once")
        if any(all(e.level for e in v) for v in per_lm.values()): seen.add("loses every edge")
        if any(all(e.kf != f for e in P.edges) for f in P.free): seen.add("free key frame without an edge")
        if not P.free: seen.add("zero free poses")
        if any(sc["kf_erased"][sc["obs_kf"][t]] for l in range(len(P.lm_role)) if P.lm_role[l] for t in range(sc["obs_offsets"][l], sc["obs_offsets"][l + 1])):
            seen.add("erased observer")
        fresh = REF.Problem(S.ref_tables(sc), [int(v) for v in sc["kf_local"]])
        if any(not (0.0 < R15.se3_map(fresh.kf_est[e.kf], fresh.lm_est[e.l])[2]) for e in fresh.edges): seen.add("z <= 0")
        if any(math.isnan(e.chi2) for e in P.edges): seen.add("NaN chi2")
    need = {"zero edges", "mono perspective", "depth perspective", "mono fisheye", "depth fisheye", "rejected steps", "ten tries", "rho zero", "seen once",
            "loses every edge", "free key frame without an edge", "zero free poses", "erased observer", "z <= 0", "NaN chi2"}
    assert need <= seen, need - seen
    assert min(sizes["free"]) <= 2 and max(sizes["free"]) >= 6 and min(sizes["fixed"] - {0}) == 1 and max(sizes["fixed"]) >= 4, sizes
    assert min(sizes["lms"]) <= 20 and max(sizes["lms"]) >= 300, sizes


def test_no_edges_leaves_the_inputs():
    got, want, r = run("no_edges")
    assert got["status"][0] == plp.LOCAL_BA_NO_EDGES and (got["kf_role"] == 0).all() and (got["outlier"] == 77).all() and (got["pose"] == -7.5).all()
    sc = dict(census()["fisheye"])
    sc["undist"] = sc["undist"].copy(); sc["undist"]["octave"] = 40          # every octave outside the table: local sets, no edge
    F, L, T = dims(sc)
    got = plp.model_local_ba(**S.call_args(sc), out=S.sentinel_out(1, F, L, T))
    free = got["kf_role"][0] == plp.LOCAL_BA_KF_FREE
    assert got["status"][0] == plp.LOCAL_BA_NO_EDGES and free.sum() == 2 and (got["outlier"] == 77).all()
    assert np.array_equal(got["pose"][0, free, :12], sc["pose"][free, :12]) and np.array_equal(got["pos_w"][0][got["lm_role"][0] == 1], sc["pos_w"][got["lm_role"][0] == 1])


# ---- anchors
@pytest.mark.parametrize("setup,robust", [(S.MONO, True), (S.MONO, False), (S.RGBD, True), (S.RGBD, False)])
def test_a_the_pose_block_is_d15s(setup, robust):
    """one free key frame that sees every landmark once: the edges of the adjuster are the pose optimiser's, in its order"""
    sc = S.make_scene(31, 1, 0, 40, setup=setup, noise=2.0, outliers=6, n_other=0, obs_share=1.0)
    lin = plp.model_local_ba_linearize(**S.call_args(sc), robust=robust)
    assert lin["free_kf"].tolist() == [0]
    idx = sc["obs_idx"]
    xr = None if sc["x_right"] is None else sc["x_right"][0, idx][None]
    d15 = plp.model_pose_linearize(sc["camera"], setup, sc["pose"][:1], np.ones((1, len(idx)), np.uint8), sc["undist"][0, idx][None], sc["pos_w"][None], S.INV_SIGMA_SQ,
                                   x_right=xr, robust=robust)
    assert lin["Hpp"][0].tobytes() == d15["H"][0].tobytes() and lin["bp"][0].tobytes() == d15["b"][0].tobytes()
    assert np.float64(lin["chi2"]).tobytes() == d15["chi2"][0].tobytes() and lin["edge_chi2"].tobytes() == d15["edge_chi2"][0].tobytes()


def test_b_the_landmark_jacobian_agrees_with_central_differences():
    sc = S.make_scene(32, 2, 2, 30, setup=S.RGBD, noise=0.5)
    P = REF.Problem(S.ref_tables(sc), [int(v) for v in sc["kf_local"]])
    worst = 0.0
    for e in P.edges:
        est, p = P.kf_est[e.kf], P.lm_est[e.l]
        _, pc, _ = R15.point_error(est, P.Tb.cam, p, e.ox, e.oy, e.orr, e.mono, e.w)
        J = REF.lm_jacobian(P.Tb.cam, est, pc, e.mono)
        rows = 2 if e.mono else 3
        for c in range(3):
            h = 1e-5
            hi = list(p); lo = list(p); hi[c] += h; lo[c] -= h
            eh = R15.point_error(est, P.Tb.cam, hi, e.ox, e.oy, e.orr, e.mono, e.w)[2]
            el = R15.point_error(est, P.Tb.cam, lo, e.ox, e.oy, e.orr, e.mono, e.w)[2]
            for r in range(rows):
                worst = max(worst, abs((eh[r] - el[r]) / (2 * h) - J[3 * r + c]) / max(abs(v) for v in J[:3 * rows]))
    print("landmark Jacobian against central differences:", worst)
    assert worst <= BOUND_JACOBIAN
    # ... and the host build's landmark blocks are the restatement's
    P.round_setup()
    Hpp, Hll, W, chi = P.linearize(True)
    lin = plp.model_local_ba_linearize(**S.call_args(sc), robust=True)
    for l, v in Hll.items():
        assert np.array(v).tobytes() == np.concatenate([lin["Hll"][l], lin["bl"][l]]).tobytes()
    for t, v in W.items():
        assert np.array(v).tobytes() == lin["W"][t].tobytes()
    assert np.float64(chi).tobytes() == np.float64(lin["chi2"]).tobytes()


def dense_system(P, M, Hpp, bp, Hll, bl, e_pose, e_lm, W, lam):
    n = 6 * P + 3 * M
    A = np.zeros((n, n)); b = np.zeros(n)
    for i in range(P):
        for r in range(6):
            for c in range(r, 6):
                A[6 * i + r, 6 * i + c] = A[6 * i + c, 6 * i + r] = Hpp[i][R15.h_index(r, c)]
        b[6 * i:6 * i + 6] = bp[i]
    sym = REF.SYM3
    for l in range(M):
        o = 6 * P + 3 * l
        for r in range(3):
            for c in range(3):
                A[o + r, o + c] = Hll[l][sym[r][c]]
        b[o:o + 3] = bl[l]
    for e in range(len(e_pose)):
        if e_pose[e] >= 0:
            i, o = 6 * e_pose[e], 6 * P + 3 * e_lm[e]
            A[i:i + 6, o:o + 3] += W[e]; A[o:o + 3, i:i + 6] += W[e].T
    return A + lam * np.eye(n), b


@pytest.mark.parametrize("seed,n_free", [(33, 1), (34, 3), (35, 11)])
def test_c_the_schur_solve_agrees_with_a_dense_solve(seed, n_free):
    sc = S.make_scene(seed, n_free, 2, 40, setup=S.RGBD, noise=0.8)
    lin = plp.model_local_ba_linearize(**S.call_args(sc), robust=True)
    P = len(lin["free_kf"])
    assert P == n_free
    row = {int(f): i for i, f in enumerate(lin["free_kf"])}
    edge = ~np.isnan(lin["edge_chi2"])
    lm_of = np.searchsorted(sc["obs_offsets"], np.arange(len(edge)), side="right") - 1
    ts = np.where(edge)[0]
    e_pose = np.array([row.get(int(sc["obs_kf"][t]), -1) for t in ts]); e_lm = lm_of[ts]
    W = np.nan_to_num(lin["W"][ts])
    M = len(sc["pos_w"])
    Hll = np.nan_to_num(lin["Hll"]); bl = np.nan_to_num(lin["bl"])
    has = np.zeros(M, bool); has[e_lm] = True
    lam = 1e-5 * max(np.abs(lin["Hpp"][:, [0, 6, 11, 15, 18, 20]]).max(), np.abs(Hll[:, [0, 3, 5]]).max())
    xp, xl, ok = plp.model_local_ba_solve(lin["Hpp"], lin["bp"], Hll, bl, e_pose, e_lm, W, lam)
    assert ok
    A, b = dense_system(P, M, lin["Hpp"], lin["bp"], Hll, bl, e_pose, e_lm, W, lam)
    keep = np.concatenate([np.ones(6 * P, bool), np.repeat(has, 3)])
    x = np.linalg.solve(A[np.ix_(keep, keep)], b[keep])
    mine = np.concatenate([xp.reshape(-1), xl.reshape(-1)])[keep]
    err = np.abs(mine - x).max() / np.abs(x).max()
    print("Schur solve against numpy.linalg.solve:", err)
    assert err <= BOUND_SOLVE
    assert (xl[~has] == 0).all()
    # the restatement's solve is the host build's
    Pr = REF.Problem(S.ref_tables(sc), [int(v) for v in sc["kf_local"]])
    Pr.round_setup()
    Hp, Hl, Wr, _ = Pr.linearize(True)
    okr, xpr, xlr = Pr.solve(Hp, Hl, Wr, float(lam))
    assert okr and all(np.array(xpr[f]).tobytes() == xp[row[f]].tobytes() for f in Pr.pa) and all(np.array(xlr[l]).tobytes() == xl[l].tobytes() for l in Pr.la)


@pytest.mark.parametrize("seed,setup,model", [(36, S.MONO, "perspective"), (37, S.RGBD, "fisheye")])
def test_d_perturbed_vertices_return_to_the_ground_truth(seed, setup, model):
    sc = S.make_scene(seed, 3, 2, 60, model=model, setup=setup, min_obs=4, n_other=0)
    F, L, T = dims(sc)
    got = plp.model_local_ba(**S.call_args(sc))
    free = got["kf_role"][0] == plp.LOCAL_BA_KF_FREE
    assert free.sum() == 3 and (got["kf_role"][0] == plp.LOCAL_BA_KF_FIXED).sum() == 2
    start = max(np.abs(sc["pose"][free, :12] - sc["pose_gt"][free]).max(), np.abs(sc["pos_w"] - sc["pos_gt"]).max())
    err = max(np.abs(got["pose"][0, free, :12] - sc["pose_gt"][free]).max(), np.abs(got["pos_w"][0] - sc["pos_gt"]).max())
    print("distance from the ground truth: start", start, "end", err)
    assert start > 1e-2 and err <= BOUND_TRUTH
    assert (got["outlier"][0] == 0).all()


@pytest.mark.parametrize("seed,setup", [(38, S.MONO), (43, S.MONO), (43, S.RGBD), (45, S.RGBD)])          # scenes for which the restatement alone meets the labels
def test_e_the_outliers_are_the_generating_labels(seed, setup):
    sc = S.make_scene(seed, 3, 3, 60, setup=setup, outliers=12, min_obs=4, n_other=0, pose_noise=0.003, lm_noise=0.005)      # no erased observer: every observation is an edge
    F, L, T = dims(sc)
    want = S.sentinel_out(1, F, L, T)
    r = S.expected(sc, sc["kf_local"], want, 0)
    edge = want["outlier"][0] != 77
    assert edge.all() and np.diff(sc["obs_offsets"]).min() >= 4 and max(sc["label"][sc["obs_offsets"][l]:sc["obs_offsets"][l + 1]].sum() for l in range(L)) == 1
    assert sc["label"].sum() >= 8 and np.array_equal(want["outlier"][0][edge], sc["label"][edge])          # the restatement alone meets the labels
    got = plp.model_local_ba(**S.call_args(sc), out=S.sentinel_out(1, F, L, T))
    assert np.array_equal(got["outlier"], want["outlier"])


@pytest.mark.parametrize("name", ["mono", "rgbd", "fisheye", "fisheye_rgbd", "large", "far_start", "behind"])
def test_f_a_round_never_raises_the_robust_chi2(name):
    """the chi2 a round starts from is its first linearisation's sum over the level-0 edges at the estimates the round begins with -- Huber on in round
    1, off in round 2 at round 1's kept estimates without the edges that went to level 1; the chi2 at the round's end must not exceed it"""
    sc = census()[name]
    got, want, r = run(name)
    start = r["problem"].start_chi                        # the restatement's, whose results the host build equals bit for bit (test_host_build_equals_the_restatement)
    assert len(start) == 2 and (got["round_info"][0, :, 0] >= 1).all()           # both rounds ran
    # round 1's start, independently: one linearisation of the inputs by the host build
    lin = plp.model_local_ba_linearize(**S.call_args(sc), robust=True)
    assert np.float64(lin["chi2"]).tobytes() == np.float64(start[0]).tobytes()
    # round 2's start, independently: the edges' own chi2 (Huber off) at round 1's kept estimates summed over the edges round 1 left at level 0, in D17's order
    P = r["problem"]
    one = REF.Problem(S.ref_tables(sc), [int(v) for v in sc["kf_local"]])
    one.current, one.lam, one.ni = 0.0, 0.0, 2.0
    one.round_setup()
    one.optimize(5, True)                                 # round 1 again, alone
    for e in one.edges:
        e.level = int(REF.is_outlier(one, e))
    one.round_setup()
    assert np.float64(one.evaluate(one.kf_est, one.lm_est, False)).tobytes() == np.float64(start[1]).tobytes()
    print(name, "round starts", start, "ends", got["round_chi2"][0, :, 0].tolist())
    for rnd in range(2):
        assert got["round_chi2"][0, rnd, 0] <= start[rnd], rnd


# ---- pieces
def test_inv3_at_its_branch_points():
    a = np.array([[2, 0, 0, 3, 0, 4], [4, 1, 2, 5, 3, 6], [1, 2, 3, 4, 6, 9], [0, 0, 0, 0, 0, 0], [math.nan, 0, 0, 1, 0, 1], [math.inf, 0, 0, 1, 0, 1], [1e-200, 0, 0, 1e-200, 0, 1e-200]], float)
    inv, ok = plp.model_inv3(a)
    assert ok.tolist() == [True, True, False, False, False, False, False]
    full = lambda v: np.array([[v[0], v[1], v[2]], [v[1], v[3], v[4]], [v[2], v[4], v[5]]])
    assert np.allclose(full(inv[1]) @ full(a[1]), np.eye(3), atol=1e-14)
    for i in range(len(a)):
        want, good = REF.inv3([float(v) for v in a[i]])
        assert good == ok[i] and S.same({"v": inv[i]}, {"v": np.array(want)})


def test_the_solve_fails_on_a_pivot_and_on_an_inverse():
    Hpp = np.zeros((1, 21)); Hpp[0, [0, 6, 11, 15, 18, 20]] = 1.0
    bp = np.ones((1, 6)); Hll = np.array([[1.0, 0, 0, 1, 0, 1]]); bl = np.ones((1, 3)); W = np.zeros((1, 6, 3))
    xp, xl, ok = plp.model_local_ba_solve(Hpp, bp, Hll, bl, [0], [0], W, 1.0)
    assert ok and np.allclose(xp, 0.5, rtol=1e-15, atol=0) and np.array_equal(xl, np.full((1, 3), 0.5))
    bad = Hpp.copy(); bad[0, 20] = -3.0                                     # the last pivot is negative
    xp, xl, ok = plp.model_local_ba_solve(bad, bp, Hll, bl, [0], [0], W, 1.0)
    assert not ok and not xp.any() and not xl.any()
    xp, xl, ok = plp.model_local_ba_solve(Hpp, bp, np.zeros((1, 6)), bl, [0], [0], W, 0.0)      # a singular landmark block
    assert not ok and not xp.any() and not xl.any()
    xp, xl, ok = plp.model_local_ba_solve(np.zeros((0, 21)), np.zeros((0, 6)), Hll, bl, [-1], [0], W, 1.0)   # no pose: the landmarks alone
    assert ok and not xp.size and np.array_equal(xl, np.full((1, 3), 0.5))


def test_the_pose_update_takes_both_branches_of_exp():
    """D17's pose update is exp(x_p) * estimate (la_update): the census, whose every output the host build reproduces bit for bit, applies updates on both
    sides of theta = 1e-5, where exp changes its formula"""
    small = large = 0
    for name in NAMES:
        got, want, r = run(name)
        th = r["problem"].thetas if "problem" in r else []
        small += sum(0.0 < t < 0.00001 for t in th); large += sum(t >= 0.00001 for t in th)
    print("pose updates with theta below / above 1e-5:", small, large)
    assert small >= 5 and large >= 5


def test_refusals_and_the_mirror_class():
    sc = census()["fisheye"]
    a = S.call_args(sc)
    eq = S.PS.camera("perspective"); eq.model = plp.CAMERA_EQUIRECTANGULAR
    with pytest.raises(plp.PlpError) as e:
        plp.model_local_ba(**{**a, "camera": eq})
    assert e.value.status == plp.PLP_ERR_UNSUPPORTED
    with pytest.raises(plp.PlpError) as e:
        plp.model_local_ba(**{**a, "num_first_iter": 0})
    assert e.value.status == plp.PLP_ERR_INVALID_ARG
    many = S.make_scene(40, 65, 1, 5, n_other=0)
    with pytest.raises(plp.PlpError) as e:
        plp.model_local_ba(**S.call_args(many))
    assert e.value.status == plp.PLP_ERR_UNSUPPORTED
    wide = dict(a, pos_w=np.zeros((16385, 3)), obs_offsets=np.zeros(16386, np.int32), obs_kf=np.zeros(0, np.int32), obs_idx=np.zeros(0, np.int32),
                lm_erased=None, kf_local=np.zeros((256, len(sc["pose"])), np.uint8))                    # G L = 2^22 + 256
    with pytest.raises(plp.PlpError) as e:
        plp.model_local_ba(**wide)
    assert e.value.status == plp.PLP_ERR_UNSUPPORTED
    got, want, r = run("fisheye")
    one = plp.local_bundle_adjuster().optimize(**{k: v for k, v in a.items()})
    assert all(np.array_equal(one[k], plp.model_local_ba(**a)[k][0]) for k in one)
