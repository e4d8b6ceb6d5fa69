"""optimize::local_bundle_adjuster_extended_line without a GPU: the host build of csrc/local_ba_lines.hpp (plp.model_local_ba_lines*) against the
plain-Python restatement of DESIGN.md D28 (tests/local_ba_lines_ref.py) bit for bit on a census of scenes, and against anchors that do not depend on
the definition: the point adjuster on a problem without a line edge, D15's pose sums, central differences, numpy's dense solve, the ground truth, the
generating outlier labels, the chi2 of a round."""
import functools

import numpy as np
import pytest

import local_ba_lines_ref as LREF
import local_ba_lines_scene as LS
import local_ba_scene as S
import pose_optimizer_ref as R15
from plp import plp

# what the restatement alone achieves on these scenes (measured by these tests, which print their figures), and the bound: ten times that -- key lines are floats
MEASURED_JACOBIAN, BOUND_JACOBIAN = 1.06e-7, 1.06e-6     # (c) the line block against central differences of the error at step 1e-5, relative to the edge's largest entry
MEASURED_SOLVE, BOUND_SOLVE = 5.5e-13, 5.5e-12           # (d) the mixed Schur solve against numpy.linalg.solve on the dense damped system, relative to max |x|
# (e) poses (12 entries), positions and normalised lines against the ground truth after 5 + 10 iterations, absolute: 6.5e-4 mono, 7.2e-4 RGB-D fisheye, both
# from the one or two lines the damping (lambda starts at 1e-5 of a diagonal of 1e7) lets move slowly; poses and positions reach 4e-5
MEASURED_TRUTH, BOUND_TRUTH = 7.2e-4, 7.2e-3

NAMES = ["mono", "rgbd", "fisheye", "far_start", "lines_only", "through_a_line", "no_information", "no_edges"]


@functools.lru_cache(None)
def census():
    return LS.census()


@functools.lru_cache(None)
def run(name):
    sc = census()[name]
    d = LS.dims(sc)
    got = plp.model_local_ba_lines(**LS.call_args(sc), out=LS.sentinel_out(1, *d))
    want = LS.sentinel_out(1, *d)
    r = LS.expected(sc, sc["kf_local"], want, 0)
    return got, want, r


def test_the_census_names_every_scene():
    assert sorted(NAMES) == sorted(census())


@pytest.mark.parametrize("name", NAMES)
def test_host_build_equals_the_restatement(name):
    got, want, r = run(name)
    assert sorted(got) == sorted(want)
    for k in want:
        assert S.same({k: got[k]}, {k: want[k]}), k


def test_the_census_reaches_what_it_has_to():
    seen = set()
    for name in NAMES:
        got, want, r = run(name)
        if r["status"] == LREF.NO_EDGES:
            seen.add("zero edges")
            continue
        P, info = r["problem"], r["round_info"]
        if info[0][0] >= 2 and info[1][0] >= 2: seen.add("both rounds with two iterations")
        if info[0][1] + info[1][1] > 0: seen.add("rejected step")
        if any(e.level for e in P.edges) and any(e.level for e in P.ledges): seen.add("a point and a line edge at level 1")
        if P.census["depth_only"]: seen.add("depth test alone")
        if P.census.get("left_round_2"): seen.add("a line leaves round 2")
        if P.fixed_by_line_only: seen.add("fixed through a line only")
        if P.census["failed_inv4"]: seen.add("failed 4 x 4 inverse")
        if not P.edges and P.ledges: seen.add("lines only")
    need = {"zero edges", "both rounds with two iterations", "rejected step", "a point and a line edge at level 1", "depth test alone", "a line leaves round 2",
            "fixed through a line only", "failed 4 x 4 inverse", "lines only"}
    assert need <= seen, need - seen


def test_the_line_oplus_host_build_equals_the_restatement():
    rng = np.random.default_rng(5)
    lines = np.array([LS.pluecker(rng.normal(size=3) * 3, rng.normal(size=3) * 3 + 5) for _ in range(40)])
    lines[::4] *= rng.uniform(0.2, 5.0, (10, 1))                 # not normalised: create_vertex takes the table's six doubles as they are
    ups = rng.normal(size=(40, 4)) * np.array([0.05, 0.05, 0.05, 0.3])
    ups[:8] = 0.0
    for d in range(4):
        ups[2 * d, d], ups[2 * d + 1, d] = 1e-9, -1e-9               # the numeric Jacobian's updates
    ups[8] = [0.9, 0.9, 0.9, 0.1]                                    # a negative radicand: NaN, followed literally
    got = plp.model_line_oplus(lines, ups)
    want = np.array([LREF.line_oplus([float(v) for v in l], [float(v) for v in u]) for l, u in zip(lines, ups)])
    assert S.same(dict(o=got), dict(o=want)) and np.isnan(got[8]).all() and np.isfinite(np.delete(got, 8, 0)).all()


# ---- anchors
def points_of(o):
    return {k: o[k] for k in plp.LOCAL_BA_OUTPUTS}


@pytest.mark.parametrize("how", ["LL = 0", "all lines erased"])
@pytest.mark.parametrize("name", ["mono", "rgbd", "fisheye"])
def test_a_without_a_line_edge_the_points_outputs_are_the_point_adjusters(name, how):
    sc = dict(census()[name])
    F, L, T, LL, TL = LS.dims(sc)
    if how == "LL = 0":
        sc.update(pluecker=np.zeros((0, 6)), obs_offsets_lines=np.zeros(1, np.int32), obs_kf_lines=np.zeros(0, np.int32), obs_idx_lines=np.zeros(0, np.int32),
                  line_erased=np.zeros(0, np.uint8))
        LL = TL = 0
    else:
        sc["line_erased"] = np.ones(LL, np.uint8)
    got = plp.model_local_ba_lines(**LS.call_args(sc), out=LS.sentinel_out(1, F, L, T, LL, TL))
    want = plp.model_local_ba(**S.call_args(sc), out=S.sentinel_out(1, F, L, T))
    assert want["status"][0] == plp.LOCAL_BA_OK and want["round_info"][0, 0, 0] >= 2
    assert S.same(points_of(got), want)
    assert (got["line_role"] == 0).all() and (got["pluecker"] == -7.5).all() and (got["outlier_lines"] == 77).all()


@pytest.mark.parametrize("robust", [True, False])
def test_b_the_pose_block_over_line_edges_is_d15s(robust):
    """one free key frame that sees every line once, no landmark: the line edges of the adjuster are the pose optimiser's, in its order"""
    sc = LS.without_points(LS.make_scene(51, 1, 0, 3, 14, line_obs_share=1.0, line_min_obs=1, noise=1.0, n_other=0))
    lin = plp.model_local_ba_lines_linearize(robust=robust, **LS.call_args(sc))
    assert lin["free_kf"].tolist() == [0] and (sc["obs_kf_lines"] == 0).all()
    idx = sc["obs_idx_lines"]
    lines = dict(valid=np.ones((1, len(idx)), np.uint8), keylines=sc["keylines"][0, idx][None], pos_w=sc["pluecker"][None], inv_level_sigma_sq_lsd=LS.INV_SIGMA_SQ_LSD)
    d15 = plp.model_pose_linearize(sc["camera"], S.MONO, sc["pose"][:1], np.zeros((1, 1), np.uint8), np.zeros((1, 1), plp.KP_DTYPE), np.zeros((1, 1, 3)), S.INV_SIGMA_SQ,
                                   lines=lines, robust=robust)
    assert lin["Hpp"][0].tobytes() == d15["H"][0].tobytes() and lin["bp"][0].tobytes() == d15["b"][0].tobytes()
    assert np.float64(lin["chi2"]).tobytes() == d15["chi2"][0].tobytes() and lin["edge_chi2_lines"].tobytes() == d15["edge_chi2_lines"][0].tobytes()


def test_c_the_line_jacobian_agrees_with_central_differences():
    sc = LS.make_scene(52, 2, 2, 10, 12, noise=0.5)
    P = LREF.Problem(LS.ref_tables(sc), [int(v) for v in sc["kf_local"]])
    P.round_setup()
    Hpp, Hll, Hnn, W, Wn, chi = P.linearize_all(True)
    worst = 0.0
    for e in P.ledges:
        est, Lc = P.kf_est[e.kf], P.ln_est[e.l]
        for c in range(4):
            h = 1e-5
            up = [0.0] * 4; dn = [0.0] * 4; up[c] = h; dn[c] = -h
            eh = R15.line_error(est, P.Tb.cam, LREF.line_oplus(Lc, up), e.xs, e.ys, e.xe, e.ye, e.w)[1]
            el = R15.line_error(est, P.Tb.cam, LREF.line_oplus(Lc, dn), e.xs, e.ys, e.xe, e.ye, e.w)[1]
            for r in range(2):
                worst = max(worst, abs((eh[r] - el[r]) / (2 * h) - e.Jl[4 * r + c]) / max(abs(v) for v in e.Jl))
    print("line Jacobian against central differences:", worst)
    assert worst <= BOUND_JACOBIAN
    # ... and the host build's line blocks are the restatement's
    lin = plp.model_local_ba_lines_linearize(robust=True, **LS.call_args(sc))
    assert lin["free_kf"].tolist() == P.pa
    for i, f in enumerate(P.pa):
        assert np.array(Hpp[f]).tobytes() == np.concatenate([lin["Hpp"][i], lin["bp"][i]]).tobytes()
    for l, v in Hll.items():
        assert np.array(v).tobytes() == np.concatenate([lin["Hll"][l], lin["bl"][l]]).tobytes()
    for l, v in Hnn.items():
        assert np.array(v).tobytes() == np.concatenate([lin["Hnn"][l], lin["bn"][l]]).tobytes()
    for t, v in Wn.items():
        assert np.array(v).tobytes() == lin["W_lines"][t].tobytes()
    assert np.float64(chi).tobytes() == np.float64(lin["chi2"]).tobytes()


def sym(tri, n):
    A = np.zeros((n, n))
    A[np.triu_indices(n)] = tri
    return A + np.triu(A, 1).T


def test_d_the_mixed_schur_solve_agrees_with_the_dense_solve():
    sc = LS.make_scene(53, 3, 2, 30, 10, noise=0.5)
    P = LREF.Problem(LS.ref_tables(sc), [int(v) for v in sc["kf_local"]])
    P.round_setup()
    Hpp, Hll, Hnn, W, Wn, chi = P.linearize_all(True)
    lam = 1e-5 * max(max(abs(Hpp[f][R15.h_index(j, j)]) for f in P.pa for j in range(6)), max(abs(Hnn[l][j]) for l in P.na for j in (0, 4, 7, 9)))
    ok, xp, xl, xn, bad4 = LREF.mixed_schur_solve(P.pa, P.la, P.na, P.by_pose, P.by_lm, P.by_pose_l, P.by_ln, Hpp, Hll, Hnn, W, Wn, lam)
    assert ok and not bad4
    np_, nl, nn = len(P.pa), len(P.la), len(P.na)
    n = 6 * np_ + 3 * nl + 4 * nn
    A = np.zeros((n, n)); b = np.zeros(n)
    ip = {f: 6 * i for i, f in enumerate(P.pa)}
    il = {l: 6 * np_ + 3 * i for i, l in enumerate(P.la)}
    iN = {l: 6 * np_ + 3 * nl + 4 * i for i, l in enumerate(P.na)}
    for f in P.pa:
        A[ip[f]:ip[f] + 6, ip[f]:ip[f] + 6] = sym(Hpp[f][:21], 6); b[ip[f]:ip[f] + 6] = Hpp[f][21:]
    for l in P.la:
        A[il[l]:il[l] + 3, il[l]:il[l] + 3] = sym(Hll[l][:6], 3); b[il[l]:il[l] + 3] = Hll[l][6:]
        for e in P.by_lm[l]:
            if e.kf in ip:
                A[ip[e.kf]:ip[e.kf] + 6, il[l]:il[l] + 3] = np.array(W[e.t]).reshape(6, 3); A[il[l]:il[l] + 3, ip[e.kf]:ip[e.kf] + 6] = np.array(W[e.t]).reshape(6, 3).T
    for l in P.na:
        A[iN[l]:iN[l] + 4, iN[l]:iN[l] + 4] = sym(Hnn[l][:10], 4); b[iN[l]:iN[l] + 4] = Hnn[l][10:]
        for e in P.by_ln[l]:
            if e.kf in ip:
                A[ip[e.kf]:ip[e.kf] + 6, iN[l]:iN[l] + 4] = np.array(Wn[e.t]).reshape(6, 4); A[iN[l]:iN[l] + 4, ip[e.kf]:ip[e.kf] + 6] = np.array(Wn[e.t]).reshape(6, 4).T
    x = np.linalg.solve(A + lam * np.eye(n), b)
    mine = np.concatenate([np.array(xp[f]) for f in P.pa] + [np.array(xl[l]) for l in P.la] + [np.array(xn[l]) for l in P.na])
    worst = np.abs(mine - x).max() / np.abs(x).max()
    print("mixed Schur solve against the dense solve:", worst)
    assert worst <= BOUND_SOLVE
    # ... and the host build's solve from the same blocks is the restatement's
    e3 = [e for l in P.la for e in P.by_lm[l]]; e4 = [e for l in P.na for e in P.by_ln[l]]
    zero3, zero4 = [0.0] * 18, [0.0] * 24
    pidx = {f: i for i, f in enumerate(P.pa)}
    gp, gl, gn, gok = plp.model_local_ba_lines_solve(
        [Hpp[f][:21] for f in P.pa], [Hpp[f][21:] for f in P.pa], [Hll[l][:6] for l in P.la], [Hll[l][6:] for l in P.la], [Hnn[l][:10] for l in P.na],
        [Hnn[l][10:] for l in P.na], [pidx.get(e.kf, -1) for e in e3], [P.la.index(e.l) for e in e3], [W.get(e.t, zero3) for e in e3],
        [pidx.get(e.kf, -1) for e in e4], [P.na.index(e.l) for e in e4], [Wn.get(e.t, zero4) for e in e4], lam)
    assert gok
    assert gp.tobytes() == np.array([xp[f] for f in P.pa]).tobytes() and gl.tobytes() == np.array([xl[l] for l in P.la]).tobytes()
    assert gn.tobytes() == np.array([xn[l] for l in P.na]).tobytes()


@pytest.mark.parametrize("name", ["mono", "rgbd", "fisheye"])
def test_h_without_lines_the_model_entries_are_the_point_adjusters(name):
    """the linearisation and the damped solve are written once for both adjusters (csrc/local_ba.hpp's la_round_setup and la_solve_system with an
    extension for the lines): with no line, the lines' model entries return what the points' return, bit for bit, a failed solve included"""
    sc = dict(census()[name])
    sc.update(pluecker=np.zeros((0, 6)), obs_offsets_lines=np.zeros(1, np.int32), obs_kf_lines=np.zeros(0, np.int32), obs_idx_lines=np.zeros(0, np.int32),
              line_erased=np.zeros(0, np.uint8))
    for robust in (True, False):
        lin = plp.model_local_ba_linearize(**S.call_args(sc), robust=robust)
        lin_l = plp.model_local_ba_lines_linearize(robust=robust, **LS.call_args(sc))
        shared = ("free_kf", "Hpp", "bp", "Hll", "bl")
        assert len(lin["free_kf"]) >= 2 and S.same({k: lin_l[k] for k in shared}, {k: lin[k] for k in shared})
        assert np.float64(lin_l["chi2"]).tobytes() == np.float64(lin["chi2"]).tobytes()
        assert lin_l["Hnn"].shape == (0, 10) and lin_l["W_lines"].shape == (0, 6, 4) and lin_l["edge_chi2_lines"].shape == (0,)
    # the blocks of the last linearisation (Huber off) as a solve's arguments, as tests/test_local_ba_cpu.py builds them
    row = {int(f): i for i, f in enumerate(lin["free_kf"])}
    ts = np.where(~np.isnan(lin["edge_chi2"]))[0]
    e_pose = np.array([row.get(int(sc["obs_kf"][t]), -1) for t in ts])
    e_lm = (np.searchsorted(sc["obs_offsets"], np.arange(len(sc["obs_kf"])), side="right") - 1)[ts]
    W = np.nan_to_num(lin["W"][ts])
    Hll, bl = np.nan_to_num(lin["Hll"]), np.nan_to_num(lin["bl"])
    lam = 1e-5 * max(np.abs(lin["Hpp"][:, [0, 6, 11, 15, 18, 20]]).max(), np.abs(Hll[:, [0, 3, 5]]).max())
    bad_pivot = lin["Hpp"].copy(); bad_pivot[-1, 20] = -1e12                 # the last pivot of the reduced system is negative
    singular = Hll.copy(); singular[e_lm[0]] = 0.0                           # a landmark block without an inverse at lambda = 0
    none_n, none_e = np.zeros((0, 10)), np.zeros(0, np.int32)
    for what, hpp, hll, lm, want_ok in [("regular", lin["Hpp"], Hll, lam, True), ("failed pivot", bad_pivot, Hll, lam, False), ("failed inverse", lin["Hpp"], singular, 0.0, False)]:
        xp, xl, ok = plp.model_local_ba_solve(hpp, lin["bp"], hll, bl, e_pose, e_lm, W, lm)
        gp, gl, gn, gok = plp.model_local_ba_lines_solve(hpp, lin["bp"], hll, bl, none_n, np.zeros((0, 4)), e_pose, e_lm, W, none_e, none_e, np.zeros((0, 6, 4)), lm)
        assert ok == want_ok and gok == ok, what
        assert S.same(dict(xp=gp, xl=gl), dict(xp=xp, xl=xl)) and gn.shape == (0, 4), what
        assert xp.any() == want_ok and xl.any() == want_ok, what


def normalised(L):
    L = np.asarray(L, float)
    return L / np.linalg.norm(L[..., 3:], axis=-1, keepdims=True)


@pytest.mark.parametrize("model,setup", [("perspective", S.MONO), ("fisheye", S.RGBD)])
def test_e_noise_free_scenes_return_to_the_ground_truth(model, setup):
    sc = LS.make_scene(56, 3, 2, 40, 12, model=model, setup=setup, n_other=0, line_min_obs=3, ln_noise=0.005)
    F, L, T, LL, TL = LS.dims(sc)
    got = plp.model_local_ba_lines(**LS.call_args(sc))
    free = got["kf_role"][0] == plp.LOCAL_BA_KF_FREE
    assert free.sum() == 3 and (got["line_role"] == 1).all()
    ln, gt = normalised(got["pluecker"][0]), normalised(sc["pluecker_gt"])
    err_ln = np.minimum(np.abs(ln - gt).max(1), np.abs(ln + gt).max(1)).max()
    worst = max(np.abs(got["pose"][0, free, :12] - sc["pose_gt"][free]).max(), np.abs(got["pos_w"][0] - sc["pos_gt"]).max(), err_ln)
    print("ground truth after 5 + 10 iterations:", model, worst, "lines", err_ln)
    assert worst <= BOUND_TRUTH
    assert not got["outlier"].any() and not got["outlier_lines"].any()


def test_f_the_line_outlier_bytes_are_the_generating_labels():
    # six or seven views of every line at one octave, so that the five robust iterations of round 1 leave every inlier below the threshold
    sc = LS.make_scene(58, 3, 4, 40, 16, n_other=0, line_outliers=5, outliers=4, line_min_obs=6, line_obs_share=0.9, line_octaves=1, pose_noise=0.003, lm_noise=0.01,
                       ln_noise=0.01)
    assert sc["label_lines"].sum() >= 3
    got = plp.model_local_ba_lines(**LS.call_args(sc))
    assert np.array_equal(got["outlier_lines"][0], sc["label_lines"]) and np.array_equal(got["outlier"][0], sc["label"])
    assert got["round_info"][0, 0, 2] == sc["label_lines"].sum() + sc["label"].sum()


@pytest.mark.parametrize("name", ["mono", "rgbd", "fisheye", "far_start", "lines_only", "through_a_line"])
def test_g_the_robust_chi2_of_a_round_never_rises(name):
    got, want, r = run(name)
    P = r["problem"]
    assert len(P.start_chi) == 2
    for rnd in range(2):
        assert got["round_chi2"][0, rnd, 0] <= P.start_chi[rnd], (rnd, got["round_chi2"][0, rnd, 0], P.start_chi[rnd])


def test_refused_calls_write_nothing():
    sc = dict(census()["mono"])
    d = LS.dims(sc)
    out = LS.sentinel_out(1, *d)
    a = LS.call_args(sc)
    eq = S.PS.camera("perspective"); eq.model = plp.CAMERA_EQUIRECTANGULAR
    with pytest.raises(plp.PlpError) as e:
        plp.model_local_ba_lines(**dict(a, camera=eq), out=out)
    assert e.value.status == plp.PLP_ERR_UNSUPPORTED
    with pytest.raises(plp.PlpError) as e:
        plp.model_local_ba_lines(**dict(a, inv_level_sigma_sq_lsd=np.ones(17, np.float32)), out=out)
    assert e.value.status == plp.PLP_ERR_INVALID_ARG
    with pytest.raises(plp.PlpError) as e:
        plp.model_local_ba_lines(**dict(a, obs_offsets_lines=sc["obs_offsets_lines"][::-1].copy()), out=out)
    assert e.value.status == plp.PLP_ERR_INVALID_ARG
    assert S.same(out, LS.sentinel_out(1, *d))
