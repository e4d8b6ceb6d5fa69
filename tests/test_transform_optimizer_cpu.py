"""optimize::transform_optimizer without a GPU: the host build of csrc/transform_opt.hpp (plp.model_transform_optimize, model_transform_linearize,
model_sim3_exp, model_chol7, model_pose_exp) against the plain-Python restatement of DESIGN.md section 5, D16 (tests/transform_optimizer_ref.py),
bit for bit on every output; exp against math.exp within D16's recorded bound; two anchors that do not rest on D16 (the ground truth of
noise-free scenes, the generating labels of gross outliers); a census of the branches the scenes reach; the refusals of the C ABI."""
import functools
import math

import numpy as np
import pytest

import transform_optimizer_ref as REF
import transform_optimizer_scene as S
from plp import plp

SENT = {np.dtype(np.uint8): 0xA5, np.dtype(np.int32): -77777, np.dtype(np.float64): -987.25}
# D16: the largest relative error of pose_exp against math.exp measured on 400 001 dense and 400 000 random arguments of [-1, 1] and of
# [-700, 700] is 2.22e-16; the bound is ten times that
EXP_MEASURED, EXP_BOUND = 2.22e-16, 2.22e-15
# D16: the largest errors of the restatement against the ground truth on the noise-free scenes below (rotation angle in rad, translation in m,
# relative scale: 5.6e-8, 2.9e-7, 4.5e-7; the key points are rounded to float); the bounds are ten times those
TRUTH_MEASURED = (5.6e-8, 2.9e-7, 4.5e-7)
TRUTH_BOUND = (5.6e-7, 2.9e-6, 4.5e-6)


def same_values(a, b):
    """the same bits, a NaN equal to any NaN"""
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and np.nan_to_num(a, nan=0.0).tobytes() == np.nan_to_num(b, nan=0.0).tobytes()


def sentinels(P, N):
    return {k: np.full((P,) + shape(N), SENT[np.dtype(dt)], dt) for k, (shape, dt, _) in plp.TRANSFORM_OPT_OUTPUTS.items()}


def compare(A, got, refs):
    """every output of the host build against the restatement's, problem by problem; slots the reference does not write keep the sentinel"""
    for p, w in enumerate(refs):
        assert int(got["status"][p]) == w["status"] and int(got["num_valid"][p]) == w["num_valid"] and int(got["num_inliers"][p]) == w["num_inliers"], (p, w)
        for k in ("rot_12", "trans_12", "scale_12", "world_to_1", "round_chi2"):
            assert same_values(got[k][p], w[k]), (p, k, got[k][p], w[k])
        assert got["round_info"][p].tolist() == w["round_info"], (p, got["round_info"][p], w["round_info"])
        cnt = int(A["counts"][p])
        assert got["kept"][p, :cnt].tolist() == w["kept"], p
        assert (got["kept"][p, cnt:] == SENT[np.dtype(np.uint8)]).all(), p


@functools.lru_cache(maxsize=None)
def census_run(model, fix_scale):
    """the census problems of one camera and one fix_scale: (pack, host build outputs on sentinels, restatement results)"""
    A = S.pack(S.census_problems(model, fix_scale), holes=0.25, seed=3)
    P, N = A["valid"].shape
    got = plp.model_transform_optimize(out=sentinels(P, N), **S.call_args(A))
    refs = [REF.optimize(q, kept=[SENT[np.dtype(np.uint8)]] * len(q.slots)) for q in S.ref_problems(A)]
    return A, got, refs


@functools.lru_cache(maxsize=None)
def nan_run():
    A = S.pack([S.nan_in_round_2_problem()])
    P, N = A["valid"].shape
    got = plp.model_transform_optimize(out=sentinels(P, N), **S.call_args(A, inv_level_sigma_sq_1=S.INV_SIGMA_SQ_W0))
    refs = [REF.optimize(q, kept=[SENT[np.dtype(np.uint8)]] * len(q.slots)) for q in S.ref_problems(A, sig1=S.INV_SIGMA_SQ_W0)]
    return A, got, refs


# ---- the pieces
def exp_arguments():
    rng = np.random.default_rng(1)
    return np.concatenate([np.linspace(-1.0, 1.0, 20001), rng.uniform(-1.0, 1.0, 20000), np.linspace(-700.0, 700.0, 20001), rng.uniform(-700.0, 700.0, 20000),
                           [0.0, -0.0, 1e-300, -1e-300, 700.0, -700.0, 0.5 * math.log(2.0), -0.5 * math.log(2.0), 1e-9, -1e-9, 1e-5, 0.03, -0.03]])


def test_pose_exp_is_the_restatements_bit_for_bit():
    x = np.concatenate([exp_arguments(), [np.nextafter(700.0, 800.0), -np.nextafter(700.0, 800.0), 1e6, np.inf, -np.inf, np.nan]])
    assert same_values(plp.model_pose_exp(x), [REF.exp(float(v)) for v in x])


def test_pose_exp_against_math_exp_within_the_recorded_bound():
    x = exp_arguments()
    got = plp.model_pose_exp(x)
    want = np.array([math.exp(float(v)) for v in x])
    err = float(np.max(np.abs(got - want) / want))
    print(f"pose_exp: largest relative error {err:.3e} (recorded {EXP_MEASURED:.3e}, bound {EXP_BOUND:.3e})")
    assert err <= EXP_BOUND
    assert plp.model_pose_exp([0.0])[0] == 1.0
    outside = plp.model_pose_exp([np.nextafter(700.0, 800.0), -701.0, np.inf, -np.inf, np.nan])
    assert np.isnan(outside).all()                            # outside the domain: NaN, and so a rejected step


def sim3_exp_cases():
    rng = np.random.default_rng(2)
    u = rng.normal(size=(400, 7)) * np.array([0.05] * 3 + [0.2] * 3 + [0.05])
    u[:60, :3] *= 1e-6                                        # theta < eps
    u[40:120, 6] *= 1e-6                                      # |sigma| < eps: both sides of both thresholds, in all four combinations
    u[120:130] = 0.0
    u[130, :3] = [1e-5, 0.0, 0.0]; u[131, 6] = 1e-5; u[132, 6] = -1e-5; u[133, 6] = 701.0; u[134, :3] = [2e6, 0.0, 0.0]; u[135, 6] = np.nan
    for d in range(7):
        u[136 + 2 * d] = 0.0; u[136 + 2 * d, d] = 1e-9
        u[137 + 2 * d] = 0.0; u[137 + 2 * d, d] = -1e-9
    q = rng.normal(size=(400, 4)); q /= np.linalg.norm(q, axis=1, keepdims=True)
    est = np.concatenate([q, rng.normal(size=(400, 3)), rng.uniform(0.5, 2.0, (400, 1))], 1)
    return u, est


@pytest.mark.parametrize("fix_scale", [False, True])
def test_sim3_exp_times_estimate_bit_for_bit(fix_scale):
    u, est = sim3_exp_cases()
    got = plp.model_sim3_exp(u, est, fix_scale)
    want = [REF.oplus([float(v) for v in u[i]], [float(v) for v in est[i]], fix_scale) for i in range(len(u))]
    assert same_values(got, want)
    reached = {REF.sim3_branch([float(v) for v in row], fix_scale) for row in u}
    assert reached == ({(True, True), (True, False)} if fix_scale else {(True, True), (True, False), (False, True), (False, False)})
    if fix_scale:                                             # sigma is taken as 0: the scale is the estimate's, bit for bit
        assert np.array_equal(got[:130, 7], est[:130, 7])


def test_chol7_bit_for_bit_and_its_failures():
    rng = np.random.default_rng(3)
    n = 200
    J = rng.normal(size=(n, 12, 7))
    H = np.einsum("nki,nkj->nij", J, J)
    H[150:160, 6, :] = 0.0; H[150:160, :, 6] = 0.0              # fix_scale: a zero row and column, solvable with lambda > 0
    H[160:170] *= -1.0                                        # not positive
    H[170, 2, 2] = np.nan; H[171, 0, 0] = np.inf; H[172] = 0.0
    b = rng.normal(size=(n, 7)); b[150:160, 6] = 0.0
    lam = rng.uniform(1e-6, 1e-2, n); lam[172] = 0.0
    iu = np.triu_indices(7)
    H28 = H[:, iu[0], iu[1]]
    x, ok = plp.model_chol7(H28, b, lam)
    for i in range(n):
        wx, wok = REF.chol7([float(v) for v in H28[i]], [float(v) for v in b[i]], float(lam[i]))
        assert bool(ok[i]) == wok and same_values(x[i], wx), i
    assert ok[:160].all() and not ok[160:173].any() and (x[160:173] == 0.0).all()
    assert (x[150:160, 6] == 0.0).all()
    good = np.flatnonzero(ok)[:150]
    full = H[good] + lam[good, None, None] * np.eye(7)
    assert np.allclose(np.einsum("nij,nj->ni", full, x[good]), b[good], rtol=0, atol=1e-8)


@pytest.mark.parametrize("fix_scale", [False, True])
def test_one_linearisation_bit_for_bit(fix_scale):
    pr = [S.make_problem(50 + i, 9 + 20 * i, fix_scale=fix_scale, noise=1.0, outlier_share=0.2) for i in range(3)] + [S.z0_problem(fix_scale=fix_scale)]
    A = S.pack(pr, holes=0.3, seed=4)
    P, N = A["valid"].shape
    active = (np.random.default_rng(5).uniform(size=(P, N)) < 0.7).astype(np.uint8)
    for act in (None, active):
        a = S.call_args(A)
        got = plp.model_transform_linearize(active=act, **{k: v for k, v in a.items()})
        for p, q in enumerate(S.ref_problems(A)):
            sums, chi2 = REF.linearize(q, None if act is None else act[p])
            assert same_values(np.concatenate([got["H"][p], got["b"][p], [got["chi2"][p]]]), sums), p
            want = np.full((N, 2), np.nan)
            for s, c in chi2.items():
                want[s] = c
            assert same_values(got["edge_chi2"][p], want), p
    if fix_scale:                                             # column 6 of the Jacobian is exactly zero by construction
        for t in [REF.h_index(i, 6) for i in range(7)] + [28 + 6]:
            assert (np.concatenate([got["H"], got["b"]], 1)[:3, t] == 0.0).all()


# ---- the whole call
@pytest.mark.parametrize("model", ["perspective", "fisheye"])
@pytest.mark.parametrize("fix_scale", [False, True])
def test_the_whole_call_bit_for_bit_on_every_output(model, fix_scale):
    compare(*census_run(model, fix_scale))


def test_the_scene_whose_round_2_ends_on_a_nan_bit_for_bit():
    compare(*nan_run())


@pytest.mark.parametrize("num_iter", [1, 3])
def test_other_iteration_counts_and_thresholds_bit_for_bit(num_iter):
    A = S.pack([S.make_problem(60 + i, 30 + 25 * i, noise=1.0, outlier_share=0.2, rot=0.05, trans=0.1) for i in range(3)], holes=0.2, seed=6)
    P, N = A["valid"].shape
    got = plp.model_transform_optimize(out=sentinels(P, N), num_iter=num_iter, chi_sq=7.5, **S.call_args(A))
    compare(A, got, [REF.optimize(q, num_iter=num_iter, kept=[SENT[np.dtype(np.uint8)]] * len(q.slots)) for q in S.ref_problems(A, chi_sq=7.5)])


def test_optional_outputs_absent_and_counts_absent():
    A = S.pack([S.make_problem(70, 25, noise=0.5)], holes=0.2, seed=7)
    full = plp.model_transform_optimize(**S.call_args(A))
    part = plp.model_transform_optimize(outputs=(), **S.call_args(A))
    assert set(full) - set(part) == {"world_to_1", "round_info", "round_chi2"}
    for k in part:
        assert same_values(part[k], full[k]), k
    B = dict(A, valid=np.where(np.arange(A["valid"].shape[1])[None] < A["counts"][:, None], A["valid"], 0).astype(np.uint8))
    none = plp.model_transform_optimize(**S.call_args(B, counts=None))
    for k in full:
        assert same_values(none[k], full[k]), k


# ---- anchors that do not rest on D16
def truth_errors(q, rot_12, trans_12, scale_12):
    s, R, t = q["truth"]
    Rg = np.asarray(rot_12).reshape(3, 3)
    ang = math.acos(max(-1.0, min(1.0, (float(np.trace(Rg.T @ R)) - 1.0) / 2.0)))
    return ang, float(np.max(np.abs(np.asarray(trans_12) - t))), abs(float(scale_12) - s) / s


@functools.lru_cache(maxsize=None)
def noise_free_scenes():
    out = []
    for fix in (False, True):
        for model in ("perspective", "fisheye"):
            pr = [S.make_problem(2000 + i, 40 + 10 * i, model=model, fix_scale=fix) for i in range(4)]
            out.append((pr, S.pack(pr, holes=0.2, seed=1)))
    return out


def test_noise_free_scenes_return_the_ground_truth():
    worst_ref, worst = [0.0] * 3, [0.0] * 3
    for pr, A in noise_free_scenes():
        got = plp.model_transform_optimize(**S.call_args(A))
        for p, (q, Pb) in enumerate(zip(pr, S.ref_problems(A))):
            r = REF.optimize(Pb)
            assert r["status"] == REF.OK and r["num_inliers"] == len(q["x1"])
            worst_ref = [max(a, b) for a, b in zip(worst_ref, truth_errors(q, r["rot_12"], r["trans_12"], r["scale_12"]))]
            assert got["status"][p] == plp.TRANSFORM_OPT_OK and got["num_inliers"][p] == len(q["x1"])
            worst = [max(a, b) for a, b in zip(worst, truth_errors(q, got["rot_12"][p], got["trans_12"][p], got["scale_12"][p]))]
            w = got["world_to_1"][p]                          # Sim3_12 * (rot_2w, trans_2w, 1): the same scale, R_12 R_2w, s R_12 t_2w + t_12
            R12, t12, s12 = got["rot_12"][p].reshape(3, 3), got["trans_12"][p], got["scale_12"][p]
            R2, t2 = A["pose_2"][p, :9].reshape(3, 3), A["pose_2"][p, 9:12]
            # (D16 normalises no quaternion: its norm drifts by some 1e-11 over the updates, and the two matrices are formed from different quaternions)
            assert np.allclose(w[:9].reshape(3, 3), R12 @ R2, rtol=0, atol=1e-9) and np.allclose(w[9:12], s12 * R12 @ t2 + t12, rtol=0, atol=1e-8) and w[12] == s12
    print(f"restatement vs truth {worst_ref} (recorded {TRUTH_MEASURED}), host build {worst}, bound {TRUTH_BOUND}")
    assert all(e <= b for e, b in zip(worst_ref, TRUTH_BOUND)) and all(e <= b for e, b in zip(worst, TRUTH_BOUND))


def test_gross_outliers_are_exactly_the_generating_labels():
    """noise-free inliers; outliers displaced by 20 px or more in one image: chi2 >= 400 / 1.2^14 = 31 > 10 at every octave"""
    for fix in (False, True):
        for model in ("perspective", "fisheye"):
            pr = [S.make_problem(2100 + i, 60 + 10 * i, model=model, fix_scale=fix, outlier_share=0.25) for i in range(3)]
            A = S.pack(pr, holes=0.2, seed=2)
            got = plp.model_transform_optimize(**S.call_args(A))
            for p, (q, Pb) in enumerate(zip(pr, S.ref_problems(A))):
                assert q["label"].any()
                want = 1 - q["label"]
                assert np.array_equal(np.asarray(REF.optimize(Pb)["kept"])[A["slot"][p]], want), "the restatement alone must meet the anchor"
                assert np.array_equal(got["kept"][p, A["slot"][p]], want) and got["num_inliers"][p] == want.sum() and got["status"][p] == plp.TRANSFORM_OPT_OK


# ---- what the scenes reach
def test_census_of_the_branches_reached():
    runs = [census_run(m, f) for m in ("perspective", "fisheye") for f in (False, True)] + [nan_run()]
    refs = [w for _, _, rs in runs for w in rs]
    info = np.array([w["round_info"] for w in refs])
    census = dict(
        status_ok=sum(w["status"] == REF.OK for w in refs), status_too_few=sum(w["status"] == REF.TOO_FEW_INLIERS for w in refs),
        rejected_steps=int((info[:, :, 1] > 0).sum()), end_iterations=int((info[:, :, 3] == REF.END_ITERATIONS).sum()),
        end_ten_tries=int((info[:, :, 3] == REF.END_TRIES).sum()), end_rho_zero=int((info[:, :, 3] == REF.END_RHO_ZERO).sum()),
        nan_outlier_round1=sum(w["census"]["nan_outlier_round1"] for w in refs), nan_inlier_round2=sum(w["census"]["nan_inlier_round2"] for w in refs),
        drops_round1=int((info[:, 0, 2] > 0).sum()), drops_round2=int((info[:, 1, 2] > 0).sum()),
        fix_scale_on=sum(bool(A["fix_scale"]) for A, _, _ in runs), fix_scale_off=sum(not A["fix_scale"] for A, _, _ in runs),
        num_valid_0=sum(w["num_valid"] == 0 for w in refs), num_valid_1=sum(w["num_valid"] == 1 for w in refs), num_valid_9=sum(w["num_valid"] == 9 for w in refs),
        num_valid_10=sum(w["num_valid"] == 10 for w in refs))
    for sig_small in (True, False):
        for th_small in (True, False):
            census[f"sim3_update_sigma_{'small' if sig_small else 'large'}_theta_{'small' if th_small else 'large'}"] = sum(
                (sig_small, th_small) in w["census"]["branches"] for w in refs)
    print(census)
    assert all(v > 0 for v in census.values()), {k: v for k, v in census.items() if not v}
    # nothing is optimised for an empty graph, and round 1 runs for a single match
    for w in refs:
        if w["num_valid"] == 0:
            assert w["round_info"] == [[0, 0, 0, 0], [0, 0, 0, 0]] and w["status"] == REF.TOO_FEW_INLIERS
        if w["num_valid"] in (1, 9):
            assert w["round_info"][0][0] > 0 and w["round_info"][1] == [0, 0, 0, 0] and w["status"] == REF.TOO_FEW_INLIERS


def test_the_early_return_hands_the_input_back_and_keeps_the_drops():
    A, got, refs = census_run("perspective", False)
    seen = 0
    for p, w in enumerate(refs):
        if w["status"] == REF.TOO_FEW_INLIERS:
            assert np.array_equal(got["rot_12"][p], A["rot_12"][p]) and np.array_equal(got["trans_12"][p], A["trans_12"][p])
            assert got["scale_12"][p] == np.float64(A["scale_12"][p]) and got["num_inliers"][p] == 0
            if w["round_info"][0][2] > 0:
                seen += 1
                assert (got["kept"][p, A["slot"][p]] == 0).sum() == w["round_info"][0][2]
    assert seen


# ---- the mirror class and the C ABI
def test_the_mirror_class_runs_one_pair():
    q = S.make_problem(80, 50, noise=0.5, outlier_share=0.2)
    A = S.pack([q])
    want = plp.model_transform_optimize(**S.call_args(A))
    n, r = plp.transform_optimizer(False, 10).optimize(A["camera"], A["valid"][0], A["pos_w_1"][0], A["pos_w_2"][0], A["undist_1"][0], A["undist_2"][0], A["pose_1"][0],
                                                       A["pose_2"][0], A["rot_12"][0].reshape(3, 3), A["trans_12"][0], A["scale_12"][0], S.INV_SIGMA_SQ, S.INV_SIGMA_SQ)
    assert n == int(want["num_inliers"][0]) and n >= 20
    for k in want:
        assert same_values(r[k], want[k][0]), k


REFUSALS = [
    ("equirectangular", lambda a: setattr(a["camera"], "model", plp.CAMERA_EQUIRECTANGULAR), plp.PLP_ERR_UNSUPPORTED),
    ("unknown model", lambda a: setattr(a["camera"], "model", 7), plp.PLP_ERR_INVALID_ARG),
    ("fx 0", lambda a: setattr(a["camera"], "fx", 0.0), plp.PLP_ERR_INVALID_ARG),
    ("fy NaN", lambda a: setattr(a["camera"], "fy", float("nan")), plp.PLP_ERR_INVALID_ARG),
    ("cx inf", lambda a: setattr(a["camera"], "cx", float("inf")), plp.PLP_ERR_INVALID_ARG),
    ("num_iter 0", lambda a: a.update(num_iter=0), plp.PLP_ERR_INVALID_ARG),
    ("chi_sq 0", lambda a: a.update(chi_sq=0.0), plp.PLP_ERR_INVALID_ARG),
    ("chi_sq NaN", lambda a: a.update(chi_sq=float("nan")), plp.PLP_ERR_INVALID_ARG),
    ("no levels", lambda a: a.update(inv_level_sigma_sq_1=np.zeros(0, np.float32), inv_level_sigma_sq_2=np.zeros(0, np.float32)), plp.PLP_ERR_INVALID_ARG),
    ("17 levels", lambda a: a.update(inv_level_sigma_sq_1=np.ones(17, np.float32), inv_level_sigma_sq_2=np.ones(17, np.float32)), plp.PLP_ERR_INVALID_ARG),
]


@pytest.mark.parametrize("name,change,status", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_write_nothing(name, change, status):
    A = S.pack([S.make_problem(90, 20)])
    a = S.call_args(A, camera=S.camera("perspective"))
    change(a)
    out = sentinels(*A["valid"].shape)
    with pytest.raises(plp.PlpError) as e:
        plp.model_transform_optimize(out=out, **a)
    assert e.value.status == status
    for k, v in out.items():
        assert (v == SENT[v.dtype]).all(), k


def test_refusals_of_the_raw_entry_and_limits():
    import ctypes as C
    L = plp.lib()
    assert L.plp_model_transform_optimize_host(None) == -plp.PLP_ERR_INVALID_ARG
    A = S.pack([S.make_problem(91, 12)])
    a, keep, P, N = plp._transform_optimize_inputs(num_iter=10, chi_sq=10.0, **S.call_args(A))
    assert L.plp_model_transform_optimize_host(C.byref(a)) == -plp.PLP_ERR_INVALID_ARG          # required outputs are NULL
    a.P = 0
    assert L.plp_model_transform_optimize_host(C.byref(a)) == 0                                 # P == 0: PLP_OK with nothing written
    a.P, a.n_cap = 1, 8193
    assert L.plp_model_transform_optimize_host(C.byref(a)) == -plp.PLP_ERR_UNSUPPORTED
    a.P, a.n_cap = 65536, N
    assert L.plp_model_transform_optimize_host(C.byref(a)) == -plp.PLP_ERR_UNSUPPORTED
    a.P, a.n_cap = -1, N
    assert L.plp_model_transform_optimize_host(C.byref(a)) == -plp.PLP_ERR_INVALID_ARG
    assert L.plp_model_sim3_exp_host(None, None, 0, 1, None) == -1 and L.plp_model_chol7_host(None, None, None, 1, None, None) == -1
    assert L.plp_model_pose_exp_host(None, 1, None) == -1 and L.plp_model_pose_exp_host(None, 0, None) == 0
