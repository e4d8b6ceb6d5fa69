"""optimize::pose_optimizer / pose_optimizer_extended_line without a GPU: the host build of csrc/pose_opt.hpp (plp.model_pose_optimize,
model_pose_linearize, model_se3_exp, model_chol6, model_pose_sincos) against the plain-Python restatement tests/pose_optimizer_ref.py, bit for
bit; D15's sin / cos against math.sin / math.cos; the point edges' analytic Jacobian against central differences of the restated error; anchors
that do not depend on the definition (the ground-truth pose of noise-free scenes, the generating outlier labels); the census of the cases the
scenes reach; the argument checks.  DESIGN.md section 5, D15 quotes the figures measured here."""
import math

import numpy as np
import pytest

import pose_optimizer_ref as REF
import pose_optimizer_scene as S
from plp import plp

SENT = {np.dtype(np.uint8): 0xA5, np.dtype(np.int32): -77777, np.dtype(np.float64): -987.25}
COMBOS = [(m, s) for m in ("perspective", "fisheye") for s in (S.MONO, S.STEREO, S.RGBD)]


def same_values(a, b):
    """the same bits, a NaN equal to any NaN (the sign and payload of a NaN differ between processors and languages, and no output's meaning carries them)"""
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and np.nan_to_num(a, nan=0.0).tobytes() == np.nan_to_num(b, nan=0.0).tobytes()


def sentinels(P, T):
    B, N = P["valid"].shape
    L = 0 if P["lines"] is None else P["lines"]["valid"].shape[1]
    return {k: np.full((B,) + shape(N, L, T), SENT[np.dtype(dt)], dt) for k, (shape, dt, _) in plp.POSE_OPT_OUTPUTS.items()}


def run_both(P, T=4, I=10):
    """the host build on sentinel-filled outputs and the restatement started from the same sentinels, compared output by output; returns both"""
    got = plp.model_pose_optimize(out=sentinels(P, T), **S.call_args(P, num_trials=T, num_each_iter=I))
    ref = []
    for b, F in enumerate(S.ref_frames(P)):
        cnt = len(F.points)
        lcnt = len(F.lines) if F.lines is not None else 0
        q = REF.optimize(F, T, I, outlier=[0xA5] * cnt, outlier_lines=[0xA5] * lcnt)
        ref.append(q)
        where = (b, q["status"], q["trial_info"])
        assert q["status"] == got["status"][b] and q["num_init_obs"] == got["num_init_obs"][b] and q["num_valid"] == got["num_valid"][b], where
        assert same_values(q["pose"], got["pose"][b]), where
        assert q["trial_info"] == got["trial_info"][b].tolist(), where
        assert same_values(q["trial_chi2"], got["trial_chi2"][b]), where
        assert q["outlier"] == got["outlier"][b, :cnt].tolist() and (got["outlier"][b, cnt:] == 0xA5).all(), where
        if lcnt or P["lines"] is not None:
            assert q["outlier_lines"] == got["outlier_lines"][b, :lcnt].tolist() and (got["outlier_lines"][b, lcnt:] == 0xA5).all(), where
    return got, ref


# ---- item 1: sin and cos, the vertex
def test_sincos_against_libm_on_dense_and_random_arguments():
    """D15 item 1: at most 1e-15 absolute on [-pi, pi].  Measured: 1.12e-16 for both (one unit in the last place below 1)."""
    x = np.concatenate([np.linspace(-math.pi, math.pi, 400001), np.random.default_rng(0).uniform(-math.pi, math.pi, 200000),
                        [0.0, -0.0, math.pi / 4, -math.pi / 4, math.pi / 2, math.pi, -math.pi, 1e-300, 1e-9]])
    s, c = plp.model_pose_sincos(x)
    es = max(abs(float(a) - math.sin(float(v))) for a, v in zip(s, x))
    ec = max(abs(float(a) - math.cos(float(v))) for a, v in zip(c, x))
    print(f"sincos: max |sin - math.sin| = {es:.3e}, max |cos - math.cos| = {ec:.3e}")
    assert es <= 1e-15 and ec <= 1e-15


def test_sincos_host_build_equals_the_restatement_also_outside_pi():
    rng = np.random.default_rng(1)
    x = np.concatenate([rng.uniform(-math.pi, math.pi, 20000), rng.uniform(-100.0, 100.0, 5000), rng.uniform(-1048576.0, 1048576.0, 5000),
                        [1048576.0, -1048576.0, 1048576.5, -2e6, math.inf, -math.inf, math.nan, 0.0, -0.0, 5e-324]])
    s, c = plp.model_pose_sincos(x)
    r = [REF.sincos(float(v)) for v in x]
    assert same_values(s, [a for a, _ in r]) and same_values(c, [b for _, b in r])
    assert np.isnan(s[-6]) and np.isnan(c[-7])         # beyond 2^20 and not finite: NaN (D15)
    # beyond pi the routine still reduces: accuracy against libm at |x| <= 100
    big = x[20000:25000]
    assert max(abs(float(a) - math.sin(float(v))) for a, v in zip(s[20000:25000], big)) <= 1e-15


def test_se3_exp_equals_the_restatement():
    rng = np.random.default_rng(2)
    n = 400
    u = rng.normal(size=(n, 6)) * rng.choice([1e-9, 1e-6, 1e-3, 0.1, 1.0, 4.0], size=(n, 1))     # both branches of exp, |omega| beyond pi
    u[0] = 0.0
    u[1, :3] = [1e-5, 0, 0]
    u[2, :3] = [9.999e-6, 0, 0]
    u[3, 0] = math.nan
    q = rng.normal(size=(n, 4)); q /= np.linalg.norm(q, axis=1, keepdims=True)
    est = np.concatenate([q * np.sign(q[:, 3:4]), rng.normal(size=(n, 3))], 1)
    got = plp.model_se3_exp(u, est)
    want = [REF.oplus([float(v) for v in u[i]], [float(v) for v in est[i]]) for i in range(n)]
    assert same_values(got, want)
    assert (np.abs(np.linalg.norm(got[4:, :4], axis=1) - 1.0) < 1e-15).all() and (got[4:, 3] >= 0).all()     # normalizeRotation


def test_chol6_equals_the_restatement_and_reports_bad_pivots():
    rng = np.random.default_rng(3)
    Hs, bs, ls = [], [], []
    for i in range(200):
        A = rng.normal(size=(8, 6)) * rng.choice([1e-3, 1.0, 1e4])
        H = A.T @ A
        if i % 5 == 1:
            H[:, 3] = H[:, 2]; H[3, :] = H[2, :]       # singular
        if i % 5 == 2:
            H = -H
        if i % 5 == 3:
            H[2, 4] = H[4, 2] = math.nan
        if i % 7 == 6:
            H[:] = 0.0
        Hs.append([H[r, c] for r in range(6) for c in range(r, 6)]); bs.append(rng.normal(size=6)); ls.append(0.0 if i % 3 else 1e-5 * abs(H.diagonal()).max())
    x, ok = plp.model_chol6(Hs, bs, ls)
    want = [REF.chol6([float(v) for v in Hs[i]], [float(v) for v in bs[i]], float(ls[i])) for i in range(200)]
    assert same_values(x, [w[0] for w in want]) and ok.tolist() == [w[1] for w in want]
    assert not ok.all() and ok.any()
    good = [i for i in range(200) if ok[i] and i % 5 == 0]
    for i in good[:20]:                                  # a solve is a solve
        H = np.zeros((6, 6)); H[np.triu_indices(6)] = Hs[i]; H = H + H.T - np.diag(H.diagonal())
        assert np.allclose((H + ls[i] * np.eye(6)) @ x[i], bs[i], rtol=1e-6, atol=1e-9)


@pytest.mark.parametrize("model,setup", COMBOS)
def test_linearize_equals_the_restatement(model, setup):
    frames = [S.make_frame(40 + i, 25, model=model, setup=setup, n_lines=4 * i, noise=1.0, outlier_share=0.2, rot=0.05, trans=0.1) for i in range(2)]
    P = S.pack(frames, holes=0.2, seed=4)
    rng = np.random.default_rng(5)
    act = (rng.uniform(size=P["valid"].shape) < 0.7).astype(np.uint8)
    actl = (rng.uniform(size=P["lines"]["valid"].shape) < 0.7).astype(np.uint8)
    for robust, a, al in ((True, None, None), (False, None, None), (True, act, actl)):
        a_ = S.call_args(P); a_.pop("num_trials", None)
        got = plp.model_pose_linearize(robust=robust, active=a, active_lines=al, **a_)
        for b, F in enumerate(S.ref_frames(P)):
            sums, chi2, lchi2 = REF.linearize(F, robust, None if a is None else a[b], None if al is None else al[b])
            assert same_values(got["H"][b], sums[:21]) and same_values(got["b"][b], sums[21:27]) and same_values(got["chi2"][b], sums[27])
            for s, v in chi2.items():
                assert same_values(got["edge_chi2"][b, s], v)
            for s, v in lchi2.items():
                assert same_values(got["edge_chi2_lines"][b, s], v)
            assert np.isnan(got["edge_chi2"][b]).sum() == P["valid"].shape[1] - len(chi2)


@pytest.mark.parametrize("model,setup", COMBOS)
def test_whole_runs_equal_the_restatement_on_the_census_scenes(model, setup):
    run_both(S.pack(S.census_frames(model, setup), holes=0.25, seed=8))


@pytest.mark.parametrize("T,I", [(1, 1), (1, 10), (2, 3), (3, 10)])
def test_whole_runs_equal_the_restatement_for_other_trial_and_iteration_counts(T, I):
    frames = [S.make_frame(60 + i, 30, setup=S.RGBD, n_lines=5, noise=1.0, outlier_share=0.25, rot=0.08, trans=0.2) for i in range(2)]
    run_both(S.pack(frames, holes=0.2, seed=6), T, I)


# ---- item 2: the analytic Jacobian of the point edges
def test_point_jacobian_against_central_differences_of_the_restated_error():
    """central differences (h = 1e-6) of point_error through oplus.  Measured with the restatement on these frames: the largest
    |numeric - analytic| / max(1, |analytic|) is 9.14e-8; the bound is ten times that."""
    worst = 0.0
    for seed in range(6):
        P = S.pack([S.make_frame(seed, 12, setup=seed % 3)])
        F = S.ref_frames(P)[0]
        est = REF.est_from_pose(F.pose12)
        for p in F.points:
            mono = p["x_right"] < 0
            args = (F.cam, p["pos_w"], p["x"], p["y"], p["x_right"], mono, 1.0)
            J = REF.point_jacobian(F.cam, REF.point_error(est, *args)[1])
            for d in range(6):
                u = [0.0] * 6
                u[d] = 1e-6
                ep = REF.point_error(REF.oplus(u, est), *args)[2]
                u[d] = -1e-6
                em = REF.point_error(REF.oplus(u, est), *args)[2]
                for r in range(2 if mono else 3):
                    worst = max(worst, abs((ep[r] - em[r]) / 2e-6 - J[6 * r + d]) / max(1.0, abs(J[6 * r + d])))
    print(f"jacobian: worst relative difference {worst:.3e}")
    assert worst <= 9.2e-7


# ---- anchors that do not depend on the definition
@pytest.mark.parametrize("model,setup", COMBOS)
def test_noise_free_scenes_return_the_ground_truth_pose(model, setup):
    """no noise, no outliers: rot_cw and trans_cw of the ground truth.  Measured over these scenes: 1.09e-7 (the key points are floats: 3e-5 px);
    the bound is ten times that (D15)."""
    for nl in (0, 8):
        frames = [S.make_frame(900 + i, 40 + 10 * i, model=model, setup=setup, n_lines=nl) for i in range(4)]
        P = S.pack(frames, holes=0.2, seed=3)
        r = plp.model_pose_optimize(**S.call_args(P))
        for b, f in enumerate(frames):
            assert np.abs(r["pose"][b][:12] - np.concatenate([f["R"].reshape(9), f["t"]])).max() <= 1.1e-6
            assert r["outlier"][b].sum() == 0 and r["num_valid"][b] == len(f["x"]) and r["outlier_lines"][b].sum() == 0
            assert same_values(r["pose"][b], plp.frame_pose(r["pose"][b][:9], r["pose"][b][9:12]))      # cam_center as frame_pose forms it


@pytest.mark.parametrize("model,setup", COMBOS)
def test_gross_outliers_are_flagged_exactly_as_generated(model, setup):
    for nl in (0, 8):
        frames = [S.make_frame(950 + i, 60, model=model, setup=setup, n_lines=nl, outlier_share=0.2) for i in range(4)]
        P = S.pack(frames, holes=0.2, seed=3)
        r = plp.model_pose_optimize(**S.call_args(P))
        for b, f in enumerate(frames):
            assert (r["outlier"][b][P["slot"][b]] == f["label"]).all()
            assert r["num_valid"][b] == P["valid"][b, :P["counts"][b]].sum() - r["outlier"][b][P["slot"][b]].sum()
            if nl:
                assert (r["outlier_lines"][b][P["line_slot"][b]] == f["l_label"]).all()


# ---- the census
def test_census_of_the_cases_the_scenes_reach():
    seen = set()
    stale = 0
    frames_run = 0
    for model, setup in COMBOS:
        frames = S.census_frames(model, setup)
        P = S.pack(frames, holes=0.25, seed=8)
        got, ref = run_both(P)
        for b, q in enumerate(ref):
            frames_run += 1
            stale += 1 if q["stale_differs"] else 0
            ti = q["trial_info"]
            ran = sum(1 for t in ti if t[3])
            n_lines = S.n_lines_of(frames[b])
            for t in ti:
                if t[0] >= 2 and t[1] >= 1 and math.isfinite(q["trial_chi2"][ti.index(t)][0]):
                    seen.add("accepted and rejected steps in one trial")     # an iteration that does not end the trial ended with a kept step
                if t[3] == REF.END_TRIES:
                    seen.add("ten tries")
            if q["status"] == 1 and q["num_init_obs"] == 4:
                seen.add("too few with 4")
                assert (got["outlier_lines"][b] == 0xA5).all()                # no line slot is touched (:161-165)
            if q["status"] == 0 and q["num_init_obs"] == 5:
                seen.add("ok with 5")
            if q["status"] == 0 and ran == 1:
                seen.add("break in trial 0")
            if q["status"] == 0 and ran == 3:
                seen.add("break in trial 2")
            if q["status"] == 0 and ran < 4 and n_lines:
                seen.add("break that skips the line loop")
                # the flags of the lines are those of the trial before: all clear when the break came in trial 0
                if ran == 1:
                    assert (got["outlier_lines"][b][P["line_slot"][b]] == 0).all()
            xr = P["x_right"][b][P["slot"][b]]
            if setup == S.RGBD and q["status"] == 0 and (xr < 0).any() and (xr >= 0).any():
                seen.add("2-D and 3-D edges in one RGB-D frame")
            if q["num_init_obs"] < len(P["slot"][b]):
                seen.add("octave outside the table")
                bad = [s for s in P["slot"][b] if not 0 <= P["undist"]["octave"][b, s] < S.NUM_LEVELS]
                assert len(bad) == 2 and (got["outlier"][b][bad] == 0xA5).all()     # no observation: the flag is left alone
            if any(not math.isfinite(c[0]) for c in q["trial_chi2"]):
                seen.add("non-finite chi2")
    # a Cholesky that fails: the non-finite system of the z_c == 0 frame, and a system without information (H = 0, lambda = 0)
    Pz = S.pack([S.z0_frame()])
    a = S.call_args(Pz)
    lin = plp.model_pose_linearize(**a)
    assert not np.isfinite(lin["H"]).all()
    assert not plp.model_chol6(lin["H"], lin["b"], [1e-5])[1][0]
    seen.add("failed Cholesky")
    a0 = dict(S.call_args(S.pack([S.make_frame(3, 12)])), inv_level_sigma_sq=np.zeros(S.NUM_LEVELS, np.float32))
    r0 = plp.model_pose_optimize(**a0)
    assert r0["trial_info"][0].tolist() == [[1, 10, 0, REF.END_TRIES]] * 4 and (r0["trial_chi2"][0] == 0).all()     # every solve fails: lambda stays 0
    # all landmarks at one point: H has rank 2, but lambda = 1e-5 max diag(H) keeps every pivot of H + lambda I positive -- no solve fails (D15 item 4)
    P1 = S.pack([S.one_point_frame()])
    lin1 = plp.model_pose_linearize(**S.call_args(P1))
    assert np.linalg.matrix_rank(np.array([[lin1["H"][0][REF.h_index(min(i, j), max(i, j))] for j in range(6)] for i in range(6)]), tol=1e-6 * lin1["H"][0].max()) == 2
    assert plp.model_chol6(lin1["H"], lin1["b"], [1e-5 * max(lin1["H"][0][REF.h_index(j, j)] for j in range(6))])[1][0]
    print(f"census: {sorted(seen)}; frames where a fresh evaluation would flag differently: {stale} of {frames_run}")
    want = {"accepted and rejected steps in one trial", "ten tries", "too few with 4", "ok with 5", "break in trial 0", "break in trial 2",
            "break that skips the line loop", "2-D and 3-D edges in one RGB-D frame", "octave outside the table", "non-finite chi2", "failed Cholesky"}
    assert want <= seen, want - seen


def test_no_lines_equals_every_line_invalid():
    frames = [S.make_frame(70 + i, 30, setup=S.STEREO, n_lines=6, noise=1.0, outlier_share=0.2) for i in range(3)]
    P = S.pack(frames, holes=0.2, seed=7)
    P["lines"]["valid"][:] = 0
    with_l = plp.model_pose_optimize(out=sentinels(P, 4), **S.call_args(P))
    P0 = dict(P, lines=None)
    without = plp.model_pose_optimize(out=sentinels(P0, 4), **S.call_args(P0))
    for k in without:
        if k != "outlier_lines":
            assert same_values(with_l[k].astype(np.float64), without[k].astype(np.float64)), k
    assert (with_l["outlier_lines"] == 0xA5).all()


def test_the_mirror_class():
    f = S.make_frame(80, 50, setup=S.RGBD, n_lines=6, noise=0.5, outlier_share=0.1)
    P = S.pack([f])
    opt = plp.pose_optimizer()
    T = np.eye(4); T[:3, :3] = f["pose_start"][:9].reshape(3, 3); T[:3, 3] = f["pose_start"][9:]
    ln = P["lines"]
    n, r = opt.optimize(P["camera"], S.RGBD, T, P["valid"][0], P["undist"][0], P["pos_w"][0], S.INV_SIGMA_SQ, x_right=P["x_right"][0],
                        lines=dict(valid=ln["valid"][0], keylines=ln["keylines"][0], pos_w=ln["pos_w"][0], inv_level_sigma_sq_lsd=S.INV_SIGMA_SQ_LSD))
    want = plp.model_pose_optimize(**S.call_args(P))
    assert n == want["num_valid"][0] and same_values(r["pose"], want["pose"][0]) and (r["outlier"] == want["outlier"][0]).all()
    assert np.allclose(r["cam_pose_cw"][:3, :3] @ r["cam_pose_cw"][:3, :3].T, np.eye(3), atol=1e-14)


# ---- the argument checks
def test_argument_checks_come_before_any_write():
    P = S.pack([S.make_frame(90, 20, n_lines=3)])
    base = S.call_args(P)

    def refused(status, **change):
        out = sentinels(P, 4)
        with pytest.raises(plp.PlpError) as e:
            plp.model_pose_optimize(out=out, **dict(base, **change))
        assert e.value.status == status, change
        for k, v in out.items():
            assert (v == SENT[v.dtype]).all(), (change, k)
    eq = S.camera("perspective"); eq.model = plp.CAMERA_EQUIRECTANGULAR
    refused(plp.PLP_ERR_UNSUPPORTED, camera=eq)
    bad = S.camera("perspective"); bad.model = 7
    refused(plp.PLP_ERR_INVALID_ARG, camera=bad)
    nofx = S.camera("perspective"); nofx.fx = 0.0
    refused(plp.PLP_ERR_INVALID_ARG, camera=nofx)
    refused(plp.PLP_ERR_INVALID_ARG, setup_type=3)
    refused(plp.PLP_ERR_INVALID_ARG, num_trials=0)
    refused(plp.PLP_ERR_INVALID_ARG, num_each_iter=0)
    refused(plp.PLP_ERR_INVALID_ARG, inv_level_sigma_sq=np.zeros(17, np.float32))
    refused(plp.PLP_ERR_INVALID_ARG, lines=dict(P["lines"], inv_level_sigma_sq_lsd=np.zeros(0, np.float32)))
    big = S.pack([S.make_frame(91, 6)], n_cap=8193)
    with pytest.raises(plp.PlpError) as e:
        plp.model_pose_optimize(**S.call_args(big))
    assert e.value.status == plp.PLP_ERR_UNSUPPORTED
    empty = {k: (v[:0] if k in ("pose_in", "valid", "undist", "pos_w", "x_right", "counts") else v) for k, v in dict(base, lines=None).items()}
    r = plp.model_pose_optimize(**empty)                           # B == 0: nothing to do, nothing written
    assert r["status"].shape == (0,) and r["pose"].shape == (0, 15) and r["outlier"].shape == (0, P["valid"].shape[1])
    for name in ("plp_pose_optimize_device", "plp_pose_optimize_host", "plp_model_pose_optimize_host", "plp_model_pose_linearize_host",
                 "plp_model_se3_exp_host", "plp_model_chol6_host", "plp_model_pose_sincos_host"):
        assert name in plp.api_symbols()
