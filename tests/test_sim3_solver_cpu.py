"""solve::sim3_solver without a GPU: the CPU builds of csrc/sim3.hpp (plp.model_sym_eig4_max, model_horn_sim3, model_sim3_ransac,
model_sim3_draw) against the plain-Python restatement tests/sim3_solver_ref.py, bit for bit, on the scenes of tests/sim3_solver_scene.py
(DESIGN.md section 5, D13); the Jacobi against numpy.linalg.eigh; the sample generator; the argument checks of include/plp_front.h."""
import ctypes as C
import itertools
import math

import numpy as np
import pytest

import sim3_solver_ref as R
import sim3_solver_scene as S
from plp import plp

# Figures measured where this file was written, over every hypothesis of SCENES (3 600 matrices); each bound leaves 16 x for another libm / LAPACK.
MEASURED_MAX_SWEEPS = 5                       # sweeps that rotated; the limit is 30
MEASURED_MAX_EIG_RESIDUAL = 8.07e-16          # |N v - lambda_max v|_2 / |N|_F, lambda_max from numpy.linalg.eigh (OpenBLAS LAPACK)
MEASURED_MAX_UNIT_ERROR = 1.0e-15             # | |v|_2 - 1 |
# 400 noise-free triples against the Sim3 that made them: max |rot_21 - R| and |scale_21 - s| (the scale is a float: 2^-24 relative), and
# |trans_21 - t|, which carries the float scale times a centroid of up to 9 m
MEASURED_MAX_NOISE_FREE_ROT = 7.83e-15
MEASURED_MAX_NOISE_FREE_TRANS = 4.19e-7
MEASURED_MAX_NOISE_FREE_SCALE = 5.85e-8
MEASURED_MAX_EIGH_POSE_DIFF = 1.39e-15        # best rot_12 / trans_12 of every scene, Jacobi vs eigh
EIG_C = 16 * MEASURED_MAX_EIG_RESIDUAL
GATE_GAP = 1e-9                               # the relative gap every dependent comparison keeps (D8 item 3)
MIN_EIG_GAP = 1e-6

SCENES = [(1000 + 10 * i + int(fix), n, n + n // 3, out, fix) for i, (n, out) in enumerate(((24, 0.3), (60, 0.4), (300, 0.5))) for fix in (False, True)]
MIN_INL = 10                                  # 24 points with 30 % outliers cannot reach the loop detector's 20


def scene(i):
    seed, n, slots, out, fix = SCENES[i]
    return S.problem(seed, n, slots, out, fix), fix


def lib_run(name, probs, fix, min_inl=20, seed=None, n_cap=None, **kw):
    a = S.pack(probs, n_cap)
    samples = dict(seed=seed) if seed is not None else dict(samples=a["samples"])
    return plp.model_sim3_ransac(plp.camera_model(S.CAMERAS[name]), a["valid"], a["pos_w_1"], a["pos_w_2"], a["octave_1"], a["octave_2"], a["pose_1"],
                                 a["pose_2"], S.SIGMA_SQ, S.SIGMA_SQ, iters=probs[0]["iters"], fix_scale=fix, min_num_inliers=min_inl, counts=a["counts"],
                                 **samples, **kw)


def bits(a):
    return np.ascontiguousarray(a).tobytes()


def assert_problem(got, p, want, label):
    for k, w in want.items():
        g = np.asarray(got[k][p])
        if k == "inliers":
            g = g[:len(w)]
        assert g.dtype == np.asarray(w).dtype and bits(g) == bits(w), (label, k, g, w)


_HYP = {}


def hypotheses():
    """every hypothesis of every scene, once: list of dict(N, pts_1, pts_2, fix, truth)"""
    if not _HYP:
        out = []
        for i in range(len(SCENES)):
            q, fix = scene(i)
            s = R.Sim3Solver(S.ref_camera("perspective"), q["valid"], q["pos_w_1"], q["pos_w_2"], q["octave_1"], q["octave_2"], q["pose_1"], q["pose_2"],
                             q["sigma_sq_1"], q["sigma_sq_2"], fix, 20)
            for idx in q["samples"]:
                pts_1 = [[s.x1[idx[c]][r] for c in range(3)] for r in range(3)]
                pts_2 = [[s.x2[idx[c]][r] for c in range(3)] for r in range(3)]
                out.append(dict(N=R.horn_matrix(pts_1, pts_2)[0], pts_1=pts_1, pts_2=pts_2, fix=fix))
        _HYP["all"] = out
    return _HYP["all"]


# ---------------------------------------------------------------------------------------------------------------- model_sym_eig4_max
def special_matrices():
    rng = np.random.default_rng(3)
    rnd = rng.standard_normal((300, 4, 4))
    rnd = rnd + rnd.transpose(0, 2, 1)
    u = rng.standard_normal(4)
    q, _ = np.linalg.qr(rng.standard_normal((4, 4)))
    two_equal = q @ np.diag([2.0, 2.0, -1.0, 0.5]) @ q.T
    nan = rnd[0].copy()
    nan[1, 2] = nan[2, 1] = np.nan
    return list(rnd) + [rnd[1] * 1e150, rnd[2] * 1e-150, rnd[3] * 1e160, np.zeros((4, 4)), np.eye(4), np.outer(u, u), -np.outer(u, u), two_equal,
                        0.5 * (two_equal + two_equal.T), np.diag([1.0, 3.0, 3.0, 2.0]), nan, np.full((4, 4), np.inf)]


def test_eigenvector_equals_the_python_jacobi_bit_for_bit():
    mats = [np.array(h["N"]) for h in hypotheses()] + special_matrices()
    v, sw = plp.model_sym_eig4_max(np.array(mats))
    for i, m in enumerate(mats):
        wv, ws, _ = R.sym_eig4_max(m.tolist())
        assert bits(v[i]) == bits(np.array(wv)) and int(sw[i]) == ws, (i, m, v[i], wv, sw[i], ws)
    n_scene = len(hypotheses())
    print("max sweeps on scene matrices:", int(sw[:n_scene].max()))
    assert int(sw[:n_scene].max()) <= MEASURED_MAX_SWEEPS < R.SWEEP_LIMIT


def test_ties_between_eigenvalues_go_to_the_lowest_column():
    v, sw = plp.model_sym_eig4_max(np.array([np.eye(4), np.zeros((4, 4)), np.diag([1.0, 3.0, 3.0, 2.0]), np.diag([-1.0, -1.0, -1.0, -1.0])]))
    assert np.array_equal(v, [[1, 0, 0, 0], [1, 0, 0, 0], [0, 1, 0, 0], [1, 0, 0, 0]]) and not sw.any()


def test_eigenvector_against_eigh():
    mats = np.array([h["N"] for h in hypotheses()])
    v, _ = plp.model_sym_eig4_max(mats)
    res = unit = 0.0
    for m, x in zip(mats, v):
        lam = np.linalg.eigh(m)[0][3]
        res = max(res, np.linalg.norm(m @ x - lam * x) / np.linalg.norm(m))
        unit = max(unit, abs(np.linalg.norm(x) - 1.0))
    print("max residual / |N|:", res, "max | |v| - 1 |:", unit)
    assert res <= EIG_C and unit <= 16 * MEASURED_MAX_UNIT_ERROR


# ---------------------------------------------------------------------------------------------------------------- model_horn_sim3
def test_horn_equals_the_restatement_bit_for_bit():
    hyp = hypotheses()
    for fix in (False, True):
        sel = [h for h in hyp if h["fix"] == fix][::3]
        got = plp.model_horn_sim3(np.array([h["pts_1"] for h in sel]), np.array([h["pts_2"] for h in sel]), fix)
        for i, h in enumerate(sel):
            want = R.horn_sim3(h["pts_1"], h["pts_2"], fix)
            for k in ("rot_12", "trans_12", "rot_21", "trans_21"):
                assert bits(got[k][i]) == bits(np.array(want[k], np.float64)), (fix, i, k)
            for k in ("scale_12", "scale_21"):
                assert bits(got[k][i]) == bits(np.float32(want[k])), (fix, i, k)
        if fix:
            assert (got["scale_21"] == np.float32(1.0)).all() and (got["scale_12"] == np.float32(1.0)).all()


def test_horn_recovers_a_known_sim3_from_noise_free_triples():
    rng = np.random.default_rng(8)
    worst = dict(rot=0.0, trans=0.0, scale=0.0)
    for fix in (False, True):
        for _ in range(200):
            s = 1.0 if fix else rng.uniform(0.8, 1.25)
            Rm, t = S.rotation(rng, 0.5), rng.uniform(-0.5, 0.5, 3)
            x1 = np.stack([rng.uniform(-3, 3, 3), rng.uniform(-2, 2, 3), rng.uniform(3.0, 9.0, 3)])        # columns are the samples
            x2 = s * Rm @ x1 + t[:, None]
            g = plp.model_horn_sim3(x1, x2, fix)
            worst["rot"] = max(worst["rot"], np.abs(g["rot_21"] - Rm).max())
            worst["trans"] = max(worst["trans"], np.abs(g["trans_21"] - t).max())
            worst["scale"] = max(worst["scale"], abs(float(g["scale_21"]) - s))
            assert np.abs(g["rot_12"] - g["rot_21"].T).max() == 0.0
    print("noise-free recovery, worst:", worst)
    assert worst["rot"] <= 16 * MEASURED_MAX_NOISE_FREE_ROT and worst["trans"] <= 16 * MEASURED_MAX_NOISE_FREE_TRANS
    assert worst["scale"] <= 16 * MEASURED_MAX_NOISE_FREE_SCALE


# ---------------------------------------------------------------------------------------------------------------- model_sim3_ransac
@pytest.mark.parametrize("name", sorted(S.CAMERAS))
@pytest.mark.parametrize("i", range(len(SCENES)))
def test_ransac_equals_the_restatement(name, i):
    q, fix = scene(i)
    got = lib_run(name, [q], fix, min_inl=MIN_INL)
    want, s = R.run_problem(S.ref_camera(name), q, q["samples"], fix, MIN_INL)
    assert_problem(got, 0, want, (name, i))
    assert int(want["status"]) == R.OK and int(want["num_inliers"]) >= MIN_INL
    tied = np.flatnonzero(want["hyp_inliers"] == want["num_inliers"])
    assert int(want["best_iter"]) == tied[0]
    TIED[(name, i)] = len(tied)
    if name == "perspective":                                   # the best hypothesis finds the scene's Sim3: most of the true inliers, no more
        true = int((~q["is_outlier"]).sum())
        assert 0.9 * true <= int(want["num_inliers"]) <= true, (i, int(want["num_inliers"]), true)


TIED = {}


def test_ties_are_exercised_and_go_to_the_first_iteration():
    """at least one scene has two or more hypotheses at the best count (best_iter == the first of them is asserted per scene above)"""
    for i in range(len(SCENES)):
        if ("perspective", i) not in TIED:
            test_ransac_equals_the_restatement("perspective", i)
    print("hypotheses tied at the best count, per scene:", [TIED[("perspective", i)] for i in range(len(SCENES))])
    assert max(TIED[("perspective", i)] for i in range(len(SCENES))) >= 2


@pytest.mark.parametrize("name", sorted(S.CAMERAS))
def test_ragged_problems_statuses_and_the_points_no_camera_reprojects(name):
    probs = [S.problem(20, 2, 7, 0.0), S.problem(21, 3, 5, 0.0), S.problem(22, 19, 30, 0.0), S.problem(23, 40, 50, 0.4, all_outliers=True),
             S.problem(24, 70, 90, 0.3, behind_own=3), S.problem(25, 25, 25, 0.0)]
    behind_other = [0]
    got = lib_run(name, probs, False, n_cap=100)
    ref_cam = S.ref_camera(name)
    for p, q in enumerate(probs):
        want, s = R.run_problem(ref_cam, q, q["samples"], False, 20)
        assert_problem(got, p, want, (name, p))
        assert (got["inliers"][p, len(q["valid"]):] == 0).all()           # zero-initialised by the wrapper, untouched by the library
        if p == 4 and name != "equirectangular":
            assert sum(r is None for r in s.rep1) == 3 and not want["inliers"][np.flatnonzero(q["valid"])[:3]].any()
            for idx in q["samples"]:                                          # some hypothesis puts a point behind the OTHER camera
                H = s.hypothesis([int(v) for v in idx])
                m21 = [[float(H["scale_21"]) * v for v in row] for row in H["rot_21"]]
                behind_other[0] += sum(R.reproject(ref_cam, m21, H["trans_21"], x) is None for x in s.x1)
    assert [int(v) for v in got["status"]] == [R.TOO_FEW_POINTS, R.TOO_FEW_POINTS, R.TOO_FEW_POINTS, R.TOO_FEW_INLIERS, R.OK, R.OK]
    bad = got["status"] != R.OK
    assert (got["best_iter"][bad] == -1).all() and not got["rot_12"][bad].any() and not got["trans_12"][bad].any() and not got["scale_12"][bad].any()
    assert not got["inliers"][bad].any() and not got["hyp_inliers"][:3].any()
    if name != "equirectangular":
        assert behind_other[0] > 0


def test_three_points_and_min_num_inliers_below_them():
    q = S.problem(21, 3, 5, 0.0)
    got = lib_run("perspective", [q], False, min_inl=3)
    want, _ = R.run_problem(S.ref_camera("perspective"), q, q["samples"], False, 3)
    assert_problem(got, 0, want, "n = 3")
    assert int(got["num_common"][0]) == 3 and int(got["status"][0]) in (R.OK, R.TOO_FEW_INLIERS)


def test_bad_samples_and_octaves_outside_the_tables():
    q = S.problem(31, 50, 60, 0.3, iters=40)
    q["samples"][2] = (4, 9, 4)
    q["samples"][5] = (50, 1, 2)
    q["samples"][6] = (3, -1, 2)
    c = np.flatnonzero(q["valid"])
    q["octave_1"][c[7]] = 8
    q["octave_2"][c[8]] = -1
    got = lib_run("perspective", [q], False)
    want, _ = R.run_problem(S.ref_camera("perspective"), q, q["samples"], False, 20)
    assert_problem(got, 0, want, "bad samples")
    assert not got["hyp_inliers"][0, [2, 5, 6]].any() and not got["inliers"][0, c[[7, 8]]].any()


def test_samples_drawn_from_a_seed_are_the_restatements():
    q, fix = scene(2)
    got = lib_run("perspective", [q, q], fix, seed=99)
    for p in range(2):
        want, _ = R.run_problem(S.ref_camera("perspective"), q, None, fix, 20, seed=99, p=p)
        assert_problem(got, p, want, ("seed", p))
    assert bits(got["hyp_inliers"][0]) != bits(got["hyp_inliers"][1])       # the problem index is part of the counter


def test_eigh_in_place_of_the_jacobi():
    worst, min_gap, min_margin = 0.0, math.inf, math.inf
    for i in range(len(SCENES)):
        q, fix = scene(i)
        cam = S.ref_camera("perspective")
        margins, gaps = [], {}
        a, sa = R.run_problem(cam, q, q["samples"], fix, MIN_INL)
        b, _ = R.run_problem(cam, q, q["samples"], fix, MIN_INL, eig=R.eig_eigh)
        for it, idx in enumerate(q["samples"]):
            pts_1 = [[sa.x1[idx[c]][r] for c in range(3)] for r in range(3)]
            pts_2 = [[sa.x2[idx[c]][r] for c in range(3)] for r in range(3)]
            N = np.array(R.horn_matrix(pts_1, pts_2)[0])
            w = np.linalg.eigh(N)[0]
            gaps[it] = (w[3] - w[2]) / np.abs(w).max()
            sa.count_inliers(sa.hypothesis([int(v) for v in idx]), margins)
        min_gap, min_margin = min(min_gap, min(gaps.values())), min(min_margin, min(margins))
        assert int(a["status"]) == int(b["status"]) and int(a["best_iter"]) == int(b["best_iter"])
        assert np.array_equal(a["hyp_inliers"], b["hyp_inliers"])               # every gap is >= MIN_EIG_GAP (asserted below)
        worst = max(worst, np.abs(a["rot_12"] - b["rot_12"]).max(), np.abs(a["trans_12"] - b["trans_12"]).max())
    print("Jacobi vs eigh: max pose difference", worst, "min eigenvalue gap", min_gap, "min threshold margin", min_margin)
    assert min_gap >= MIN_EIG_GAP and min_margin >= GATE_GAP
    assert worst <= 16 * MEASURED_MAX_EIGH_POSE_DIFF < 1e-9


# ---------------------------------------------------------------------------------------------------------------- the generator
def test_generator_is_the_restatements_distinct_in_range_and_deterministic():
    for n in (3, 4, 7, 300, 8192):
        d = plp.model_sim3_draw(12345, 3, 200, n)
        assert np.array_equal(d, np.array([R.draw(12345, 3, it, n) for it in range(200)]))
        assert d.min() >= 0 and d.max() < n
        assert (d[:, 0] != d[:, 1]).all() and (d[:, 0] != d[:, 2]).all() and (d[:, 1] != d[:, 2]).all()
    a = plp.model_sim3_draw(5, 0, 64, 1000)
    assert np.array_equal(a, plp.model_sim3_draw(5, 0, 64, 1000)) and np.array_equal(a[10:20], plp.model_sim3_draw(5, 0, 10, 1000, iter0=10))
    assert not np.array_equal(a, plp.model_sim3_draw(5, 1, 64, 1000)) and not np.array_equal(a, plp.model_sim3_draw(6, 0, 64, 1000))
    assert len({tuple(r) for r in a}) == 64


def test_generator_is_uniform_over_the_triples():
    d = np.sort(plp.model_sim3_draw(2024, 1, 20000, 7), 1)
    counts = {t: 0 for t in itertools.combinations(range(7), 3)}
    for r in d:
        counts[tuple(int(v) for v in r)] += 1
    mean = 20000 / 35
    sd = math.sqrt(20000 * (1 / 35) * (34 / 35))
    assert len(counts) == 35 and min(counts.values()) > 0
    assert max(abs(c - mean) for c in counts.values()) <= 5 * sd, counts
    first = np.bincount(plp.model_sim3_draw(2024, 1, 20000, 7)[:, 0], minlength=7)      # ... and over the first position
    assert np.abs(first - 20000 / 7).max() <= 5 * math.sqrt(20000 * (1 / 7) * (6 / 7))


# ---------------------------------------------------------------------------------------------------------------- the argument checks
def test_every_invalid_argument_line_of_the_header():
    L = plp.lib()
    q = S.problem(1, 30, 40, 0.3, iters=8)
    a = S.pack([q])
    sig = S.SIGMA_SQ
    o = {k: np.zeros((1,) + shape(40, 8), dt) for k, (shape, dt, _) in plp.SIM3_OUTPUTS.items()}
    P = lambda v: v.ctypes.data

    def args(**over):
        s = plp.sim3_ransac_args_c()
        s.camera = plp.camera_model_c.from_buffer_copy(plp.camera_model(S.CAMERAS["perspective"]))
        f = dict(P=1, n_cap=40, fix_scale=0, min_num_inliers=20, iters=8, seed=0, level_sigma_sq_1=P(sig), level_sigma_sq_2=P(sig), num_levels=8,
                 counts=P(a["counts"]), valid=P(a["valid"]), pos_w_1=P(a["pos_w_1"]), pos_w_2=P(a["pos_w_2"]), octave_1=P(a["octave_1"]),
                 octave_2=P(a["octave_2"]), pose_1=P(a["pose_1"]), pose_2=P(a["pose_2"]), samples=P(a["samples"]), out_status=P(o["status"]),
                 out_num_common=P(o["num_common"]), out_rot_12=P(o["rot_12"]), out_trans_12=P(o["trans_12"]), out_scale_12=P(o["scale_12"]),
                 out_num_inliers=P(o["num_inliers"]), out_best_iter=P(o["best_iter"]), out_inliers=P(o["inliers"]), out_hyp_inliers=P(o["hyp_inliers"]))
        f.update(over)
        for k, v in f.items():
            setattr(s, k, v)
        return s
    run = lambda s: L.plp_model_sim3_ransac_host(C.byref(s))
    assert run(args()) == 1 and int(o["status"][0]) == R.OK
    assert L.plp_model_sim3_ransac_host(None) == -1
    bad = [dict(P=-1), dict(n_cap=-1), dict(iters=0), dict(min_num_inliers=-1), dict(num_levels=0), dict(num_levels=17), dict(level_sigma_sq_1=None),
           dict(level_sigma_sq_2=None), dict(n_cap=8193), dict(P=65536)]
    bad += [{k: None} for k in ("valid", "pos_w_1", "pos_w_2", "octave_1", "octave_2", "pose_1", "pose_2", "out_status", "out_num_common", "out_rot_12",
                                "out_trans_12", "out_scale_12", "out_num_inliers", "out_best_iter")]
    before = {k: v.copy() for k, v in o.items()}
    for over in bad:
        assert run(args(**over)) == -1, over
    for cam_over in (dict(model=3), dict(fx=0.0), dict(fy=0.0)):
        s = args()
        for k, v in cam_over.items():
            setattr(s.camera, k, v)
        assert run(s) == -1, cam_over
    s = args()
    s.camera = plp.camera_model_c.from_buffer_copy(plp.camera_model(S.CAMERAS["equirectangular"]))
    s.camera.cols = 0
    assert run(s) == -1
    assert all(np.array_equal(o[k], before[k]) for k in o), "a rejected call wrote an output"
    # nothing to do: PLP_OK, nothing written; the optional outputs and counts may be NULL
    assert run(args(P=0)) == 0 and run(args(n_cap=0)) == 1 and all(np.array_equal(o[k], before[k]) for k in o)
    assert run(args(out_inliers=None, out_hyp_inliers=None, counts=None, samples=None)) == 1
    # the other host builds
    assert L.plp_model_sym_eig4_max_host(None, 1, None, None) == -1 and L.plp_model_sym_eig4_max_host(None, 0, None, None) == 0
    assert L.plp_model_horn_sim3_host(None, None, 1, 0, None, None, None, None, None, None, None) == -1
    assert L.plp_model_sim3_draw_host(1, 0, 0, 4, 2, None) == -1 and L.plp_model_sim3_draw_host(1, 0, 0, 4, 3, None) == -1


def test_the_mirror_class_has_the_references_surface():
    q, fix = scene(2)
    cam = plp.camera_model(S.CAMERAS["perspective"])
    s = plp.sim3_solver(cam, q["valid"], q["pos_w_1"], q["pos_w_2"], q["octave_1"], q["octave_2"], q["pose_1"], q["pose_2"], S.SIGMA_SQ, S.SIGMA_SQ,
                        fix_scale=fix, min_num_inliers=20, samples=q["samples"])
    assert not s.solution_is_valid()
    s.find_via_ransac(200)
    want, _ = R.run_problem(S.ref_camera("perspective"), q, q["samples"], fix, 20)
    assert s.solution_is_valid() and bits(s.get_best_rotation_12()) == bits(want["rot_12"]) and bits(s.get_best_translation_12()) == bits(want["trans_12"])
    assert np.float32(s.get_best_scale_12()) == want["scale_12"] and np.array_equal(s.get_inliers(), want["inliers"].astype(bool))
    # X1 = s_12 R_12 X2 + t_12 against the scene's X2 = s R X1 + t
    sc, Rm, t = q["truth"]
    assert np.abs(s.get_best_rotation_12() - Rm.T).max() < 2e-2 and abs(s.get_best_scale_12() * sc - 1.0) < 2e-2
