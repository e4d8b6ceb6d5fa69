"""Planar_Mapping_module's RANSAC and refine_points, host build (csrc/plane_fit.hpp) against the restatement of DESIGN.md section 5, D19
(tests/plane_ransac_ref.py), no GPU: bit for bit on every output, a census of the branches the scenes reach, anchors against numpy's LAPACK
that do not depend on the definition, the generating labels on the margin scenes, and the argument checks."""
import ctypes as C
import functools

import numpy as np
import pytest

import plane_ransac_ref as PR
import plane_ransac_scene as PS
from plp import plp

SCENES = PS.scenes()
NAMES = sorted(SCENES)


@functools.lru_cache(maxsize=None)
def ref(name):
    """the restatement's result of a scene, and the point list of every fit it made (computed once, shared, never changed)"""
    record = []
    return PS.run_ref(SCENES[name][0], record=record), record


def same(got, want):
    return np.array_equal(got, want, equal_nan=np.asarray(want).dtype.kind == "f")


def run_model(problems, mode_fn=None, n_cap=None):
    a = PS.pack(problems, n_cap)
    q = problems[0]
    P, M = a["flags"].shape
    out = {k: np.full((P,) + shape(M, q["iters"]), PR.SENTINEL[k], dt) for k, (shape, dt, _) in plp.PLANE_RANSAC_OUTPUTS.items()}
    fn = mode_fn or plp.model_plane_ransac
    return fn(q["mode"], a["pos_w"], a["flags"], a["dist_thresh"], a["error_thresh"], out=out, **PS.call_kwargs(problems, a)), M


# ---------------------------------------------------------------------------------------------------------------- bit for bit
@pytest.mark.parametrize("name", NAMES)
def test_host_build_equals_the_restatement_bit_for_bit(name):
    q = SCENES[name][0]
    got, M = run_model([q])
    want = PR.expected([ref(name)[0]], M, q["iters"])
    assert set(want) == set(plp.PLANE_RANSAC_OUTPUTS)
    for k in want:
        assert same(got[k], want[k]), (name, k, got[k], want[k])


@pytest.mark.parametrize("mode", [PR.CREATE, PR.UPDATE])
def test_ragged_problems_of_one_call_drawn_samples(mode):
    """problem p draws with its own index; rows of count 0 between full ones; slots above a count keep the caller's values"""
    qs = [PS.problem(40 + i, n, mode=mode, outliers=0.05, erased=e, unowned=u, iters=6) for i, (n, e, u) in
          enumerate([(70, 3, 2), (0, 0, 0), (130, 0, 5), (17, 0, 0), (64, 64, 0), (65, 1, 1)])]
    for q in qs:
        q["seed"] = 40                                  # one seed per call
    got, M = run_model(qs, n_cap=140)
    want = PR.expected([PS.run_ref(q, p=p) for p, q in enumerate(qs)], M, 6)
    for k in want:
        assert same(got[k], want[k]), (k, got[k], want[k])
    assert [int(want["status"][p]) for p in (1, 3, 4)] == [PR.TOO_FEW_POINTS, PR.TOO_FEW_POINTS, PR.NO_ELIGIBLE]
    if mode == PR.CREATE:
        assert PR.OK in [int(want["status"][p]) for p in (0, 2, 5)]
    assert (got["inliers"][1] == PR.SENTINEL["inliers"]).all() and (got["inliers"][0, 70:] == PR.SENTINEL["inliers"]).all()


def test_fit_and_draw_equal_the_restatement():
    lists, pts = [], []
    for name in NAMES:
        for X in ref(name)[1][:6]:
            lists.append(np.arange(len(X)) + sum(len(p) for p in pts))
            pts.append(X)
    eq, res, sw = plp.model_plane_fit(np.concatenate(pts), lists)
    assert len(lists) > 40
    for l, X in enumerate(pts):
        w_eq, w_res, w_sw = PR.fit(X)
        assert same(eq[l], np.array(w_eq)) and same(res[l], np.float64(w_res)) and sw[l] == w_sw
    # one point, the same point many times, an index outside the table, an empty list
    one = np.array([[1.5, -2.0, 0.25]])
    eq, res, _ = plp.model_plane_fit(one, [[0], [0] * 70, [0, 1], []])
    for l in (0, 1):
        w_eq, w_res, _ = PR.fit(one[[0] * (1 if l == 0 else 70)])
        assert same(eq[l], np.array(w_eq)) and same(res[l], np.float64(w_res))
    assert (eq[2:] == 0.0).all() and (res[2:] == PR.DBL_MAX).all()
    for seed, p, it0, m, n_el in [(0, 0, 0, 18, 1), (7, 3, 5, 18, 200), (2 ** 64 - 1, 65534, 1000, 100, 8192), (99, 1, 0, 6554, 8192)]:
        got = plp.model_plane_draw(seed, p, 4, m, n_el, iter0=it0)
        want = np.array([[PR.draw(seed, p, it0 + i, k, n_el) for k in range(m)] for i in range(4)], np.int32)
        assert np.array_equal(got, want) and got.min() >= 0 and got.max() < n_el
    counts = np.bincount(plp.model_plane_draw(5, 0, 2000, 18, 9).ravel(), minlength=9)      # uniform over the ranks: 5 sigma of a binomial
    assert np.abs(counts - 4000).max() <= 5 * np.sqrt(36000 * (1 / 9) * (8 / 9))
    for n in range(0, 200):
        assert plp.plane_sample_size(PR.UPDATE, n, 18) == PR.sample_size(PR.UPDATE, n, 18)


def test_refine_points_equals_the_restatement():
    for M in (1, 64, 65, 300):
        sc = PS.refine_scene(M, M)
        want_pos, want_ch = PR.refine_points(**sc)
        got_pos, got_ch = plp.model_plane_refine_points(**sc)
        assert same(got_pos, want_pos) and np.array_equal(got_ch, want_ch)
    sc = PS.refine_scene(7, 400)
    pos, ch = PR.refine_points(**sc)
    eq = sc["equation"][np.clip(sc["lm_plane"], 0, 4)]
    side = (eq[:, :3] * sc["pos_w"]).sum(1) + eq[:, 3]
    live = (sc["lm_plane"] >= 0) & (sc["lm_plane"] < 5) & (sc["lm_plane"] != 1) & (sc["flags"] == PR.LM_OWNED)
    assert ch[live & (side > 0.01 * PS.DIST_THRESH) & (side < 0.5 * PS.DIST_THRESH)].all(), "a point just above its plane moves onto it"
    assert not ch[side < 0].any(), "dist_old is a fabs: a point on the negative side moves away and is rejected (:986)"
    assert not ch[~live].any() and same(pos[ch == 0], sc["pos_w"][ch == 0])
    on = live & (sc["lm_plane"] == 0) & (sc["pos_w"][:, 2] == 2.0)
    assert on.sum() > 3 and not ch[on].any(), "dist_old == 0 (:977)"


# ---------------------------------------------------------------------------------------------------------------- the branches
def test_branch_census():
    reached = set()
    for name in NAMES:
        q, (r, _) = SCENES[name][0], ref(name)
        t, n, U = r["trace"], len(q["flags"]), q["mode"] == PR.UPDATE
        if t["gate"]:
            reached.add("gate")                                                   # :359
        elif r["status"] == PR.TOO_FEW_POINTS:
            reached.add("u_invalid_few" if U else "too_few")                      # :428, :602
            assert r["flags"] == (PR.FLAG_INVALID if U else 0)
        if r["status"] == PR.NO_ELIGIBLE:
            reached.add("no_eligible")
        if not U and t["broke_at"] == 0:
            reached.add("break_0")
        if not U and t["broke_at"] is not None and 0 < t["broke_at"] < q["iters"] - 1:
            reached.add("break_mid")
            assert r["last_iter"] == t["broke_at"] == r["best_iter"]
        if not U and t["ran"] == q["iters"] and t["broke_at"] is None:
            reached.add("no_break")
        if t["ran"] and not t["accepted"]:
            reached.add("never")
            assert r["status"] == PR.NOT_FOUND
        if t["accepted"] and r["status"] == PR.ERROR_ABOVE_THRESHOLD:
            reached.add("u_above" if U else "above")
        if U and r["status"] == PR.TOO_FEW_LEFT:
            reached.add("u_too_few_left")
            assert r["flags"] == PR.FLAG_INVALID
        if U and r["flags"] == PR.FLAG_NEED_REFINEMENT:
            reached.add("u_need_refinement")
        if t["ran"] and r["best_iter"] >= 0 and r["best_iter"] != r["last_iter"]:
            reached.add("best_not_last")
            # the outputs follow the LAST iteration: its sample fit, not the accepted refit of best_iter
            assert r["best_error"] == r["hyp_residual"][r["last_iter"]] and r["best_error"] != r["hyp_error"][r["best_iter"]]
        if SCENES[name][1] is not None:
            assert SCENES[name][1] in reached, (name, SCENES[name][1], r["status"], t)
    assert reached >= {"gate", "too_few", "no_eligible", "break_0", "break_mid", "no_break", "never", "above", "u_invalid_few", "u_too_few_left",
                       "u_need_refinement", "u_above", "best_not_last"}, reached


# ---------------------------------------------------------------------------------------------------------------- anchors
# Bounds: the restatement alone was run against numpy's LAPACK over the sample fits and refits of all scenes (301 fits; 4 left out, below);
# each bound is ten times the worst value measured, which stands beside it.
ANGLE_BOUND = 2.2e-14      # measured 2.15e-15 rad
RESIDUAL_BOUND = 8.5e-13   # measured 8.44e-14, relative
OFFSET_BOUND = 2.6e-14     # measured 2.52e-15, relative to max(1, |d|)


def test_anchors_against_lapack():
    """D19's normal against numpy.linalg.svd(Xc)'s third left singular vector up to sign, the residual against numpy's, and d and the residual
    against their formulas with numpy's normal.  Left out: fits whose two smallest singular values are closer than 1e-6 of the largest (samples
    of one or two distinct points: the normal is not determined); the residual is compared where it is above 1e-9 sigma_1 / sqrt(m) (an exact
    plane through three distinct points has a residual of rounding noise only)."""
    worst = dict(angle=0.0, residual=0.0, offset=0.0, formula=0.0)
    fits = skipped = 0
    for name in NAMES:
        for X in ref(name)[1]:
            eq, res, _ = PR.fit(X)
            m, c = len(X), X.mean(0)
            U, sv, _ = np.linalg.svd((X - c).T)
            if sv[1] - sv[2] < 1e-6 * sv[0]:
                skipped += 1
                continue
            fits += 1
            n, u3 = np.array(eq[:3]), U[:, 2]
            worst["angle"] = max(worst["angle"], float(np.arcsin(min(1.0, np.linalg.norm(np.cross(n, u3))))))
            assert abs(np.linalg.norm(n) - 1.0) < 4e-16 and n[np.argmax(np.abs(n))] > 0
            if np.dot(n, u3) < 0:
                u3 = -u3
            d_np = -float(u3 @ c)
            worst["offset"] = max(worst["offset"], abs(eq[3] - d_np) / max(1.0, abs(d_np)))
            res_np = abs(np.linalg.norm(X @ u3 + d_np) / m)
            if res_np > 1e-9 * sv[0] / np.sqrt(m):
                worst["residual"] = max(worst["residual"], abs(res - res_np) / res_np)
                formula = abs(np.linalg.norm(X @ u3 + eq[3]) / m)
                worst["formula"] = max(worst["formula"], abs(res - formula) / formula)
    print("anchors:", worst, fits, "fits,", skipped, "left out")
    assert fits >= 290 and skipped <= 6
    assert worst["angle"] <= ANGLE_BOUND and worst["residual"] <= RESIDUAL_BOUND and worst["formula"] <= RESIDUAL_BOUND and worst["offset"] <= OFFSET_BOUND, worst


# The margin scenes: noise at most a quarter of dist_thresh, outliers at least four thresholds off.  None had to be left out: on every margin
# scene whose restatement ends PLP_PLANE_OK the membership equals the generating labels (checked with the restatement alone).
MARGIN_LEFT_OUT = []


def test_inliers_equal_the_generating_labels_on_the_margin_scenes():
    checked = 0
    for name in NAMES:
        q, (r, _) = SCENES[name][0], ref(name)
        if not q["margin"] or r["status"] != PR.OK or name in MARGIN_LEFT_OUT:
            continue
        got, _ = run_model([q])
        assert np.array_equal(r["inliers"], q["labels"]) and np.array_equal(got["inliers"][0, :len(q["labels"])], q["labels"]), name
        assert got["num_inliers"][0] == q["labels"].sum()
        checked += 1
    assert checked >= 7 and len(MARGIN_LEFT_OUT) * 10 <= len(NAMES)


# ---------------------------------------------------------------------------------------------------------------- the argument checks
def test_every_invalid_argument_line_of_the_header():
    L = plp.lib()
    q = PS.problem(4, 120, mode=PR.UPDATE, outliers=0.1, plan="cccccccc")
    a = PS.pack([q])
    o = {k: np.full((1,) + shape(120, 8), PR.SENTINEL[k], dt) for k, (shape, dt, _) in plp.PLANE_RANSAC_OUTPUTS.items()}
    P = lambda v: v.ctypes.data

    def args(**over):
        s = plp.plane_ransac_args_c()
        f = dict(mode=PR.UPDATE, P=1, n_cap=120, points_per_ransac=18, min_points_before_ransac=12, iters=8, inliers_ratio_thr=0.7, seed=0,
                 m_cap=a["samples"].shape[2], counts=P(a["counts"]), pos_w=P(a["pos_w"]), flags=P(a["flags"]), dist_thresh=P(a["dist_thresh"]),
                 error_thresh=P(a["error_thresh"]), best_error_in=P(a["best_error_in"]), equation_in=P(a["equation_in"]), samples=P(a["samples"]),
                 **{"out_" + k: P(v) for k, v in o.items()})
        f.update(over)
        for k, v in f.items():
            setattr(s, k, v)
        return s
    run = lambda s: L.plp_model_plane_ransac_host(C.byref(s))
    before = {k: v.copy() for k, v in o.items()}
    assert L.plp_model_plane_ransac_host(None) == -1
    bad = [dict(mode=2), dict(mode=-1), dict(P=-1), dict(n_cap=-1), dict(iters=0), dict(points_per_ransac=0), dict(min_points_before_ransac=-1),
           dict(n_cap=8193), dict(P=65536), dict(iters=1025), dict(m_cap=95), dict(mode=PR.CREATE, m_cap=17)]
    bad += [{k: None} for k in ("pos_w", "flags", "dist_thresh", "error_thresh", "best_error_in", "equation_in", "out_status", "out_flags", "out_equation",
                                "out_best_error", "out_best_iter", "out_last_iter", "out_num_inliers", "out_inliers")]
    for over in bad:
        assert run(args(**over)) == -1, over
    assert run(args(n_cap=8193)) == -1 and b"8192" in L.plp_last_error()
    assert all(np.array_equal(o[k], before[k]) for k in o), "a rejected call wrote an output"
    # nothing to do: PLP_OK, nothing written
    assert run(args(P=0)) == 0 and run(args(n_cap=0)) == 1 and all(np.array_equal(o[k], before[k]) for k in o)
    # CREATE does not need the plane's earlier state; the optional outputs, counts and samples may be NULL
    assert run(args(mode=PR.CREATE, best_error_in=None, equation_in=None, out_hyp_residual=None, out_hyp_inliers=None, out_hyp_error=None, counts=None,
                    samples=None)) == 1
    assert run(args()) == 1 and int(o["status"][0]) == PR.OK
    # the other host builds
    assert L.plp_model_plane_fit_host(None, 0, None, None, 1, None, None, None) == -1 and L.plp_model_plane_fit_host(None, 0, None, None, 0, None, None, None) == 0
    assert L.plp_model_plane_draw_host(1, 0, 0, 4, 18, 0, None) == -1 and L.plp_model_plane_draw_host(1, 0, 0, 4, 18, 5, None) == -1
    r = plp.plane_refine_args_c()
    assert L.plp_model_plane_refine_points_host(None) == -1 and L.plp_model_plane_refine_points_host(C.byref(r)) == 0
    r.M = 3
    assert L.plp_model_plane_refine_points_host(C.byref(r)) == -1
    r.M = -1
    assert L.plp_model_plane_refine_points_host(C.byref(r)) == -1


def test_api_and_the_mirror_class():
    for name in ("plp_plane_ransac_device", "plp_plane_ransac_host", "plp_model_plane_ransac_host", "plp_model_plane_fit_host", "plp_model_plane_draw_host",
                 "plp_plane_refine_points_device", "plp_plane_refine_points_host", "plp_model_plane_refine_points_host"):
        assert name in plp.api_symbols()
    for name in ("plane_ransac", "plane_ransac_device", "plane_refine_points", "plane_refine_points_device"):
        assert hasattr(plp.matcher, name)
    cfg = {"Threshold.iterationsCount": 8, "Threshold.inliers_ratio_thr": 0.7, "Threshold.min_number_points_before_ransac": 12,
           "Threshold.point_per_ransac": 18, "Threshold.plane_distance_correction": 0.04, "Threshold.final_error_correction": 0.004}
    pm = plp.planar_mapper(cfg)
    pm.set_map_scale(0.5)
    assert pm.planar_distance_thresh == PS.DIST_THRESH and pm.final_error_thresh == PS.ERROR_THRESH
    q, (r, _) = SCENES["break_mid"][0], ref("break_mid")
    got = pm.estimate_plane_sequential_RANSAC(q["pos_w"], q["flags"], samples=q["samples"])
    assert got["status"] == PR.OK and same(got["equation"], np.array(r["equation"])) and np.array_equal(got["inliers"], r["inliers"])
    q, (r, _) = SCENES["u_ok"][0], ref("u_ok")
    got = pm.update_plane_via_RANSAC(q["pos_w"], q["flags"], q["equation_in"], q["best_error_in"], samples=q["samples"])
    assert got["status"] == PR.OK and same(got["equation"], np.array(r["equation"])) and got["best_iter"] == r["best_iter"] != got["last_iter"]
    sc = PS.refine_scene(3, 50)
    del sc["dist_thresh"]
    assert same(pm.refine_points(**sc)[0], PR.refine_points(dist_thresh=PS.DIST_THRESH, **sc)[0])
    with pytest.raises(plp.PlpError):
        plp.planar_mapper({**cfg, "Threshold.use_graph_cut": True})
