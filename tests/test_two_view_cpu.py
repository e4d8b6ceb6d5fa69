"""solve::essential_solver without a GPU: the host build of csrc/essential.hpp (plp.model_essential_*) against the
plain-Python restatement tests/two_view_ref.py, bit for bit, on every scene of tests/two_view_scene.py and every output over sentinel-filled
arrays; the restatement against an independent routine (numpy.linalg.svd in place of D24 item b) on the anchor scenes; the rules of D24
(recompute, ties, bad samples, NaN scores, too few matches, a match beyond counts_2), the generator, the argument checks of the header and
the mirror class."""
import ctypes as C
import itertools
import math

import numpy as np
import pytest

import two_view_ref as R
import two_view_scene as S
from plp import plp

SCENES = S.scenes()
SCENES["degenerate"] = S.degenerate_problem()
SCENES["nan"] = S.nan_problem()

# D24: the largest sign-aligned relative difference of E_21 between the definition and the numpy variant over the anchor scenes, as measured
# (profiles/r28_two_view.md); the test holds ten times that, the headroom being for other BLAS builds
MEASURED_MAX_SVD_E_DIFF = 5.8e-10
# a hypothesis of an anchor scene whose inlier tests all stay this far (relative) from the threshold cannot change a flag by the difference above
ANCHOR_MARGIN = 1e-5


def bits(a):
    return np.ascontiguousarray(a).tobytes()


def sentinels(want):
    return {k: np.full_like(v, R.SENTINEL[k]) for k, v in want.items()}


def model(q, recompute=True, samples="given", seed=0, **kw):
    return plp.model_essential_ransac(q["bearing_1"][None], q["bearing_2"][None], q["match"][None], iters=q["iters"], recompute=recompute,
                                      samples=q["samples"][None] if samples == "given" else None, seed=seed, **kw)


_ref_cache = {}


def ref(name, recompute=True, samples="given", seed=0, linalg="jacobi"):
    """the restatement's result of a scene, computed once and shared"""
    key = (name, recompute, samples, seed, linalg)
    if key not in _ref_cache:
        _ref_cache[key] = S.run_ref(SCENES[name], recompute, samples, seed, 0, linalg)
    return _ref_cache[key]


# ---------------------------------------------------------------------------------------------------------------- host build == restatement
WITH_SAMPLES = sorted(n for n, q in SCENES.items() if (q["match"] >= 0).sum() >= 8)      # the scenes whose samples name matches


@pytest.mark.parametrize("name", WITH_SAMPLES)
def test_fit_of_eight_rows_and_of_all_rows_is_the_restatements(name):
    q = SCENES[name]
    slots = np.flatnonzero(q["match"] >= 0)
    b1, b2 = q["bearing_1"][slots], q["bearing_2"][q["match"][slots]]
    lists = [np.asarray(s) for s in q["samples"][:6] if 0 <= min(s) and max(s) < len(slots)] + [np.arange(len(slots))]
    off = np.cumsum([0] + [len(l) for l in lists]).astype(np.int32)
    got = plp.model_essential_fit(np.concatenate([b1[l] for l in lists]), np.concatenate([b2[l] for l in lists]), off)
    for i, l in enumerate(lists):
        E, sweeps = R.compute_E_21(b1[l].tolist(), b2[l].tolist())
        assert bits(got["E_21"][i]) == bits(np.array(E)), (name, i)
        assert tuple(got["sweeps"][i]) == sweeps and max(sweeps) < 60


def test_fit_of_fewer_than_eight_rows_is_the_restatements():
    """compute_E_21 is defined for any number of rows: 7, 1 and 0 (A^T A of rank below 8: whichever column the Jacobi leaves last)"""
    q = SCENES["seven"]
    slots = np.flatnonzero(q["match"] >= 0)
    for rows in (7, 1, 0):
        b1, b2 = q["bearing_1"][slots[:rows]], q["bearing_2"][q["match"][slots[:rows]]]
        assert bits(plp.model_essential_fit(b1, b2)["E_21"]) == bits(np.array(R.compute_E_21(b1.tolist(), b2.tolist())[0])), rows


@pytest.mark.parametrize("name", WITH_SAMPLES)
def test_check_is_the_restatements(name):
    q = SCENES[name]
    r = ref(name, recompute=False)
    slots = R.matched_slots(q["match"].tolist(), len(q["match"]), len(q["bearing_2"]))
    its = [it for it in range(q["iters"]) if r["hyp_flags"][it] is not None][:5]
    assert its
    B1, B2 = q["bearing_1"][slots], q["bearing_2"][q["match"][slots]]
    Es = np.array([R.compute_E_21(B1[q["samples"][it]].tolist(), B2[q["samples"][it]].tolist())[0] for it in its])
    got = plp.model_essential_check(q["bearing_1"], q["bearing_2"], q["match"], Es)
    for i, it in enumerate(its):
        assert bits(got["score"][i]) == bits(np.float32(r["hyp_score"][it])), (name, it)
        flags = np.zeros(len(q["match"]), np.uint8)
        flags[slots] = r["hyp_flags"][it]
        assert np.array_equal(got["inliers"][i], flags) and got["num_inliers"][i] == flags.sum()


@pytest.mark.parametrize("samples", ["given", "drawn"])
@pytest.mark.parametrize("recompute", [True, False])
@pytest.mark.parametrize("name", sorted(SCENES))
def test_ransac_is_the_restatements_on_every_output(name, recompute, samples):
    q = SCENES[name]
    r = ref(name, recompute, samples, seed=41)
    want = R.expected([r], len(q["match"]), q["iters"])
    got = model(q, recompute, samples, seed=41, out=sentinels(want))
    for k in want:
        assert bits(got[k]) == bits(want[k]), (name, k, got[k], want[k])


def test_batched_ragged_problems_are_the_restatements():
    names = ["fisheye_64", "seven", "all_mismatched", "perspective_64", "none", "equirectangular_64"]
    qs = [SCENES[n] for n in names]
    a = S.pack(qs)
    rs = []
    for p, q in enumerate(qs):
        rs.append(R.find_via_ransac(a["bearing_1"][p], a["bearing_2"][p], a["match"][p].tolist(), iters=24, samples=None, seed=9, p=p,
                                    count_1=a["counts_1"][p], count_2=a["counts_2"][p]))
    want = R.expected(rs, a["match"].shape[1], 24)
    got = plp.model_essential_ransac(a["bearing_1"], a["bearing_2"], a["match"], iters=24, seed=9, counts_1=a["counts_1"], counts_2=a["counts_2"],
                                     out=sentinels(want))
    for k in want:
        assert bits(got[k]) == bits(want[k]), k
    assert set(want["status"].tolist()) == {R.OK, R.TOO_FEW_MATCHES, R.INVALID}


def test_every_status_is_reached_by_some_scene():
    seen = {ref(n, rec)["status"] for n in SCENES for rec in (True, False)}
    assert seen == {R.OK, R.TOO_FEW_MATCHES, R.INVALID}


# ---------------------------------------------------------------------------------------------------------------- anchors
def aligned_rel_diff(E, F):
    E, F = np.asarray(E), np.asarray(F)
    return min(np.abs(E - F).max(), np.abs(E + F).max()) / np.abs(F).max()


def test_anchor_scenes_agree_with_numpys_svd():
    """Condition: on the anchor scenes the inlier mask of every hypothesis and best_iter are equal between the definition and the variant that
    takes numpy.linalg.svd of the N x 9 matrix.  Bound: E_21 agrees up to sign within ten times the measured difference."""
    worst, min_margin = 0.0, math.inf
    for name in S.ANCHORS:
        for recompute in (False, True):
            a, b = ref(name, recompute), ref(name, recompute, linalg="svd")
            assert a["status"] == b["status"] == R.OK and a["best_iter"] == b["best_iter"], name
            assert a["hyp_flags"] == b["hyp_flags"] and a["inliers"] == b["inliers"], name
            min_margin = min(min_margin, a["margin"])
            worst = max(worst, aligned_rel_diff(a["E_21"], b["E_21"]))
        q = SCENES[name]
        slots = np.flatnonzero(q["match"] >= 0)
        B1, B2 = q["bearing_1"][slots], q["bearing_2"][q["match"][slots]]
        for s in q["samples"]:
            worst = max(worst, aligned_rel_diff(R.compute_E_21(B1[s].tolist(), B2[s].tolist())[0], R.compute_E_21(B1[s].tolist(), B2[s].tolist(), "svd")[0]))
    print("Jacobi on A^T A vs numpy svd of A: max sign-aligned relative difference of E_21", worst, "min threshold margin", min_margin)
    assert min_margin >= ANCHOR_MARGIN
    assert worst <= 10 * MEASURED_MAX_SVD_E_DIFF


def epipolar_truth(q):
    Rm, t = q["truth"]
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    E = tx @ Rm
    return E / np.linalg.norm(E)


GROUND_TRUTH = [n for n, q in SCENES.items() if q["kind"] == "cloud" and n not in ("degenerate", "nan", "all_mismatched", "seven", "none") and len(q["match"]) >= 64]


@pytest.mark.parametrize("name", GROUND_TRUTH)
def test_refit_matrix_of_the_host_build_against_the_scenes_essential_matrix(name):
    """out_E_21 of plp.model_essential_ransac (refit on) against [t]x R of the scene, both scaled to unit Frobenius norm, up to sign.  A scene
    without noise whose inliers are all true matches: 1e-9.  Otherwise the bound is the error of the same fit by an independent routine --
    numpy.linalg.svd of the N x 9 matrix over the same inliers, those of the best hypothesis -- against the truth, times two, and the two
    matrices agree within ten times the measured 5.8e-10 of the anchors."""
    q = SCENES[name]
    got = model(q, True)
    best = model(q, False)
    assert got["status"][0] == R.OK
    slots = np.flatnonzero(best["inliers"][0])
    T = epipolar_truth(q)
    err = lambda E: min(np.abs(E / np.linalg.norm(E) - T).max(), np.abs(E / np.linalg.norm(E) + T).max())
    E_np = np.array(R.compute_E_21(q["bearing_1"][slots].tolist(), q["bearing_2"][q["match"][slots]].tolist(), "svd")[0])
    assert aligned_rel_diff(got["E_21"][0], E_np) <= 10 * MEASURED_MAX_SVD_E_DIFF
    matched = np.flatnonzero(q["match"] >= 0)
    clean = q["noise"] == 0.0 and not best["inliers"][0][matched][q["is_mismatch"]].any()
    print(name, "error of the host build", err(got["E_21"][0]), "of numpy's fit", err(E_np))
    assert err(got["E_21"][0]) <= (1e-9 if clean else 2 * err(E_np))


# ---------------------------------------------------------------------------------------------------------------- the rules of D24
def test_recompute_refits_over_the_inliers_and_checks_again():
    q = SCENES["perspective_200"]
    a, b = ref("perspective_200", False), ref("perspective_200", True)
    assert a["best_iter"] == b["best_iter"] and a["status"] == b["status"] == R.OK
    slots = np.flatnonzero(q["match"] >= 0)
    keep = np.array(a["inliers"])[slots].astype(bool)
    E = plp.model_essential_fit(q["bearing_1"][slots][keep], q["bearing_2"][q["match"][slots]][keep])["E_21"]
    chk = plp.model_essential_check(q["bearing_1"], q["bearing_2"], q["match"], E)
    got = model(q, True)
    assert bits(got["E_21"][0]) == bits(E) and bits(got["score"][0]) == bits(chk["score"]) and np.array_equal(got["inliers"][0], chk["inliers"])
    assert got["num_inliers"][0] == chk["num_inliers"] == b["num_inliers"]


def test_a_tie_goes_to_the_lowest_iteration():
    q = dict(SCENES["fisheye_64"])
    r0 = ref("fisheye_64", False)
    top = int(np.argmax(r0["hyp_score"]))
    s = q["samples"].copy()
    other = s[(top + 1) % len(s)].copy()
    s[:] = other
    s[5] = s[11] = s[17] = q["samples"][top]
    q["samples"] = s
    if r0["hyp_score"][(top + 1) % len(s)] == r0["hyp_score"][top]:
        pytest.fail("the scene's two best samples tie")
    got = model(q, False, outputs=("hyp_score",))
    assert got["best_iter"][0] == 5 and got["hyp_score"][0][5] == got["hyp_score"][0][11] == got["hyp_score"][0][17] == got["hyp_score"][0].max()


def test_bad_samples_and_nan_scores_never_win():
    got = model(SCENES["degenerate"], False)
    h = got["hyp_score"][0]
    assert h[0] == 0 and h[1] == 0 and h[2] == 0 and h[3] == h[4] and got["best_iter"][0] == int(np.argmax(h))
    q = SCENES["nan"]
    got = model(q)
    assert np.isnan(got["hyp_score"][0]).all() and got["status"][0] == R.INVALID and got["best_iter"][0] == -1
    assert not got["E_21"].any() and got["score"][0] == 0 and got["num_inliers"][0] == 0 and not got["inliers"].any()
    only_bad = dict(q, samples=np.tile(np.array([0, 1, 2, 3, 4, 5, 6, 6], np.int32), (q["iters"], 1)), bearing_1=np.nan_to_num(q["bearing_1"], nan=0.1))
    got = model(only_bad)
    assert got["status"][0] == R.INVALID and not got["hyp_score"].any()


def test_fewer_than_eight_matches_and_exactly_eight():
    got = model(SCENES["seven"])
    assert got["status"][0] == R.TOO_FEW_MATCHES and got["num_matches"][0] == 7 and got["best_iter"][0] == -1 and not got["hyp_score"].any()
    got = model(SCENES["perspective_8"])
    assert got["status"][0] == R.OK and got["num_matches"][0] == 8 and got["num_inliers"][0] == 8
    d = model(SCENES["perspective_8"], samples="drawn", seed=3)                    # n == 8: every drawn sample is a permutation of all matches
    assert d["status"][0] == R.OK


def test_a_match_beyond_counts_2_is_no_match():
    q = SCENES["perspective_64"]
    m = len(q["bearing_2"])
    slots = np.flatnonzero(q["match"] >= 0)
    cut = int(np.sort(q["match"][slots])[len(slots) // 2])
    got = model(q, samples="drawn", seed=1, counts_2=np.array([cut], np.int32))
    hidden = dict(q, match=np.where(q["match"] >= cut, -1, q["match"]).astype(np.int32))
    want = model(hidden, samples="drawn", seed=1)
    assert got["num_matches"][0] == int((q["match"][slots] < cut).sum()) < len(slots) and m > cut
    for k in want:
        assert bits(got[k]) == bits(want[k]), k
    r = R.find_via_ransac(q["bearing_1"], q["bearing_2"], q["match"].tolist(), iters=q["iters"], samples=None, seed=1, count_2=cut)
    assert bits(got["E_21"][0]) == bits(np.array(r["E_21"])) and got["inliers"][0].tolist() == r["inliers"]


def test_slots_at_or_above_counts_1_keep_the_callers_value():
    q = SCENES["fisheye_64"]
    out = {"inliers": np.full((1, len(q["match"])), 0xEE, np.uint8)}
    got = model(q, counts_1=np.array([40], np.int32), out=out, samples="drawn")
    assert (got["inliers"][0, 40:] == 0xEE).all() and (got["inliers"][0, :40] <= 1).all()
    assert got["num_matches"][0] == int((q["match"][:40] >= 0).sum())


# ---------------------------------------------------------------------------------------------------------------- the generator
def test_generator_is_the_restatements_distinct_in_range_and_deterministic():
    for n in (8, 9, 17, 300, 8192):
        d = plp.model_essential_draw(12345, 3, 200, n)
        assert np.array_equal(d, np.array([R.draw(12345, 3, it, n) for it in range(200)]))
        assert d.min() >= 0 and d.max() < n
        assert all(len(set(r.tolist())) == 8 for r in d)
    a = plp.model_essential_draw(5, 0, 64, 1000)
    assert np.array_equal(a, plp.model_essential_draw(5, 0, 64, 1000)) and np.array_equal(a[10:20], plp.model_essential_draw(5, 0, 10, 1000, iter0=10))
    assert not np.array_equal(a, plp.model_essential_draw(5, 1, 64, 1000)) and not np.array_equal(a, plp.model_essential_draw(6, 0, 64, 1000))
    assert len({tuple(r) for r in a}) == 64


def test_generator_is_uniform_over_the_octuples_and_the_positions():
    d = plp.model_essential_draw(2024, 1, 20000, 10)
    counts = {t: 0 for t in itertools.combinations(range(10), 8)}
    for r in np.sort(d, 1):
        counts[tuple(int(v) for v in r)] += 1
    mean = 20000 / 45
    sd = math.sqrt(20000 * (1 / 45) * (44 / 45))
    assert len(counts) == 45 and min(counts.values()) > 0
    assert max(abs(c - mean) for c in counts.values()) <= 5 * sd, counts
    for pos in range(8):                                                               # ... and every index equally often at every position
        first = np.bincount(d[:, pos], minlength=10)
        assert np.abs(first - 20000 / 10).max() <= 5 * math.sqrt(20000 * (1 / 10) * (9 / 10)), pos


# ---------------------------------------------------------------------------------------------------------------- the argument checks
def test_every_invalid_argument_line_of_the_header():
    L = plp.lib()
    q = SCENES["perspective_64"]
    a = S.pack([q])
    n_cap, m_cap = a["match"].shape[1], a["bearing_2"].shape[1]
    o = {k: np.zeros((1,) + shape(n_cap, 24), dt) for k, (shape, dt, _) in plp.ESSENTIAL_OUTPUTS.items()}
    P = lambda v: v.ctypes.data

    def args(**over):
        s = plp.essential_ransac_args_c()
        f = dict(P=1, n_cap=n_cap, m_cap=m_cap, iters=24, recompute=1, seed=0, counts_1=P(a["counts_1"]), counts_2=P(a["counts_2"]), bearing_1=P(a["bearing_1"]),
                 bearing_2=P(a["bearing_2"]), match=P(a["match"]), samples=P(a["samples"]), out_status=P(o["status"]), out_num_matches=P(o["num_matches"]),
                 out_E_21=P(o["E_21"]), out_score=P(o["score"]), out_num_inliers=P(o["num_inliers"]), out_best_iter=P(o["best_iter"]),
                 out_inliers=P(o["inliers"]), out_hyp_score=P(o["hyp_score"]))
        f.update(over)
        for k, v in f.items():
            setattr(s, k, v)
        return s
    run = lambda s: L.plp_model_essential_ransac_host(C.byref(s))
    assert run(args()) == 1 and int(o["status"][0]) == R.OK
    assert L.plp_model_essential_ransac_host(None) == -1
    bad = [dict(P=-1), dict(n_cap=-1), dict(m_cap=-1), dict(iters=0), dict(n_cap=8193), dict(P=65536), dict(iters=65537)]
    bad += [{k: None} for k in ("bearing_1", "bearing_2", "match", "out_status", "out_num_matches", "out_E_21", "out_score", "out_num_inliers", "out_best_iter")]
    before = {k: v.copy() for k, v in o.items()}
    for over in bad:
        assert run(args(**over)) == -1, over
    assert all(np.array_equal(o[k], before[k]) for k in o), "a rejected call wrote an output"
    # nothing to do: PLP_OK, nothing written; the optional outputs, the counts and the samples may be NULL
    assert run(args(P=0)) == 0 and run(args(n_cap=0)) == 1 and all(np.array_equal(o[k], before[k]) for k in o)
    assert run(args(out_inliers=None, out_hyp_score=None, counts_1=None, counts_2=None, samples=None)) == 1
    assert run(args(m_cap=0, bearing_2=None, counts_2=None)) == 1 and int(o["status"][0]) == R.TOO_FEW_MATCHES
    # the other host builds
    assert L.plp_model_essential_fit_host(None, None, None, 1, None, None) == -1 and L.plp_model_essential_fit_host(None, None, None, 0, None, None) == 0
    assert L.plp_model_essential_check_host(None, None, None, 4, 4, None, 0, None, None, None) == -1
    assert L.plp_model_essential_check_host(None, None, None, 0, 0, None, 1, None, None, None) == -1
    assert L.plp_model_essential_draw_host(1, 0, 0, 4, 7, None) == -1 and L.plp_model_essential_draw_host(1, 0, 0, 4, 8, None) == -1


def test_the_mirror_class_has_the_references_surface():
    q = SCENES["perspective_200"]
    pairs = [(s, int(m)) for s, m in enumerate(q["match"]) if m >= 0]
    s = plp.essential_solver(q["bearing_1"], q["bearing_2"], pairs, samples=q["samples"])
    assert not s.solution_is_valid()
    s.find_via_ransac(q["iters"])
    want = ref("perspective_200", True)
    assert s.solution_is_valid() and bits(s.get_best_E_21()) == bits(np.array(want["E_21"])) and np.float32(s.get_best_score()) == np.float32(want["score"])
    flags = s.get_inlier_matches()
    assert flags.dtype == bool and len(flags) == len(pairs) and flags.tolist() == [bool(want["inliers"][i]) for i, _ in pairs]
    s.find_via_ransac(q["iters"], False)
    assert bits(s.get_best_E_21()) == bits(np.array(ref("perspective_200", False)["E_21"]))
    with pytest.raises(plp.PlpError):
        plp.essential_solver(q["bearing_1"], q["bearing_2"], pairs[::-1])
    for name in ("find_via_ransac", "solution_is_valid", "get_best_E_21", "get_best_score", "get_inlier_matches"):
        assert callable(getattr(plp.essential_solver, name))
