"""The two solvers of initialize::perspective without a GPU: the host build of csrc/perspective_init.hpp
(plp.model_perspective_ransac and the plp.model_* pieces) against the plain-Python restatement tests/perspective_init_ref.py, bit for bit, on every
scene of tests/perspective_init_scene.py and every output over sentinel-filled arrays; a census of what the scenes reach; the restatement against an
independent linear algebra (numpy.linalg.svd and numpy.linalg.inv in place of the Jacobi and the cofactor inverse) on the anchor scenes; the matrices
against the scenes' ground truth; the rules of D27 (recompute, ties, bad samples, a singular sample, NaN and constant frames, too few matches, the
counts, a given homography, the two sample streams), the argument checks of the header and the mirror classes.

Measured on the anchor scenes (printed by test_anchor_scenes_agree_with_numpys_linear_algebra): the largest relative difference, up to scale and
sign, between the definition and the numpy variant is 8.2e-14 for H_21 and 2.7e-10 for F_21, the smallest relative distance of an inlier test from
its threshold 9.6e-5; with numpy's SVD also in the two decompositions, no hypothesis of an anchor scene's pose step deviates by more than 1.4e-12
(test_anchor_poses_agree_with_numpys_linear_algebra)."""
import ctypes as C
import math

import numpy as np
import pytest

import perspective_init_ref as R
import perspective_init_scene as S
from plp import plp

SCENES = S.scenes()
SCENES["degenerate"] = S.degenerate_problem()
SCENES["nan"] = S.nan_problem()
SCENES["constant"] = S.constant_frame_problem()

# D27: the largest relative difference, up to scale and sign, of H_21 and of F_21 between the definition and the numpy variant over the anchor scenes, as
# measured; the test holds each matrix to ten times its own figure (D24's margin: the Jacobi and LAPACK agree to rounding, the factor is for another libm or BLAS build)
MEASURED_MAX_SVD_DIFF = dict(h=8.2e-14, f=2.7e-10)
# a hypothesis of an anchor scene whose inlier tests all stay this far (relative) from the threshold cannot change a flag by the difference above
ANCHOR_MARGIN = 5e-5


def bits(a):
    return np.ascontiguousarray(a).tobytes()


def sentinels(want):
    return {k: np.full_like(v, R.SENTINEL[k]) for k, v in want.items()}


def model(q, recompute=True, samples="given", seed=0, given=None, **kw):
    a = S.pack([q], given=None if given is None else {0: given})
    pos, k = S.call_kwargs(a, recompute, None if samples == "given" else seed)
    k.update(kw)
    return plp.model_perspective_ransac(*pos, **k)


_ref_cache = {}


def ref(name, recompute=True, samples="given", seed=0, linalg="jacobi"):
    """the restatement's result of a scene, computed once and shared"""
    key = (name, recompute, samples, seed, linalg)
    if key not in _ref_cache:
        _ref_cache[key] = S.run_ref(SCENES[name], recompute, samples, seed, 0, linalg)
    return _ref_cache[key]


def matched(q):
    """the matches' points as the key points hold them (n, 4) and the frames' normalisations"""
    slots = np.flatnonzero(q["match"] >= 0)
    k1, k2 = S.xy(q["undist_1"]), S.xy(q["undist_2"])
    return slots, np.concatenate([k1[slots], k2[q["match"][slots]]], 1)


# ---------------------------------------------------------------------------------------------------------------- host build == restatement
WITH_SAMPLES = sorted(n for n, q in SCENES.items() if (q["match"] >= 0).sum() >= 8)


@pytest.mark.parametrize("name", sorted(SCENES))
def test_normalize_is_the_restatements(name):
    q = SCENES[name]
    for kp in (q["undist_1"], q["undist_2"], q["undist_1"][:1], q["undist_1"][:0]):
        got = plp.model_normalize_keypoints(kp)
        nrm = R.normalize(S.xy(kp).tolist())
        want = np.array(nrm, np.float32)
        assert np.array_equal(np.isnan(got["stats"]), np.isnan(want)) and bits(np.nan_to_num(got["stats"])) == bits(np.nan_to_num(want)), name
        T = np.array(R.transform(nrm))
        assert np.array_equal(np.isnan(T), np.isnan(got["transform"])) and bits(np.nan_to_num(T)) == bits(np.nan_to_num(got["transform"]))
        pts = np.array([[R.normalized(x, nrm[0], nrm[2]), R.normalized(y, nrm[1], nrm[3])] for x, y in S.xy(kp).tolist()], np.float32).reshape(-1, 2)
        assert bits(np.nan_to_num(pts)) == bits(np.nan_to_num(got["normalized"])) and np.array_equal(np.isnan(pts), np.isnan(got["normalized"]))


def normalized_pairs(q):
    slots, pts = matched(q)
    n1, n2 = R.normalize(S.xy(q["undist_1"]).tolist()), R.normalize(S.xy(q["undist_2"]).tolist())
    return [(R.normalized(a, n1[0], n1[2]), R.normalized(b, n1[1], n1[3]), R.normalized(c, n2[0], n2[2]), R.normalized(d, n2[1], n2[3])) for a, b, c, d in pts.tolist()]


IDENT = [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]


@pytest.mark.parametrize("name", [n for n in WITH_SAMPLES if n not in ("nan", "constant")])
def test_fits_of_eight_pairs_and_of_all_pairs_are_the_restatements(name):
    q = SCENES[name]
    pairs = np.array(normalized_pairs(q), np.float32)
    lists = [np.asarray(s) for s in q["samples_h"][:4] if 0 <= min(s) and max(s) < len(pairs)] + [np.arange(len(pairs)), np.arange(7), np.arange(1), np.arange(0)]
    off = np.cumsum([0] + [len(l) for l in lists]).astype(np.int32)
    p1, p2 = np.concatenate([pairs[l, :2] for l in lists]), np.concatenate([pairs[l, 2:] for l in lists])
    for solver, fn, key in ((R.H, plp.model_homography_fit, "H_21"), (R.F, plp.model_fundamental_fit, "F_21")):
        got = fn(p1, p2, off)
        for i, l in enumerate(lists):
            M, sweeps = R.fit(solver, [tuple(map(float, r)) for r in pairs[l]], IDENT, IDENT)
            assert bits(got[key][i]) == bits(np.array(M)), (name, key, i)
            assert got["sweeps"][i] == sweeps < 60


@pytest.mark.parametrize("name", WITH_SAMPLES)
def test_checks_are_the_restatements(name):
    q = SCENES[name]
    r = ref(name, recompute=False)
    slots, pts = matched(q)
    rng = np.random.default_rng(5)
    for solver, key, fn in ((R.H, "h", plp.model_homography_check), (R.F, "f", plp.model_fundamental_check)):
        Ms = rng.standard_normal((3, 3, 3))
        Ms[0] = np.eye(3)
        Ms[2] = np.outer([1.0, 2.0, 3.0], [0.5, -1.0, 2.0]) if solver == R.H else Ms[2]   # a singular homography: its inverse is infinite
        got = fn(q["undist_1"], q["undist_2"], q["match"], Ms)
        for i, M in enumerate(Ms):
            score, flags, _ = R.check_inliers(solver, M.tolist(), pts.tolist())
            assert (math.isnan(score) and np.isnan(got["score"][i])) or bits(got["score"][i]) == bits(np.float32(score)), (name, key, i)
            want = np.zeros(len(q["match"]), np.uint8)
            want[slots] = flags
            assert np.array_equal(got["inliers"][i], want) and got["num_inliers"][i] == want.sum()
        if solver == R.H:
            assert not got["score"][2] > 0, "a singular homography must not score"


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


def given_cases():
    """name -> (scene, H, count): the planar scene's own matrix (valid), the same with a count below eight, a matrix that fits nothing, a singular one"""
    planar = ref("planar")
    Hm = np.array(planar["h"]["M"])
    return dict(valid=("planar", Hm, planar["h"]["num_inliers"]), low_count=("planar", Hm, 7), misfit=("cloud_64", np.eye(3), 40),
                singular=("planar", np.outer([1.0, 2.0, 3.0], [0.5, -1.0, 2.0]), 40), few=("seven", np.eye(3), 30), refit_of_f=("cloud_200", np.eye(3) * 2.0, 9))


@pytest.mark.parametrize("case", sorted(given_cases()))
def test_a_given_homography_is_the_restatements(case):
    name, Hm, count = given_cases()[case]
    q = SCENES[name]
    r = S.run_ref(q, given=(Hm, count))
    want = R.expected([r], len(q["match"]), q["iters"])
    got = model(q, given=(Hm, count), out=sentinels(want))
    for k in want:
        assert bits(got[k]) == bits(want[k]), (case, k)
    status = dict(valid=R.OK, low_count=R.INVALID, misfit=R.INVALID, singular=R.INVALID, few=R.TOO_FEW_MATCHES, refit_of_f=R.INVALID)[case]
    assert got["status_h"][0] == status and got["best_iter_h"][0] == -1 and not got["hyp_score_h"].any()
    if case == "valid":
        assert bits(got["H_21"][0]) == bits(Hm) and got["choice"][0] == R.CHOICE_H and got["num_inliers_h"][0] == count
    base = ref(name)
    assert got["status_f"][0] == base["f"]["status"] and bits(got["F_21"][0]) == bits(np.array(base["f"]["M"]))    # F is not affected


def test_batched_ragged_problems_are_the_restatements():
    names = ["planar", "seven", "all_mismatched", "cloud_64", "none", "nan", "fisheye_200"]
    qs = [dict(SCENES[n]) for n in names]
    for q in qs:
        q["samples_h"], q["samples_f"], q["iters"] = q["samples_h"][:6], q["samples_f"][:6], 6
    given = {3: (np.array(ref("planar")["h"]["M"]), 20)}
    a = S.pack(qs, given=given)
    rs = []
    for p, q in enumerate(qs):
        kp1, kp2 = S.xy(a["undist_1"][p]).tolist(), S.xy(a["undist_2"][p]).tolist()
        g = dict(given_H=given[p][0], given_count=given[p][1]) if p in given else {}
        rs.append(R.perspective_ransac(kp1, kp2, a["match"][p].tolist(), iters=6, samples_h=None, samples_f=None, seed=9, p=p, count_1=a["counts_1"][p],
                                       count_2=a["counts_2"][p], **g))
    want = R.expected(rs, a["match"].shape[1], 6)
    pos, kw = S.call_kwargs(a, True, 9)
    got = plp.model_perspective_ransac(*pos, out=sentinels(want), **kw)
    for k in want:
        assert bits(got[k]) == bits(want[k]), k
    assert set(want["status_f"].tolist()) == {R.OK, R.TOO_FEW_MATCHES, R.INVALID}


# ---------------------------------------------------------------------------------------------------------------- the census
def test_census_of_what_the_scenes_reach():
    runs = {(n, rec): ref(n, rec) for n in SCENES for rec in (True, False)}
    choices = {r["choice"] for r in runs.values()}
    assert choices == {R.CHOICE_NONE, R.CHOICE_H, R.CHOICE_F}, choices
    assert runs[("planar", True)]["choice"] == R.CHOICE_H and runs[("cloud_200", True)]["choice"] == R.CHOICE_F
    assert runs[("all_mismatched", True)]["choice"] == R.CHOICE_NONE and runs[("all_mismatched", True)]["h"]["status"] == R.INVALID
    for key in ("h", "f"):
        assert {r[key]["status"] for r in runs.values()} == {R.OK, R.TOO_FEW_MATCHES, R.INVALID}, key
    # a solver that is not valid with a score above 0: fewer than eight inliers; the score still enters rel_score_h
    assert any(r["h"]["status"] == R.INVALID and r["h"]["score"] > 0 and not math.isnan(r["rel_score_h"]) for r in runs.values())
    # H valid and yet F chosen: rel_score_h at or below 0.40
    assert any(r["h"]["status"] == R.OK and r["choice"] == R.CHOICE_F and r["rel_score_h"] <= 0.40 for r in runs.values())
    # the given homography, valid and invalid
    statuses = {case: S.run_ref(SCENES[name], given=(Hm, count))["h"]["status"] for case, (name, Hm, count) in given_cases().items()}
    assert statuses["valid"] == R.OK and statuses["low_count"] == statuses["singular"] == statuses["misfit"] == R.INVALID
    # the sample of eight collinear key points (iteration 5 of the degenerate problem) does not win, and neither does a NaN
    d = runs[("degenerate", False)]
    assert d["h"]["hyp_flags"][5] is not None and d["h"]["best_iter"] != 5 and not d["h"]["hyp_score"][5] > max(d["h"]["hyp_score"][3], 0.0)
    n = runs[("nan", True)]
    assert all(math.isnan(s) for s in n["h"]["hyp_score"] + n["f"]["hyp_score"]) and n["choice"] == R.CHOICE_NONE and math.isnan(n["rel_score_h"])
    c = runs[("constant", True)]
    assert c["h"]["status"] == c["f"]["status"] == R.INVALID


# ---------------------------------------------------------------------------------------------------------------- anchors
def scaled_rel_diff(A, B):
    """the largest entry of A / |A| -+ B / |B|, the smaller of the two signs"""
    A, B = np.asarray(A), np.asarray(B)
    A, B = A / np.linalg.norm(A), B / np.linalg.norm(B)
    return min(np.abs(A - B).max(), np.abs(A + B).max())


def test_anchor_scenes_agree_with_numpys_linear_algebra():
    """Condition: on the anchor scenes the inlier mask of every hypothesis of both solvers, both best iterations, the H/F choice and the chosen mask
    are equal between the definition and the variant that takes numpy.linalg.svd of the row matrix and numpy.linalg.inv.  Bound: H_21 and F_21 agree up
    to scale and sign, each within ten times its own measured difference (8.2e-14 for H_21, 2.7e-10 for F_21; the margin of the inlier tests 9.6e-5)."""
    worst, min_margin = dict(h=0.0, f=0.0), math.inf
    for name in S.ANCHORS:
        for recompute in (False, True):
            a, b = ref(name, recompute), ref(name, recompute, linalg="svd")
            assert a["choice"] == b["choice"] != R.CHOICE_NONE and a["inliers"] == b["inliers"], name
            for key in ("h", "f"):
                assert a[key]["status"] == b[key]["status"] and a[key]["best_iter"] == b[key]["best_iter"], (name, key)
                assert a[key]["hyp_flags"] == b[key]["hyp_flags"] and a[key]["flags"] == b[key]["flags"], (name, key)
                min_margin = min(min_margin, a[key]["margin"])
                if a[key]["status"] == R.OK:
                    worst[key] = max(worst[key], scaled_rel_diff(a[key]["M"], b[key]["M"]))
    print("Jacobi / cofactor inverse vs numpy svd / inv: max relative difference up to scale and sign", worst, "min threshold margin", min_margin)
    assert min_margin >= ANCHOR_MARGIN
    assert all(worst[key] <= 10 * MEASURED_MAX_SVD_DIFF[key] for key in worst), worst


K = np.array([[517.3, 0.0, 318.6], [0.0, 516.5, 255.3], [0.0, 0.0, 1.0]])


def truth_matrix(q, solver):
    """the homography of the planar scene's plane (n . X = 6 in frame 1) or the fundamental matrix of the scene's motion, in pixels"""
    Rm, t = q["truth"]
    if solver == R.H:
        nrm = np.array([0.2, -0.1, 1.0]) / np.linalg.norm([0.2, -0.1, 1.0])
        return K @ (Rm + np.outer(t, nrm) / 6.0) @ np.linalg.inv(K)
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    return np.linalg.inv(K).T @ tx @ Rm @ np.linalg.inv(K)


@pytest.mark.parametrize("name,solver", [("planar", R.H), ("cloud_64", R.F), ("cloud_200", R.F), ("exact", R.F)])
def test_refit_matrix_of_the_host_build_against_the_scenes_ground_truth(name, solver):
    """out_H_21 of the planar scene and out_F_21 of the cloud scenes (refit on) against the matrix of the scene's motion, up to scale and sign.  The
    bound is the error of the same fit by an independent routine -- numpy.linalg.svd of the row matrix over the same inliers, those of the best
    hypothesis -- against the truth, times two (1e-7 at least: the key points are floats), and the two fits agree within ten times the anchors'
    measured difference."""
    q = SCENES[name]
    key, out = ("h", "H_21") if solver == R.H else ("f", "F_21")
    got, best = model(q, True), ref(name, False)
    assert got["status_" + key][0] == R.OK and got["choice"][0] == (R.CHOICE_H if solver == R.H else R.CHOICE_F)
    pairs = normalized_pairs(q)
    n1, n2 = R.normalize(S.xy(q["undist_1"]).tolist()), R.normalize(S.xy(q["undist_2"]).tolist())
    M_np, _ = R.fit(solver, [pairs[k] for k in range(len(pairs)) if best[key]["flags"][k]], R.transform(n1), R.transform(n2), "svd")
    assert scaled_rel_diff(got[out][0], M_np) <= 10 * MEASURED_MAX_SVD_DIFF[key]
    T = truth_matrix(q, solver)
    print(name, "error of the host build", scaled_rel_diff(got[out][0], T), "of numpy's fit", scaled_rel_diff(M_np, T))
    assert scaled_rel_diff(got[out][0], T) <= max(2 * scaled_rel_diff(M_np, T), 1e-7)
    # the mask of the matrix returned keeps the true matches and drops the gross mismatches
    slots = np.flatnonzero(q["match"] >= 0)
    mask = got["inliers"][0][slots].astype(bool)
    assert mask[~q["is_mismatch"]].mean() >= 0.9 and mask[q["is_mismatch"]].mean() <= 0.1 if q["is_mismatch"].any() else mask.all()


# ---------------------------------------------------------------------------------------------------------------- the rules of D27
def test_recompute_refits_over_the_inliers_and_checks_again():
    q = SCENES["planar"]
    a, b = ref("planar", False), ref("planar", True)
    pairs = np.array(normalized_pairs(q), np.float32)
    got = model(q, True)
    t1, t2 = plp.model_normalize_keypoints(q["undist_1"])["transform"], plp.model_normalize_keypoints(q["undist_2"])["transform"]
    for key, out, fit, chk in (("h", "H_21", plp.model_homography_fit, plp.model_homography_check), ("f", "F_21", plp.model_fundamental_fit, plp.model_fundamental_check)):
        assert a[key]["best_iter"] == b[key]["best_iter"] and a[key]["status"] == b[key]["status"] == R.OK
        keep = np.array(a[key]["flags"], bool)
        Mn = fit(pairs[keep, :2], pairs[keep, 2:])[out]
        M = np.array(R.mul3(R.mul3(R.inv3(t2.tolist()) if key == "h" else R.transpose3(t2.tolist()), Mn.tolist()), t1.tolist()))
        c = chk(q["undist_1"], q["undist_2"], q["match"], M)
        assert bits(got[out][0]) == bits(M) and bits(got["score_" + key][0]) == bits(c["score"]) and np.array_equal(got["inliers_" + key][0], c["inliers"])
        assert got["num_inliers_" + key][0] == c["num_inliers"] == b[key]["num_inliers"]


def test_a_tie_goes_to_the_lowest_iteration():
    q = dict(SCENES["planar"])
    r0 = ref("planar", False)
    for key in ("h", "f"):
        top = int(np.argmax(r0[key]["hyp_score"]))
        s = q["samples_" + key].copy()
        s[:] = s[(top + 1) % len(s)].copy()
        s[5] = s[11] = s[17] = q["samples_" + key][top]
        assert r0[key]["hyp_score"][(top + 1) % len(s)] != r0[key]["hyp_score"][top]
        q["samples_" + key] = s
    got = model(q, False)
    for key in ("h", "f"):
        h = got["hyp_score_" + key][0]
        assert got["best_iter_" + key][0] == 5 and h[5] == h[11] == h[17] == h.max()


def test_bad_samples_a_singular_sample_and_nan_scores_never_win():
    got = model(SCENES["degenerate"], False)
    for key in ("h", "f"):
        h = got["hyp_score_" + key][0]
        assert h[0] == 0 and h[1] == 0 and h[2] == 0 and h[3] == h[4] and got["best_iter_" + key][0] in (-1, int(np.nanargmax(h)))
    assert got["best_iter_h"][0] != 5
    q = SCENES["nan"]
    got = model(q)
    assert np.isnan(got["hyp_score_h"][0]).all() and np.isnan(got["hyp_score_f"][0]).all() and np.isnan(got["rel_score_h"][0])
    assert got["status_h"][0] == got["status_f"][0] == R.INVALID and got["choice"][0] == R.CHOICE_NONE and not got["inliers"].any()
    assert not got["H_21"].any() and not got["F_21"].any() and got["score_h"][0] == got["score_f"][0] == 0
    assert bits(got["rel_score_h"]) == bits(np.array([np.nan], np.float32)), "a NaN output is the canonical quiet NaN"


def test_fewer_than_eight_matches_and_exactly_eight():
    got = model(SCENES["seven"])
    assert got["status_h"][0] == got["status_f"][0] == R.TOO_FEW_MATCHES and got["num_matches"][0] == 7 and got["choice"][0] == R.CHOICE_NONE
    assert not got["hyp_score_h"].any() and not got["hyp_score_f"].any() and np.isnan(got["rel_score_h"][0])
    got = model(SCENES["eight"])
    assert got["status_f"][0] == R.OK and got["num_matches"][0] == 8 and got["num_inliers_f"][0] == 8
    assert model(SCENES["eight"], samples="drawn", seed=3)["status_f"][0] == R.OK     # n == 8: every drawn sample is a permutation of all matches


def test_the_counts_hide_key_points_matches_and_slots():
    q = SCENES["cloud_64"]
    slots = np.flatnonzero(q["match"] >= 0)
    cut = int(np.sort(q["match"][slots])[len(slots) // 2])
    got = model(q, samples="drawn", seed=1, counts_2=np.array([cut], np.int32))
    r = S.run_ref(q, samples="drawn", seed=1, count_2=cut)
    assert got["num_matches"][0] == int((q["match"][slots] < cut).sum()) < len(slots)
    assert bits(got["F_21"][0]) == bits(np.array(r["f"]["M"])) and got["inliers"][0].tolist() == r["inliers"]
    hidden = dict(q, match=np.where(q["match"] >= cut, -1, q["match"]).astype(np.int32))
    other = model(hidden, samples="drawn", seed=1)
    assert bits(other["F_21"]) != bits(got["F_21"]), "the normalisation runs over the key points the count leaves, not over the matched ones"
    out = {"inliers": np.full((1, len(q["match"])), 0xEE, np.uint8)}
    got = model(q, counts_1=np.array([40], np.int32), out=out, samples="drawn")
    assert (got["inliers"][0, 40:] == 0xEE).all() and (got["inliers"][0, :40] <= 1).all() and got["num_matches"][0] == int((q["match"][:40] >= 0).sum())


def test_the_two_solvers_draw_from_different_streams_of_the_generator():
    for n in (8, 9, 300, 8192):
        h, f = plp.model_perspective_draw(0, 12345, 3, 50, n), plp.model_perspective_draw(1, 12345, 3, 50, n)
        assert np.array_equal(h, np.array([R.draw(12345, 3, it, n) for it in range(50)]))
        assert np.array_equal(f, np.array([R.draw(12345, 3 + R.STREAM_OF_F, it, n) for it in range(50)]))
        assert np.array_equal(h, plp.model_essential_draw(12345, 3, 50, n)) and (n == 8 or not np.array_equal(h, f))
        assert all(len(set(r.tolist())) == 8 and r.min() >= 0 and r.max() < n for r in np.concatenate([h, f]))
    assert np.array_equal(plp.model_perspective_draw(1, 5, 0, 10, 100, iter0=10), plp.model_perspective_draw(1, 5, 0, 20, 100)[10:])
    with pytest.raises(plp.PlpError):
        plp.model_perspective_draw(2, 5, 0, 10, 100)


# ---------------------------------------------------------------------------------------------------------------- the argument checks
def test_every_invalid_argument_line_of_the_header():
    L = plp.lib()
    q = SCENES["cloud_64"]
    a = S.pack([q], given={0: (np.eye(3), -1)})
    n_cap, m_cap = a["match"].shape[1], a["undist_2"].shape[1]
    o = {k: np.zeros((1,) + shape(n_cap, 24), dt) for k, (shape, dt, _) in plp.PERSPECTIVE_RANSAC_OUTPUTS.items()}
    P = lambda v: v.ctypes.data
    required = [k for k, v in plp.PERSPECTIVE_RANSAC_OUTPUTS.items() if not v[2]]

    def args(**over):
        s = plp.perspective_ransac_args_c()
        f = dict(P=1, n_cap=n_cap, m_cap=m_cap, iters=24, recompute=1, seed=0, **{k: P(a[k]) for k in a}, **{"out_" + k: P(v) for k, v in o.items()})
        f.update(over)
        for k, v in f.items():
            setattr(s, k, v)
        return s
    run = lambda s: L.plp_model_perspective_ransac_host(C.byref(s))
    assert run(args()) == 1 and int(o["status_f"][0]) == R.OK
    assert L.plp_model_perspective_ransac_host(None) == -1
    bad = [dict(P=-1), dict(n_cap=-1), dict(m_cap=-1), dict(iters=0), dict(n_cap=8193), dict(P=65536), dict(iters=65537), dict(given_H_21=None),
           dict(given_H_num_inliers=None)]
    bad += [{k: None} for k in ("undist_1", "undist_2", "match")] + [{"out_" + k: None} for k in required]
    before = {k: v.copy() for k, v in o.items()}
    for over in bad:
        assert run(args(**over)) == -1, over
    assert all(np.array_equal(o[k], before[k]) for k in o), "a rejected call wrote an output"
    # nothing to do: PLP_OK, nothing written; the optional outputs, the counts, the samples and the given homography may be NULL
    assert run(args(P=0)) == 0 and run(args(n_cap=0)) == 1 and all(np.array_equal(o[k], before[k]) for k in o)
    assert run(args(out_inliers_h=None, out_inliers_f=None, out_hyp_score_h=None, out_hyp_score_f=None, counts_1=None, counts_2=None, samples_h=None, samples_f=None,
                    given_H_21=None, given_H_num_inliers=None)) == 1
    assert run(args(m_cap=0, undist_2=None, counts_2=None)) == 1 and int(o["status_h"][0]) == int(o["status_f"][0]) == R.TOO_FEW_MATCHES
    # the other host builds
    assert L.plp_model_homography_fit_host(None, None, None, 1, None, None) == -1 and L.plp_model_fundamental_fit_host(None, None, None, 0, None, None) == 0
    assert L.plp_model_homography_check_host(None, None, None, 4, 4, None, 0, None, None, None) == -1
    assert L.plp_model_fundamental_check_host(None, None, None, 0, 0, None, 1, None, None, None) == -1
    assert L.plp_model_normalize_keypoints_host(None, 3, None, None, None) == -1
    assert L.plp_model_perspective_draw_host(0, 1, 0, 0, 4, 7, None) == -1 and L.plp_model_perspective_draw_host(0, 1, 0, 0, 4, 8, None) == -1


def test_the_mirror_classes_have_the_references_surface():
    q = SCENES["planar"]
    pairs = [(s, int(m)) for s, m in enumerate(q["match"]) if m >= 0]
    want = ref("planar", True)
    for cls, key, get in ((plp.homography_solver, "h", "get_best_H_21"), (plp.fundamental_solver, "f", "get_best_F_21")):
        s = cls(q["undist_1"], q["undist_2"], pairs, 1.0, samples=q["samples_" + key])
        assert not s.solution_is_valid()
        s.find_via_ransac(q["iters"])
        assert s.solution_is_valid() and bits(getattr(s, get)()) == bits(np.array(want[key]["M"])) and np.float32(s.get_best_score()) == np.float32(want[key]["score"])
        flags = s.get_inlier_matches()
        assert flags.dtype == bool and len(flags) == len(pairs) and flags.tolist() == [bool(f) for f in want[key]["flags"]]
        s.find_via_ransac(q["iters"], False)
        assert bits(getattr(s, get)()) == bits(np.array(ref("planar", False)[key]["M"]))
        with pytest.raises(plp.PlpError):
            cls(q["undist_1"], q["undist_2"], pairs[::-1])
        with pytest.raises(plp.PlpError):
            cls(q["undist_1"], q["undist_2"], pairs, 2.0)
        for name in ("find_via_ransac", "solution_is_valid", get, "get_best_score", "get_inlier_matches"):
            assert callable(getattr(s, name))
    s = plp.homography_solver(S.xy(q["undist_1"]), S.xy(q["undist_2"]), pairs)
    s.use_matrix(want["h"]["M"], want["h"]["num_inliers"])
    assert s.solution_is_valid() and bits(s.get_best_H_21()) == bits(np.array(want["h"]["M"]))
    s.use_matrix(want["h"]["M"], 7)
    assert not s.solution_is_valid()


# ---------------------------------------------------------------------------------------------------------------- from the chosen matrix to the pose
import two_view_ref as TR
import two_view_scene as TS

POSE_SCENES = dict(SCENES, planar_pose=S.problem(510, 150, "perspective", n_slots=160, noise=5e-4, mismatch=0.1, kind="planar"))


def pose_inputs(q, **kw):
    """the RANSAC's outputs of a scene (host build) and the pose entry's arguments"""
    e = model(q)
    cam = plp.camera_model(TS.CAMERAS[q["camera"]])
    pos = (cam, e["choice"], e["H_21"], e["F_21"], e["inliers"], q["match"][None], q["bearing_1"][None], q["bearing_2"][None], q["undist_1"][None], q["undist_2"][None])
    return e, pos, dict(img_bounds=q["bounds"], **kw)


def pose_ref(q, e, choice=None, Hm=None, **kw):
    return R.perspective_pose(TS.ref_camera(q["camera"]), [float(v) for v in q["bounds"]], int(e["choice"][0]) if choice is None else choice,
                              (e["H_21"][0] if Hm is None else Hm).tolist(), e["F_21"][0].tolist(), e["inliers"][0].tolist(), q["match"].tolist(), q["bearing_1"],
                              q["bearing_2"], S.xy(q["undist_1"]).tolist(), S.xy(q["undist_2"]).tolist(), **kw)


def pose_sentinels(want):
    return {k: np.full_like(v, TR.TV_SENTINEL[k]) for k, v in want.items()}


POSE_CASES = [(n, {}) for n in sorted(POSE_SCENES) if n not in ("nan", "constant")] + [("cloud_64", dict(min_num_triangulated=20)),
                                                                                        ("degenerate", dict(min_num_triangulated=20))]


@pytest.mark.parametrize("name,kw", POSE_CASES)
def test_pose_is_the_restatements_on_every_output(name, kw):
    q = POSE_SCENES[name]
    e, pos, k = pose_inputs(q, **kw)
    want = R.pose_expected([pose_ref(q, e, **kw)], len(q["match"]))
    got = plp.model_perspective_pose(*pos, out=pose_sentinels(want), **k)
    for key in want:
        assert bits(got[key]) == bits(want[key]), (name, key)


# D27: the largest deviation (an entry of a rotation, a component of a unit translation) of any hypothesis of the anchor scenes between the definition and
# the numpy variant of the whole chain, as measured; the test holds ten times it
MEASURED_MAX_SVD_POSE_DIFF = 1.4e-12


def pose_of_ref(q, r, linalg):
    o = R.perspective_pose(TS.ref_camera(q["camera"]), [float(v) for v in q["bounds"]], r["choice"], r["h"]["M"], r["f"]["M"], r["inliers"], q["match"].tolist(),
                           q["bearing_1"], q["bearing_2"], S.xy(q["undist_1"]).tolist(), S.xy(q["undist_2"]).tolist(), linalg=linalg)
    return dict(o, choice_is_h=r["choice"] == R.CHOICE_H)


def test_anchor_poses_agree_with_numpys_linear_algebra():
    """The whole chain of every anchor scene -- both RANSACs, the choice, the decomposition of the chosen matrix and find_most_plausible_pose -- by the
    definition and with numpy.linalg.svd / numpy.linalg.inv in the place of every Jacobi and cofactor inverse (the 3 x 3 SVD of K^-1 H K and of
    K^T F K included, under D27 item e's and D24 item c's sign rules): the same status, the same chosen hypothesis (for F up to the order
    the routine's basis of the double singular value gives the four), the same count of valid points and the same triangulated flags for every hypothesis; every hypothesis's rotation and translation, and so the pose, within ten times the measured
    deviation (MEASURED_MAX_SVD_POSE_DIFF)."""
    worst = 0.0
    for name in S.ANCHORS:
        q = SCENES[name]
        a, b = pose_of_ref(q, ref(name), "jacobi"), pose_of_ref(q, ref(name, linalg="svd"), "svd")
        nh = len(a["rots"])
        hyp_dev = lambda i, j: max(np.abs(np.array(a["rots"][i]) - np.array(b["rots"][j])).max(), np.abs(np.array(a["transes"][i]) - np.array(b["transes"][j])).max())
        # H: the singular values of K^-1 H K are distinct and the hypotheses come in one order.  F: the two equal singular values of an essential matrix
        # leave the basis of their plane to the routine, and D24 item c's sign rule on another basis swaps rot_1 with rot_2 and t with -t: the same
        # four hypotheses in another order, so hypothesis j of the variant is held against the one of the definition nearest to it
        perm = list(range(nh)) if a["choice_is_h"] else [min(range(nh), key=lambda i: hyp_dev(i, j)) for j in range(nh)]
        assert sorted(perm) == list(range(nh)) and a["status"] == b["status"], name
        assert (b["hypothesis"] == -1 and a["hypothesis"] == -1) or perm[b["hypothesis"]] == a["hypothesis"], name
        assert all(a["num_valid"][perm[j]] == b["num_valid"][j] and a["hyp_is_triangulated"][perm[j]] == b["hyp_is_triangulated"][j] for j in range(nh)), name
        assert max(a["num_valid"]) > 0, name
        dev = max(hyp_dev(perm[j], j) for j in range(nh))
        dev = max(dev, np.abs(np.array(a["rot"]) - np.array(b["rot"])).max(), np.abs(np.array(a["trans"]) - np.array(b["trans"])).max())
        print(name, "status", a["status"], "hypothesis", a["hypothesis"], "num_valid", a["num_valid"], "max deviation of a hypothesis", dev)
        worst = max(worst, dev)
    print("max deviation over the anchors", worst)
    assert worst <= 10 * MEASURED_MAX_SVD_POSE_DIFF


def rotation_homography(q):
    return K @ q["truth"][0] @ np.linalg.inv(K)                       # no baseline: all three singular values of K^-1 H K are 1


def test_homography_decompose_is_the_restatements_and_holds_the_true_pose():
    rng = np.random.default_rng(3)
    Hs = [truth_matrix(POSE_SCENES[n], R.H) for n in ("planar", "planar_pose")] + [np.array(ref("planar")["h"]["M"]), rotation_homography(SCENES["planar"]),
                                                                                   np.outer([1.0, 2.0, 3.0], [0.5, -1.0, 2.0]), K @ rng.standard_normal((3, 3)) @ np.linalg.inv(K)]
    got = plp.model_homography_decompose(np.array(Hs), K)
    for i, Hm in enumerate(Hs):
        d = R.decompose_h(Hm.tolist(), K.tolist())
        assert bool(got["ok"][i]) == (d is not None), i
        if d is not None:
            assert bits(got["rots"][i]) == bits(np.array(d[0])) and bits(got["transes"][i]) == bits(np.array(d[1])), i
    assert got["ok"].tolist() == [True, True, True, False, True, True]
    for i, n in enumerate(("planar", "planar_pose")):                  # the scene's motion is one of the eight hypotheses
        Rt, tt = POSE_SCENES[n]["truth"]
        errs = [max(np.abs(got["rots"][i][h] - Rt).max(), np.abs(got["transes"][i][h] - tt / np.linalg.norm(tt)).max()) for h in range(8)]
        assert min(errs) <= 1e-5, (n, errs)
        assert all(abs(np.linalg.det(got["rots"][i][h]) - 1.0) <= 1e-5 for h in range(8))


def test_pose_census_and_ground_truth():
    """every PLP_TWO_VIEW_* status, the failed decomposition, and the scenes' motions: the planar scene through H, the cloud scene through F.  The
    bound on the pose is the one tests/test_two_view_pose_cpu.py holds its noisy scenes to against ground truth."""
    seen = {}
    for name, kw in POSE_CASES:
        q = POSE_SCENES[name]
        e, pos, k = pose_inputs(q, **kw)
        got = plp.model_perspective_pose(*pos, **k)
        seen.setdefault(int(got["status"][0]), []).append((name, int(e["choice"][0])))
        if name in ("planar_pose", "cloud_200", "exact"):
            assert got["status"][0] == TR.TV_OK and e["choice"][0] == (R.CHOICE_H if name == "planar_pose" else R.CHOICE_F), name
            Rt, tt = q["truth"]
            rot, tr = angle_rot(got["rot_ref_to_cur"][0], Rt), angle_dir(got["trans_ref_to_cur"][0], tt)
            rot_i, tr_i = independent_pose_error(q, name)
            print(name, "rotation error", rot, "(numpy fit:", rot_i, ") translation direction error", tr, "(numpy fit:", tr_i, ")")
            assert rot <= max(2 * rot_i, 1e-6) and tr <= max(2 * tr_i, 1e-5), name
            tri = got["is_triangulated"][0].astype(bool)
            assert tri.sum() >= 50 and not tri[q["match"] < 0].any()
    q = POSE_SCENES["planar"]
    e, pos, k = pose_inputs(q)
    pos = list(pos)
    pos[1], pos[2] = np.array([R.CHOICE_H], np.uint8), rotation_homography(q)[None]
    got = plp.model_perspective_pose(*pos, **k)
    want = R.pose_expected([pose_ref(q, e, choice=R.CHOICE_H, Hm=rotation_homography(q))], len(q["match"]))
    assert got["status"][0] == R.NO_DECOMPOSITION and all(bits(got[key]) == bits(want[key]) for key in want)
    assert set(seen) == {TR.TV_OK, TR.TV_NO_SOLUTION, TR.TV_TOO_FEW_TRIANGULATED, TR.TV_AMBIGUOUS, TR.TV_SMALL_PARALLAX}, seen
    assert any(c == R.CHOICE_H for n, c in seen[TR.TV_OK]) and any(c == R.CHOICE_F for n, c in seen[TR.TV_OK])


def angle_rot(A, B):
    D = A @ B.T
    return math.atan2(0.5 * float(np.linalg.norm([D[2, 1] - D[1, 2], D[0, 2] - D[2, 0], D[1, 0] - D[0, 1]])), 0.5 * (float(np.trace(D)) - 1.0))


def angle_dir(a, b):
    return math.atan2(float(np.linalg.norm(np.cross(a, b))), float(a @ b))


def independent_pose_error(q, name):
    """as tests/test_two_view_pose_cpu.py holds its perspective and fisheye scenes: the same fit over the inliers of the best hypothesis with
    numpy.linalg.svd / inv in place of D27's routines, decomposed by the restatement; of its poses the one nearest the truth, and its two errors"""
    solver, key = (R.H, "h") if q["kind"] == "planar" else (R.F, "f")
    best = S.run_ref(q, recompute=False)
    pairs = normalized_pairs(q)
    n1, n2 = R.normalize(S.xy(q["undist_1"]).tolist()), R.normalize(S.xy(q["undist_2"]).tolist())
    M, _ = R.fit(solver, [pairs[k] for k in range(len(pairs)) if best[key]["flags"][k]], R.transform(n1), R.transform(n2), "svd")
    rots, transes = R.decompose_h(M, K.tolist()) if solver == R.H else R.decompose_f(M, K.tolist())
    Rt, tt = q["truth"]
    return min(((angle_rot(np.array(r), Rt), angle_dir(np.array(t), tt)) for r, t in zip(rots, transes)), key=sum)


def test_pose_argument_checks_and_the_equirectangular_camera():
    q = SCENES["cloud_64"]
    e, pos, k = pose_inputs(q)
    out = pose_sentinels(R.pose_expected([pose_ref(q, e)], len(q["match"])))
    with pytest.raises(plp.PlpError):
        plp.model_perspective_pose(plp.camera_model(TS.CAMERAS["equirectangular"]), *pos[1:], out=out, img_bounds=q["bounds"])
    with pytest.raises(plp.PlpError):
        plp.model_perspective_pose(*pos, min_num_triangulated=-1, out=out, img_bounds=q["bounds"])
    assert all((v == TR.TV_SENTINEL[key]).all() for key, v in out.items()), "a rejected call wrote an output"
    L = plp.lib()
    assert L.plp_model_perspective_pose_host(None) == -1 and L.plp_model_homography_decompose_host(None, None, 1, None, None, None) == -1


def test_the_initializer_mirror_has_the_references_surface():
    q = POSE_SCENES["planar_pose"]
    cam = plp.camera_model(TS.CAMERAS["perspective"])
    init = plp.perspective_initializer(cam, q["undist_1"], q["bearing_1"], num_ransac_iters=q["iters"], samples_h=q["samples_h"][None], samples_f=q["samples_f"][None])
    assert init.initialize(q["undist_2"], q["bearing_2"], q["match"])
    e, pos, k = pose_inputs(q)
    want = plp.model_perspective_pose(*pos, **k)
    assert bits(init.get_rotation_ref_to_cur()) == bits(want["rot_ref_to_cur"][0]) and bits(init.get_translation_ref_to_cur()) == bits(want["trans_ref_to_cur"][0])
    assert bits(init.get_triangulated_pts()) == bits(want["triangulated_pts"][0]) and init.get_triangulated_flags().tolist() == want["is_triangulated"][0].astype(bool).tolist()
    assert init.initialize(q["undist_2"], q["bearing_2"], q["match"], given_H=(init.ransac["H_21"][0], int(init.ransac["num_inliers_h"][0])))
    assert int(init.ransac["best_iter_h"][0]) == -1 and bits(init.get_rotation_ref_to_cur()) == bits(want["rot_ref_to_cur"][0])


def test_the_solver_classes_decompose_as_the_restatement_does():
    """homography_solver::decompose and fundamental_solver::decompose, static members as in the reference, against the restatement bit for bit"""
    r = ref("planar")
    ok, rots, transes = plp.homography_solver.decompose(np.array(r["h"]["M"]), K, K)
    want = R.decompose_h(r["h"]["M"], K.tolist())
    assert ok and bits(rots) == bits(np.array(want[0])) and bits(transes) == bits(np.array(want[1]))
    assert not plp.homography_solver.decompose(rotation_homography(SCENES["planar"]), K)[0]
    Fm = ref("cloud_200")["f"]["M"]
    ok, rots, transes = plp.fundamental_solver.decompose(np.array(Fm), K, K)
    want = R.decompose_f(Fm, K.tolist())
    assert ok and rots.shape == (4, 3, 3) and bits(rots) == bits(np.array(want[0])) and bits(transes) == bits(np.array(want[1]))
    with pytest.raises(plp.PlpError):
        plp.fundamental_solver.decompose(np.array(Fm), K, 2 * K)
