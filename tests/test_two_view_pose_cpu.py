"""bearing_vector::reconstruct_with_E without a GPU (DESIGN.md section 5, D24 items c, f, g): the host build of csrc/two_view.hpp
(plp.model_essential_decompose, model_check_pose, model_two_view_pose) against the plain-Python restatement tests/two_view_ref.py, bit for bit, on
every pose scene of tests/two_view_scene.py for all three cameras and every output over sentinel-filled arrays; the census of statuses and of
the `continue`s of check_pose; the chosen pose against the scenes' ground truth; the argument checks and the mirror class."""
import ctypes as C
import math

import numpy as np
import pytest

import two_view_ref as R
import two_view_scene as S
from plp import plp

SCENES = S.pose_scenes()
SCENES["near_rotation"] = S.pose_problem(457, 150, "perspective", noise=1e-4, kind="near_rotation")
_cache = {}


def bits(a):
    return np.ascontiguousarray(a).tobytes()


def camera(q):
    return plp.camera_model(S.CAMERAS[q["camera"]])


def ransac(name):
    """the RANSAC's result of a scene by the host build (tests/test_two_view_cpu.py holds it to the restatement), computed once"""
    if name not in _cache:
        q = SCENES[name]
        _cache[name] = plp.model_essential_ransac(q["bearing_1"][None], q["bearing_2"][None], q["match"][None], iters=q["iters"], samples=q["samples"][None])
    return _cache[name]


def kps(a):
    return [(float(k["x"]), float(k["y"])) for k in a]


def ref_pose(name, depth_is_positive=False, **kw):
    key = (name, depth_is_positive, tuple(sorted(kw.items())))
    if key not in _cache:
        q, e = SCENES[name], ransac(name)
        _cache[key] = R.two_view_pose(S.ref_camera(q["camera"]), [float(x) for x in q["bounds"]], e["E_21"][0].tolist(), e["inliers"][0].tolist(), q["match"].tolist(),
                                      q["bearing_1"], q["bearing_2"], kps(q["undist_1"]), kps(q["undist_2"]), depth_is_positive=depth_is_positive,
                                      in_status=int(e["status"][0]), **kw)
    return _cache[key]


def model_pose(name, depth_is_positive=False, out=None, **kw):
    q, e = SCENES[name], ransac(name)
    return plp.model_two_view_pose(camera(q), e["E_21"], e["inliers"], q["match"][None], q["bearing_1"][None], q["bearing_2"][None], q["undist_1"][None],
                                   q["undist_2"][None], depth_is_positive=depth_is_positive, in_status=e["status"], img_bounds=q["bounds"], out=out, **kw)


# ---------------------------------------------------------------------------------------------------------------- host build == restatement
@pytest.mark.parametrize("name", sorted(SCENES))
def test_decomposition_is_the_restatements(name):
    E = ransac(name)["E_21"][0]
    rots, transes = R.decompose(E.tolist())
    got = plp.model_essential_decompose(E)
    if E.any():
        assert bits(got["rots"]) == bits(np.array(rots)) and bits(got["transes"]) == bits(np.array(transes))
    else:                                                                  # the zero matrix of a problem without a solution: 0 / 0, a NaN whose sign is nobody's
        assert np.array_equal(got["rots"], np.array(rots), equal_nan=True) and np.array_equal(got["transes"], np.array(transes), equal_nan=True)
    if E.any():                                                            # four proper rotations, unit translations, [t]x R = U diag(1, 1, 0) V^T up to sign
        for h in range(4):
            Rm, t = got["rots"][h], got["transes"][h]
            assert abs(np.linalg.det(Rm) - 1.0) < 1e-9 and np.abs(Rm @ Rm.T - np.eye(3)).max() < 1e-9 and abs(np.linalg.norm(t) - 1.0) < 1e-12
            tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
            Un, _, Vtn = np.linalg.svd(E)                                  # E with its two singular values made equal, by an independent routine
            F, En = tx @ Rm, Un @ np.diag([1.0, 1.0, 0.0]) @ Vtn
            F, En = F / np.linalg.norm(F), En / np.linalg.norm(En)
            assert min(np.abs(F - En).max(), np.abs(F + En).max()) < 1e-9


@pytest.mark.parametrize("depth_is_positive", [False, True])
@pytest.mark.parametrize("name", sorted(SCENES))
def test_check_pose_is_the_restatements_for_every_hypothesis(name, depth_is_positive):
    q, e = SCENES[name], ransac(name)
    if int(e["status"][0]) != R.OK:
        return test_no_solution_writes_zeros()
    rots, transes = R.decompose(e["E_21"][0].tolist())
    for h in range(4):
        want = R.check_pose(S.ref_camera(q["camera"]), [float(x) for x in q["bounds"]], rots[h], transes[h], e["inliers"][0].tolist(), q["match"].tolist(),
                            q["bearing_1"], q["bearing_2"], kps(q["undist_1"]), kps(q["undist_2"]), depth_is_positive=depth_is_positive)
        got = plp.model_check_pose(camera(q), rots[h], transes[h], e["inliers"][0], q["match"], q["bearing_1"], q["bearing_2"], q["undist_1"], q["undist_2"],
                                   depth_is_positive=depth_is_positive, img_bounds=q["bounds"])
        assert got["num_valid"] == want["num_valid"] and bits(got["parallax_deg"]) == bits(np.float32(want["parallax_deg"])), (name, h)
        assert got["code"].tolist() == want["code"] and got["is_triangulated"].tolist() == want["is_triangulated"] and bits(got["pts"]) == bits(np.array(want["pts"]))


@pytest.mark.parametrize("depth_is_positive", [False, True])
@pytest.mark.parametrize("name", sorted(SCENES))
def test_pose_entry_is_the_restatements_on_every_output(name, depth_is_positive):
    r = ref_pose(name, depth_is_positive)
    want = R.tv_expected([r], len(SCENES[name]["match"]))
    got = model_pose(name, depth_is_positive, out={k: np.full_like(v, R.TV_SENTINEL[k]) for k, v in want.items()})
    for k in want:
        assert bits(got[k]) == bits(want[k]), (name, k)


def test_batched_ragged_problems_with_counts_are_the_restatements():
    names = ["fisheye_200", "few", "all_mismatched", "fisheye_64"]
    qs = [dict(SCENES[n], iters=8, samples=SCENES[n]["samples"][:8]) for n in names]
    a = S.pose_pack(qs)
    e = plp.model_essential_ransac(a["bearing_1"], a["bearing_2"], a["match"], iters=16, seed=3, counts_1=a["counts_1"], counts_2=a["counts_2"])
    cam = S.ref_camera("fisheye")
    b = [float(x) for x in S.bounds(cam)]
    rs = [R.two_view_pose(cam, b, e["E_21"][p].tolist(), e["inliers"][p].tolist(), a["match"][p].tolist(), a["bearing_1"][p], a["bearing_2"][p], kps(a["undist_1"][p]),
                          kps(a["undist_2"][p]), in_status=int(e["status"][p]), count_2=int(a["counts_2"][p])) for p in range(len(qs))]
    want = R.tv_expected(rs, a["match"].shape[1], a["counts_1"])
    got = plp.model_two_view_pose(plp.camera_model(S.CAMERAS["fisheye"]), e["E_21"], np.where(np.arange(a["match"].shape[1])[None] < a["counts_1"][:, None], e["inliers"], 1),
                                  a["match"], a["bearing_1"], a["bearing_2"], a["undist_1"], a["undist_2"], in_status=e["status"], counts_1=a["counts_1"],
                                  counts_2=a["counts_2"], img_bounds=S.bounds(cam), out={k: np.full_like(v, R.TV_SENTINEL[k]) for k, v in want.items()})
    for k in want:
        assert bits(got[k]) == bits(want[k]), k


# ---------------------------------------------------------------------------------------------------------------- the census
def test_every_status_and_every_continue_of_check_pose_is_reached():
    statuses, codes = set(), set()
    for name in SCENES:
        for dip in (False, True):
            r = ref_pose(name, dip)
            statuses.add(r["status"])
            for c in r["codes"]:
                codes |= set(c)
    # :158-161, a triangulation that is not finite: a zero bearing makes the 2 x 2 matrix singular
    q = SCENES["exact"]
    b1 = q["bearing_1"].copy()
    s0 = int(np.flatnonzero(q["match"] >= 0)[0])
    b1[s0] = 0.0
    Rt, tt = q["truth"]
    inl = (q["match"] >= 0).astype(np.uint8)
    got = plp.model_check_pose(camera(q), Rt, tt, inl, q["match"], b1, q["bearing_2"], q["undist_1"], q["undist_2"], img_bounds=q["bounds"])
    want = R.check_pose(S.ref_camera(q["camera"]), [float(x) for x in q["bounds"]], Rt.tolist(), tt.tolist(), inl.tolist(), q["match"].tolist(), b1, q["bearing_2"],
                        kps(q["undist_1"]), kps(q["undist_2"]))
    assert got["code"].tolist() == want["code"] and want["code"][s0] == R.NOT_FINITE and got["num_valid"] == want["num_valid"] == 149
    codes |= set(want["code"])
    assert statuses == {R.TV_OK, R.TV_NO_SOLUTION, R.TV_TOO_FEW_TRIANGULATED, R.TV_AMBIGUOUS, R.TV_SMALL_PARALLAX}, statuses
    assert codes == set(range(10)), codes                                   # 0: no inlier match; 1 .. 7: the continues of :158-218; 8, 9: valid


def test_the_special_scenes_end_where_they_must():
    # a rotation with a twentieth of the baseline: one hypothesis explains the matches, and its parallax is too small.  Without any baseline the sign
    # of a triangulated depth is the noise's, the matches split between (R, t) and (R, -t), and the reference leaves at :103 first
    assert ref_pose("near_rotation")["status"] in (R.TV_SMALL_PARALLAX, R.TV_TOO_FEW_TRIANGULATED)
    assert ref_pose("rotation")["status"] in (R.TV_SMALL_PARALLAX, R.TV_TOO_FEW_TRIANGULATED, R.TV_AMBIGUOUS)
    r = ref_pose("mirrored")
    assert r["status"] == R.TV_AMBIGUOUS and sorted(r["num_valid"])[2] > 0.8 * max(r["num_valid"])
    r = ref_pose("few")
    assert r["status"] == R.TV_TOO_FEW_TRIANGULATED and 0 < max(r["num_valid"]) < 50
    assert ref_pose("few", min_num_triangulated=20)["status"] == R.TV_OK
    assert ref_pose("all_mismatched")["status"] == R.TV_NO_SOLUTION
    assert ref_pose("exact")["status"] == R.TV_OK and ref_pose("exact", parallax_deg_thr=30.0)["status"] == R.TV_SMALL_PARALLAX


def test_no_solution_writes_zeros():
    got = model_pose("all_mismatched")
    assert got["status"][0] == R.TV_NO_SOLUTION and got["hypothesis"][0] == -1
    assert not any(got[k].any() for k in ("rot_ref_to_cur", "trans_ref_to_cur", "num_valid", "parallax_deg", "triangulated_pts", "is_triangulated", "hyp_is_triangulated"))


# ---------------------------------------------------------------------------------------------------------------- ground truth
def angle_between_rotations(A, B):
    """the angle of A B^T from its skew part and its trace: exact for small angles, where acos of the trace alone is not"""
    D = A @ B.T
    return math.atan2(0.5 * float(np.linalg.norm([D[2, 1] - D[1, 2], D[0, 2] - D[2, 0], D[1, 0] - D[0, 1]])), 0.5 * (float(np.trace(D)) - 1.0))


def angle_between_directions(a, b):
    return math.atan2(float(np.linalg.norm(np.cross(a, b))), float(a @ b))


def independent_pose(q, inliers, truth):
    """the eight-point fit of the same inliers and its decomposition by numpy.linalg.svd alone; of the four poses the one nearest the truth"""
    slots = np.flatnonzero(inliers)
    E = np.array(R.compute_E_21(q["bearing_1"][slots].tolist(), q["bearing_2"][q["match"][slots]].tolist(), "svd")[0])
    U, _, Vt = np.linalg.svd(E)
    W = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    cands = []
    for Rm in (U @ W @ Vt, U @ W.T @ Vt):
        Rm = Rm * np.sign(np.linalg.det(Rm))
        for t in (U[:, 2], -U[:, 2]):
            cands.append((Rm, t))
    return min(cands, key=lambda c: angle_between_rotations(c[0], truth[0]) + angle_between_directions(c[1], truth[1]))


@pytest.mark.parametrize("model", S.MODELS)
@pytest.mark.parametrize("noise", [0.0, 5e-4, 1e-3])
def test_chosen_pose_against_ground_truth(model, noise):
    """200 true matches, the refit over the inliers of the best hypothesis; the rotation angle error and the angle between the translation directions.
    Noise-free: both within 1e-9.  With bearing noise sigma (radians) on the equirectangular camera, whose bearings cover the sphere, the
    translation direction comes from N = 200 epipolar constraints over a parallax p >= 3 degrees = 0.052, an error of the order
    sigma / (p sqrt(N)), and the rotation's is of the order sigma / sqrt(N); both are held to ten times that.  On the perspective (22 degrees) and
    fisheye (48 degrees) cameras the linear eight-point fit couples rotation and sideways translation, and the reference's rule of the greatest
    score keeps a hypothesis with fewer inliers to refit over; no bound in sigma alone holds for that (measured: perspective 2.9e-3 / 2.5e-2 rad
    at sigma 5e-4, 1.1e-2 / 1.2e-1 at 1e-3; fisheye 1.1e-3 / 7.8e-3 and 2.1e-3 / 1.7e-2): there the
    pose is held to what the same fit gives with numpy.linalg.svd in place of D24's routines -- twice that routine's own error against the
    truth -- and, on every camera, to that routine's pose itself within 1e-6 rad (the matrices agree within 5.8e-10, test_two_view_cpu.py)."""
    q = S.pose_problem(600 + S.MODELS.index(model), 200, model, n_slots=210, noise=noise, iters=6)
    e = plp.model_essential_ransac(q["bearing_1"][None], q["bearing_2"][None], q["match"][None], iters=6, samples=q["samples"][None])
    got = plp.model_two_view_pose(camera(q), e["E_21"], e["inliers"], q["match"][None], q["bearing_1"][None], q["bearing_2"][None], q["undist_1"][None],
                                  q["undist_2"][None], in_status=e["status"], img_bounds=q["bounds"])
    assert got["status"][0] == R.TV_OK and got["is_triangulated"][0].sum() >= 150
    Rt, tt = q["truth"]
    Rg, tg = got["rot_ref_to_cur"][0], got["trans_ref_to_cur"][0]
    rot, tr = angle_between_rotations(Rg, Rt), angle_between_directions(tg, tt)
    e0 = plp.model_essential_ransac(q["bearing_1"][None], q["bearing_2"][None], q["match"][None], iters=6, samples=q["samples"][None], recompute=False)
    Ri, ti = independent_pose(q, e0["inliers"][0], q["truth"])            # the refit runs over the inliers of the best hypothesis (:109-116)
    rot_i, tr_i = angle_between_rotations(Ri, Rt), angle_between_directions(ti, tt)
    print(model, noise, "rotation error", rot, "(numpy:", rot_i, ") translation direction error", tr, "(numpy:", tr_i, ")")
    assert angle_between_rotations(Rg, Ri) <= 1e-6 and angle_between_directions(tg, ti) <= 1e-6
    if noise == 0.0:
        assert rot <= 1e-9 and tr <= 1e-9
    elif model == "equirectangular":
        assert rot <= 10 * noise / math.sqrt(200) and tr <= 10 * noise / (0.052 * math.sqrt(200))
    else:
        assert rot <= 2 * rot_i and tr <= 2 * tr_i


# ---------------------------------------------------------------------------------------------------------------- arguments, mirror class
def test_every_invalid_argument_line_of_the_header():
    L = plp.lib()
    q, e = SCENES["perspective_64"], ransac("perspective_64")
    a = S.pose_pack([q])
    n_cap, m_cap = a["match"].shape[1], a["bearing_2"].shape[1]
    o = {k: np.zeros((1,) + shape(n_cap), dt) for k, (shape, dt, _) in plp.TWO_VIEW_OUTPUTS.items()}
    P = lambda v: v.ctypes.data
    inl = np.ascontiguousarray(e["inliers"])
    E = np.ascontiguousarray(e["E_21"])

    def args(**over):
        f = dict(P=1, n_cap=n_cap, m_cap=m_cap, min_num_triangulated=50, parallax_deg_thr=1.0, reproj_err_thr=4.0, depth_is_positive=0)
        ptr = dict(counts_1=P(a["counts_1"]), counts_2=P(a["counts_2"]), in_status=P(e["status"]), E_21=P(E), inliers=P(inl), match=P(a["match"]),
                   bearing_1=P(a["bearing_1"]), bearing_2=P(a["bearing_2"]), undist_1=P(a["undist_1"]), undist_2=P(a["undist_2"]))
        ptr.update({"out_" + k: P(v) for k, v in o.items()})
        for k, v in over.items():
            (f if k in f else ptr)[k] = v
        return plp.two_view_args(camera(q), f, ptr, q["bounds"])
    run = lambda s: L.plp_model_two_view_pose_host(C.byref(s))
    assert run(args()) == 1 and int(o["status"][0]) == int(ref_pose("perspective_64")["status"])
    assert L.plp_model_two_view_pose_host(None) == -1
    bad = [dict(P=-1), dict(n_cap=-1), dict(m_cap=-1), dict(min_num_triangulated=-1), dict(n_cap=8193), dict(P=65536)]
    bad += [{k: None} for k in ("E_21", "inliers", "match", "bearing_1", "bearing_2", "undist_1", "undist_2", "out_status", "out_rot_ref_to_cur",
                                "out_trans_ref_to_cur", "out_hypothesis", "out_num_valid", "out_parallax_deg", "out_triangulated_pts", "out_is_triangulated")]
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
    assert run(args(P=0)) == 0 and run(args(n_cap=0)) == 1 and all(np.array_equal(o[k], before[k]) for k in o)
    assert run(args(out_hyp_is_triangulated=None, counts_1=None, counts_2=None, in_status=None)) == 1
    assert L.plp_model_essential_decompose_host(None, 1, None, None) == -1 and L.plp_model_essential_decompose_host(None, 0, None, None) == 0
    assert L.plp_model_check_pose_host(None, None, None, None, None, None, None, None) == -1


def test_the_mirror_class_has_the_references_surface():
    q = SCENES["perspective_200"]
    init = plp.bearing_vector_initializer(camera(q), q["undist_1"], q["bearing_1"], num_ransac_iters=q["iters"], samples=q["samples"][None])
    assert init.initialize(q["undist_2"], q["bearing_2"], q["match"]) is True
    want = ref_pose("perspective_200")
    assert bits(init.get_rotation_ref_to_cur()) == bits(np.array(want["rot"])) and bits(init.get_translation_ref_to_cur()) == bits(np.array(want["trans"]))
    assert bits(init.get_triangulated_pts()) == bits(np.array(want["pts"])) and init.get_triangulated_flags().tolist() == [bool(v) for v in want["is_triangulated"]]
    q = SCENES["all_mismatched"]
    bad = plp.bearing_vector_initializer(camera(q), q["undist_1"], q["bearing_1"], num_ransac_iters=q["iters"], samples=q["samples"][None])
    assert bad.initialize(q["undist_2"], q["bearing_2"], q["match"]) is False and not bad.get_rotation_ref_to_cur().any()
    for name in ("initialize", "get_rotation_ref_to_cur", "get_translation_ref_to_cur", "get_triangulated_pts", "get_triangulated_flags"):
        assert callable(getattr(plp.bearing_vector_initializer, name))
