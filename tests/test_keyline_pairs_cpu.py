"""The CPU restatement of the key-frame pair line triangulation (tests/keyline_pairs_ref.py) on its own: hand-derived cases for every status
code, the two threshold sets, the duplicate rule on hand-made groups, compute_median_depth against numpy.sort, and -- on the scenes the GPU
tests compare the device with (tests/keyline_pairs_scene.py) -- that every branch is reached and that no parallax comparison is a near tie
(DESIGN.md section 5, D8 item 3).  No GPU."""
import collections

import numpy as np
import pytest

import keyline_pairs_ref as KP
import keyline_pairs_scene as S
import stereo_keylines_ref as SK

f32, f64 = np.float32, np.float64
CAM = S.CAM
SF, LS = S.scale_tables()


# ------------------------------------------------------------------------------------------------------------ a two-key-frame fixture
def _kf(P, segs, n_kp=10, setup=KP.MONOCULAR, median=5.0):
    """a key frame that sees the 3-D segments exactly (float-rounded pixels), monocular unless told otherwise"""
    kls = np.zeros(len(segs), S.plp.KL_DTYPE)
    for s, (a, b) in enumerate(segs):
        ua, va, _ = SK.project(CAM, P, a)
        ub, vb, _ = SK.project(CAM, P, b)
        kls[s] = S._keyline(ua, va, ub, vb, 0)
    fn = np.array([S._line_function(k) for k in kls], np.float64).reshape(len(segs), 3)
    return dict(keylines=kls, line_functions=fn, kl_x_right=np.full((len(segs), 2), -1.0, np.float32),
                kp_depths=np.full(n_kp, 5.0, np.float32), pose=P, median_depth=f32(median), lines_3d=None,
                occupied=np.zeros(len(segs), np.uint8))


SEG = (np.array([0.1, -0.3, 5.0]), np.array([0.2, 0.3, 5.0]))      # nearly vertical in the image, 5 m in front of both cameras
P_A = SK.frame_pose(np.eye(3), np.zeros(3))
P_B = SK.frame_pose(np.eye(3), -np.array([0.5, 0.0, 0.0]))         # camera centre (0.5, 0, 0): 5.7 degrees of parallax at 5 m


def _pair(segs=(SEG,), P2=P_B, **kw):
    return _kf(P_A, segs, **kw), _kf(P2, segs, **kw)


def _tri(kf1, kf2, j=0, t=0, setup=KP.MONOCULAR, gaps=None):
    return KP.triangulate(CAM, setup, S.TRUE_BASELINE, SF, LS, S.SCALE_FACTOR, KP.cos_parallax_thr(1.0), kf1, kf2, j, t, gaps)


def _group(kfs, ngh, matches, gates=KP.MAPPING_GATES, setup=KP.MONOCULAR, info=None):
    return KP.triangulate_group(CAM, setup, S.TRUE_BASELINE, SF, LS, S.SCALE_FACTOR, 1.0, gates, kfs, 0, ngh, matches, None, info)


def _m(idx, dist):
    return np.array(idx, np.int32), np.array(dist, np.int32)


# ------------------------------------------------------------------------------------------------------------ one case per status code
def test_created_recovers_the_segment():
    a, b = _pair()
    st, pos, branch = _tri(a, b)
    assert st == KP.CREATED and branch == 1
    # pixels are rounded to float (2^-15 px at u = 330): 5 m / (500 px * 0.5 m baseline) * 5 m * 3e-5 px = 3e-6 m in depth
    assert np.allclose(pos, np.concatenate(SEG), atol=2e-5), pos


def test_gates_in_the_reference_order():
    a, b = _pair()
    g = KP.MAPPING_GATES
    gate = lambda k1, k2, d: KP.gate(k1, k2, d, g["dist_thr"], g["endpoint_thr"], g["angle_thr"])
    assert gate(a["keylines"][0], b["keylines"][0], 49) == KP.CREATED
    assert gate(a["keylines"][0], b["keylines"][0], 50) == KP.GATE_DISTANCE                    # strict, in float
    far = b["keylines"][0].copy()
    far["startPointX"] = a["keylines"][0]["startPointX"] + f32(401.0)                           # same row: 401 px; the end point still matches
    assert gate(a["keylines"][0], far, 10) == KP.GATE_ENDPOINTS
    near = b["keylines"][0].copy()
    near["startPointX"] = a["keylines"][0]["startPointX"] + f32(399.0)
    assert gate(a["keylines"][0], near, 10) == KP.CREATED
    turned = b["keylines"][0].copy()
    turned["angle"] = f32(float(turned["angle"]) - 0.36)                                        # 0.36 rad * 180 / 3.14 = 20.6 > 20
    assert gate(a["keylines"][0], turned, 10) == KP.GATE_ANGLE
    turned["angle"] = f32(float(b["keylines"][0]["angle"]) - 0.34)                              # 19.5 < 20
    assert gate(a["keylines"][0], turned, 10) == KP.CREATED
    both = far.copy()
    both["angle"] = turned["angle"] - f32(0.2)
    assert gate(a["keylines"][0], both, 10) == KP.GATE_ENDPOINTS                               # the end points are reported before the angle
    # a group: no 1-NN, an index outside the neighbour, a far descriptor
    _, _, st, _ = _group([a, b], [1], [_m([-1], [256])])
    assert st[0][0] == KP.GATE_DISTANCE
    _, _, st, _ = _group([a, b], [1], [_m([1], [3])])
    assert st[0][0] == KP.GATE_DISTANCE


def test_occupied_cur_and_ngh():
    a, b = _pair()
    a["occupied"][0] = 1
    b["occupied"][0] = 1
    _, _, st, _ = _group([a, b], [1], [_m([0], [5])])
    assert st[0][0] == KP.OCCUPIED_CUR                                                          # cur is asked first (:564)
    a["occupied"][0] = 0
    m, _, st, occ = _group([a, b], [1], [_m([0], [5])])
    assert st[0][0] == KP.OCCUPIED_NGH and m[0][0] == -1 and occ[0] == 0
    m, _, st, occ = _group([a, b], [1], [_m([0], [5])], gates=KP.INITIALIZER_GATES)            # the initialiser's loop has no such check
    assert st[0][0] == KP.CREATED and m[0][0] == 0 and occ[0] == 1


def test_no_parallax_when_the_centres_coincide():
    a, b = _pair(P2=P_A)
    assert _tri(a, b)[0] == KP.NO_PARALLAX                                                      # cos = 1 is not below cos(1 degree)
    # 1 degree at 5 m is 8.7 cm: 8 cm is too little, 10 cm enough
    for dx, want in ((0.08, KP.NO_PARALLAX), (0.10, KP.CREATED)):
        a, b = _pair(P2=SK.frame_pose(np.eye(3), -np.array([dx, 0.0, 0.0])))
        assert _tri(a, b)[0] == want, dx


def test_too_close_and_too_long_read_key_frame_2s_median():
    a, b = _pair()
    b["median_depth"] = f32(17.0)                                                               # 5.0 / 17 = 0.294 < 0.3
    assert _tri(a, b)[0] == KP.TOO_CLOSE
    b["median_depth"] = f32(16.0)                                                               # 0.3128
    assert _tri(a, b)[0] == KP.CREATED
    a["median_depth"] = f32(1000.0)                                                             # key frame 1's is never read
    assert _tri(a, b)[0] == KP.CREATED
    b["median_depth"] = f32(0.67)                                                               # |ep - sp| = 0.6083; / 0.67 = 0.908 > 0.9
    assert _tri(a, b)[0] == KP.TOO_LONG
    b["median_depth"] = f32(0.68)                                                               # 0.8945
    assert _tri(a, b)[0] == KP.CREATED


def test_depth_negative_disparity():
    a, b = _pair()
    for k in ("startPointX", "endPointX", "pt_x"):
        b["keylines"][0][k] = a["keylines"][0][k] + f32(50.0)                                   # 50 px to the RIGHT of view 1: z = 500 * 0.5 / -50 = -5
    b["line_functions"][0] = S._line_function(b["keylines"][0])
    b["median_depth"] = f32(5.0)
    st, _, branch = _tri(a, b)
    assert st == KP.DEPTH and branch == 1


def test_reprojection_mid_and_end():
    a, b = _pair()
    d = np.array([b["keylines"][0]["endPointX"] - b["keylines"][0]["startPointX"], b["keylines"][0]["endPointY"] - b["keylines"][0]["startPointY"]], np.float64)
    d /= np.linalg.norm(d)
    for shift, want in ((2.5, KP.REPROJ_MID), (2.4, KP.CREATED)):                               # 2.5^2 = 6.25 > 5.99146 > 5.76 = 2.4^2
        b2 = dict(b, keylines=b["keylines"].copy())
        b2["keylines"][0]["pt_x"] += f32(shift * d[0])
        b2["keylines"][0]["pt_y"] += f32(shift * d[1])
        assert _tri(a, b2)[0] == want, shift
    n = np.hypot(b["line_functions"][0][0], b["line_functions"][0][1])
    for shift, want in ((6.1, KP.REPROJ_END), (5.9, KP.CREATED), (-6.1, KP.REPROJ_END)):        # |err| against 5.99146, no square
        b2 = dict(b, line_functions=b["line_functions"].copy())
        b2["line_functions"][0][2] += shift * n
        assert _tri(a, b2)[0] == want, shift
    a2 = dict(a, keylines=a["keylines"].copy())
    a2["keylines"][0]["octave"] = 2                                                             # sigma_sq = 1.44^2: 5.99146 * 2.0736 = 12.4
    a2["line_functions"] = a["line_functions"].copy()
    a2["line_functions"][0][2] += 12.0 * np.hypot(a["line_functions"][0][0], a["line_functions"][0][1])
    assert _tri(a2, b)[0] == KP.CREATED
    a2["line_functions"][0][2] += 1.0 * np.hypot(a["line_functions"][0][0], a["line_functions"][0][1])
    assert _tri(a2, b)[0] == KP.REPROJ_END


def test_scale_factors():
    a, b = _pair()
    a["keylines"][0]["octave"] = 5                                                              # 1.2^5 = 2.49 >= 2.4 = 2 * 1.2 at equal distances
    assert _tri(a, b)[0] == KP.SCALE
    a["keylines"][0]["octave"] = 4                                                              # 2.07
    assert _tri(a, b)[0] == KP.CREATED
    b["keylines"][0]["octave"] = 5                                                              # the other way round: 1 / 2.49
    a["keylines"][0]["octave"] = 0
    assert _tri(a, b)[0] == KP.SCALE


def test_non_finite_exactly_horizontal_key_line():
    seg = (np.array([-0.6, 0.2, 5.0]), np.array([0.5, 0.2, 5.0]))                              # one image row in the identity key frame
    a, b = _pair(segs=(seg,))
    assert a["keylines"][0]["startPointY"] == a["keylines"][0]["endPointY"]
    st, pos, _ = _tri(a, b)
    assert st == KP.NON_FINITE and pos is None                                                  # l1 = 0: l2 / l1 is not finite


def test_kp_depth_range_reads_the_key_points_vector():
    segs = (SEG, (np.array([-0.5, -0.2, 6.0]), np.array([-0.4, 0.3, 6.0])))
    a, b = _pair(segs=segs, n_kp=1)
    for kf in (a, b):
        kf["kl_x_right"][:] = 1.0
        kf["lines_3d"] = np.zeros((2, 6))
    assert _tri(a, b, 0, 0, KP.RGBD)[0] != KP.KP_DEPTH_RANGE
    assert _tri(a, b, 1, 0, KP.RGBD)[0] == KP.KP_DEPTH_RANGE                                   # idx_1 = 1 >= depths_.size() = 1
    assert _tri(a, b, 0, 1, KP.RGBD)[0] == KP.KP_DEPTH_RANGE
    a["kl_x_right"][1] = -1.0                                                                   # not stereo: depths_ is not read for it
    assert _tri(a, b, 1, 0, KP.RGBD)[0] != KP.KP_DEPTH_RANGE


def test_stereo_branches_pick_the_nearer_depth_and_keep_a_zero_row():
    a, b = _pair(P2=SK.frame_pose(np.eye(3), -np.array([0.01, 0.0, 0.0])))                     # 1 cm: less parallax than the 10 cm baseline
    truth = np.concatenate(SEG)
    for kf in (a, b):
        kf["kl_x_right"][:] = 1.0
        kf["lines_3d"] = truth[None].copy()
    a["kp_depths"][0], b["kp_depths"][0] = 4.0, 6.0
    gaps = []
    st, pos, branch = _tri(a, b, setup=KP.RGBD, gaps=gaps)
    assert (st, branch) == (KP.CREATED, 2) and np.array_equal(pos, truth)
    assert [k for k, _ in gaps] == ["rays", "stereo"]
    a["kp_depths"][0] = 7.0
    b["lines_3d"] = truth[None] + 1e-3
    st, pos, branch = _tri(a, b, setup=KP.RGBD)
    assert (st, branch) == (KP.CREATED, 3) and np.array_equal(pos, b["lines_3d"][0])
    b["lines_3d"] = np.zeros((1, 6))                                                            # Vec6_t::Zero(): the checks decide
    st, _, branch = _tri(a, b, setup=KP.RGBD)
    assert (st, branch) == (KP.TOO_CLOSE, 3)
    b["kp_depths"][0] = 7.0                                                                     # equal depths: neither is smaller
    gaps = []
    assert _tri(a, b, setup=KP.RGBD, gaps=gaps)[0] == KP.NO_PARALLAX
    assert gaps[-1] == ("stereo_equal_inputs", 0.0)


# ------------------------------------------------------------------------------------------------------------ thresholds, duplicates
def test_mapping_and_initialiser_thresholds_differ_on_the_same_pair():
    a, b = _pair()
    b["keylines"][0]["angle"] = f32(float(b["keylines"][0]["angle"]) - 0.2)                     # 11.5 degrees: inside 20, outside 5
    for gates, want in ((KP.MAPPING_GATES, KP.CREATED), (KP.INITIALIZER_GATES, KP.GATE_ANGLE)):
        assert _group([a, b], [1], [_m([0], [10])], gates=gates)[2][0][0] == want
    a, b = _pair()
    for gates, want in ((KP.MAPPING_GATES, KP.CREATED), (KP.INITIALIZER_GATES, KP.GATE_DISTANCE)):
        assert _group([a, b], [1], [_m([0], [40])], gates=gates)[2][0][0] == want
    a, b = _pair(P2=SK.frame_pose(np.eye(3), -np.array([2.5, 0.0, 0.0])))                      # 250 px of disparity
    for gates, want in ((KP.MAPPING_GATES, KP.CREATED), (KP.INITIALIZER_GATES, KP.GATE_ENDPOINTS)):
        assert _group([a, b], [1], [_m([0], [10])], gates=gates)[2][0][0] == want


def test_two_queries_with_one_train_index():
    a, b = _pair()
    a = dict(a, keylines=np.repeat(a["keylines"], 2), line_functions=np.repeat(a["line_functions"], 2, 0),
             kl_x_right=np.repeat(a["kl_x_right"], 2, 0), occupied=np.zeros(2, np.uint8))
    broken = a["line_functions"].copy()
    # the first fails its geometry, the second succeeds: the second creates the landmark
    a1 = dict(a, line_functions=broken.copy())
    a1["line_functions"][0][2] += 50 * np.hypot(*broken[0][:2])
    info = []
    m, pw, st, occ = _group([a1, b], [1], [_m([0, 0], [5, 6])], info=info)
    assert list(st[0]) == [KP.REPROJ_END, KP.CREATED] and list(m[0]) == [-1, 0] and list(occ) == [0, 1]
    assert not pw[0][0].any() and pw[0][1].any()
    # the reverse: the first creates it, the second finds the neighbour's slot taken by an earlier winner of the same pair
    a2 = dict(a, line_functions=broken.copy())
    a2["line_functions"][1][2] += 50 * np.hypot(*broken[1][:2])
    info = []
    m, _, st, occ = _group([a2, b], [1], [_m([0, 0], [5, 6])], info=info)
    assert list(st[0]) == [KP.CREATED, KP.OCCUPIED_NGH] and list(m[0]) == [0, -1] and list(occ) == [1, 0]
    assert (1, "earlier winner") in info[0]
    # without the duplicate check both are created
    m, _, st, occ = _group([a, b], [1], [_m([0, 0], [5, 6])], gates=KP.INITIALIZER_GATES)
    assert list(st[0]) == [KP.CREATED, KP.CREATED] and list(occ) == [1, 1]


def test_a_query_taken_by_the_first_neighbour_is_skipped_at_the_second():
    a, b = _pair()
    c = _kf(SK.frame_pose(np.eye(3), -np.array([-0.4, 0.1, 0.0])), (SEG,))
    info = []
    m, _, st, occ = _group([a, b, c], [1, 2], [_m([0], [5]), _m([0], [7])], info=info)
    assert st[0][0] == KP.CREATED and st[1][0] == KP.OCCUPIED_CUR and m[1][0] == -1 and occ[0] == 1
    assert info[1] == [(0, "earlier neighbour")]
    assert c["occupied"][0] == 0 and b["occupied"][0] == 0                                      # the inputs are not modified
    m, _, st, _ = _group([a, b, c], [2, 1], [_m([0], [7]), _m([0], [5])])                       # the order of the neighbours decides
    assert st[0][0] == KP.CREATED and st[1][0] == KP.OCCUPIED_CUR


# ------------------------------------------------------------------------------------------------------------ median depth
@pytest.mark.parametrize("n", [1, 2, 3, 8, 9, 250])
@pytest.mark.parametrize("abs_flag", [False, True])
def test_median_depth_against_numpy_sort(n, abs_flag):
    rng = np.random.default_rng(100 + n)
    R = S._rot(rng.normal(size=3) * 0.4)
    P = SK.frame_pose(R, rng.normal(size=3))
    X = rng.normal(size=(n + 5, 3)) * 4
    valid = np.ones(n + 5, np.uint8)
    valid[rng.permutation(n + 5)[:5]] = 0
    med, cnt = KP.median_depth(P, X, valid, abs_flag)
    z = np.array([((P[6] * x[0] + P[7] * x[1]) + P[8] * x[2]) + f64(f32(P[11])) for x in X[valid != 0]])
    d = np.sort((np.abs(z) if abs_flag else z).astype(np.float32))
    assert cnt == n and med == d[(n - 1) // 2] and med.dtype == np.float32
    if n % 2 == 0:
        assert med == d[n // 2 - 1]                                                             # the LOWER of the two middle elements


def test_median_depth_float_translation_and_empty():
    P = SK.frame_pose(np.eye(3), np.array([0.0, 0.0, 0.1]))                                     # 0.1 is not a float: (float)0.1 = 0.1 + 1.49e-9
    y = f32(1.1)
    half_way = (f64(y) + f64(np.nextafter(y, f32(2)))) / 2                                      # between two neighbouring floats
    X = np.array([[0.0, 0.0, half_way - 0.1 - 0.7e-9]])                                         # + 0.1: just below it, + (float)0.1: just above
    assert f32(X[0][2] + 0.1) == y and f32(X[0][2] + f64(f32(0.1))) == np.nextafter(y, f32(2))  # rounding t_z first changes the float returned
    med, cnt = KP.median_depth(P, X, None, True)
    assert cnt == 1 and med == np.nextafter(y, f32(2))
    assert KP.median_depth(P, X, np.zeros(1, np.uint8), True) == (f32(0.0), 0)
    assert KP.median_depth(P, np.zeros((0, 3)), None, False) == (f32(0.0), 0)


# ------------------------------------------------------------------------------------------------------------ the scenes of the GPU tests
def test_scenes_reach_every_branch_and_have_no_near_tie():
    tot, causes, branches = collections.Counter(), collections.Counter(), collections.Counter()
    gaps_all, equal = [], 0
    for name, _, setup, gates in S.SCENES:
        scene, groups, matches, _, (om, op, os_, oc), gaps, info = S.scene_case(name)
        assert scene["F"] >= 6 and len(groups) >= 8 and all(3 <= len(n) <= 10 for _, n in groups)
        assert any(len(kf["keylines"]) == 0 for kf in scene["kfs"])
        tot.update(int(v) for v in os_.ravel() if v != S.SENT_U8)
        for notes in info:
            for _, cause in notes:
                (branches if cause.startswith("branch") else causes)[cause] += 1
        gaps_all += [g for k, g in gaps if k != "stereo_equal_inputs"]
        equal += sum(1 for k, _ in gaps if k == "stereo_equal_inputs")
        # written exactly where the contract says: slots below cur's count
        p = 0
        for kf1, ngh in groups:
            n = len(scene["kfs"][kf1]["keylines"])
            for _ in ngh:
                assert (os_[p, :n] != S.SENT_U8).all() and (os_[p, n:] == S.SENT_U8).all()
                assert ((om[p, :n] >= 0) == (os_[p, :n] == KP.CREATED)).all()
                p += 1
    print({KP.STATUS_NAMES[k]: v for k, v in sorted(tot.items())}, dict(causes), dict(branches))
    for code in range(15):
        if code in (KP.NON_FINITE, KP.KP_DEPTH_RANGE):
            continue                                                                            # directed cases (tests/test_gpu_keyline_pairs.py)
        assert tot[code] >= (100 if code == KP.CREATED else 5), (KP.STATUS_NAMES[code], tot[code])
    assert causes["earlier winner"] >= 5 and causes["earlier neighbour"] >= 5, causes
    assert all(branches[f"branch {b}"] >= 10 for b in (1, 2, 3)), branches
    # D8 item 3: the only comparisons a libm can change.  The smallest relative gap between the two cosines, over every slot of every scene
    # whose sides do not come from bit-identical inputs, is seven orders above an f64 cos / atan2 discrepancy.
    smallest = min(gaps_all)
    print(f"parallax comparisons: {len(gaps_all)}, {equal} more with bit-identical inputs; smallest relative gap {smallest:.3e}")
    assert len(gaps_all) >= 1000 and smallest >= 1e-9, smallest


def test_directed_scenes_reach_non_finite_and_kp_depth_range():
    scene = S.make_scene(31, KP.MONOCULAR, extra_horizontal=True)
    groups = [(0, [2, 4, 6])]
    _, _, os_, _ = S.run_ref(scene, groups, S.match_all(scene, groups), KP.INITIALIZER_GATES)
    assert (os_ == KP.NON_FINITE).sum() >= 3
    scene = S.make_scene(32, KP.RGBD)
    groups = [(4, [0, 2, 5]), (2, [4, 6])]
    _, _, os_, _ = S.run_ref(scene, groups, S.match_all(scene, groups), KP.INITIALIZER_GATES)
    assert (os_ == KP.KP_DEPTH_RANGE).sum() >= 5


def test_created_lines_lie_on_the_true_segment():
    """accuracy, apart from parity: unperturbed projections (float-rounded pixels), correct pairings, two-camera branch"""
    worst = 0.0
    for seed, setup in ((41, KP.MONOCULAR), (42, KP.RGBD)):
        scene = S.make_scene(seed, setup, perturb=0.0, occupied_rate=0.0)
        groups = S.make_groups(seed, scene["F"])
        info = []
        om, op, os_, _ = S.run_ref(scene, groups, S.match_all(scene, groups), KP.INITIALIZER_GATES, info=info)
        p, seen = 0, 0
        for kf1, ngh in groups:
            for kf2 in ngh:
                br = {j: c for j, c in info[p] if c.startswith("branch")}
                for j in np.nonzero(om[p] >= 0)[0]:
                    a, b = scene["segments"][scene["seg"][kf1][j]]
                    if scene["seg"][kf2][om[p, j]] != scene["seg"][kf1][j] or br[j] != "branch 1":
                        continue
                    d = (b - a) / np.linalg.norm(b - a)
                    for e in (op[p, j, :3], op[p, j, 3:]):
                        worst = max(worst, np.linalg.norm(np.cross(e - a, d)))
                    seen += 1
                p += 1
        assert seen >= 100
    print(f"largest distance of a created end point from its true line: {worst:.3e} m")
    # measured maximum of the restatement on these two scenes: 9.22e-05 m (pixels rounded to float, key frames up to 13 m from the segment,
    # parallax down to one degree); the bound is ten times that
    assert worst < 9.22e-4


