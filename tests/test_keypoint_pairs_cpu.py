"""The key-frame pair point triangulation without a GPU: the shipped null-vector code against the restatement's
Python Jacobi bit for bit, the restatement against LAPACK's SVD on every slot of every scene, every status reached, no near tie in a
comparison the GPU decides with its own arithmetic, and the pair geometry against ground truth."""
import functools

import numpy as np
import pytest

import keypoint_pairs_ref as KR
import keypoint_pairs_scene as S
from plp import plp

# The largest relative difference of pos_w between the Jacobi and numpy.linalg.svd (OpenBLAS LAPACK dgesdd) over the 2 646 CREATED slots of
# the scenes, measured where this file was written: 8.96e-14.  The bound leaves 16 x for another LAPACK or libm.
MEASURED_MAX_REL_POS_DIFF = 8.96e-14
POS_BOUND = 16 * MEASURED_MAX_REL_POS_DIFF
GATE_GAP = 1e-9                                                 # the relative gap every dependent comparison keeps (D8 item 3, D10)


@functools.lru_cache(maxsize=None)
def scene_run(si):
    setup, model = S.SETUPS[si]
    sc = S.make_scene(100 + si, setup, model)
    pairs = S.default_pairs(sc)
    mq, qf = S.make_matches(sc, pairs, 200 + si)
    skip, epi, base = S.reference_geometry(sc, pairs)
    gaps, infos = [], []
    jac = S.reference_pairs(sc, pairs, mq, qf, skip, gaps=gaps, infos=infos)
    svd = S.reference_pairs(sc, pairs, mq, qf, skip, null=KR.null_vector4_svd)
    return dict(scene=sc, pairs=pairs, mq=mq, qf=qf, skip=skip, epi=epi, base=base, jac=jac, svd=svd, gaps=gaps, infos=infos)


ALL = range(len(S.SETUPS))


def _scene_matrices():
    return [i["matrix"] for si in ALL for inf in scene_run(si)["infos"] for _, _, _, i in inf if i.get("branch") == 1]


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def test_null_vector_host_build_equals_the_python_jacobi_bit_for_bit():
    rng = np.random.default_rng(7)
    scene = _scene_matrices()
    assert len(scene) > 2000
    mats = [np.array(m, np.float64) for m in scene]
    mats += [rng.normal(size=16) for _ in range(300)]
    mats += [rng.normal(size=16) * 10.0 ** rng.uniform(-150, 150) for _ in range(100)]
    # degenerate: rank 2, rank 1, zero, equal columns, a zero column, the identity, non-finite entries
    mats += [(rng.normal(size=(4, 2)) @ rng.normal(size=(2, 4))).ravel() for _ in range(20)]
    mats += [np.outer(rng.normal(size=4), rng.normal(size=4)).ravel() for _ in range(10)]
    mats.append(np.zeros(16))
    mats.append(np.ones(16))
    eq = rng.normal(size=(4, 4)); eq[:, 2] = eq[:, 0]; mats.append(eq.ravel())
    zc = rng.normal(size=(4, 4)); zc[:, 1] = 0.0; mats.append(zc.ravel())
    mats.append(np.eye(4).ravel())
    bad = rng.normal(size=16); bad[5] = np.nan; mats.append(bad)
    bad = rng.normal(size=16); bad[9] = np.inf; mats.append(bad)
    v, sw = plp.model_null_vector4(np.array(mats).reshape(-1, 4, 4))
    for i, m in enumerate(mats):
        pv, ps = KR.null_vector4(m)
        assert ps == sw[i] and np.array_equal(_bits(pv), _bits(v[i])), (i, m, pv, v[i], ps, sw[i])
    n = len(scene)
    assert sw[:n].max() < KR.NULL4_SWEEP_LIMIT and sw[:n].max() <= 6, sw[:n].max()      # the limit is never reached on scene matrices
    # the vector is a null vector: |A v| is the smallest singular value, up to rounding
    for i in list(range(0, n, 97)) + list(range(n, n + 300, 13)):
        A = np.array(mats[i]).reshape(4, 4)
        smin = np.linalg.svd(A, compute_uv=False)[3]
        assert abs(np.linalg.norm(A @ v[i]) - smin) <= 1e-13 * np.linalg.norm(A), i
        assert abs(np.linalg.norm(v[i]) - 1.0) < 1e-14
    single, s1 = plp.model_null_vector4(np.array(mats[0]).reshape(4, 4))
    assert np.array_equal(_bits(single), _bits(v[0])) and s1 == sw[0]


def test_ties_go_to_the_lowest_index():
    v, sw = plp.model_null_vector4(np.zeros((4, 4)))
    assert sw == 0 and v.tolist() == [1.0, 0.0, 0.0, 0.0]
    A = np.diag([1.0, 0.0, 2.0, 0.0])
    v, sw = plp.model_null_vector4(A)
    assert sw == 0 and v.tolist() == [0.0, 1.0, 0.0, 0.0]


@pytest.mark.parametrize("si", ALL)
def test_svd_in_place_of_the_jacobi_gives_the_same_status_on_every_slot(si):
    r = scene_run(si)
    (_, pos_j, st_j, _, _), (_, pos_s, st_s, _, _) = r["jac"], r["svd"]
    assert np.array_equal(st_j, st_s)
    made = st_j == KR.CREATED
    assert made.sum() > 250
    rel = np.abs(pos_j[made] - pos_s[made]).max(1) / np.abs(pos_s[made]).max(1)
    print(f"scene {si}: max relative pos_w difference Jacobi vs SVD over {made.sum()} created slots: {rel.max():.3e}")
    assert POS_BOUND < 1e-9
    assert rel.max() <= POS_BOUND, rel.max()


def test_every_status_is_reached():
    seen = np.zeros(10, np.int64)
    for si in ALL:
        st = scene_run(si)["jac"][2]
        seen += np.bincount(st[st != S.SENT_U8], minlength=10)
    print(dict(zip(KR.STATUS_NAMES, seen.tolist())))
    assert (seen > 0).all(), dict(zip(KR.STATUS_NAMES, seen.tolist()))
    branches = np.zeros(4, np.int64)
    for si in ALL:
        branches += np.bincount([i.get("branch", 0) for inf in scene_run(si)["infos"] for _, _, _, i in inf], minlength=4)
    assert (branches[1:] > 30).all(), branches               # two cameras, stereo of key frame 1, of key frame 2


def test_dependent_comparisons_keep_their_gap():
    smallest = {}
    for si in ALL:
        for kind, g in scene_run(si)["gaps"]:
            smallest[kind] = min(smallest.get(kind, 1.0), g)
    print(smallest)
    assert set(smallest) >= {"rays", "stereo", "depth", "reproj", "scale"}
    for kind, g in smallest.items():
        if kind != "stereo_equal_inputs":                       # equal depths: both sides bit-identical on any libm
            assert g >= GATE_GAP, (kind, g)


def test_equal_stereo_depths_tie_exactly():
    sc = S.make_scene(300, KR.RGBD, "perspective")
    k1, k2 = sc["kfs"][0], sc["kfs"][2]
    j = int(np.nonzero(k1["x_right"] >= 0)[0][0])
    t = int(np.nonzero(k2["x_right"] >= 0)[0][0])
    k2["depths"][t] = k1["depths"][j]
    k2["bearings"][t] = k2["pose"][:9].reshape(3, 3) @ (k1["pose"][:9].reshape(3, 3).T @ k1["bearings"][j])   # parallel rays: cos = 1
    sf, ls = S.scale_tables()
    gaps = []
    st, _ = KR.triangulate(sc["cam"], KR.RGBD, S.TRUE_BASELINE, sf, ls, S.SCALE_FACTOR, KR.cos_parallax_thr(1.0), k1, k2, j, t, gaps=gaps)
    assert st == KR.NO_PARALLAX and ("stereo_equal_inputs", 0.0) in gaps


@pytest.mark.parametrize("si", ALL)
def test_pair_geometry(si):
    r = scene_run(si)
    sc, pairs = r["scene"], r["pairs"]
    F = sc["F"]
    for p, (f1, f2) in enumerate(pairs):
        k1, k2 = sc["kfs"][f1], sc["kfs"][f2]
        E, epi = r["epi"][p, :9].reshape(3, 3), r["epi"][p, 9:]
        R1, R2 = k1["pose"][:9].reshape(3, 3), k2["pose"][:9].reshape(3, 3)
        c1, c2 = k1["pose"][12:], k2["pose"][12:]
        assert abs(r["base"][p] - np.linalg.norm(c2 - c1)) < 1e-14
        # b1^T E_12 b2 = 0 on ground-truth correspondences (exact bearings of the scene's points)
        for X in sc["points"][:20]:
            b1, b2 = R1 @ (X - c1), R2 @ (X - c2)
            b1, b2 = b1 / np.linalg.norm(b1), b2 / np.linalg.norm(b2)
            assert abs(b1 @ E @ b2) < 1e-13 * max(1.0, np.abs(E).max())
        # the epipole: key frame 1's centre in key frame 2, normalised unless it lies behind a perspective / fisheye camera
        raw = R2 @ (c1 - c2)
        if sc["cam"]["model"] != "equirectangular" and raw[2] <= 0:
            assert np.allclose(epi, raw, rtol=0, atol=1e-14)
            if (f1, f2) == (F - 2, 0):
                assert abs(np.linalg.norm(epi) - 1.0) > 0.05     # the un-normalised case is really un-normalised
        elif np.linalg.norm(raw) > 0:
            # rot_2w c_1 + trans_2w cancels to |raw|: the rounding of the terms (about 1e-16 each) is divided by that length
            assert np.allclose(epi, raw / np.linalg.norm(raw), rtol=0, atol=1e-14 / min(1.0, np.linalg.norm(raw)))
    behind = [p for p, (f1, f2) in enumerate(pairs) if (f1, f2) == (F - 2, 0)]
    assert behind
    # both sides of the gate of this setup
    assert r["skip"][[p for p, (f1, f2) in enumerate(pairs) if (f1, f2) == (1, 3)][0]] == 1
    assert r["skip"][0] == 0 and 0 < r["skip"].sum() < len(pairs)
    for p, (f1, f2) in enumerate(pairs):
        lim = 0.02 * float(sc["kfs"][f2]["median_depth"]) if sc["setup_type"] == KR.MONOCULAR else S.TRUE_BASELINE
        assert bool(r["skip"][p]) == (r["base"][p] < lim)


def test_the_gate_is_decided_at_the_threshold_itself():
    cam = S.CAMS["perspective"]
    P1 = KR.frame_pose(np.eye(3), np.zeros(3))
    for d, med, want in ((0.1, 5.0, False), (np.nextafter(0.1, 0), 5.0, True), (0.2, 10.0, False), (0.25, 12.5, False)):
        P2 = KR.frame_pose(np.eye(3), np.array([-d, 0.0, 0.0]))
        skip, _, dist = KR.pair_geometry(cam, KR.MONOCULAR, 0.0, P1, P2, np.float32(med))
        assert dist == d and skip == (d < 0.02 * float(np.float32(med))) == want
        skip, _, _ = KR.pair_geometry(cam, KR.STEREO, 0.1, P1, P2, None)
        assert skip == (d < 0.1)


def test_skipped_pair_and_sentinels_of_the_restatement():
    r = scene_run(0)
    idx, pos, st, _, _ = r["jac"]
    p = int(np.nonzero(r["skip"])[0][0])
    n2 = len(r["scene"]["kfs"][r["pairs"][p][1]]["keypts"])
    assert (st[p, :n2] == KR.PAIR_SKIPPED).all() and (st[p, n2:] == S.SENT_U8).all() and (idx[p] == S.SENT_I32).all()
