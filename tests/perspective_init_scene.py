"""Seeded frame pairs for the two solvers of initialize::perspective (tests/test_perspective_init_cpu.py, tests/test_gpu_perspective_ransac.py): the
pose scenes of tests/two_view_scene.py -- a planar scene, general clouds, a low-parallax scene, with pixel noise and mismatches -- seen through
their undistorted key points, with one sample table per solver, and the special problems of DESIGN.md D27."""
import numpy as np

import two_view_scene as S
from plp import plp

KP = plp.KP_DTYPE


def problem(seed, n_matches, model="perspective", n_slots=None, noise=1e-3, mismatch=0.0, iters=24, kind="cloud"):
    """S.pose_problem plus samples_h / samples_f (iters, 8): distinct octuples of matches, another table per solver"""
    q = S.pose_problem(seed, n_matches, model, n_slots, noise, mismatch, iters, kind)
    rng = np.random.default_rng(seed + 7919)
    q["samples_h"] = q.pop("samples")
    q["samples_f"] = np.stack([rng.choice(n_matches, 8, replace=False) if n_matches >= 8 else np.arange(8) for _ in range(iters)]).astype(np.int32)
    return q


def scenes():
    out = {}
    out["planar"] = problem(500, 150, "perspective", n_slots=160, noise=5e-4, mismatch=0.1, kind="planar")
    out["cloud_64"] = problem(501, 64, "perspective", n_slots=71, noise=1e-3, mismatch=0.2)
    out["cloud_200"] = problem(502, 200, "perspective", n_slots=214, noise=3e-4, mismatch=0.15, iters=24)
    out["fisheye_200"] = problem(503, 200, "fisheye", n_slots=207, noise=2e-3, mismatch=0.2, iters=12)
    out["low_parallax"] = problem(504, 120, "perspective", n_slots=130, noise=5e-4, mismatch=0.1, kind="near_rotation")
    out["exact"] = problem(505, 90, "perspective", noise=0.0)
    out["eight"] = problem(506, 8, "perspective", noise=0.0)
    out["all_mismatched"] = problem(507, 60, "perspective", mismatch=1.0)
    out["seven"] = problem(508, 7, "perspective", n_slots=12)
    out["none"] = problem(509, 0, "perspective", n_slots=9)
    return out


ANCHORS = ("planar", "cloud_64", "cloud_200", "fisheye_200", "low_parallax")   # the scenes held against numpy's svd and inverse


def degenerate_problem():
    """the degenerate samples in one problem, the same table for both solvers: iteration 0 a bad index, 1 a repeated index, 2 a negative index, 3 a
    sample of exact matches, 4 the same sample again (a tie), 5 eight matches whose key points of frame 1 lie on one line (the homography through
    them is singular), 6 the sample of 3 in another order, 7 another sample of exact matches"""
    q = problem(71, 40, "perspective", n_slots=48, noise=0.0, mismatch=0.2, iters=8)
    slots = np.flatnonzero(q["match"] >= 0)
    good = np.flatnonzero(~q["is_mismatch"])
    good = good[good > 18]
    for i, k in enumerate(range(10, 18)):                               # eight key points of frame 1 on the line y = 100 + x / 2
        q["undist_1"]["x"][slots[k]] = 80.0 + 40.0 * i
        q["undist_1"]["y"][slots[k]] = 140.0 + 20.0 * i
    s = np.zeros((8, 8), np.int32)
    s[0] = [0, 5, 40, 7, 1, 2, 3, 4]
    s[1] = [4, 9, 4, 8, 1, 2, 3, 5]
    s[2] = [0, 5, -1, 7, 1, 2, 3, 4]
    s[3] = good[:8]
    s[4] = good[:8]
    s[5] = np.arange(10, 18)
    s[6] = good[:8][::-1]
    s[7] = good[3:11]
    q["samples_h"], q["samples_f"] = s, s.copy()
    return q


def nan_problem():
    """one NaN key point among the matches of frame 1: the frame's normalisation, every hypothesis and every score are NaN, which never wins"""
    q = problem(72, 30, "perspective", n_slots=34, iters=6)
    q["undist_1"]["x"][np.flatnonzero(q["match"] >= 0)[11]] = np.nan
    return q


def constant_frame_problem():
    """every key point of frame 2 at one place: a zero deviation, an infinite reciprocal (D27 item a)"""
    q = problem(73, 30, "perspective", n_slots=34, iters=6)
    q["undist_2"]["x"], q["undist_2"]["y"] = 100.0, 50.0
    return q


def xy(kp):
    return np.stack([kp["x"], kp["y"]], -1)


def pack(problems, n_cap=None, m_cap=None, given=None):
    """the [P][n_cap] / [P][m_cap] arrays of plp_perspective_ransac_args for problems of one iteration count: slots at or above a problem's own hold
    matches and key points that the counts hide.  given: {p: (H (3, 3), count)} -> given_H_21 / given_H_num_inliers, -1 for the other problems"""
    P = len(problems)
    n_cap = max(len(q["match"]) for q in problems) if n_cap is None else n_cap
    m_cap = max(len(q["undist_2"]) for q in problems) if m_cap is None else m_cap
    iters = problems[0]["iters"]
    hidden = np.zeros((), KP)
    hidden["x"], hidden["y"] = 12345.0, -777.0
    a = dict(undist_1=np.full((P, n_cap), hidden, KP), undist_2=np.full((P, m_cap), hidden, KP), match=np.zeros((P, n_cap), np.int32),
             samples_h=np.zeros((P, iters, 8), np.int32), samples_f=np.zeros((P, iters, 8), np.int32), counts_1=np.zeros(P, np.int32), counts_2=np.zeros(P, np.int32))
    for p, q in enumerate(problems):
        n, m = len(q["match"]), len(q["undist_2"])
        assert q["iters"] == iters and n <= n_cap and m <= m_cap
        a["undist_1"][p, :n], a["undist_2"][p, :m], a["match"][p, :n] = q["undist_1"], q["undist_2"], q["match"]
        a["samples_h"][p], a["samples_f"][p] = q["samples_h"], q["samples_f"]
        a["counts_1"][p], a["counts_2"][p] = n, m
    if given is not None:
        a["given_H_21"], a["given_H_num_inliers"] = np.zeros((P, 3, 3)), np.full(P, -1, np.int32)
        for p, (Hm, count) in given.items():
            a["given_H_21"][p], a["given_H_num_inliers"][p] = Hm, count
    return a


def call_kwargs(a, recompute=True, seed=None):
    """the arguments of plp.model_perspective_ransac / matcher.perspective_ransac for a pack: (positional, keywords)"""
    kw = dict(iters=a["samples_h"].shape[1], recompute=recompute, counts_1=a["counts_1"], counts_2=a["counts_2"])
    kw.update(dict(seed=seed) if seed is not None else dict(samples_h=a["samples_h"], samples_f=a["samples_f"]))
    if "given_H_21" in a:
        kw.update(given_H_21=a["given_H_21"], given_H_num_inliers=a["given_H_num_inliers"])
    return (a["undist_1"], a["undist_2"], a["match"]), kw


def run_ref(q, recompute=True, samples="given", seed=0, p=0, linalg="jacobi", given=None, count_1=None, count_2=None):
    import perspective_init_ref as R
    g = dict(given_H=given[0], given_count=given[1]) if given is not None else {}
    return R.perspective_ransac(xy(q["undist_1"]).tolist(), xy(q["undist_2"]).tolist(), q["match"].tolist(), iters=q["iters"], recompute=recompute,
                                samples_h=q["samples_h"].tolist() if samples == "given" else None, samples_f=q["samples_f"].tolist() if samples == "given" else None,
                                seed=seed, p=p, linalg=linalg, count_1=count_1, count_2=count_2, **g)
