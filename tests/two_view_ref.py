"""A plain-Python restatement of solve::essential_solver (src/PLPSLAM/solve/essential_solver.cc:33-253) and of DESIGN.md section 5, D24,
written from those two texts: Python floats (IEEE f64), math.sqrt, lists; a float (f32) value is a Python float rounded through numpy.float32.
It shares no code with the library (the one-sided Jacobi is the restatement of D14, tests/pnp_solver_ref.py); tests/test_two_view_cpu.py holds
the host build of csrc/essential.hpp to it bit for bit.

`linalg="svd"` swaps the two Jacobi uses of compute_E_21 for numpy.linalg.svd of the N x 9 matrix and of the 3 x 3 matrix: the stand-in for an
Eigen build, not the code under test."""
import math

import numpy as np

from pnp_solver_ref import INF, MASK, div, hestenes, identity, mix64, norm2, ranks, sqrt_

OK, TOO_FEW_MATCHES, INVALID = range(3)
MIN_SET = 8
RESIDUAL_COS_THR = float(np.float32(0.01745240643))


def f32(x):
    """the value narrowed to float: a product, sum or quotient of two floats rounded once from its f64 value equals the float operation"""
    with np.errstate(all="ignore"):
        return float(np.float32(x))


# ---- D24 items b and c: compute_E_21
def coefficient_rows(b1s, b2s):
    """the rows of A (:130-135): A(i, 3 r + c) = bearing_2(r) * bearing_1(c)"""
    return [[b2[r] * b1[c] for r in range(3) for c in range(3)] for b1, b2 in zip(b1s, b2s)]


def null_vector(A):
    """the column of V of rank 8 of the Jacobi on M = A^T A, every entry of M one accumulator over the rows in ascending order"""
    M = [[0.0] * 9 for _ in range(9)]
    for a in range(9):
        for b in range(a, 9):
            acc = 0.0
            for row in A:
                acc = acc + row[a] * row[b]
            M[a][b] = M[b][a] = acc
    G = [[M[i][j] for i in range(9)] for j in range(9)]
    V = identity(9)
    sweeps = hestenes(G, V)
    rk, _ = ranks([norm2(g) for g in G])
    return list(V[rk.index(8)]), sweeps


def sign_rule(v):
    """the component of largest magnitude is made non-negative, the first of equals"""
    big = 0
    for i in range(1, len(v)):
        if abs(v[i]) > abs(v[big]):
            big = i
    return [-x for x in v] if v[big] < 0 else list(v)


def rank_two(v):
    """E_21 = g_r0 v_r0^T + g_r1 v_r1^T of the Jacobi on the 3 x 3 matrix the vector fills row by row (:141-151)"""
    G = [[v[3 * i + j] for i in range(3)] for j in range(3)]
    V = identity(3)
    sweeps = hestenes(G, V)
    rk, _ = ranks([norm2(g) for g in G])
    r0, r1 = rk.index(0), rk.index(1)
    return [[G[r0][i] * V[r0][k] + G[r1][i] * V[r1][k] for k in range(3)] for i in range(3)], sweeps


def compute_E_21(b1s, b2s, linalg="jacobi"):
    """compute_E_21 (:121-154).  Returns (E rows, (sweeps 9 x 9, sweeps 3 x 3))"""
    A = coefficient_rows(b1s, b2s)
    if linalg == "svd":
        An = np.array(A, np.float64).reshape(-1, 9)
        if len(An) < 9:
            An = np.vstack([An, np.zeros((9 - len(An), 9))])        # ComputeFullV: V is 9 x 9 whatever the number of rows
        v = np.linalg.svd(An)[2][8]
        U, s, Vt = np.linalg.svd(v.reshape(3, 3))
        return (U @ np.diag([s[0], s[1], 0.0]) @ Vt).tolist(), (0, 0)
    v, s0 = null_vector(A)
    E, s1 = rank_two(sign_rule(v))
    return E, (s0, s1)


# ---- check_inliers (:196-253)
def residuals(E, b1, b2):
    """the two float residuals of a match and its code: bit 0 = residual_in_2 is added to the score, bit 1 = residual_in_1 too, an inlier"""
    p = [(E[r][0] * b1[0] + E[r][1] * b1[1]) + E[r][2] * b1[2] for r in range(3)]
    r2 = f32(abs(div((p[0] * b2[0] + p[1] * b2[1]) + p[2] * b2[2], sqrt_((p[0] * p[0] + p[1] * p[1]) + p[2] * p[2]))))
    q = [(E[0][c] * b2[0] + E[1][c] * b2[1]) + E[2][c] * b2[2] for c in range(3)]
    r1 = f32(abs(div((q[0] * b1[0] + q[1] * b1[1]) + q[2] * b1[2], sqrt_((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]))))
    if RESIDUAL_COS_THR < r2:
        return r2, r1, 0
    if RESIDUAL_COS_THR < r1:
        return r2, r1, 1
    return r2, r1, 3


def check_inliers(E, B1, B2):
    """Returns (score, flags, margin: the smallest |residual - thr| / thr over the comparisons made)"""
    score, flags, margin = 0.0, [], INF
    for b1, b2 in zip(B1, B2):
        r2, r1, code = residuals(E, b1, b2)
        if r2 == r2:
            margin = min(margin, abs(r2 - RESIDUAL_COS_THR) / RESIDUAL_COS_THR)
        if code & 1:
            score = f32(score + r2)
            if r1 == r1:
                margin = min(margin, abs(r1 - RESIDUAL_COS_THR) / RESIDUAL_COS_THR)
        if code & 2:
            score = f32(score + r1)
        flags.append(1 if code == 3 else 0)
    return score, flags, margin


# ---- D24 item d: the samples
def draw(seed, p, it, n):
    """eight distinct indices of [0, n), n >= 8: eight steps of D13's partial Fisher-Yates shuffle"""
    base = mix64((seed & MASK) ^ mix64((((p & 0xFFFFFFFF) << 32) | (it & 0xFFFFFFFF))))
    a = {}
    out = []
    for k in range(MIN_SET):
        r = mix64((base + (k + 1) * 0x9E3779B97F4A7C15) & MASK)
        j = k + (r >> 32) % (n - k)
        aj, ak = a.get(j, j), a.get(k, k)
        out.append(aj)
        a[j], a[k] = ak, aj
    return out


def matched_slots(match, count_1, count_2):
    return [s for s in range(count_1) if 0 <= match[s] < count_2]


def find_via_ransac(bearing_1, bearing_2, match, iters=100, recompute=True, samples=None, seed=0, p=0, count_1=None, count_2=None, linalg="jacobi"):
    """constructor + find_via_ransac (:33-119) of one problem in slot form.  Returns dict(status, num_matches, E_21 rows, score, num_inliers,
    best_iter, inliers per slot, hyp_score, hyp_flags: the inlier flags of every hypothesis per match, margin)"""
    n_cap = len(match)
    count_1 = n_cap if count_1 is None else max(0, min(int(count_1), n_cap))
    count_2 = len(bearing_2) if count_2 is None else max(0, min(int(count_2), len(bearing_2)))
    slots = matched_slots(match, count_1, count_2)
    n = len(slots)
    B1 = [list(map(float, bearing_1[s])) for s in slots]
    B2 = [list(map(float, bearing_2[match[s]])) for s in slots]
    res = dict(status=OK, num_matches=n, E_21=[[0.0] * 3 for _ in range(3)], score=0.0, num_inliers=0, best_iter=-1, inliers=[0] * n_cap,
               hyp_score=[0.0] * iters, hyp_flags=[None] * iters, margin=INF, count_1=count_1)
    if n < MIN_SET:                                                  # :45
        res["status"] = TOO_FEW_MATCHES
        return res
    best_score, best_E, best_flags, best_iter = 0.0, None, [0] * n, -1
    for it in range(iters):
        idx = list(samples[it]) if samples is not None else draw(seed, p, it, n)
        if any(not (0 <= i < n) for i in idx) or len(set(idx)) != MIN_SET:
            continue
        E, _ = compute_E_21([B1[i] for i in idx], [B2[i] for i in idx], linalg)
        score, flags, margin = check_inliers(E, B1, B2)
        res["margin"] = min(res["margin"], margin)
        res["hyp_score"][it] = score
        res["hyp_flags"][it] = flags
        if best_score < score:                                       # :87
            best_score, best_E, best_flags, best_iter = score, E, flags, it
    if not (best_score > 0.0 and sum(best_flags) >= MIN_SET):        # :96
        res["status"] = INVALID
        return res
    if recompute:                                                    # :103-118
        best_E, _ = compute_E_21([B1[k] for k in range(n) if best_flags[k]], [B2[k] for k in range(n) if best_flags[k]], linalg)
        best_score, best_flags, margin = check_inliers(best_E, B1, B2)
        res["margin"] = min(res["margin"], margin)
    res.update(E_21=best_E, score=best_score, num_inliers=sum(best_flags), best_iter=best_iter)
    for k in range(n):
        res["inliers"][slots[k]] = best_flags[k]
    return res


# ---- what the entries leave in sentinel-filled arrays
SENTINEL = dict(status=0xEE, num_matches=-77, E_21=-7.25, score=-3.5, num_inliers=-77, best_iter=-77, inliers=0xEE, hyp_score=-3.5)


def expected(results, n_cap, iters):
    """the outputs of plp_essential_ransac_* over arrays filled with SENTINEL, from find_via_ransac's results"""
    P = len(results)
    o = dict(status=np.zeros(P, np.uint8), num_matches=np.zeros(P, np.int32), E_21=np.zeros((P, 3, 3)), score=np.zeros(P, np.float32),
             num_inliers=np.zeros(P, np.int32), best_iter=np.zeros(P, np.int32), inliers=np.full((P, n_cap), SENTINEL["inliers"], np.uint8),
             hyp_score=np.zeros((P, iters), np.float32))
    for p, r in enumerate(results):
        o["status"][p], o["num_matches"][p], o["E_21"][p], o["score"][p] = r["status"], r["num_matches"], r["E_21"], r["score"]
        o["num_inliers"][p], o["best_iter"][p] = r["num_inliers"], r["best_iter"]
        o["inliers"][p, :r["count_1"]] = r["inliers"][:r["count_1"]]
        o["hyp_score"][p] = r["hyp_score"]
    return o


# ---------------------------------------------------------------------------------------------------------------- D24 items c, f, g
# essential_solver::decompose (:156-186), initialize::base::check_pose and find_most_plausible_pose (initialize/base.cc:62-243) with
# solve::triangulator::triangulate (solve/triangulator.h:86-103).  acos is the restatement of D22's (tests/pose_graph_ref.py), the cameras are the
# restatement of camera::*::reproject_to_image (tests/sim3_solver_ref.py).
import struct

from pose_graph_ref import acos as d22_acos
from sim3_solver_ref import EQUIRECTANGULAR
from sim3_solver_ref import reproject as camera_reproject

TV_OK, TV_NO_SOLUTION, TV_TOO_FEW_TRIANGULATED, TV_AMBIGUOUS, TV_SMALL_PARALLAX = range(5)
NOT_FINITE, DEPTH_REF, DEPTH_CUR, INVALID_REF, ERR_REF, INVALID_CUR, ERR_CUR, VALID_SMALL, VALID = range(1, 10)   # where a match leaves the loop of check_pose
COS_PARALLAX_THR = f32(0.99996192306)
IDENT = [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]


def dot3(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def decompose(E):
    """Returns (rots: four 3 x 3 row lists, transes: four vectors) in the order of :182-183"""
    G = [[E[i][j] for i in range(3)] for j in range(3)]
    V = identity(3)
    hestenes(G, V)
    rk, keys = ranks([norm2(g) for g in G])
    U, W = [], []
    for a in (0, 1):
        j = rk.index(a)
        sg = math.sqrt(keys[j])
        have = 0.0 < sg < INF
        u = [G[j][i] / sg if have else 0.0 for i in range(3)]
        v = list(V[j])
        big = 0
        for i in (1, 2):
            if abs(v[i]) > abs(v[big]):
                big = i
        if v[big] < 0:
            u, v = [-x for x in u], [-x for x in v]
        U.append(u)
        W.append(v)
    cross = lambda a, b: [a[(i + 1) % 3] * b[(i + 2) % 3] - a[(i + 2) % 3] * b[(i + 1) % 3] for i in range(3)]
    U.append(cross(U[0], U[1]))
    W.append(cross(W[0], W[1]))
    nrm = sqrt_((U[2][0] * U[2][0] + U[2][1] * U[2][1]) + U[2][2] * U[2][2])
    trans = [div(x, nrm) for x in U[2]]
    rot_1 = [[(U[1][i] * W[0][k] + (-U[0][i]) * W[1][k]) + U[2][i] * W[2][k] for k in range(3)] for i in range(3)]
    rot_2 = [[((-U[1][i]) * W[0][k] + U[0][i] * W[1][k]) + U[2][i] * W[2][k] for k in range(3)] for i in range(3)]
    out = []
    for R in (rot_1, rot_2):
        det = R[0][0] * R[1][1] * R[2][2] + R[0][1] * R[1][2] * R[2][0] + R[0][2] * R[1][0] * R[2][1] - R[0][2] * R[1][1] * R[2][0] \
            - R[0][1] * R[1][0] * R[2][2] - R[0][0] * R[1][2] * R[2][1]
        out.append([[x * -1.0 for x in r] for r in R] if det < 0 else R)
    neg = [-x for x in trans]
    return [out[0], out[0], out[1], out[1]], [trans, neg, list(trans), list(neg)]


def center(R, t):
    """-rot^T * trans"""
    return [((-R[0][i]) * t[0] + (-R[1][i]) * t[1]) + (-R[2][i]) * t[2] for i in range(3)]


def reproject_in(cam, bounds, R, t, x):
    """reproject_to_image: (u, v, the function's result); (0, 0) where the camera writes nothing"""
    r = camera_reproject(cam, R, t, x)
    if r is None:
        return 0.0, 0.0, False
    if cam["model"] == EQUIRECTANGULAR:
        return r[0], r[1], True
    return r[0], r[1], bounds[0] < r[0] < bounds[1] and bounds[2] < r[1] < bounds[3]


def check_match(cam, bounds, R, t, c, b1, b2, kp1, kp2, reproj_err_thr, depth_is_positive):
    """the loop body of check_pose (:153-227).  Returns (code, pos, cos_parallax)"""
    q = [(R[0][i] * b2[0] + R[1][i] * b2[1]) + R[2][i] * b2[2] for i in range(3)]
    a00, a10, a11 = dot3(b1, b1), dot3(b1, q), -dot3(q, q)
    a01 = -a10
    r0, r1 = dot3(b1, c), dot3(q, c)
    inv_det = div(1.0, a00 * a11 - a01 * a10)
    i00, i01, i10, i11 = a11 * inv_det, (-a01) * inv_det, (-a10) * inv_det, a00 * inv_det
    l0, l1 = i00 * r0 + i01 * r1, i10 * r0 + i11 * r1
    pos = [(l0 * b1[i] + (l1 * q[i] + c[i])) / 2.0 for i in range(3)]
    if not all(math.isfinite(v) for v in pos):
        return NOT_FINITE, pos, 0.0
    cn = [pos[i] - c[i] for i in range(3)]
    ref_norm, cur_norm = f32(sqrt_(dot3(pos, pos))), f32(sqrt_(dot3(cn, cn)))
    cosp = f32(div(dot3(pos, cn), f32(ref_norm * cur_norm)))
    small = COS_PARALLAX_THR < cosp
    if depth_is_positive:
        if not small and pos[2] <= 0:
            return DEPTH_REF, pos, cosp
        zc = ((R[2][0] * pos[0] + R[2][1] * pos[1]) + R[2][2] * pos[2]) + t[2]
        if not small and zc <= 0:
            return DEPTH_CUR, pos, cosp
    thr = f32(reproj_err_thr)
    thr_sq = f32(thr * thr)
    u, v, ok = reproject_in(cam, bounds, IDENT, [0.0, 0.0, 0.0], pos)
    if not small and not ok:
        return INVALID_REF, pos, cosp
    if thr_sq < f32((u - kp1[0]) * (u - kp1[0]) + (v - kp1[1]) * (v - kp1[1])):
        return ERR_REF, pos, cosp
    u, v, ok = reproject_in(cam, bounds, R, t, pos)
    if not small and not ok:
        return INVALID_CUR, pos, cosp
    if thr_sq < f32((u - kp2[0]) * (u - kp2[0]) + (v - kp2[1]) * (v - kp2[1])):
        return ERR_CUR, pos, cosp
    return (VALID_SMALL if small else VALID), pos, cosp


def float_key(v):
    u = struct.unpack("I", struct.pack("f", v))[0]
    return (~u & 0xFFFFFFFF) if u & 0x80000000 else (u | 0x80000000)


def check_pose(cam, bounds, R, t, inliers, match, bearing_1, bearing_2, kps_1, kps_2, reproj_err_thr=4.0, depth_is_positive=False, count_2=None):
    """check_pose (:123-243) in slot form.  Returns dict(num_valid, parallax_deg, pts, is_triangulated, code per slot)"""
    n_cap = len(match)
    count_2 = len(bearing_2) if count_2 is None else count_2
    c = center(R, t)
    res = dict(num_valid=0, parallax_deg=0.0, pts=[[0.0] * 3 for _ in range(n_cap)], is_triangulated=[0] * n_cap, code=[0] * n_cap)
    cos_parallaxes = []
    for s in range(n_cap):
        if not inliers[s] or not (0 <= match[s] < count_2):
            continue
        m = match[s]
        code, pos, cosp = check_match(cam, bounds, R, t, c, [float(x) for x in bearing_1[s]], [float(x) for x in bearing_2[m]],
                                      (float(kps_1[s][0]), float(kps_1[s][1])), (float(kps_2[m][0]), float(kps_2[m][1])), reproj_err_thr, depth_is_positive)
        res["code"][s] = code
        if code >= VALID_SMALL:
            res["num_valid"] += 1
            cos_parallaxes.append(cosp)
        if code == VALID:
            res["pts"][s], res["is_triangulated"][s] = pos, 1
    if cos_parallaxes:
        cos_parallaxes.sort(key=float_key)
        res["parallax_deg"] = f32(d22_acos(cos_parallaxes[min(50, len(cos_parallaxes) - 1)]) * 180.0 / math.pi)
    return res


def find_most_plausible_pose(checks, min_num_triangulated, parallax_deg_thr):
    """:83-120 behind the four check_pose results.  Returns (status, chosen or -1)"""
    nums = [r["num_valid"] for r in checks]
    best = nums.index(max(nums))
    if nums[best] < min_num_triangulated:
        return TV_TOO_FEW_TRIANGULATED, -1
    if 1 < sum(1 for n in nums if 0.8 * nums[best] < n):
        return TV_AMBIGUOUS, -1
    if checks[best]["parallax_deg"] < f32(parallax_deg_thr):
        return TV_SMALL_PARALLAX, -1
    return TV_OK, best


def two_view_pose(cam, bounds, E, inliers, match, bearing_1, bearing_2, kps_1, kps_2, min_num_triangulated=50, parallax_deg_thr=1.0, reproj_err_thr=4.0,
                  depth_is_positive=False, in_status=0, count_2=None):
    """reconstruct_with_E (bearing_vector.cc:84-107) of one problem.  Returns dict(status, rot, trans, hypothesis, num_valid, parallax_deg, pts,
    is_triangulated, hyp_is_triangulated, codes: per hypothesis the code of every slot)"""
    n_cap = len(match)
    res = dict(status=TV_NO_SOLUTION, rot=[[0.0] * 3 for _ in range(3)], trans=[0.0] * 3, hypothesis=-1, num_valid=[0] * 4, parallax_deg=[0.0] * 4,
               pts=[[0.0] * 3 for _ in range(n_cap)], is_triangulated=[0] * n_cap, hyp_is_triangulated=[[0] * n_cap for _ in range(4)], codes=[[0] * n_cap] * 4)
    if in_status != 0:
        return res
    rots, transes = decompose(E)
    checks = [check_pose(cam, bounds, rots[h], transes[h], inliers, match, bearing_1, bearing_2, kps_1, kps_2, reproj_err_thr, depth_is_positive, count_2)
              for h in range(4)]
    status, chosen = find_most_plausible_pose(checks, min_num_triangulated, parallax_deg_thr)
    res.update(status=status, hypothesis=chosen, num_valid=[r["num_valid"] for r in checks], parallax_deg=[r["parallax_deg"] for r in checks],
               hyp_is_triangulated=[r["is_triangulated"] for r in checks], codes=[r["code"] for r in checks])
    if chosen >= 0:
        res.update(rot=rots[chosen], trans=transes[chosen], pts=checks[chosen]["pts"], is_triangulated=checks[chosen]["is_triangulated"])
    return res


TV_SENTINEL = dict(status=0xEE, rot_ref_to_cur=-7.25, trans_ref_to_cur=-7.25, hypothesis=-77, num_valid=-77, parallax_deg=-3.5, triangulated_pts=-7.25,
                   is_triangulated=0xEE, hyp_is_triangulated=0xEE)


def tv_expected(results, n_cap, counts_1=None):
    """the outputs of plp_two_view_pose_* over arrays filled with TV_SENTINEL"""
    P = len(results)
    o = dict(status=np.zeros(P, np.uint8), rot_ref_to_cur=np.zeros((P, 3, 3)), trans_ref_to_cur=np.zeros((P, 3)), hypothesis=np.zeros(P, np.int32),
             num_valid=np.zeros((P, 4), np.int32), parallax_deg=np.zeros((P, 4), np.float32), triangulated_pts=np.full((P, n_cap, 3), TV_SENTINEL["triangulated_pts"]),
             is_triangulated=np.full((P, n_cap), 0xEE, np.uint8), hyp_is_triangulated=np.full((P, 4, n_cap), 0xEE, np.uint8))
    for p, r in enumerate(results):
        n = len(r["is_triangulated"]) if counts_1 is None else int(counts_1[p])
        o["status"][p], o["rot_ref_to_cur"][p], o["trans_ref_to_cur"][p], o["hypothesis"][p] = r["status"], r["rot"], r["trans"], r["hypothesis"]
        o["num_valid"][p], o["parallax_deg"][p] = r["num_valid"], r["parallax_deg"]
        o["triangulated_pts"][p, :n], o["is_triangulated"][p, :n] = np.array(r["pts"])[:n], r["is_triangulated"][:n]
        o["hyp_is_triangulated"][p, :, :n] = np.array(r["hyp_is_triangulated"])[:, :n]
    return o
