"""A plain-Python restatement of the two solvers of initialize::perspective::initialize (src/PLPSLAM/initialize/perspective.cc:84-120):
solve::homography_solver (solve/homography_solver.cc:60-155, :388-402, :405-436, :556-631), solve::fundamental_solver
(solve/fundamental_solver.cc:50-144, :299-332, :349-426), solve::normalize (solve/common.cc:31-76), and of DESIGN.md section 5, D27, written from
those texts: Python floats (IEEE f64), lists; a float (f32) value is a Python float rounded through numpy.float32.  It shares no code with the
library (the Jacobi, the sign rule, the rank-two step and the generator are the restatements of D14 and D24, tests/pnp_solver_ref.py and
tests/two_view_ref.py); tests/test_perspective_init_cpu.py holds the host build of csrc/perspective_init.hpp to it bit for bit.

`linalg="svd"` swaps the Jacobi uses for numpy.linalg.svd of the row matrix and of the 3 x 3 matrix and the cofactor inverse for numpy.linalg.inv:
the stand-in for an Eigen build, not the code under test."""
import numpy as np

from pnp_solver_ref import INF, div
from two_view_ref import draw, f32, matched_slots, null_vector, rank_two, sign_rule

OK, TOO_FEW_MATCHES, INVALID = range(3)
CHOICE_NONE, CHOICE_H, CHOICE_F = range(3)
H, F = 0, 1
MIN_SET = 8
CHI_SQ_2 = f32(5.991)
CHI_SQ_1 = f32(3.841)
STREAM_OF_F = 65536


# ---- D27 item a: solve::normalize
def normalize(pts):
    """pts: the (x, y) of ALL key points of a frame.  Returns (mean_x, mean_y, inv_x, inv_y) as floats"""
    n = float(len(pts))
    mean, inv = [], []
    for c in range(2):
        acc = 0.0
        for pt in pts:
            acc = f32(acc + pt[c])
        mean.append(f32(div(acc, n)))
    for c in range(2):
        acc = 0.0
        for pt in pts:
            acc = f32(acc + abs(f32(pt[c] - mean[c])))
        inv.append(f32(div(1.0, f32(div(acc, n)))))
    return mean[0], mean[1], inv[0], inv[1]


def fmul(a, b):
    with np.errstate(all="ignore"):
        return float(np.float32(a) * np.float32(b))


def normalized(v, mean, inv):
    return fmul(f32(v - mean), inv)


def transform(nrm):
    return [[nrm[2], 0.0, fmul(-nrm[0], nrm[2])], [0.0, nrm[3], fmul(-nrm[1], nrm[3])], [0.0, 0.0, 1.0]]


# ---- 3 x 3
def mul3(A, B):
    return [[(A[i][0] * B[0][j] + A[i][1] * B[1][j]) + A[i][2] * B[2][j] for j in range(3)] for i in range(3)]


def transpose3(A):
    return [[A[j][i] for j in range(3)] for i in range(3)]


def inv3(A, linalg="jacobi"):
    """D27 item c: every cofactor over the determinant expanded along the first row"""
    if linalg == "svd":
        with np.errstate(all="ignore"):
            try:
                return np.linalg.inv(np.array(A, np.float64)).tolist()
            except np.linalg.LinAlgError:
                return [[float("nan")] * 3 for _ in range(3)]
    a = [x for r in A for x in r]
    c00, c01, c02 = a[4] * a[8] - a[5] * a[7], a[3] * a[8] - a[5] * a[6], a[3] * a[7] - a[4] * a[6]
    det = (a[0] * c00 - a[1] * c01) + a[2] * c02
    o = [c00, a[2] * a[7] - a[1] * a[8], a[1] * a[5] - a[2] * a[4], a[5] * a[6] - a[3] * a[8], a[0] * a[8] - a[2] * a[6], a[2] * a[3] - a[0] * a[5], c02,
         a[1] * a[6] - a[0] * a[7], a[0] * a[4] - a[1] * a[3]]
    o = [div(x, det) for x in o]
    return [o[0:3], o[3:6], o[6:9]]


# ---- D27 item b: the rows of compute_H_21 (:418-423) and compute_F_21 (:310-312); a pair is (u1, v1, u2, v2) normalised
def rows_h(pairs):
    out = []
    for u1, v1, u2, v2 in pairs:
        h = [u1, v1, 1.0]
        out.append([0.0, 0.0, 0.0] + [-x for x in h] + [v2 * x for x in h])
        out.append(h + [0.0, 0.0, 0.0] + [(-u2) * x for x in h])
    return out


def rows_f(pairs):
    return [[u2 * x for x in (u1, v1, 1.0)] + [v2 * x for x in (u1, v1, 1.0)] + [u1, v1, 1.0] for u1, v1, u2, v2 in pairs]


def svd_null(A):
    An = np.array(A, np.float64).reshape(-1, 9)
    if len(An) < 9:
        An = np.vstack([An, np.zeros((9 - len(An), 9))])
    return np.linalg.svd(An)[2][8].tolist()


def fit(solver, pairs, T1, T2, linalg="jacobi"):
    """compute_H_21 / compute_F_21 and the de-normalisation (:116, :105).  Returns (matrix rows, sweeps of the 9 x 9 Jacobi)"""
    A = rows_h(pairs) if solver == H else rows_f(pairs)
    v, sweeps = (svd_null(A), 0) if linalg == "svd" else null_vector(A)
    if solver == H:
        v = sign_rule(v)
        Mn = [v[0:3], v[3:6], v[6:9]]
        return mul3(mul3(inv3(T2, linalg), Mn), T1), sweeps
    if linalg == "svd":
        U, s, Vt = np.linalg.svd(np.array(v).reshape(3, 3))
        Mn = (U @ np.diag([s[0], s[1], 0.0]) @ Vt).tolist()
    else:
        Mn, _ = rank_two(sign_rule(v))
    return mul3(mul3(transpose3(T2), Mn), T1), sweeps


# ---- the loop bodies of check_inliers; chi_a is the side tested first
def residuals_h(M, N, x1, y1, x2, y2):
    def side(Q, u, v, pu, pv):
        t = [(Q[r][0] * u + Q[r][1] * v) + Q[r][2] for r in range(3)]
        dx, dy, dz = pu - div(t[0], t[2]), pv - div(t[1], t[2]), 1.0 - div(t[2], t[2])
        return f32((dx * dx + dy * dy) + dz * dz)
    return side(M, x1, y1, x2, y2), side(N, x2, y2, x1, y1), CHI_SQ_2


def residuals_f(M, _, x1, y1, x2, y2):
    def side(Q, u, v, pu, pv):
        l = [(Q[r][0] * u + Q[r][1] * v) + Q[r][2] for r in range(3)]
        r = f32((l[0] * pu + l[1] * pv) + l[2])
        return f32(div(fmul(r, r), l[0] * l[0] + l[1] * l[1]))
    return side(M, x1, y1, x2, y2), side(transpose3(M), x2, y2, x1, y1), CHI_SQ_1


def check_inliers(solver, M, pts, linalg="jacobi"):
    """pts: (x1, y1, x2, y2) of the matches as the key points hold them.  Returns (score, flags, margin: the smallest |chi - thr| / thr over the
    comparisons made)"""
    N = inv3(M, linalg) if solver == H else None
    score, flags, margin = 0.0, [], INF
    for x1, y1, x2, y2 in pts:
        ca, cb, thr = (residuals_h if solver == H else residuals_f)(M, N, x1, y1, x2, y2)
        if ca == ca:
            margin = min(margin, abs(ca - thr) / thr)
        if thr < ca:
            flags.append(0)
            continue
        score = f32(score + f32(CHI_SQ_2 - ca))
        if cb == cb:
            margin = min(margin, abs(cb - thr) / thr)
        if thr < cb:
            flags.append(0)
            continue
        score = f32(score + f32(CHI_SQ_2 - cb))
        flags.append(1)
    return score, flags, margin


def solve(solver, pts, npairs, T1, T2, iters, recompute, samples, seed, p, given=None, linalg="jacobi"):
    """find_via_ransac of one solver, or with given = (H rows, count) what the graph-cut path does with its matrix (:388-402)"""
    n = len(pts)
    r = dict(status=OK, M=[[0.0] * 3 for _ in range(3)], score=0.0, num_inliers=0, best_iter=-1, flags=[0] * n, hyp_score=[0.0] * iters, hyp_flags=[None] * iters,
             margin=INF)
    if n < MIN_SET:
        r["status"] = TOO_FEW_MATCHES
        return r
    if given is not None:
        M, count = given
        r["score"], flags, r["margin"] = check_inliers(solver, M, pts, linalg)
        if r["score"] > 0.0 and count >= MIN_SET:
            r.update(M=M, num_inliers=sum(flags), flags=flags)
        else:
            r["status"] = INVALID
        return r
    best_score, best_M, best_flags, best_iter = 0.0, None, [0] * n, -1
    for it in range(iters):
        idx = list(samples[it]) if samples is not None else draw(seed, p + solver * STREAM_OF_F, it, n)
        if any(not (0 <= i < n) for i in idx) or len(set(idx)) != MIN_SET:
            continue
        M, _ = fit(solver, [npairs[i] for i in idx], T1, T2, linalg)
        score, flags, margin = check_inliers(solver, M, pts, linalg)
        r["margin"] = min(r["margin"], margin)
        r["hyp_score"][it], r["hyp_flags"][it] = score, flags
        if best_score < score:
            best_score, best_M, best_flags, best_iter = score, M, flags, it
    r["score"] = best_score
    if not (best_score > 0.0 and sum(best_flags) >= MIN_SET):
        r["status"] = INVALID
        return r
    if recompute:
        best_M, _ = fit(solver, [npairs[k] for k in range(n) if best_flags[k]], T1, T2, linalg)
        best_score, best_flags, margin = check_inliers(solver, best_M, pts, linalg)
        r["margin"] = min(r["margin"], margin)
    r.update(M=best_M, score=best_score, num_inliers=sum(best_flags), best_iter=best_iter, flags=best_flags)
    return r


def perspective_ransac(undist_1, undist_2, match, iters=100, recompute=True, samples_h=None, samples_f=None, seed=0, p=0, count_1=None, count_2=None,
                       given_H=None, given_count=-1, linalg="jacobi"):
    """One problem in slot form; undist_1 / undist_2: (x, y) per key point.  Returns dict(h, f: solve()'s results, num_matches, rel_score_h, choice,
    inliers / inliers_h / inliers_f per slot, count_1)"""
    n_cap = len(match)
    count_1 = n_cap if count_1 is None else max(0, min(int(count_1), n_cap))
    count_2 = len(undist_2) if count_2 is None else max(0, min(int(count_2), len(undist_2)))
    slots = matched_slots(match, count_1, count_2)
    k1 = [(float(undist_1[i][0]), float(undist_1[i][1])) for i in range(count_1)]
    k2 = [(float(undist_2[i][0]), float(undist_2[i][1])) for i in range(count_2)]
    n1, n2 = normalize(k1), normalize(k2)
    T1, T2 = transform(n1), transform(n2)
    pts = [k1[s] + k2[match[s]] for s in slots]
    npairs = [(normalized(a, n1[0], n1[2]), normalized(b, n1[1], n1[3]), normalized(c, n2[0], n2[2]), normalized(d, n2[1], n2[3])) for a, b, c, d in pts]
    given = None if given_H is None or given_count < 0 else ([list(map(float, r)) for r in np.asarray(given_H).reshape(3, 3)], int(given_count))
    h = solve(H, pts, npairs, T1, T2, iters, recompute, samples_h, seed, p, given, linalg)
    f = solve(F, pts, npairs, T1, T2, iters, recompute, samples_f, seed, p, None, linalg)
    rel = f32(div(h["score"], f32(h["score"] + f["score"])))
    choice = CHOICE_H if (0.40 < rel and h["status"] == OK) else CHOICE_F if f["status"] == OK else CHOICE_NONE
    res = dict(h=h, f=f, num_matches=len(slots), rel_score_h=rel, choice=choice, count_1=count_1, slots=slots)
    for key, on, src in (("inliers", choice != CHOICE_NONE, f if choice == CHOICE_F else h), ("inliers_h", h["status"] == OK, h), ("inliers_f", f["status"] == OK, f)):
        mask = [0] * n_cap
        if on:
            for k, s in enumerate(slots):
                mask[s] = src["flags"][k]
        res[key] = mask
    return res


# ---- what the entries leave in sentinel-filled arrays
SENTINEL = dict(status_h=0xEE, status_f=0xEE, num_matches=-77, H_21=-7.25, F_21=-7.25, score_h=-3.5, score_f=-3.5, best_iter_h=-77, best_iter_f=-77, num_inliers_h=-77,
                num_inliers_f=-77, rel_score_h=-3.5, choice=0xEE, inliers=0xEE, inliers_h=0xEE, inliers_f=0xEE, hyp_score_h=-3.5, hyp_score_f=-3.5)


def expected(results, n_cap, iters):
    """the outputs of plp_perspective_ransac_* over arrays filled with SENTINEL, from perspective_ransac's results"""
    P = len(results)
    u8, i32, f32_ = np.uint8, np.int32, np.float32
    o = dict(status_h=np.zeros(P, u8), status_f=np.zeros(P, u8), num_matches=np.zeros(P, i32), H_21=np.zeros((P, 3, 3)), F_21=np.zeros((P, 3, 3)),
             score_h=np.zeros(P, f32_), score_f=np.zeros(P, f32_), best_iter_h=np.zeros(P, i32), best_iter_f=np.zeros(P, i32), num_inliers_h=np.zeros(P, i32),
             num_inliers_f=np.zeros(P, i32), rel_score_h=np.zeros(P, f32_), choice=np.zeros(P, u8), inliers=np.full((P, n_cap), 0xEE, u8),
             inliers_h=np.full((P, n_cap), 0xEE, u8), inliers_f=np.full((P, n_cap), 0xEE, u8), hyp_score_h=np.zeros((P, iters), f32_),
             hyp_score_f=np.zeros((P, iters), f32_))
    for p, r in enumerate(results):
        for s, name in ((r["h"], "h"), (r["f"], "f")):
            o["status_" + name][p], o["score_" + name][p], o["num_inliers_" + name][p] = s["status"], s["score"], s["num_inliers"]
            o["best_iter_" + name][p], o["hyp_score_" + name][p] = s["best_iter"], s["hyp_score"]
        o["H_21"][p], o["F_21"][p] = r["h"]["M"], r["f"]["M"]
        o["num_matches"][p], o["rel_score_h"][p], o["choice"][p] = r["num_matches"], r["rel_score_h"], r["choice"]
        for k in ("inliers", "inliers_h", "inliers_f"):
            o[k][p, :r["count_1"]] = r[k][:r["count_1"]]
    for k, v in o.items():                                               # D27 item g: a NaN output is the canonical quiet NaN
        if v.dtype.kind == "f":
            v[np.isnan(v)] = np.nan
    return o


# ---------------------------------------------------------------------------------------------------------------- D27 items e and h
# homography_solver::decompose (:438-554), fundamental_solver::decompose (:334-340) and reconstruct_with_H / reconstruct_with_F
# (initialize/perspective.cc:123-174) over tests/two_view_ref.py's check_pose and find_most_plausible_pose
import math

import two_view_ref as TR
from pnp_solver_ref import hestenes, identity, norm2, ranks, sqrt_

NO_DECOMPOSITION = 5


def fdiv(a, b):
    return f32(div(a, b))


def fsqrt(v):
    return f32(sqrt_(v))


def det3(R):
    return R[0][0] * R[1][1] * R[2][2] + R[0][1] * R[1][2] * R[2][0] + R[0][2] * R[1][0] * R[2][1] - R[0][2] * R[1][1] * R[2][0] \
        - R[0][1] * R[1][0] * R[2][2] - R[0][0] * R[1][2] * R[2][1]


def cam_matrix(cam):
    return [[cam["fx"], 0.0, cam["cx"]], [0.0, cam["fy"], cam["cy"]], [0.0, 0.0, 1.0]]


def svd_pairs(A, linalg="jacobi"):
    """the singular pairs of a 3 x 3 matrix in the order of descending singular value: (U rows u_a, W rows v_a, sg), a u_a of a singular value that is 0
    or not finite left as zeros.  linalg="svd": numpy.linalg.svd in the place of the Jacobi"""
    if linalg == "svd":
        Un, sn, Vt = np.linalg.svd(np.array(A, np.float64))
        sg = [float(x) for x in sn]
        return [[float(Un[i][a]) if 0.0 < sg[a] < INF else 0.0 for i in range(3)] for a in range(3)], [[float(x) for x in Vt[a]] for a in range(3)], sg
    G = [[A[i][j] for i in range(3)] for j in range(3)]
    V = identity(3)
    hestenes(G, V)
    rk, keys = ranks([norm2(g) for g in G])
    U, W, sg = [None] * 3, [None] * 3, [0.0] * 3
    for a in range(3):
        j = rk.index(a)
        sg[a] = sqrt_(keys[j])
        have = 0.0 < sg[a] < INF
        U[a], W[a] = [div(G[j][i], sg[a]) if have else 0.0 for i in range(3)], list(V[j])
    return U, W, sg


def sign_pair(u, v):
    """D24 item c's rule: the component of largest magnitude of v is made non-negative (the first of equals), u follows"""
    big = 0
    for i in (1, 2):
        if abs(v[i]) > abs(v[big]):
            big = i
    return ([-x for x in u], [-x for x in v]) if v[big] < 0 else (u, v)


def cross3(a, b):
    return [a[(i + 1) % 3] * b[(i + 2) % 3] - a[(i + 2) % 3] * b[(i + 1) % 3] for i in range(3)]


def decompose_h(Hm, K, linalg="jacobi"):
    """Returns (rots: eight 3 x 3 row lists, transes: eight vectors) in the reference's order, or None where the rank test of :462 fails"""
    A = mul3(mul3(inv3(K, linalg), Hm), K)
    U, W, sg = svd_pairs(A, linalg)                       # rows: u_a, v_a in the order of descending singular value
    for a in range(3):
        if a == 2 and not (0.0 < sg[2] < INF):
            U[2] = cross3(U[0], U[1])
        U[a], W[a] = sign_pair(U[a], W[a])
    d1, d2, d3 = f32(sg[0]), f32(sg[1]), f32(sg[2])
    if fdiv(d1, d2) < 1.0001 or fdiv(d2, d3) < 1.0001:
        return None
    s = f32(det3(U) * det3(W))
    p12, p23, p13 = f32(fmul(d1, d1) - fmul(d2, d2)), f32(fmul(d2, d2) - fmul(d3, d3)), f32(fmul(d1, d1) - fmul(d3, d3))
    aux_1, aux_3 = fsqrt(fdiv(p12, p13)), fsqrt(fdiv(p23, p13))
    root = fsqrt(fmul(p12, p23))
    sum13, dif13 = f32(d1 + d3), f32(d1 - d3)
    sin_theta, cos_theta = fdiv(root, fmul(sum13, d2)), fdiv(f32(fmul(d2, d2) + fmul(d1, d3)), fmul(sum13, d2))
    sin_phi, cos_phi = fdiv(root, fmul(dif13, d2)), fdiv(f32(fmul(d1, d3) - fmul(d2, d2)), fmul(dif13, d2))
    Um = [[U[a][i] for a in range(3)] for i in range(3)]   # the matrix U: columns u_a
    SU = [[s * Um[i][a] for a in range(3)] for i in range(3)]
    rots, transes = [], []
    for h in range(8):
        i = h & 3
        x1, x3 = (aux_1 if i < 2 else -aux_1), (-aux_3 if i & 1 else aux_3)
        plus = i in (0, 3)
        if h < 4:
            sn = sin_theta if plus else -sin_theta
            aux = [[cos_theta, 0.0, -sn], [0.0, 1.0, 0.0], [sn, 0.0, cos_theta]]
            at = [x1 * dif13, 0.0 * dif13, (-x3) * dif13]
        else:
            sn = sin_phi if plus else -sin_phi
            aux = [[cos_phi, 0.0, sn], [0.0, -1.0, 0.0], [sn, 0.0, -cos_phi]]
            at = [x1 * sum13, 0.0 * sum13, x3 * sum13]
        rots.append(mul3(mul3(SU, aux), W))
        t = [(Um[r][0] * at[0] + Um[r][1] * at[1]) + Um[r][2] * at[2] for r in range(3)]
        nrm = sqrt_((t[0] * t[0] + t[1] * t[1]) + t[2] * t[2])
        transes.append([div(x, nrm) for x in t])
    return rots, transes


def decompose_f(Fm, K, linalg="jacobi"):
    """fundamental_solver::decompose: E_21 = (K^T * F_21) * K, then D24 item c (tests/two_view_ref.py's decompose); linalg="svd": the same rule over
    numpy's singular pairs"""
    E = mul3(mul3(transpose3(K), Fm), K)
    if linalg != "svd":
        return TR.decompose(E)
    U, W, _ = svd_pairs(E, linalg)
    for a in (0, 1):
        U[a], W[a] = sign_pair(U[a], W[a])
    U[2], W[2] = cross3(U[0], U[1]), cross3(W[0], W[1])
    nrm = sqrt_((U[2][0] * U[2][0] + U[2][1] * U[2][1]) + U[2][2] * U[2][2])
    trans = [div(x, nrm) for x in U[2]]
    rot_1 = [[(U[1][i] * W[0][k] + (-U[0][i]) * W[1][k]) + U[2][i] * W[2][k] for k in range(3)] for i in range(3)]
    rot_2 = [[((-U[1][i]) * W[0][k] + U[0][i] * W[1][k]) + U[2][i] * W[2][k] for k in range(3)] for i in range(3)]
    out = [[[x * -1.0 for x in r] for r in R] if det3(R) < 0 else R for R in (rot_1, rot_2)]
    neg = [-x for x in trans]
    return [out[0], out[0], out[1], out[1]], [trans, neg, list(trans), list(neg)]


def perspective_pose(cam, bounds, choice, Hm, Fm, inliers, match, bearing_1, bearing_2, kps_1, kps_2, min_num_triangulated=50, parallax_deg_thr=1.0,
                     reproj_err_thr=4.0, count_2=None, linalg="jacobi"):
    """reconstruct_with_H / reconstruct_with_F of one problem.  Returns two_view_ref.two_view_pose's dict over eight hypotheses, and rots / transes:
    the hypotheses themselves"""
    n_cap = len(match)
    res = dict(status=TR.TV_NO_SOLUTION, rot=[[0.0] * 3 for _ in range(3)], trans=[0.0] * 3, hypothesis=-1, num_valid=[0] * 8, parallax_deg=[0.0] * 8,
               pts=[[0.0] * 3 for _ in range(n_cap)], is_triangulated=[0] * n_cap, hyp_is_triangulated=[[0] * n_cap for _ in range(8)])
    if choice not in (CHOICE_H, CHOICE_F):
        return res
    K = cam_matrix(cam)
    dec = decompose_h([list(map(float, r)) for r in Hm], K, linalg) if choice == CHOICE_H else decompose_f([list(map(float, r)) for r in Fm], K, linalg)
    if dec is None:
        res["status"] = NO_DECOMPOSITION
        return res
    rots, transes = dec
    res.update(rots=rots, transes=transes)
    checks = [TR.check_pose(cam, bounds, rots[h], transes[h], inliers, match, bearing_1, bearing_2, kps_1, kps_2, reproj_err_thr, True, count_2) for h in range(len(rots))]
    status, chosen = TR.find_most_plausible_pose(checks, min_num_triangulated, parallax_deg_thr)
    pad = 8 - len(checks)
    res.update(status=status, hypothesis=chosen, num_valid=[r["num_valid"] for r in checks] + [0] * pad, parallax_deg=[r["parallax_deg"] for r in checks] + [0.0] * pad,
               hyp_is_triangulated=[r["is_triangulated"] for r in checks] + [[0] * n_cap] * pad)
    if chosen >= 0:
        res.update(rot=rots[chosen], trans=transes[chosen], pts=checks[chosen]["pts"], is_triangulated=checks[chosen]["is_triangulated"])
    return res


def pose_expected(results, n_cap, counts_1=None):
    """the outputs of plp_perspective_pose_* over arrays filled with two_view_ref.TV_SENTINEL"""
    P = len(results)
    o = dict(status=np.zeros(P, np.uint8), rot_ref_to_cur=np.zeros((P, 3, 3)), trans_ref_to_cur=np.zeros((P, 3)), hypothesis=np.zeros(P, np.int32),
             num_valid=np.zeros((P, 8), np.int32), parallax_deg=np.zeros((P, 8), np.float32), triangulated_pts=np.full((P, n_cap, 3), TR.TV_SENTINEL["triangulated_pts"]),
             is_triangulated=np.full((P, n_cap), 0xEE, np.uint8), hyp_is_triangulated=np.full((P, 8, n_cap), 0xEE, np.uint8))
    for p, r in enumerate(results):
        n = len(r["is_triangulated"]) if counts_1 is None else int(counts_1[p])
        o["status"][p], o["rot_ref_to_cur"][p], o["trans_ref_to_cur"][p], o["hypothesis"][p] = r["status"], r["rot"], r["trans"], r["hypothesis"]
        o["num_valid"][p], o["parallax_deg"][p] = r["num_valid"], r["parallax_deg"]
        o["triangulated_pts"][p, :n], o["is_triangulated"][p, :n] = np.array(r["pts"])[:n], r["is_triangulated"][:n]
        o["hyp_is_triangulated"][p, :, :n] = np.array(r["hyp_is_triangulated"])[:, :n]
    return o
